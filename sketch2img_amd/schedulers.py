"""Configuration holders with the constructor signatures the reference uses for its schedulers
(app.py:13-25, evaluation.py:21-32, modules/clip_guided_inf.py:15-26).  diffusers is not a dependency of this
package: these classes carry the configuration only; the arithmetic lives in sketch2img_amd.sampler
(host-side tables) and libskg.so (the latent update kernels).  A real diffusers scheduler object passed as
`scheduler=` works too - the pipeline reads its `.config`.
"""
from __future__ import annotations

from types import SimpleNamespace


class _ConfigScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **kwargs):
        self.config = SimpleNamespace(**kwargs)

    def scale_model_input(self, sample, timestep=None):       # identity for DDIM and DPM-Solver++ (modules/pipeline.py:86)
        return sample


class DDIMScheduler(_ConfigScheduler):
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kwargs):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError("scaled_linear betas (Stable Diffusion) only")
        if clip_sample:
            raise NotImplementedError("clip_sample=False (Stable Diffusion) only")
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                         steps_offset=steps_offset, **kwargs)


class DPMSolverMultistepScheduler(_ConfigScheduler):
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 trained_betas=None, solver_order=2, predict_epsilon=True, thresholding=False,
                 algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, use_karras_sigmas=False,
                 **kwargs):
        if beta_schedule != "scaled_linear" or trained_betas is not None:
            raise NotImplementedError("scaled_linear betas (Stable Diffusion) only")
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, solver_order=solver_order,
                         predict_epsilon=predict_epsilon, thresholding=thresholding, algorithm_type=algorithm_type,
                         solver_type=solver_type, lower_order_final=lower_order_final, use_karras_sigmas=use_karras_sigmas,
                         **kwargs)


def euler_unsupported(get) -> list:
    """The options of an Euler / Euler-ancestral scheduler config that change the arithmetic and are not implemented, as
    'name=value' strings (`get(key, default)` reads the config: these classes' or a real diffusers scheduler's).  The pipeline
    rejects them, never ignores them."""
    bad = []
    for k, ok in (("beta_schedule", "scaled_linear"), ("trained_betas", None), ("interpolation_type", "linear"), ("sigma_min", None),
                  ("sigma_max", None), ("timestep_type", "discrete"), ("rescale_betas_zero_snr", False),
                  ("use_exponential_sigmas", False), ("use_beta_sigmas", False), ("final_sigmas_type", "zero")):
        v = get(k, ok)
        if v is not ok and v != ok:
            bad.append(f"{k}={v!r}")
    if get("timestep_spacing", "linspace") not in ("leading", "trailing", "linspace"):
        bad.append(f"timestep_spacing={get('timestep_spacing', None)!r}")
    if get("prediction_type", "epsilon") not in ("epsilon", "v_prediction"):
        bad.append(f"prediction_type={get('prediction_type', None)!r}")
    return bad


class _EulerConfig(_ConfigScheduler):
    """init_noise_sigma and scale_model_input depend on the number of steps and on the step: sampler.EulerTables has both."""
    init_noise_sigma = None

    def scale_model_input(self, sample, timestep=None):
        raise NotImplementedError("a configuration holder: sampler.EulerTables.c_in(i) is the model-input scale of step i")

    def __init__(self, **kwargs):
        bad = euler_unsupported(lambda k, d: kwargs.get(k, d))
        if bad:
            raise NotImplementedError(f"{type(self).__name__}: {', '.join(bad)} is not implemented")
        super().__init__(**kwargs)


class EulerDiscreteScheduler(_EulerConfig):
    """"Euler".  diffusers' constructor keywords and its "linspace" / steps_offset 0 defaults (SD's model repos ship "leading" and
    1); the betas default to Stable Diffusion's, as in the classes above."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 trained_betas=None, prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False,
                 use_exponential_sigmas=False, use_beta_sigmas=False, sigma_min=None, sigma_max=None, timestep_spacing="linspace",
                 timestep_type="discrete", steps_offset=0, rescale_betas_zero_snr=False, final_sigmas_type="zero", **kwargs):
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                         trained_betas=trained_betas, prediction_type=prediction_type, interpolation_type=interpolation_type,
                         use_karras_sigmas=use_karras_sigmas, use_exponential_sigmas=use_exponential_sigmas,
                         use_beta_sigmas=use_beta_sigmas, sigma_min=sigma_min, sigma_max=sigma_max, timestep_spacing=timestep_spacing,
                         timestep_type=timestep_type, steps_offset=steps_offset, rescale_betas_zero_snr=rescale_betas_zero_snr,
                         final_sigmas_type=final_sigmas_type, **kwargs)


class EulerAncestralDiscreteScheduler(_EulerConfig):
    """"Euler a".  diffusers' constructor keywords; use_karras_sigmas, which diffusers' class does not have, is accepted as well
    (k-diffusion's "Euler a Karras")."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                 rescale_betas_zero_snr=False, use_karras_sigmas=False, **kwargs):
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                         trained_betas=trained_betas, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                         steps_offset=steps_offset, rescale_betas_zero_snr=rescale_betas_zero_snr,
                         use_karras_sigmas=use_karras_sigmas, **kwargs)
