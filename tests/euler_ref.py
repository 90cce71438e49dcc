"""Float64 restatement of the Euler and Euler-ancestral schedulers (diffusers' EulerDiscreteScheduler and
EulerAncestralDiscreteScheduler with final_sigmas_type="zero"), shared by tests/test_host_euler.py and tests/test_gpu_euler.py.
Written from the published formulas, independent of sketch2img_amd.sampler: the checker of both files.

  sigma table     sigma_t = sqrt((1 - abar_t)/abar_t) over the fp32 alphas_cumprod table, t = 0..999
  timesteps       "leading": (N-1 .. 0) * (1000 // N) + steps_offset;  "trailing": round(1000 - k * 1000/N) - 1;
                  "linspace": 999 - k * 999/(N-1) (fractional)
  sigmas          the table interpolated linearly at those timesteps, then a final 0; the UNet runs at round(timestep)
  Karras          rho = 7 spacing between the first and last interpolated sigma; the timestep of each is the rounded piecewise-linear
                  interpolation of t in log sigma
  model input     x / sqrt(sigma^2 + 1);  start latent  init_noise_sigma * draw, max sigma (sqrt(max sigma^2 + 1) for "leading")
  step            x0 = x - sigma m  (v prediction: x/(sigma^2 + 1) - sigma m/sqrt(sigma^2 + 1));  d = (x - x0)/sigma;
                  x_prev = x + (sigma_to - sigma) d + sigma_up z;  Euler: sigma_to = sigma_next, sigma_up = 0;  ancestral:
                  sigma_up = sqrt(sigma_next^2 (sigma^2 - sigma_next^2)/sigma^2), sigma_to = sqrt(sigma_next^2 - sigma_up^2)"""
import math

import numpy as np

from tests.dpm_ref import U32, sd_alphas_cumprod      # noqa: F401  (U32 is re-exported to both test files)


def sigma_table():
    acp = sd_alphas_cumprod().double().numpy()
    return np.sqrt((1.0 - acp) / acp)


def timesteps_ref(N, spacing, steps_offset=0):
    """-> [N] float64, descending; fractional under "linspace"."""
    if spacing == "leading":
        return np.array([float(k * (1000 // N) + steps_offset) for k in range(N - 1, -1, -1)])
    if spacing == "trailing":
        return np.array([float(np.round(1000.0 - k * (1000.0 / N))) - 1.0 for k in range(N)])
    if spacing == "linspace":
        return np.array([999.0 - k * (999.0 / (N - 1)) if N > 1 else 0.0 for k in range(N)])
    raise ValueError(spacing)


def schedule_ref(N, spacing, steps_offset=0, karras=False, rho=7.0):
    """-> (sigmas [N + 1] float64 with the final 0, UNet timesteps [N] int64, init_noise_sigma)."""
    table = sigma_table()
    ts = timesteps_ref(N, spacing, steps_offset)
    sig = np.empty(N)
    for k, t in enumerate(ts):
        lo = min(int(math.floor(t)), 998)
        w = t - lo
        sig[k] = (1.0 - w) * table[lo] + w * table[lo + 1]
    its = np.round(ts).astype(np.int64)
    if karras:
        smax, smin = sig[0], sig[-1]
        sig = np.array([(smax ** (1 / rho) + (i / (N - 1) if N > 1 else 0.0) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
                        for i in range(N)])
        its = np.round(np.interp(np.log(sig), np.log(table), np.arange(1000.0))).astype(np.int64)
    top = float(sig.max())
    return np.concatenate([sig, [0.0]]), its, math.sqrt(top * top + 1.0) if spacing == "leading" else top


def ancestral_ref(s, sn):
    """(sigma_up, sigma_down) of the step sigma -> sigma_next."""
    up = math.sqrt(sn * sn * (s * s - sn * sn) / (s * s))
    return up, math.sqrt(max(sn * sn - up * up, 0.0))


def step_scalars_ref(sigmas, i, ancestral):
    """(sigma, sigma_to, sigma_up) of step i in float64."""
    s, sn = float(sigmas[i]), float(sigmas[i + 1])
    if not ancestral:
        return s, sn, 0.0
    up, down = ancestral_ref(s, sn)
    return s, down, up


def euler_step_ref(x, u, c, z, g, s, s_to, s_up, vpred):
    """One update in float64 on float64 operands (torch or numpy): -> (x_prev, d).  z may be None when s_up == 0."""
    m = u + g * (c - u)
    if vpred:
        x0 = x / (s * s + 1.0) - s / math.sqrt(s * s + 1.0) * m
    else:
        x0 = x - s * m
    d = (x - x0) / s
    xp = x + (s_to - s) * d
    if s_up != 0.0:
        xp = xp + s_up * z
    return xp, d
