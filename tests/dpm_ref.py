"""Float64 restatement of DPM-Solver++ 2M with Karras sigmas and of its stochastic variant (diffusers' sigma-based formulation with
final_sigmas_type="zero"), shared by tests/test_host_dpm_karras_sde.py and tests/test_gpu_dpm_karras_sde.py.  Written from the
published formulas, independent of sketch2img_amd.sampler: the checker of both files."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24                      # unit roundoff of fp32: one cast to fp32 is off by at most U32 relative


def sd_alphas_cumprod():
    """The fp32 table every scheduler of this project starts from (scaled_linear betas 0.00085 .. 0.012, 1000 steps)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def karras_ref(N, rho=7.0):
    """-> (sigmas [N] float64, timesteps [N] int64): sigma_i = (smax^(1/rho) + i/(N-1) (smin^(1/rho) - smax^(1/rho)))^rho, t_i the
    rounded piecewise-linear interpolation of t in log sigma over the table, clipped to [0, 999]."""
    acp = sd_alphas_cumprod().double().numpy()
    table = np.sqrt((1.0 - acp) / acp)
    smin, smax = table[0], table[-1]
    sig = np.array([(smax ** (1 / rho) + (i / (N - 1) if N > 1 else 0.0) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
                    for i in range(N)])
    tau = np.interp(np.log(sig), np.log(table), np.arange(1000.0))            # (np.interp clips to the end values)
    return sig, np.round(tau).astype(np.int64)


def source_ref(tab, karras, N):
    """[(alpha, sigma_hat, lambda)] for entries 0..N in float64: from the restated sigmas, or alpha and sigma_hat from the fp32
    tables at the uniform integer timesteps (final target t = 0) with lambda = log(alpha / sigma_hat) of those two values - the
    identities below hold exactly only for a lambda that agrees with alpha and sigma_hat, which the table's own fp32 lambda_t
    does to fp32 rounding only."""
    if karras:
        sig, _ = karras_ref(N)
        out = [(1.0 / math.sqrt(1.0 + s * s), s / math.sqrt(1.0 + s * s), -math.log(s)) for s in sig]
        return out + [(1.0, 0.0, math.inf)]
    ts = np.linspace(0, 999, N + 1).round()[::-1][:-1].astype(np.int64).tolist() + [0]
    return [(float(tab.alpha_t[t]), float(tab.sigma_t[t]), math.log(float(tab.alpha_t[t]) / float(tab.sigma_t[t]))) for t in ts]


def sde_ref(src, i, order):
    """(a, b, c, d) of the issue's formulas in float64."""
    (al_s, sg_s, lam_s), (al_t, sg_t, lam_t) = src[i], src[i + 1]
    h = lam_t - lam_s
    q = 1.0 - math.exp(-2.0 * h)
    a, b, d = (sg_t / sg_s) * math.exp(-h), al_t * q, sg_t * math.sqrt(q)
    if order == 1:
        return a, b, 0.0, d
    r0 = (lam_s - src[i - 1][2]) / h
    return a, b * (1.0 + 0.5 / r0), -0.5 * b / r0, d


def ode_ref(src, i, order):
    (al_s, sg_s, lam_s), (al_t, sg_t, lam_t) = src[i], src[i + 1]
    h = lam_t - lam_s
    k0 = al_t * (math.exp(-h) - 1.0)
    if order == 1:
        return sg_t / sg_s, -k0, 0.0
    r0 = (lam_s - src[i - 1][2]) / h
    return sg_t / sg_s, -(k0 + 0.5 * k0 / r0), 0.5 * k0 / r0


def orders(tab):
    seen, out = 0, []
    for i in range(len(tab.timesteps)):
        out.append(tab.order(i, seen))
        seen = min(seen + 1, tab.solver_order)
    return out
