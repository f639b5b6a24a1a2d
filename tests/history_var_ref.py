"""Float64 numpy restatement of the variance the history carries and of the history denoiser's start values (include/spcbpt.h:
spcbpt_history_denoise), written from the formulas in the header on top of tests/reproject_ref.py and tests/denoise_var_ref.py.
Shared by tests/test_history_variance_host.py and tests/test_gpu_history_denoise.py."""
import numpy as np

from tests import reproject_ref as rr
from tests.denoise_var_ref import atrous_var_ref


def film_variance_ref(accum, m2n):
    """VA, (..., 3) float64: max(M2, 0) / (n (n - 1)) where n >= 2, accum^2 elsewhere (m2n None: n = 0 everywhere)."""
    a = np.asarray(accum, np.float64)[..., :3]
    if m2n is None:
        return a * a
    m = np.asarray(m2n, np.float64)
    n = m[..., 3]
    ok = n >= 2
    nn = np.where(ok, n * (n - 1), 1.0)
    return np.where(ok[..., None], np.maximum(m[..., :3], 0.0) / nn[..., None], a * a)


def prior_variance_ref(cam, normal_depth, cam_h, G, H, HV, sigma_n, sigma_x, max_history):
    """(R, PV): the float64 prior (h, w, 4) and PV (h, w, 3) -- the reprojection with the payload (HV.rgb, H.n): the same taps, weights
    and cut, so PV is that run's rgb (zero wherever R is)."""
    payload = np.concatenate([np.asarray(HV, np.float64)[..., :3], np.asarray(H, np.float64)[..., 3:4]], -1)
    R = rr.reproject_ref(cam, normal_depth, cam_h, G, H, sigma_n, sigma_x, max_history)
    PV = rr.reproject_ref(cam, normal_depth, cam_h, G, payload, sigma_n, sigma_x, max_history)
    assert np.array_equal(R[..., 3], PV[..., 3])
    return R, PV[..., :3]


def resolve_variance_ref(prior, prior_var, accum, m2n, frames):
    """RV, (..., 3) float64: (m^2 PV + Nf^2 VA) / (m + Nf)^2, m = prior.w; VA itself without a prior."""
    va = film_variance_ref(accum, m2n)
    if prior is None:
        return va
    m = np.asarray(prior, np.float64)[..., 3:4]
    pv = np.asarray(prior_var, np.float64)[..., :3]
    nf = float(frames)
    return (m * m * pv + nf * nf * va) / (m + nf) ** 2


def history_denoise_ref(resolved, resolved_var, albedo, normal_depth, U, V, W, iterations, sigma_v, sigma_n, sigma_x):
    """denoised rgb, (h, w, 3) float64: atrous_var_ref's iterations from c_0 = resolved / max(albedo, 1e-3) and
    v_0 = (sum_k w_k sqrt(RV_k) / max(albedo_k, 1e-3))^2.  atrous_var_ref takes its start variance from a moments plane as
    sd_k = sqrt(M2_k / (n (n - 1))); the plane (2 RV, n = 2) has sd_k = sqrt(RV_k), so it is handed that (in float64)."""
    rv = np.asarray(resolved_var, np.float64)
    stand_in = np.concatenate([2.0 * rv[..., :3], np.full(rv.shape[:-1] + (1,), 2.0)], -1)
    return atrous_var_ref(np.asarray(resolved), stand_in, np.asarray(albedo), np.asarray(normal_depth), U, V, W, iterations, sigma_v, sigma_n, sigma_x)
