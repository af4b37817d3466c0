"""NumPy fp32 restatement of dynamic thresholding as include/dsg.h pins it (``dsg_dynthresh_scale``, ``dsg_ddpm_step_thr``,
``dsg_ddim_step_thr``): sort-based, every operation rounded to fp32 on its own, the two ``fmaf`` of the interpolation emulated
by an exact fp64 product and ONE rounding of the sum to fp32.  Test infrastructure: the specification the tests import;
nothing in the package touches it.

diffusers 0.20.0 ``_threshold_sample`` (Saharia et al., "Imagen", 2022, section 2.3), per sample:
    s = clamp(torch.quantile(|x0|, q), 1, sample_max_value);   x0 <- clamp(x0, -s, s) / s
"""
import numpy as np

F = np.float32


def fmaf(a, b, c):
    """fp32 fma(a, b, c) of three fp32 scalars: the product of two fp32 values is exact in fp64; the fp64 sum is rounded once,
    and where that sum sits exactly half way between two fp32 neighbours while the true sum does not, it is nudged to the true
    sum's side first (the one case in which rounding fp64 -> fp32 a second time would differ from a single rounding)."""
    a, b, c = np.float64(F(a)), np.float64(F(b)), np.float64(F(c))
    p = a * b
    s = p + c
    if not np.isfinite(s):
        return F(s)
    bb = s - p                                       # TwoSum: err is exactly (p + c) - s
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and (np.float64(s).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000):
        s = np.nextafter(s, np.float64(np.inf) if err > 0 else np.float64(-np.inf))
    return F(s)


def ranks(per, q):
    """(k_lo, k_hi, w): torch.quantile's rank of the q-quantile of `per` values, an fp32 product."""
    rank = F(q) * F(per - 1)
    k_lo = min(int(np.floor(rank)), per - 1)
    k_hi = min(int(np.ceil(rank)), per - 1)
    w = F(rank - F(k_lo)) if k_hi > k_lo else F(0)
    return k_lo, k_hi, w


def scale_of_abs(a_rows, q, max_value):
    """s [N] from the rows of magnitudes a_rows [N, per] (fp32)."""
    a_rows = np.ascontiguousarray(a_rows, dtype=F)
    n, per = a_rows.shape
    k_lo, k_hi, w = ranks(per, q)
    out = np.empty(n, dtype=F)
    for r in range(n):
        row = a_rows[r]
        if np.isnan(row).any():
            out[r] = np.nan
            continue
        part = np.partition(row, (k_lo, k_hi))
        v_lo, v_hi = part[k_lo], part[k_hi]
        with np.errstate(invalid="ignore"):
            d = F(v_hi - v_lo)
            quant = fmaf(w, d, v_lo) if w < F(0.5) else fmaf(-d, F(F(1) - w), v_hi)
        out[r] = np.nan if np.isnan(quant) else min(max(quant, F(1)), F(max_value))
    return out


def pred_x0(x, e, sb, sa):
    """p0 = (x - sb*e) / sa, unclipped."""
    with np.errstate(all="ignore"):
        return ((x.astype(F) - F(sb) * e.astype(F)) / F(sa)).astype(F)


def scale(x, e, sb, sa, q, max_value):
    """s [N] of the samples x, e [N, ...]."""
    p0 = pred_x0(x, e, sb, sa)
    return scale_of_abs(np.abs(p0).reshape(p0.shape[0], -1), q, max_value)


def thresholded_x0(x, e, sb, sa, s):
    p0 = pred_x0(x, e, sb, sa)
    sv = s.astype(F).reshape((-1,) + (1,) * (p0.ndim - 1))
    with np.errstate(all="ignore"):
        return (np.minimum(np.maximum(p0, -sv), sv) / sv).astype(F)


def ddpm_step(x, e, z, sc, q, max_value):
    """(prev, s): sc = DDPMScheduler.step_scalars(t); z None at t == 0."""
    s = scale(x, e, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], q, max_value)
    p0 = thresholded_x0(x, e, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], s)
    with np.errstate(all="ignore"):
        prev = F(sc["coef_x0"]) * p0 + F(sc["coef_xt"]) * x.astype(F)
        if z is not None:
            prev = prev + F(sc["sigma"]) * z.astype(F)
    return prev.astype(F), s


def ddim_step(x, e, sc, q, max_value):
    """(prev, s): sc = DDIMScheduler.step_scalars(t)."""
    s = scale(x, e, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], q, max_value)
    p0 = thresholded_x0(x, e, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], s)
    with np.errstate(all="ignore"):
        prev = F(sc["sqrt_alpha_prev"]) * p0 + F(sc["dir_coef"]) * e.astype(F)
    return prev.astype(F), s
