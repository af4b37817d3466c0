"""Plain torch-CPU fp32 restatement of the prediction-type feature (include/dsg.h: ``dsg_ddpm_step_pt``, ``dsg_ddim_step_pt``,
``dsg_add_noise_target``, ``dsg_mse_loss_weighted``) and of the host tables that go with it, written from the formulas of
diffusers 0.20.0, op for op.  Every scalar enters as a 0-d fp32 tensor, so each line is one individually rounded fp32 operation
(tensor / tensor is an IEEE division; torch never fuses a multiply into an add across two calls).
"""
import math

import numpy as np
import torch

F32 = torch.float32


def _s(v):
    return torch.tensor(float(v), dtype=F32)


# ---- host tables ------------------------------------------------------------------------------------------------------------
def betas(schedule, n=1000, beta_start=0.0001, beta_end=0.02):
    if schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=F32)
    if schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=F32) ** 2
    assert schedule == "squaredcos_cap_v2"

    def ab(t):
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    return torch.tensor([min(1 - ab((i + 1) / n) / ab(i / n), 0.999) for i in range(n)], dtype=F32)


def rescale_zero_terminal_snr(b):
    s = torch.cumprod(1.0 - b, dim=0).sqrt()
    a0, aT = s[0].clone(), s[-1].clone()
    s -= aT
    s *= a0 / (a0 - aT)
    ab = s ** 2
    alphas = torch.cat([ab[0:1], ab[1:] / ab[:-1]])
    return 1 - alphas


def alphas_cumprod(b):
    return torch.cumprod(1.0 - b, dim=0)


def timesteps(spacing, n_train, steps, steps_offset=0):
    if spacing == "leading":
        return ((np.arange(0, steps) * (n_train // steps)).round()[::-1].copy().astype(np.int64) + steps_offset).tolist()
    if spacing == "linspace":
        return np.linspace(0, n_train - 1, steps).round()[::-1].copy().astype(np.int64).tolist()
    assert spacing == "trailing"
    return (np.round(np.arange(n_train, 0, -n_train / steps)) - 1).astype(np.int64).tolist()


def snr_weights(ac, gamma, prediction):
    snr = (torch.sqrt(ac) / torch.sqrt(1 - ac)) ** 2
    w = torch.minimum(snr, _s(gamma))
    if prediction == "epsilon":
        return w / snr
    if prediction == "v_prediction":
        return w / (snr + 1)
    assert prediction == "sample"
    return w


# ---- per-element formulas ---------------------------------------------------------------------------------------------------
def predictions(x, m, sb, sa, clip, prediction):
    """(p0, pe): the data prediction, clamped to +-clip when clip > 0, and the noise prediction from the UNCLAMPED values."""
    sb, sa = _s(sb), _s(sa)
    if prediction == "epsilon":
        p0 = (x - sb * m) / sa
        pe = m
    elif prediction == "sample":
        p0 = m
        pe = (x - sa * m) / sb
    else:
        assert prediction == "v_prediction"
        p0 = sa * x - sb * m
        pe = sa * m + sb * x
    if clip > 0:
        p0 = torch.clamp(p0, -float(clip), float(clip))
    return p0, pe


def ddpm_step(x, m, z, sc, prediction, clip):
    """`sc`: the scheduler's ``step_scalars(t)``; `z` None where the step has no noise term (t == 0)."""
    p0, _ = predictions(x, m, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], clip, prediction)
    prev = _s(sc["coef_x0"]) * p0 + _s(sc["coef_xt"]) * x
    if z is not None:
        prev = prev + _s(sc["sigma"]) * z
    return prev


def ddim_step(x, m, sc, prediction, clip):
    p0, pe = predictions(x, m, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], clip, prediction)
    return _s(sc["sqrt_alpha_prev"]) * p0 + _s(sc["dir_coef"]) * pe


def _per_sample(v, like):
    return v.to(F32).reshape(-1, *([1] * (like.dim() - 1)))


def add_noise(x0, z, sa, sb):
    """sa, sb: fp32 [N], one per leading-dim sample"""
    return _per_sample(sa, x0) * x0 + _per_sample(sb, x0) * z


def velocity(x0, z, sa, sb):
    return _per_sample(sa, x0) * z - _per_sample(sb, x0) * x0


def sqrt_tables(ac):
    return ac ** 0.5, (1 - ac) ** 0.5


# ---- the weighted loss ------------------------------------------------------------------------------------------------------
def weighted_mse_fp64(pred, target, w):
    d = (pred - target).double()        # (the fp32 difference, as the kernel forms it; everything after in fp64)
    return float((_per_sample(w, pred).double() * d * d).sum() / pred.numel())


def weighted_mse_grad(pred, target, w, grad_scale=1.0):
    coef = torch.tensor(2.0 * grad_scale, dtype=F32) / torch.tensor(float(pred.numel()), dtype=F32)
    return (coef * _per_sample(w, pred)) * (pred - target)
