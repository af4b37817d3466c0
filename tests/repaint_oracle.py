"""NumPy fp32 restatement of RePaint (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers 0.20.0 ``RePaintScheduler`` /
``RePaintPipeline``) -- TEST INFRASTRUCTURE for tests/test_repaint_cpu.py and tests/test_gpu_repaint.py.

Parity is unpinned by the reference (its tree holds no RePaint code, diffusers is not installed): the formulas of
include/dsg.h (``dsg_repaint_step`` / ``dsg_repaint_undo``) and the paper are the specification.  Every operation below acts
on ``np.float32`` values and is rounded once, in the order the header states; nothing here imports the package under test.
"""
import numpy as np

F = np.float32


# ---- tables (diffusers: torch.linspace(beta_start, beta_end, n, dtype=float32), 1 - betas, cumprod) -------------------------
def linspace_f32(start, end, steps):
    """torch.linspace's fp32 CPU kernel: step = (end - start) / (steps - 1) rounded to fp32; the first half counts up from
    `start`, the second half down from `end`, each element ONE fused multiply-add (evaluated here in float64, where the product
    of an fp32 step and an index below 2^24 is exact, then rounded to fp32)."""
    start, end = F(start), F(end)
    step = float(F((end - start) / F(steps - 1)))
    i = np.arange(steps)
    up = (float(start) + step * i).astype(F)
    down = (float(end) - step * (steps - 1 - i)).astype(F)
    return np.where(i < steps // 2, up, down).astype(F)


def tables(num_train=1000, beta_start=1e-4, beta_end=0.02):
    betas = linspace_f32(beta_start, beta_end, num_train)
    alphas = (F(1.0) - betas).astype(F)
    # torch.cumprod on the CPU keeps its running product in the accumulation type of fp32, float64, and rounds each output
    acp = np.cumprod(alphas.astype(np.float64)).astype(F)
    return betas, acp


# ---- timestep table -----------------------------------------------------------------------------------------------------
def timesteps(num_inference_steps, jump_length=10, jump_n_sample=10, num_train=1000):
    n = min(num_train, num_inference_steps)
    jumps = {j: jump_n_sample - 1 for j in range(0, n - jump_length, jump_length)}
    out, t = [], n
    while t >= 1:
        t -= 1
        out.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            for _ in range(jump_length):
                t += 1
                out.append(t)
    return np.array(out, dtype=np.int64) * (num_train // n)


def plan(ts):
    """True where the loop runs the network + step, False where it jumps back (diffusers' ``t < t_last``)."""
    out, t_last = [], int(ts[0]) + 1
    for t in ts:
        out.append(int(t) < t_last)
        t_last = int(t)
    return out


def _sqrt(v):
    """diffusers writes every square root of a host scalar as ``x ** 0.5`` on a 0-d fp32 torch tensor, and torch's CPU kernel
    for it is NOT the correctly rounded square root (it differs from np.sqrt by one ulp on 7 of the 1000 default betas).  The
    protocol is diffusers', so this one function is taken from torch; every other operation here is NumPy fp32."""
    import torch
    return F(float(torch.tensor(float(v), dtype=torch.float32) ** 0.5))


# ---- scalars ------------------------------------------------------------------------------------------------------------
def step_scalars(t, n, eta, num_train=1000, tabs=None):
    _, acp = tabs if tabs is not None else tables(num_train)
    prev_t = t - num_train // n
    a_t = acp[t]
    a_prev = acp[prev_t] if prev_t >= 0 else F(1.0)
    b_t = F(F(1.0) - a_t)
    b_prev = F(F(1.0) - a_prev)
    variance = F(F(b_prev / b_t) * F(F(1.0) - F(a_t / a_prev)))
    std = F(F(eta) * _sqrt(variance))
    dc = _sqrt(F(F(F(1.0) - a_prev) - F(std * std)))
    return dict(sb=_sqrt(b_t), sa=_sqrt(a_t), sap=_sqrt(a_prev), dc=F(dc), std=F(std),
                sbp=_sqrt(F(F(1.0) - a_prev)))


def undo_scalars(t, n, num_train=1000, tabs=None):
    betas, _ = tabs if tabs is not None else tables(num_train)
    return [(_sqrt(F(F(1.0) - betas[t + i])), _sqrt(betas[t + i])) for i in range(num_train // n)]


def undo_scalars_fused(t, n, num_train=1000, tabs=None):
    betas, _ = tabs if tabs is not None else tables(num_train)
    keep = np.prod([1.0 - float(betas[t + i]) for i in range(num_train // n)], dtype=np.float64)
    return F(np.sqrt(keep)), F(np.sqrt(1.0 - keep))


# ---- tensor math ----------------------------------------------------------------------------------------------------------
def step(x, e, orig, m, z, s, clip=1.0, add_std=False):
    """The order of include/dsg.h; `orig` / `m` broadcast by numpy over [N, C, H, W]."""
    x, e, orig, m, z = (np.asarray(a, dtype=F) for a in (x, e, orig, m, z))
    p0 = ((x - (s["sb"] * e).astype(F)).astype(F) / s["sa"]).astype(F)
    if clip > 0:
        p0 = np.minimum(np.maximum(p0, F(-clip)), F(clip)).astype(F)
    unknown = ((s["sap"] * p0).astype(F) + (s["dc"] * e).astype(F)).astype(F)
    if add_std:
        unknown = (unknown + (s["std"] * z).astype(F)).astype(F)
    known = ((s["sap"] * orig).astype(F) + (s["sbp"] * z).astype(F)).astype(F)
    return ((m * known).astype(F) + ((F(1.0) - m).astype(F) * unknown).astype(F)).astype(F)


def undo(x, z, ck, cz):
    x, z = np.asarray(x, dtype=F), np.asarray(z, dtype=F)
    return ((F(ck) * x).astype(F) + (F(cz) * z).astype(F)).astype(F)


# ---- the loop -------------------------------------------------------------------------------------------------------------
def run(eps_fn, orig, mask, shape, num_inference_steps, jump_length, jump_n_sample, eta, generator, clip=1.0,
        num_train=1000):
    """diffusers' ``RePaintPipeline.__call__`` loop on the CPU.  `eps_fn(x [N,C,H,W] fp32 ndarray, t) -> ndarray` is the
    network; `generator` a seeded torch CPU generator, drawn from in the protocol's order: x_T, then one [N,C,H,W] tensor per
    step entry and ``num_train // n`` per undo entry.  Returns (final x, records): one dict per entry with kind ("step" /
    "undo"), t (the entry's timestep; an undo entry starts from `t_from`), x_in, x_out, and eps for step entries."""
    import torch

    def randn():
        return torch.randn(tuple(shape), generator=generator, dtype=torch.float32).numpy()

    tabs = tables(num_train)
    n = min(num_train, num_inference_steps)
    ts = timesteps(num_inference_steps, jump_length, jump_n_sample, num_train)
    x = randn()
    records, t_last = [], int(ts[0]) + 1
    for t in (int(v) for v in ts):
        if t < t_last:
            eps = np.asarray(eps_fn(x, t), dtype=F)
            z = randn()
            out = step(x, eps, orig, mask, z, step_scalars(t, n, eta, num_train, tabs), clip, add_std=(t > 0 and eta > 0))
            records.append(dict(kind="step", t=t, x_in=x, eps=eps, x_out=out))
        else:
            out = x
            for ck, cz in undo_scalars(t_last, n, num_train, tabs):
                out = undo(out, randn(), ck, cz)
            records.append(dict(kind="undo", t=t, t_from=t_last, x_in=x, x_out=out))
        x, t_last = out, t
    return x, records
