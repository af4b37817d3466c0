"""fp64 restatements of the streaming operations around the convolutions: GroupNorm forward / backward over cat(src0, src1),
per-channel sums, the small linear layers, SiLU, the timestep sinusoid, the loss reductions, unscale / clip / AdamW, nearest x2
and its adjoint.  Plain NumPy, no GPU import: tests/test_gpu_stream_edges.py compares the HIP kernels with these, and
tests/test_stream_oracle_cpu.py checks these against torch fp64 autograd and torch.optim.AdamW.

Every function takes array-likes and computes in float64 unless its name ends in _f32 (those restate a kernel's fp32 expression
in its order, for the bitwise checks).  For the 16-bit operations the caller passes the operands as stored after rounding
(round_bf16 / round_fp16) and gets fp64 back."""
import numpy as np

EPS_GN = 1e-5


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the two 16-bit roundings and the blocked layout, in host terms ------------------------------------------------------------
def round_bf16(x):
    """fp32 -> nearest bfloat16 (ties to even) -> fp32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def round_fp16(x):
    """fp32 -> nearest float16 (ties to even) -> fp32"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


ROUND = {"bf16": round_bf16, "fp16": round_fp16, "fp32": lambda x: np.asarray(x, dtype=np.float32)}


def to_blocked(x):
    """[N, C, H, W] -> [N, C/8, H, W, 8]"""
    x = np.asarray(x)
    n, c, h, w = x.shape
    return np.ascontiguousarray(x.reshape(n, c // 8, 8, h, w).transpose(0, 1, 3, 4, 2))


def from_blocked(xb):
    """[N, C/8, H, W, 8] -> [N, C, H, W]"""
    xb = np.asarray(xb)
    n, cb, h, w, _ = xb.shape
    return np.ascontiguousarray(xb.transpose(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w))


# ---- SiLU ----------------------------------------------------------------------------------------------------------------------
def sigmoid(z):
    z = f64(z)
    e = np.exp(-np.abs(z))          # never overflows
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def silu(z):
    return f64(z) * sigmoid(z)


def dsilu(z):
    s = sigmoid(z)
    return s * (1.0 + f64(z) * (1.0 - s))


# ---- GroupNorm over cat(src0, src1) ----------------------------------------------------------------------------------------------
def _cat(src0, src1):
    x = f64(src0)
    if src1 is not None:
        x = np.concatenate([x, f64(src1)], axis=1)
    return x.reshape(x.shape[0], x.shape[1], -1)          # [N, C, hw]


def gn_moments(sums, groups, hw, eps=EPS_GN):
    """per-(n, c) (sum, sum of squares) [N, C, 2] -> per-channel (mean, rstd), each [N, C] (a group's value on all its channels)"""
    sums = f64(sums)
    n, c, _ = sums.shape
    cpg = c // groups
    g = sums.reshape(n, groups, cpg, 2).sum(2)
    cnt = float(cpg) * float(hw)
    mean = g[..., 0] / cnt
    var = np.maximum(g[..., 1] / cnt - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    return np.repeat(mean, cpg, axis=1), np.repeat(rstd, cpg, axis=1)


def gn_forward(src0, gamma, beta, groups, src1=None, eps=EPS_GN, silu_on=False):
    """dict(mean, rstd, scale, shift [N, C]; y [N, C, hw]) of silu?(GroupNorm(cat(src0, src1))); the moments are taken about the
    mean (two passes), so they carry no cancellation whatever the group's mean / std ratio"""
    x = _cat(src0, src1)
    n, c, hw = x.shape
    cpg = c // groups
    xg = x.reshape(n, groups, cpg * hw)
    mean = xg.mean(2)
    var = ((xg - mean[..., None]) ** 2).mean(2)
    rstd = 1.0 / np.sqrt(var + eps)
    mean, rstd = np.repeat(mean, cpg, axis=1), np.repeat(rstd, cpg, axis=1)
    scale = rstd * f64(gamma)[None, :]
    shift = f64(beta)[None, :] - mean * scale
    y = (x - mean[..., None]) * scale[..., None] + f64(beta)[None, :, None]
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift, y=silu(y) if silu_on else y, x=x)


def gn_from_parts(stats0, gamma, beta, groups, hw, stats1=None, eps=EPS_GN):
    """the same four tables from per-tile partial statistics [N, c_i, tiles_i, 2]"""
    s = f64(stats0).sum(2)
    if stats1 is not None:
        s = np.concatenate([s, f64(stats1).sum(2)], axis=1)
    mean, rstd = gn_moments(s, groups, hw, eps)
    scale = rstd * f64(gamma)[None, :]
    return dict(mean=mean, rstd=rstd, scale=scale, shift=f64(beta)[None, :] - mean * scale)


def gn_backward(src0, dy, gamma, beta, groups, src1=None, eps=EPS_GN, silu_on=False):
    """closed-form gradients of L = <silu?(GroupNorm(cat(src0, src1))), dy>: (dx [N, C, hw], dgamma [C], dbeta [C]).
    With xhat = (x - mean) * rstd, u = xhat * gamma + beta, du = dy * silu'(u) and M the elements of a group:
      dgamma = sum_{n, hw} du * xhat,  dbeta = sum_{n, hw} du,
      dx = rstd * (gamma * du - (sum_group gamma * du) / M - xhat * (sum_group gamma * du * xhat) / M)."""
    f = gn_forward(src0, gamma, beta, groups, src1, eps)
    x = f["x"]
    n, c, hw = x.shape
    cpg = c // groups
    xhat = (x - f["mean"][..., None]) * f["rstd"][..., None]
    du = f64(dy).reshape(n, c, hw)
    if silu_on:
        du = du * dsilu(f["y"])
    dgamma, dbeta = (du * xhat).sum((0, 2)), du.sum((0, 2))
    gdu = du * f64(gamma)[None, :, None]
    m = float(cpg * hw)
    g1 = np.repeat(gdu.reshape(n, groups, -1).sum(2), cpg, axis=1)[..., None] / m
    g2 = np.repeat((gdu * xhat).reshape(n, groups, -1).sum(2), cpg, axis=1)[..., None] / m
    dx = f["rstd"][..., None] * (gdu - g1 - xhat * g2)
    return dx, dgamma, dbeta


def split_stats(x, tiles):
    """[N, C, ...] -> [N, C, tiles, 2]: (sum, sum of squares) of `tiles` consecutive runs of each channel's pixels (run lengths
    differ by at most one)"""
    x = f64(x)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    runs = np.array_split(np.arange(x.shape[2]), tiles)
    return np.stack([np.stack([x[:, :, r].sum(2), (x[:, :, r] ** 2).sum(2)], -1) for r in runs], 2)


def channel_sums(x):
    """([N, C] sums over the trailing dims, [N, C] sums of |x|)"""
    x = f64(x)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    return x.sum(2), np.abs(x).sum(2)


# ---- linear layer ----------------------------------------------------------------------------------------------------------------
def linear(x, w, b=None):
    y = f64(x) @ f64(w).T
    return y if b is None else y + f64(b)[None, :]


def linear_bwd(x, w, dy):
    """(dx, dw, db) of y = x W^T + b"""
    x, w, dy = f64(x), f64(w), f64(dy)
    return dy @ w, dy.T @ x, dy.sum(0)


# ---- timestep embedding ------------------------------------------------------------------------------------------------------------
def sinusoid(timesteps, freqs):
    """[N, 2 * len(freqs)], cos first: fp64 cos / sin of the fp32 angle fl(t * freq) the kernel forms"""
    t = np.asarray(timesteps).astype(np.float32)[:, None]
    ang = (t * np.asarray(freqs, dtype=np.float32)[None, :]).astype(np.float32)
    return np.concatenate([np.cos(f64(ang)), np.sin(f64(ang))], axis=1)


def time_embed(timesteps, freqs, w1, b1, w2, b2):
    """dict(emb, z1, z2, act): act = silu(z2), z2 = linear_2(silu(z1)), z1 = linear_1(emb)"""
    emb = sinusoid(timesteps, freqs)
    z1 = linear(emb, w1, b1)
    z2 = linear(silu(z1), w2, b2)
    return dict(emb=emb, z1=z1, z2=z2, act=silu(z2))


# ---- losses and norm -----------------------------------------------------------------------------------------------------------
def mse(pred, target, grad_scale=1.0):
    d = f64(pred) - f64(target)
    return float((d * d).mean()), 2.0 * grad_scale / d.size * d


def mse_weighted(pred, target, weights, grad_scale=1.0):
    """mean over all elements of weights[n] * (pred - target)^2, one weight per leading-dim sample"""
    d = f64(pred) - f64(target)
    w = f64(weights).reshape((-1,) + (1,) * (d.ndim - 1))
    return float((w * d * d).mean()), 2.0 * grad_scale / d.size * w * d


def l2_norm(x):
    return float(np.sqrt((f64(x) ** 2).sum()))


# ---- GradScaler.unscale_, clip_grad_norm_, AdamW ---------------------------------------------------------------------------------
def unscale_check_f32(g, inv_scale, found=0):
    """torch's _amp_foreach_non_finite_check_and_unscale_: found |= any element non-finite BEFORE scaling; g * inv in fp32"""
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        out = g * np.float32(inv_scale)
    return out, int(bool(found) or not np.isfinite(g).all())


def clip_factor_f32(total_norm, max_norm):
    """clip_grad_norm_'s factor as the kernels form it in fp32: max_norm / (norm + 1e-6); applied only when < 1"""
    return np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, total_norm=None, max_norm=0.0):
    """torch.optim.AdamW's single-tensor rule (decoupled decay, bias corrections) in fp64, the gradient first scaled by
    min(1, max_norm / (total_norm + 1e-6)) when total_norm is given; returns new (p, m, v)"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    if total_norm is not None:
        g = g * min(1.0, max_norm / (float(total_norm) + 1e-6))
    b1, b2 = betas
    p = p * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v


# ---- nearest x2 and its adjoint --------------------------------------------------------------------------------------------------
def upsample_nearest2x(x, axes=(-2, -1)):
    """every pixel copied to its 2x2 block; `axes`: the (h, w) axes ((-3, -2) for the blocked layout)"""
    x = np.asarray(x)
    return np.repeat(np.repeat(x, 2, axis=axes[0]), 2, axis=axes[1])


def _quads(x, axes):
    x = np.moveaxis(np.asarray(x), axes, (-2, -1))
    return x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]


def sumpool2x2(x, add=None, axes=(-2, -1)):
    a, b, c, d = (f64(q) for q in _quads(x, axes))
    out = np.moveaxis(a + b + c + d, (-2, -1), axes)
    return out if add is None else out + f64(add)


def sumpool2x2_f32(x, add=None, axes=(-2, -1)):
    """the kernels' fp32 expression: (a + b) + (c + d), then + add -- a, b the upper pixel pair, c, d the lower one"""
    a, b, c, d = (np.asarray(q, dtype=np.float32) for q in _quads(x, axes))
    out = np.moveaxis((a + b) + (c + d), (-2, -1), axes)
    return out if add is None else out + np.asarray(add, dtype=np.float32)
