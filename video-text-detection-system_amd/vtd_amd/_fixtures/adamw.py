"""The AdamW recurrence of include/vtd.h (vtd_adamw_step) restated in numpy float32, and the normalised error levels the optimiser
tests hold a float32 run to.  It restates torch's documented AdamW update (decoupled weight decay, bias-corrected moments), every
operation rounded once to float32 in the order the kernel uses; the three scalars are formed in double and rounded once, as torch does
with its Python scalars."""
import math

import numpy as np

F32 = np.float32


def adamw_scalars(step, lr, betas, weight_decay):
    """(decay, step_size, bc2_sqrt) of one step as Python doubles; the caller rounds each once to float32."""
    beta1, beta2 = betas
    return 1.0 - lr * weight_decay, lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)


def adamw_step_f32(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """One AdamW step on float32 arrays: returns new (p, m, v), the inputs are left alone.  ``step`` is the 1-based step count."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    decay, step_size, bc2_sqrt = (F32(x) for x in adamw_scalars(step, lr, betas, weight_decay))
    omb1, beta2, omb2, eps = F32(1.0 - betas[0]), F32(betas[1]), F32(1.0 - betas[1]), F32(eps)
    with np.errstate(all="ignore"):
        p1 = p * decay
        m1 = m + omb1 * (g - m)
        v1 = v * beta2 + (omb2 * g) * g
        den = np.sqrt(v1) / bc2_sqrt + eps
        p2 = p1 - step_size * (m1 / den)
    assert p2.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
    return p2, m1, v1


def adamw_case(n, steps, seed):
    """(p0 [n], grads [steps, n]) float32 for the optimiser tests: parameters ~ N(0, 1); gradients ~ N(0, 1) times a per-element scale
    spread log-uniformly over 1e-22 .. 10 (their squares reach down into float32's subnormals and below), and an all-zero gradient at
    every 97th element.  Finite values only."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(F32)
    scale = 10.0 ** rng.uniform(-22.0, 1.0, n)
    scale[::97] = 0.0
    grads = (rng.standard_normal((steps, n)) * scale).astype(F32)
    return p0, grads


def adamw_levels(got, exact, grads, lr):
    """Normalised errors of a float32 run ``got`` = (p, m, v) against a float64 run ``exact`` of the same gradients, in units of
    float32's 2^-23:
        p: max |dp| / (max(|p|, lr) 2^-23)         one step moves p by about lr, so lr is the scale of a parameter near zero
        m: max |dm| / (max_k |g_k| 2^-23)          m is a running mean of the gradients the element has seen
        v: max |dv| / (max_k g_k^2 2^-23 + 2^-149) likewise for their squares; 2^-149 is the subnormal spacing
    ``grads``: [steps, n], every gradient the element received.  An element that only ever saw zero gradients has m = 0 exactly: any
    error there is reported as inf."""
    u = 2.0 ** -23
    gmax = np.abs(np.asarray(grads, dtype=np.float64)).max(axis=0)
    dp, dm, dv = (np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) for a, b in zip(got, exact))
    with np.errstate(divide="ignore", invalid="ignore"):
        lm = np.where(gmax > 0, dm / (gmax * u), np.where(dm == 0, 0.0, np.inf))
    return {"p": float((dp / (np.maximum(np.abs(np.asarray(exact[0], dtype=np.float64)), lr) * u)).max()),
            "m": float(lm.max()),
            "v": float((dv / (gmax * gmax * u + 2.0 ** -149)).max())}
