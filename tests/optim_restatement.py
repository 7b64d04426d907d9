"""The lines of ptg_optim_step (include/ptg_env.h) in NumPy: every element converted to float64, every operation one NumPy float64
operation (each rounded once, no fused multiply-add), results rounded once to the tensors' dtype.  tests/test_optim_host.py pins this
file against torch.optim.Adam, torch.optim.RMSprop, clip_grad_norm_ and SB3's polyak_update on the CPU; tests/test_optim.py compares
the kernels with it bit for bit, feeding it the kernel's own total norm (the one quantity whose value depends on a summation order)."""
import math

import numpy as np


def new_state():
    """the device state before the first step: step count and the running products beta1^t, beta2^t"""
    return {"t": 0.0, "p1": 1.0, "p2": 1.0}


def total_norm(grads):
    """clip_grad_norm_'s L2 norm over every element of every gradient: the square root of the exactly rounded sum (math.fsum) of the
    float64 squares"""
    return math.sqrt(math.fsum(float(x) * float(x) for g in grads for x in np.asarray(g, np.float64).ravel()))


def clip_coef(total, max_norm):
    """min(max_norm / (total + 1e-6), 1.0) with torch.clamp's rule for NaN (it stays); None: no clipping"""
    if max_norm is None:
        return 1.0
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(total) + np.float64(1e-6))
    return 1.0 if c > 1.0 else float(c)


def polyak(params, targets, tau):
    """SB3's polyak_update on the stored parameters -> the new targets"""
    tau = np.float64(tau)
    with np.errstate(all="ignore"):
        return [((np.float64(1.0) - tau) * q.astype(np.float64) + tau * p.astype(np.float64)).astype(q.dtype) for p, q in zip(params, targets)]


def step(kind, params, grads, state1, state2, st, lr, betas=(0.9, 0.999), eps=1e-8, alpha=0.99, max_norm=None, targets=None, tau=None, total=None,
         zero_grad=False):
    """One step.  params, grads, state1 (exp_avg | square_avg), state2 (exp_avg_sq; None for RMSprop), targets (optional): lists of
    arrays of one dtype; st: new_state() or what an earlier step left (advanced in place).  total: the total norm to clip with --
    None: total_norm(grads).  Returns dict(params, state1, state2, targets, grads, total, coef) with fresh arrays."""
    assert kind in ("adam", "rmsprop")
    f = np.float64
    if max_norm is not None and total is None:
        total = total_norm(grads)
    coef = f(clip_coef(total, max_norm))
    lr, eps = f(lr), f(eps)
    one = f(1.0)
    out = dict(params=[], state1=[], state2=[], targets=None, grads=[], total=total, coef=float(coef))
    with np.errstate(all="ignore"):
        st["t"] += 1.0
        if kind == "adam":
            b1, b2 = f(betas[0]), f(betas[1])
            st["p1"] = float(f(st["p1"]) * b1)
            st["p2"] = float(f(st["p2"]) * b2)
            step_size = lr / (one - f(st["p1"]))
            bc2 = np.sqrt(one - f(st["p2"]))
        for k, (p, g) in enumerate(zip(params, grads)):
            dt = p.dtype
            p64, gp = p.astype(f), g.astype(f) * coef
            if kind == "adam":
                m = b1 * state1[k].astype(f) + (one - b1) * gp
                v = b2 * state2[k].astype(f) + ((one - b2) * gp) * gp
                denom = np.sqrt(v) / bc2 + eps
                p64 = p64 + ((-step_size) * m) / denom
                out["state1"].append(m.astype(dt)); out["state2"].append(v.astype(dt))
            else:
                a = f(alpha)
                s = a * state1[k].astype(f) + ((one - a) * gp) * gp
                avg = np.sqrt(s) + eps
                p64 = p64 + ((-lr) * gp) / avg
                out["state1"].append(s.astype(dt))
            out["params"].append(p64.astype(dt))
            out["grads"].append(np.zeros_like(g) if zero_grad else g.copy())
    if targets is not None:
        out["targets"] = polyak(out["params"], targets, tau)
    return out
