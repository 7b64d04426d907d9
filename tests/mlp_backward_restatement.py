"""ptg_mlp_backward's arithmetic (include/ptg_env.h) restated in NumPy, on the fma of tests/mlp_restatement.py.  All float32, one rounding
per step.  Layer l with fan-in K, width O, input x, post-activation output h, g the gradient with respect to h:
    dz:  NONE g;  RELU h > 0 ? g : (h != h ? g : 0), a select;  TANH t = h * h; u = 1 - t; dz = g * u, three roundings
    dx[b][k] = the chain acc = 0;    acc = fmaf(dz[b][j], W[j][k], acc) over ascending j
    dW[j][k] = the chain acc = init; acc = fmaf(dz[b][j], x[b][k], acc) over ascending b
    db[j]    = the chain acc = init; acc = acc + dz[b][j] over ascending b
init is 0 or, accumulating, the value already there.  tests/test_mlp_backward_host.py pins these against exact float64 sums."""
import numpy as np

from mlp_restatement import NONE, RELU, TANH, act, fma32, forward, same_bits      # noqa: F401  (re-exported for the tests)

F32 = np.float32


def dact(h, g, kind):
    """dz from the kept post-activation output h and the gradient g with respect to it"""
    h, g = np.asarray(h, F32), np.asarray(g, F32)
    if kind == RELU:
        with np.errstate(invalid="ignore"):
            return np.where(h > 0, g, np.where(h != h, g, F32(0.0))).astype(F32)
    if kind == TANH:
        with np.errstate(all="ignore"):
            t = (h * h).astype(F32)
            u = (F32(1.0) - t).astype(F32)
            return (g * u).astype(F32)
    assert kind is NONE
    return g


def dx_chain(dz, W):
    """[B, O] dz, [O, K] W -> [B, K], j ascending from 0"""
    dz, W = np.asarray(dz, F32), np.asarray(W, F32)
    acc = np.zeros((dz.shape[0], W.shape[1]), F32)
    for j in range(W.shape[0]):
        acc = fma32(dz[:, j:j + 1], W[j][None, :], acc)
    return acc


def dw_chain(dz, x, init=None):
    """[B, O] dz, [B, K] x -> [O, K], b ascending from init (0 when None)"""
    dz, x = np.asarray(dz, F32), np.asarray(x, F32)
    acc = np.zeros((dz.shape[1], x.shape[1]), F32) if init is None else np.array(init, F32)
    for b in range(dz.shape[0]):
        acc = fma32(dz[b][:, None], x[b][None, :], acc)
    return acc


def db_chain(dz, init=None):
    """[B, O] dz -> [O], b ascending from init (0 when None): plain float32 additions"""
    dz = np.asarray(dz, F32)
    acc = np.zeros(dz.shape[1], F32) if init is None else np.array(init, F32)
    with np.errstate(all="ignore"):
        for b in range(dz.shape[0]):
            acc = (acc + dz[b]).astype(F32)
    return acc


def backward(gout, x, weights, hidden, out, hidden_act=RELU, out_act=NONE, x2=None, init_w=None, init_b=None, want_dx=True):
    """the whole pass on kept activations (hidden: the n - 1 post-activation hidden layers, out: the output) ->
    (dx [B, K0] or None, [dW_l], [db_l], [dz_l]); init_w / init_b: lists of the gradients to accumulate onto, or None"""
    x = np.asarray(x, F32) if x2 is None else np.concatenate([np.asarray(x, F32), np.asarray(x2, F32)], axis=1)
    n = len(weights)
    ins = [x] + [np.asarray(h, F32) for h in hidden]
    dz = dact(out, gout, out_act)
    dws, dbs, dzs, dx = [None] * n, [None] * n, [None] * n, None
    for l in range(n - 1, -1, -1):
        dzs[l] = dz
        dws[l] = dw_chain(dz, ins[l], None if init_w is None else init_w[l])
        dbs[l] = db_chain(dz, None if init_b is None else init_b[l])
        if l or want_dx:
            g = dx_chain(dz, weights[l])
            if l:
                dz = dact(ins[l], g, hidden_act)
            else:
                dx = g
    return dx, dws, dbs, dzs


def chain_bound(a, b, n):
    """gamma_(n+1) * sum |a| |b| for an n-step chain; a [R, n], b [n, C] -> [R, C]"""
    nu = (n + 1) * 2.0 ** -24
    return nu / (1.0 - nu) * (np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)))
