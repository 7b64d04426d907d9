"""ptg_mlp_forward's arithmetic (include/ptg_env.h) restated in NumPy: per row b and unit j of a layer with fan-in K
    acc = bias[j];   for k = 0 .. K - 1 ascending: acc = fmaf(x[b][k], W[j][k], acc)   (float32, one rounding per step);   y = act(acc)
NumPy has no fma, so fma32 builds one: the product of two float32 is exact in float64 (48 bits), TwoSum gives the exact error of the
float64 sum p + c, the sum is moved to the ODD neighbour when it is inexact (round to odd), and the cast to float32 then rounds once --
float64 carries 53 >= 24 + 2 bits, so the double rounding is innocuous, subnormal float32 results included.
tests/test_mlp_host.py pins fma32 against exact rationals."""
import numpy as np

RELU, TANH, NONE = "relu", "tanh", None


def fma32(a, b, c):
    """the correctly rounded float32 of a * b + c for float32 arrays (broadcast); NaN / Inf go through float64's own rules"""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)      # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                      # TwoSum: p + c = s + e exactly
        fin = np.isfinite(s)
        bits = np.atleast_1d(s).view(np.int64).reshape(np.shape(s))
        even = (bits & 1) == 0
        move = fin & (e != 0) & even
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(move, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def act(v, kind):
    v = np.asarray(v, np.float32)
    if kind == RELU:
        with np.errstate(invalid="ignore"):
            return np.where(v > 0, v, np.where(v != v, v, np.float32(0.0))).astype(np.float32)
    if kind == TANH:
        return np.tanh(v.astype(np.float64)).astype(np.float32)
    assert kind is NONE
    return v


def pre_activation(x, W, b):
    """[B, K] x, [O, K] W, [O] b -> the float32 chains [B, O], k ascending"""
    x, W, b = np.asarray(x, np.float32), np.asarray(W, np.float32), np.asarray(b, np.float32)
    acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(np.float32)
    for k in range(W.shape[1]):
        acc = fma32(x[:, k:k + 1], W[None, :, k], acc)
    return acc


def forward(x, weights, biases, hidden_act=RELU, out_act=NONE, x2=None):
    """-> (out, [post-activation hidden layers])"""
    h = np.asarray(x, np.float32) if x2 is None else np.concatenate([np.asarray(x, np.float32), np.asarray(x2, np.float32)], axis=1)
    hidden = []
    n = len(weights)
    for l in range(n):
        h = act(pre_activation(h, weights[l], biases[l]), out_act if l == n - 1 else hidden_act)
        if l < n - 1:
            hidden.append(h)
    return h, hidden


def chain_bound(x, W, b):
    """the derived bound of a K-step fmaf chain against the exact sum: gamma_(K+1) * (|b| + sum |x| |w|), gamma_n = n u / (1 - n u), u = 2^-24"""
    K = W.shape[1]
    nu = (K + 1) * 2.0 ** -24
    mag = np.abs(np.asarray(b, np.float64))[None, :] + np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return nu / (1.0 - nu) * mag


def net(rng, fan_in, widths, scale=1.0):
    """random float32 weights and biases of a net, sized so that activations stay O(1)"""
    ws, bs, k = [], [], fan_in
    for o in widths:
        ws.append((rng.standard_normal((o, k)) * scale / np.sqrt(k)).astype(np.float32))
        bs.append((rng.standard_normal(o) * 0.1).astype(np.float32))
        k = o
    return ws, bs


def same_bits(got, ref):
    """float32 arrays equal through integer views, +0 == -0, a NaN meets a NaN"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, r = np.where(nan | (got == 0), np.float32(0), got), np.where(nan | (ref == 0), np.float32(0), ref)
    return bool(np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(r).view(np.int32)))
