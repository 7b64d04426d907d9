"""What ptg_mlp_forward rests on that needs no GPU: the NumPy fma of tests/mlp_restatement.py against exact rationals, a restated layer
against a float64 matmul within the derived chain bound, a net by hand, the struct layout, the workspace sizes, every Python-level
refusal (TypeError before ValueError, nothing touched) and DeviceMLP's parsing of Sequentials."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import mlp_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _round_f32(v):
    """a Fraction rounded to the nearest float32, ties to even, subnormals included (no overflow in these tests)"""
    if v == 0:
        return F32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    while Fraction(2) ** e > v:
        e -= 1
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = v / ulp
    n, r = divmod(q.numerator, q.denominator)
    rem = Fraction(r, q.denominator)
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return F32(sign * float(n * ulp))


def _exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.int32)[0])


def test_fma32_against_exact_rationals_on_random_cases():
    rng = np.random.default_rng(0)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3]) * (1 + rng.integers(-3, 4, len(c[::3])) * 2.0 ** -23)).astype(F32)      # planted cancellation
    got = mr.fma32(a, b, c)
    for i in range(n):
        assert _bits(got[i]) == _bits(_exact(a[i], b[i], c[i])), (a[i], b[i], c[i])


def test_fma32_on_planted_cases():
    one, eps = F32(1.0), F32(2.0 ** -23)
    cases = [
        (F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12), F32(0.0)),                             # 1 + 2^-11 + 2^-24: an exact tie at a float32 midpoint, to even
        (F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12), eps),                                # the same tie above an odd neighbour: rounds up
        (F32(3.0), F32(2.0 ** -25), one),                                               # 1 + 1.5 * 2^-24: above the midpoint
        (F32(1.25), F32(-0.8), F32(1.25) * F32(0.8)),                                   # near-total cancellation: the low bits of the product survive
        (F32(7.0), F32(-3.0), F32(21.0)),                                               # total cancellation: +0
        (F32(2.0 ** -70), F32(2.0 ** -70), F32(0.0)),                                   # a subnormal product kept: 2^-140
        (F32(2.0 ** -70), F32(1.5 * 2.0 ** -70), F32(2.0 ** -149)),                     # subnormal sum
        (F32(2.0 ** -75), F32(2.0 ** -75), F32(0.0)),                                   # 2^-150: the tie below the smallest subnormal, to even = 0
        (F32(0.0), F32(0.0), F32(-0.0)),                                                # fmaf(0, 0, -0) = +0
    ]
    for a, b, c in cases:
        got = mr.fma32(a, b, c)
        assert _bits(got) == _bits(_exact(a, b, c)), (a, b, c, got)
    assert _bits(mr.fma32(F32(0.0), F32(0.0), F32(-0.0))) == 0
    assert float(mr.fma32(F32(2.0 ** -70), F32(2.0 ** -70), F32(0.0))) == 2.0 ** -140
    # a double-rounding case: a * b + c = 1 + 2^-11 + 2^-24 + 2^-60 exactly.  float64 rounds it to 1 + 2^-11 + 2^-24, a float32 midpoint, and
    # casting that goes to even, 1 + 2^-11; the single rounding sees the 2^-60 and gives 1 + 2^-11 + 2^-23
    a, b = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12)                                     # a * b = 1 + 2^-11 + 2^-24 exactly
    c = F32(2.0 ** -60)
    with np.errstate(all="ignore"):
        naive = F32(np.float64(a) * np.float64(b) + np.float64(c))
    assert float(naive) == 1 + 2.0 ** -11                                               # float32(float64(a * b + c)): the tie went to even -- wrong
    assert float(mr.fma32(a, b, c)) == 1 + 2.0 ** -11 + 2.0 ** -23 == float(_exact(a, b, c))
    assert np.isnan(mr.fma32(F32(np.inf), F32(0.0), one)) and np.isinf(mr.fma32(F32(np.inf), one, one)) and np.isnan(mr.fma32(one, one, F32(np.nan)))


@pytest.mark.parametrize("K,O,kind", [(1, 1, mr.RELU), (5, 17, mr.RELU), (41, 33, mr.TANH), (233, 37, mr.RELU), (808, 16, mr.TANH)])
def test_a_restated_net_against_float64_layer_by_layer(K, O, kind):
    """each layer's float32 chain against the float64 matmul of the SAME (restated) inputs: within gamma_(K+1) * (|b| + sum |x| |w|)"""
    rng = np.random.default_rng(K)
    B = 9
    ws, bs = mr.net(rng, K, [O, 7, 3])
    x = rng.standard_normal((B, K)).astype(F32)
    out, hidden = mr.forward(x, ws, bs, hidden_act=kind)
    h = x
    for l in range(3):
        pre = mr.pre_activation(h, ws[l], bs[l])
        ref = h.astype(np.float64) @ ws[l].astype(np.float64).T + bs[l].astype(np.float64)
        assert (np.abs(pre.astype(np.float64) - ref) <= mr.chain_bound(h, ws[l], bs[l])).all()
        h = mr.act(pre, kind if l < 2 else mr.NONE)
        assert mr.same_bits(h, hidden[l] if l < 2 else out)


def test_a_net_by_hand():
    """2 -> 2 -> 1, ReLU, then tanh on the output; x = (1, -2) and (0.5, 4)"""
    W0, b0 = np.array([[1.0, 0.5], [-1.0, 0.25]], F32), np.array([0.5, -1.0], F32)
    W1, b1 = np.array([[2.0, -3.0]], F32), np.array([0.125], F32)
    x = np.array([[1.0, -2.0], [0.5, 4.0]], F32)
    # row 0: (0.5 + 1 - 1, -1 - 1 - 0.5) = (0.5, -2.5) -> relu (0.5, 0) -> 0.125 + 1 - 0 = 1.125
    # row 1: (0.5 + 0.5 + 2, -1 - 0.5 + 1) = (3, -0.5) -> relu (3, 0) -> 0.125 + 6 = 6.125
    out, hidden = mr.forward(x, [W0, W1], [b0, b1])
    assert hidden[0].tolist() == [[0.5, 0.0], [3.0, 0.0]] and out.tolist() == [[1.125], [6.125]]
    out, _ = mr.forward(x[:, :1], [W0, W1], [b0, b1], out_act=mr.TANH, x2=x[:, 1:])
    assert out.tolist() == [[float(F32(np.tanh(1.125)))], [float(F32(np.tanh(6.125)))]]
    assert mr.act(np.array([-0.0, np.nan, -1.0, 2.0], F32), mr.RELU).view(np.int32).tolist()[0] == 0 and np.isnan(mr.act(np.array([np.nan], F32), mr.RELU))[0]
    assert mr.same_bits(np.array([0.0, np.nan], F32), np.array([-0.0, np.nan], F32)) and not mr.same_bits(np.array([1.0], F32), np.array([np.nextafter(F32(1), F32(2))], F32))


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_symbols_and_the_abi_stays_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in ("ptg_mlp_forward", "ptg_mlp_workspace"))
    assert L.ptg_abi_version() == 13
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_MLP_RELU = 0, PTG_MLP_TANH = 1, PTG_MLP_NONE = 2" in hdr and "PTG_MLP_KEEP_HIDDEN = 1, PTG_MLP_NARROW = 2, PTG_MLP_WIDE = 4" in hdr
    assert "#define PTG_MLP_MAX_LAYERS 10" in hdr and "#define PTG_MLP_MAX_WIDTH 1024" in hdr
    assert (_lib.MLP_RELU, _lib.MLP_TANH, _lib.MLP_NONE, _lib.MLP_KEEP_HIDDEN, _lib.MLP_NARROW, _lib.MLP_WIDE) == (0, 1, 2, 1, 2, 4)
    assert (_lib.MLP_MAX_LAYERS, _lib.MLP_MAX_WIDTH) == (10, 1024)


def test_the_struct_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    fs = [f for f, _ in _lib.PtgMlp._fields_]
    body = 'printf("%zu", sizeof(ptg_mlp));\n' + "\n".join('printf(" %%zu", offsetof(ptg_mlp, %s));' % f for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.PtgMlp)] + [getattr(_lib.PtgMlp, f).offset for f in fs]


def test_the_workspace_sizes_and_the_null_handle():
    from helpers import host_engine
    from rl_ptg_amd import _lib
    L = _lib.lib()
    eng = host_engine(4)

    def W(B, widths, flags=0):
        return L.ptg_mlp_workspace(B, len(widths), (C.c_int32 * max(len(widths), 1))(*widths), flags)

    K = _lib.MLP_KEEP_HIDDEN
    assert W(1, [5]) == 16 and W(7, [5], K) == 16                                      # no hidden layer
    assert W(6, [64, 64, 5]) == 2 * 6 * 64 * 4 and W(6, [64, 64, 5], K) == 6 * 128 * 4
    assert W(17, [233, 37, 3]) == 2 * 17 * 236 * 4 and W(17, [233, 37, 3], K) == 17 * (236 + 40) * 4      # rows padded to 16 bytes
    assert W(1, [1, 1]) == 32 and W(1, [1, 1], K) == 16
    assert W(2 ** 31, [1024] * 10) == 2 * 2 ** 31 * 1024 * 4 and W(2 ** 31, [1024] * 10, K) == 9 * 2 ** 31 * 1024 * 4
    assert W(5, [8, 3], _lib.MLP_NARROW) == W(5, [8, 3], _lib.MLP_WIDE) == W(5, [8, 3])
    for bad in (W(0, [5]), W(2 ** 31 + 1, [5]), W(4, []), W(4, [5] * 11), W(4, [0, 5]), W(4, [5, 1025]), W(4, [5], 8), W(4, [5], _lib.MLP_NARROW | _lib.MLP_WIDE)):
        assert bad < 0
    assert L.ptg_mlp_workspace(4, 1, None, 0) < 0
    rng = np.random.default_rng(3)
    for _ in range(200):                                     # the Python restatement of the size that the argument checks use
        B, widths, keep = int(rng.integers(1, 5000)), [int(w) for w in rng.integers(1, 1025, int(rng.integers(1, 11)))], bool(rng.integers(0, 2))
        assert eng.mlp_workspace(B, widths, keep) == W(B, widths, K if keep else 0)
    for bad in ((0, [5]), (2 ** 31 + 1, [5]), (4, []), (4, [5] * 11), (4, [0]), (4, [1025])):
        with pytest.raises(ValueError):
            eng.mlp_workspace(*bad)
    assert L.ptg_mlp_forward(None, C.byref(_lib.PtgMlp()), None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the Python argument checks
def _net(fan_in, widths):
    import torch
    ws, bs, k = [], [], fan_in
    for o in widths:
        ws.append(torch.zeros(o, k))
        bs.append(torch.zeros(o))
        k = o
    return ws, bs


def test_python_argument_checks_need_no_device():
    import torch
    from helpers import faulty_mlp_nets, host_engine
    eng = host_engine(4)
    B = 6
    x, x2 = torch.zeros(B, 40), torch.zeros(B, 1)
    ws, bs = _net(41, [8, 8, 5])
    other = torch.device("meta")
    f = lambda **kw: eng.mlp_forward(**{**dict(x=x, weights=ws, biases=bs, x2=x2), **kw})
    need = eng.mlp_workspace(B, [8, 8, 5])
    # what the values are, the names, the counts, shapes, strides, devices of the net: the list mlp_backward is held to as well
    refused = [(exc, lambda kw=kw: eng.mlp_forward(**kw)) for exc, kw in faulty_mlp_nets(B)] + [
        (ValueError, lambda: f(_route="split")),
        # out and workspace
        (ValueError, lambda: f(out=torch.zeros(B, 5).double())), (ValueError, lambda: f(out=torch.zeros(B, 4))), (ValueError, lambda: f(out=torch.zeros(B + 1, 5))),
        (ValueError, lambda: f(out=torch.zeros(5, B).t())), (ValueError, lambda: f(out=torch.zeros(B, 5, device=other))), (ValueError, lambda: f(out=[torch.zeros(B, 5)])),
        (ValueError, lambda: f(workspace=torch.zeros(need))), (ValueError, lambda: f(workspace=torch.zeros(need - 1, dtype=torch.uint8))),
        (ValueError, lambda: f(workspace=torch.zeros(need + 8, dtype=torch.uint8)[1:])), (ValueError, lambda: f(workspace=torch.zeros(2 * need, dtype=torch.uint8)[::2])),
        (ValueError, lambda: eng.mlp_forward(x, *_net(40, [5]), workspace=torch.zeros(15, dtype=torch.uint8))),      # one layer still takes 16 bytes
    ]
    assert len(refused) == 49
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc, match="mlp_forward|mlp_workspace"):
            fn()
        assert eng._L is None, k


def test_a_refusal_reaches_nothing_and_a_good_call_reaches_the_library_once():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B = 17
    wide = torch.zeros(B, 50)
    x, x2 = wide[:, :40], wide[:, 45:46]                     # column slices of a wider buffer: row stride 50
    ws, bs = _net(41, [233, 37, 5])
    wpad = torch.zeros(233, 48)
    ws[0] = wpad[:, :41]                                     # a weight with a row stride above its fan-in
    with pytest.raises(TypeError):
        eng.mlp_forward(x.double(), ws, bs, x2=x2)
    with pytest.raises(ValueError):
        eng.mlp_forward(x, ws, bs)                           # fan-in 41 without the second piece
    with pytest.raises(ValueError):
        eng.mlp_forward(x, ws, bs, x2=x2, workspace=torch.zeros(16, dtype=torch.uint8))
    assert eng._L.calls == []
    outw = torch.zeros(B, 8)
    res = eng.mlp_forward(x, ws, bs, hidden_activation="tanh", out_activation="tanh", x2=x2, out=outw[:, 1:6], keep_hidden=True, _route="wide")
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_forward"]
    d = eng._L.calls[0][1][1]._obj
    assert (d.batch, d.n_layers, d.flags, d.hidden_act, d.out_act, d.f1, d.f2) == (B, 3, _lib.MLP_KEEP_HIDDEN | _lib.MLP_WIDE, _lib.MLP_TANH, _lib.MLP_TANH, 40, 1)
    assert (d.x_dev, d.x_s_n, d.x2_dev, d.x2_s_n) == (x.data_ptr(), 50, x2.data_ptr(), 50)
    assert list(d.w_dev)[:4] == [w.data_ptr() for w in ws] + [None] and list(d.w_s_n)[:3] == [48, 233, 37] and list(d.width)[:4] == [233, 37, 5, 0]
    assert list(d.b_dev)[:3] == [b.data_ptr() for b in bs]
    assert (d.out_dev, d.out_s_n) == (outw[:, 1:6].data_ptr(), 8) and res.out.data_ptr() == d.out_dev
    assert d.ws_bytes == 17 * (236 + 40) * 4 and len(res.hidden) == 2
    h0, h1 = res.hidden
    assert h0.shape == (B, 233) and h0.stride() == (236, 1) and h0.data_ptr() == d.ws_dev
    assert h1.shape == (B, 37) and h1.stride() == (40, 1) and h1.data_ptr() == d.ws_dev + 17 * 236 * 4
    eng._L.calls.clear()
    res = eng.mlp_forward(x[:1, :], [torch.zeros(3, 40)], [torch.zeros(3)])          # one row, one layer, everything allocated
    d = eng._L.calls[0][1][1]._obj
    assert (d.batch, d.n_layers, d.flags, d.hidden_act, d.out_act, d.f1, d.f2, d.x2_dev, d.x_s_n, d.ws_bytes) == (1, 1, 0, _lib.MLP_RELU, _lib.MLP_NONE, 40, 0, None, 50, 16)
    assert res.hidden is None and res.out.shape == (1, 3) and res.out.dtype == torch.float32


# ------------------------------------------------------------------------------------------------- DeviceMLP
def test_device_mlp_parses_sequentials_and_refuses_the_rest():
    import torch
    from torch import nn
    from helpers import host_engine, recording_engine
    from rl_ptg_amd.mlp import DeviceMLP, parse_mlp
    trunk = nn.Sequential(nn.Linear(40, 16), nn.ReLU(), nn.Linear(16, 16), nn.ReLU())
    mu, log_std = nn.Linear(16, 1), nn.Linear(16, 1)
    lin, hid, out = parse_mlp(trunk)
    assert [m.out_features for m in lin] == [16, 16] and (hid, out) == ("relu", "relu")          # a trunk alone ends in its activation
    lin, hid, out = parse_mlp([trunk, mu])
    assert [m.out_features for m in lin] == [16, 16, 1] and (hid, out) == ("relu", None) and lin[2] is mu
    lin, hid, out = parse_mlp(nn.Sequential(nn.Linear(40, 8), nn.Tanh(), nn.Linear(8, 5)))
    assert (hid, out) == ("tanh", None)
    lin, hid, out = parse_mlp(nn.Sequential(nn.Linear(40, 8), nn.ReLU(), nn.Linear(8, 1), nn.Tanh()))      # TD3's actor
    assert (hid, out) == ("relu", "tanh")
    assert parse_mlp(mu)[1:] == ("relu", None) and parse_mlp([log_std, nn.Tanh()])[1:] == ("relu", "tanh")
    half = nn.Linear(16, 1).half()
    t, v = TypeError, ValueError
    refused = [
        (t, nn.Sequential(nn.Linear(4, 4), nn.Sigmoid())), (t, [trunk, nn.LayerNorm(16), mu]), (t, [trunk, "mu"]), (t, [trunk, half]), (t, nn.Linear(4, 4).double()),
        (t, nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 4), nn.GELU())),      # TypeError before the mixed activations
        (v, nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 4))), (v, nn.Sequential(nn.Linear(4, 4), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 2))),
        (v, nn.Sequential(nn.ReLU(), nn.Linear(4, 4))), (v, nn.Sequential(nn.Linear(4, 4), nn.ReLU(), nn.ReLU())), (v, nn.Sequential()), (v, [nn.ReLU()]),
        (v, nn.Sequential(*[nn.Linear(4, 4) if i % 2 == 0 else nn.ReLU() for i in range(21)])), (v, nn.Linear(4, 4, bias=False)),
        (v, [nn.Linear(4, 5), nn.ReLU(), nn.Linear(4, 5)]),
    ]
    eng = host_engine(4)
    for k, (exc, m) in enumerate(refused):
        with pytest.raises(exc, match="DeviceMLP"):
            DeviceMLP(eng, m, batch=6)
        assert eng._L is None, k
    strided = nn.Linear(4, 4)
    strided.weight = nn.Parameter(torch.zeros(4, 4).t())
    with pytest.raises(ValueError):
        DeviceMLP(eng, strided, batch=6)
    with pytest.raises(ValueError):
        DeviceMLP(host_engine(4, device=torch.device("meta")), [trunk, mu], batch=6)          # the modules live on the CPU
    with pytest.raises(ValueError):
        DeviceMLP(eng, [trunk, mu], batch=0)
    assert eng._L is None
    # by reference: the call reads the parameters where they are; fewer rows than allocated give the first rows of the output
    eng = recording_engine(4)
    net = DeviceMLP(eng, [trunk, mu], batch=8, hidden=True)
    assert eng._L.calls == [] and net.out.shape == (8, 1) and net.workspace.numel() == 8 * 32 * 4
    y = net(torch.zeros(6, 40))
    d = eng._L.calls[0][1][1]._obj
    assert list(d.w_dev)[:3] == [trunk[0].weight.data_ptr(), trunk[2].weight.data_ptr(), mu.weight.data_ptr()] and list(d.b_dev)[2] == mu.bias.data_ptr()
    assert y.shape == (6, 1) and y.data_ptr() == net.out.data_ptr() and not y.requires_grad and len(net.hidden) == 2 and d.flags == _lib_keep()
    with pytest.raises(ValueError):
        net(torch.zeros(9, 40))
    with pytest.raises(TypeError):
        net(torch.zeros(6, 40).double())
    assert len(eng._L.calls) == 1


def _lib_keep():
    from rl_ptg_amd import _lib
    return _lib.MLP_KEEP_HIDDEN
