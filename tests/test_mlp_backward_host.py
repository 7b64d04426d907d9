"""What ptg_mlp_backward rests on that needs no GPU: the restatement (tests/mlp_backward_restatement.py) against exact float64 sums within
the derived chain bound gamma_(n+1) * sum |.||.| (n the chain length), two nets by hand, the ReLU select and the three Tanh roundings on
planted cases, the accumulate-split property, the struct layout, the workspace sizes, every Python-level refusal (TypeError before
ValueError, nothing touched) and TrainMLP's parsing."""
import ctypes as C
import os

import numpy as np
import pytest

import mlp_backward_restatement as br
import mlp_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _bits(x):
    return np.asarray(x, F32).view(np.int32).tolist()


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("K,O,kind", [(1, 1, mr.RELU), (5, 17, mr.RELU), (41, 33, mr.TANH), (233, 37, mr.RELU), (63, 129, mr.TANH)])
def test_the_restated_chains_against_float64_layer_by_layer(K, O, kind):
    """each layer's dx, dW and db chain against the float64 sums of the SAME (restated) float32 operands: within gamma_(n+1) * sum |.||.|,
    n = O for dx and n = B for dW and db"""
    rng = np.random.default_rng(K + O)
    B = 19
    ws, bs = mr.net(rng, K, [O, 7, 3])
    x = rng.standard_normal((B, K)).astype(F32)
    out, hidden = mr.forward(x, ws, bs, hidden_act=kind, out_act=kind)
    gout = rng.standard_normal((B, 3)).astype(F32)
    dx, dws, dbs, dzs = br.backward(gout, x, ws, hidden, out, hidden_act=kind, out_act=kind)
    ins = [x] + hidden
    f64 = lambda a: np.asarray(a, np.float64)
    for l in range(3):
        dz = dzs[l]
        assert (np.abs(f64(dws[l]) - f64(dz).T @ f64(ins[l])) <= br.chain_bound(dz.T, ins[l], B)).all()
        assert (np.abs(f64(dbs[l]) - f64(dz).sum(0)) <= br.chain_bound(dz.T, np.ones((B, 1)), B)[:, 0]).all()
        g = br.dx_chain(dz, ws[l])
        assert (np.abs(f64(g) - f64(dz) @ f64(ws[l])) <= br.chain_bound(dz, ws[l], ws[l].shape[0])).all()
        if l:
            assert mr.same_bits(dzs[l - 1], br.dact(ins[l], g, kind))
        else:
            assert mr.same_bits(dx, g)


def test_a_relu_net_by_hand():
    """2 -> 2 -> 1, ReLU; the forward of tests/test_mlp_host.py: hidden (0.5, 0) and (3, 0), out 1.125 and 6.125; gout = (2, -1)"""
    W0, b0 = np.array([[1.0, 0.5], [-1.0, 0.25]], F32), np.array([0.5, -1.0], F32)
    W1, b1 = np.array([[2.0, -3.0]], F32), np.array([0.125], F32)
    x = np.array([[1.0, -2.0], [0.5, 4.0]], F32)
    out, hidden = mr.forward(x, [W0, W1], [b0, b1])
    gout = np.array([[2.0], [-1.0]], F32)
    dx, dws, dbs, dzs = br.backward(gout, x, [W0, W1], hidden, out)
    # layer 1: dz1 = gout; dW1 = 2 * (0.5, 0) - (3, 0) = (-2, 0); db1 = 1; g = dz1 * W1 = (4, -6), (-2, 3); unit 1 is dead in both rows
    assert dzs[1].tolist() == [[2.0], [-1.0]] and dws[1].tolist() == [[-2.0, 0.0]] and dbs[1].tolist() == [1.0]
    assert dzs[0].tolist() == [[4.0, 0.0], [-2.0, 0.0]]
    # layer 0: dW0 row 0 = 4 * (1, -2) - 2 * (0.5, 4) = (3, -16), row 1 = 0; db0 = (2, 0); dx = dz0 @ W0 = (4, 2), (-2, -1)
    assert dws[0].tolist() == [[3.0, -16.0], [0.0, 0.0]] and dbs[0].tolist() == [2.0, 0.0]
    assert dx.tolist() == [[4.0, 2.0], [-2.0, -1.0]]
    dx2, _, _, _ = br.backward(gout, x[:, :1], [W0, W1], hidden, out, x2=x[:, 1:])
    assert mr.same_bits(dx, dx2)
    assert br.backward(gout, x, [W0, W1], hidden, out, want_dx=False)[0] is None


def test_a_tanh_net_by_hand():
    """2 -> 2 -> 1, Tanh hidden and output, weights chosen so that every pre-activation is exact; the derivative in three roundings"""
    W0, b0 = np.array([[1.0, 0.0], [0.0, 0.5]], F32), np.array([0.0, 0.0], F32)
    W1, b1 = np.array([[1.0, -2.0]], F32), np.array([0.0], F32)
    x = np.array([[0.5, 1.0]], F32)
    out, hidden = mr.forward(x, [W0, W1], [b0, b1], hidden_act=mr.TANH, out_act=mr.TANH)
    h = F32(np.tanh(0.5))
    assert hidden[0].tolist() == [[float(h), float(h)]]
    o = out[0, 0]
    gout = np.array([[3.0]], F32)
    dx, dws, dbs, dzs = br.backward(gout, x, [W0, W1], hidden, out, hidden_act=mr.TANH, out_act=mr.TANH)
    dz1 = F32(F32(3.0) * F32(F32(1.0) - F32(o * o)))
    assert _bits(dzs[1]) == _bits([[dz1]]) and _bits(dbs[1]) == _bits([dz1]) and _bits(dws[1]) == _bits([[F32(dz1 * h), F32(dz1 * h)]])
    u = F32(F32(1.0) - F32(h * h))
    dz0 = [F32(dz1 * u), F32(F32(dz1 * F32(-2.0)) * u)]
    assert _bits(dzs[0]) == _bits([dz0])
    assert _bits(dws[0]) == _bits([[F32(dz0[0] * F32(0.5)), dz0[0]], [F32(dz0[1] * F32(0.5)), dz0[1]]]) and _bits(dbs[0]) == _bits(dz0)
    assert _bits(dx) == _bits([[dz0[0], F32(dz0[1] * F32(0.5))]])


def test_the_relu_select_cases():
    nan, inf = F32(np.nan), F32(np.inf)
    h = np.array([0.0, -0.0, np.nan, -1.0, -1.0, -1.0, 2.0, 2.0, np.nan], F32)
    g = np.array([5.0, 5.0, 5.0, np.nan, np.inf, 5.0, np.nan, -0.0, np.nan], F32)
    dz = br.dact(h, g, mr.RELU)
    # h = +0 and -0 are dead: 0.  A NaN unit passes g.  A NaN or Inf g under a dead unit gives 0 -- a product g * 0 would give NaN
    assert dz[:3].tolist()[:2] == [0.0, 0.0] and dz[2] == 5.0
    assert _bits(dz[3:6]) == [0, 0, 0]
    assert np.isnan(dz[6]) and _bits(dz[7:8]) == _bits([-0.0]) and np.isnan(dz[8])
    with np.errstate(invalid="ignore"):
        assert np.isnan(nan * F32(0.0)) and np.isnan(inf * F32(0.0))                   # what the select avoids
    assert mr.same_bits(br.dact(h, g, mr.NONE), g)


def test_the_three_tanh_roundings_on_a_planted_case():
    """h = 1 - 2^-13: h * h = 1 - 2^-12 + 2^-26 rounds to t = 1 - 2^-12 (spacing 2^-24 below 1), u = 2^-12 exactly, and g * u = g * 2^-12.
    A fused u = fma(-h, h, 1) keeps the 2^-26: u = 2^-12 - 2^-26, a different float32"""
    h, g = F32(1 - 2.0 ** -13), F32(3.0)
    dz = br.dact(np.array([h]), np.array([g]), mr.TANH)
    assert float(dz[0]) == 3.0 * 2.0 ** -12
    fused_u = mr.fma32(-h, h, F32(1.0))
    assert float(fused_u) == 2.0 ** -12 - 2.0 ** -26 and float(F32(g * fused_u)) != float(dz[0])
    # and the form 1 - tanh^2 through (1 - h) * (1 + h) differs too
    assert float(F32(F32(F32(1) - h) * F32(F32(1) + h))) != 2.0 ** -12


def test_a_split_call_with_accumulate_leaves_the_bits_of_one_call():
    rng = np.random.default_rng(8)
    B, B1 = 23, 9
    ws, bs = mr.net(rng, 6, [11, 4])
    x = rng.standard_normal((B, 6)).astype(F32)
    gout = rng.standard_normal((B, 4)).astype(F32)
    out, hidden = mr.forward(x, ws, bs)
    _, dws, dbs, _ = br.backward(gout, x, ws, hidden, out)
    _, w1, b1, _ = br.backward(gout[:B1], x[:B1], ws, [h[:B1] for h in hidden], out[:B1])
    _, w2, b2, _ = br.backward(gout[B1:], x[B1:], ws, [h[B1:] for h in hidden], out[B1:], init_w=w1, init_b=b1)
    for l in range(2):
        assert _bits(w2[l]) == _bits(dws[l]) and _bits(b2[l]) == _bits(dbs[l])
    # the other order of the halves is another chain: the property is about order, not about addition
    _, w3, b3, _ = br.backward(gout[B1:], x[B1:], ws, [h[B1:] for h in hidden], out[B1:])
    _, w4, _, _ = br.backward(gout[:B1], x[:B1], ws, [h[:B1] for h in hidden], out[:B1], init_w=w3, init_b=b3)
    assert not mr.same_bits(w4[0], dws[0])


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_symbols_and_the_abi_stays():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in ("ptg_mlp_backward", "ptg_mlp_backward_workspace"))
    assert L.ptg_abi_version() == 13
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_MLP_ACCUMULATE = 8" in hdr and _lib.MLP_ACCUMULATE == 8
    assert _lib.MLP_ACCUMULATE & (_lib.MLP_KEEP_HIDDEN | _lib.MLP_NARROW | _lib.MLP_WIDE) == 0


def test_the_struct_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    fs = [f for f, _ in _lib.PtgMlpBwd._fields_]
    body = 'printf("%zu", sizeof(ptg_mlp_bwd));\n' + "\n".join('printf(" %%zu", offsetof(ptg_mlp_bwd, %s));' % f for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.PtgMlpBwd)] + [getattr(_lib.PtgMlpBwd, f).offset for f in fs]
    assert _lib.PtgMlpBwd.fwd.offset == 0 and _lib.PtgMlpBwd.fwd.size == C.sizeof(_lib.PtgMlp)


def test_the_workspace_sizes_and_the_null_handle():
    from helpers import host_engine
    from rl_ptg_amd import _lib
    L = _lib.lib()
    eng = host_engine(4)

    def W(B, widths, flags=0):
        return L.ptg_mlp_backward_workspace(B, len(widths), (C.c_int32 * max(len(widths), 1))(*widths), flags)

    assert W(1, [5]) == 2 * 8 * 4 and W(7, [1]) == 7 * 2 * 4 * 4
    assert W(6, [64, 64, 5]) == 2 * 6 * 64 * 4
    assert W(17, [37, 3, 233]) == 2 * 17 * 236 * 4                                     # the widest of ALL widths, the last one too, padded to 16 bytes
    assert W(2 ** 31, [1024] * 10) == 2 * 2 ** 31 * 1024 * 4
    assert W(5, [8, 3], _lib.MLP_ACCUMULATE) == W(5, [8, 3])
    for bad in (W(0, [5]), W(2 ** 31 + 1, [5]), W(4, []), W(4, [5] * 11), W(4, [0, 5]), W(4, [5, 1025]), W(4, [5], 1), W(4, [5], 2), W(4, [5], 4), W(4, [5], 16)):
        assert bad < 0
    assert L.ptg_mlp_backward_workspace(4, 1, None, 0) < 0
    rng = np.random.default_rng(3)
    for _ in range(200):
        B, widths = int(rng.integers(1, 5000)), [int(w) for w in rng.integers(1, 1025, int(rng.integers(1, 11)))]
        assert eng.mlp_backward_workspace(B, widths) == W(B, widths)
    assert eng.mlp_backward_workspace(2 ** 31, [1024]) == W(2 ** 31, [1024])
    for bad in ((0, [5]), (2 ** 31 + 1, [5]), (4, []), (4, [5] * 11), (4, [0]), (4, [1025])):
        with pytest.raises(ValueError):
            eng.mlp_backward_workspace(*bad)
    assert L.ptg_mlp_backward(None, C.byref(_lib.PtgMlpBwd()), None) == _lib.E_INVALID


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
    from helpers import host_engine
    eng = host_engine(4)
    B, widths = 6, [8, 8, 5]
    x, x2 = torch.zeros(B, 40), torch.zeros(B, 1)
    ws, bs = _net(41, widths)
    gws, gbs = _net(41, widths)
    other = torch.device("meta")
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)
    need_f, need_b = eng.mlp_workspace(B, widths, True), eng.mlp_backward_workspace(B, widths)
    base = dict(grad_out=torch.zeros(B, 5), x=x, weights=ws, biases=bs, out=torch.zeros(B, 5), workspace=u8(need_f), x2=x2, grad_weights=gws, grad_biases=gbs,
                grad_x=torch.zeros(B, 40), grad_x2=torch.zeros(B, 1), backward_workspace=u8(need_b))
    f = lambda **kw: eng.mlp_backward(**{**base, **kw})
    sub = lambda xs, l, t: xs[:l] + [t] + xs[l + 1:]
    refused = [
        # what the values are
        (TypeError, lambda: f(grad_out=None)), (TypeError, lambda: f(grad_out=torch.zeros(B, 5).double())), (TypeError, lambda: f(x=x.numpy())),
        (TypeError, lambda: f(x2=x2.half())), (TypeError, lambda: f(weights=ws[0])), (TypeError, lambda: f(biases=None)),
        (TypeError, lambda: f(weights=sub(ws, 1, ws[1].double()))), (TypeError, lambda: f(biases=sub(bs, 2, None))),
        (TypeError, lambda: f(grad_weights=None)), (TypeError, lambda: f(grad_biases=None)), (TypeError, lambda: f(grad_weights=gws[0])),
        (TypeError, lambda: f(x=torch.zeros(B, 2, 3), weights=sub(ws, 1, ws[1].double()))),        # TypeError before the ValueError of another argument
        (TypeError, lambda: f(hidden_activation="gelu", grad_out=torch.zeros(B, 5).long())),
        # the names, the counts
        (ValueError, lambda: f(hidden_activation="gelu")), (ValueError, lambda: f(hidden_activation=None)), (ValueError, lambda: f(out_activation="sigmoid")),
        (ValueError, lambda: f(weights=[], biases=[])), (ValueError, lambda: f(biases=bs[:2])), (ValueError, lambda: f(grad_weights=gws[:2])),
        (ValueError, lambda: f(grad_biases=gbs + gbs[:1])),
        # shapes, strides, devices
        (ValueError, lambda: f(x=torch.zeros(B))), (ValueError, lambda: f(x=torch.zeros(40, B).t())), (ValueError, lambda: f(x=torch.zeros(B, 40, device=other))),
        (ValueError, lambda: f(x2=torch.zeros(B + 1, 1))), (ValueError, lambda: f(x2=None, grad_x2=None)), (ValueError, lambda: f(x=x[:0], x2=x2[:0])),
        (ValueError, lambda: f(weights=sub(ws, 1, torch.zeros(8, 9)))), (ValueError, lambda: f(weights=sub(ws, 0, torch.zeros(41, 8).t()))),
        (ValueError, lambda: f(biases=sub(bs, 0, torch.zeros(9)))),
        (ValueError, lambda: f(grad_out=torch.zeros(B, 4))), (ValueError, lambda: f(grad_out=torch.zeros(B + 1, 5))), (ValueError, lambda: f(grad_out=torch.zeros(1, 5).expand(B, 5))),
        (ValueError, lambda: f(grad_out=torch.zeros(5, B).t())), (ValueError, lambda: f(grad_out=torch.zeros(B, 5, device=other))),
        (ValueError, lambda: f(out=None)), (ValueError, lambda: f(out=torch.zeros(B, 4))), (ValueError, lambda: f(out=torch.zeros(B, 5).double())),
        (ValueError, lambda: f(workspace=None)), (ValueError, lambda: f(workspace=u8(need_f - 1))), (ValueError, lambda: f(workspace=u8(need_f + 8)[1:])),
        (ValueError, lambda: f(workspace=torch.zeros(need_f))), (ValueError, lambda: f(workspace=u8(need_f - 4))),
        # the gradients
        (ValueError, lambda: f(grad_weights=sub(gws, 1, None))), (ValueError, lambda: f(grad_biases=sub(gbs, 0, None))),
        (ValueError, lambda: f(grad_weights=sub(gws, 0, torch.zeros(8, 40)))), (ValueError, lambda: f(grad_weights=sub(gws, 2, torch.zeros(5, 8).double()))),
        (ValueError, lambda: f(grad_weights=sub(gws, 0, torch.zeros(41, 8).t()))), (ValueError, lambda: f(grad_weights=sub(gws, 0, torch.zeros(8, 41, device=other)))),
        (ValueError, lambda: f(grad_biases=sub(gbs, 1, torch.zeros(9)))), (ValueError, lambda: f(grad_biases=sub(gbs, 1, torch.zeros(16)[::2]))),
        (ValueError, lambda: f(grad_x=torch.zeros(B, 41))), (ValueError, lambda: f(grad_x=torch.zeros(B + 1, 40))), (ValueError, lambda: f(grad_x=torch.zeros(40, B).t())),
        (ValueError, lambda: f(grad_x2=torch.zeros(B, 2))), (ValueError, lambda: f(x2=None, weights=sub(ws, 0, torch.zeros(8, 40)), grad_weights=sub(gws, 0, torch.zeros(8, 40)))),
        (ValueError, lambda: f(backward_workspace=u8(need_b - 1))), (ValueError, lambda: f(backward_workspace=u8(need_b + 8)[1:])),
        (ValueError, lambda: f(backward_workspace=torch.zeros(need_b))), (ValueError, lambda: f(backward_workspace=u8(2 * need_b)[::2])),
        (ValueError, lambda: f(grad_weights=sub(gws, 1, gws[1]), grad_biases=sub(gbs, 1, gbs[0]))),       # one tensor given twice
        (ValueError, lambda: f(grad_x2=base["grad_x"][:, :1])),
    ]
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc, match="mlp_backward|mlp_workspace"):
            fn()
        assert eng._L is None, k


def test_a_faulty_net_is_refused_in_the_forwards_words():
    """every faulty (x, x2, weights, biases, activations) of the forward's refusal list (helpers.faulty_mlp_nets, all 37 of them: none
    had to be left out), given to mlp_backward with otherwise good arguments: the same exception class, and the same text once the
    leading mlp_forward reads mlp_backward"""
    import torch
    from helpers import faulty_mlp_nets, host_engine
    eng = host_engine(4)
    B = 6
    nets = faulty_mlp_nets(B)
    assert len(nets) == 37
    rest = dict(grad_out=torch.zeros(B, 5), out=torch.zeros(B, 5), workspace=torch.zeros(eng.mlp_workspace(B, [8, 8, 5], True), dtype=torch.uint8))
    for k, (exc, kw) in enumerate(nets):
        with pytest.raises(exc) as fwd:
            eng.mlp_forward(**kw)
        with pytest.raises(exc) as bwd:
            eng.mlp_backward(**rest, **kw)
        text = str(fwd.value)
        assert type(fwd.value) is exc and type(bwd.value) is exc and text.startswith("mlp_forward: "), (k, text)
        assert str(bwd.value) == "mlp_backward" + text[len("mlp_forward"):], (k, text, str(bwd.value))
        assert eng._L is None, k


def test_a_refusal_reaches_nothing_and_a_good_call_reaches_the_library_once():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B, widths = 17, [233, 37, 5]
    wide = torch.zeros(B, 50)
    x, x2 = wide[:, :40], wide[:, 45:46]
    ws, bs = _net(41, widths)
    gws, gbs = _net(41, widths)
    gpad = torch.zeros(233, 48)
    gws[0] = gpad[:, :41]                                    # a weight gradient with a row stride above its fan-in
    gws[1], gbs[1] = None, None                              # a frozen layer
    out, gout = torch.zeros(B, 5), torch.zeros(B, 8)[:, 2:7]
    work = torch.zeros(eng.mlp_workspace(B, widths, True), dtype=torch.uint8)
    gxw = torch.zeros(B, 41)
    with pytest.raises(TypeError):
        eng.mlp_backward(gout.double(), x, ws, bs, out, work, x2=x2)
    with pytest.raises(ValueError):
        eng.mlp_backward(gout, x, ws, bs, out, work)         # fan-in 41 without the second piece
    assert eng._L.calls == []
    bws = eng.mlp_backward(gout, x, ws, bs, out, work, hidden_activation="tanh", out_activation="tanh", x2=x2, grad_weights=gws, grad_biases=gbs,
                           grad_x2=gxw[:, 40:], accumulate=True)
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_backward"]
    d = eng._L.calls[0][1][1]._obj
    fw = d.fwd
    assert (fw.batch, fw.n_layers, fw.flags, fw.hidden_act, fw.out_act, fw.f1, fw.f2) == (B, 3, _lib.MLP_KEEP_HIDDEN, _lib.MLP_TANH, _lib.MLP_TANH, 40, 1)
    assert (fw.x_dev, fw.x_s_n, fw.x2_dev, fw.x2_s_n, fw.out_dev, fw.out_s_n) == (x.data_ptr(), 50, x2.data_ptr(), 50, out.data_ptr(), 5)
    assert list(fw.w_dev)[:4] == [w.data_ptr() for w in ws] + [None] and list(fw.width)[:4] == [233, 37, 5, 0] and list(fw.b_dev)[:3] == [b.data_ptr() for b in bs]
    assert (fw.ws_dev, fw.ws_bytes) == (work.data_ptr(), work.numel())
    assert (d.gout_dev, d.gout_s_n, d.flags) == (gout.data_ptr(), 8, _lib.MLP_ACCUMULATE)
    assert list(d.dw_dev)[:4] == [gws[0].data_ptr(), None, gws[2].data_ptr(), None] and list(d.dw_s_n)[:3] == [48, 0, 37]
    assert list(d.db_dev)[:3] == [gbs[0].data_ptr(), None, gbs[2].data_ptr()]
    assert (d.dx_dev, d.dx2_dev, d.dx2_s_n) == (None, gxw[:, 40:].data_ptr(), 41)
    assert (d.bws_dev, d.bws_bytes) == (bws.data_ptr(), 2 * 17 * 236 * 4) and bws.dtype == torch.uint8
    eng._L.calls.clear()
    eng.mlp_backward(gout[:1, :3], x[:1], [torch.zeros(3, 40)], [torch.zeros(3)], out[:1, :3], torch.zeros(16, dtype=torch.uint8))      # one row, one layer, nothing asked for
    d = eng._L.calls[0][1][1]._obj
    assert (d.fwd.batch, d.fwd.n_layers, d.fwd.f2, d.flags, d.dx_dev, d.dx2_dev, d.bws_bytes) == (1, 1, 0, 0, None, None, 32) and list(d.dw_dev) == [None] * 10


# ------------------------------------------------------------------------------------------------- TrainMLP
def test_train_mlp_parses_sequentials_and_refuses_the_rest():
    import torch
    from torch import nn
    from helpers import host_engine, recording_engine
    from rl_ptg_amd import TrainMLP
    trunk = nn.Sequential(nn.Linear(40, 16), nn.ReLU(), nn.Linear(16, 16), nn.ReLU())
    mu = nn.Linear(16, 1)
    t, v = TypeError, ValueError
    refused = [(t, nn.Sequential(nn.Linear(4, 4), nn.Sigmoid())), (t, [trunk, nn.LayerNorm(16), mu]), (t, nn.Linear(4, 4).double()),
               (v, nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 4))), (v, nn.Sequential()), (v, nn.Linear(4, 4, bias=False)),
               (v, [nn.Linear(4, 5), nn.ReLU(), nn.Linear(4, 5)])]
    eng = host_engine(4)
    for k, (exc, m) in enumerate(refused):
        with pytest.raises(exc):
            TrainMLP(eng, m, batch=6)
        assert eng._L is None, k
    with pytest.raises(ValueError, match="TrainMLP"):
        TrainMLP(host_engine(4, device=torch.device("meta")), [trunk, mu], batch=6)
    with pytest.raises(ValueError):
        TrainMLP(eng, [trunk, mu], batch=0)
    eng = recording_engine(4)
    net = TrainMLP(eng, [trunk, mu], batch=8)
    assert eng._L.calls == [] and net.out.shape == (8, 1) and net.workspace.numel() == 8 * 32 * 4 and net.backward_workspace.numel() == 2 * 8 * 16 * 4
    assert [g.shape for g in net.grad_weights] == [(16, 40), (16, 16), (1, 16)] and net.grad_input.shape == (8, 40)
    x = torch.zeros(6, 40, requires_grad=True)
    y = net(x)
    assert y.shape == (6, 1) and y.grad_fn is not None and y.data_ptr() == net.out.data_ptr() and net.calls == 1
    d = eng._L.calls[0][1][1]._obj
    assert d.flags == 1 and list(d.w_dev)[:3] == [trunk[0].weight.data_ptr(), trunk[2].weight.data_ptr(), mu.weight.data_ptr()]      # by reference, keep_hidden
    y.sum().backward()
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_forward", "ptg_mlp_backward"]
    b = eng._L.calls[1][1][1]._obj
    assert b.dx_dev == net.grad_input.data_ptr() and b.dx2_dev is None and list(b.dw_dev)[:3] == [g.data_ptr() for g in net.grad_weights]
    assert mu.weight.grad is not None and mu.weight.grad.data_ptr() != net.grad_weights[2].data_ptr() and x.grad.shape == (6, 40)
    # a stale forward: the counter, not a copy
    y1 = net(x)
    net(x)
    with pytest.raises(RuntimeError, match="latest forward"):
        y1.sum().backward()
    # a frozen net and an input without a gradient: no dw and no first-layer dx
    for p in net.parameters():
        p.requires_grad_(False)
        p.grad = None
    eng._L.calls.clear()
    x2 = torch.zeros(6, 39)
    a = torch.zeros(6, 1, requires_grad=True)
    net(x2, x2=a).sum().backward()
    b = eng._L.calls[1][1][1]._obj
    assert list(b.dw_dev) == [None] * 10 and b.dx_dev is None and b.dx2_dev == net.grad_input[:, 39:].data_ptr() and b.dx2_s_n == 40
    assert all(p.grad is None for p in net.parameters()) and a.grad.shape == (6, 1)
    with pytest.raises(ValueError):
        net(torch.zeros(9, 40))
    with pytest.raises(TypeError):
        net(torch.zeros(6, 40).double())
