"""What the split input of the MLP ops (PTG_MLP_SPLIT_INPUT) rests on that needs no GPU: the restatement's column
map against oracle/sb3_flat_oracle.py, the validity predicate of an index, the additive ABI, every new Python refusal with nothing
touched, what reaches the library, and DeviceMLP / TrainMLP(obs="split") on CPU modules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mlp_split_restatement as msr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sb3_flat_oracle as flat_oracle  # noqa: E402

F32 = np.float32
CONFIGS = [(raw, P) for raw in ("mod", "raw") for P in (1, 13, 25)]
WIDTH = {("mod", 1): 16, ("mod", 13): 40, ("mod", 25): 64, ("raw", 1): 19, ("raw", 13): 31, ("raw", 25): 43}


def _series(rng, n_hours=97, n_days=9, sets=3):
    return {k: rng.standard_normal((sets, n)).astype(F32) for k, n in (("featA", n_hours), ("featB", n_hours), ("gas_n", n_days), ("eua_n", n_days))}


def _rows(rng, B, series, raw, P):
    """[B, 16] split rows: a one-hot status, random env columns, indices over the whole valid range"""
    lh, ld = msr.last_valid(series, raw, P)
    rows = rng.standard_normal((B, 16)).astype(F32)
    rows[:, :6] = np.eye(6, dtype=F32)[rng.integers(0, 6, B)]
    rows[:, 14] = rng.integers(0, lh + 1, B)
    rows[:, 15] = rng.integers(0, ld + 1, B)
    rows[0, 14:16] = 0
    rows[-1, 14:16] = lh, ld
    return rows


# ------------------------------------------------------------------------------------------------- the column map
@pytest.mark.parametrize("raw,P", CONFIGS)
def test_the_column_map_against_the_flat_oracle(raw, P):
    """a canonical row (the reference's insertion order) built from a split row and the series, flattened by the oracle, is flat_rows()"""
    rng = np.random.default_rng(P + (raw == "raw"))
    series = _series(rng)
    B = 23
    rows = _rows(rng, B, series, raw, P)
    hi, di = rows[:, 14].astype(int), rows[:, 15].astype(int)
    win = lambda name, idx, w: series[name].reshape(-1)[idx[:, None] + np.arange(w)[None, :]]
    market = [win("featA", hi, P), win("featB", hi, P)] if raw == "mod" else [win("featA", hi, P), win("gas_n", di, 2), win("eua_n", di, 2)]
    canon = np.concatenate(market + [np.argmax(rows[:, :6], axis=1)[:, None].astype(F32), rows[:, 6:14]], axis=1)
    ref = flat_oracle.flatten_rows(canon, raw, P)
    got = msr.flat_rows(rows, series, raw, P)
    assert got.shape == ref.shape == (B, WIDTH[raw, P]) and got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    cmap = msr.column_map(raw, P)
    assert len(cmap) == WIDTH[raw, P] and sorted(c for kind, c in cmap if kind == "env") == list(range(14))
    assert len(msr.market_columns(raw, P)) == (2 * P if raw == "mod" else P + 4)


def test_the_validity_predicate_on_planted_indices():
    last = 84
    planted = np.array([0, last, last + 1, -1, 0.5, np.nan, 2.0 ** 24, np.inf, -np.inf, -0.0, last - 0.25, 1e30], F32)
    assert msr.valid_index(planted, last).tolist() == [True, True, False, False, False, False, False, False, False, True, False, False]
    assert msr.valid_index(F32(2.0 ** 24), 2 ** 24) and not msr.valid_index(F32(2.0 ** 24), 2 ** 24 - 1)
    rng = np.random.default_rng(0)
    series = _series(rng)
    for raw, P in CONFIGS:
        lh, ld = msr.last_valid(series, raw, P)
        assert (lh, ld) == (3 * 97 - P, 3 * 9 - 2)
        rows = _rows(rng, 9, series, raw, P)
        rows[1, 14], rows[2, 14], rows[3, 14], rows[4, 14], rows[5, 15], rows[6, 15] = lh + 1, -1, 0.5, np.nan, ld + 1, np.nan
        bad = msr.invalid_rows(rows, series, raw, P)
        assert bad.tolist() == [False, True, True, True, True, raw == "raw", raw == "raw", False, False]          # 'mod' never reads the day index
        flat = msr.flat_rows(rows, series, raw, P)
        mc = msr.market_columns(raw, P)
        ec = [k for k in range(flat.shape[1]) if k not in mc]
        assert np.isnan(flat[np.ix_(bad, mc)]).all() and np.isfinite(flat[np.ix_(~bad, mc)]).all() and np.isfinite(flat[:, ec]).all()
        ws, bs = msr.mr.net(rng, flat.shape[1], [5, 3])
        out, _ = msr.forward(rows, series, raw, P, ws, bs)
        assert np.isnan(out[bad]).all() and np.isfinite(out[~bad]).all()


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_flag_is_additive_to_abi_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert L.ptg_abi_version() == 13 and _lib.MLP_SPLIT_INPUT == 16
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_MLP_SPLIT_INPUT = 16" in hdr and "PTG_MLP_KEEP_HIDDEN = 1, PTG_MLP_NARROW = 2, PTG_MLP_WIDE = 4" in hdr and "PTG_MLP_ACCUMULATE = 8" in hdr
    W = lambda flags: L.ptg_mlp_workspace(17, 3, (C.c_int32 * 3)(233, 37, 3), flags)
    S, K = _lib.MLP_SPLIT_INPUT, _lib.MLP_KEEP_HIDDEN
    assert W(S) == W(0) > 0 and W(S | K) == W(K) > 0 and W(S | _lib.MLP_WIDE) == W(0)          # accepted and ignored
    assert W(S | _lib.MLP_NARROW | _lib.MLP_WIDE) < 0 and W(32) < 0 and W(S | 8) < 0
    assert L.ptg_mlp_backward_workspace(17, 3, (C.c_int32 * 3)(233, 37, 3), S) < 0            # the backward's own flags know no split


# ------------------------------------------------------------------------------------------------- the Python argument checks
def _engine(make, raw="mod", P=13, **attrs):
    return make(4, consts=dict(raw_modified=int(raw == "mod"), price_ahead=P), **attrs)


def test_every_new_python_refusal_touches_nothing():
    import torch
    from helpers import host_engine, mlp_layers
    B = 6
    rows, x2 = torch.zeros(B, 16), torch.zeros(B, 1)
    for raw, P in CONFIGS:
        eng = _engine(host_engine, raw, P)
        flat = WIDTH[raw, P]
        ws, bs = mlp_layers(flat + 1, [8, 8, 5])
        ws1, bs1 = mlp_layers(flat, [8, 8, 5])
        out, work = torch.zeros(B, 5), torch.zeros(eng.mlp_workspace(B, [8, 8, 5], True), dtype=torch.uint8)
        gw, gb = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs]
        fwd = lambda **kw: eng.mlp_forward(**{**dict(x=rows, weights=ws, biases=bs, x2=x2, split=True), **kw})
        bwd = lambda **kw: eng.mlp_backward(**{**dict(grad_out=out, x=rows, weights=ws, biases=bs, out=out, workspace=work, x2=x2, grad_weights=gw, grad_biases=gb,
                                                      split=True), **kw})
        gfw = lambda **kw: eng.mlp_group_forward(**{**dict(xs=rows, weights=[ws, ws], biases=[bs, bs], x2s=[x2, x2], split=True), **kw})
        gbw = lambda **kw: eng.mlp_group_backward(**{**dict(grad_outs=[out, out], xs=rows, weights=[ws, ws], biases=[bs, bs], outs=[out, out], workspaces=[work, work],
                                                            x2s=[x2, x2], split=True), **kw})
        refused = [
            # x is not [B, 16]
            (ValueError, lambda: fwd(x=torch.zeros(B, flat if flat != 16 else 17))), (ValueError, lambda: fwd(x=torch.zeros(B, 15))),
            (ValueError, lambda: bwd(x=torch.zeros(B, 40 if flat != 40 else 41))), (ValueError, lambda: gfw(xs=torch.zeros(B, 17))),
            (ValueError, lambda: gbw(xs=[rows, torch.zeros(B, 15)])),
            # the first weight's fan-in is not the flat width + F2
            (ValueError, lambda: fwd(x2=None)), (ValueError, lambda: fwd(weights=ws1, biases=bs1)),
            (ValueError, lambda: fwd(weights=mlp_layers(flat + 2, [8, 8, 5])[0])), (ValueError, lambda: bwd(weights=ws1, biases=bs1, grad_weights=None, grad_biases=None)),
            (ValueError, lambda: gfw(weights=[ws, ws1])), (ValueError, lambda: gbw(weights=[ws1, ws])),
            # an observation has no gradient
            (ValueError, lambda: bwd(grad_x=torch.zeros(B, flat))), (ValueError, lambda: bwd(grad_x=torch.zeros(B, 16))),
            (ValueError, lambda: gbw(grad_xs=[None, torch.zeros(B, flat)])),
            # TypeError stays first
            (TypeError, lambda: fwd(x=rows.double())), (TypeError, lambda: bwd(x=rows.numpy())),
        ]
        for k, (exc, fn) in enumerate(refused):
            with pytest.raises(exc, match="mlp_forward|mlp_backward|mlp_group"):
                fn()
            assert eng._L is None, (raw, P, k)
    with pytest.raises(ValueError, match="no gradient"):
        _engine(host_engine).mlp_backward(out, rows, *mlp_layers(40, [5]), out, torch.zeros(16, dtype=torch.uint8), grad_x=torch.zeros(B, 40), split=True)


def test_what_reaches_the_library():
    import torch
    from helpers import mlp_layers, recording_engine
    from rl_ptg_amd import _lib
    S, K = _lib.MLP_SPLIT_INPUT, _lib.MLP_KEEP_HIDDEN
    for raw, P in CONFIGS:
        eng = _engine(recording_engine, raw, P)
        flat, B = WIDTH[raw, P], 17
        wide = torch.zeros(B, 19)
        rows, x2 = wide[:, :16], torch.zeros(B, 3)                       # a column slice: row stride 19, guard columns behind the row
        ws, bs = mlp_layers(flat + 3, [9, 4])
        res = eng.mlp_forward(rows, ws, bs, x2=x2, keep_hidden=True, split=True, _route="narrow")
        assert [c[0] for c in eng._L.calls] == ["ptg_mlp_forward"]
        d = eng._L.calls[0][1][1]._obj
        assert (d.batch, d.n_layers, d.flags, d.f1, d.f2, d.x_dev, d.x_s_n, d.x2_dev, d.x2_s_n) == (B, 2, S | K | _lib.MLP_NARROW, flat, 3, rows.data_ptr(), 19, x2.data_ptr(), 3)
        assert list(d.w_s_n)[:2] == [flat + 3, 9] and list(d.width)[:3] == [9, 4, 0] and res.out.shape == (B, 4) and len(res.hidden) == 1
        eng._L.calls.clear()
        eng.mlp_forward(torch.zeros(1, 16), *mlp_layers(flat, [4]), split=True)                            # one piece, a contiguous row: stride 16
        d = eng._L.calls[0][1][1]._obj
        assert (d.flags, d.f1, d.f2, d.x_s_n, d.x2_dev) == (S, flat, 0, 16, None)
        eng._L.calls.clear()
        eng.mlp_forward(torch.zeros(1, flat), *mlp_layers(flat, [4]))                                       # without split: as before
        d = eng._L.calls[0][1][1]._obj
        assert (d.flags, d.f1, d.x_s_n) == (0, flat, flat)
        eng._L.calls.clear()
        # the backward: the flag travels in fwd.flags, the backward's own flags stay 0 / ACCUMULATE, dx stays NULL, dx2 is passed on
        out, work = res.out, torch.zeros(eng.mlp_workspace(B, [9, 4], True), dtype=torch.uint8)
        gw, gb, gx2 = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs], torch.zeros(B, 3)
        eng.mlp_backward(out, rows, ws, bs, out, work, x2=x2, grad_weights=gw, grad_biases=gb, grad_x2=gx2, accumulate=True, split=True)
        d = eng._L.calls[0][1][1]._obj
        assert (d.fwd.flags, d.flags, d.fwd.f1, d.fwd.x_s_n, d.dx_dev, d.dx2_dev, d.dx2_s_n) == (S | K, _lib.MLP_ACCUMULATE, flat, 19, None, gx2.data_ptr(), 3)
        assert list(d.dw_s_n)[:2] == [flat + 3, 9]
        eng._L.calls.clear()
        # the groups: every descriptor carries the flag
        eng.mlp_group_forward(rows, [ws, ws], [bs, bs], x2s=[x2, x2], split=True)
        name, args = eng._L.calls[0]
        assert name == "ptg_mlp_group_forward" and args[2] == 2 and [(n.flags, n.f1, n.x_s_n) for n in args[1]] == [(S, flat, 19)] * 2
        eng._L.calls.clear()
        eng.mlp_group_backward([out, out.clone()], rows, [ws, ws], [bs, bs], [out, out], [work, work.clone()], x2s=[x2, x2], grad_x2s=[gx2, None], split=True)
        name, args = eng._L.calls[0]
        assert name == "ptg_mlp_group_backward" and [(n.fwd.flags, n.flags, n.dx_dev, n.dx2_dev) for n in args[1]] == [(S | K, 0, None, gx2.data_ptr()), (S | K, 0, None, None)]


# ------------------------------------------------------------------------------------------------- the classes
def test_the_classes_take_obs_split_on_cpu_modules():
    import torch
    from torch import nn
    from helpers import host_engine, recording_engine
    from rl_ptg_amd import _lib
    from rl_ptg_amd.mlp import DeviceMLP, DeviceMLPGroup, TrainMLP, TrainMLPGroup
    S, K = _lib.MLP_SPLIT_INPUT, _lib.MLP_KEEP_HIDDEN
    pi = nn.Sequential(nn.Linear(40, 16), nn.Tanh(), nn.Linear(16, 5))
    qf = lambda: nn.Sequential(nn.Linear(41, 16), nn.ReLU(), nn.Linear(16, 1))
    for cls in (DeviceMLP, TrainMLP):
        with pytest.raises(ValueError, match="obs must be"):
            cls(_engine(host_engine), pi, batch=8, obs="rows")
    with pytest.raises(ValueError, match="TrainMLP"):
        TrainMLP(_engine(recording_engine), nn.Linear(39, 4), batch=8, obs="split")     # narrower than the flat row alone
    eng = _engine(recording_engine)
    net = DeviceMLP(eng, pi, batch=8, obs="split")
    assert net.split and net.in_features == 40 and eng._L.calls == []
    rows = torch.zeros(6, 16)
    y = net(rows)
    d = eng._L.calls[0][1][1]._obj
    assert (d.flags, d.f1, d.f2, d.x_s_n, d.batch) == (S, 40, 0, 16, 6) and y.shape == (6, 5) and y.data_ptr() == net.out.data_ptr()
    with pytest.raises(ValueError):
        net(torch.zeros(6, 40))                              # flat rows into a split net
    with pytest.raises(ValueError):
        DeviceMLP(eng, pi, batch=8)(rows)                    # split rows into a flat net
    with pytest.raises(ValueError):
        DeviceMLP(_engine(recording_engine, "raw", 13), pi, batch=8, obs="split")(rows)          # 'raw' at 13 has 31 columns, the net takes 40
    assert len(eng._L.calls) == 1
    eng._L.calls.clear()
    # TrainMLP: the gradient of x is None, grad_input holds the x2 part alone
    critic = TrainMLP(eng, qf(), batch=8, obs="split")
    assert critic.grad_input.shape == (8, 1) and TrainMLP(eng, pi, batch=8, obs="split").grad_input.shape == (8, 0)
    assert TrainMLP(eng, pi, batch=8).grad_input.shape == (8, 40)
    x, act = rows.clone().requires_grad_(True), torch.zeros(6, 1, requires_grad=True)
    q = critic(x, x2=act)
    q.backward(torch.ones_like(q))
    names = [c[0] for c in eng._L.calls]
    assert names == ["ptg_mlp_forward", "ptg_mlp_backward"]
    f, b = eng._L.calls[0][1][1]._obj, eng._L.calls[1][1][1]._obj
    assert (f.flags, f.f1, f.f2) == (S | K, 40, 1) and (b.fwd.flags, b.dx_dev, b.dx2_dev, b.dx2_s_n) == (S | K, None, critic.grad_input.data_ptr(), 1)
    assert x.grad is None and act.grad is not None and act.grad.shape == (6, 1)
    assert all(p.grad is not None for p in critic.parameters())
    eng._L.calls.clear()
    # the groups hand the flag to every member
    twins = TrainMLPGroup(eng, [qf(), qf()], batch=8, obs="split")
    assert all(n.split and n.grad_input.shape == (8, 1) for n in twins.nets)
    q0, q1 = twins(x, x2=act)
    torch.autograd.backward([q0, q1], [torch.ones_like(q0), torch.ones_like(q1)])
    (n0, a0), (n1, a1) = eng._L.calls
    assert (n0, n1) == ("ptg_mlp_group_forward", "ptg_mlp_group_backward")
    assert [n.flags for n in a0[1]] == [S | K] * 2 and [(n.fwd.flags, n.dx_dev) for n in a1[1]] == [(S | K, None)] * 2 and all(n.dx2_dev for n in a1[1])
    eng._L.calls.clear()
    out = DeviceMLPGroup(eng, [qf(), qf()], batch=8, obs="split")(rows, x2=act.detach())
    assert len(out) == 2 and [n.flags for n in eng._L.calls[0][1][1]] == [S] * 2
    assert not any(n.split for n in DeviceMLPGroup(eng, [qf(), qf()], batch=8).nets)
