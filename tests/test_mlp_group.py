"""ptg_mlp_group_forward / ptg_mlp_group_backward, HipEngine.mlp_group_forward / mlp_group_backward, DeviceMLPGroup and TrainMLPGroup
(include/ptg_env.h) against the SINGLE ops on the same tensors, bit for bit through mlp_restatement.same_bits: a grouped call is defined
as what the single call on each network's descriptor writes, and an element of the single ops does not depend on the grid, so there is no
tolerance anywhere in this file.  One test compares directly against the NumPy restatements, so that the file does not rest on the single
ops alone.

The harness is tests/test_mlp_backward.py's: the same sentinel frames around every strided output of every network (a workgroup that took
another network's strides or widths writes into a frame, a pad column or a workspace tail), the same result dictionary per network.  The
shapes are the smallest at which the grouped grid can go wrong: tile edges at 16, and networks whose tile counts differ in both grid
dimensions of every kernel, so that the early exit of a workgroup outside its own network runs next to workgroups that must not exit."""
import ctypes as C

import numpy as np
import pytest

import mlp_restatement as mr
import test_mlp_backward as tb

pytestmark = pytest.mark.gpu

SENTINEL = tb.SENTINEL
_engine, _t, _h, _pitch, _guarded, _frame_intact, _strided_in = tb._engine, tb._t, tb._h, tb._pitch, tb._guarded, tb._frame_intact, tb._strided_in

# (fan-in, its first piece or None, the widths at depth 3): unequal widths, a two-piece input, a network that is a single tile throughout;
# depth d takes the last d widths' worth: widths[3 - d:], the fan-in stays
NETS = [(40, None, [37, 37, 5]), (41, 40, [17, 17, 1]), (3, None, [33, 33, 17]), (5, None, [16, 9, 3]),
        (40, 1, [64, 33, 2]), (17, None, [5, 40, 16]), (33, 16, [3, 3, 33]), (16, None, [17, 16, 1])]


def _net_case(seed, B, i, depth):
    fi, f1, widths = NETS[i]
    x, ws, bs, gout = tb._case(seed * 100 + i, B, fi, widths[3 - depth:])
    return dict(x=x, ws=ws, bs=bs, gout=gout, f1=f1)


def _single(eng, c, **kw):
    return tb._run(eng, c["x"], c["ws"], c["bs"], c["gout"], f1=c["f1"], **{k: v for k, v in c.items() if k not in ("x", "ws", "bs", "gout", "f1")}, **kw)


def _run_group(eng, cases, hidden_act="relu", out_act=None, strided=False, accumulate=False, shared_x=False, order=None):
    """mlp_group_forward(keep_hidden) and mlp_group_backward on host arrays: tb._run for a group.  cases: per network a dict with x, ws, bs,
    gout, f1 and optionally params, frozen, want_dx, want_dx2, init_w, init_b (tb._run's arguments).  shared_x: every network reads
    network 0's input tensor(s).  order: the networks' places in the descriptor array.  Returns tb._run's dictionary per network."""
    import torch
    G = len(cases)
    si = _strided_in if strided else (lambda a, *_: _t(a))
    nets = []
    for i, c in enumerate(cases):
        x, ws, f1 = c["x"], c["ws"], c["f1"]
        B, K0 = x.shape
        n, widths = len(ws), [w.shape[0] for w in ws]
        if shared_x and i:
            xd, x2d = nets[0]["xd"], nets[0]["x2d"]
        else:
            xd = si(x if f1 is None else x[:, :f1])
            x2d = None if f1 is None else si(x[:, f1:], 1, 1)
        need_f, need_b = eng.mlp_workspace(B, widths, True), eng.mlp_backward_workspace(B, widths)
        nets.append(dict(B=B, K0=K0, n=n, widths=widths, F1=K0 if f1 is None else f1, xd=xd, x2d=x2d, wd=[si(w, 0, 5) for w in ws], bd=[_t(b) for b in c["bs"]],
                         need_f=need_f, need_b=need_b, work=torch.full((need_f + 64,), 0x5A, dtype=torch.uint8, device="cuda"), gd=si(c["gout"], 1, 2)))
    order = list(range(G)) if order is None else order
    pick = lambda key, f=None: [(nets[i][key] if f is None else f(nets[i])) for i in order]
    fwd = eng.mlp_group_forward(pick("xd"), pick("wd"), pick("bd"), hidden_activation=hidden_act, out_activation=out_act, x2s=pick("x2d"),
                                workspaces=pick(None, lambda t: t["work"][:t["need_f"]]), keep_hidden=True)
    eng.sync()
    for i, r in zip(order, fwd):
        nets[i]["fwd"], nets[i]["work_before"], nets[i]["out_before"] = r, nets[i]["work"].clone(), r.out.clone()
    for c, t in zip(cases, nets):
        n, widths, B, K0, F1 = t["n"], t["widths"], t["B"], t["K0"], t["F1"]
        fans = [K0] + widths[:-1]
        gw, gb, frames = None, None, []
        if c.get("params", True):
            gw, gb = [], []
            for l in range(n):
                if l in c.get("frozen", ()):
                    gw.append(None)
                    gb.append(None)
                    frames.append(None)
                    continue
                v, g = _guarded(widths[l], fans[l], None if c.get("init_w") is None else c["init_w"][l], strided)
                bv, bg = _guarded(1, widths[l], None if c.get("init_b") is None else c["init_b"][l][None, :], True)
                gw.append(v)
                gb.append(bv[0])
                frames.append((v.shape, g, bg))
        gx, gxf = _guarded(B, F1, None, strided) if c.get("want_dx", True) else (None, None)
        gx2, gx2f = _guarded(B, K0 - F1, None, strided) if (c["f1"] is not None and c.get("want_dx2", True)) else (None, None)
        t.update(gw=gw, gb=gb, frames=frames, gx=gx, gxf=gxf, gx2=gx2, gx2f=gx2f, bws=torch.full((t["need_b"] + 64,), 0x5A, dtype=torch.uint8, device="cuda"))
    ret = eng.mlp_group_backward(pick("gd"), pick("xd"), pick("wd"), pick("bd"), pick(None, lambda t: t["fwd"].out), pick(None, lambda t: t["work"][:t["need_f"]]),
                                 hidden_activation=hidden_act, out_activation=out_act, x2s=pick("x2d"), grad_weights=pick("gw"), grad_biases=pick("gb"), grad_xs=pick("gx"),
                                 grad_x2s=pick("gx2"), backward_workspaces=pick(None, lambda t: t["bws"][:t["need_b"]]), accumulate=accumulate)
    eng.sync()
    res = []
    for k, t in enumerate(nets):
        B, K0, F1, n, widths, need_b, bws, fw = t["B"], t["K0"], t["F1"], t["n"], t["widths"], t["need_b"], t["bws"], t["fwd"]
        ok = ret[order.index(k)].data_ptr() == bws.data_ptr() and bool((t["work"] == t["work_before"]).all()) and bool(torch.equal(fw.out, t["out_before"]))
        ok = ok and bool((bws[need_b:] == 0x5A).all())
        for fr in t["frames"]:
            if fr is not None:
                ok = ok and _frame_intact(fr[0], fr[1], strided) and _frame_intact((1, fr[2].shape[1] - 3), fr[2], True)
        ok = ok and (t["gx"] is None or _frame_intact((B, F1), t["gxf"], strided)) and (t["gx2"] is None or _frame_intact((B, K0 - F1), t["gx2f"], strided))
        Pw = max(_pitch(w) for w in widths)
        may = np.zeros(need_b // 4, bool)
        dz = {}
        flat = _h(bws[:need_b].view(torch.float32))
        for l in range(n):
            if l < n - 1 or out_act is not None:
                P = _pitch(widths[l])
                idx = (l & 1) * B * Pw + (np.arange(B)[:, None] * P + np.arange(widths[l])[None, :])
                may[idx.ravel()] = True
                if l < 2:
                    dz[l] = flat[idx]
        ok = ok and bool((_h(bws[:need_b]).reshape(-1, 4)[~may] == 0x5A).all())      # pad columns and what no layer owns
        dx = None
        if t["gx"] is not None or t["gx2"] is not None:
            dx = np.full((B, K0), np.nan, np.float32)
            if t["gx"] is not None:
                dx[:, :F1] = _h(t["gx"])
            if t["gx2"] is not None:
                dx[:, F1:] = _h(t["gx2"])
        gw, gb = t["gw"], t["gb"]
        res.append(dict(out=_h(fw.out), hidden=[_h(h) for h in fw.hidden], dx=dx, dws=None if gw is None else [None if g is None else _h(g) for g in gw],
                        dbs=None if gb is None else [None if g is None else _h(g) for g in gb], dz=dz, ok=ok, has_dx=t["gx"] is not None, has_dx2=t["gx2"] is not None, F1=F1))
    return res


def _same(got, ref, what=""):
    """two result dictionaries of one network, every array of them bit for bit"""
    assert got["ok"] and ref["ok"], f"{what}: a guard, a frozen gradient, a pad column, a workspace tail, the forward's workspace or the output was written"
    assert mr.same_bits(got["out"], ref["out"]), (what, "out")
    assert len(got["hidden"]) == len(ref["hidden"]) and all(mr.same_bits(a, b) for a, b in zip(got["hidden"], ref["hidden"])), (what, "hidden")
    assert (got["dx"] is None) == (ref["dx"] is None) and (got["dx"] is None or mr.same_bits(got["dx"], ref["dx"])), (what, "dx")
    assert (got["dws"] is None) == (ref["dws"] is None), (what, "dws")
    for l in range(len(got["dws"] or [])):
        assert (got["dws"][l] is None) == (ref["dws"][l] is None), (what, "frozen", l)
        if got["dws"][l] is not None:
            assert mr.same_bits(got["dws"][l], ref["dws"][l]), (what, "dW", l)
            assert mr.same_bits(got["dbs"][l], ref["dbs"][l]), (what, "db", l)
    assert got["dz"].keys() == ref["dz"].keys() and all(mr.same_bits(got["dz"][l], ref["dz"][l]) for l in got["dz"]), (what, "dz")


# ------------------------------------------------------------------------------------------------- groups of 1, 2, 3 and 8 over the grid
@pytest.mark.parametrize("B", [1, 6, 16, 17, 33])
def test_every_network_of_a_group_has_the_bits_of_its_single_call(B):
    """G in {1, 2, 3, 8}; the depth (1, 2, 3), the hidden activation, the output activation (NONE, TANH: the grouped k_mlp_dz_out) and the
    strided layout in sentinel frames walk with G and B.  out, every kept hidden layer, dx / dx2, every dW and db, dz of layers 0 and 1"""
    eng = _engine()
    ib = [1, 6, 16, 17, 33].index(B)
    for ig, G in enumerate((1, 2, 3, 8)):
        d = ib + ig
        depth, hidden_act, out_act, strided = 1 + d % 3, ("relu", "tanh")[d % 2], (None, "tanh")[(d // 2) % 2], (ib + 2 * ig) % 3 != 0
        cases = [_net_case(B, B, i, depth) for i in range(G)]
        got = _run_group(eng, cases, hidden_act=hidden_act, out_act=out_act, strided=strided)
        for i, c in enumerate(cases):
            _same(got[i], _single(eng, c, hidden_act=hidden_act, out_act=out_act, strided=strided), (B, G, i, depth, hidden_act, out_act, strided))


def test_the_row_rule_against_the_restatements():
    """three networks at B = 17, the NumPy restatements fed the op's own kept activations, as tests/test_mlp_backward.py does for one: the
    forward's chains on each kept layer, the backward's on the kept layers and the output"""
    eng = _engine()
    for hidden_act, out_act in (("relu", None), ("tanh", "tanh")):
        cases = [_net_case(7, 17, i, 3) for i in range(3)]
        got = _run_group(eng, cases, hidden_act=hidden_act, out_act=out_act, strided=True)
        for i, (c, r) in enumerate(zip(cases, got)):
            ins = [c["x"]] + r["hidden"]
            for l in range(3):
                want = mr.act(mr.pre_activation(ins[l], c["ws"][l], c["bs"][l]), out_act if l == 2 else hidden_act)
                assert mr.same_bits(r["hidden"][l] if l < 2 else r["out"], want), (i, l, hidden_act)
            tb._same_as_ref(r, tb._ref(r, c["x"], c["ws"], c["gout"], hidden_act=hidden_act, out_act=out_act), (i, hidden_act, out_act))


# ------------------------------------------------------------------------------------------------- shared inputs
def test_shared_inputs_and_shared_weights():
    """one x (two pieces, strided) read by three networks: twins of equal shapes and different weights give different, individually correct
    results; a third network that shares the first one's weight TENSORS gives the first one's bits"""
    import torch
    eng = _engine()
    B = 33
    a = _net_case(1, B, 1, 3)                                # 41 as 40 + 1 -> 17 -> 17 -> 1
    rng = np.random.default_rng(5)
    ws2, bs2 = mr.net(rng, 41, [17, 17, 1], scale=1.5)
    b = dict(a, ws=ws2, bs=bs2, gout=rng.standard_normal((B, 1)).astype(np.float32))
    got = _run_group(eng, [a, b, dict(a)], strided=True, shared_x=True)
    _same(got[0], _single(eng, a, strided=True), "twin 0")
    _same(got[1], _single(eng, b, strided=True), "twin 1")
    _same(got[2], got[0], "same weights")
    assert not np.array_equal(got[0]["out"], got[1]["out"]) and not np.array_equal(got[0]["dx"], got[1]["dx"])
    # the weight tensors themselves shared, through the raw call
    x, ws, bs = _t(a["x"][:, :40]), [_t(w) for w in a["ws"]], [_t(v) for v in a["bs"]]
    x2 = _t(a["x"][:, 40:])
    res = eng.mlp_group_forward(x, [ws, ws], [bs, bs], x2s=[x2, x2])
    eng.sync()
    assert res[0].out.data_ptr() != res[1].out.data_ptr() and torch.equal(res[0].out, res[1].out) and mr.same_bits(_h(res[0].out), got[0]["out"])


# ------------------------------------------------------------------------------------------------- per-network options
def test_per_network_options_leave_the_other_networks_alone():
    """a layer frozen in network 0 only; all parameter gradients off in network 1 only; dx wanted by network 2 only; dx2 only in network 1:
    the buffers a network did not ask for are untouched (they do not exist, and every frame around the others is intact), the rest of
    every network is its single call's with the same options"""
    eng = _engine()
    B = 33
    base = [_net_case(3, B, i, 3) for i in range(3)]
    plain = [_single(eng, c, strided=True) for c in base]
    for hidden_act in ("relu", "tanh"):
        opts = [dict(frozen=(1,), want_dx=False), dict(params=False, want_dx=False, want_dx2=True), dict(want_dx=True)]
        cases = [dict(c, **o) for c, o in zip(base, opts)]
        got = _run_group(eng, cases, hidden_act=hidden_act, strided=True)
        for i, c in enumerate(cases):
            _same(got[i], _single(eng, c, hidden_act=hidden_act, strided=True), (hidden_act, i))
        assert got[0]["dx"] is None and got[0]["dws"][1] is None and got[1]["dws"] is None and got[2]["dx"] is not None
        assert np.isnan(got[1]["dx"][:, :40]).all() and not np.isnan(got[1]["dx"][:, 40:]).any()
        if hidden_act == "relu":                             # and what was asked for does not depend on the options of the others
            assert mr.same_bits(got[0]["dws"][0], plain[0]["dws"][0]) and mr.same_bits(got[0]["dws"][2], plain[0]["dws"][2])
            assert mr.same_bits(got[1]["dx"][:, 40:], plain[1]["dx"][:, 40:]) and mr.same_bits(got[2]["dx"], plain[2]["dx"])
            assert all(mr.same_bits(a, b) for a, b in zip(got[2]["dws"] + got[2]["dbs"], plain[2]["dws"] + plain[2]["dbs"]))
    # no network wants parameter gradients of layer 1, and none wants dx: those launches are not issued, the rest is unchanged
    cases = [dict(c, frozen=(1,), want_dx=False, want_dx2=False) for c in base]
    got = _run_group(eng, cases)
    for i, c in enumerate(cases):
        _same(got[i], _single(eng, c), ("none", i))
    # dx wanted by the LAST network only, whose input is the narrowest: the dx grid is that network's
    cases = [dict(c, want_dx=(i == 2), want_dx2=False) for i, c in enumerate(base)]
    got = _run_group(eng, cases, strided=True)
    for i, c in enumerate(cases):
        _same(got[i], _single(eng, c, strided=True), ("last", i))


def test_accumulate_per_network():
    """rows [0, 17) plus an accumulating call on rows [17, 33) = one call on 33 rows, for each of three networks"""
    eng = _engine()
    B = 33
    cases = [_net_case(4, B, i, 3) for i in range(3)]
    cut = lambda c, s: dict(c, x=c["x"][s], gout=c["gout"][s])
    full = _run_group(eng, cases)
    first = _run_group(eng, [cut(c, slice(0, 17)) for c in cases])
    second = _run_group(eng, [dict(cut(c, slice(17, B)), init_w=f["dws"], init_b=f["dbs"]) for c, f in zip(cases, first)], accumulate=True, strided=True)
    for i in range(3):
        assert first[i]["ok"] and second[i]["ok"] and full[i]["ok"]
        for l in range(3):
            assert mr.same_bits(second[i]["dws"][l], full[i]["dws"][l]) and mr.same_bits(second[i]["dbs"][l], full[i]["dbs"][l]), (i, l)
        _same(full[i], _single(eng, cases[i]), i)


def test_the_order_of_the_networks_changes_no_bits_and_two_runs_agree():
    eng = _engine()
    cases = [_net_case(5, 17, i, 3) for i in (0, 1, 2, 3)]
    a = _run_group(eng, cases, hidden_act="tanh", out_act="tanh", strided=True)
    b = _run_group(eng, cases, hidden_act="tanh", out_act="tanh", strided=True, order=[3, 2, 1, 0])
    c = _run_group(eng, cases, hidden_act="tanh", out_act="tanh", strided=True)
    for i in range(4):
        _same(b[i], a[i], ("reversed", i))
        _same(c[i], a[i], ("again", i))


def test_the_skip_rules_of_the_one_walk_through_both_entries():
    """The launches the shared walk leaves out, decided by one rule for ptg_mlp_backward and ptg_mlp_group_backward: every layer frozen with
    grad_x and grad_x2 wanted (no dw launch at all), layer 1 frozen alone, and neither grad_x nor grad_x2 (the walk ends after dw(0)), each
    without and with an output activation (the dz_out launch), through the single entry and as network 0 of a group of two whose other
    network wants everything.  B = 17 and 41 (40 + 1) -> 33 -> 17 -> 5: a ragged tile in every grid dimension of every kernel, and the
    bias column K = 16 k + 1 of dw(1) and dw(2) in a tile of its own.  What a pattern still writes has the bits of the call that wants
    everything; a frozen layer and an unwanted dx have no tensor, and every sentinel frame, pad column and workspace tail around the
    written ones is intact (the harness's `ok`)"""
    eng = _engine()
    B = 17
    x, ws, bs, gout = tb._case(77, B, 41, [33, 17, 5])
    net = dict(x=x, ws=ws, bs=bs, gout=gout, f1=40)
    other = _net_case(77, B, 0, 3)                           # 40 -> 37 -> 37 -> 5: other tile counts in every launch
    patterns = [dict(frozen=(0, 1, 2)), dict(frozen=(1,)), dict(want_dx=False, want_dx2=False)]

    def written_same(got, full, p, what):
        assert got["ok"] and full["ok"], what
        assert mr.same_bits(got["out"], full["out"]) and all(mr.same_bits(a, b) for a, b in zip(got["hidden"], full["hidden"])), what
        for l in range(3):
            if l in p.get("frozen", ()):
                assert got["dws"][l] is None and got["dbs"][l] is None, (what, l)
            else:
                assert mr.same_bits(got["dws"][l], full["dws"][l]) and mr.same_bits(got["dbs"][l], full["dbs"][l]), (what, l)
        if p.get("want_dx", True):
            assert not np.isnan(got["dx"]).any() and mr.same_bits(got["dx"], full["dx"]), what
        else:
            assert got["dx"] is None and not got["has_dx"] and not got["has_dx2"], what
        assert got["dz"].keys() == full["dz"].keys() == {0, 1} and all(mr.same_bits(got["dz"][l], full["dz"][l]) for l in (0, 1)), what

    for hidden_act, out_act in (("relu", None), ("tanh", "tanh")):
        kw = dict(hidden_act=hidden_act, out_act=out_act, strided=True)
        full, other_full = _single(eng, net, **kw), _single(eng, other, **kw)
        for p in patterns:
            written_same(_single(eng, dict(net, **p), **kw), full, p, ("single", out_act, p))
            got = _run_group(eng, [dict(net, **p), other], **kw)
            written_same(got[0], full, p, ("group", out_act, p))
            _same(got[1], other_full, ("the other network", out_act, p))


# ------------------------------------------------------------------------------------------------- the classes
def _moved(eng, modules):
    """a DeviceOptimizer step and a Polyak update move the parameters IN PLACE: what the classes hold by reference must follow"""
    import torch
    from rl_ptg_amd import DeviceOptimizer
    params = [p for m in modules for p in m.parameters()]
    for k, p in enumerate(params):
        p.grad = torch.full_like(p, 0.01 * (k + 1))
    DeviceOptimizer(eng, params, kind="adam", lr=1e-2).step()
    targets = [torch.zeros_like(p) for p in params]
    eng.polyak_update([p.detach() for p in params], targets, 0.5)
    with torch.no_grad():
        for p, t in zip(params, targets):
            p.copy_(t + 0.5 * p)
    for p in params:
        p.grad = None
    eng.sync()


def test_device_mlp_group_is_its_device_mlps():
    import torch
    from rl_ptg_amd import DeviceMLP, DeviceMLPGroup
    eng = _engine()
    B = 33
    mods = [tb._seq([41, 37, 37, 1], seed=1), tb._seq([41, 17, 33, 1], seed=2), tb._seq([41, 5, 16, 2], seed=3)]
    grp = DeviceMLPGroup(eng, mods, batch=64)
    singles = [DeviceMLP(eng, m, batch=64) for m in mods]
    rng = np.random.default_rng(8)
    x, x2 = _t(rng.standard_normal((B, 40)).astype(np.float32)), _t(rng.standard_normal((B, 1)).astype(np.float32))
    before = [_h(o).copy() for o in grp(x, x2=x2)]
    _moved(eng, mods)
    outs = grp(x, x2=x2)
    eng.sync()
    assert len(outs) == 3 and all(o.shape == (B, w) and o.grad_fn is None for o, w in zip(outs, (1, 1, 2)))
    for i, s in enumerate(singles):
        want = s(x, x2=x2)
        eng.sync()
        assert mr.same_bits(_h(outs[i]), _h(want)) and not np.array_equal(_h(outs[i]), before[i]), i
    own = [x, _t(rng.standard_normal((B, 40)).astype(np.float32)), x]      # a list: each network its own input
    outs = grp(own, x2=[x2, x2, x2])
    eng.sync()
    assert mr.same_bits(_h(outs[1]), _h(singles[1](own[1], x2=x2)))


def test_train_mlp_group_gradients_are_its_train_mlps():
    import copy
    import torch
    from rl_ptg_amd import TrainMLP, TrainMLPGroup
    eng = _engine()
    B = 33
    mods = [tb._seq([41, 37, 37, 1], seed=4), tb._seq([41, 17, 33, 1], seed=5)]
    twins = copy.deepcopy(mods)
    grp, singles = TrainMLPGroup(eng, mods, batch=64), [TrainMLP(eng, m, batch=64) for m in twins]
    rng = np.random.default_rng(9)
    x, x2 = rng.standard_normal((B, 40)).astype(np.float32), rng.standard_normal((B, 1)).astype(np.float32)
    gouts = [_t(rng.standard_normal((B, 1)).astype(np.float32)) for _ in mods]
    same = lambda a, b: np.array_equal(_h(a).view(np.int32), _h(b).view(np.int32))
    xa, xb = _t(x).requires_grad_(True), _t(x2).requires_grad_(True)
    qs = grp(xa, x2=xb)
    assert all(q.grad_fn is not None and q.shape == (B, 1) for q in qs) and [p is q for p, q in zip(grp.parameters(), [p for m in mods for p in m.parameters()])] == [True] * 12
    torch.autograd.backward(list(qs), gouts)
    eng.sync()
    dxs = []
    for i, s in enumerate(singles):                          # each TrainMLP on its own leaves: dx_i of the raw op
        ya, yb = _t(x).requires_grad_(True), _t(x2).requires_grad_(True)
        q = s(ya, x2=yb)
        assert same(q, qs[i])
        q.backward(gouts[i])
        eng.sync()
        dxs.append((ya.grad.clone(), yb.grad.clone()))
        assert all(p.grad is not None and same(p.grad, t.grad) for p, t in zip(mods[i].parameters(), twins[i].parameters())), i
    # the shared input: autograd's own sum of the networks' dx, in network order, in float32
    assert same(xa.grad, dxs[0][0] + dxs[1][0]) and same(xb.grad, dxs[0][1] + dxs[1][1])
    # a second backward adds to .grad
    g0 = _h(mods[0][0].weight.grad).copy()
    torch.autograd.backward(list(grp(xa, x2=xb)), gouts)
    eng.sync()
    assert np.array_equal(_h(mods[0][0].weight.grad), g0 + g0)
    # a network whose output is unused keeps .grad None; the other one's gradients are unchanged
    for p in grp.parameters():
        p.grad = None
    grp(xa, x2=xb)[1].backward(gouts[1])
    eng.sync()
    assert all(p.grad is None for p in mods[0].parameters()) and all(same(p.grad, t.grad) for p, t in zip(mods[1].parameters(), twins[1].parameters()))
    # the stale forward
    stale = grp(xa, x2=xb)
    grp(xa, x2=xb)
    with pytest.raises(RuntimeError, match="latest forward"):
        stale[0].backward(gouts[0])
    # a frozen network launches nothing for its parameters: its gradient buffers keep the sentinel, the input's gradient is still the raw op's
    for p in list(mods[0].parameters()) + list(mods[1].parameters()):
        p.grad = None
    for p in mods[0].parameters():
        p.requires_grad_(False)
    for t in grp.nets[0].grad_weights + grp.nets[0].grad_biases:
        t.fill_(SENTINEL)
    xa.grad = xb.grad = None
    torch.autograd.backward(list(grp(xa.detach(), x2=xb)), gouts)
    eng.sync()
    assert all(bool((t == SENTINEL).all()) for t in grp.nets[0].grad_weights + grp.nets[0].grad_biases) and all(p.grad is None for p in mods[0].parameters())
    assert all(same(p.grad, t.grad) for p, t in zip(mods[1].parameters(), twins[1].parameters())) and xa.grad is None and same(xb.grad, dxs[0][1] + dxs[1][1])
    with torch.no_grad():
        assert all(q.grad_fn is None for q in grp(xa, x2=xb))


# ------------------------------------------------------------------------------------------------- one integrated step, captured
def test_a_captured_td3_twin_critic_step_replayed_three_times():
    """twin critics 41 (40 + 1) -> 37 -> 37 -> 1 at B = 33: mlp_group_forward(keep_hidden) -> td_loss("td3") -> mlp_group_backward into
    preallocated .grad tensors -> DeviceOptimizer.step() with clipping, captured on a side stream at the default hardware-queue setting and
    replayed three times with fresh batches written in place: the parameters are bit-equal to a twin pair's driven eagerly through the
    SINGLE ops"""
    import torch
    from rl_ptg_amd import DeviceOptimizer
    eng = _engine()
    B, F, widths = 33, 40, [37, 37, 1]

    class Step:
        def __init__(self, grouped):
            self.grouped = grouped
            self.nets = [tb._seq([F + 1] + widths, seed=21 + k) for k in range(2)]
            self.lin = [[m for m in net if isinstance(m, torch.nn.Linear)] for net in self.nets]
            params = [p for net in self.nets for p in net.parameters()]
            for p in params:
                p.grad = torch.zeros_like(p)
            self.w, self.b = [[m.weight.detach() for m in lin] for lin in self.lin], [[m.bias.detach() for m in lin] for lin in self.lin]
            self.gw, self.gb = [[m.weight.grad for m in lin] for lin in self.lin], [[m.bias.grad for m in lin] for lin in self.lin]
            z = lambda *s, **kw: torch.zeros(*s, device="cuda", **kw)
            self.obs, self.act, self.nq, self.rew, self.done = z(B, F), z(B, 1), [z(B, 1), z(B, 1)], z(B), z(B)
            self.out = [z(B, 1), z(B, 1)]
            self.ws = [torch.empty(eng.mlp_workspace(B, widths, True), dtype=torch.uint8, device="cuda") for _ in range(2)]
            self.bws = [torch.empty(eng.mlp_backward_workspace(B, widths), dtype=torch.uint8, device="cuda") for _ in range(2)]
            self.tdws = eng.td_loss_workspace(B)
            self.td = None
            self.opt = DeviceOptimizer(eng, params, kind="adam", lr=1e-3, max_grad_norm=0.5)

        def load(self, k):
            rng = np.random.default_rng(2000 + k)
            f = lambda *s: _t(rng.standard_normal(s).astype(np.float32))
            self.obs.copy_(f(B, F))
            self.act.copy_(f(B, 1))
            self.nq[0].copy_(f(B, 1))
            self.nq[1].copy_(f(B, 1))
            self.rew.copy_(f(B))
            self.done.copy_(_t((rng.random(B) < 0.2).astype(np.float32)))

        def __call__(self):
            if self.grouped:
                eng.mlp_group_forward(self.obs, self.w, self.b, x2s=[self.act, self.act], outs=self.out, workspaces=self.ws, keep_hidden=True)
            else:
                for k in range(2):
                    eng.mlp_forward(self.obs, self.w[k], self.b[k], x2=self.act, out=self.out[k], workspace=self.ws[k], keep_hidden=True)
            self.td = eng.td_loss("td3", self.out, self.nq, self.rew, self.done, 0.97, out=self.td, workspace=self.tdws)
            gq = list(self.td.grad_q)
            if self.grouped:
                eng.mlp_group_backward(gq, self.obs, self.w, self.b, self.out, self.ws, x2s=[self.act, self.act], grad_weights=self.gw, grad_biases=self.gb,
                                       backward_workspaces=self.bws)
            else:
                for k in range(2):
                    eng.mlp_backward(gq[k], self.obs, self.w[k], self.b[k], self.out[k], self.ws[k], x2=self.act, grad_weights=self.gw[k], grad_biases=self.gb[k],
                                     backward_workspace=self.bws[k])
            self.opt.step()

    cap, twin = Step(True), Step(False)
    for s in (cap, twin):                                    # one eager step each: code objects loaded, the optimiser's tables built
        s.load(0)
        s()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    params = lambda s: [p for net in s.nets for p in net.parameters()]
    before = [_h(p).copy() for p in params(cap)]
    for k in (1, 2, 3):
        cap.load(k)
        graph.replay()
        twin.load(k)
        twin()
        torch.cuda.synchronize()
        for p, q in zip(params(cap), params(twin)):
            assert np.array_equal(_h(p).view(np.int32), _h(q).view(np.int32)), k
    assert all(not np.array_equal(a, _h(p)) for a, p in zip(before, params(cap)))
    eng.sync()


# ------------------------------------------------------------------------------------------------- runtime guarantees
def test_no_host_synchronisation_and_no_allocation():
    """tests/test_mlp_backward.py's condition for a grouped forward + backward: the stream is busy with fused steps before the calls and
    still busy when they have returned; with every output and workspace given, the allocator hands out nothing during them"""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    B, widths = 257, [[64, 33, 5], [17, 40, 1]]
    cs = [tb._case(1 + i, B, 40, w) for i, w in enumerate(widths)]
    xd = _t(cs[0][0])
    wd, bd, gd = [[_t(w) for w in c[1]] for c in cs], [[_t(b) for b in c[2]] for c in cs], [_t(c[3]) for c in cs]
    outs = [torch.empty((B, w[-1]), device="cuda") for w in widths]
    works = [torch.empty(eng.mlp_workspace(B, w, True), dtype=torch.uint8, device="cuda") for w in widths]
    bws = [torch.empty(eng.mlp_backward_workspace(B, w), dtype=torch.uint8, device="cuda") for w in widths]
    gw, gb, gx = [[torch.empty_like(w) for w in ws] for ws in wd], [[torch.empty_like(b) for b in bs] for bs in bd], [torch.empty_like(xd) for _ in widths]

    def op():
        eng.mlp_group_forward(xd, wd, bd, outs=outs, workspaces=works, keep_hidden=True)
        eng.mlp_group_backward(gd, xd, wd, bd, outs, works, grad_weights=gw, grad_biases=gb, grad_xs=gx, backward_workspaces=bws)

    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                        # warm: first-launch work is not part of the condition
    op()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    op()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: they waited for the device"
    assert allocs_after == allocs, "calls with every output and workspace given allocated device memory"
    eng.sync()
    eng.close()


def test_refused_descriptor_groups_enqueue_nothing():
    """every refusal of the C ABI with a real handle: the counts, a faulty descriptor in a non-first place (the single call's words behind
    "net i: "), PTG_MLP_WIDE, and a disagreement in each field the launches share.  The stream stays idle and every output and workspace
    of every network keeps its fill.  Every call here is refused on the host before a launch"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, G = 20, 3
    L, h, stream = eng._L, eng._h, eng._stream()
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    need, needb = eng.mlp_workspace(B, [8, 8, 5], True), eng.mlp_backward_workspace(B, [8, 8, 5])
    x, x2, gout = full(B, 42), full(B, 2), full(B, 6)                                  # read-only: shared
    w, b = [full(8, 44), full(8, 8), full(5, 8)], [full(8), full(8), full(5)]
    T = [dict(out=full(B, 6), gw=[full(8, 44), full(8, 8), full(5, 8)], gb=[full(8), full(8), full(5)], gx=full(B, 42), gx2=full(B, 2),
              ws=torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda"), bws=torch.full((needb + 8,), 0x5A, dtype=torch.uint8, device="cuda")) for _ in range(G)]
    torch.cuda.synchronize()

    def fill(d, a):
        for k, v in a.items():
            if isinstance(v, (list, tuple)):
                for j, e in enumerate(v):
                    getattr(d, k)[j] = e
            else:
                setattr(d, k, v)

    def group(edits=None, n=G):
        """the good group of n networks; edits: {network: (forward fields, backward fields)}"""
        arr = (_lib.PtgMlpBwd * max(n, 1))()
        for i in range(n):
            t = T[i % G]
            f = dict(batch=B, n_layers=3, flags=_lib.MLP_KEEP_HIDDEN, hidden_act=_lib.MLP_TANH, out_act=_lib.MLP_TANH, f1=40, f2=1, x_dev=p(x), x_s_n=42, x2_dev=p(x2), x2_s_n=2,
                     w_dev=[p(v) for v in w], w_s_n=[44, 8, 8], b_dev=[p(v) for v in b], width=[8, 8, 5], out_dev=p(t["out"]), out_s_n=6, ws_dev=p(t["ws"]), ws_bytes=need)
            a = dict(gout_dev=p(gout), gout_s_n=6, dw_dev=[p(v) for v in t["gw"]], dw_s_n=[44, 8, 8], db_dev=[p(v) for v in t["gb"]], dx_dev=p(t["gx"]), dx_s_n=42,
                     dx2_dev=p(t["gx2"]), dx2_s_n=2, bws_dev=p(t["bws"]), bws_bytes=needb, flags=0)
            fe, be = (edits or {}).get(i, ({}, {}))
            f.update(fe)
            a.update(be)
            fill(arr[i].fwd, f)
            fill(arr[i], a)
        return arr

    def both(arr, n):
        """(return code and text of the backward, of the forward on the embedded descriptors)"""
        rb = L.ptg_mlp_group_backward(h, arr, n, stream)
        wb = L.ptg_last_error(h).decode()
        fw = (_lib.PtgMlp * len(arr))(*[e.fwd for e in arr])
        rf = L.ptg_mlp_group_forward(h, fw, n, stream)
        return rb, wb, rf, L.ptg_last_error(h).decode()

    E = _lib.E_INVALID
    for n in (0, 9, -1):                                      # the counts
        rb, wb, rf, wf = both(group(n=9), n)
        assert rb == E and rf == E and "n_nets" in wb and "n_nets" in wf, n
    assert L.ptg_mlp_group_backward(h, None, 2, stream) == E and L.ptg_mlp_group_forward(h, None, 2, stream) == E
    assert L.ptg_mlp_group_backward(None, group(), G, stream) == E and L.ptg_mlp_group_forward(None, (_lib.PtgMlp * G)(), G, stream) == E
    K = _lib.MLP_KEEP_HIDDEN
    # a faulty descriptor in place 1 or 2: the single call's words behind "net i: "
    fwd_faults = [dict(batch=0), dict(n_layers=11), dict(flags=K | 8), dict(flags=K | _lib.MLP_NARROW | _lib.MLP_WIDE), dict(hidden_act=2), dict(out_act=3), dict(f1=0), dict(x_dev=None),
                  dict(x_s_n=39), dict(x2_dev=None), dict(w_dev=[p(w[0]), None, p(w[2])]), dict(w_s_n=[40, 8, 8]), dict(width=[8, 0, 5]), dict(out_dev=None), dict(out_s_n=4),
                  dict(ws_dev=p(T[1]["ws"], 2)), dict(ws_bytes=need - 1)]
    for k, fe in enumerate(fwd_faults):
        i = 1 + k % 2
        arr = group({i: (fe, {})})
        rb, wb, rf, wf = both(arr, G)
        assert L.ptg_mlp_forward(h, C.byref(arr[i].fwd), stream) == E, k
        single = L.ptg_last_error(h).decode()
        assert single.startswith("ptg_mlp_forward: ")
        assert rf == E and wf == f"ptg_mlp_group_forward: net {i}: " + single[len("ptg_mlp_forward: "):], (k, wf, single)
        assert rb == E and wb == f"ptg_mlp_group_backward: net {i}: the forward's descriptor: " + single[len("ptg_mlp_forward: "):], (k, wb, single)
    bwd_faults = [({}, dict(gout_dev=None)), ({}, dict(gout_s_n=4)), ({}, dict(dw_dev=[p(T[1]["gw"][0]), None, p(T[1]["gw"][2])])), ({}, dict(dw_s_n=[40, 8, 8])), ({}, dict(dx_s_n=39)),
                  ({}, dict(dx2_s_n=0)), (dict(f2=0, x2_dev=None, w_s_n=[40, 8, 8]), {}), ({}, dict(bws_dev=None)), ({}, dict(bws_bytes=needb - 1)), ({}, dict(flags=16)),
                  (dict(flags=0), {})]
    for k, (fe, be) in enumerate(bwd_faults):
        i = 1 + k % 2
        arr = group({i: (fe, be)})
        assert L.ptg_mlp_group_backward(h, arr, G, stream) == E, k
        wb = L.ptg_last_error(h).decode()
        assert L.ptg_mlp_backward(h, C.byref(arr[i]), stream) == E, k
        single = L.ptg_last_error(h).decode()
        assert wb == f"ptg_mlp_group_backward: net {i}: " + single[len("ptg_mlp_backward: "):], (k, wb, single)
    # PTG_MLP_WIDE, and the fields that must agree: the text names the two networks and the field
    narrow = {i: (dict(flags=K | _lib.MLP_NARROW), {}) for i in range(G)}
    for k, (edits, words) in enumerate([({1: (dict(flags=K | _lib.MLP_WIDE), {})}, ("net 1", "PTG_MLP_WIDE")), ({i: (dict(flags=K | _lib.MLP_WIDE), {}) for i in range(G)}, ("net 0", "PTG_MLP_WIDE")),
                                        ({2: (dict(batch=B - 1), {})}, ("nets 0 and 2", "batch")), ({1: (dict(n_layers=2, width=[8, 5, 0], w_s_n=[44, 8, 0]), {})}, ("nets 0 and 1", "n_layers")),
                                        ({1: (dict(hidden_act=_lib.MLP_RELU), {})}, ("nets 0 and 1", "hidden_act")), ({2: (dict(out_act=_lib.MLP_NONE), {})}, ("nets 0 and 2", "out_act")),
                                        ({1: (dict(flags=K | _lib.MLP_NARROW), {})}, ("nets 0 and 1", "flags"))]):
        rb, wb, rf, wf = both(group(edits), G)
        assert rb == E and rf == E and all(s in wb for s in words) and all(s in wf for s in words), (k, wb, wf)
    assert L.ptg_mlp_group_backward(h, group({2: ({}, dict(flags=_lib.MLP_ACCUMULATE))}), G, stream) == E
    why = L.ptg_last_error(h).decode()
    assert "nets 0 and 2" in why and "flags" in why
    assert torch.cuda.current_stream().query() is True        # nothing was enqueued
    torch.cuda.synchronize()
    for t in T:
        assert all(bool((v == SENTINEL).all()) for v in t["gw"] + t["gb"] + [t["gx"], t["gx2"], t["out"]]) and bool((t["bws"] == 0x5A).all()) and bool((t["ws"] == 0x5A).all())
    # the good group, PTG_MLP_NARROW in every descriptor (accepted, means nothing), the forward first
    good = group(narrow)
    fw = (_lib.PtgMlp * G)(*[e.fwd for e in good])
    assert L.ptg_mlp_group_forward(h, fw, G, stream) == 0 and L.ptg_mlp_group_backward(h, good, G, stream) == 0
    eng.sync()
    for t in T:
        assert bool((t["gw"][0][:, :41] != SENTINEL).all()) and bool((t["gw"][0][:, 41:] == SENTINEL).all()) and bool((t["gx"][:, :40] != SENTINEL).all())
        assert bool((t["gx"][:, 40:] == SENTINEL).all()) and bool((t["out"][:, :5] != SENTINEL).all()) and bool((t["out"][:, 5] == SENTINEL).all())
        assert torch.equal(t["out"], T[0]["out"]) and torch.equal(t["gw"][1], T[0]["gw"][1]) and bool((t["bws"][needb:] == 0x5A).all())
