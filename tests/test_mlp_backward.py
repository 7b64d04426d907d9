"""ptg_mlp_backward, HipEngine.mlp_backward and rl_ptg_amd.TrainMLP (include/ptg_env.h) against the NumPy restatement
(tests/mlp_backward_restatement.py, pinned against float64 sums and nets by hand in tests/test_mlp_backward_host.py).

What is compared, and how.
  bit for bit, through integer views with +0 == -0 (mlp_restatement.same_bits): dx, every dW, every db and the dz the call leaves in its
    workspace, the restatement FED THE OP'S OWN kept hidden layers and output (the forward has its own tests), so that a tanh of another
    library or a ReLU unit next to 0 cannot enter.  This rests on v_mfma_f32_16x16x4_f32 being an ordered fmaf chain from its C operand
    (DESIGN.md sections 18 and 19); the lane-map tests with exact integers come first and do not rest on it.
  dz: the two alternating buffers keep dz of layers 0 and 1.  The dz of a deeper layer l is read through a second call on the top of the
    net (layers l .., fed the kept hidden layer l - 1): by the row rule its dz_0 has the bits of the whole net's dz_l.  The 10-layer test
    does that for every layer; everywhere else a wrong dz_l shows in dW_l and db_l, which are chains over it.
  against float64: no fixed tolerance; torch's own float32 CPU autograd on the same inputs is the yardstick, the op may deviate from the
    float64 result at most 4 times as far (both figures are printed).  The integrated steps use the same rule on their own chain: the
    nn.Sequential chain in float64 is the reference, the nn.Sequential chain in float32 the yardstick.

The grid is thinned diagonally as tests/test_mlp.py's is: at every B all ten (fan-in, out) pairs are run, and the depth (1, 2, 3: d % 3), the
strided layout with guards ((d + 1) % 5 < 2), the two-piece input (d % 7 < 3) and the hidden activation's companion -- out_act NONE
throughout, as the issue sets -- walk diagonally, d = B's position + the pair's; 3, 5 and 7 are pairwise co-prime."""
import ctypes as C

import numpy as np
import pytest

import mlp_backward_restatement as br
import mlp_restatement as mr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
BS = [1, 6, 15, 16, 17, 31, 32, 33, 65, 129]
PAIRS = [(1, 1), (2, 3), (3, 5), (4, 16), (5, 17), (40, 64), (41, 33), (31, 233), (233, 37), (63, 129)]
_engines = {}
_spec = []
_yard = {}


def _engine(n=64):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    _engines[n] = eng
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(t):
    return t.detach().cpu().numpy()


def _pitch(w):
    return (w + 3) // 4 * 4


def _widths(fi, out, n):
    return [out if l % 2 == 0 else fi for l in range(n)]


def _case(seed, B, fi, widths):
    rng = np.random.default_rng(seed)
    ws, bs = mr.net(rng, fi, widths, scale=1.5)
    x = rng.standard_normal((B, fi)).astype(np.float32)
    gout = rng.standard_normal((B, widths[-1])).astype(np.float32)
    return x, ws, bs, gout


def _guarded(rows, cols, init=None, strided=True):
    """a [rows, cols] tensor of sentinels (or init) -- strided: inside a [rows + 2, cols + 3] tensor of sentinels.  Returns (view, frame)"""
    import torch
    g = torch.full((rows + 2, cols + 3), SENTINEL, device="cuda") if strided else torch.full((rows, cols), SENTINEL, device="cuda")
    v = g[1:rows + 1, 1:cols + 1] if strided else g
    if init is not None:
        v.copy_(_t(init))
    return v, g


def _frame_intact(view_shape, g, strided):
    if not strided:
        return True
    m = np.ones(g.shape, bool)
    m[1:view_shape[0] + 1, 1:view_shape[1] + 1] = False
    return bool((_h(g)[m] == SENTINEL).all())


def _strided_in(x, lead=2, tail=3):
    import torch
    w = torch.full((x.shape[0], lead + x.shape[1] + tail), SENTINEL, device="cuda")
    w[:, lead:lead + x.shape[1]] = _t(x)
    return w[:, lead:lead + x.shape[1]]


def _run(eng, x, ws, bs, gout, hidden_act="relu", out_act=None, f1=None, strided=False, params=True, frozen=(), want_dx=True, want_dx2=True,
         init_w=None, init_b=None, accumulate=False):
    """mlp_forward(keep_hidden) and mlp_backward on host arrays.  f1: the input goes in as two pieces split there.  Returns a dict of host
    arrays -- out, hidden, dx (the pieces joined; None when neither was asked for), dws, dbs (None entries for frozen layers), dz (what the
    workspace keeps: {layer: array}) -- and ok: guards, frozen gradients, pad columns, the workspace tails, the forward's workspace and the
    output are untouched by the backward"""
    import torch
    B, K0 = x.shape
    n, widths = len(ws), [w.shape[0] for w in ws]
    si = _strided_in if strided else (lambda a, *_: _t(a))
    xd = si(x if f1 is None else x[:, :f1])
    x2d = None if f1 is None else si(x[:, f1:], 1, 1)
    wd, bd = [si(w, 0, 5) for w in ws], [_t(b) for b in bs]
    need_f, need_b = eng.mlp_workspace(B, widths, True), eng.mlp_backward_workspace(B, widths)
    work = torch.full((need_f + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    fwd = eng.mlp_forward(xd, wd, bd, hidden_activation=hidden_act, out_activation=out_act, x2=x2d, workspace=work[:need_f], keep_hidden=True)
    eng.sync()
    work_before, out_before = work.clone(), fwd.out.clone()
    gd = si(gout, 1, 2)
    fans = [K0] + widths[:-1]
    gw, gb, frames = None, None, []
    if params:
        gw, gb = [], []
        for l in range(n):
            if l in frozen:
                gw.append(None)
                gb.append(None)
                frames.append(None)
                continue
            v, g = _guarded(widths[l], fans[l], None if init_w is None else init_w[l], strided)
            bv, bg = _guarded(1, widths[l], None if init_b is None else init_b[l][None, :], True)
            gw.append(v)
            gb.append(bv[0])
            frames.append((v.shape, g, bg))
    F1 = K0 if f1 is None else f1
    gx, gxf = _guarded(B, F1, None, strided) if want_dx else (None, None)
    gx2, gx2f = _guarded(B, K0 - F1, None, strided) if (f1 is not None and want_dx2) else (None, None)
    bws = torch.full((need_b + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    ret = eng.mlp_backward(gd, xd, wd, bd, fwd.out, work[:need_f], hidden_activation=hidden_act, out_activation=out_act, x2=x2d, grad_weights=gw, grad_biases=gb,
                           grad_x=gx, grad_x2=gx2, backward_workspace=bws[:need_b], accumulate=accumulate)
    eng.sync()
    ok = ret.data_ptr() == bws.data_ptr() and bool((work == work_before).all()) and bool(torch.equal(fwd.out, out_before)) and bool((bws[need_b:] == 0x5A).all())
    for fr in frames:
        if fr is not None:
            ok = ok and _frame_intact(fr[0], fr[1], strided) and _frame_intact((1, fr[2].shape[1] - 3), fr[2], True)
    ok = ok and (gx is None or _frame_intact((B, F1), gxf, strided)) and (gx2 is None or _frame_intact((B, K0 - F1), gx2f, strided))
    # the dz buffers: layer l is stored when it is hidden, or the last one under an output activation, and left when l < 2 ... unless the
    # chain stopped above it (no dx asked for and l = 0 is the input: dz_0 is still needed for dW_0, so it is always there)
    Pw = max(_pitch(w) for w in widths)
    may = np.zeros(need_b // 4, bool)
    dz = {}
    flat = bws[:need_b].view(torch.float32)
    for l in range(n):
        if l < n - 1 or out_act is not None:
            P = _pitch(widths[l])
            idx = (l & 1) * B * Pw + (np.arange(B)[:, None] * P + np.arange(widths[l])[None, :])
            may[idx.ravel()] = True
            if l < 2:
                dz[l] = _h(flat)[idx]
    ok = ok and bool((_h(bws[:need_b]).reshape(-1, 4)[~may] == 0x5A).all())
    dx = None
    if gx is not None or gx2 is not None:
        dx = np.full((B, K0), np.nan, np.float32)
        if gx is not None:
            dx[:, :F1] = _h(gx)
        if gx2 is not None:
            dx[:, F1:] = _h(gx2)
    return dict(out=_h(fwd.out), hidden=[_h(t) for t in fwd.hidden], dx=dx, dws=None if gw is None else [None if t is None else _h(t) for t in gw],
                dbs=None if gb is None else [None if t is None else _h(t) for t in gb], dz=dz, ok=ok, has_dx=gx is not None, has_dx2=gx2 is not None, F1=F1)


def _ref(r, x, ws, gout, hidden_act="relu", out_act=None, **kw):
    return br.backward(gout, x, ws, r["hidden"], r["out"], hidden_act=hidden_act, out_act=out_act, **kw)


def _same_as_ref(r, ref, what=""):
    dx, dws, dbs, dzs = ref
    assert r["ok"], f"{what}: a guard, a frozen gradient, a pad column, a workspace tail, the forward's workspace or the output was written"
    if r["dx"] is not None:
        cols = np.r_[0:r["F1"] if r["has_dx"] else 0, r["F1"] if r["has_dx2"] else dx.shape[1]:dx.shape[1]].astype(int)
        assert mr.same_bits(r["dx"][:, cols], dx[:, cols]), (what, "dx", float(np.nanmax(np.abs(r["dx"][:, cols] - dx[:, cols]))))
    if r["dws"] is not None:
        for l, (w, b) in enumerate(zip(r["dws"], r["dbs"])):
            if w is not None:
                assert mr.same_bits(w, dws[l]), (what, "dW", l, float(np.nanmax(np.abs(w - dws[l]))))
                assert mr.same_bits(b, dbs[l]), (what, "db", l, float(np.nanmax(np.abs(b - dbs[l]))))
    for l, z in r["dz"].items():
        assert mr.same_bits(z, dzs[l]), (what, "dz", l)


# ------------------------------------------------------------------------------------------------- the lane maps, with exact integers
def _asym(O, K):
    W = ((3 * np.arange(O)[:, None] + 5 * np.arange(K)[None, :]) % 11 - 4 + (np.arange(O)[:, None] > np.arange(K)[None, :])).astype(np.int64)
    m = min(O, K)
    assert m < 2 or not np.array_equal(W[:m, :m], W[:m, :m].T)
    return W


@pytest.mark.parametrize("B,K,O", [(13, 11, 9), (37, 19, 45), (70, 70, 50)])
def test_the_lane_maps_with_exact_integer_data(B, K, O):
    """one-layer nets without activation, small integers: every partial sum is exact, the order cannot matter, an int64 matmul is the
    reference -- a swapped index or a wrong lane map shows whatever the numerics.  dz = I reads W back through k_mlp_dx; x = I reads dz^T
    through k_mlp_dw (and db = the row sums of dz^T); then random small integers, one tile (13, 11, 9) and several"""
    eng = _engine()
    rng = np.random.default_rng(5)
    W = _asym(O, K)
    f = lambda a: a.astype(np.float32)
    zb = np.zeros(O, np.float32)
    r = _run(eng, f(rng.integers(-3, 4, (O, K))), [f(W)], [zb], f(np.eye(O, dtype=np.int64)))                   # B = O rows, dz = I: dx = W
    assert r["ok"] and np.array_equal(r["dx"].astype(np.int64), W)
    G = _asym(K, O)                                                                                            # [K rows][O]: dz, asymmetric
    r = _run(eng, f(np.eye(K, dtype=np.int64)), [f(W)], [zb], f(G))                                             # B = K rows, x = I: dW = dz^T
    assert r["ok"] and np.array_equal(r["dws"][0].astype(np.int64), G.T) and np.array_equal(r["dbs"][0].astype(np.int64), G.sum(0))
    x, g = rng.integers(-3, 4, (B, K)), rng.integers(-3, 4, (B, O))
    for strided in (False, True):
        r = _run(eng, f(x), [f(W)], [zb], f(g), strided=strided, f1=K // 2 if strided else None)
        assert r["ok"] and np.array_equal(r["dx"].astype(np.int64), g @ W)
        assert np.array_equal(r["dws"][0].astype(np.int64), g.T @ x) and np.array_equal(r["dbs"][0].astype(np.int64), g.sum(0))
    # two layers with a ReLU between: the epilogue's select and the second buffer
    W2 = rng.integers(-2, 3, (7, O))
    g2 = rng.integers(-3, 4, (B, 7))
    b1 = rng.integers(-9, 10, O)
    r = _run(eng, f(x), [f(W), f(W2)], [f(b1), np.zeros(7, np.float32)], f(g2))
    hid = np.maximum(x @ W.T + b1, 0)
    dz0 = (g2 @ W2) * (hid > 0)
    assert r["ok"] and np.array_equal(r["hidden"][0].astype(np.int64), hid) and np.array_equal(r["dz"][0].astype(np.int64), dz0)
    assert np.array_equal(r["dws"][1].astype(np.int64), g2.T @ hid) and np.array_equal(r["dws"][0].astype(np.int64), dz0.T @ x)
    assert np.array_equal(r["dbs"][0].astype(np.int64), dz0.sum(0)) and np.array_equal(r["dx"].astype(np.int64), dz0 @ W)


# ------------------------------------------------------------------------------------------------- bit for bit over the grid
@pytest.mark.parametrize("B", BS)
def test_relu_nets_bit_for_bit_over_the_grid(B):
    eng = _engine()
    ib = BS.index(B)
    for ip, (fi, out) in enumerate(PAIRS):
        d = ib + ip
        widths = _widths(fi, out, 1 + d % 3)
        x, ws, bs, gout = _case(100 * ib + ip, B, fi, widths)
        f1 = fi // 2 if fi >= 2 and d % 7 < 3 else None
        r = _run(eng, x, ws, bs, gout, strided=(d + 1) % 5 < 2, f1=f1)
        _same_as_ref(r, _ref(r, x, ws, gout), (B, fi, widths))


def test_a_ten_layer_net_and_every_dz_of_it():
    eng = _engine()
    B, fi = 17, 31
    widths = [33, 17, 40, 5, 64, 3, 37, 16, 9, 6]
    x, ws, bs, gout = _case(77, B, fi, widths)
    r = _run(eng, x, ws, bs, gout)
    ref = _ref(r, x, ws, gout)
    _same_as_ref(r, ref, "ten layers")
    for l in range(2, 10):                                   # dz_l of the whole net = dz_0 of the net's top, fed the kept hidden layer l - 1
        top = _run(eng, r["hidden"][l - 1], ws[l:], bs[l:], gout, want_dx=False)
        assert top["ok"] and mr.same_bits(top["out"], r["out"])
        if l < 9:
            assert mr.same_bits(top["dz"][0], ref[3][l]), l
        assert mr.same_bits(top["dws"][0], ref[1][l]) and mr.same_bits(top["dbs"][0], ref[2][l])


def test_the_widest_net():
    """1024 -> 1024 -> 5 at B = 17: the limits of fan-in and width, 64 x 65 tiles of k_mlp_dw and 64 column tiles of k_mlp_dx"""
    eng = _engine()
    x, ws, bs, gout = _case(11, 17, 1024, [1024, 5])
    r = _run(eng, x, ws, bs, gout)
    _same_as_ref(r, _ref(r, x, ws, gout), "1024")


RING = [1, 31, 32, 33, 64, 65, 128, 129, 160, 257]           # chunks of 32: below, at, one above and at twice the ring depths 2 and 4, with and without a ragged last chunk


@pytest.mark.parametrize("R", RING)
@pytest.mark.parametrize("kernel", ["dx", "dw"])
def test_the_ring_at_its_edges(kernel, R):
    """the reduction length at the edges of the chunk ring: the upper layer's O in k_mlp_dx (four chunks in flight), B in k_mlp_dw (two);
    the other dimensions 17: two tiles, one ragged.  Strided, in guard frames"""
    B, widths = (17, [17, R]) if kernel == "dx" else (R, [17, 17])
    x, ws, bs, gout = _case(9000 + R, B, 17, widths)
    r = _run(_engine(), x, ws, bs, gout, strided=True)
    _same_as_ref(r, _ref(r, x, ws, gout), (kernel, R))


def test_a_reduction_over_several_chunks_of_rows():
    """B = 257: nine chunks of 32 rows, so the ring of four chunks in flight wraps twice and the last chunk holds one row"""
    eng = _engine()
    x, ws, bs, gout = _case(12, 257, 41, [33, 17, 5])
    r = _run(eng, x, ws, bs, gout, f1=40, strided=True)
    _same_as_ref(r, _ref(r, x, ws, gout), "B = 257")


# ------------------------------------------------------------------------------------------------- tanh
@pytest.mark.parametrize("B,fi,widths,hidden_act,out_act", [(33, 41, [33, 17, 5], "tanh", None), (65, 40, [64, 37, 1], "relu", "tanh"), (6, 31, [233, 33, 2], "tanh", "tanh"),
                                                           (17, 5, [17, 17, 3], "relu", "relu")])
def test_tanh_nets_hidden_and_output(B, fi, widths, hidden_act, out_act):
    """the chains bit for bit, and dz bit for bit against the three-rounding restatement on the op's own h: dz_0 and dz_1 from the
    workspace, and -- with an output activation -- the last layer's through a one-layer call"""
    eng = _engine()
    x, ws, bs, gout = _case(B + fi, B, fi, widths)
    x *= 2.0
    r = _run(eng, x, ws, bs, gout, hidden_act=hidden_act, out_act=out_act)
    ref = _ref(r, x, ws, gout, hidden_act=hidden_act, out_act=out_act)
    _same_as_ref(r, ref, (B, fi, widths, hidden_act, out_act))
    assert mr.same_bits(r["dz"][0], br.dact(r["hidden"][0], br.dx_chain(r["dz"][1], ws[1]), hidden_act))
    if out_act is not None:
        one = _run(eng, r["hidden"][-1], ws[-1:], bs[-1:], gout, out_act=out_act)
        assert one["ok"] and mr.same_bits(one["out"], r["out"]) and mr.same_bits(one["dz"][0], br.dact(r["out"], gout, out_act))
        assert mr.same_bits(one["dz"][0], ref[3][-1])


# ------------------------------------------------------------------------------------------------- optional and two-piece outputs
@pytest.mark.parametrize("f1", [1, 15, 17])
def test_two_piece_dx_against_the_one_piece_result(f1):
    eng = _engine()
    B, fi, widths = 33, 41, [33, 9, 2]
    x, ws, bs, gout = _case(f1, B, fi, widths)
    whole = _run(eng, x, ws, bs, gout)
    _same_as_ref(whole, _ref(whole, x, ws, gout), "one piece")
    for strided in (False, True):
        split = _run(eng, x, ws, bs, gout, f1=f1, strided=strided)
        assert split["ok"] and np.array_equal(split["dx"].view(np.int32), whole["dx"].view(np.int32))
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(split["dws"] + split["dbs"], whole["dws"] + whole["dbs"]))
    only1 = _run(eng, x, ws, bs, gout, f1=f1, want_dx2=False, strided=True)
    only2 = _run(eng, x, ws, bs, gout, f1=f1, want_dx=False, strided=True)
    none = _run(eng, x, ws, bs, gout, f1=f1, want_dx=False, want_dx2=False)
    assert only1["ok"] and only2["ok"] and none["ok"] and none["dx"] is None
    assert np.array_equal(only1["dx"][:, :f1].view(np.int32), whole["dx"][:, :f1].view(np.int32)) and np.isnan(only1["dx"][:, f1:]).all()
    assert np.array_equal(only2["dx"][:, f1:].view(np.int32), whole["dx"][:, f1:].view(np.int32)) and np.isnan(only2["dx"][:, :f1]).all()
    for r in (only1, only2, none):
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(r["dws"] + r["dbs"], whole["dws"] + whole["dbs"]))


def test_parameter_gradients_off_and_one_frozen_layer():
    eng = _engine()
    x, ws, bs, gout = _case(40, 33, 40, [37, 17, 5])
    whole = _run(eng, x, ws, bs, gout)
    off = _run(eng, x, ws, bs, gout, params=False, f1=39, want_dx=False, strided=True)         # a critic inside an actor loss: the action's gradient alone
    assert off["ok"] and off["dws"] is None and np.array_equal(off["dx"][:, 39:].view(np.int32), whole["dx"][:, 39:].view(np.int32))
    for frozen in (0, 1, 2):
        r = _run(eng, x, ws, bs, gout, frozen=(frozen,), strided=frozen == 1)
        assert r["ok"] and r["dws"][frozen] is None and np.array_equal(r["dx"].view(np.int32), whole["dx"].view(np.int32))
        for l in range(3):
            if l != frozen:
                assert np.array_equal(r["dws"][l].view(np.int32), whole["dws"][l].view(np.int32)) and np.array_equal(r["dbs"][l].view(np.int32), whole["dbs"][l].view(np.int32))


# ------------------------------------------------------------------------------------------------- batch and accumulation
def test_a_row_of_dx_does_not_depend_on_the_batch_and_a_split_call_accumulates_exactly():
    eng = _engine()
    B = 129
    x, ws, bs, gout = _case(3, B, 40, [64, 33, 5])
    full = _run(eng, x, ws, bs, gout)
    ref = _ref(full, x, ws, gout)
    _same_as_ref(full, ref, "B = 129")
    for b in (0, 1, 15, 16, 17, 64, 127, 128):
        one = _run(eng, x[b:b + 1], ws, bs, gout[b:b + 1])
        assert one["ok"] and np.array_equal(one["dx"].view(np.int32), full["dx"][b:b + 1].view(np.int32)), b
    part = _run(eng, x[50:81], ws, bs, gout[50:81])
    assert np.array_equal(part["dx"].view(np.int32), full["dx"][50:81].view(np.int32))
    # 65 rows, then the next 64 accumulating: the bits of one call on 129, all dW and db
    first = _run(eng, x[:65], ws, bs, gout[:65])
    second = _run(eng, x[65:], ws, bs, gout[65:], init_w=first["dws"], init_b=first["dbs"], accumulate=True, strided=True)
    assert first["ok"] and second["ok"]
    for l in range(3):
        assert mr.same_bits(second["dws"][l], full["dws"][l]) and mr.same_bits(second["dbs"][l], full["dbs"][l]), l
    # and onto a gradient that is not a chain's head: against the restatement
    rng = np.random.default_rng(9)
    iw = [rng.standard_normal(w.shape).astype(np.float32) for w in ws]
    ib = [rng.standard_normal(b.shape).astype(np.float32) for b in bs]
    acc = _run(eng, x[:33], ws, bs, gout[:33], init_w=iw, init_b=ib, accumulate=True)
    _same_as_ref(acc, _ref(acc, x[:33], ws, gout[:33], init_w=iw, init_b=ib), "accumulate")
    plain = _run(eng, x[:33], ws, bs, gout[:33], init_w=iw, init_b=ib)                       # without the flag what was there is overwritten
    _same_as_ref(plain, _ref(plain, x[:33], ws, gout[:33]), "overwrite")


# ------------------------------------------------------------------------------------------------- planted values
def test_planted_values():
    """a NaN row and an Inf row in gout stay in their rows of dx and reach the dW / db the restatement says; subnormal products; -0"""
    eng = _engine()
    B = 70
    x, ws, bs, gout = _case(9, B, 41, [33, 5])
    clean = _run(eng, x, ws, bs, gout)
    bad = gout.copy()
    bad[20, 2] = np.nan
    bad[66, :] = np.inf
    r = _run(eng, x, ws, bs, bad)
    ref = _ref(r, x, ws, bad)
    _same_as_ref(r, ref, "planted")
    rest = np.ones(B, bool)
    rest[[20, 66]] = False
    assert np.array_equal(r["dx"][rest].view(np.int32), clean["dx"][rest].view(np.int32)) and np.isfinite(r["dx"][rest]).all()
    assert not np.isfinite(r["dx"][20]).any() and not np.isfinite(r["dx"][66]).any()
    assert np.isnan(r["dws"][1][2]).all() and not np.isfinite(r["dbs"][1]).any() and np.isnan(ref[1][1][2]).all()
    # a dead ReLU unit under the NaN row gives dz = 0 there: the select
    dead = r["hidden"][0][20] <= 0
    assert dead.any() and (r["dz"][0][20][dead] == 0).all() and np.isnan(r["dz"][0][20][~dead]).all()
    rng = np.random.default_rng(2)
    K, O = 23, 19
    tiny_x = (rng.integers(1, 8, (B, K)) * 2.0 ** -70).astype(np.float32)
    tiny_g = (rng.integers(-7, 8, (B, O)) * 2.0 ** -70).astype(np.float32)
    tiny_w = (rng.integers(-7, 8, (O, K)) * 2.0 ** -70).astype(np.float32)
    tiny_g[5] = -0.0
    r = _run(eng, tiny_x, [tiny_w], [np.zeros(O, np.float32)], tiny_g)
    ref = _ref(r, tiny_x, [tiny_w], tiny_g)
    _same_as_ref(r, ref, "subnormal")
    assert (np.abs(ref[1][0]) < 2.0 ** -126).all() and (ref[1][0] != 0).sum() > O * K // 2 and (ref[0] != 0).sum() > B * K // 2      # un-flushed
    assert (r["dx"][5] == 0).all()


# ------------------------------------------------------------------------------------------------- against float64
def _f64_backward(x, ws, bs, gout, hidden, hidden_act):
    """float64 forward and backward; the ReLU mask is taken from the op's float32 hidden layers"""
    f = lambda a: np.asarray(a, np.float64)
    hs, h = [f(x)], f(x)
    n = len(ws)
    for l in range(n - 1):
        z = h @ f(ws[l]).T + f(bs[l])
        h = np.tanh(z) if hidden_act == "tanh" else np.where(hidden[l] > 0, z, 0.0)
        hs.append(h)
    dz, dws, dbs = f(gout), [None] * n, [None] * n
    for l in range(n - 1, -1, -1):
        dws[l], dbs[l] = dz.T @ hs[l], dz.sum(0)
        g = dz @ f(ws[l])
        if l:
            dz = g * (1 - hs[l] ** 2) if hidden_act == "tanh" else np.where(hidden[l - 1] > 0, g, 0.0)
    return [g] + dws + dbs


def _rel_dev(got, ref):
    return max(float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()) for a, b in zip(got, ref))


@pytest.mark.parametrize("hidden_act", ["relu", "tanh"])
def test_against_float64_with_torch_float32_as_the_yardstick(hidden_act):
    import torch
    from torch import nn
    eng = _engine()
    x, ws, bs, gout = _case(64, 33, 40, [37, 37, 5])
    r = _run(eng, x, ws, bs, gout, hidden_act=hidden_act)
    assert r["ok"]
    ref = _f64_backward(x, ws, bs, gout, r["hidden"], hidden_act)
    act = nn.ReLU if hidden_act == "relu" else nn.Tanh
    seq = nn.Sequential(nn.Linear(40, 37), act(), nn.Linear(37, 37), act(), nn.Linear(37, 5))
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    with torch.no_grad():
        for m, w, b in zip(lin, ws, bs):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    xt = torch.from_numpy(x).requires_grad_(True)
    seq(xt).backward(torch.from_numpy(gout))
    yard = _rel_dev([xt.grad.numpy()] + [m.weight.grad.numpy() for m in lin] + [m.bias.grad.numpy() for m in lin], ref)
    mine = _rel_dev([r["dx"]] + r["dws"] + r["dbs"], ref)
    _yard[hidden_act] = yard
    print(f"{hidden_act} 40 -> 37 -> 37 -> 5 at B = 33, largest deviation from float64 relative to the tensor's largest element: op {mine:.3e}, torch float32 CPU autograd {yard:.3e}")
    assert mine <= 4.0 * yard, (mine, yard)


# ------------------------------------------------------------------------------------------------- TrainMLP under autograd
def _seq(sizes, hidden_act="relu", out_act=None, seed=0):
    import torch
    from torch import nn
    torch.manual_seed(seed)
    act = nn.ReLU if hidden_act == "relu" else nn.Tanh
    mods = []
    for l in range(len(sizes) - 1):
        mods.append(nn.Linear(sizes[l], sizes[l + 1]))
        if l < len(sizes) - 2:
            mods.append(act())
    if out_act is not None:
        mods.append(nn.ReLU() if out_act == "relu" else nn.Tanh())
    return nn.Sequential(*mods).cuda()


def test_train_mlp_gradients_are_the_raw_ops():
    import torch
    from rl_ptg_amd import TrainMLP
    eng = _engine()
    B = 33
    seq = _seq([41, 37, 17, 5], seed=3)
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    net = TrainMLP(eng, seq, batch=64)
    rng = np.random.default_rng(6)
    x, gout = rng.standard_normal((B, 41)).astype(np.float32), rng.standard_normal((B, 5)).astype(np.float32)
    xa, xb = _t(x[:, :40]).requires_grad_(True), _t(x[:, 40:]).requires_grad_(True)
    y = net(xa, x2=xb)
    assert y.grad_fn is not None and y.shape == (B, 5) and y.data_ptr() == net.out.data_ptr()
    y.backward(_t(gout))
    eng.sync()
    ws, bs = [_h(m.weight) for m in lin], [_h(m.bias) for m in lin]
    raw = _run(eng, x, ws, bs, gout, f1=40)
    assert mr.same_bits(_h(y), raw["out"])
    same = lambda a, b: np.array_equal(_h(a).view(np.int32), b.view(np.int32))
    assert same(xa.grad, raw["dx"][:, :40]) and same(xb.grad, raw["dx"][:, 40:])
    assert all(same(m.weight.grad, raw["dws"][l]) and same(m.bias.grad, raw["dbs"][l]) for l, m in enumerate(lin))
    # a second backward adds to .grad, as autograd does
    net(xa, x2=xb).backward(_t(gout))
    eng.sync()
    assert np.array_equal(_h(lin[0].weight.grad), raw["dws"][0] + raw["dws"][0])
    # the stale forward
    y1 = net(xa, x2=xb)
    net(xa, x2=xb)
    with pytest.raises(RuntimeError, match="latest forward"):
        y1.backward(_t(gout))
    # a frozen net: .grad stays None, the input's gradient is still the raw op's
    for p in seq.parameters():
        p.requires_grad_(False)
        p.grad = None
    xa.grad = xb.grad = None
    net(xa.detach(), x2=xb).backward(_t(gout))
    eng.sync()
    assert all(p.grad is None for p in seq.parameters()) and same(xb.grad, raw["dx"][:, 40:])
    with torch.no_grad():
        assert net(xa, x2=xb).grad_fn is None


def _chain_dev(run):
    """run(dtype, project) -> a list of tensors.  (the project chain's and torch float32's largest deviation from the float64 chain)"""
    import torch
    ref = [_h(t).astype(np.float64) for t in run(torch.float64, False)]
    yard = _rel_dev([_h(t) for t in run(torch.float32, False)], ref)
    mine = _rel_dev([_h(t) for t in run(torch.float32, True)], ref)
    return mine, yard


def test_a_sac_actor_step_through_two_train_mlps():
    """actor TrainMLP -> squashed_rsample -> critic TrainMLP(x2 = actions) with frozen parameters -> sac_actor_loss -> backward(): the
    actor's .grad against the same chain with nn.Sequential; only the networks differ between the chains"""
    import torch
    from rl_ptg_amd import TrainMLP, sac_actor_loss, squashed_rsample
    eng = _engine()
    B, F = 33, 40
    obs32 = _t(np.random.default_rng(1).standard_normal((B, F)).astype(np.float32))
    counter = eng.new_draw_counter()

    def run(dtype, project):
        actor, critics = _seq([F, 37, 37, 2], seed=1), [_seq([F + 1, 33, 33, 1], seed=2 + k) for k in range(2)]
        for m in [actor] + critics:
            m.to(dtype)
        for c in critics:
            for p in c.parameters():
                p.requires_grad_(False)
        obs = obs32.to(dtype)
        counter.zero_()
        if project:
            ml = TrainMLP(eng, actor, batch=B)(obs)
        else:
            ml = actor(obs)
        a, lp = squashed_rsample(eng, ml[:, :1], ml[:, 1:], counter, seed=3)
        if project:
            q = [TrainMLP(eng, c, batch=B)(obs, x2=a) for c in critics]
        else:
            q = [c(torch.cat([obs, a], dim=1)) for c in critics]
        loss, _ = sac_actor_loss(eng, q, lp, ent_coef=0.2)
        loss.backward()
        eng.sync()
        assert all(p.grad is None for c in critics for p in c.parameters())
        return [p.grad for p in actor.parameters()]

    mine, yard = _chain_dev(run)
    print(f"SAC actor step, the actor's .grad, largest relative deviation from the float64 chain: TrainMLP {mine:.3e}, nn.Sequential float32 {yard:.3e}")
    assert mine <= 4.0 * yard, (mine, yard)


def test_a_dqn_step_through_train_mlp_and_the_device_optimizer():
    import torch
    from rl_ptg_amd import DeviceOptimizer, TrainMLP, dqn_loss
    eng = _engine()
    B, F, A = 33, 40, 5
    rng = np.random.default_rng(2)
    obs32, nq32 = _t(rng.standard_normal((B, F)).astype(np.float32)), _t(rng.standard_normal((B, A)).astype(np.float32))
    actions, rewards, dones = _t(rng.integers(0, A, B).astype(np.int64)), _t(rng.standard_normal(B).astype(np.float32)), _t((rng.random(B) < 0.2).astype(np.float32))

    def run(dtype, project):
        net = _seq([F, 37, 37, 37, A], seed=7).to(dtype)
        start = [p.detach().clone() for p in net.parameters()]
        opt = DeviceOptimizer(eng, net.parameters(), kind="adam", lr=1e-3)
        q = TrainMLP(eng, net, batch=B)(obs32) if project else net(obs32.to(dtype))
        loss, _ = dqn_loss(eng, q, nq32.to(dtype), actions, rewards, dones, gamma=0.97)
        loss.backward()
        opt.step()
        eng.sync()
        return [p.detach() - p0 for p, p0 in zip(net.parameters(), start)]      # the step each parameter took

    mine, yard = _chain_dev(run)
    print(f"DQN step, the step Adam took, largest relative deviation from the float64 chain: TrainMLP {mine:.3e}, nn.Sequential float32 {yard:.3e}")
    assert mine <= 4.0 * yard, (mine, yard)


# ------------------------------------------------------------------------------------------------- a whole captured gradient step
def test_one_captured_gradient_step_replayed_three_times():
    """mlp_forward(keep_hidden) -> td_loss -> mlp_backward into preallocated .grad tensors -> DeviceOptimizer.step(), captured on a side
    stream at the default hardware-queue setting and replayed three times with fresh batches written in place: the parameters are bit-equal
    to a twin's after the same steps run eagerly"""
    import torch
    from rl_ptg_amd import DeviceOptimizer
    eng = _engine()
    B, F, A = 65, 40, 5
    widths = [37, 33, A]

    class Step:
        def __init__(self):
            self.net = _seq([F] + widths, seed=11)
            self.lin = [m for m in self.net if isinstance(m, torch.nn.Linear)]
            for p in self.net.parameters():
                p.grad = torch.zeros_like(p)
            self.w, self.b = [m.weight.detach() for m in self.lin], [m.bias.detach() for m in self.lin]
            self.gw, self.gb = [m.weight.grad for m in self.lin], [m.bias.grad for m in self.lin]
            z = lambda *s, **kw: torch.zeros(*s, device="cuda", **kw)
            self.obs, self.nq, self.act, self.rew, self.done = z(B, F), z(B, A), z(B, dtype=torch.int64), z(B), z(B)
            self.out = z(B, A)
            self.ws = torch.empty(eng.mlp_workspace(B, widths, True), dtype=torch.uint8, device="cuda")
            self.bws = torch.empty(eng.mlp_backward_workspace(B, widths), dtype=torch.uint8, device="cuda")
            self.tdws = eng.td_loss_workspace(B)
            self.td = None
            self.opt = DeviceOptimizer(eng, self.net.parameters(), kind="adam", lr=1e-3, max_grad_norm=10.0)

        def load(self, k):
            rng = np.random.default_rng(1000 + k)
            self.obs.copy_(_t(rng.standard_normal((B, F)).astype(np.float32)))
            self.nq.copy_(_t(rng.standard_normal((B, A)).astype(np.float32)))
            self.act.copy_(_t(rng.integers(0, A, B).astype(np.int64)))
            self.rew.copy_(_t(rng.standard_normal(B).astype(np.float32)))
            self.done.copy_(_t((rng.random(B) < 0.2).astype(np.float32)))

        def __call__(self):
            eng.mlp_forward(self.obs, self.w, self.b, out=self.out, workspace=self.ws, keep_hidden=True)
            self.td = eng.td_loss("dqn", self.out, self.nq, self.rew, self.done, 0.97, actions=self.act, out=self.td, workspace=self.tdws)
            eng.mlp_backward(self.td.grad_q, self.obs, self.w, self.b, self.out, self.ws, grad_weights=self.gw, grad_biases=self.gb, backward_workspace=self.bws)
            self.opt.step()

    cap, twin = Step(), Step()
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
    before = [_h(p).copy() for p in cap.net.parameters()]
    for k in (1, 2, 3):
        cap.load(k)
        graph.replay()
        twin.load(k)
        twin()
        torch.cuda.synchronize()
        for p, q in zip(cap.net.parameters(), twin.net.parameters()):
            assert np.array_equal(_h(p).view(np.int32), _h(q).view(np.int32)), k
    assert all(not np.array_equal(a, _h(p)) for a, p in zip(before, cap.net.parameters()))
    eng.sync()


# ------------------------------------------------------------------------------------------------- runtime guarantees
def test_no_host_synchronisation_no_allocation_and_identical_bits_on_two_runs():
    """A condition, not a timing: the stream is busy with fused steps before the call and still busy when it has returned; with every
    output and both workspaces given, the allocator hands out nothing during it.  Then the same call again: identical bits"""
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
    B, widths = 257, [64, 33, 5]
    x, ws, bs, gout = _case(1, B, 40, widths)
    xd, wd, bd, gd = _t(x), [_t(w) for w in ws], [_t(b) for b in bs], _t(gout)
    out = torch.empty((B, 5), device="cuda")
    work = torch.empty(eng.mlp_workspace(B, widths, True), dtype=torch.uint8, device="cuda")
    bws = torch.empty(eng.mlp_backward_workspace(B, widths), dtype=torch.uint8, device="cuda")
    gw, gb, gx = [torch.empty_like(w) for w in wd], [torch.empty_like(b) for b in bd], torch.empty_like(xd)
    eng.mlp_forward(xd, wd, bd, out=out, workspace=work, keep_hidden=True)

    def op():
        eng.mlp_backward(gd, xd, wd, bd, out, work, grad_weights=gw, grad_biases=gb, grad_x=gx, backward_workspace=bws)

    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                        # warm: first-launch work is not part of the condition
    op()
    torch.cuda.synchronize()
    first = [_h(t).copy() for t in gw + gb + [gx]]
    for t in gw + gb + [gx]:
        t.fill_(SENTINEL)
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
    assert busy_before is False, "the rollouts were over before the call: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the call had returned: it waited for the device"
    assert allocs_after == allocs, "a call with every output and both workspaces given allocated device memory"
    eng.sync()
    assert all(np.array_equal(a.view(np.int32), _h(t).view(np.int32)) for a, t in zip(first, gw + gb + [gx]))
    eng.close()


def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B = 20
    L, h, stream = eng._L, eng._h, eng._stream()
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    x, x2, out, gout = full(B, 42), full(B, 2), full(B, 6), full(B, 6)
    w = [full(8, 44), full(8, 8), full(5, 8)]
    b = [full(8), full(8), full(5)]
    gw, gb = [full(8, 44), full(8, 8), full(5, 8)], [full(8), full(8), full(5)]
    gx, gx2 = full(B, 42), full(B, 2)
    need, needb = eng.mlp_workspace(B, [8, 8, 5], True), eng.mlp_backward_workspace(B, [8, 8, 5])
    ws = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    bws = torch.full((needb + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t, off=0: t.data_ptr() + off

    def fill(d, a):
        for k, v in a.items():
            if isinstance(v, (list, tuple)):
                for j, e in enumerate(v):
                    getattr(d, k)[j] = e
            else:
                setattr(d, k, v)

    def desc(fwd=None, **kw):
        f = dict(batch=B, n_layers=3, flags=_lib.MLP_KEEP_HIDDEN, hidden_act=_lib.MLP_TANH, out_act=_lib.MLP_TANH, f1=40, f2=1, x_dev=p(x), x_s_n=42, x2_dev=p(x2), x2_s_n=2,
                 w_dev=[p(t) for t in w], w_s_n=[44, 8, 8], b_dev=[p(t) for t in b], width=[8, 8, 5], out_dev=p(out), out_s_n=6, ws_dev=p(ws), ws_bytes=need)
        f.update(fwd or {})
        a = dict(gout_dev=p(gout), gout_s_n=6, dw_dev=[p(t) for t in gw], dw_s_n=[44, 8, 8], db_dev=[p(t) for t in gb], dx_dev=p(gx), dx_s_n=42, dx2_dev=p(gx2), dx2_s_n=2,
                 bws_dev=p(bws), bws_bytes=needb, flags=0)
        a.update(kw)
        d = _lib.PtgMlpBwd()
        fill(d.fwd, f)
        fill(d, a)
        return d

    F = lambda **kw: desc(fwd=kw)
    bad = [F(batch=0), F(batch=2 ** 31 + 1), F(n_layers=0), F(n_layers=11), F(flags=0), F(flags=_lib.MLP_KEEP_HIDDEN | 8), F(flags=_lib.MLP_KEEP_HIDDEN | _lib.MLP_NARROW | _lib.MLP_WIDE),
           F(hidden_act=2), F(out_act=3), F(f1=0), F(f2=-1), F(x_dev=None), F(x_s_n=39), F(x2_dev=None), F(x2_s_n=0), F(w_dev=[p(w[0]), None, p(w[2])]),
           F(b_dev=[None, p(b[1]), p(b[2])]), F(w_s_n=[40, 8, 8]), F(width=[8, 0, 5]), F(width=[8, 8, 1025]), F(out_dev=None), F(out_dev=p(out, 2)), F(out_s_n=4),
           F(ws_dev=None), F(ws_dev=p(ws, 2)), F(ws_bytes=need - 1)]
    n_fwd = len(bad)                                          # so far: faults of the embedded forward descriptor
    bad += [desc(gout_dev=None), desc(gout_s_n=4), desc(dw_dev=[p(gw[0]), None, p(gw[2])]), desc(db_dev=[None, p(gb[1]), p(gb[2])]), desc(dw_s_n=[40, 8, 8]),
           desc(dw_s_n=[44, 7, 8]), desc(dx_s_n=39), desc(dx2_s_n=0), desc(fwd=dict(f2=0, x2_dev=None, w_s_n=[40, 8, 8])), desc(bws_dev=None), desc(bws_dev=p(bws, 2)),
           desc(bws_bytes=needb - 1), desc(bws_bytes=0), desc(flags=1), desc(flags=2), desc(flags=4), desc(flags=16), desc(flags=-1)]
    for k, d in enumerate(bad):
        assert L.ptg_mlp_backward(h, C.byref(d), stream) == _lib.E_INVALID, k
        why = L.ptg_last_error(h).decode()
        assert why.startswith("ptg_mlp_backward:"), k
        if k < n_fwd and d.fwd.flags != 0:                   # a faulty embedded descriptor (F(flags=0) the forward accepts): one check, the forward's words
            assert L.ptg_mlp_forward(h, C.byref(d.fwd), stream) == _lib.E_INVALID, k
            fwd_why = L.ptg_last_error(h).decode()
            assert fwd_why.startswith("ptg_mlp_forward: ") and why == "ptg_mlp_backward: the forward's descriptor: " + fwd_why[len("ptg_mlp_forward: "):], (k, why, fwd_why)
    assert L.ptg_mlp_backward(None, C.byref(desc()), stream) == _lib.E_INVALID and L.ptg_mlp_backward(h, None, stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True        # nothing was enqueued
    torch.cuda.synchronize()
    for t in gw + gb + [gx, gx2]:
        assert bool((t == SENTINEL).all())
    assert bool((bws == 0x5A).all()) and bool((ws == 0x5A).all())
    good = desc(bws_dev=p(bws, 4), fwd=dict(ws_dev=p(ws, 4)))      # 4-byte alignment is enough; the forward first
    assert L.ptg_mlp_forward(h, C.byref(good.fwd), stream) == 0 and L.ptg_mlp_backward(h, C.byref(good), stream) == 0
    eng.sync()
    assert bool((gw[0][:, :41] != SENTINEL).all()) and bool((gw[0][:, 41:] == SENTINEL).all()) and bool((gx[:, :40] != SENTINEL).all()) and bool((gx[:, 40:] == SENTINEL).all())
    assert bool((gx2[:, :1] != SENTINEL).all()) and bool((gx2[:, 1] == SENTINEL).all()) and bool((bws[:4] == 0x5A).all()) and bool((bws[needb + 4:] == 0x5A).all())
