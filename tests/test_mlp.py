"""ptg_mlp_forward, HipEngine.mlp_forward and rl_ptg_amd.DeviceMLP (include/ptg_env.h) against the NumPy restatement
(tests/mlp_restatement.py, pinned against exact rationals and a float64 matmul by tests/test_mlp_host.py).

Bounds, derived and not measured.
  bit for bit, through integer views with +0 == -0: every pre-activation chain (bias, then fmaf over ascending k), hence the output and
    every kept hidden layer of a ReLU net, whatever B, the row's place in the batch and the tile route.  This rests on the exact-float32
    MFMA being a k-ordered fmaf chain; should it fail, the chain holds mlp_restatement.chain_bound against float64 and DESIGN.md
    section 18 says so
  tanh: the kernel evaluates the double-precision library tanh on the float32 chain and rounds once; NumPy's tanh is another library, both
    within an ulp of float64, far below half a float32 spacing except next to a float32 midpoint: within ONE float32 spacing of the
    rounded np.tanh (section 17's float32 bound).  A tanh net is therefore checked layer by layer, the restatement FED THE OP'S OWN
    previous hidden layer (keep_hidden), so that this spacing is not counted twice
Each tanh test prints its measured maximum in float32 spacings.

The grid is thinned diagonally as tests/test_quantile_loss.py's and tests/test_actor.py's are: at every B all ten (fan-in, out) pairs are
run, and the depth (1, 2, 3, 10 layers: d % 4), keep_hidden (d % 3 == 0), the strided layout with guards ((d + 1) % 5 < 2) and the two-piece
input (d % 7 < 3) walk diagonally over them, d = B's position + the pair's; the moduli are pairwise co-prime, so over d = 0 .. 19 every
depth meets keep_hidden on and off and each layout, and every value of every axis meets every pair and every B somewhere.  All of these B are below the host's
switch to the wide route, so every pair also runs at B = 17 and B = 129 through BOTH routes, forced, with keep_hidden."""
import ctypes as C

import numpy as np
import pytest

import mlp_restatement as mr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
BS = [1, 6, 15, 16, 17, 31, 33, 64, 65, 129, 257]
PAIRS = [(1, 1), (2, 3), (3, 5), (4, 16), (5, 17), (40, 64), (41, 33), (31, 233), (233, 37), (63, 129)]
DEPTHS = [1, 2, 3, 10]
_engines = {}
_spec = []
_worst = {"tanh": 0.0}


def _engine(n=64, fresh=False):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if not fresh and n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])      # 139-step episodes
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[n] = eng
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(t):
    return t.detach().cpu().numpy()


def _widths(fi, out, n):
    """the net that starts with the pair: fi -> out -> fi -> out ..., n layers"""
    return [out if l % 2 == 0 else fi for l in range(n)]


def _case(seed, B, fi, widths):
    rng = np.random.default_rng(seed)
    ws, bs = mr.net(rng, fi, widths, scale=1.5)
    return rng.standard_normal((B, fi)).astype(np.float32), ws, bs


def _strided_in(x, lead=2, tail=3):
    """a host [B, F] array as columns lead .. lead + F of a [B, lead + F + tail] device tensor"""
    import torch
    w = torch.full((x.shape[0], lead + x.shape[1] + tail), SENTINEL, device="cuda")
    w[:, lead:lead + x.shape[1]] = _t(x)
    return w[:, lead:lead + x.shape[1]]


def _guarded_out(B, O):
    """[B, O] inside a [B + 2, O + 3] tensor of sentinels: a guard row above and below, one guard column left and two right"""
    import torch
    g = torch.full((B + 2, O + 3), SENTINEL, device="cuda")
    return g[1:B + 1, 1:O + 1], g


def _guards_intact(g, B, O):
    m = np.ones(g.shape, bool)
    m[1:B + 1, 1:O + 1] = False
    return bool((_h(g)[m] == SENTINEL).all())


def _forward(eng, x, ws, bs, strided=False, **kw):
    """mlp_forward on host arrays; the weights of a strided call are column slices too.  Returns (out, hidden, everything else intact)"""
    import torch
    B, O = x.shape[0], ws[-1].shape[0]
    keep = kw.get("keep_hidden", False)
    xd = _strided_in(x) if strided else _t(x)
    if kw.get("x2") is not None:
        kw["x2"] = _strided_in(kw["x2"], 1, 1) if strided else _t(kw["x2"])
    wd = [_strided_in(w, 0, 5) if strided else _t(w) for w in ws]
    out, g = _guarded_out(B, O) if strided else (None, None)
    need = eng.mlp_workspace(B, [w.shape[0] for w in ws], keep)
    work = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    res = eng.mlp_forward(xd, wd, [_t(b) for b in bs], out=out, workspace=work[:need], **kw)
    eng.sync()
    ok = (g is None or _guards_intact(g, B, O)) and bool((work[need:] == 0x5A).all())
    if keep:                                                 # the pad columns of the kept rows are never stored
        off = 0
        for w in [w.shape[0] for w in ws[:-1]]:
            p = (w + 3) // 4 * 4
            ok = ok and bool((work[off:off + 4 * B * p].view(B, 4 * p)[:, 4 * w:] == 0x5A).all())
            off += 4 * B * p
    return _h(res.out), None if res.hidden is None else [_h(t) for t in res.hidden], ok


# ------------------------------------------------------------------------------------------------- the lane maps, with exact integers
@pytest.mark.parametrize("route,B,K,O", [("narrow", 37, 19, 45), ("wide", 150, 70, 150), ("narrow", 150, 70, 150), ("wide", 37, 19, 45)])
def test_the_lane_maps_with_exact_integer_data(route, B, K, O):
    """small integers, an ASYMMETRIC integer W and integer biases: every partial sum is exact, so the order cannot matter and an int64
    matmul is the reference -- a swapped row / column or a wrong lane map shows whatever the numerics.  First A = I: the op returns W^T"""
    eng = _engine()
    rng = np.random.default_rng(5)
    W = ((3 * np.arange(O)[:, None] + 5 * np.arange(K)[None, :]) % 11 - 4 + (np.arange(O)[:, None] > np.arange(K)[None, :])).astype(np.int64)
    assert not np.array_equal(W[:min(O, K), :min(O, K)], W[:min(O, K), :min(O, K)].T)
    b = rng.integers(-9, 10, O)
    eye = np.eye(K, dtype=np.int64)
    out, _, ok = _forward(eng, eye.astype(np.float32), [W.astype(np.float32)], [np.zeros(O, np.float32)], _route=route)
    assert ok and np.array_equal(out.astype(np.int64), W.T)
    x = rng.integers(-3, 4, (B, K))
    out, _, ok = _forward(eng, x.astype(np.float32), [W.astype(np.float32)], [b.astype(np.float32)], strided=True, _route=route)
    assert ok and np.array_equal(out.astype(np.int64), x @ W.T + b)
    W2 = rng.integers(-2, 3, (7, O))
    out, hid, ok = _forward(eng, x.astype(np.float32), [W.astype(np.float32), W2.astype(np.float32)], [b.astype(np.float32), np.zeros(7, np.float32)],
                            keep_hidden=True, _route=route)
    h = np.maximum(x @ W.T + b, 0)
    assert ok and np.array_equal(hid[0].astype(np.int64), h) and np.array_equal(out.astype(np.int64), h @ W2.T)


# ------------------------------------------------------------------------------------------------- bit for bit over the grid
def _check_relu_net(eng, seed, B, fi, widths, keep, strided, two_piece, route=None):
    x, ws, bs = _case(seed, B, fi, widths)
    kw = dict(keep_hidden=keep, _route=route)
    ref_out, ref_hid = mr.forward(x, ws, bs)
    if two_piece:
        cut = fi // 2
        out, hid, ok = _forward(eng, x[:, :cut], ws, bs, strided=strided, x2=x[:, cut:], **kw)
    else:
        out, hid, ok = _forward(eng, x, ws, bs, strided=strided, **kw)
    assert ok, "a guard column, a guard row, the workspace's tail or a pad column was written"
    assert mr.same_bits(out, ref_out), (B, fi, widths, float(np.abs(out - ref_out).max()), float(mr.chain_bound(ref_hid[-1] if ref_hid else x, ws[-1], bs[-1]).max()))
    if keep:
        assert len(hid) == len(widths) - 1
        for l, hl in enumerate(hid):
            assert mr.same_bits(hl, ref_hid[l]), (B, fi, widths, l)
    return out


@pytest.mark.parametrize("B", BS)
def test_relu_nets_bit_for_bit_over_the_grid(B):
    eng = _engine()
    ib = BS.index(B)
    for ip, (fi, out) in enumerate(PAIRS):
        d = ib + ip
        n = DEPTHS[d % 4]
        _check_relu_net(eng, 100 * ib + ip, B, fi, _widths(fi, out, n), keep=d % 3 == 0, strided=(d + 1) % 5 < 2, two_piece=fi >= 2 and d % 7 < 3)


@pytest.mark.parametrize("B", [17, 129])
def test_every_pair_through_both_routes(B):
    eng = _engine()
    for ip, (fi, out) in enumerate(PAIRS):
        outs = [_check_relu_net(eng, 7000 + ip, B, fi, _widths(fi, out, 3), keep=True, strided=ip % 2 == 0, two_piece=fi >= 2 and ip % 3 == 0, route=r)
                for r in ("narrow", "wide")]
        assert mr.same_bits(outs[0], outs[1])


RING = [1, 31, 32, 33, 64, 65, 128, 129, 160, 257]           # chunks of 32: below, at, one above and at twice the ring depths 2 and 4, with and without a ragged last chunk


@pytest.mark.parametrize("K", RING)
@pytest.mark.parametrize("route,rest", [("narrow", 17), ("wide", 70)])
def test_the_ring_at_its_edges(route, rest, K):
    """the reduction length K at the edges of the chunk ring (four chunks in flight NARROW, two WIDE); B = O = 17: two tiles, one ragged;
    WIDE at B = O = 70: one workgroup, two live, partly filled quadrants per side.  Strided, in guard frames, hidden layer kept"""
    _check_relu_net(_engine(), 8000 + K, rest, K, [rest, rest], keep=True, strided=True, two_piece=False, route=route)


def test_the_widest_net():
    """1024 -> 1024 -> 5 at B = 17: the limits of fan-in and width, 64 unit tiles of the narrow route and 8 of the wide one"""
    eng = _engine()
    x, ws, bs = _case(11, 17, 1024, [1024, 5])
    ref_out, ref_hid = mr.forward(x, ws, bs)
    for route in (None, "wide"):
        out, hid, ok = _forward(eng, x, ws, bs, keep_hidden=True, _route=route)
        assert ok and mr.same_bits(hid[0], ref_hid[0]) and mr.same_bits(out, ref_out)


def test_the_hosts_own_switch_and_a_call_that_mixes_the_routes():
    """no route flag: at B = 16 384 a 257-wide hidden layer takes the wide route and the 5-unit output the narrow one; at B = 4 096 a
    513-wide layer is wide already and a 257-wide one is not.  Rows from both ends and the middle against the restatement, and the whole
    output against the same call forced onto the narrow route"""
    eng = _engine()
    for B, widths in ((16384, [257, 5]), (4096, [513, 257, 5])):
        x, ws, bs = _case(B, B, 40, widths)
        out, hid, ok = _forward(eng, x, ws, bs, keep_hidden=True)
        narrow, _, _ = _forward(eng, x, ws, bs, _route="narrow")
        rows = np.r_[0:20, B // 2 - 10:B // 2 + 10, B - 20:B]
        ref_out, ref_hid = mr.forward(x[rows], ws, bs)
        assert ok and np.array_equal(out.view(np.int32), narrow.view(np.int32)) and mr.same_bits(out[rows], ref_out)
        assert all(mr.same_bits(h[rows], r) for h, r in zip(hid, ref_hid))


def test_the_two_piece_input_against_the_concatenated_tensor():
    eng = _engine()
    for B, f1, f2, route in ((33, 40, 1, None), (129, 37, 4, "wide"), (6, 1, 40, "narrow")):
        x, ws, bs = _case(B, B, f1 + f2, [33, 9, 2])
        whole, _, ok1 = _forward(eng, x, ws, bs, _route=route)
        split, _, ok2 = _forward(eng, x[:, :f1], ws, bs, x2=x[:, f1:], strided=True, _route=route)
        assert ok1 and ok2 and np.array_equal(whole.view(np.int32), split.view(np.int32)) and mr.same_bits(whole, mr.forward(x, ws, bs)[0])


# ------------------------------------------------------------------------------------------------- tanh
def _tanh_spacings(got, pre):
    ref = np.tanh(pre.astype(np.float64)).astype(np.float32)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())


def _check_tanh_layers(eng, x, ws, bs, hid, out, out_act=None):
    """layer l of the op against the restatement fed the op's own layer l - 1: the chain bit for bit -- read through a one-layer call without
    activation, whose bits the batch / route invariance makes the fused call's -- and the tanh of that chain within one float32 spacing"""
    h, worst = x, 0.0
    n = len(ws)
    for l in range(n):
        pre = mr.pre_activation(h, ws[l], bs[l])
        chain, _, ok = _forward(eng, h, [ws[l]], [bs[l]])
        assert ok and mr.same_bits(chain, pre), l
        got = out if l == n - 1 else hid[l]
        if l < n - 1 or out_act == "tanh":
            worst = max(worst, _tanh_spacings(got, pre))
        else:
            assert mr.same_bits(got, mr.act(pre, out_act)), l
        h = got
    assert worst <= 1.0, worst
    _worst["tanh"] = max(_worst["tanh"], worst)
    return worst


@pytest.mark.parametrize("B,fi,widths,out_act,route", [(33, 41, [33, 17, 5], None, None), (129, 40, [64, 233, 37, 1], "tanh", "wide"), (6, 31, [233, 233, 2], "tanh", None),
                                                       (257, 5, [17] * 9 + [3], None, None)])
def test_tanh_nets_layer_by_layer(B, fi, widths, out_act, route):
    eng = _engine()
    x, ws, bs = _case(B + fi, B, fi, widths)
    x *= 2.0                                                 # pre-activations across tanh's bend and into its flat part
    out, hid, ok = _forward(eng, x, ws, bs, hidden_activation="tanh", out_activation=out_act, keep_hidden=True, _route=route)
    assert ok
    worst = _check_tanh_layers(eng, x, ws, bs, hid, out, out_act)
    print(f"tanh net B={B} {fi}->{widths}: max |op - float32(np.tanh)| = {worst:.3f} float32 spacings (bound 1); so far {_worst['tanh']:.3f}")


# ------------------------------------------------------------------------------------------------- invariance, planted values
def test_a_row_does_not_depend_on_the_batch_its_place_or_the_route():
    eng = _engine()
    B = 257
    x, ws, bs = _case(3, B, 40, [64, 33, 5])
    full, _, _ = _forward(eng, x, ws, bs, _route="narrow")
    other, _, _ = _forward(eng, x, ws, bs, _route="wide")
    assert np.array_equal(full.view(np.int32), other.view(np.int32)) and mr.same_bits(full, mr.forward(x, ws, bs)[0])
    for b in (0, 1, 15, 16, 17, 127, 128, 255, 256):
        for route in ("narrow", "wide"):
            one, _, _ = _forward(eng, x[b:b + 1], ws, bs, _route=route)
            assert np.array_equal(one.view(np.int32), full[b:b + 1].view(np.int32)), (b, route)
    part, _, _ = _forward(eng, x[100:131], ws, bs)           # 31 rows from the middle land in other tile rows
    assert np.array_equal(part.view(np.int32), full[100:131].view(np.int32))


def test_planted_values():
    """a NaN and an Inf input row stay in their rows; float32-subnormal products (2^-70 * 2^-70) and a subnormal bias come through
    un-flushed; -0 inputs"""
    eng = _engine()
    B = 70
    x, ws, bs = _case(9, B, 41, [33, 5])
    clean, _, _ = _forward(eng, x, ws, bs)
    bad = x.copy()
    bad[20, 7] = np.nan
    bad[66, 40] = np.inf
    for route in ("narrow", "wide"):
        out, hid, ok = _forward(eng, bad, ws, bs, keep_hidden=True, _route=route)
        ref_out, ref_hid = mr.forward(bad, ws, bs)
        rest = np.ones(B, bool)
        rest[[20, 66]] = False
        assert ok and np.array_equal(out[rest].view(np.int32), clean[rest].view(np.int32))
        assert mr.same_bits(out, ref_out) and mr.same_bits(hid[0], ref_hid[0]) and np.isnan(out[20]).all() and np.isnan(hid[0][20]).all()
        one, _, _ = _forward(eng, bad, ws[:1], bs[:1], _route=route)                  # without an activation the Inf row is +-Inf throughout
        assert mr.same_bits(one, mr.pre_activation(bad, ws[0], bs[0])) and not np.isfinite(one[66]).any() and not np.isfinite(one[20]).any()
        assert np.isfinite(one[rest]).all()
    rng = np.random.default_rng(2)
    K, O = 23, 19
    tiny_x = (rng.integers(1, 8, (B, K)) * 2.0 ** -70).astype(np.float32)
    tiny_w = (rng.integers(-7, 8, (O, K)) * 2.0 ** -70).astype(np.float32)
    tiny_b = (rng.integers(-3, 4, O) * 2.0 ** -149).astype(np.float32)
    tiny_x[5] = -0.0
    for route in ("narrow", "wide"):
        out, _, ok = _forward(eng, tiny_x, [tiny_w], [tiny_b], _route=route)
        ref = mr.pre_activation(tiny_x, tiny_w, tiny_b)
        assert ok and mr.same_bits(out, ref) and (np.abs(ref[rest]) < 2.0 ** -126).all() and (ref != 0).sum() > B * O // 2
        assert mr.same_bits(out[5], np.broadcast_to(tiny_b, (O,)))               # -0 inputs: the bias alone
    zeros = np.full((4, K), -0.0, np.float32)
    out, _, _ = _forward(eng, zeros, [tiny_w, np.ones((2, O), np.float32)], [np.zeros(O, np.float32), np.zeros(2, np.float32)])
    assert (out == 0).all()


def test_two_runs_give_identical_bits():
    eng = _engine()
    x, ws, bs = _case(21, 257, 63, [129, 129, 7])
    a, ha, _ = _forward(eng, x, ws, bs, hidden_activation="tanh", keep_hidden=True)
    b, hb, _ = _forward(eng, x, ws, bs, hidden_activation="tanh", keep_hidden=True)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(ha, hb))


# ------------------------------------------------------------------------------------------------- DeviceMLP
def _params(mods):
    """(weights, biases) of the Linear layers of torch modules, as they are on the device now"""
    import torch
    lin = [m for seq in mods for m in (seq if isinstance(seq, torch.nn.Sequential) else [seq]) if isinstance(m, torch.nn.Linear)]
    return [_h(m.weight) for m in lin], [_h(m.bias) for m in lin]


def test_device_mlp_reads_the_parameters_where_the_optimiser_and_polyak_left_them():
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, DeviceOptimizer
    eng = _engine()
    torch.manual_seed(5)
    B = 33
    net = nn.Sequential(nn.Linear(40, 37), nn.ReLU(), nn.Linear(37, 37), nn.ReLU(), nn.Linear(37, 5)).cuda()
    target = nn.Sequential(nn.Linear(40, 37), nn.ReLU(), nn.Linear(37, 37), nn.ReLU(), nn.Linear(37, 5)).cuda()
    x = np.random.default_rng(1).standard_normal((B, 40)).astype(np.float32)
    xd = _t(x)
    q, q_t = DeviceMLP(eng, net, batch=64), DeviceMLP(eng, target, batch=64)
    y = q(xd)
    assert y.shape == (B, 5) and not y.requires_grad and y.data_ptr() == q.out.data_ptr()
    assert mr.same_bits(_h(y), mr.forward(x, *_params([net]))[0])
    before = _params([net])
    opt = DeviceOptimizer(eng, net.parameters(), kind="adam", lr=1e-2)
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt.step()
    y = q(xd)
    eng.sync()
    after = _params([net])
    assert all(not np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert mr.same_bits(_h(y), mr.forward(x, *after)[0]) and not mr.same_bits(_h(y), mr.forward(x, *before)[0])
    t_before = _params([target])
    plan = eng.polyak_update([p.detach() for p in net.parameters()], [p.detach() for p in target.parameters()], 0.25)
    y_t = q_t(xd)
    eng.sync()
    t_after = _params([target])
    assert plan.kind == "polyak"
    assert all(not np.array_equal(a, b) for a, b in zip(t_before[0], t_after[0]))
    assert mr.same_bits(_h(y_t), mr.forward(x, *t_after)[0])


def test_device_mlp_as_td3_actor_and_as_sac_trunk_with_two_heads():
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP
    eng = _engine()
    N = eng.n
    torch.manual_seed(6)
    x = np.random.default_rng(4).standard_normal((N, 40)).astype(np.float32)
    xd = _t(x)
    # TD3: create_mlp(..., squash_output=True) ends in Tanh
    mu = nn.Sequential(nn.Linear(40, 33), nn.ReLU(), nn.Linear(33, 17), nn.ReLU(), nn.Linear(17, 1), nn.Tanh()).cuda()
    actor = DeviceMLP(eng, mu, batch=N, hidden=True)
    assert (actor.hidden_activation, actor.out_activation) == ("relu", "tanh")
    a = actor(xd)
    eng.sync()
    ws, bs = _params([mu])
    _, ref_hid = mr.forward(x, ws, bs)
    assert all(mr.same_bits(_h(h), r) for h, r in zip(actor.hidden, ref_hid))
    worst = _tanh_spacings(_h(a), mr.pre_activation(ref_hid[-1], ws[2], bs[2]))
    assert worst <= 1.0 and (np.abs(_h(a)) <= 1).all()
    # SAC: latent_pi, then mu and log_std on the latent; the mean lands in a column of a wider tensor, and both feed the Gaussian head
    latent_pi = nn.Sequential(nn.Linear(40, 33), nn.ReLU(), nn.Linear(33, 33), nn.ReLU()).cuda()
    head_mu, head_ls = nn.Linear(33, 1).cuda(), nn.Linear(33, 1).cuda()
    trunk = DeviceMLP(eng, latent_pi, batch=N)
    assert trunk.out_activation == "relu"
    latent = trunk(xd)
    wide = torch.full((N, 3), SENTINEL, device="cuda")
    mean = eng.mlp_forward(latent, [head_mu.weight.detach()], [head_mu.bias.detach()], out=wide[:, 1:2]).out
    log_std = DeviceMLP(eng, head_ls, batch=N)(latent)
    res = eng.act_gaussian(mean, log_std, None, squash=True, deterministic=True)
    eng.sync()
    (w0, w1), (b0, b1) = _params([latent_pi])
    lat_ref, _ = mr.forward(x, [w0, w1], [b0, b1], out_act=mr.RELU)
    m_ref = mr.pre_activation(lat_ref, _h(head_mu.weight), _h(head_mu.bias))
    assert mr.same_bits(_h(latent), lat_ref) and mr.same_bits(_h(mean), m_ref) and mr.same_bits(_h(log_std), mr.pre_activation(lat_ref, _h(head_ls.weight), _h(head_ls.bias)))
    assert bool((wide[:, 0] == SENTINEL).all()) and bool((wide[:, 2] == SENTINEL).all())
    assert _tanh_spacings(_h(res.actions).reshape(N, 1), m_ref) <= 1.0
    # both chained in one object: [latent_pi, mu]
    both = DeviceMLP(eng, [latent_pi, head_mu], batch=N)
    assert np.array_equal(_h(both(xd)).view(np.int32), _h(mean).view(np.int32))


def test_one_captured_collect_step_replayed_three_times():
    """DeviceMLP (F -> 37 -> 37 -> 5, tanh) -> act_categorical -> replay-proof step, captured once on a side stream at the default
    hardware-queue setting and replayed three times with the weights rewritten in place between the replays: every replay's logits are
    the restatement's on that replay's observations and weights (layer by layer, fed the op's own hidden layers), every action is
    act_categorical's on those logits"""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP
    N = 64
    eng = _engine(N, fresh=True)
    eng.set_replay_proof(True)
    F = eng.obs_dim
    torch.manual_seed(8)
    pi = nn.Sequential(nn.Linear(F, 37), nn.Tanh(), nn.Linear(37, 37), nn.Tanh(), nn.Linear(37, 5)).cuda()
    policy = DeviceMLP(eng, pi, batch=N, hidden=True)
    prev = eng.reset().clone()
    obs, rew, done, fin = eng.alloc_obs(zero=True), torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), eng.alloc_obs(zero=True)
    res = eng.act_categorical(policy(prev), None, deterministic=True)                # the static outputs
    seen = torch.zeros_like(prev)

    def one():
        seen.copy_(prev)                                     # what the policy saw, for the check
        eng.act_categorical(policy(prev), None, deterministic=True, out=res)
        eng.step(res.actions, obs, rew, done, final_obs=fin)
        prev.copy_(obs)

    def check(k):
        ws, bs = _params([pi])
        logits = _h(policy.out)
        worst = _check_tanh_layers(eng, _h(seen), ws, bs, [_h(t) for t in policy.hidden], logits)
        again = eng.act_categorical(policy.out.clone(), None, deterministic=True)
        eng.sync()
        assert torch.equal(again.actions, res.actions) and np.array_equal(_h(res.actions), np.argmax(logits, axis=1)), k
        return worst

    one()                                                    # eager once: code objects are loaded before the capture
    eng.sync()
    worst = check(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    views = []
    for k in (1, 2, 3):
        with torch.no_grad():
            for p in pi.parameters():
                p.mul_(1.0 - 0.1 * k).add_(0.01 * k)         # in place: the graph holds these addresses
        before = _h(seen).copy()
        graph.replay()
        torch.cuda.synchronize()
        assert not np.array_equal(_h(seen), before)          # the env moved on: other observations every replay
        worst = max(worst, check(k))
        views.append(_h(policy.out).copy())
    assert not np.array_equal(views[0], views[1]) and not np.array_equal(views[1], views[2])
    eng.note_replays(3 - 1)
    eng.sync()
    print(f"captured collect step: max tanh error over the eager step and three replays {worst:.3f} float32 spacings")
    eng.close()


# ------------------------------------------------------------------------------------------------- streams, synchronisation, state
def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they have
    returned; with out= and workspace= the allocator hands out nothing during them.  Afterwards env state, finished ring and vn
    statistics equal a twin's that made no call."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    engs = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(5)
        e.vn_init()
        e.reset()
        engs.append(e)
    eng, twin = engs
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    x, ws, bs = _case(1, n, 40, [64, 5])
    xd, wd, bd = _t(x), [_t(w) for w in ws], [_t(b) for b in bs]
    out = torch.empty((n, 5), device="cuda")
    work = torch.empty(eng.mlp_workspace(n, [64, 5], True), dtype=torch.uint8, device="cuda")

    def ops():
        return eng.mlp_forward(xd, wd, bd, out=out, workspace=work, keep_hidden=True)

    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    ops()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    res = ops()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the call: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the call had returned: it waited for the device"
    assert allocs_after == allocs, "a call with out= and workspace= allocated device memory"
    eng.sync()
    rows = np.r_[0:40, n - 40:n]                                                 # the restatement on both ends of the batch
    ref_out, ref_hid = mr.forward(x[rows], ws, bs)
    assert mr.same_bits(_h(res.out)[rows], ref_out) and mr.same_bits(_h(res.hidden[0])[rows], ref_hid[0])
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


def test_on_a_side_stream():
    import torch
    eng = _engine()
    x, ws, bs = _case(31, 129, 41, [33, 5])
    xd, wd, bd = _t(x), [_t(w) for w in ws], [_t(b) for b in bs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = eng.mlp_forward(xd, wd, bd)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    assert mr.same_bits(_h(res.out), mr.forward(x, ws, bs)[0])


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B = 20
    L, h, stream = eng._L, eng._h, eng._stream()
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    x, x2, out = full(B, 42), full(B, 2), full(B, 6)
    w = [full(8, 44), full(8, 8), full(5, 8)]
    b = [full(8), full(8), full(5)]
    need = eng.mlp_workspace(B, [8, 8, 5], True)
    ws = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t, off=0: t.data_ptr() + off

    def desc(**kw):
        a = dict(batch=B, n_layers=3, flags=_lib.MLP_KEEP_HIDDEN, hidden_act=_lib.MLP_TANH, out_act=_lib.MLP_NONE, f1=40, f2=1, x_dev=p(x), x_s_n=42, x2_dev=p(x2), x2_s_n=2,
                 w_dev=[p(t) for t in w], w_s_n=[44, 8, 8], b_dev=[p(t) for t in b], width=[8, 8, 5], out_dev=p(out), out_s_n=6, ws_dev=p(ws), ws_bytes=need)
        a.update(kw)
        d = _lib.PtgMlp()
        for k, v in a.items():
            if isinstance(v, (list, tuple)):
                for j, e in enumerate(v):
                    getattr(d, k)[j] = e
            else:
                setattr(d, k, v)
        return d

    bad = [desc(batch=0), desc(batch=-1), desc(batch=2 ** 31 + 1), desc(n_layers=0), desc(n_layers=11), desc(flags=8), desc(flags=_lib.MLP_NARROW | _lib.MLP_WIDE),
           desc(hidden_act=2), desc(hidden_act=-1), desc(hidden_act=3), desc(out_act=3), desc(out_act=-1), desc(f1=0), desc(f2=-1), desc(f1=1024, f2=1, x_s_n=1024),
           desc(x_dev=None), desc(x_s_n=39), desc(x2_dev=None), desc(f2=0, w_s_n=[40, 8, 8]), desc(x2_s_n=0), desc(w_dev=[p(w[0]), None, p(w[2])]),
           desc(b_dev=[None, p(b[1]), p(b[2])]), desc(w_s_n=[40, 8, 8]), desc(w_s_n=[44, 7, 8]), desc(w_s_n=[44, 8, -8]), desc(width=[8, 0, 5]), desc(width=[8, 8, 1025]),
           desc(width=[9, 8, 5]), desc(out_dev=None), desc(out_dev=p(out, 2)), desc(out_s_n=4), desc(ws_dev=None), desc(ws_dev=p(ws, 2)), desc(ws_bytes=need - 1),
           desc(ws_bytes=0), desc(flags=0, ws_bytes=eng.mlp_workspace(B, [8, 8, 5]) - 1)]
    for k, d in enumerate(bad):
        assert L.ptg_mlp_forward(h, C.byref(d), stream) == _lib.E_INVALID, k
        assert L.ptg_last_error(h).decode().startswith("ptg_mlp_forward:"), k
    assert L.ptg_mlp_forward(None, C.byref(desc()), stream) == _lib.E_INVALID and L.ptg_mlp_forward(h, None, stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True        # nothing was enqueued
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all())
    good = desc(ws_dev=p(ws, 4), ws_bytes=need)              # 4-byte alignment is enough
    assert L.ptg_mlp_forward(h, C.byref(good), stream) == 0
    eng.sync()
    assert bool((out[:, :5] != SENTINEL).all()) and bool((out[:, 5] == SENTINEL).all()) and bool((ws[:4] == 0x5A).all()) and bool((ws[need + 4:] == 0x5A).all())
