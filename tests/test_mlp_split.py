"""PTG_MLP_SPLIT_INPUT on the GPU (include/ptg_env.h): split observation rows as the first layer's input of
ptg_mlp_forward, ptg_mlp_backward and the group calls.  The definition is one sentence -- a split call's result has the bits of the same
call on the rebuilt flat rows -- so the yardstick of every comparison is THE OP'S OWN FLAT CALL on policy_split.flat_rows_from_split(rows),
bit for bit through integer views with +0 == -0 (mr.same_bits), and for a thinned subset the NumPy restatement
(tests/mlp_split_restatement.py).  The rows are synthetic: random float32 env columns, indices over the whole valid range with 0, the
last valid one and one in the second and in the third market set planted; the engines come from prep.synthetic_spec with three sets."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mlp_restatement as mr
import mlp_split_restatement as msr

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 7.5
CONFIGS = [(raw, P) for raw in ("mod", "raw") for P in (1, 13, 25)]
WIDTH = {("mod", 1): 16, ("mod", 13): 40, ("mod", 25): 64, ("raw", 1): 19, ("raw", 13): 31, ("raw", 25): 43}      # below, at and above one 32-chunk, and exactly two
_ctx = {}


class _Ctx:
    """an engine with three market sets (its own obs_layout does not matter to the flag: 'mod' engines are split, 'raw' ones row-major),
    its series and the last valid indices"""

    def __init__(self, raw, P, n=64, layout=None):
        from rl_ptg_amd.engine import HipEngine
        from rl_ptg_amd.prep import synthetic_spec
        specs = [synthetic_spec(scenario=q, operation="OP2", eps_len_d=1, raw_modified=raw, price_ahead=P, train_steps=200000)[0] for q in (1, 2, 3)]
        self.spec = specs[0]
        self.markets = [s.markets[0] for s in specs]
        self.raw, self.P, self.flat = raw, P, WIDTH[raw, P]
        self.eng = HipEngine(self.spec.consts, self.spec.tables, self.markets, n, device=0, out_dtype="float32", obs_layout=layout or ("split" if raw == "mod" else "row"))
        self.series = self.eng.market_feature_series()
        assert self.eng.n_sets == 3 and self.series["featA"].shape[0] == 3
        self.lh, self.ld = msr.last_valid(self.series, raw, P)
        self.nh, self.nd = self.series["featA"].shape[1], self.series["gas_n"].shape[1]

    def rows(self, rng, B):
        r = rng.standard_normal((B, 16)).astype(F32)
        r[:, 14] = rng.integers(0, self.lh + 1, B)
        r[:, 15] = rng.integers(0, self.ld + 1, B)
        r[B - 1, 14:16] = 2 * self.nh + 3, 2 * self.nd + 1                      # the third set
        if B >= 4:
            r[0, 14:16] = 0
            r[1, 14:16] = self.lh, self.ld
            r[2, 14:16] = self.nh + 5, self.nd + 2                              # the second set
        return r

    def flat_rows(self, rows_dev):
        from rl_ptg_amd.policy_split import flat_rows_from_split
        return flat_rows_from_split(rows_dev, self.series, self.raw, self.P).contiguous()


def _ctx_of(raw, P):
    if (raw, P) not in _ctx:
        _ctx[raw, P] = _Ctx(raw, P)
    return _ctx[raw, P]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(t):
    return t.detach().cpu().numpy()


def _wide_rows(rows, x_s_n):
    """host [B, 16] rows as the first 16 columns of a [B, x_s_n] device tensor whose other columns are NaN guards: a read past column 15
    would poison the result"""
    import torch
    w = torch.full((rows.shape[0], x_s_n), float("nan"), device="cuda")
    w[:, :16] = _t(rows)
    return w[:, :16]


def _net(rng, fan_in, widths):
    ws, bs = mr.net(rng, fan_in, widths, scale=1.5)
    return ws, bs, [_t(w) for w in ws], [_t(b) for b in bs]


def _both(ctx, rows_dev, wd, bd, x2=None, route=None, flat_route=None, **kw):
    """(split result, flat result) of mlp_forward; the flat call on the rebuilt rows"""
    eng = ctx.eng
    got = eng.mlp_forward(rows_dev, wd, bd, x2=x2, split=True, _route=route, **kw)
    ref = eng.mlp_forward(ctx.flat_rows(rows_dev), wd, bd, x2=x2, _route=flat_route, **kw)
    eng.sync()
    return got, ref


def _same_out(got, ref):
    ok = mr.same_bits(_h(got.out), _h(ref.out))
    if got.hidden is not None:
        ok = ok and len(got.hidden) == len(ref.hidden) and all(mr.same_bits(_h(a), _h(b)) for a, b in zip(got.hidden, ref.hidden))
    return ok


# ------------------------------------------------------------------------------------------------- the forward grid
GRID = list(itertools.product([1, 15, 16, 17, 65, 129], [1, 16, 17, 64], [1, 3], ["relu", "tanh"], [False, True], [16, 19], [0, 1, 3]))      # B, first width, depth, act, keep, x_s_n, f2


@pytest.mark.parametrize("raw,P", CONFIGS)
def test_the_forward_grid(raw, P):
    """The thinning: of the 1152 cells of GRID (B x first width x depth x activation x keep_hidden x x_s_n x f2) a configuration keeps
    every 13th, starting at its own offset -- 13 is coprime to every axis length, so the kept cells run diagonally through the grid and
    every value of every axis occurs (asserted).  89 cells per configuration against the flat call; every 6th of them with
    B <= 17 against the restatement too."""
    ctx = _ctx_of(raw, P)
    rng = np.random.default_rng(100 + CONFIGS.index((raw, P)))
    kept = GRID[CONFIGS.index((raw, P))::13]
    for axis in range(7):
        assert {c[axis] for c in kept} == {c[axis] for c in GRID}, axis
    restated = 0
    for i, (B, O, depth, act, keep, xsn, f2) in enumerate(kept):
        widths = [O] if depth == 1 else [O, 9, 5]
        ws, bs, wd, bd = _net(rng, ctx.flat + f2, widths)
        rows = ctx.rows(rng, B)
        x2 = rng.standard_normal((B, f2)).astype(F32) if f2 else None
        x2d = None if x2 is None else _t(x2)
        got, ref = _both(ctx, _wide_rows(rows, xsn), wd, bd, x2=x2d, hidden_activation=act, keep_hidden=keep)
        assert _same_out(got, ref), (B, O, depth, act, keep, xsn, f2)
        assert np.isfinite(_h(got.out)).all()                                   # no guard column was read
        if i % 6 == 0 and B <= 17:
            out, hid = msr.forward(rows, ctx.series, raw, P, ws, bs, hidden_act=act, x2=x2)
            if act == "relu":                                                   # tanh is the library's, within a spacing (tests/test_mlp.py pins it): layer 0 alone
                assert mr.same_bits(_h(got.out), out) and (not keep or all(mr.same_bits(_h(a), b) for a, b in zip(got.hidden, hid)))
            else:
                pre = mr.pre_activation(np.concatenate([msr.flat_rows(rows, ctx.series, raw, P)] + ([x2] if f2 else []), axis=1), ws[0], bs[0])
                lin = ctx.eng.mlp_forward(_t(rows), wd[:1], bd[:1], x2=x2d, split=True)
                ctx.eng.sync()
                assert mr.same_bits(_h(lin.out), pre)
            restated += 1
    assert restated >= 3


# ------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("raw,P", CONFIGS)
@pytest.mark.parametrize("B", [17, 129])
def test_both_routes_forced(B, raw, P):
    ctx = _ctx_of(raw, P)
    rng = np.random.default_rng(B + P)
    rows, x2 = _t(ctx.rows(rng, B)), _t(rng.standard_normal((B, 1)).astype(F32))
    ws, bs, wd, bd = _net(rng, ctx.flat + 1, [70, 17, 5])
    outs = []
    for route in ("narrow", "wide"):
        got, ref = _both(ctx, rows, wd, bd, x2=x2, route=route, flat_route="narrow", keep_hidden=True)
        assert _same_out(got, ref), route
        outs.append(_h(got.out))
    assert mr.same_bits(outs[0], outs[1])
    if B == 17:
        out, hid = msr.forward(_h(rows), ctx.series, raw, P, ws, bs, x2=_h(x2))
        assert mr.same_bits(outs[1], out)


def test_the_hosts_own_switch_takes_the_wide_first_layer():
    """B = 16 384 with 40 -> 257 -> 5: the first layer goes WIDE by the host's own switch (B >= 16 384, O > 256), the second NARROW;
    the whole batch against the flat call, and rows from both ends and the middle against the restatement"""
    ctx = _ctx_of("mod", 13)
    rng = np.random.default_rng(5)
    B = 16384
    rows = ctx.rows(rng, B)
    ws, bs, wd, bd = _net(rng, 40, [257, 5])
    got, ref = _both(ctx, _t(rows), wd, bd, keep_hidden=True)
    assert _same_out(got, ref)
    forced, _ = _both(ctx, _t(rows), wd, bd, route="narrow", keep_hidden=True)
    assert _same_out(forced, got)
    pick = np.r_[0:20, B // 2 - 10:B // 2 + 10, B - 20:B]
    out, hid = msr.forward(rows[pick], ctx.series, "mod", 13, ws, bs)
    assert mr.same_bits(_h(got.out)[pick], out) and mr.same_bits(_h(got.hidden[0])[pick], hid[0])


def test_a_row_does_not_depend_on_the_batch():
    for raw, P in (("mod", 13), ("raw", 25)):
        ctx = _ctx_of(raw, P)
        rng = np.random.default_rng(9)
        rows = _t(ctx.rows(rng, 129))
        ws, bs, wd, bd = _net(rng, ctx.flat, [33, 5])
        whole = ctx.eng.mlp_forward(rows, wd, bd, hidden_activation="tanh", split=True).out.clone()
        for b in (0, 1, 64, 128):
            one = ctx.eng.mlp_forward(rows[b:b + 1], wd, bd, hidden_activation="tanh", split=True).out
            ctx.eng.sync()
            assert np.array_equal(_h(one).view(np.int32), _h(whole[b:b + 1]).view(np.int32)), (raw, P, b)


# ------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("G", [2, 3])
def test_a_group_shares_the_split_rows(G):
    """twin (and triple) critics on one split x with their own actions: each equals its single call, forward and backward"""
    import torch
    for raw, P in (("mod", 13), ("raw", 1)):
        ctx = _ctx_of(raw, P)
        eng = ctx.eng
        rng = np.random.default_rng(G + P)
        B = 65
        rows = _t(ctx.rows(rng, B))
        x2s = [_t(rng.standard_normal((B, 3)).astype(F32)) for _ in range(G)]
        nets = [_net(rng, ctx.flat + 3, [17 + 16 * i, 9, 2]) for i in range(G)]
        wds, bds = [n[2] for n in nets], [n[3] for n in nets]
        space = lambda i: torch.empty(eng.mlp_workspace(B, [w.shape[0] for w in wds[i]], True), dtype=torch.uint8, device="cuda")
        wg, wsingle = [space(i) for i in range(G)], [space(i) for i in range(G)]
        res = eng.mlp_group_forward(rows, wds, bds, x2s=x2s, workspaces=wg, keep_hidden=True, split=True)
        single = [eng.mlp_forward(rows, wds[i], bds[i], x2=x2s[i], workspace=wsingle[i], keep_hidden=True, split=True) for i in range(G)]
        flat = [eng.mlp_forward(ctx.flat_rows(rows), wds[i], bds[i], x2=x2s[i], keep_hidden=True) for i in range(G)]
        eng.sync()
        assert all(_same_out(res[i], single[i]) and _same_out(res[i], flat[i]) for i in range(G))
        gouts = [_t(rng.standard_normal((B, 2)).astype(F32)) for _ in range(G)]
        z = lambda ts: [torch.full_like(t, SENTINEL) for t in ts]
        gw, gb, gx2 = [z(w) for w in wds], [z(b) for b in bds], z(x2s)
        eng.mlp_group_backward(gouts, rows, wds, bds, [r.out for r in res], wg, x2s=x2s, grad_weights=gw, grad_biases=gb, grad_x2s=gx2, split=True)
        for i in range(G):
            sw, sb, sx2 = z(wds[i]), z(bds[i]), z([x2s[i]])[0]
            eng.mlp_backward(gouts[i], rows, wds[i], bds[i], single[i].out, wsingle[i], x2=x2s[i], grad_weights=sw, grad_biases=sb, grad_x2=sx2, split=True)
            eng.sync()
            assert all(mr.same_bits(_h(a), _h(b)) for a, b in zip(gw[i] + gb[i] + [gx2[i]], sw + sb + [sx2])), (raw, P, i)


# ------------------------------------------------------------------------------------------------- the backward
def _backward_pair(ctx, rng, B, widths, f2, act, out_act=None, accumulate_at=None):
    """gradients of the split call and of the flat call on the rebuilt rows: ([dW..., db..., dx2], the same of the flat call)"""
    import torch
    eng = ctx.eng
    rows = _t(ctx.rows(rng, B))
    x2 = _t(rng.standard_normal((B, f2)).astype(F32)) if f2 else None
    ws, bs, wd, bd = _net(rng, ctx.flat + f2, widths)
    gout = _t(rng.standard_normal((B, widths[-1])).astype(F32))
    sides = []
    for split in (True, False):
        x = rows if split else ctx.flat_rows(rows)
        gw, gb = [torch.full_like(w, SENTINEL) for w in wd], [torch.full_like(b, SENTINEL) for b in bd]
        gx2 = torch.full_like(x2, SENTINEL) if f2 else None
        cuts = [(0, B)] if accumulate_at is None or not split else [(0, accumulate_at), (accumulate_at, B)]
        for k, (lo, hi) in enumerate(cuts):
            sl = slice(lo, hi)
            work = torch.empty(eng.mlp_workspace(hi - lo, widths, True), dtype=torch.uint8, device="cuda")
            fw = eng.mlp_forward(x[sl], wd, bd, hidden_activation=act, out_activation=out_act, x2=None if x2 is None else x2[sl], workspace=work, keep_hidden=True, split=split)
            eng.mlp_backward(gout[sl], x[sl], wd, bd, fw.out, work, hidden_activation=act, out_activation=out_act, x2=None if x2 is None else x2[sl], grad_weights=gw,
                             grad_biases=gb, grad_x2=None if gx2 is None else gx2[sl], accumulate=k > 0, split=split)
        eng.sync()
        sides.append([_h(t) for t in gw + gb + ([gx2] if f2 else [])])
    return sides, (rows, x2, ws, bs, gout)


@pytest.mark.parametrize("raw,P", CONFIGS)
def test_the_backward_equals_the_flat_calls(raw, P):
    ctx = _ctx_of(raw, P)
    rng = np.random.default_rng(7 + P)
    for B, widths, f2, act, out_act in ((1, [5], 0, "relu", None), (17, [17, 9, 3], 1, "tanh", "tanh"), (65, [33, 16, 2], 3, "relu", None), (257, [16, 5], 0, "relu", "relu")):
        (got, ref), (rows, x2, ws, bs, gout) = _backward_pair(ctx, rng, B, widths, f2, act, out_act)
        assert len(got) == 2 * len(widths) + (1 if f2 else 0)
        assert all(mr.same_bits(a, b) for a, b in zip(got, ref)), (B, widths, f2)
        assert not any((a == SENTINEL).any() for a in got)
        if B == 17 and act == "relu" or B == 1:                                 # the restatement where no library tanh is involved
            out, hid = msr.forward(_h(rows), ctx.series, raw, P, ws, bs, hidden_act=act, out_act=out_act, x2=None if x2 is None else _h(x2))
            dx2, dws, dbs = msr.backward(_h(gout), _h(rows), ctx.series, raw, P, ws, hid, out, hidden_act=act, out_act=out_act, x2=None if x2 is None else _h(x2))
            assert all(mr.same_bits(a, b) for a, b in zip(got, dws + dbs + ([dx2] if f2 else [])))


def test_accumulating_over_two_row_ranges_equals_the_one_call():
    for raw, P in (("mod", 13), ("raw", 13)):
        ctx = _ctx_of(raw, P)
        (got, ref), _ = _backward_pair(ctx, np.random.default_rng(3), 257, [19, 8, 2], 1, "relu", accumulate_at=100)
        assert all(mr.same_bits(a, b) for a, b in zip(got, ref)), (raw, P)      # [0, 100) then [100, 257) accumulated, against one flat call


def test_train_mlp_and_its_group_under_autograd():
    import torch
    from torch import nn
    from rl_ptg_amd import TrainMLP, TrainMLPGroup
    ctx = _ctx_of("mod", 13)
    eng = ctx.eng
    rng = np.random.default_rng(21)
    B = 65
    rows = _t(ctx.rows(rng, B)).requires_grad_(True)         # asks for a gradient and gets None
    flat = ctx.flat_rows(rows.detach())
    torch.manual_seed(3)
    make = lambda: nn.Sequential(nn.Linear(41, 33), nn.Tanh(), nn.Linear(33, 1)).cuda()
    mods = [make(), make()]
    target = _t(rng.standard_normal((B, 1)).astype(F32))
    grads = {}
    for obs, x in (("split", rows), ("flat", flat)):
        act = torch.linspace(-1, 1, B, device="cuda").view(B, 1).clone().requires_grad_(True)
        for m in mods:
            m.zero_grad(set_to_none=True)
        net = TrainMLP(eng, mods[0], batch=80, obs=obs)
        loss = ((net(x, x2=act) - target) ** 2).mean()
        loss.backward()
        eng.sync()
        single = [_h(p.grad) for p in net.parameters()] + [_h(act.grad)]
        assert (rows.grad is None) and net.grad_input.shape == ((80, 1) if obs == "split" else (80, 41))
        for m in mods:
            m.zero_grad(set_to_none=True)
        act2 = act.detach().clone().requires_grad_(True)
        grp = TrainMLPGroup(eng, mods, batch=80, obs=obs)
        q0, q1 = grp(x, x2=act2)
        (((q0 - target) ** 2).mean() + ((q1 + target) ** 2).mean()).backward()
        eng.sync()
        grads[obs] = single, [_h(p.grad) for p in grp.parameters()] + [_h(act2.grad)]
        assert all(mr.same_bits(a, b) for a, b in zip(single[:4], grads[obs][1][:4]))          # the group's first member is the single net
    for a, b in zip(grads["split"], grads["flat"]):
        assert len(a) == len(b) and all(mr.same_bits(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------- invalid indices
@pytest.mark.parametrize("raw,P", [("mod", 13), ("raw", 13), ("raw", 1)])
def test_an_invalid_index_is_clamped_poisons_its_row_alone_and_is_reported_once(raw, P):
    """One row each with -1, last valid + 1, 0.5 and NaN as the hour index (for 'raw' as the day index too) among valid rows: those rows
    are NaN, every other row keeps its bits, ptg_sync returns PTG_E_INDEX once and 0 afterwards; in the backward dW and db are NaN.  The
    load behind such an index is clamped into the series: 2^24, 1e30 and -Inf are planted too."""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    ctx = _ctx_of(raw, P)
    eng = ctx.eng
    rng = np.random.default_rng(17)
    B = 70
    clean = ctx.rows(rng, B)
    rows = clean.copy()
    planted = {5: (14, -1.0), 17: (14, ctx.lh + 1.0), 33: (14, 0.5), 34: (14, np.nan), 50: (14, 2.0 ** 24), 51: (14, 1e30), 52: (14, -np.inf)}
    if raw == "raw":
        planted.update({9: (15, -1.0), 20: (15, ctx.ld + 1.0), 40: (15, 0.5), 41: (15, np.nan)})
    else:
        rows[3, 15], rows[4, 15] = np.nan, -7.0                                # 'mod' never reads the day index
    for b, (c, v) in planted.items():
        rows[b, c] = v
    bad = np.zeros(B, bool)
    bad[list(planted)] = True
    assert np.array_equal(msr.invalid_rows(rows, ctx.series, raw, P), bad)
    ws, bs, wd, bd = _net(rng, ctx.flat, [19, 9, 3])
    eng.sync()
    for route in ("narrow", "wide"):
        work = torch.empty(eng.mlp_workspace(B, [19, 9, 3], True), dtype=torch.uint8, device="cuda")
        res = eng.mlp_forward(_t(rows), wd, bd, workspace=work, keep_hidden=True, split=True, _route=route)
        with pytest.raises(PtgError) as e:
            eng.sync()
        assert e.value.code == _lib.E_INDEX and "split row" in str(e.value)
        eng.sync()                                                              # once
        out = _h(res.out)
        ref = eng.mlp_forward(_t(clean), wd, bd, split=True)
        eng.sync()
        assert np.isnan(out[bad]).all() and np.isfinite(out[~bad]).all()
        assert mr.same_bits(out[~bad], _h(ref.out)[~bad]), route
        assert mr.same_bits(out, msr.forward(rows, ctx.series, raw, P, ws, bs)[0])
    # the backward: the gradient of a loss on NaN outputs is NaN in those rows
    gout = torch.where(torch.isnan(res.out), res.out, torch.ones_like(res.out))
    gw, gb = [torch.zeros_like(w) for w in wd], [torch.zeros_like(b) for b in bd]
    eng.mlp_backward(gout, _t(rows), wd, bd, res.out, work, grad_weights=gw, grad_biases=gb, split=True)
    with pytest.raises(PtgError) as e:
        eng.sync()
    assert e.value.code == _lib.E_INDEX
    eng.sync()
    assert all(np.isnan(_h(t)).all() for t in gw + gb)
    # a valid batch afterwards: no error left behind
    eng.mlp_forward(_t(clean), wd, bd, split=True)
    eng.sync()


# ------------------------------------------------------------------------------------------------- end to end
def test_twin_engines_end_to_end():
    """Twin engines with the same seed, one sb3_flat and one split, three market sets: a rollout of T = 3 at N = 65; DeviceMLP on the
    [T N, 16] rows against DeviceMLP on the [T N, 40] rows; minibatches over the split buffer into TrainMLP(obs="split") against the flat
    twin's gradients; a DeviceReplayBuffer of split rows whose samples go through DeviceMLPGroup(obs="split")."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, DeviceMLPGroup, TrainMLP
    from rl_ptg_amd.replay import DeviceReplayBuffer
    T, N = 3, 65
    a, b = _Ctx("mod", 13, n=N, layout="split"), _Ctx("mod", 13, n=N, layout="sb3_flat")
    prev = {}
    for c in (a, b):
        c.eng.set_market_assignment(np.arange(N) % 3)
        c.eng.set_episode_plan(c.spec.eps_ind, N, N)
        c.eng.set_noise_rng(seed=4)
        prev[c] = c.eng.reset().clone()
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    acts = torch.randint(0, 5, (T, N), dtype=torch.int32, device="cuda", generator=g)
    (so, sr, sd), (fo, fr, fd) = a.eng.rollout(acts), b.eng.rollout(acts)
    a.eng.sync(); b.eng.sync()
    assert so.shape == (T, N, 16) and fo.shape == (T, N, 40) and torch.equal(sr, fr)
    assert np.array_equal(_h(a.flat_rows(so)).view(np.int32), _h(fo).view(np.int32))          # the premise: the rebuilt rows ARE the flat twin's
    assert len(set(_h(so[..., 14]).astype(int).ravel() // a.nh)) == 3                          # all three sets
    torch.manual_seed(5)
    pi = nn.Sequential(nn.Linear(40, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 5)).cuda()
    ys = DeviceMLP(a.eng, pi, batch=T * N, obs="split")(so.view(T * N, 16))
    yf = DeviceMLP(b.eng, pi, batch=T * N)(fo.view(T * N, 40))
    a.eng.sync(); b.eng.sync()
    assert np.array_equal(_h(ys).view(np.int32), _h(yf).view(np.int32))
    # minibatches -> TrainMLP
    perm = torch.randperm(T * N, device="cuda", generator=g)
    adv = torch.randn((T, N), device="cuda", generator=g)
    grads = []
    for c, obs, kind in ((a, so, "split"), (b, fo, "flat")):
        net = TrainMLP(c.eng, pi, batch=64, obs=kind)
        mine = []
        for x, (w,) in c.eng.minibatches(perm, 64, obs=obs, columns=[adv]):
            pi.zero_grad(set_to_none=True)
            (net(x) * w[:, None]).sum().backward()
            c.eng.sync()
            mine.append([_h(p.grad).copy() for p in net.parameters()])
        grads.append(mine)
    assert len(grads[0]) == 4 and all(mr.same_bits(u, v) for m0, m1 in zip(*grads) for u, v in zip(m0, m1))
    # the replay buffer holds split rows; its samples go through a group
    qf = [nn.Sequential(nn.Linear(41, 33), nn.ReLU(), nn.Linear(33, 1)).cuda() for _ in range(2)]
    idx = torch.randint(0, T * N, (50,), device="cuda", generator=g)
    qs = []
    for c, obs, kind in ((a, so, "split"), (b, fo, "flat")):
        rb = DeviceReplayBuffer(c.eng, T * N)
        rb.add(prev[c], obs, sr, sd, actions=acts.long())
        s = rb.sample(idx=idx)
        assert s.observations.shape == (50, 16 if kind == "split" else 40)
        qs.append([_h(q).copy() for q in DeviceMLPGroup(c.eng, qf, batch=50, obs=kind)(s.observations, x2=s.actions.float())])
        c.eng.sync()
    assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(*qs))
    a.eng.close(); b.eng.close()


# ------------------------------------------------------------------------------------------------- capture
def test_one_captured_collect_step_against_the_eager_flat_twin():
    """step -> DeviceMLP(obs="split") -> act_categorical at 64 envs, captured once on a side stream at the default hardware-queue setting
    and replayed three times with the weights rewritten in place; a flat twin engine runs the same loop eagerly: every replay's logits
    and actions are the twin's, bit for bit"""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP
    N = 64
    a, b = _Ctx("mod", 13, n=N, layout="split"), _Ctx("mod", 13, n=N, layout="sb3_flat")
    for c in (a, b):
        c.eng.set_market_assignment(np.arange(N) % 3)
        c.eng.set_episode_plan(c.spec.eps_ind, N, N)
        c.eng.set_noise_rng(seed=4)
        c.eng.set_replay_proof(True)
    torch.manual_seed(8)
    pi = nn.Sequential(nn.Linear(40, 37), nn.Tanh(), nn.Linear(37, 37), nn.Tanh(), nn.Linear(37, 5)).cuda()
    ps, pf = DeviceMLP(a.eng, pi, batch=N, obs="split"), DeviceMLP(b.eng, pi, batch=N)
    loops = []
    for c, policy in ((a, ps), (b, pf)):
        eng = c.eng
        prev = eng.reset().clone()
        obs, rew, done, fin = eng.alloc_obs(zero=True), torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), eng.alloc_obs(zero=True)
        res = eng.act_categorical(policy(prev), None, deterministic=True)

        def one(eng=eng, policy=policy, prev=prev, obs=obs, rew=rew, done=done, fin=fin, res=res):
            eng.act_categorical(policy(prev), None, deterministic=True, out=res)
            eng.step(res.actions, obs, rew, done, final_obs=fin)
            prev.copy_(obs)

        loops.append((one, res, rew))
    (one_s, res_s, rew_s), (one_f, res_f, rew_f) = loops

    def same(k):
        a.eng.sync(); b.eng.sync()
        assert np.array_equal(_h(ps.out).view(np.int32), _h(pf.out).view(np.int32)), k
        assert torch.equal(res_s.actions, res_f.actions) and torch.equal(rew_s, rew_f), k

    one_s(); one_f()                                         # eager once: code objects are loaded before the capture
    same(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one_s()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()                                 # a capture records and runs nothing: the twin does not move
    views = []
    for k in (1, 2, 3):
        with torch.no_grad():
            for p in pi.parameters():
                p.mul_(1.0 - 0.1 * k).add_(0.01 * k)         # in place: the graph holds these addresses
        graph.replay()
        torch.cuda.synchronize()
        one_f()
        same(k)
        views.append(_h(ps.out).copy())
    assert not np.array_equal(views[0], views[1]) and not np.array_equal(views[1], views[2])
    a.eng.note_replays(3 - 1)
    a.eng.sync()
    a.eng.close(); b.eng.close()


def test_no_host_synchronisation_and_no_allocation_across_a_call():
    """A condition, not a timing (tests/test_mlp.py has the flat twin of this test): the stream is busy with milliseconds of fused steps
    before the calls and still busy when they have returned; with out= and workspaces the allocator hands out nothing during them."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="split")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    rng = np.random.default_rng(1)
    ws, bs, wd, bd = _net(rng, 40, [64, 5])
    out, gout = torch.empty((n, 5), device="cuda"), torch.ones((n, 5), device="cuda")
    work = torch.empty(eng.mlp_workspace(n, [64, 5], True), dtype=torch.uint8, device="cuda")
    bwork = torch.empty(eng.mlp_backward_workspace(n, [64, 5]), dtype=torch.uint8, device="cuda")
    gw, gb = [torch.empty_like(w) for w in wd], [torch.empty_like(b) for b in bd]
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")

    def ops():
        res = eng.mlp_forward(obs[T - 1], wd, bd, out=out, workspace=work, keep_hidden=True, split=True)
        eng.mlp_backward(gout, obs[T - 1], wd, bd, out, work, grad_weights=gw, grad_biases=gb, backward_workspace=bwork, split=True)
        return res

    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
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
    assert allocs_after == allocs, "a call with out= and workspaces allocated device memory"
    eng.sync()
    pick = np.r_[0:40, n - 40:n]
    rows = _h(obs[T - 1])[pick]
    ref_out, ref_hid = msr.forward(rows, eng.market_feature_series(), "mod", 13, ws, bs)
    assert mr.same_bits(_h(res.out)[pick], ref_out) and mr.same_bits(_h(res.hidden[0])[pick], ref_hid[0])
    eng.close()


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    ctx = _ctx_of("mod", 13)
    eng = ctx.eng
    B = 20
    L, h, stream = eng._L, eng._h, eng._stream()
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    x, x2, out, gout = torch.zeros(B, 18, device="cuda"), full(B, 2), full(B, 6), full(B, 5)
    w, b = [full(8, 44), full(8, 8), full(5, 8)], [full(8), full(8), full(5)]
    dw, db, dx, dx2 = [full(8, 44), full(8, 8), full(5, 8)], [full(8), full(8), full(5)], full(B, 42), full(B, 2)
    need, needb = eng.mlp_workspace(B, [8, 8, 5], True), eng.mlp_backward_workspace(B, [8, 8, 5])
    ws, bws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((needb,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    S, K = _lib.MLP_SPLIT_INPUT, _lib.MLP_KEEP_HIDDEN

    def fill(d, a):
        for k, v in a.items():
            if isinstance(v, (list, tuple)):
                for j, e in enumerate(v):
                    getattr(d, k)[j] = e
            else:
                setattr(d, k, v)
        return d

    def fwd(**kw):
        a = dict(batch=B, n_layers=3, flags=S | K, hidden_act=_lib.MLP_TANH, out_act=_lib.MLP_NONE, f1=40, f2=1, x_dev=p(x), x_s_n=18, x2_dev=p(x2), x2_s_n=2,
                 w_dev=[p(t) for t in w], w_s_n=[44, 8, 8], b_dev=[p(t) for t in b], width=[8, 8, 5], out_dev=p(out), out_s_n=6, ws_dev=p(ws), ws_bytes=need)
        a.update(kw)
        return a

    def bwd(f=None, **kw):
        d = fill(_lib.PtgMlpBwd(), dict(dict(gout_dev=p(gout), gout_s_n=5, dw_dev=[p(t) for t in dw], dw_s_n=[44, 8, 8], db_dev=[p(t) for t in db], dx2_dev=p(dx2), dx2_s_n=2,
                                             bws_dev=p(bws), bws_bytes=needb, flags=0), **kw))
        fill(d.fwd, fwd(**(f or {})))
        return d

    E = _lib.E_INVALID
    cases = [(fwd(f1=39, f2=2), "f1"), (fwd(f1=41, f2=0, x2_dev=None), "f1"), (fwd(f1=16), "f1"), (fwd(x_s_n=15), "x_s_n"), (fwd(x_s_n=0), "x_s_n"), (fwd(x_dev=None), "x_dev")]
    for k, (a, word) in enumerate(cases):
        assert L.ptg_mlp_forward(h, C.byref(fill(_lib.PtgMlp(), a)), stream) == E, k
        msg = L.ptg_last_error(h).decode()
        assert msg.startswith("ptg_mlp_forward:") and word in msg, (k, msg)
        assert L.ptg_mlp_backward(h, C.byref(bwd(f=a)), stream) == E and word in L.ptg_last_error(h).decode(), k
        pair = (_lib.PtgMlp * 2)(fill(_lib.PtgMlp(), fwd()), fill(_lib.PtgMlp(), a))
        assert L.ptg_mlp_group_forward(h, pair, 2, stream) == E and "net 1" in L.ptg_last_error(h).decode(), k
    assert L.ptg_mlp_backward(h, C.byref(bwd(dx_dev=p(dx), dx_s_n=42)), stream) == E and "dx_dev" in L.ptg_last_error(h).decode()
    assert L.ptg_mlp_backward(h, C.byref(bwd(flags=S)), stream) == E and "unknown flag" in L.ptg_last_error(h).decode()          # the backward's own flags
    two = (_lib.PtgMlpBwd * 2)(bwd(), bwd(dx_dev=p(dx), dx_s_n=42))
    assert L.ptg_mlp_group_backward(h, two, 2, stream) == E and "net 1" in L.ptg_last_error(h).decode() and "dx_dev" in L.ptg_last_error(h).decode()
    mixed = (_lib.PtgMlp * 2)(fill(_lib.PtgMlp(), fwd()), fill(_lib.PtgMlp(), fwd(flags=K, x_dev=p(dx), x_s_n=42)))      # in a group the flag must agree
    assert L.ptg_mlp_group_forward(h, mixed, 2, stream) == E and "flags" in L.ptg_last_error(h).decode()
    assert torch.cuda.current_stream().query() is True        # nothing was enqueued
    torch.cuda.synchronize()
    untouched = [out, dx, dx2] + dw + db
    assert all(bool((t == SENTINEL).all()) for t in untouched) and bool((ws == 0x5A).all()) and bool((bws == 0x5A).all())
    # the good descriptors run: rows of zeros index hour 0, day 0
    assert L.ptg_mlp_forward(h, C.byref(fill(_lib.PtgMlp(), fwd())), stream) == 0
    assert L.ptg_mlp_backward(h, C.byref(bwd()), stream) == 0
    eng.sync()
    assert bool((out[:, :5] != SENTINEL).all()) and bool((out[:, 5] == SENTINEL).all()) and bool((dx == SENTINEL).all())
    assert bool((dx2[:, 0] != SENTINEL).all()) and bool((dx2[:, 1] == SENTINEL).all())
    assert bool((dw[0][:, :41] != SENTINEL).all()) and bool((dw[0][:, 41:] == SENTINEL).all())
