"""The reward-normalisation kernels (k_vn_moments, k_vn_merge, k_vn_scan, k_vn_norm, k_vn_clear_done behind ptg_vn_*) on synthetic
[T, N] rewards and done flags fed straight to the handle -- no env rollout -- against the restated SB3 algorithm
(oracle/vecnormalize_oracle.py), at the shapes where a reduction or a scan goes wrong: wave edges (64 envs), more waves than
k_vn_merge has lanes (N > 4 096), the 8-step load batches and 64-step LDS tiles of k_vn_moments, empty lanes and multi-step
chunks of k_vn_scan (T <= 64 / T > 64), calls split and resumed, sharded handles, frozen statistics and NaN rewards.

Tolerances (the largest observed margin of each group is written to $PTG_VN_MARGIN_LOG when set):
- returns: the device runs returns * gamma + reward per env in the oracle's operand order, in float64, without contraction
  (-ffp-contract=off) -- the same two roundings per step, so equal to 1e-12 relative (in practice bit for bit);
- statistics and float64 outputs: the per-step batch moments are summed in another order (per-wave serial sums merged by Chan's
  formula vs numpy's pairwise mean and two-pass variance), and the running moments are merged as a prefix scan rather than one
  step after another.  Every merge adds non-negative M2 terms, so the error stays a few ulp times the number of merges on the
  longest path (< 1e4 here): 1e-10 relative.  The mean is a weighted average of returns of either sign, so its error is held
  against the largest |return| it averaged (1e-10 of that), not against itself;
- float32 outputs: one rounding of a float64 quotient that is within 1e-10 of the oracle's, so within 1 float32 ulp of
  float32(oracle);
- clipped outputs are the clip bound exactly in both; an exact zero reward gives an exact zero in both.
"""
import atexit
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vecnormalize_oracle as vo          # noqa: E402
from rl_ptg_amd import dist as ptg_dist   # noqa: E402

pytestmark = pytest.mark.gpu

RTOL_STATS = 1e-10
RTOL_OUT64 = 1e-10
RTOL_RET = 1e-12
SB3 = dict(gamma=0.99, epsilon=1e-8, clip_reward=10.0)
E_INVALID = -1

_margins = {}


def _margin(group, value):
    if not _margins and os.environ.get("PTG_VN_MARGIN_LOG"):
        atexit.register(_write_margins)
    _margins[group] = max(float(value), _margins.get(group, 0.0))


def _write_margins():
    with open(os.environ["PTG_VN_MARGIN_LOG"], "a") as f:
        for g, v in sorted(_margins.items()):
            f.write(f"{g}\t{v:.3e}\n")


_spec = None


def _engine(n, out_dtype):
    """A handle of n envs; only its n and out_dtype matter to the ptg_vn_* calls."""
    global _spec
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if _spec is None:
        _spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=1, train_steps=400000)
    return HipEngine(_spec.consts, _spec.tables, _spec.markets, n, device=0, out_dtype=out_dtype, obs_layout="row")


def _rewards(kind, T, N, rng):
    if kind == "offset":                                  # mean 1e3, sd 10: the returns' M2 cancels against a large mean
        return rng.normal(1e3, 10.0, (T, N))
    if kind == "const_cols":                              # every 5th env gets one constant reward for the whole window
        r = rng.normal(0.0, 1.0, (T, N))
        r[:, ::5] = rng.uniform(-3.0, 3.0, N)[::5]
        return r
    if kind == "zeros":                                   # batch variance 0: the denominator goes to sqrt(epsilon) from var 1
        return np.zeros((T, N))
    if kind == "spikes":                                  # rare +-1e4 rewards, two of them on the first step: both clip bounds
        r = rng.normal(0.0, 1.0, (T, N))
        m = rng.random((T, N)) < 2e-3
        r[m] = rng.choice([-1e4, 1e4], int(m.sum()))
        r[0, 0], r[0, min(1, N - 1)] = 1e4, -1e4
        return r
    raise ValueError(kind)


def _dones(kind, T, N, rng):
    d = np.zeros((T, N), np.uint8)
    if kind == "edges":                                   # the whole batch, on the first step, both sides of a tile edge, the last step
        for t in (0, 63, 64, T - 1):
            if t < T:
                d[t] = 1
    elif kind == "bernoulli":                             # staggered per env
        d[:] = rng.random((T, N)) < 0.02
    elif kind == "every":
        d[:] = 1
    elif kind != "none":
        raise ValueError(kind)
    return d


def _inputs(T, N, out_dtype, rkind="offset", dkind="bernoulli", seed=0):
    """Device tensors [T, N] (rewards in the handle's dtype, uint8 dones) and the float64 values the oracle sees."""
    import torch
    rng = np.random.default_rng(seed)
    r = _rewards(rkind, T, N, rng).astype(out_dtype)
    d = _dones(dkind, T, N, rng)
    return torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda(), r.astype(np.float64), d


def _oracle(ora, r64, d):
    """Normalised rewards [T, N] and the largest |return| the running mean averaged."""
    out = np.empty_like(r64)
    big = 0.0
    for t in range(len(r64)):
        if ora.training:                                  # the returns this step averages (NaN never wins max())
            big = max(big, float(np.max(np.abs(ora.returns * ora.gamma + r64[t]))))
        out[t] = ora.step(r64[t], d[t])
    return out, big


def _check_out(got, exp, out_dtype, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == exp.shape
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    g, e = got[~nan].astype(np.float64), exp[~nan]
    if out_dtype == "float32":
        e32 = e.astype(np.float32)
        ulp = np.spacing(np.abs(e32)).astype(np.float64)
        err = np.abs(g - e32.astype(np.float64)) / ulp
        if err.size:
            _margin("out_f32_ulp", err.max())
            worst = int(np.argmax(err))
            assert err[worst] <= 1.0, f"{what}: {err[worst]:.2f} ulp at flat index {worst}: {g[worst]!r} vs {e[worst]!r}"
    else:
        err = np.abs(g - e) / np.maximum(np.abs(e), 1e-300)
        if err.size:
            _margin("out_f64_rel", err.max())
        np.testing.assert_allclose(g, e, rtol=RTOL_OUT64, atol=0, err_msg=what)


def _check_state(eng, ora, big, what=""):
    st, ret = eng.vn_get()
    rs = ora.ret_rms
    if np.isnan(rs.mean):
        assert np.isnan(st["mean"]) and np.isnan(st["var"]), what
    else:
        np.testing.assert_allclose(st["count"], rs.count, rtol=RTOL_STATS, atol=0, err_msg=what)
        np.testing.assert_allclose(st["var"], rs.var, rtol=RTOL_STATS, atol=0, err_msg=what)
        assert abs(st["mean"] - rs.mean) <= RTOL_STATS * max(big, abs(rs.mean)), (what, st["mean"], rs.mean, big)
        _margin("stats_rel", max(abs(st["count"] / rs.count - 1), abs(st["var"] / rs.var - 1),
                                 abs(st["mean"] - rs.mean) / max(big, abs(rs.mean), 1e-300)))
    np.testing.assert_allclose(ret, ora.returns, rtol=RTOL_RET, atol=0, equal_nan=True, err_msg=what)
    ok = ~np.isnan(ora.returns) & (ora.returns != 0)
    if ok.any():
        _margin("returns_rel", np.max(np.abs(ret[ok] / ora.returns[ok] - 1)))
    return st, ret


def _run(N, T, out_dtype, rkind="offset", dkind="bernoulli", seed=0, hyper=SB3):
    eng = _engine(N, out_dtype)
    try:
        r, d, r64, dn = _inputs(T, N, out_dtype, rkind, dkind, seed)
        eng.vn_init(**hyper)
        got = eng.vn_normalize(r, d)
        ora = vo.RewardNormalizer(N, **hyper)
        exp, big = _oracle(ora, r64, dn)
        what = f"N={N} T={T} {out_dtype} {rkind}/{dkind} {hyper}"
        _check_out(got, exp, out_dtype, what)
        _check_state(eng, ora, big, what)
        return exp
    finally:
        eng.close()


DTYPES = ["float32", "float64"]


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 4095, 4096, 4097, 65536, 65537])
def test_n_sweep(N, out_dtype):
    """Ragged and full last waves, one wave and many; N > 4 096 is more than 64 waves, so k_vn_merge's lanes take two or more."""
    _run(N, 65, out_dtype, seed=N)


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 7, 8, 9, 63, 64, 65, 129, 4097, 8193])
def test_t_sweep(T, out_dtype):
    """8-step load batches, 64-step LDS tiles, k_vn_scan with empty lanes (T <= 64, and T = 65: lanes 33..63) and chunks of
    several steps (T > 64), at N = 4 097 (65 waves, the last with one env).  Dones on the edges of the tiles and at T - 1."""
    _run(4097, T, out_dtype, dkind="edges", seed=T)


PATTERNS = [
    ("offset", "none", SB3),
    ("offset", "edges", SB3),
    ("offset", "every", SB3),
    ("const_cols", "bernoulli", SB3),
    ("zeros", "edges", SB3),
    ("zeros", "none", dict(gamma=0.99, epsilon=0.0, clip_reward=10.0)),
    ("spikes", "bernoulli", SB3),
    ("spikes", "none", dict(gamma=0.5, epsilon=1.0, clip_reward=0.5)),
    ("offset", "bernoulli", dict(gamma=0.0, epsilon=0.0, clip_reward=1e300)),
    ("offset", "edges", dict(gamma=1.0, epsilon=1.0, clip_reward=0.5)),
    ("const_cols", "every", dict(gamma=1.0, epsilon=0.0, clip_reward=1e300)),
    ("spikes", "edges", dict(gamma=0.0, epsilon=1e-8, clip_reward=10.0)),
]


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("rkind,dkind,hyper", PATTERNS, ids=[f"{r}-{d}-g{h['gamma']}-e{h['epsilon']}-c{h['clip_reward']}" for r, d, h in PATTERNS])
def test_reward_done_and_hyperparameter_patterns(rkind, dkind, hyper, out_dtype):
    exp = _run(4097, 130, out_dtype, rkind, dkind, seed=7, hyper=hyper)
    c = hyper["clip_reward"]
    if rkind == "spikes":                                 # the clip engages on both signs
        assert (exp == c).any() and (exp == -c).any()
    if c == 1e300:
        assert np.abs(exp).max() < c


def test_invalid_arguments():
    import torch
    eng = _engine(64, "float32")
    try:
        L, h, s = eng._L, eng._h, eng._stream()
        r = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
        d = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
        o = torch.empty_like(r)
        rp, dp, op = C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(o.data_ptr())
        # before ptg_vn_init
        assert L.ptg_vn_batch_moments(h, rp, dp, 4, None, s) == E_INVALID
        assert L.ptg_vn_apply(h, rp, 4, None, op, 1, s) == E_INVALID
        assert L.ptg_vn_clear_done(h, dp, 4, s) == E_INVALID
        nan = float("nan")
        for g, e, c in [(-0.1, 1e-8, 10.0), (nan, 1e-8, 10.0), (0.99, -1e-8, 10.0), (0.99, nan, 10.0), (0.99, 1e-8, 0.0),
                        (0.99, 1e-8, -1.0), (0.99, 1e-8, nan)]:
            assert L.ptg_vn_init(h, g, e, c) == E_INVALID, (g, e, c)
        assert L.ptg_vn_init(h, 0.99, 1e-8, 10.0) == 0
        assert L.ptg_vn_batch_moments(h, rp, dp, 0, None, s) == E_INVALID
        assert L.ptg_vn_apply(h, rp, 0, None, op, 1, s) == E_INVALID
        assert L.ptg_vn_clear_done(h, dp, 0, s) == E_INVALID
        assert L.ptg_vn_batch_moments(h, rp, dp, 4, None, s) == 0
        assert L.ptg_vn_apply(h, rp, 4, None, op, 1, s) == 0
        eng.sync()
    finally:
        eng.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_split_calls_equal_one_call(out_dtype):
    """T = 4 162 in one call, and as calls of 1, 4 097 and 64 steps (the scratch grows, then is reused): both against the oracle;
    the returns bit for bit equal (a per-env sequential recurrence), the statistics to rounding (the scan's grouping differs)."""
    import torch
    N, T = 4097, 1 + 4097 + 64
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "bernoulli", seed=11)
    ora = vo.RewardNormalizer(N)
    exp, big = _oracle(ora, r64, dn)
    one, split = _engine(N, out_dtype), _engine(N, out_dtype)
    try:
        one.vn_init()
        got1 = one.vn_normalize(r, d)
        split.vn_init()
        got2 = torch.cat([split.vn_normalize(r[a:b], d[a:b]) for a, b in ((0, 1), (1, 4098), (4098, T))])
        _check_out(got1, exp, out_dtype, "one call")
        _check_out(got2, exp, out_dtype, "split calls")
        st1, ret1 = _check_state(one, ora, big, "one call")
        st2, ret2 = _check_state(split, ora, big, "split calls")
        assert np.array_equal(ret1, ret2)
    finally:
        one.close(); split.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_resume_from_set_statistics(out_dtype):
    """A fresh handle given the oracle's mid-run state by vn_set (count 1e7, far from the initial 1e-4), then continued."""
    N, T = 4097, 200
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "bernoulli", seed=12)
    ora = vo.RewardNormalizer(N)
    _oracle(ora, r64[:100], dn[:100])
    ora.ret_rms.count = 1e7
    eng = _engine(N, out_dtype)
    try:
        eng.vn_init()
        eng.vn_set(stats=dict(mean=float(ora.ret_rms.mean), var=float(ora.ret_rms.var), count=ora.ret_rms.count), returns=ora.returns)
        got = eng.vn_normalize(r[100:].contiguous(), d[100:].contiguous())
        exp, big = _oracle(ora, r64[100:], dn[100:])
        _check_out(got, exp, out_dtype, "resumed")
        _check_state(eng, ora, big, "resumed")
    finally:
        eng.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_train_frozen_train(out_dtype):
    """Training, then frozen statistics over a window with staggered and whole-batch dones (returns[done] = 0 all the same, as
    SB3's step_wait does), then training again from the cleared returns."""
    N, T = 4097, 300
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "bernoulli", seed=13)
    d[150] = 1; dn[150] = 1
    ora = vo.RewardNormalizer(N)
    eng = _engine(N, out_dtype)
    try:
        eng.vn_init()
        big = 0.0
        for a, b, training in ((0, 100, True), (100, 200, False), (200, T, True)):
            ora.training = training
            got = eng.vn_normalize(r[a:b].contiguous(), d[a:b].contiguous(), training=training)
            exp, bg = _oracle(ora, r64[a:b], dn[a:b])
            big = max(big, bg)
            _check_out(got, exp, out_dtype, f"steps {a}..{b} training={training}")
            st, ret = _check_state(eng, ora, big, f"after steps {a}..{b} training={training}")
            if not training:
                assert (ret == 0).all()                   # the whole batch ended an episode on step 150
    finally:
        eng.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_frozen_clears_only_finished_envs(out_dtype):
    """Frozen statistics over a window where only some envs finish: exactly those returns are zeroed, the others untouched."""
    N, T = 4097, 40
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "bernoulli", seed=14)
    ora = vo.RewardNormalizer(N)
    eng = _engine(N, out_dtype)
    try:
        eng.vn_init()
        eng.vn_normalize(r, d)
        _oracle(ora, r64, dn)
        _, ret0 = eng.vn_get()
        ora.training = False
        dw = np.zeros((9, N), np.uint8)
        dw[np.arange(N) % 9, np.arange(N)] = np.arange(N) % 3 == 0
        import torch
        got = eng.vn_normalize(r[:9].contiguous(), torch.from_numpy(dw).cuda(), training=False)
        exp, _ = _oracle(ora, r64[:9], dw)
        _check_out(got, exp, out_dtype, "frozen")
        _, ret = eng.vn_get()
        fin = dw.any(0)
        assert 0 < fin.sum() < N and (ret[fin] == 0).all() and np.array_equal(ret[~fin], ret0[~fin])
        np.testing.assert_allclose(ret, ora.returns, rtol=RTOL_RET, atol=0)
    finally:
        eng.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_null_moments_route_and_in_place(out_dtype):
    """The documented single-GPU C route (moments_dev = NULL in both calls) == HipEngine.vn_normalize bit for bit; out = rew
    (in place) == the out-of-place result bit for bit."""
    import torch
    N, T = 4097, 130
    r, d, r64, dn = _inputs(T, N, out_dtype, "spikes", "edges", seed=15)
    a, b, c = _engine(N, out_dtype), _engine(N, out_dtype), _engine(N, out_dtype)
    try:
        for e in (a, b, c):
            e.vn_init()
        o = torch.empty_like(r)
        L, h, s = a._L, a._h, a._stream()
        a._chk(L.ptg_vn_batch_moments(h, C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), T, None, s))
        a._chk(L.ptg_vn_apply(h, C.c_void_p(r.data_ptr()), T, None, C.c_void_p(o.data_ptr()), 1, s))
        ref = b.vn_normalize(r, d)
        inplace = r.clone()
        res = c.vn_normalize(inplace, d, out=inplace)
        assert res.data_ptr() == inplace.data_ptr()
        assert torch.equal(o, ref) and torch.equal(inplace, ref)
        sa, ra = a.vn_get()
        for e in (b, c):
            se, re_ = e.vn_get()
            assert se == sa and np.array_equal(re_, ra)
        ora = vo.RewardNormalizer(N)
        exp, big = _oracle(ora, r64, dn)
        _check_out(o, exp, out_dtype, "NULL moments")
        _check_state(a, ora, big, "NULL moments")
    finally:
        a.close(); b.close(); c.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_shards_equal_one_oracle_over_all_envs(out_dtype):
    """Three handles of 4 097, 65 and 1 envs (ragged shards, one wider than a wave): batch moments of each, merged in shard
    order (rl_ptg_amd.dist.merge_moments), applied on each == one oracle over the 4 163 concatenated envs; all three handles
    end with the same statistics."""
    import torch
    sizes, T = (4097, 65, 1), 150
    N = sum(sizes)
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "bernoulli", seed=16)
    engs = [_engine(n, out_dtype) for n in sizes]
    try:
        cols = np.cumsum((0,) + sizes)
        parts, moms = [], []
        for e, a, b in zip(engs, cols[:-1], cols[1:]):
            e.vn_init()
            rr, dd = r[:, a:b].contiguous(), d[:, a:b].contiguous()
            m = torch.empty((T, 3), dtype=torch.float64, device="cuda")
            e._chk(e._L.ptg_vn_batch_moments(e._h, C.c_void_p(rr.data_ptr()), C.c_void_p(dd.data_ptr()), T, C.c_void_p(m.data_ptr()), e._stream()))
            parts.append(rr); moms.append(m)
        merged = ptg_dist.merge_moments(torch.stack(moms)).contiguous()
        outs = []
        for e, rr in zip(engs, parts):
            o = torch.empty_like(rr)
            e._chk(e._L.ptg_vn_apply(e._h, C.c_void_p(rr.data_ptr()), T, C.c_void_p(merged.data_ptr()), C.c_void_p(o.data_ptr()), 1, e._stream()))
            outs.append(o)
        ora = vo.RewardNormalizer(N)
        exp, big = _oracle(ora, r64, dn)
        _check_out(torch.cat(outs, dim=1), exp, out_dtype, "shards")
        sts = []
        for e, a, b in zip(engs, cols[:-1], cols[1:]):
            st, ret = e.vn_get()
            sts.append(st)
            rs = ora.ret_rms
            np.testing.assert_allclose([st["count"], st["var"]], [rs.count, rs.var], rtol=RTOL_STATS, atol=0)
            assert abs(st["mean"] - rs.mean) <= RTOL_STATS * max(big, abs(rs.mean))
            np.testing.assert_allclose(ret, ora.returns[a:b], rtol=RTOL_RET, atol=0)
        assert sts[0] == sts[1] == sts[2]
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_nan_reward_propagates_like_np_clip(out_dtype):
    """One NaN reward at (t = 5, env 17): the oracle's np.clip keeps it, so env 17's return, the statistics and every output
    from step 5 on are NaN; fmin / fmax would have turned them into -clip_reward."""
    N, T = 65, 12
    r, d, r64, dn = _inputs(T, N, out_dtype, "offset", "none", seed=17)
    r[5, 17] = float("nan"); r64[5, 17] = np.nan
    eng = _engine(N, out_dtype)
    try:
        eng.vn_init()
        got = eng.vn_normalize(r, d).cpu().numpy()
        ora = vo.RewardNormalizer(N)
        with np.errstate(invalid="ignore"):
            exp, big = _oracle(ora, r64, dn)
        assert np.isnan(exp[5:]).all() and not np.isnan(exp[:5]).any()
        np.testing.assert_allclose(got, exp, rtol=RTOL_OUT64 if out_dtype == "float64" else 2e-7, atol=0, equal_nan=True)
        _check_out(got, exp, out_dtype, "NaN reward")
        st, ret = _check_state(eng, ora, big, "NaN reward")
        assert np.isnan(ret[17]) and not np.isnan(np.delete(ret, 17)).any()
    finally:
        eng.close()
