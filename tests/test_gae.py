"""ptg_gae / HipEngine.gae (include/ptg_env.h) -- the advantages and returns of a rollout on the device -- against the NumPy
restatement of SB3's RolloutBuffer.compute_returns_and_advantage (tests/gae_restatement.py, pinned by tests/test_gae_host.py).

Every comparison is bit for bit.  That is derived, not measured: the kernel runs the same IEEE-754 operations as NumPy does on
arrays of the same dtype, in the same order, each rounded once (no fused multiply-add), on the same float32 / float64 casts of
gamma and of the double product gamma * gae_lambda.  NaNs compare equal to NaNs at the same place (payloads are not compared);
everything else, signed zeros and infinities included, must have the same bits.  Inputs stay in the normal range (subnormal
handling is unspecified).  Synthetic [T, N] inputs are fed straight to a handle of N envs: only its n_envs matters to the call."""
import ctypes as C

import numpy as np
import pytest

import gae_restatement as gr

pytestmark = pytest.mark.gpu

A2C = (0.9393, 0.9819)               # the reference's config/config_agent.yaml
PPO = (0.973, 0.8002)
SB3_DEFAULT = (0.99, 0.95)
HYPERS = [A2C, PPO, SB3_DEFAULT, (1.0, 1.0), (0.0, 0.0), (0.9393, 0.0)]
DTYPES = ["float32", "float64"]
NS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 65536, 65537]
TS = [1, 7, 8, 9, 63, 64, 65, 129, 658]
PATTERNS = ["none", "all", "first", "last", "sync", "two_consecutive", "bernoulli"]
SENTINEL = -777.25

_spec = None


def _engine(n, out_dtype="float32"):
    global _spec
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if _spec is None:
        _spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=1, train_steps=400000)
    return HipEngine(_spec.consts, _spec.tables, _spec.markets, n, device=0, out_dtype=out_dtype, obs_layout="row")


def _dones(kind, T, N, rng):
    d = np.zeros((T, N), np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[T - 1] = 1
    elif kind == "sync":                                  # the whole batch on one step in the middle: a synchronised batch
        d[T // 2] = 1
    elif kind == "two_consecutive":
        d[T // 3] = 1
        d[min(T // 3 + 1, T - 1)] = 1
    elif kind == "bernoulli":
        d[:] = rng.random((T, N)) < 0.01
        d[d != 0] = rng.integers(1, 256, int(d.sum()))    # any non-zero byte is a done flag
    elif kind != "none":
        raise ValueError(kind)
    return d


def _inputs(T, N, dtype, dkind="bernoulli", seed=0):
    """host arrays rew, val [T, N], done [T, N] uint8, last_val [N] in `dtype`: rewards of both signs around an offset, values O(1)"""
    rng = np.random.default_rng([seed, T, N])
    rew = (rng.normal(0.3, 2.0, (T, N))).astype(dtype)
    val = rng.normal(0.0, 1.5, (T, N)).astype(dtype)
    last = rng.normal(0.0, 1.5, N).astype(dtype)
    return rew, val, _dones(dkind, T, N, rng), last


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _same_bits(got, exp, what=""):
    """NaN where the restatement has NaN; the same bits everywhere else"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    np.testing.assert_array_equal(got, exp, err_msg=what)          # NaNs equal NaNs; reports the mismatching elements
    nan = np.isnan(exp)
    iv = np.int32 if got.dtype == np.float32 else np.int64
    assert np.array_equal(got.view(iv)[~nan], exp.view(iv)[~nan]), what + ": equal values with different bits (a signed zero)"


def _run(eng, rew, val, done, last, gamma, lam, **kw):
    """HipEngine.gae on device copies of the host arrays -> host (adv, ret)"""
    import torch
    r, v, d, l = _dev(rew, val, done, last)
    adv, ret = eng.gae(r, v, d, l, gamma, lam, **kw)
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy()


def _check(eng, T, N, dtype, dkind, gamma, lam, seed=0):
    rew, val, done, last = _inputs(T, N, dtype, dkind, seed)
    adv, ret = _run(eng, rew, val, done, last, gamma, lam)
    e_adv, e_ret = gr.gae(rew, val, done, last, gamma, lam, dtype)
    what = f"T={T} N={N} {dtype} done={dkind} gamma={gamma} lambda={lam}"
    _same_bits(adv, e_adv, what + " adv")
    _same_bits(ret, e_ret, what + " ret")


def _ts_for(i):
    """The thinned product: the i-th N takes the i-th T and two more that rotate through the list; with ten N every T is met at
    least three times per dtype.  658 (the reference's A2C n_steps) always rides with the widest batches."""
    ts = {TS[i % len(TS)], TS[(i + 3) % len(TS)], TS[(2 * i + 5) % len(TS)]}
    if NS[i] >= 65536:
        ts.add(658)
    return sorted(ts)


def test_the_thinned_product_covers_every_edge():
    assert {t for i in range(len(NS)) for t in _ts_for(i)} == set(TS)


@pytest.mark.parametrize("i", range(len(NS)), ids=[f"N{n}" for n in NS])
def test_edges_of_wave_and_load_batch(i):
    """N at the wave (64) and 64-wave edges and past 65 536; T at the edges of the 16-step (float64) and 32-step (float32) load
    batches, of several batches, and at the reference's 658 -- staggered done flags, the reference's two pairs alternating"""
    N = NS[i]
    eng = _engine(N)
    for k, T in enumerate(_ts_for(i)):
        for dtype in DTYPES:
            _check(eng, T, N, dtype, "bernoulli", *(A2C, PPO)[k % 2], seed=i)
    eng.close()


@pytest.mark.parametrize("T", [15, 16, 17, 31, 32, 33])
def test_load_batch_edges(T):
    eng = _engine(130)
    for dtype in DTYPES:
        _check(eng, T, 130, dtype, "bernoulli", *PPO)
    eng.close()


@pytest.mark.parametrize("dkind", PATTERNS)
def test_done_patterns_and_hyper_parameters(dkind):
    N = 193
    eng = _engine(N)
    for T in (1, 50):
        for dtype in DTYPES:
            for gamma, lam in HYPERS:
                _check(eng, T, N, dtype, dkind, gamma, lam, seed=3)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_propagate_as_in_numpy(dtype):
    """NaN, +Inf and -Inf in the values, the last values and the rewards, each once behind a finished step (where the non-terminal
    factor 0 MULTIPLIES it: Inf * 0 = NaN) and once behind an unfinished one, each in a column of its own; with gamma = 0 too
    (0 * Inf) and with lambda = 0."""
    T, N = 40, 70
    rew, val, done, last = _inputs(T, N, dtype, "none", seed=5)
    bad = [np.nan, np.inf, -np.inf]
    col = 0
    for x in bad:
        for finished in (0, 1):
            val[21, col] = x; done[20, col] = finished; col += 1            # next value of step 20
            rew[20, col] = x; done[20, col] = finished; col += 1            # reward of the step itself
            last[col] = x; done[T - 1, col] = finished; col += 1            # next value of the last step
            val[0, col] = x; done[0, col] = finished; col += 1              # own value of step 0
    assert col <= N - 10                                                    # the last ten columns stay clean
    eng = _engine(N)
    for gamma, lam in [A2C, (0.0, 0.5), (0.97, 0.0)]:
        adv, ret = _run(eng, rew, val, done, last, gamma, lam)
        e_adv, e_ret = gr.gae(rew, val, done, last, gamma, lam, dtype)
        assert np.isnan(e_adv).any() and np.isinf(e_adv).any() and np.isfinite(e_adv[:, -10:]).all()
        _same_bits(adv, e_adv, f"adv {dtype} {gamma} {lam}")
        _same_bits(ret, e_ret, f"ret {dtype} {gamma} {lam}")
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_behind_a_finished_step_reaches_it(dtype):
    """Env e finishes on step t0.  Other rewards and values behind t0 (and another last value) leave adv[: t0 + 1, e] as it was,
    bit for bit, and every other env untouched."""
    T, N, t0 = 90, 131, 37
    envs = [0, 63, 64, 130]
    rew, val, done, last = _inputs(T, N, dtype, "none", seed=6)
    done[t0, envs] = 1
    eng = _engine(N)
    adv1, ret1 = _run(eng, rew, val, done, last, *A2C)
    rew2, val2, last2 = rew.copy(), val.copy(), last.copy()
    rng = np.random.default_rng(60)
    for e in envs:
        rew2[t0 + 1:, e] = rng.normal(5.0, 3.0, T - t0 - 1)
        val2[t0 + 1:, e] = rng.normal(-5.0, 3.0, T - t0 - 1)
        last2[e] = 1e6
    adv2, ret2 = _run(eng, rew2, val2, done, last2, *A2C)
    others = np.setdiff1d(np.arange(N), envs)
    _same_bits(adv2[:t0 + 1, envs], adv1[:t0 + 1, envs], "before the episode end")
    _same_bits(ret2[:t0 + 1, envs], ret1[:t0 + 1, envs], "before the episode end")
    _same_bits(adv2[:, others], adv1[:, others], "other envs")
    _same_bits(ret2[:, others], ret1[:, others], "other envs")
    assert not np.array_equal(adv2[t0 + 1:, envs], adv1[t0 + 1:, envs])       # the change did arrive behind the episode end
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,N", [(1, 5), (17, 64), (129, 4097), (658, 300)])
def test_documented_aliasing_gives_the_same_bits(dtype, T, N):
    """adv is rew and ret is values, both at once and one at a time"""
    import torch
    rew, val, done, last = _inputs(T, N, dtype, "bernoulli", seed=7)
    eng = _engine(N)
    adv0, ret0 = _run(eng, rew, val, done, last, *PPO)
    for alias_adv, alias_ret in [(True, True), (True, False), (False, True)]:
        r, v, d, l = _dev(rew, val, done, last)
        adv, ret = eng.gae(r, v, d, l, *PPO, adv=r if alias_adv else None, ret=v if alias_ret else None)
        torch.cuda.synchronize()
        assert (adv.data_ptr() == r.data_ptr()) == alias_adv and (ret.data_ptr() == v.data_ptr()) == alias_ret
        _same_bits(adv.cpu().numpy(), adv0, f"adv aliased={alias_adv},{alias_ret}")
        _same_bits(ret.cpu().numpy(), ret0, f"ret aliased={alias_adv},{alias_ret}")
        if not alias_adv:
            assert np.array_equal(r.cpu().numpy(), rew)
        if not alias_ret:
            assert np.array_equal(v.cpu().numpy(), val)
    eng.close()


def test_one_row_tensors_and_a_null_return_buffer():
    """[N] tensors are one step; HipEngine.gae(ret=None) allocates the returns; the C entry point takes ret_dev = NULL and then
    writes the advantages alone"""
    import torch
    N = 100
    rew, val, done, last = _inputs(1, N, "float32", "bernoulli", seed=8)
    done[0, ::7] = 1
    eng = _engine(N)
    r, v, d, l = _dev(rew[0], val[0], done[0], last)
    adv, ret = eng.gae(r, v, d, l, *A2C, ret=None)
    torch.cuda.synchronize()
    assert adv.shape == (N,) and ret.shape == (N,)
    e_adv, e_ret = gr.gae(rew, val, done, last, *A2C, "float32")
    _same_bits(adv.cpu().numpy(), e_adv[0]); _same_bits(ret.cpu().numpy(), e_ret[0])
    T = 20
    rew, val, done, last = _inputs(T, N, "float64", "bernoulli", seed=9)
    r, v, d, l = _dev(rew, val, done, last)
    adv = torch.full((T, N), SENTINEL, dtype=torch.float64, device="cuda")
    from rl_ptg_amd import _lib
    rc = eng._L.ptg_gae(eng._h, C.c_void_p(r.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(l.data_ptr()),
                        T, _lib.OUT_F64, PPO[0], PPO[1], C.c_void_p(adv.data_ptr()), None, eng._stream())
    assert rc == 0
    torch.cuda.synchronize()
    _same_bits(adv.cpu().numpy(), gr.gae(rew, val, done, last, *PPO, "float64")[0])
    eng.close()


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_end_to_end_behind_a_real_rollout(out_dtype):
    """rollout -> vn_normalize -> random float32 critic values -> gae on a real engine with device noise: 139-step episodes
    (synthetic_spec(eps_len_d=1): eps_sim_steps - 5 calls), so a 300-step window crosses two episode ends.  Twin engines on the
    same noise streams: the one that also ran gae has the state, the finished-episode list and the normaliser of the other.  A
    critic is float32 whatever the engine writes, so the float64 engine's rewards are cast."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    from rl_ptg_amd import _lib
    n, T = 200, 300
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)
    twins = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype=out_dtype, obs_layout="row")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(seed=21)
        e.vn_init()
        e.reset()
        twins.append(e)
    A, B = twins
    ep_len = A.steps_to_episode_end()
    assert 2 * ep_len < T < 3 * ep_len
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    values = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    last_values = torch.randn((n,), dtype=torch.float32, device="cuda", generator=g)
    outs = []
    for e in twins:
        obs, rew, done = e.rollout(acts)
        outs.append((rew, done, e.vn_normalize(rew, done)))
    rew_n = outs[0][2].float()
    done = outs[0][1]
    adv, ret = A.gae(rew_n, values, done, last_values, *A2C)
    adv64, ret64 = A.gae(outs[0][2].double(), values.double(), done, last_values.double(), *A2C)      # and in float64, same handle
    torch.cuda.synchronize()
    d = done.cpu().numpy()
    assert d.sum() == 2 * n and set(np.nonzero(d)[0].tolist()) == {ep_len - 1, 2 * ep_len - 1}
    e_adv, e_ret = gr.gae(rew_n.cpu().numpy(), values.cpu().numpy(), d, last_values.cpu().numpy(), *A2C, "float32")
    _same_bits(adv.cpu().numpy(), e_adv, "adv"); _same_bits(ret.cpu().numpy(), e_ret, "ret")
    e_adv, e_ret = gr.gae(outs[0][2].double().cpu().numpy(), values.double().cpu().numpy(), d, last_values.double().cpu().numpy(), *A2C, "float64")
    _same_bits(adv64.cpu().numpy(), e_adv, "adv64"); _same_bits(ret64.cpu().numpy(), e_ret, "ret64")
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for f in _lib.STATE_FIELDS:
        assert np.array_equal(A.get_state(f), B.get_state(f)), f
    (sa, ra), (sb, rb) = A.vn_get(), B.vn_get()
    assert sa == sb and np.array_equal(ra, rb)
    fa, fb = A.finished_episodes(), B.finished_episodes()
    assert len(fa[0]) == 2 * n
    oa, ob = np.lexsort((fa[0], fa[1], fa[2])), np.lexsort((fb[0], fb[1], fb[2]))      # waves push in any order: by env id, length, return
    for x, y in zip(fa, fb):
        assert np.array_equal(x[oa], y[ob])
    A.close(); B.close()


def test_on_a_side_stream():
    import torch
    T, N = 65, 1000
    rew, val, done, last = _inputs(T, N, "float32", "bernoulli", seed=10)
    eng = _engine(N)
    adv0, ret0 = _run(eng, rew, val, done, last, *A2C)
    r, v, d, l = _dev(rew, val, done, last)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        adv, ret = eng.gae(r, v, d, l, *A2C)
    side.synchronize()
    _same_bits(adv.cpu().numpy(), adv0); _same_bits(ret.cpu().numpy(), ret0)
    eng.close()


def test_captured_behind_a_replay_proof_step_and_replayed():
    """ptg_set_replay_proof, then ONE linear graph: ptg_step, the step's reward row copied to the end of a T-row window, gae over
    the window.  Replayed over an episode end; after every replay the graph's advantages and returns are the eager call's on the
    same window, bit for bit, and the step's outputs are the eagerly stepped twin's."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T = 300, 24
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=4, sim_step=3600)       # 96-step episodes: the 91st call terminates
    twins = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(seed=77)
        e.reset()
        twins.append(e)
    A, B = twins
    B.set_replay_proof(True)
    to_end = A.steps_to_episode_end()
    R = to_end + 10
    g = torch.Generator(device="cuda"); g.manual_seed(12)
    acts = torch.randint(0, 5, (R, n), dtype=torch.int32, device="cuda", generator=g)
    values = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    last_values = torch.randn((n,), dtype=torch.float32, device="cuda", generator=g)
    win_rew = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    win_done = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
    act_buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    obs, rew, done = B.alloc_obs(1)[0], torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    adv, ret = torch.zeros_like(win_rew), torch.zeros_like(win_rew)

    def body():
        B.step(act_buf, obs, rew, done, want_final=False)
        win_rew[T - 1].copy_(rew)
        win_done[T - 1].copy_(done)
        B.gae(win_rew, values, win_done, last_values, *PPO, adv=adv, ret=ret)

    act_buf.copy_(acts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    finished = 0
    for t in range(R):
        act_buf.copy_(acts[t])
        graph.replay()
        o_ref, r_ref, d_ref = A.step(acts[t], want_final=False)
        e_adv, e_ret = A.gae(win_rew, values, win_done, last_values, *PPO)         # eager, behind the replay on the same stream
        torch.cuda.synchronize()
        assert torch.equal(done, d_ref) and torch.equal(rew, r_ref) and torch.equal(obs, o_ref), f"replay {t}"
        assert torch.equal(win_rew[T - 1], r_ref) and torch.equal(win_done[T - 1], d_ref)
        _same_bits(adv.cpu().numpy(), e_adv.cpu().numpy(), f"replay {t} adv")
        _same_bits(ret.cpu().numpy(), e_ret.cpu().numpy(), f"replay {t} ret")
        finished += int(d_ref.sum())
    assert finished == n                                                     # the replays crossed the episode end
    x = gr.gae(win_rew.cpu().numpy(), values.cpu().numpy(), win_done.cpu().numpy(), last_values.cpu().numpy(), *PPO, "float32")
    _same_bits(adv.cpu().numpy(), x[0]); _same_bits(ret.cpu().numpy(), x[1])
    B.note_replays(R - 1)
    assert A.steps_to_episode_end() == B.steps_to_episode_end()
    A.close(); B.close()


def test_gae_does_not_synchronise_the_host():
    """A condition, not a timing (the way tests/test_finished_dev.py checks its drain): 2 000 fused steps at 65 536 envs are
    milliseconds of device time, far more than the host needs to enqueue them and the gae call behind them.  The stream is busy
    before the call and still busy when it has returned."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    assert eng.steps_to_episode_end() > T * (calls + 1)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs = eng.alloc_obs(T)
    rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
    done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    values = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    last_values = torch.randn((n,), dtype=torch.float32, device="cuda", generator=g)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    eng.rollout(acts, obs, rew, done)                                        # warm: first-launch work is not part of the condition
    eng.gae(rew, values, done, last_values, *A2C, adv=adv, ret=ret)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    eng.gae(rew, values, done, last_values, *A2C, adv=adv, ret=ret)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before gae was called: the check would prove nothing"
    assert busy_after is False, "the stream was idle when gae returned: the call waited for the device"
    eng.sync()
    e_adv, e_ret = gr.gae(rew.cpu().numpy(), values.cpu().numpy(), done.cpu().numpy(), last_values.cpu().numpy(), *A2C, "float32")
    _same_bits(adv.cpu().numpy(), e_adv); _same_bits(ret.cpu().numpy(), e_ret)
    eng.close()


def test_bad_arguments_raise_and_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    T, N = 12, 64
    rew, val, done, last = _inputs(T, N, "float32", "bernoulli", seed=11)
    eng = _engine(N)
    r, v, d, l = _dev(rew, val, done, last)
    adv = torch.full((T, N), SENTINEL, dtype=torch.float32, device="cuda")
    ret = torch.full((T, N), SENTINEL, dtype=torch.float32, device="cuda")
    strided, v64, l64, d32, adv64 = r.t().contiguous().t(), v.double(), l.double(), d.int(), adv.double()
    r16, v16, l16 = r.half(), v.half(), l.half()
    torch.cuda.synchronize()                                                 # the stream is idle from here on
    assert torch.cuda.current_stream().query() is True
    L, h, st = eng._L, eng._h, eng._stream()
    p = {k: C.c_void_p(x.data_ptr()) for k, x in dict(r=r, v=v, d=d, l=l, a=adv, t=ret).items()}

    def call(r="r", v="v", d="d", l="l", n_steps=T, dtype=_lib.OUT_F32, gamma=0.99, lam=0.95, a="a", handle=h):
        return L.ptg_gae(handle, p.get(r), p.get(v), p.get(d), p.get(l), n_steps, dtype, gamma, lam, p.get(a), p["t"], st)

    bad = [dict(handle=None), dict(r=None), dict(v=None), dict(d=None), dict(l=None), dict(a=None), dict(n_steps=0), dict(n_steps=-3),
           dict(dtype=2), dict(dtype=-1), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(lam=float("nan")),
           dict(lam=float("-inf"))]
    for kw in bad:
        assert call(**kw) == -1, kw                                          # PTG_E_INVALID
        if "handle" not in kw:
            assert b"ptg_gae" in L.ptg_last_error(h)
            with pytest.raises(PtgError):
                eng._chk(call(**kw))
    for gamma, lam in [(float("nan"), 0.95), (0.99, float("inf"))]:          # through the method: the library's refusal surfaces
        with pytest.raises(PtgError):
            eng.gae(r, v, d, l, gamma, lam, adv=adv, ret=ret)
    with pytest.raises(PtgError):                                            # an empty window: n_steps = 0
        eng.gae(r[:0], v[:0], d[:0], l, 0.99, 0.95, adv=adv[:0], ret=ret[:0])
    # what the method itself refuses before the library sees it: shapes, mixed dtypes, strided views, wide done flags
    with pytest.raises(ValueError):
        eng.gae(r[:, :32], v[:, :32], d[:, :32], l[:32], 0.99, 0.95)
    with pytest.raises(ValueError):
        eng.gae(r, v[:T - 1], d, l, 0.99, 0.95)
    with pytest.raises(ValueError):
        eng.gae(strided, v, d, l, 0.99, 0.95, adv=adv, ret=ret)
    with pytest.raises(TypeError):
        eng.gae(r, v64, d, l, 0.99, 0.95, adv=adv, ret=ret)
    with pytest.raises(TypeError):
        eng.gae(r, v, d, l64, 0.99, 0.95, adv=adv, ret=ret)
    with pytest.raises(TypeError):
        eng.gae(r16, v16, d, l16, 0.99, 0.95)
    with pytest.raises(TypeError):
        eng.gae(r, v, d32, l, 0.99, 0.95, adv=adv, ret=ret)
    with pytest.raises(ValueError):
        eng.gae(r, v, d, l, 0.99, 0.95, adv=adv64, ret=ret)
    assert torch.cuda.current_stream().query() is True                      # nothing was enqueued
    assert bool((adv == SENTINEL).all()) and bool((ret == SENTINEL).all())
    assert call() == 0                                                       # and the same buffers are fine with good arguments
    torch.cuda.synchronize()
    e_adv, e_ret = gr.gae(rew, val, done, last, 0.99, 0.95, "float32")
    _same_bits(adv.cpu().numpy(), e_adv); _same_bits(ret.cpu().numpy(), e_ret)
    eng.close()
