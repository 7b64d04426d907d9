"""ptg_act and HipEngine.act_categorical / act_eps_greedy / act_gaussian (include/ptg_env.h) -- the action head while collecting --
against the NumPy restatement (tests/act_restatement.py, pinned by tests/test_act_host.py).

Tolerances, derived and not measured: the kernel computes in float64 and rounds once on the store, so against the float64
restatement only the last-place difference between the device's and libm's exp / log / cos / tanh can show.
  float32 outputs  within one float32 spacing of the restatement rounded to float32
  float64 outputs  within 1e-12 * max(1, |ref|): four orders above what two double implementations differ by, five below what
                   any float32 intermediate would leave
  Gaussian samples an additional absolute 1e-12 * sigma, for the cosine near its zeros
Discrete actions and everything epsilon-greedy are compared exactly; tests/test_act_host.py shows that no categorical row drawn
here is ambiguous.  Each test prints its measured maxima (in units of its tolerance)."""
import ctypes as C

import numpy as np
import pytest

import act_restatement as ar

pytestmark = pytest.mark.gpu

_specs = {}
_engines = {}


def _engine(n, action_type="discrete", layout="sb3_flat", fresh=False):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    key = (n, action_type, layout)
    if not fresh and key in _engines:
        return _engines[key]
    if action_type not in _specs:
        _specs[action_type] = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000, action_type=action_type)[0]    # 139-step episodes
    s = _specs[action_type]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout=layout)
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[key] = eng
    return eng


def _tdt(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _dev(x, pad=0):
    """host [N, A] -> device tensor with row stride A + pad (a column slice of a wider tensor)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not pad:
        return t
    wide = torch.full((x.shape[0], x.shape[1] + pad), 7.5, dtype=t.dtype, device="cuda")
    wide[:, :x.shape[1]] = t
    return wide[:, :x.shape[1]]


def _err(got, ref64, dt, extra_abs=0.0):
    """max error of a float output in units of its tolerance (<= 1 passes); NaN must meet NaN"""
    got = got.cpu().numpy()
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan)
    if nan.all():
        return 0.0
    if got.dtype == np.float32:
        ref = ref64.astype(np.float32)
        tol = np.spacing(np.abs(ref)).astype(np.float64) + extra_abs
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    else:
        tol = 1e-12 * np.maximum(1.0, np.abs(ref64)) + extra_abs
        d = np.abs(got - ref64)
    return float((d[~nan] / np.broadcast_to(tol, d.shape)[~nan]).max())


def _words(seed, c, n, offset=0):
    return ar.words(seed, c, np.arange(offset, offset + n))


@pytest.mark.parametrize("N", ar.NS)
def test_discrete_heads_over_every_shape(N):
    """N at 1, around the wave and past one block; A in {2, 5, 32}; float32 and float64; row stride A (int32 actions) and A + 1
    (int64); planted rows: all equal, one -Inf, all but one -Inf, underflow everywhere but the maximum, a tie"""
    import torch
    eng = _engine(N)
    cnt, cnt_e = eng.new_draw_counter(), eng.new_draw_counter()
    worst = dict(logp32=0.0, ent32=0.0, logp64=0.0, ent64=0.0)
    calls = 0
    for n_, A, dt, c in ar.sweep_cases():
        if n_ != N:
            continue
        x = ar.logits_case(N, A, dt)
        tag = "32" if dt == np.float32 else "64"
        for k, (pad, adt) in enumerate(((0, torch.int32), (1, torch.int64))):
            xd = _dev(x, pad)
            res = eng.act_categorical(xd, cnt, seed=ar.SEED, act_dtype=adt)
            eng.sync()
            ref = ar.categorical(x, *_words(ar.SEED, c + k, N))
            assert res.actions.dtype == adt and res.log_prob.dtype == _tdt(dt)
            assert np.array_equal(res.actions.cpu().numpy(), ref["action"]), (N, A, dt, pad)
            worst["logp" + tag] = max(worst["logp" + tag], _err(res.log_prob, ref["logp"], dt))
            worst["ent" + tag] = max(worst["ent" + tag], _err(res.entropy, ref["entropy"], dt))
            det = eng.act_categorical(xd, None, deterministic=True, act_dtype=adt, want_entropy=False)
            eng.sync()
            dref = ar.categorical(x, deterministic=True)
            assert det.entropy is None and np.array_equal(det.actions.cpu().numpy(), dref["action"])
            worst["logp" + tag] = max(worst["logp" + tag], _err(det.log_prob, dref["logp"], dt))
            for eps in (0.0, 1.0, 0.3):
                ce = int(cnt_e.item())
                got = eng.act_eps_greedy(xd, eps, cnt_e, seed=ar.SEED + 1, act_dtype=adt)
                eng.sync()
                eref = ar.eps_greedy(x, eps, *_words(ar.SEED + 1, ce, N))
                assert np.array_equal(got.actions.cpu().numpy(), eref["action"]), (N, A, dt, pad, eps)
                assert eref["explore"].all() if eps == 1.0 else (not eref["explore"].any() if eps == 0.0 else True)
            g = eng.act_eps_greedy(xd, None, None, deterministic=True, act_dtype=adt)
            eng.sync()
            assert np.array_equal(g.actions.cpu().numpy(), ar.eps_greedy(x, deterministic=True)["action"])
            if N > 4:
                assert int(g.actions[4]) == 0 and x[4, 0] == x[4, A - 1] == 31.0                # the tie goes to the first maximum
            calls += 1
        assert int(cnt.item()) == c + 2
    assert calls == 2 * len(ar.AS) * len(ar.DTYPES) and max(worst.values()) <= 1.0, worst
    print(f"N={N}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("N", ar.NS)
def test_gaussian_heads(N):
    """plain and squashed, scalar and per-env log_std, clip bounds that bite, the deterministic form; float32 env actions"""
    import torch
    eng = _engine(N)
    cnt = eng.new_draw_counter()
    worst = {}
    c = 0
    for dt in ar.DTYPES:
        for per_env in (False, True):
            mean, ls = ar.gaussian_case(N, dt, per_env)
            md, ld = torch.from_numpy(mean).cuda(), torch.from_numpy(ls).cuda()
            for squash, clip in ((False, (-0.5, 0.5)), (True, (-0.6, 0.6))):
                for det in (False, True):
                    res = eng.act_gaussian(md, ld, None if det else cnt, clip=clip, squash=squash, seed=ar.SEED, deterministic=det)
                    eng.sync()
                    w = (None, None) if det else _words(ar.SEED, c, N)
                    ref = ar.gaussian(mean, ls, *w, clip=clip, squash=squash, deterministic=det)
                    c += 0 if det else 1
                    assert res.actions.dtype == torch.float32 and res.raw.dtype == _tdt(dt) and (res.entropy is None) == squash
                    extra = 1e-12 * ref["sigma"]
                    tag = ("32" if dt == np.float32 else "64") + ("s" if squash else "p")
                    e = dict(act=_err(res.actions, ref["action"], dt, extra), raw=_err(res.raw, ref["raw"], dt, extra), logp=_err(res.log_prob, ref["logp"], dt))
                    if not squash:
                        e["ent"] = _err(res.entropy, ref["entropy"], dt)
                    for k, v in e.items():
                        worst[k + tag] = max(worst.get(k + tag, 0.0), v)
                    a = res.actions.cpu().numpy()
                    assert a.min() >= np.float32(clip[0]) and a.max() <= np.float32(clip[1])
                    if N >= 63:
                        assert (a == np.float32(clip[0])).any() or (a == np.float32(clip[1])).any()      # the bounds bite
                    if det:
                        assert np.array_equal(res.raw.cpu().numpy(), mean)
    assert int(cnt.item()) == c == 8 and max(worst.values()) <= 1.0, worst
    print(f"N={N}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


def test_a_continuous_engine_steps_on_the_gaussian_actions():
    import torch
    N = 65
    eng, twin = _engine(N, "continuous", fresh=True), _engine(N, "continuous", fresh=True)
    eng.reset(); twin.reset()
    mean, ls = ar.gaussian_case(N, np.float32, True)
    cnt = eng.new_draw_counter()
    for c in range(3):
        res = eng.act_gaussian(torch.from_numpy(mean).cuda(), torch.from_numpy(ls).cuda(), cnt, seed=ar.SEED)
        obs, rew, _ = eng.step(res.actions)
        eng.sync()
        ref = ar.gaussian(mean, ls, *_words(ar.SEED, c, N))
        assert _err(res.actions, ref["action"], np.float32, 1e-12 * ref["sigma"]) <= 1.0
        o2, r2, _ = twin.step(res.actions.cpu().numpy())
        twin.sync()
        assert torch.equal(obs, o2) and torch.equal(rew, r2) and bool(torch.isfinite(rew).all())
    eng.close(); twin.close()


def test_the_counter_the_seed_and_a_shard():
    """one step of the counter per stochastic call, none per deterministic one; two calls differ; the same (seed, counter) repeats;
    rows 100..199 of a 200-env engine equal a 100-env engine at global offset 100"""
    import torch
    x = ar.logits_case(200, 5, np.float32)
    eng, shard = _engine(200), _engine(100, fresh=True)
    shard.set_global_env_offset(100)
    cnt = eng.new_draw_counter()
    xd = _dev(x)
    a = eng.act_categorical(xd, cnt, seed=11)
    b = eng.act_categorical(xd, cnt, seed=11)
    d = eng.act_categorical(xd, cnt, seed=11, deterministic=True)
    mean = np.linspace(-1, 1, 400).astype(np.float32)
    g = eng.act_gaussian(torch.from_numpy(mean).cuda()[::2], torch.full((1,), -1.0, device="cuda"), cnt, seed=11)      # a strided mean
    eng.sync()
    assert int(cnt.item()) == 3
    gref = ar.gaussian(mean[::2], np.float32(-1.0), *_words(11, 2, 200))
    assert _err(g.raw, gref["raw"], np.float32) <= 1.0 and _err(g.log_prob, gref["logp"], np.float32) <= 1.0
    for c, r in enumerate((a, b)):
        assert np.array_equal(r.actions.cpu().numpy(), ar.categorical(x, *_words(11, c, 200))["action"])
    assert not torch.equal(a.actions, b.actions)
    assert np.array_equal(d.actions.cpu().numpy(), ar.categorical(x, deterministic=True)["action"])
    cnt.zero_()
    again = eng.act_categorical(xd, cnt, seed=11)
    other = eng.act_categorical(xd, cnt.zero_(), seed=12)
    eng.sync()
    assert all(torch.equal(p, q) for p, q in zip(a, again)) and not torch.equal(a.actions, other.actions)
    sc = shard.new_draw_counter()
    s = shard.act_categorical(_dev(x[100:]), sc, seed=11)
    shard.sync()
    assert int(sc.item()) == 1
    assert torch.equal(s.actions, a.actions[100:]) and torch.equal(s.log_prob, a.log_prob[100:]) and torch.equal(s.entropy, a.entropy[100:])
    assert not torch.equal(s.actions, a.actions[:100])
    shard.close()


def test_rows_that_cannot_be_acted_on():
    """a NaN logit, a +Inf logit, an all -Inf row, a NaN epsilon, a non-finite mean: action 0 and NaN outputs on those rows only,
    PTG_E_NONFINITE once at the next sync, and a clean call syncs clean"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    N = 65
    eng = _engine(N)
    x = ar.logits_case(N, 5, np.float32)
    x[7, 2] = np.nan; x[20, 0] = np.inf; x[64] = -np.inf
    bad_rows = [7, 20, 64]
    cnt = eng.new_draw_counter()

    def raises_once():
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == _lib.E_NONFINITE == -6 and "ptg_act" in str(ei.value)
        eng.sync()

    res = eng.act_categorical(_dev(x), cnt, seed=5)
    raises_once()
    ref = ar.categorical(x, *_words(5, 0, N))
    assert np.nonzero(ref["bad"])[0].tolist() == bad_rows
    assert np.array_equal(res.actions.cpu().numpy(), ref["action"]) and (res.actions[bad_rows] == 0).all()
    assert _err(res.log_prob, ref["logp"], np.float32) <= 1.0 and _err(res.entropy, ref["entropy"], np.float32) <= 1.0
    assert bool(torch.isnan(res.log_prob[bad_rows]).all()) and int(torch.isnan(res.entropy).sum()) == 3
    q = eng.act_eps_greedy(_dev(x), 0.25, cnt, seed=5)
    raises_once()
    assert np.array_equal(q.actions.cpu().numpy(), ar.eps_greedy(x, 0.25, *_words(5, 1, N))["action"])
    clean = ar.logits_case(N, 5, np.float32)
    for eps in (float("nan"), 1.5, -0.25):
        q = eng.act_eps_greedy(_dev(clean), torch.tensor([eps], dtype=torch.float64, device="cuda"), cnt, seed=5)
        raises_once()
        assert int(q.actions.abs().sum()) == 0
    q = eng.act_eps_greedy(_dev(clean), torch.tensor([float("nan")], dtype=torch.float64, device="cuda"), None, deterministic=True)      # epsilon is not read
    eng.sync()
    assert np.array_equal(q.actions.cpu().numpy(), ar.eps_greedy(clean, deterministic=True)["action"])
    mean, ls = ar.gaussian_case(N, np.float64, True)
    mean[3] = np.nan; mean[4] = -np.inf; ls[9] = np.nan; ls[10] = np.inf
    c = int(cnt.item())
    g = eng.act_gaussian(torch.from_numpy(mean).cuda(), torch.from_numpy(ls).cuda(), cnt, seed=5)
    raises_once()
    gref = ar.gaussian(mean, ls, *_words(5, c, N))
    assert np.nonzero(gref["bad"])[0].tolist() == [3, 4, 9, 10] and (g.actions[[3, 4, 9, 10]] == 0).all()
    ex = 1e-12 * np.where(gref["bad"], 0.0, gref["sigma"])
    assert max(_err(g.actions, gref["action"], np.float64, ex), _err(g.raw, gref["raw"], np.float64, ex), _err(g.log_prob, gref["logp"], np.float64),
               _err(g.entropy, gref["entropy"], np.float64)) <= 1.0
    res = eng.act_categorical(_dev(clean), cnt, seed=5)                               # a clean call syncs clean
    eng.sync()
    assert np.array_equal(res.actions.cpu().numpy(), ar.categorical(clean, *_words(5, c + 1, N))["action"])


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_captured_act_step_add_replayed_three_times():
    """act_categorical -> step -> replay add (and an epsilon-greedy head beside them) captured once on a replay-proof engine, on a
    side stream, replayed three times with the logits and epsilon rewritten in between: every replay equals the restatement at its
    counter value; env state, finished ring and vn statistics equal a twin stepped eagerly with the same actions"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    N, A = 70, 5
    eng, twin = _engine(N, fresh=True), _engine(N, fresh=True)
    for e in (eng, twin):
        e.vn_init()
        e.set_replay_proof(True)
    buf = DeviceReplayBuffer(eng, 8 * N, columns={"actions": torch.int32, "log_prob": torch.float32}, seed=5)
    xs = ar.capture_case(N, A)                               # [N, A + 1] each: logits and a value column
    epss = [0.0, 0.9, 0.4, 1.0]
    wide = torch.zeros((N, A + 1), device="cuda")
    logits = wide[:, :A]
    eps = torch.zeros(1, dtype=torch.float64, device="cuda")
    cnt, cnt_e = eng.new_draw_counter(), eng.new_draw_counter()
    prev = eng.reset().clone()
    twin.reset()
    obs, rew, done, fin = eng.alloc_obs(zero=True), torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), eng.alloc_obs(zero=True)
    res = eng.act_categorical(logits, None, deterministic=True)                      # the static outputs
    res_e = eng.act_eps_greedy(logits, None, None, deterministic=True)

    def one():
        eng.act_categorical(logits, cnt, seed=21, out=res)
        eng.act_eps_greedy(logits, eps, cnt_e, seed=22, out=res_e)
        eng.step(res.actions, obs, rew, done, final_obs=fin)
        buf.add(prev, obs, rew, done, final_obs=fin, actions=res.actions, log_prob=res.log_prob)
        prev.copy_(obs)

    def check(k):
        ref = ar.categorical(xs[k][:, :A], *_words(21, k, N))
        assert np.array_equal(res.actions.cpu().numpy(), ref["action"]), f"call {k}"
        assert _err(res.log_prob, ref["logp"], np.float32) <= 1.0 and _err(res.entropy, ref["entropy"], np.float32) <= 1.0
        assert np.array_equal(res_e.actions.cpu().numpy(), ar.eps_greedy(xs[k][:, :A], epss[k], *_words(22, k, N))["action"]), f"call {k}"
        assert int(cnt.item()) == int(cnt_e.item()) == k + 1 and buf.cursor()[0] == k + 1
        assert torch.equal(buf.column("actions")[k], res.actions) and torch.equal(buf.column("log_prob")[k], res.log_prob)
        twin.step(res.actions.clone())
        twin.sync()
        assert torch.equal(twin.obs, obs) and torch.equal(twin.rew, rew)

    wide.copy_(torch.from_numpy(xs[0])); eps.fill_(epss[0])
    one()                                                    # eager once: code objects are loaded before the capture
    eng.sync()
    check(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    assert int(cnt.item()) == 1 and buf.cursor()[0] == 1     # capturing enqueued nothing
    for k in (1, 2, 3):
        wide.copy_(torch.from_numpy(xs[k])); eps.fill_(epss[k])
        graph.replay()
        torch.cuda.synchronize()
        check(k)
    eng.note_replays(3 - 1)                                  # three replays; the capture call counted as one step on the host
    eng.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0]) == 0
    eng.close(); twin.close()


def test_act_does_not_synchronise_the_host_and_touches_nothing_else():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the three calls and still busy when
    they have returned.  Afterwards env state, finished ring, vn statistics and a replay cursor equal a twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
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
    buf = DeviceReplayBuffer(eng, 2 * n)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    x = torch.from_numpy(ar.nosync_case()).cuda()
    eps = torch.full((1,), 0.1, dtype=torch.float64, device="cuda")
    ls = torch.zeros(1, device="cuda")
    cnt = eng.new_draw_counter()
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    r1, r2, r3 = eng.act_categorical(x, cnt), eng.act_eps_greedy(x, eps, cnt), eng.act_gaussian(x[:, 0], ls, cnt)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    eng.act_categorical(x, cnt, out=r1)
    eng.act_eps_greedy(x, eps, cnt, out=r2)
    eng.act_gaussian(x[:, 0], ls, cnt, out=r3)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    eng.sync()
    assert int(cnt.item()) == 6
    ref = ar.categorical(ar.nosync_case(), *_words(0, 3, n))        # the fourth draw on this counter; vetted on the host: no ambiguous row
    assert np.array_equal(r1.actions.cpu().numpy(), ref["action"])
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


def test_a_python_float_epsilon_is_kept_by_a_captured_call():
    """eps given as a float is written by a fill kernel inside the capture: every replay explores with that value, whatever later
    eager calls pass"""
    import torch
    N = 65
    eng = _engine(N)
    x = ar.logits_case(N, 5, np.float32)
    xd, cnt = _dev(x), eng.new_draw_counter()
    out = eng.act_eps_greedy(xd, 0.75, cnt, seed=31)          # eager once: counter 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.act_eps_greedy(xd, 0.75, cnt, seed=31, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for c in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        ref = ar.eps_greedy(x, 0.75, *_words(31, c, N))
        assert np.array_equal(out.actions.cpu().numpy(), ref["action"]) and 0 < ref["explore"].sum() < N
        other = eng.act_eps_greedy(xd, 0.0, eng.new_draw_counter(), seed=31)      # an eager call with another epsilon in between
        eng.sync()
        assert np.array_equal(other.actions.cpu().numpy(), ar.eps_greedy(x, deterministic=True)["action"])
    assert int(cnt.item()) == 3


def test_on_a_side_stream():
    import torch
    N = 257
    eng = _engine(N)
    x = ar.logits_case(N, 5, np.float64)
    xd, cnt = _dev(x), eng.new_draw_counter()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = eng.act_categorical(xd, cnt, seed=ar.SEED)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    ref = ar.categorical(x, *_words(ar.SEED, 0, N))
    assert np.array_equal(res.actions.cpu().numpy(), ref["action"]) and _err(res.log_prob, ref["logp"], np.float64) <= 1.0 and int(cnt.item()) == 1


def test_refused_arguments_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    N, A = 64, 5
    eng = _engine(N)
    L, h, stream = eng._L, eng._h, eng._stream()
    x = torch.zeros((N, A), device="cuda")
    x64 = x.double()
    eps = torch.full((1,), 0.5, dtype=torch.float64, device="cuda")
    ls = torch.zeros(1, device="cuda")
    cnt = eng.new_draw_counter()
    act_i = torch.full((N,), -9, dtype=torch.int32, device="cuda")
    act_f = torch.full((N,), -9.0, device="cuda")
    outs = [torch.full((N,), -3.5, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    def head(kind, **kw):
        d = dict(kind=kind, flags=0, n_actions=A, in_dtype=_lib.OUT_F32, in_dev=x.data_ptr(), in_s_n=A, seed=1, counter_dev=cnt.data_ptr())
        if kind == _lib.HEAD_GAUSSIAN:
            d.update(in_s_n=1, param_dev=ls.data_ptr(), param_s_n=0, act_kind=_lib.ACT_F32, clip_lo=-1.0, clip_hi=1.0, act_dev=act_f.data_ptr(),
                     raw_dev=outs[0].data_ptr(), logp_dev=outs[1].data_ptr(), ent_dev=outs[2].data_ptr())
        else:
            d.update(act_kind=_lib.ACT_I32, act_dev=act_i.data_ptr())
            if kind == _lib.HEAD_EPS_GREEDY:
                d.update(param_dev=eps.data_ptr())
            else:
                d.update(logp_dev=outs[1].data_ptr(), ent_dev=outs[2].data_ptr())
        d.update(kw)
        return _lib.PtgHead(**d)

    CAT, EPS, GAU, DET, SQ = _lib.HEAD_CATEGORICAL, _lib.HEAD_EPS_GREEDY, _lib.HEAD_GAUSSIAN, _lib.HEAD_DETERMINISTIC, _lib.HEAD_SQUASH
    bad = [head(CAT, in_dev=None), head(CAT, act_dev=None), head(CAT, counter_dev=None), head(EPS, counter_dev=None), head(GAU, counter_dev=None),
           head(3), head(-1), head(CAT, flags=4), head(CAT, flags=8 | DET), head(CAT, flags=SQ), head(EPS, flags=SQ | DET),
           head(CAT, n_actions=1), head(CAT, n_actions=33, in_s_n=33), head(EPS, n_actions=0), head(CAT, in_s_n=A - 1), head(EPS, in_s_n=0), head(GAU, in_s_n=0),
           head(CAT, in_dtype=2), head(GAU, in_dtype=-1), head(CAT, act_kind=_lib.ACT_F32), head(EPS, act_kind=3), head(GAU, act_kind=_lib.ACT_I32),
           head(EPS, param_dev=None), head(GAU, param_dev=None), head(GAU, param_s_n=2), head(GAU, param_s_n=-1),
           head(GAU, clip_lo=1.0, clip_hi=-1.0), head(GAU, clip_lo=float("nan")), head(GAU, clip_hi=float("nan")),
           head(EPS, logp_dev=outs[1].data_ptr()), head(EPS, ent_dev=outs[2].data_ptr()), head(GAU, flags=SQ), head(CAT, raw_dev=outs[0].data_ptr()),
           head(EPS, raw_dev=outs[0].data_ptr())]
    for k, hd in enumerate(bad):
        assert L.ptg_act(h, C.byref(hd), stream) == _lib.E_INVALID, k
        assert b"ptg_act" in L.ptg_last_error(h)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_act(h, None, stream) == _lib.E_INVALID and L.ptg_act(None, C.byref(head(CAT)), stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True
    assert int(cnt.item()) == 0 and bool((act_i == -9).all()) and bool((act_f == -9.0).all()) and all(bool((o == -3.5).all()) for o in outs)
    good = [head(CAT), head(EPS), head(GAU), head(GAU, flags=SQ, ent_dev=None), head(CAT, flags=DET, counter_dev=None), head(EPS, flags=DET, counter_dev=None, param_dev=None),
            head(CAT, in_dtype=_lib.OUT_F64, in_dev=x64.data_ptr(), logp_dev=None, ent_dev=None)]
    for k, hd in enumerate(good):
        assert L.ptg_act(h, C.byref(hd), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()
    assert int(cnt.item()) == 5 and int(act_i.min()) >= 0 and float(act_f.abs().max()) <= 1.0
