"""PtGVecEnv.step() on every route the batch's byte size picks, against the CPU oracle: what SB3 receives (Dict observation,
float32 rewards, bool dones, Monitor / DummyVecEnv infos, terminal observations, reset observations and reset infos) step by step,
across at least two episode ends per case.  Routes, by ptg_host_layout_ex and the library's limits:
  A  copy-out, zero-copy   block <= 64 KiB, block + final rows + info rows + actions <= 256 KiB: kernels write the pinned block
  B  ring views, zero-copy block  > 64 KiB, all <= 256 KiB: the same, into one of OBS_RING pinned blocks
  C  ring views, staged    above 256 KiB: device staging, k_pack_status, two copies, final rows fetched by ptg_step_host_end
  D  copy-out, staged      copy_obs=True on a staged batch
  E  device route          norm_reward=True (HipEngine.step + vn_normalize + copies)
Also: the VecEnv lifecycle around a step that step_async began (reset / load_state_dict / seed / close before step_wait), step_tensors
mixed with step() under noise="numpy", and ptg_step_host with pageable buffers and int64 actions as a C caller would drive it."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ZC_MAX, COPY_MAX = 256 << 10, 64 << 10        # ptg_step_host_begin's zero-copy limit, PtGVecEnv's copy-out limit
K = 290                                        # 139-step episodes (eps_len_d = 1): ends after steps 138 and 277
SEED = 3654
M_TAPE = K + 64                                # oracle tape: at most one draw per env and step, never wraps
N_THREADS = 8


# ---------------------------------------------------------------------------------------------------------------- set-up
_specs = {}


def _spec(real=False, action_type="discrete", mode="train"):
    key = (real, action_type, mode)
    if key not in _specs:
        from rl_ptg_amd.prep import EnvSpec, Preprocessing, synthetic_spec
        if real:
            # the reference's real training set through Preprocessing; 1-day episodes so that they end inside the run, every env
            # in its own draw of the shuffled eps_ind (1 517 sub-periods)
            from rl_ptg_amd.config import EnvConfig
            z = np.load(os.path.join(H.GOLD, "market_real.npz"))
            pre = Preprocessing({k: z[k] for k in z.files}, H.load_tables("OP2"), EnvConfig(scenario=2, operation="OP2", eps_len_d=1),
                                seed_train=SEED, train_steps=1500000, action_type=action_type)
            spec = EnvSpec.from_dict_input(pre.dict_env_kwargs("train"), mode)
            assert pre.n_eps == 1517 and spec.consts["eps_sim_steps"] == 144
        else:
            spec = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, action_type=action_type, train_or_eval=mode)[0]
        _specs[key] = spec
    return _specs[key]


def _oracle(spec, n):
    m = spec.markets[0]
    consts = dict(spec.consts, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])
    return H.po.OracleVecEnv(consts, spec.tables, dict(m, eps_ind=spec.eps_ind), n, ep_index0=0)


def _numpy_tape(seed, n, sigma, m=M_TAPE):
    """The first m draws of global env e's Gymnasium stream Generator(PCG64(SeedSequence(seed + e))), e = 0 .. n - 1."""
    return np.stack([np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + e))).normal(0, sigma, size=m) for e in range(n)])


def _device_tape(spec, seed, n, m=M_TAPE):
    """The first m draws of the in-kernel counter RNG of global envs 0 .. n - 1 (ptg_fill_noise_tape on a twin at offset 0)."""
    from rl_ptg_amd.engine import HipEngine
    twin = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float64", obs_layout="row")
    twin.set_global_env_offset(0)
    twin.fill_noise_tape(seed=seed, per_env_len=m)
    tape = twin.get_noise_tape(m)
    twin.close()
    return tape


class _Actions:
    """Sticky random actions (each env holds an action for 1-11 steps), discrete or continuous, for the whole oracle batch."""

    def __init__(self, n, continuous, seed):
        self.rng = np.random.default_rng(seed)
        self.continuous, self.n, self.t = continuous, n, 0
        self.hold = self.rng.integers(1, 12, n)
        self.cur = np.full(n, 0.3, np.float32) if continuous else np.full(n, 2, np.int32)

    def __call__(self):
        new = self.rng.uniform(-1, 1, self.n).astype(np.float32) if self.continuous else self.rng.integers(0, 5, self.n).astype(np.int32)
        self.cur = np.where(self.t % self.hold == 0, new, self.cur)
        self.t += 1
        return self.cur.copy()


def host_route(env):
    """The route of PtGVecEnv.step for this env, restated from ptg_host_layout_ex and the 64 KiB / 256 KiB rules."""
    if env.norm_reward:
        return "E"
    eng = env.engine
    o_rew, o_done, o_stat, total = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert eng._L.ptg_host_layout_ex(eng._h, C.byref(o_rew), C.byref(o_done), C.byref(o_stat), C.byref(total)) == 0
    n, F, osz = env.num_envs, eng.obs_dim, np.dtype(env._odt).itemsize
    final, info, act = n * F * osz, (n * 24 * 8 if eng.eval_mode else 0), n * 4
    pinned = all(t.is_pinned() for t in env._keep)
    zc = pinned and total.value + final + info + act <= ZC_MAX
    copy_out = total.value <= COPY_MAX if env._copy_obs_arg is None else bool(env._copy_obs_arg)
    assert env._copy_out == copy_out and len(env._blk) == (1 if copy_out else env.OBS_RING)
    return {(True, True): "A", (False, True): "B", (False, False): "C", (True, False): "D"}[(copy_out, zc)]


class Lockstep:
    """A PtGVecEnv and the oracle on the same spec, noise streams and actions; the oracle may hold the whole global batch of a
    sharded env (world_size > 1), the env is its slice [offset, offset + n)."""

    def __init__(self, spec, n, mode="train", out_dtype="float32", layout="row", noise="device", tape_len=32, world_size=1, rank=0,
                 norm_reward=False, copy_obs=None, seed=SEED, act_seed=7):
        from rl_ptg_amd.vec_env import PtGVecEnv
        self.spec, self.n, self.mode, self.dtype, self.noise = spec, n, mode, out_dtype, noise
        self.env = PtGVecEnv(spec, n, train_or_eval=mode, seed=seed, out_dtype=out_dtype, obs_layout=layout, noise=noise,
                             noise_tape_len=tape_len, world_size=world_size, rank=rank, norm_reward=norm_reward, copy_obs=copy_obs)
        self.N = n * world_size
        self.lo = n * rank
        self.sl = slice(self.lo, self.lo + n)
        self.ora = _oracle(spec, self.N)
        self.set_seed(seed)
        self.continuous = spec.consts["action_type"] == 1
        self.acts = _Actions(self.N, self.continuous, act_seed)
        self.odt = np.dtype(out_dtype)
        self.rtol, self.atol = (H.RTOL64, H.ATOL64) if out_dtype == "float64" else (H.RTOL32, H.ATOL32)
        self.ret = np.zeros(self.N)
        self.len = np.zeros(self.N, np.int64)
        self.n_end_steps = 0
        self.rn = None
        if norm_reward:
            from vecnormalize_oracle import RewardNormalizer
            self.rn = RewardNormalizer(n)
        ints = [0, 1, n // 2, n - 1]
        if n > 256 and n % 256:
            ints.append((n // 256) * 256 + (n % 256) // 2)          # inside the ragged last wave of 256-thread blocks
        self.sample = sorted(set(ints))

    def set_seed(self, seed):
        sigma = float(self.spec.consts["noise"])
        self.ora.set_noise_tape(_numpy_tape(seed, self.N, sigma) if self.noise == "numpy" else _device_tape(self.spec, seed, self.N))

    def mine(self, a):
        a = a[self.sl]
        return a.reshape(-1, 1) if self.continuous else a

    # ------------------------------------------------------------------ oracle side
    def expect(self, a):
        o, r, d, f, i = self.ora.step(a, n_threads=N_THREADS)
        self.ret += r
        self.len += 1
        d = d.astype(bool)
        ep_r, ep_l = self.ret.copy(), self.len.copy()
        self.ret[d] = 0.0
        self.len[d] = 0
        sl = self.sl
        return dict(obs=o[sl], rew=r[sl], done=d[sl], final=f[sl], info=None if i is None else i[sl], ep_r=ep_r[sl], ep_l=ep_l[sl])

    # ------------------------------------------------------------------ checks
    def check_obs(self, obs, ref, what):
        spaces = self.env.observation_space.spaces
        assert list(obs) == list(spaces), what
        for k, sl in self.env._cols.items():
            v = obs[k]
            if k == "METH_STATUS":
                assert v.dtype == np.int64 and v.shape == (self.n,), (what, k)
                assert np.array_equal(v, ref[:, sl.start].astype(np.int64)), (what, k, np.nonzero(v != ref[:, sl.start])[0][:8])
            else:
                assert v.dtype == self.odt and v.shape == (self.n,) + tuple(spaces[k].shape), (what, k, v.dtype, v.shape)
                np.testing.assert_allclose(v, ref[:, sl], rtol=self.rtol, atol=self.atol, err_msg=f"{what} {k}")

    def check_row_dict(self, row, ref, what):
        """terminal_observation: one row as a dict of the declared sub-spaces, METH_STATUS a Python int."""
        for k, sl in self.env._cols.items():
            if k == "METH_STATUS":
                assert type(row[k]) is int and row[k] == int(ref[sl.start]), (what, row[k], ref[sl.start])
            else:
                np.testing.assert_allclose(np.asarray(row[k]), ref[sl], rtol=self.rtol, atol=self.atol, err_msg=f"{what} {k}")

    def check_info_dict(self, d, ref, what):
        from rl_ptg_amd.engine import ACTIONS
        from rl_ptg_amd.vec_env import INFO_KEYS
        assert list(d.keys())[:24] == INFO_KEYS, what
        for q, k in enumerate(INFO_KEYS):
            v = d[k]
            if k == "Meth_Action":
                assert v == ACTIONS[int(ref[q])], (what, v, ref[q])
            elif k in ("step", "Meth_State", "Meth_Hot_Cold"):
                assert type(v) is int and v == int(ref[q]), (what, k, v, ref[q])
            else:
                assert type(v) is float and abs(v - ref[q]) <= H.RTOL64 * abs(ref[q]) + H.ATOL64, (what, k, v, ref[q])

    def check_reset(self, obs, o_ref, i_ref):
        from rl_ptg_amd.engine import ACTIONS
        from rl_ptg_amd.vec_env import INFO_KEYS
        self.check_obs(obs, o_ref[self.sl], "reset")
        ri = self.env.reset_infos
        assert len(ri) == self.n
        if self.n > self.env.RESET_INFO_MAX_ENVS:
            assert all(d == {} for d in ri)
            return
        i_ref = i_ref[self.sl]
        for e in range(self.n):
            assert list(ri[e]) == INFO_KEYS, e
            for q, k in enumerate(INFO_KEYS):
                want = ACTIONS[int(i_ref[e, q])] if k == "Meth_Action" else i_ref[e, q]
                assert ri[e][k] == want, ("reset info", e, k, ri[e][k], i_ref[e, q])

    def check(self, out, ref, t):
        from rl_ptg_amd.vec_env import INFO_KEYS
        obs, rew, done, infos = out
        n, what = self.n, f"step {t}"
        self.check_obs(obs, ref["obs"], what)                  # finished envs: the oracle's post-reset rows
        assert rew.dtype == np.float32 and rew.shape == (n,) and done.dtype == bool and done.shape == (n,)
        assert np.array_equal(done, ref["done"]), what
        if self.rn is not None:
            np.testing.assert_allclose(rew, self.rn.step(ref["rew"], ref["done"]), rtol=2e-6, atol=1e-30, err_msg=f"normalised reward {what}")
            H.assert_rewards(self.env.get_original_reward(), ref["rew"], "float32", err_msg=f"original reward {what}")
        else:
            H.assert_rewards(rew, ref["rew"], "float32", err_msg=f"reward {what}")
        assert isinstance(infos, list) and len(infos) == n
        idx = np.nonzero(ref["done"])[0]
        if self.mode == "eval":
            if self.env._lazy_info:
                mat = self.env._info_cur
            else:
                assert all(type(d) is dict for d in infos)
                mat = np.array([[float(d[k]) if k != "Meth_Action" else float(_act_index(d[k])) for k in INFO_KEYS] for d in infos])
            np.testing.assert_allclose(mat, ref["info"], rtol=H.RTOL64, atol=H.ATOL64, err_msg=f"info rows {what}")
            for e in self.sample:
                self.check_info_dict(infos[e], ref["info"][e], (what, e))
        else:
            lens = np.fromiter(map(len, infos), np.int64, n)
            assert not lens[~ref["done"]].any(), what                  # empty dicts except on finished envs
        if len(idx):
            self.n_end_steps += 1
            for e in idx:
                d = infos[e]
                if self.mode == "train":
                    assert set(d) == {"terminal_observation", "TimeLimit.truncated", "episode"}, (what, e, set(d))
                assert d["TimeLimit.truncated"] is False
                ep = d["episode"]
                assert ep["l"] == ref["ep_l"][e], (what, e, ep, ref["ep_l"][e])
                assert not np.isnan(ep["r"]) and abs(ep["r"] - round(float(ref["ep_r"][e]), 6)) <= 1.01e-6, (what, e, ep, ref["ep_r"][e])
            self._check_terminal(infos, idx, ref["final"], what)
            if self.mode == "eval":
                for e in self.sample:
                    assert {"terminal_observation", "TimeLimit.truncated", "episode"} <= set(infos[e].keys())

    def _check_terminal(self, infos, idx, final, what):
        """terminal observations of all finished envs, gathered key by key (no per-env comparison loop)"""
        for k, sl in self.env._cols.items():
            got = [infos[e]["terminal_observation"][k] for e in idx]
            if k == "METH_STATUS":
                assert all(type(v) is int for v in got)
                assert np.array_equal(np.array(got), final[idx, sl.start].astype(np.int64)), (what, k)
            else:
                np.testing.assert_allclose(np.stack(got), final[idx][:, sl], rtol=self.rtol, atol=self.atol, err_msg=f"terminal obs {what} {k}")

    # ------------------------------------------------------------------ driving
    def reset(self):
        obs = self.env.reset()
        o_ref, i_ref = self.ora.reset()
        self.ret[:] = 0.0
        self.len[:] = 0
        if self.rn is not None:
            self.rn.returns[:] = 0.0
        self.check_reset(obs, o_ref, i_ref)

    def step(self, t):
        a = self.acts()
        out = self.env.step(self.mine(a))
        self.check(out, self.expect(a), t)
        return out

    def assert_tape_never_wrapped(self):
        used = max(self.ora.noise_count(e) for e in range(self.N))
        assert 0 < used < M_TAPE, used

    def close(self):
        self.env.close()
        self.ora.close()


def _act_index(name):
    from rl_ptg_amd.engine import ACTIONS
    return list(ACTIONS).index(name)


# ---------------------------------------------------------------------------------------------------------------- the routes
CASES = {
    # id: (route, n, dict(spec / env arguments))
    "A_train_real_f32_numpy": ("A", 256, dict(real=True, out_dtype="float32", noise="numpy")),
    "A_eval_eager_f64": ("A", 48, dict(mode="eval", out_dtype="float64", noise="device")),
    "B_train_continuous_f32_numpy": ("B", 640, dict(action_type="continuous", out_dtype="float32", noise="numpy")),
    "B_eval_lazy_f32": ("B", 500, dict(mode="eval", out_dtype="float32", noise="device")),
    "C_train_f32_device": ("C", 4096, dict(out_dtype="float32", noise="device")),
    "C_train_f64_feature_ragged_numpy": ("C", 1001, dict(out_dtype="float64", layout="feature", noise="numpy")),
    "C_eval_lazy_f32": ("C", 1024, dict(mode="eval", out_dtype="float32", noise="device")),
    "D_copy_obs_f32": ("D", 4096, dict(out_dtype="float32", noise="device", copy_obs=True)),
    "E_norm_reward_f64": ("E", 4096, dict(out_dtype="float64", noise="device", norm_reward=True)),
    "B_rank1_of_2_real_numpy": ("B", 512, dict(real=True, out_dtype="float32", noise="numpy", world_size=2, rank=1)),
}


def _lockstep(n, real=False, action_type="discrete", mode="train", **kw):
    return Lockstep(_spec(real, action_type, mode), n, mode=mode, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_vec_env_route_vs_oracle(case):
    route, n, kw = CASES[case]
    lk = _lockstep(n, **kw)
    env = lk.env
    got = host_route(env)
    print(f"{case}: route {got}, n = {n}, block {env._blk_bytes} B")
    assert got == route, (case, got)
    if env._lazy_info:
        assert kw.get("mode") == "eval" and n > env.EAGER_INFO_MAX and len(env._info_blocks) == 2
    lk.reset()
    prev = None
    for t in range(K):
        out = lk.step(t)
        if route == "D":                                       # fresh arrays and a new infos list every step
            assert not any(np.shares_memory(v, b) for v in out[0].values() for b in env._blk)
            if prev is not None:
                assert out[3] is not prev[3] and all(out[0][k] is not prev[0][k] for k in out[0])
            prev = out
    assert lk.n_end_steps >= 2, lk.n_end_steps
    lk.assert_tape_never_wrapped()
    lk.close()


def test_numpy_noise_streams_concatenate():
    """The numpy tape's refill (PtGVecEnv._refill_tape) relies on consecutive Generator.normal calls continuing one stream: the
    oracle's tape of the first M draws is what the env sees through any number of refills."""
    for seed in (0, SEED, 2 ** 31 + 5):
        g1 = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        g2 = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        parts = [g1.normal(0, 10.0, size=32)] + [g1.normal(0, 10.0, size=u) for u in (1, 7, 0, 32, 13)]
        assert np.array_equal(np.concatenate(parts), g2.normal(0, 10.0, size=85))


def test_mid_run_reset_continues_noise():
    """SB3 calls reset() at every learn(): both sides reset inside an episode, reset observations and reset_infos agree, the noise
    streams continue (not restart) and the following episodes still agree."""
    lk = _lockstep(256, out_dtype="float64", noise="numpy", tape_len=16)
    lk.reset()
    t = 0
    for _ in range(60):
        lk.step(t); t += 1
    counts = [lk.ora.noise_count(e) for e in range(lk.n)]
    assert max(counts) > 0 and lk.env._steps_since_refill == 60 % 16          # draws taken, the tape refilled three times
    lk.reset()
    assert [lk.ora.noise_count(e) for e in range(lk.n)] == counts
    for _ in range(160):
        lk.step(t); t += 1
    assert lk.n_end_steps >= 1
    lk.assert_tape_never_wrapped()
    lk.close()


# ---------------------------------------------------------------------------------------------------------------- lifecycle
LIFECYCLE = ["reset", "load_state_dict", "seed_reset", "close", "second_step_async"]


@pytest.mark.parametrize("n", [6, 4096])
@pytest.mark.parametrize("what", LIFECYCLE)
def test_abandoned_step_async(what, n):
    """A step begun by step_async and never collected by step_wait is drained by reset / load_state_dict / seed / close, and the env
    goes on in lockstep with the oracle.  The abandoned step has run (its noise draws count), so the oracle takes it too -- except
    after load_state_dict, which puts everything back.  A second step_async before step_wait raises RuntimeError and leaves the first
    step to be collected."""
    lk = _lockstep(n, out_dtype="float32", noise="numpy", tape_len=8)
    env = lk.env
    assert host_route(env) == ("A" if n == 6 else "C")
    lk.reset()
    t = 0
    for _ in range(5):
        lk.step(t); t += 1
    a = lk.acts()
    if what == "load_state_dict":
        sd = env.state_dict()
        env.step_async(lk.mine(a))
        env.load_state_dict(sd)                                # back to before the abandoned step: the oracle never takes it
    elif what == "second_step_async":
        env.step_async(lk.mine(a))
        with pytest.raises(RuntimeError, match="step_async"):
            env.step_async(lk.mine(lk.acts()))
        lk.check(env.step_wait(), lk.expect(a), t); t += 1
    else:
        env.step_async(lk.mine(a))
        lk.expect(a)
        if what == "close":
            env.close()
            lk.ora.close()
            return
        if what == "seed_reset":
            assert env.seed(99) == [99 + e for e in range(n)]
            lk.set_seed(99)
        lk.reset()
    for _ in range(12):
        lk.step(t); t += 1
    lk.close()


def test_step_tensors_and_step_share_the_numpy_noise_tape():
    """step_tensors draws from the same numpy tape as step(): mixed over several noise_tape_len periods, both stay on the
    reference's noise streams (the tape is refilled on the same step count, whichever call made the step)."""
    import torch
    lk = _lockstep(48, out_dtype="float64", noise="numpy", tape_len=8)
    env = lk.env
    lk.reset()
    rng = np.random.default_rng(5)
    for t in range(100):
        a = rng.integers(0, 5, lk.N).astype(np.int32)          # a fresh action every step: many state changes, many draws
        if t % 3 == 1:
            o, r, d = env.step_tensors(torch.from_numpy(a).cuda())
            env.engine.sync()
            ref = lk.expect(a)
            np.testing.assert_allclose(env.engine.rows(o).cpu().numpy(), ref["obs"], rtol=H.RTOL64, atol=H.ATOL64, err_msg=f"step_tensors obs {t}")
            H.assert_rewards(r.cpu().numpy(), ref["rew"], "float64", err_msg=f"step_tensors reward {t}")
            assert np.array_equal(d.cpu().numpy().astype(bool), ref["done"])
        else:
            lk.check(env.step(a), lk.expect(a), t)
    assert max(lk.ora.noise_count(e) for e in range(lk.n)) > 3 * 8        # several tape periods were consumed
    lk.assert_tape_never_wrapped()
    lk.close()


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("n,dtype,layout", [(48, "float64", "row"), (4096, "float32", "feature")])
def test_step_host_pageable_buffers_vs_oracle(n, dtype, layout):
    """ptg_step_host with plain (pageable) NumPy buffers -- a C caller's default and the library's route when pinning is refused --
    int64 actions, final rows and info rows, against the oracle across two episode ends.  At n = 48 the sizes alone would allow the
    zero-copy route; pageable memory must send it through the staging buffers all the same."""
    from rl_ptg_amd.engine import HipEngine
    spec = _spec(mode="eval")
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype=dtype, obs_layout=layout)
    eng.set_episode_plan(spec.eps_ind, n, n)
    tape = _numpy_tape(SEED, n, float(spec.consts["noise"]))
    eng.set_noise_tape(tape)
    ora = _oracle(spec, n)
    ora.set_noise_tape(tape)
    L, h, F = eng._L, eng._h, eng.obs_dim
    npdt = np.dtype(dtype)
    rtol, atol = (H.RTOL64, H.ATOL64) if dtype == "float64" else (H.RTOL32, H.ATOL32)
    o_rew, o_done, o_stat, total = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.ptg_host_layout_ex(h, C.byref(o_rew), C.byref(o_done), C.byref(o_stat), C.byref(total)) == 0
    blk = np.zeros(total.value, np.uint8)
    act = np.zeros(n, np.int64)
    fin = np.zeros(n * F, npdt)
    info = np.zeros((n, 24))

    def mat_of(flat):
        return flat.reshape(F, n).T if layout == "feature" else flat.reshape(n, F)
    o_ref, _ = ora.reset()
    np.testing.assert_allclose(eng.rows(eng.reset()).cpu().numpy(), o_ref, rtol=rtol, atol=atol)
    q_stat = 2 * spec.consts["price_ahead"]                     # METH_STATUS column of a 'mod' row
    acts = _Actions(n, False, 11)
    nd = C.c_int(-1)
    ends = 0
    for t in range(K):
        a = acts()
        act[:] = a
        fin[:] = np.nan                                         # a missing final-row copy cannot pass on stale rows
        rc = L.ptg_step_host(h, C.c_void_p(act.ctypes.data), 2, C.c_void_p(blk.ctypes.data), C.c_void_p(fin.ctypes.data),
                             C.c_void_p(info.ctypes.data), C.byref(nd), eng._stream())
        assert rc == 0, eng._L.ptg_last_error(h)
        o_ref, r_ref, d_ref, f_ref, i_ref = ora.step(a, n_threads=N_THREADS)
        mat = mat_of(blk[:n * F * npdt.itemsize].view(npdt))
        np.testing.assert_allclose(mat, o_ref, rtol=rtol, atol=atol, err_msg=f"obs step {t}")
        H.assert_rewards(blk[o_rew.value:o_rew.value + n * npdt.itemsize].view(npdt), r_ref, dtype, err_msg=f"reward step {t}")
        done = blk[o_done.value:o_done.value + n]
        assert np.array_equal(done, d_ref) and nd.value == int(d_ref.sum()), t
        assert np.array_equal(blk[o_stat.value:o_stat.value + n].astype(np.int64), o_ref[:, q_stat].astype(np.int64)), t
        np.testing.assert_allclose(info, i_ref, rtol=H.RTOL64, atol=H.ATOL64, err_msg=f"info rows step {t}")
        if d_ref.any():
            ends += 1
            d = d_ref.astype(bool)
            np.testing.assert_allclose(mat_of(fin)[d], f_ref[d], rtol=rtol, atol=atol, err_msg=f"final rows step {t}")
    assert ends >= 2
    assert max(ora.noise_count(e) for e in range(n)) < M_TAPE
    eng.close()
    ora.close()
