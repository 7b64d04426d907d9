"""hipGraph replays of the hot path against the CPU oracle (include/ptg_env.h, "hipGraph capture").  tests/test_graph_replay.py holds a
replayed handle to an eager one; here every replayed step meets the float64 oracle instead: observations (RTOL64 / RTOL32), rewards
(helpers.assert_rewards), done flags and terminal observations exactly, the 24 info fields of a captured ptg_rollout_info, the
finished-episode list, and after every replay sequence each ptg_get_state field.

Captured forms: a default ptg_step (the hot kernel alone, replayed up to the episode's terminating step, which is then taken eagerly), a
replay-proof ptg_step across two episode ends, a ptg_rollout in whole launches, a ptg_rollout_info (float64: the fused kernel; float32:
T generic launches), and a ptg_step captured while the batch is de-synchronised (the generic kernel).  Configurations cover both output
dtypes, the four layouts (one with a feature pitch), 'mod' and 'raw', discrete int32 and continuous float32 actions (with the decode
edges of tests/test_state_sweep.py), OP1 / OP2, a mixed-scenario batch, the real market data of the golden fixtures, batch sizes 1, 63,
65, 257 and one wider than a fused launch (65 792 envs, a 256-env slice across the launch boundary against the oracle).

De-synchronising the batch after the capture (a partial reset, ptg_set_state of unequal step counts): a default captured step or a
captured rollout is refused -- no state change, PTG_E_INVALID at the next synchronising call, the handle stays usable, a full reset
re-arms the graph --, and a replay-proof step hands every replay to its generic kernel, which is right for each env's own clock."""
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
import sb3_flat_oracle as flat_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

ORA_INT = ["meth_state", "i", "j", "hot_cold", "standby_tid", "startup_tid", "partial_tid", "full_tid", "k", "current_action"]
REAL_CASE = "real_bs2_op2_mod_disc_train"       # the golden prep fixture prep_real_bs2_OP2 behind it (tests/helpers.py load_traj)
TAPE_L = 64


def _capture(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return g


def _decode_edges():
    """the continuous-action values test_state_sweep.py decodes: every threshold and its float32 neighbours, +-0, +-1, +-1.5, +-inf, NaN"""
    thr = [np.float32(x) for x in -1 + np.arange(6) * ((1 - (-1)) / 5)]
    vals = set(thr + [np.nextafter(x, np.float32(-np.inf)) for x in thr] + [np.nextafter(x, np.float32(np.inf)) for x in thr]
               + [np.float32(x) for x in (0.0, -0.0, 1.0, -1.0, -1.5, 1.5, np.inf, -np.inf)])
    return np.array(sorted(vals, key=float) + [np.float32(np.nan)], np.float32)


def _actions(K, n, continuous, seed):
    """sticky actions (held ~5 steps) so that envs reach partial / full load; discrete in [-5, 4], continuous half decode edges"""
    rng = np.random.default_rng(seed)
    if continuous:
        edges = _decode_edges()
        draw = lambda: np.where(rng.random(n) < 0.5, edges[rng.integers(0, len(edges), n)], rng.uniform(-1.2, 1.2, n)).astype(np.float32)
    else:
        draw = lambda: rng.integers(-5, 5, n).astype(np.int32)
    out, cur = [], draw()
    for _ in range(K):
        cur = np.where(rng.random(n) < 0.2, draw(), cur)
        out.append(cur.copy())
    return np.stack(out)


_spec_cache = {}


def _synth(scenario, op, raw, action, evaluate):
    """4-day episodes of hourly steps: 96 steps, k_term = 90, the 91st step terminates"""
    from rl_ptg_amd.prep import synthetic_spec
    key = (scenario, op, raw, action, evaluate)
    if key not in _spec_cache:
        spec, _ = synthetic_spec(scenario=scenario, operation=op, eps_len_d=4, sim_step=3600, raw_modified=raw, action_type=action,
                                 train_or_eval="eval" if evaluate else "train", train_steps=200000)
        _spec_cache[key] = spec
    return _spec_cache[key]


def _ora_consts(spec, q=0):
    m = spec.markets[q]
    return dict(spec.consts, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])


class Pair:
    """A HipEngine and the oracle envs that follow its envs [lo, lo + m) (all of them unless `cover` is given), driven with the same
    actions and the same noise tape; every output of the engine is compared with the oracle's."""

    def __init__(self, n, out_dtype="float32", layout="row", raw="mod", action="discrete", op="OP2", scenario=2, data="synth",
                 pitch=None, plan=True, evaluate=False, noise="tape", cover=None, seed=5):
        from rl_ptg_amd.engine import HipEngine
        from rl_ptg_amd.prep import EnvSpec
        self.n, self.out_dtype, self.layout = n, out_dtype, layout
        self.lo, self.m = (0, n) if cover is None else cover
        self.sl = slice(self.lo, self.lo + self.m)
        self.rtol, self.atol = (H.RTOL64, H.ATOL64) if out_dtype == "float64" else (H.RTOL32, H.ATOL32)
        assign = None
        if data == "real":
            _, consts, tables, market = H.load_traj(REAL_CASE)
            raw, action = ("mod" if consts["raw_modified"] else "raw"), ("continuous" if consts["action_type"] else "discrete")
            markets, eps_ind = [H.market_for_engine(consts, market)], market["eps_ind"]
            ora_specs = [(consts, tables, market)]
        elif data == "mixed":
            specs = [_synth(q, op, raw, action, evaluate) for q in (1, 2, 3)]
            spec = EnvSpec.merge_scenarios(specs)
            consts, tables, markets, eps_ind = spec.consts, spec.tables, spec.markets, spec.eps_ind
            assign = (np.arange(n) % 3).astype(np.uint8)
            ora_specs = [(_ora_consts(s), s.tables, s.markets[0]) for s in specs]
        else:
            spec = _synth(scenario, op, raw, action, evaluate)
            consts, tables, markets, eps_ind = spec.consts, spec.tables, spec.markets, spec.eps_ind
            ora_specs = [(_ora_consts(spec), spec.tables, spec.markets[0])]
        consts = dict(consts, train_or_eval=1 if evaluate else 0)
        self.raw, self.continuous, self.evaluate = raw, action == "continuous", evaluate
        self.eps_ind = eps_ind if plan else None
        assert self.eps_ind is None or (self.m == n and (assign is None or n % 3 == 0)), "an episode plan needs the whole batch"
        self.k_term = consts["eps_sim_steps"] - 6
        self.eng = eng = HipEngine(consts, tables, markets, n, device=0, out_dtype=out_dtype, obs_layout=layout, obs_pitch=pitch)
        if assign is not None:
            eng.set_market_assignment(assign)
        self.sets = np.zeros(self.m, np.int64) if assign is None else assign[self.sl].astype(np.int64)
        if self.eps_ind is not None:
            eng.set_episode_plan(self.eps_ind, n, n)
        else:
            eng.set_episode_plan(None, 0, 0)
        if noise == "tape":
            eng.fill_noise_tape(seed=seed, per_env_len=TAPE_L)
            tape = eng.get_noise_tape(TAPE_L)[self.sl]
        else:                                   # in-kernel RNG; the oracle's tape: the same counter streams from a twin at the slice's offset
            eng.set_noise_rng(seed)
            twin = HipEngine(consts, tables, markets[:1], self.m, device=0, out_dtype=out_dtype, obs_layout="row")
            twin.set_global_env_offset(self.lo)
            twin.fill_noise_tape(seed=seed, per_env_len=TAPE_L)
            tape = twin.get_noise_tape(TAPE_L)
            twin.close()
        self.parts = []                         # (oracle, positions in the covered range)
        for q, (c, t, mk) in enumerate(ora_specs):
            idx = np.flatnonzero(self.sets == q)
            ei = None
            if self.eps_ind is not None:
                ei = self.eps_ind if len(ora_specs) == 1 else self.eps_ind[q::3]    # env 3 i + q of the batch = env i of oracle q
            ora = H.po.OracleVecEnv(dict(c, train_or_eval=1 if evaluate else 0), t, dict(mk, eps_ind=ei), len(idx), ep_index0=0)
            ora.set_noise_tape(tape[idx])
            self.parts.append((ora, idx))
        self.F = self.parts[0][0].obs_dim
        self.series = eng.market_feature_series() if layout == "split" else None
        self.ret, self.abs_ret = np.zeros(self.m), np.zeros(self.m)
        self.length, self.n_resets = np.zeros(self.m, np.int64), np.zeros(self.m, np.int64)
        self.fin_exp = []

    def close(self):
        self.eng.close()
        for o, _ in self.parts:
            o.close()

    # ---------------------------------------------------------------- the two sides
    def rows(self, obs):
        """engine observations of the covered envs as [m, F'] NumPy rows (split rows rebuilt into the flat row)"""
        from rl_ptg_amd.policy_split import flat_rows_from_split
        r = self.eng.rows(obs)[self.sl]
        if self.layout == "split":
            r = flat_rows_from_split(r, self.series, self.raw)
        return r.cpu().numpy()

    def conv(self, o):
        """oracle rows (canonical column order, float64) in the engine's layout"""
        return flat_oracle.flatten_rows(o, self.raw) if self.layout in ("sb3_flat", "split") else o

    def ref_step(self, a):
        a = np.asarray(a)[self.sl]
        m, F = self.m, self.F
        o, f, r, d = np.empty((m, F)), np.empty((m, F)), np.empty(m), np.empty(m, np.uint8)
        inf = np.empty((m, 24)) if self.evaluate else None
        for ora, idx in self.parts:
            oo, rr, dd, ff, ii = ora.step(a[idx], n_threads=16 if len(idx) >= 1024 else 0)
            o[idx], r[idx], d[idx], f[idx] = oo, rr, dd, ff
            if inf is not None:
                inf[idx] = ii
        self.ret += r
        self.abs_ret += np.abs(r)
        self.length += 1
        for j in np.flatnonzero(d):
            self.fin_exp.append((self.lo + int(j), int(self.length[j]), self.ret[j], self.abs_ret[j]))
        w = d.astype(bool)
        self.ret[w], self.abs_ret[w], self.length[w] = 0.0, 0.0, 0
        self.n_resets[w] += 1
        return o, r, d, f, inf

    def reset(self):
        o = self.rows(self.eng.reset())
        ref = np.empty((self.m, self.F))
        for ora, idx in self.parts:
            ref[idx] = ora.reset()[0]
        np.testing.assert_allclose(o, self.conv(ref), rtol=self.rtol, atol=self.atol, err_msg="reset")
        self.ret[:], self.abs_ret[:], self.length[:] = 0.0, 0.0, 0
        self.n_resets += 1
        return o

    def partial_reset(self, mask):
        o = self.rows(self.eng.reset(mask))
        for j in np.flatnonzero(mask[self.sl]):
            ora, idx = next(p for p in self.parts if j in p[1])
            loc = int(np.flatnonzero(idx == j)[0])
            ref = ora.reset(loc)[0][loc]
            np.testing.assert_allclose(o[j], self.conv(ref[None])[0], rtol=self.rtol, atol=self.atol, err_msg=f"reset env {j}")
            self.ret[j], self.abs_ret[j], self.length[j] = 0.0, 0.0, 0
            self.n_resets[j] += 1

    def oracle_state(self):
        ints, f64 = np.empty((self.m, 12), np.int64), np.empty((self.m, 8))
        nc = np.empty(self.m, np.int64)
        for ora, idx in self.parts:
            ints[idx], f64[idx] = ora.state()
            nc[idx] = [ora.noise_count(e) for e in range(ora.n)]
        return ints, f64, nc

    def set_field(self, name, values):
        """the same state field written into both sides (k: the step count; cum_rew)"""
        self.eng.set_state(name, values)
        if name == "k":                         # the episode length the finished-episode list reports is the step count
            self.length[:] = np.asarray(values)[self.sl]
        col = {"k": (0, 8), "cum_rew": (1, 1)}[name]
        for ora, idx in self.parts:
            ints, f64 = ora.state()
            nc = np.array([ora.noise_count(e) for e in range(ora.n)])
            (ints if col[0] == 0 else f64)[:, col[1]] = np.asarray(values)[self.sl][idx]
            ora.set_state(ints, f64, nc)

    # ---------------------------------------------------------------- comparisons
    def check(self, tag, obs, rew, done, a, final=None, info=None):
        """one vector step of the oracle against the engine's outputs of that step"""
        o_ref, r_ref, d_ref, f_ref, i_ref = self.ref_step(a)
        assert np.array_equal(done[self.sl].cpu().numpy().astype(bool), d_ref.astype(bool)), f"{tag}: done flags"
        H.assert_rewards(rew[self.sl].cpu().numpy(), r_ref, self.out_dtype, err_msg=f"{tag}: reward")
        np.testing.assert_allclose(self.rows(obs), self.conv(o_ref), rtol=self.rtol, atol=self.atol, err_msg=f"{tag}: obs")
        w = d_ref.astype(bool)
        if final is not None and w.any():
            np.testing.assert_allclose(self.rows(final)[w], self.conv(f_ref)[w], rtol=self.rtol, atol=self.atol, err_msg=f"{tag}: final obs")
        if info is not None:
            np.testing.assert_allclose(info[self.sl].cpu().numpy(), i_ref, rtol=H.RTOL64, atol=H.ATOL64, err_msg=f"{tag}: info")
        return d_ref

    def check_state(self, tag=""):
        """every ptg_get_state field of the covered envs against the oracle (ep_ptr from the resets each env went through)"""
        ints, f64, nc = self.oracle_state()
        got = lambda f: self.eng.get_state(f)[self.sl]
        for c, name in enumerate(ORA_INT):
            assert np.array_equal(got(name), ints[:, c]), f"{tag}: {name}"
        assert np.array_equal(got("act_ep_d"), ints[:, 11]), f"{tag}: act_ep_d"
        assert np.array_equal(got("T_cat"), f64[:, 2]), f"{tag}: T_cat"
        np.testing.assert_allclose(got("cum_rew"), f64[:, 1], rtol=1e-11, atol=1e-9, err_msg=f"{tag}: cum_rew")
        assert np.array_equal(got("noise_count"), nc), f"{tag}: noise_count"
        assert np.array_equal(got("market_set"), self.sets), f"{tag}: market_set"
        assert np.array_equal(got("n_state_changes"), np.zeros(self.m)), f"{tag}: n_state_changes (no penalty: not tracked)"
        e = np.arange(self.lo, self.lo + self.m)
        E = 0 if self.eps_ind is None else len(self.eps_ind)
        ptr = (self.n + e + self.n_resets * self.n) % E if E else np.zeros(self.m, np.int64)
        assert np.array_equal(got("ep_ptr"), ptr), f"{tag}: ep_ptr"

    def check_finished(self, tag=""):
        """ptg_finished_episodes (returns to 1e-12 of the episode's absolute reward sum, lengths, env ids) against the oracle's episodes"""
        r, l, ids = self.eng.finished_episodes()
        keep = (ids >= self.lo) & (ids < self.lo + self.m)
        got = sorted(zip(ids[keep].tolist(), l[keep].tolist(), r[keep].tolist()))
        exp = sorted(self.fin_exp)
        self.fin_exp = []
        assert len(got) == len(exp), f"{tag}: {len(got)} finished episodes, the oracle has {len(exp)}"
        for (e1, l1, r1), (e2, l2, r2, a2) in zip(got, exp):
            assert e1 == e2 and l1 == l2 and abs(r1 - r2) <= 1e-12 * a2 + 1e-12, (tag, e1, e2, l1, l2, r1, r2)
        return len(got)

    def expect_to_end(self):
        """what ptg_steps_to_episode_end must say for the oracle's (synchronised) step count"""
        k = self.oracle_state()[0][:, 8]
        assert np.all(k == k[0])
        return self.k_term - int(k[0]) + 1

    def eager(self, acts, tag):
        for t in range(acts.shape[0]):
            o, r, d = self.eng.step(acts[t])
            self.eng.sync()
            self.check(f"{tag} eager {t}", o, r, d, acts[t], final=self.eng.final_obs, info=self.eng.info)

    # ---------------------------------------------------------------- captured forms
    def step_graph(self, final=False):
        import torch
        eng = self.eng
        self.act_buf = torch.zeros(self.n, dtype=torch.float32 if self.continuous else torch.int32, device="cuda")
        self.g_obs, self.g_rew = eng.alloc_obs(1, zero=True)[0], torch.zeros(self.n, dtype=eng.out_dtype, device="cuda")
        self.g_done = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        self.g_fin = eng.alloc_obs(1, zero=True)[0] if final else None
        return _capture(lambda: eng.step(self.act_buf, self.g_obs, self.g_rew, self.g_done, final_obs=self.g_fin, want_final=final))

    def replay_steps(self, g, acts, tag):
        import torch
        ends = []
        for t in range(acts.shape[0]):
            self.act_buf.copy_(torch.as_tensor(acts[t], device="cuda"))
            g.replay()
            self.eng.sync()
            d = self.check(f"{tag} replay {t}", self.g_obs, self.g_rew, self.g_done, acts[t], final=self.g_fin)
            if d.any():
                ends.append(t)
        return ends

    def rollout_graph(self, T, info=False):
        import torch
        eng = self.eng
        self.act_buf = torch.zeros((T, self.n), dtype=torch.float32 if self.continuous else torch.int32, device="cuda")
        self.g_obs, self.g_rew = eng.alloc_obs(T, zero=True), torch.zeros((T, self.n), dtype=eng.out_dtype, device="cuda")
        self.g_done = torch.zeros((T, self.n), dtype=torch.uint8, device="cuda")
        self.g_info = torch.zeros((T, self.n, 24), dtype=torch.float64, device="cuda") if info else None
        L, C = eng._L, __import__("ctypes")
        if info:                                # ptg_rollout_info into fixed buffers (HipEngine.rollout_info allocates its own)
            fn = lambda: eng._chk(L.ptg_rollout_info(eng._h, C.c_void_p(self.act_buf.data_ptr()), eng._action_kind(self.act_buf), T,
                                                     C.c_void_p(self.g_obs.data_ptr()), C.c_void_p(self.g_rew.data_ptr()),
                                                     C.c_void_p(self.g_done.data_ptr()), C.c_void_p(self.g_info.data_ptr()), eng._stream()))
        else:
            fn = lambda: eng.rollout(self.act_buf, self.g_obs, self.g_rew, self.g_done)
        return _capture(fn)

    def replay_rollouts(self, g, acts, tag):
        import torch
        T = self.act_buf.shape[0]
        for q in range(acts.shape[0] // T):
            self.act_buf.copy_(torch.as_tensor(acts[q * T:(q + 1) * T], device="cuda"))
            g.replay()
            self.eng.sync()
            for t in range(T):
                self.check(f"{tag} replay {q} step {t}", self.g_obs[t], self.g_rew[t], self.g_done[t], acts[q * T + t],
                           info=None if self.g_info is None else self.g_info[t])


# ======================================================================================= captured forms on a synchronised batch
DEFAULT_STEP = {
    "n63_f32_row_mod_disc_op2": dict(n=63),
    "n257_f64_feature_pitch_raw_cont_op1": dict(n=257, out_dtype="float64", layout="feature", pitch=257 + 5, raw="raw", action="continuous",
                                                op="OP1", scenario=1),
    "n65_f32_split_real": dict(n=65, layout="split", data="real"),
    "n96_f32_sb3flat_mixed": dict(n=96, layout="sb3_flat", data="mixed"),
    "n1_f64_row_mod_disc_op1_bs3": dict(n=1, out_dtype="float64", op="OP1", scenario=3),
    "n257_f32_sb3flat_raw_cont_op2_bs1": dict(n=257, layout="sb3_flat", raw="raw", action="continuous", scenario=1),
    "n4096_f64_feature_autopitch_mod_disc_op2": dict(n=4096, out_dtype="float64", layout="feature", pitch="auto"),
}


@pytest.mark.parametrize("cfg", list(DEFAULT_STEP))
def test_default_captured_step_vs_oracle(cfg):
    """The hot kernel alone, replayed steps_to_episode_end() - 1 times; ptg_note_replays; the terminating step eagerly (terminal
    observations, auto-reset from the episode plan), a few eager steps after it."""
    P = Pair(**DEFAULT_STEP[cfg])
    eng = P.eng
    P.reset()
    if cfg.endswith("real"):                  # 5 328-step episodes: start 40 steps before the end (one common k: still synchronised)
        P.set_field("k", np.full(P.n, P.k_term - 40))
    R = eng.steps_to_episode_end() - 1
    assert R + 1 == P.expect_to_end() and R >= 40
    acts = _actions(R + 5, P.n, P.continuous, seed=P.n)
    g = P.step_graph()
    P.replay_steps(g, acts[:R], cfg)
    P.check_state(f"{cfg} after the replays")
    eng.note_replays(R - 1)                   # the capture call counted as one step
    assert eng.steps_to_episode_end() == 1 == P.expect_to_end()
    o, r, d = eng.step(acts[R])
    eng.sync()
    assert P.check(f"{cfg} terminating step", o, r, d, acts[R], final=eng.final_obs).all()
    P.eager(acts[R + 1:], cfg)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    assert P.check_finished(cfg) == P.m
    P.check_state(f"{cfg} after the eager steps")
    P.close()


REPLAY_PROOF = {
    "n65_f32_sb3flat_mod_disc_op2": dict(n=65, layout="sb3_flat"),
    "n257_f64_row_raw_cont_op1_bs3": dict(n=257, out_dtype="float64", raw="raw", action="continuous", op="OP1", scenario=3),
    "n63_f32_split_mod_cont_op2": dict(n=63, layout="split", action="continuous"),
    "n96_f32_feature_mixed": dict(n=96, layout="feature", data="mixed"),
}


@pytest.mark.parametrize("cfg", list(REPLAY_PROOF))
def test_replay_proof_step_across_episode_ends_vs_oracle(cfg):
    """ptg_set_replay_proof: the captured step replayed over two episode ends and beyond -- terminal observations, post-reset observations
    from the episode plan, the finished-episode list (queried between the ends too), ptg_note_replays wrapping at the episode length."""
    P = Pair(**REPLAY_PROOF[cfg])
    eng = P.eng
    eng.set_replay_proof(True)
    P.reset()
    R = 2 * (P.k_term + 1) + 17
    acts = _actions(R + 4, P.n, P.continuous, seed=11 + P.n)
    g = P.step_graph(final=True)
    first = P.k_term + 5                      # past the first episode end
    ends = P.replay_steps(g, acts[:first], cfg)
    assert ends == [P.k_term]
    eng.note_replays(first - 1)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    assert P.check_finished(f"{cfg} first end") == P.m
    ends = P.replay_steps(g, acts[first:R], cfg)
    assert ends == [2 * P.k_term + 1 - first]
    eng.note_replays(R - first)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    assert P.check_finished(f"{cfg} second end") == P.m
    assert len(np.unique(eng.get_state("act_ep_d"))) > 1
    P.check_state(f"{cfg} after the replays")
    P.eager(acts[R:], cfg)
    P.check_state(f"{cfg} after the eager steps")
    P.close()


ROLLOUT = {
    "n1_f32_split_mod_cont_op2": (10, dict(n=1, layout="split", action="continuous")),
    "n255_f64_feature_mixed": (9, dict(n=255, out_dtype="float64", layout="feature", data="mixed")),
    "n257_f32_sb3flat_raw_cont_op1": (10, dict(n=257, layout="sb3_flat", raw="raw", action="continuous", op="OP1", scenario=1)),
    "n63_f64_row_real": (8, dict(n=63, out_dtype="float64", data="real")),
    "n65792_f32_row_rng_slice": (15, dict(n=65536 + 256, noise="rng", plan=False, cover=(65536 - 128, 256))),
}


@pytest.mark.parametrize("cfg", list(ROLLOUT))
def test_captured_rollout_vs_oracle(cfg):
    """A captured ptg_rollout replayed in whole launches up to the episode's terminating step, which is then taken eagerly; 65 792 envs:
    two fused launches per replay, the oracle follows 256 envs across their boundary."""
    T, kw = ROLLOUT[cfg]
    P = Pair(**kw)
    eng = P.eng
    P.reset()
    if cfg.endswith("real"):                  # 5 328-step episodes: start 40 steps before the end
        P.set_field("k", np.full(P.n, P.k_term - 40))
    R = (eng.steps_to_episode_end() - 1) // T
    assert R * T + 1 == eng.steps_to_episode_end() == P.expect_to_end()
    acts = _actions(R * T + 5, P.n, P.continuous, seed=3)
    g = P.rollout_graph(T)
    P.replay_rollouts(g, acts[:R * T], cfg)
    P.check_state(f"{cfg} after the replays")
    eng.note_replays((R - 1) * T)
    assert eng.steps_to_episode_end() == 1 == P.expect_to_end()
    o, r, d = eng.step(acts[R * T])
    eng.sync()
    assert P.check(f"{cfg} terminating step", o, r, d, acts[R * T], final=eng.final_obs).all()
    o, r, d = eng.rollout(acts[R * T + 1:])
    eng.sync()
    for t in range(4):
        P.check(f"{cfg} eager rollout {t}", o[t], r[t], d[t], acts[R * T + 1 + t])
    assert P.check_finished(cfg) == P.m
    P.check_state(f"{cfg} after the eager steps")
    P.close()


@pytest.mark.parametrize("cfg", ["n63_f64_row_mod_disc_fused", "n65_f32_feature_raw_cont_generic"])
def test_captured_rollout_info_vs_oracle(cfg):
    """ptg_rollout_info captured and replayed: float64 outputs take the fused kernel, float32 outputs T generic launches; all 24 info
    fields of every step against the oracle's info rows."""
    f64 = "f64" in cfg
    P = Pair(63 if f64 else 65, out_dtype="float64" if f64 else "float32", layout="row" if f64 else "feature", raw="mod" if f64 else "raw",
             action="discrete" if f64 else "continuous", plan=False, evaluate=True)
    eng = P.eng
    P.reset()
    T, R = 10, 4
    acts = _actions(R * T + 3, P.n, P.continuous, seed=8)
    g = P.rollout_graph(T, info=True)
    P.replay_rollouts(g, acts[:R * T], cfg)
    eng.note_replays((R - 1) * T)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.check_state(f"{cfg} after the replays")
    P.eager(acts[R * T:], cfg)
    P.check_state(f"{cfg} after the eager steps")
    P.close()


def test_step_captured_on_a_desynchronised_batch_vs_oracle():
    """Every 7th env reset mid-episode, THEN the capture: the host enqueues the generic kernel, whose replays run across the staggered
    episode ends; ptg_note_replays on the de-synchronised batch keeps the finished-episode list reachable."""
    P = Pair(257, plan=False)
    eng = P.eng
    P.reset()
    acts = _actions(P.k_term + 40, P.n, False, seed=21)
    P.eager(acts[:30], "synchronised")
    mask = (np.arange(P.n) % 7 == 0).astype(np.uint8)
    n_reset = int(mask.sum())
    P.partial_reset(mask)
    assert eng.steps_to_episode_end() == 0
    g = P.step_graph(final=True)
    P.replay_steps(g, acts[30:35], "desynchronised")
    assert P.check_finished("no episode ended yet") == 0          # (the query clears the host's "episodes may have ended" mark)
    first = P.k_term - 30 + 2                 # replays 0 .. first - 1: past the end of the envs that were not reset (replay k_term - 30)
    ends = P.replay_steps(g, acts[35:30 + first], "desynchronised")
    assert ends == [P.k_term - 30 - 5]
    eng.note_replays(first - 1)               # de-synchronised: no count to advance, but episodes may have ended
    assert eng.steps_to_episode_end() == 0
    assert P.check_finished("the envs that were not reset") == P.m - n_reset
    ends = P.replay_steps(g, acts[30 + first:30 + P.k_term + 3], "desynchronised")
    assert ends == [P.k_term - first]         # the reset envs end on replay k_term
    eng.note_replays(P.k_term + 3 - first)
    assert P.check_finished("the reset envs") == n_reset
    P.check_state("after the replays")
    P.eager(acts[30 + P.k_term + 3:30 + P.k_term + 6], "eager after the replays")
    P.check_state("after the eager steps")
    P.close()


# ======================================================================================= de-synchronised after the capture
def _refused(P, g, replay, tag):
    """replays of a launch captured while the batch was synchronised, now that it is not: refused, state and outputs untouched"""
    import torch
    from rl_ptg_amd.engine import PtgError
    before = {f: P.eng.get_state(f) for f in ("i", "j", "k", "meth_state", "cum_rew", "noise_count", "T_cat")}
    out = [t.clone() for t in (P.g_obs, P.g_rew, P.g_done)]
    for _ in range(2):
        replay()
    with pytest.raises(PtgError, match="de-synchronised"):
        P.eng.sync()
    P.eng.sync()                              # reported once
    torch.cuda.synchronize()
    for f, v in before.items():
        assert np.array_equal(P.eng.get_state(f), v), f"{tag}: {f} changed by a refused replay"
    assert all(torch.equal(a, b) for a, b in zip(out, (P.g_obs, P.g_rew, P.g_done))), f"{tag}: outputs written by a refused replay"
    P.check_state(f"{tag}: refused replays")


@pytest.mark.parametrize("form", ["step", "rollout"])
def test_replay_after_partial_reset_is_refused_and_a_full_reset_rearms(form):
    P = Pair(200, out_dtype="float32" if form == "step" else "float64", layout="row" if form == "step" else "feature", plan=False)
    eng = P.eng
    P.reset()
    T = 1 if form == "step" else 5
    acts = _actions(60, P.n, False, seed=4)
    g = P.step_graph() if form == "step" else P.rollout_graph(T)
    run = (lambda a, tag: P.replay_steps(g, a, tag)) if form == "step" else (lambda a, tag: P.replay_rollouts(g, a, tag))
    run(acts[:3 * T], "synchronised")
    eng.note_replays(2 * T)
    P.partial_reset((np.arange(P.n) % 7 == 0).astype(np.uint8))
    _refused(P, g, g.replay, form)
    P.eager(acts[3 * T:3 * T + 3], "eager after the refusal")          # the handle stays usable (generic kernels)
    eng.note_replays(0)                                                  # allowed on a de-synchronised batch
    P.reset()                                                            # full reset: synchronised again, the same graph replays
    run(acts[20:20 + 4 * T], "re-armed")
    eng.note_replays(4 * T)                   # (the count the capture added was dropped by the reset: every replay counts)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.eager(acts[20 + 4 * T:20 + 4 * T + 2], "eager after re-arming")
    P.check_state("after re-arming")
    P.close()


def test_replay_after_unequal_step_counts_is_refused():
    """ptg_set_state("k", unequal): refused like a partial reset; equal counts set again re-arm the graph"""
    P = Pair(130, layout="sb3_flat", plan=False)
    eng = P.eng
    P.reset()
    acts = _actions(40, P.n, False, seed=5)
    g = P.step_graph()
    P.replay_steps(g, acts[:6], "synchronised")
    eng.note_replays(5)
    k = eng.get_state("k")
    P.set_field("k", k + 3 * (np.arange(P.n) % 2))
    assert eng.steps_to_episode_end() == 0
    _refused(P, g, g.replay, "unequal k")
    P.eager(acts[6:9], "eager after the refusal")
    P.set_field("k", np.full(P.n, int(eng.get_state("k").max())))
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.replay_steps(g, acts[9:15], "re-armed")
    eng.note_replays(6)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.eager(acts[15:17], "eager after re-arming")
    P.check_state("after re-arming")
    P.close()


def test_set_state_of_another_field_keeps_replays_valid():
    P = Pair(64, out_dtype="float64", plan=False)
    eng = P.eng
    P.reset()
    acts = _actions(20, P.n, False, seed=6)
    g = P.step_graph()
    P.replay_steps(g, acts[:5], "before")
    P.set_field("cum_rew", np.linspace(-50.0, 50.0, P.n))
    P.replay_steps(g, acts[5:12], "after set_state(cum_rew)")
    eng.sync()
    eng.note_replays(11)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.eager(acts[12:14], "eager")
    P.check_state("cum_rew set by hand")
    P.close()


def test_replay_proof_step_across_a_partial_reset_vs_oracle():
    """A replay-proof step captured on a synchronised batch, replayed after a partial reset: every replay is the generic kernel's
    (the hot kernel hands it over), right for each env's own clock across the staggered episode ends; eager calls on the handle take
    no part in the hand-over; a full reset brings the hot kernel back."""
    P = Pair(257, plan=False)
    eng = P.eng
    eng.set_replay_proof(True)
    P.reset()
    acts = _actions(2 * P.k_term + 60, P.n, False, seed=7)
    g = P.step_graph(final=True)
    P.replay_steps(g, acts[:30], "synchronised")
    eng.note_replays(29)
    assert P.check_finished("no episode ended yet") == 0          # (clears the host's "episodes may have ended" mark)
    P.partial_reset((np.arange(P.n) % 7 == 3).astype(np.uint8))
    first = P.k_term + 1 - 30 + 3
    ends = P.replay_steps(g, acts[30:30 + first], "after the partial reset")
    assert ends == [P.k_term - 30]
    eng.note_replays(first)                   # de-synchronised: only marks finished episodes as possible
    assert P.check_finished("the envs that were not reset") == P.m - len(range(3, P.n, 7))
    ends = P.replay_steps(g, acts[30 + first:30 + first + 32], "after the partial reset")
    assert ends == [P.k_term - first]
    eng.note_replays(32)
    assert P.check_finished("the reset envs") == len(range(3, P.n, 7))
    t = 30 + first + 32
    P.eager(acts[t:t + 3], "eager on the replay-proof handle")
    P.check_state("after the replays")
    P.reset()
    P.replay_steps(g, acts[t + 3:t + 10], "after a full reset")
    eng.note_replays(7)
    assert eng.steps_to_episode_end() == P.expect_to_end()
    P.check_state("after the full reset")
    P.close()
