"""obs_layout="split" (PTG_OBS_SPLIT) against the CPU oracle on a batch of THREE market sets that differ in every series.

The split row carries two indices, market_set * series_length + hour (column 14) and + day (column 15), that every kernel family
writes by itself (generic step / reset rows, k_step_hot, k_rollout_pc), and the consumer (rl_ptg_amd/policy_split.py) rebuilds the
market columns from them.  tests/test_split_layout.py and the split configurations of the other files run one market set, so the set
strides never mattered there; and the three scenarios of prep.synthetic_spec share one el / gas / eua trace, so in 'raw' a wrong set
offset would read the right numbers.  Here scenario q runs over its own trace (synthetic_market(38, 20250614 + 10 q)), env e is in
set e % 3 (195 envs: every wave mixes the sets, the last one is ragged), and oracle q follows envs q::3 from its own single-scenario
spec.  Per step and env: done flags exact, rewards under helpers.assert_rewards, columns 0-13 against the env columns of the oracle's
flattened row (one-hot exact, the rest RTOL32 / RTOL64), columns 14 / 15 as exact integers against a value computed from the
ORACLE's state, and the flat row rebuilt by flat_rows_from_split against the oracle's within the float32 tolerance -- in float64 runs
too, because ptg_market_feature_series is float32 whatever the handle's dtype (include/ptg_env.h, SPLIT)."""
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
import sb3_flat_oracle as flat_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

S, M = 3, 65
N = S * M                    # 195 envs: three sets x 65, set e % 3
TAPE_L = 400                 # noise draws per env (at most one per step; 360 steps)
ORA_INT = ["meth_state", "i", "j", "hot_cold", "standby_tid", "startup_tid", "partial_tid", "full_tid", "k", "current_action"]
# columns 6-13 of a split row (include/ptg_env.h, SPLIT)
SPLIT_ENV = ["T_CAT", "H2_in_MolarFlow", "CH4_syn_MolarFlow", "H2_res_MolarFlow", "H2O_DE_MassFlow", "Elec_Heating", "Temp_hour_enc_sin",
             "Temp_hour_enc_cos"]
K_TERM = 282                 # 2-day episodes of 600-s steps: 288 - 6; the step taken at k = 282 (the 283rd) terminates


# ---------------------------------------------------------------------------------------------------------------- specs
_spec_cache = {}


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _specs(raw, action, P, penalty=0.0, evaluate=False, eps_len_d=2):
    """Three single-scenario specs built the way prep.synthetic_spec builds one, each over its OWN market trace; the preconditions
    the comparison rests on are asserted here: equal consts and episode plans, pairwise different series."""
    from rl_ptg_amd.config import EnvConfig
    from rl_ptg_amd.prep import EnvSpec, Preprocessing
    from rl_ptg_amd.synthetic import synthetic_market
    from rl_ptg_amd.tables import load_op_tables
    key = (raw, action, P, penalty, evaluate, eps_len_d)
    if key in _spec_cache:
        return _spec_cache[key]
    specs = []
    for q in (1, 2, 3):
        cfg = EnvConfig(scenario=q, operation="OP2", eps_len_d=eps_len_d, raw_modified=raw, sim_step=600, state_change_penalty=penalty, price_ahead=P)
        prices = {}
        for j, (split, days) in enumerate((("train", 38), ("val", 9), ("test", 9))):
            el, gas, eua = synthetic_market(days, 20250614 + 10 * q + j)
            prices.update({f"el_{split}": el, f"gas_{split}": gas, f"eua_{split}": eua})
        pre = Preprocessing(prices, load_op_tables("OP2"), cfg, seed_train=3654, train_steps=200000, action_type=action)
        specs.append(EnvSpec.from_dict_input(pre.dict_env_kwargs("train"), "eval" if evaluate else "train"))
    for s in specs[1:]:
        assert _same(s.consts, specs[0].consts) and np.array_equal(s.eps_ind, specs[0].eps_ind)
        assert all(np.array_equal(s.tables[k], specs[0].tables[k]) for k in specs[0].tables)
    assert specs[0].consts["eps_sim_steps"] == 144 * eps_len_d and (eps_len_d != 2 or len(specs[0].eps_ind) == 6880)
    assert np.array_equal(specs[0].eps_ind, np.rint(specs[0].eps_ind))         # whole numbers: int(v * eps_len_d) = int(v) * eps_len_d
    for a in range(S):
        for b in range(a + 1, S):
            for k in ("el", "gas", "eua", "pot_rew", "part_full"):
                x, y = specs[a].markets[0][k], specs[b].markets[0][k]
                assert x.shape == y.shape and not np.array_equal(x, y), (a, b, k)
                if k != "part_full":                          # (part_full is 0 / 1 / 2: it differs in some hours, not in most)
                    assert np.mean(x != y) > 0.9, (a, b, k)
    _spec_cache[key] = specs
    return specs


def _ora_consts(spec):
    m = spec.markets[0]
    return dict(spec.consts, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])


# ---------------------------------------------------------------------------------------------------------------- the oracle's flat row
class _FlatMap:
    """Where flatten_rows puts every canonical column (found by flattening a row of markers, not taken from policy_split), and the
    float64 form of its output: flatten_rows rounds to float32 like SB3's tensors, which is right for the one-hot columns and too
    coarse a reference for the float64 runs' RTOL64."""

    def __init__(self, raw, P):
        self.raw, self.P = raw, P
        keys = flat_oracle.reference_keys(raw, P)
        canon, c = {}, 0
        for k, w in keys:
            canon[k] = c
            c += w
        marker = 100.0 + np.arange(c)[None]
        marker[0, canon["METH_STATUS"]] = 0.0
        f = flat_oracle.flatten_rows(marker, raw, P)[0]
        self.width = len(f)
        self.src = np.where(f >= 100, np.rint(f - 100), -1).astype(np.int64)          # canonical column behind each flat column; -1: one-hot
        hot = np.flatnonzero(self.src < 0)
        assert len(hot) == 6 and np.array_equal(hot, hot[0] + np.arange(6)) and f[hot[0]] == 1.0
        self.env_cols = list(hot) + [int(np.flatnonzero(self.src == canon[k])[0]) for k in SPLIT_ENV]
        self.market_cols = np.setdiff1d(np.arange(self.width), self.env_cols)
        assert len(self.market_cols) == (2 * P if raw == "mod" else P + 4)

    def flat64(self, o):
        f = flat_oracle.flatten_rows(o, self.raw, self.P).astype(np.float64)
        keep = self.src >= 0
        f[:, keep] = np.asarray(o)[:, self.src[keep]]
        return f


# ---------------------------------------------------------------------------------------------------------------- the two sides
class _Oracles:
    """The three oracles behind the batch's env order: env e = 3 i + q is env i of oracle q (its own consts, market scalars, series)."""

    def __init__(self, specs, tape, eps_ind):
        self.o = []
        for q in range(S):
            m = specs[q].markets[0]
            ora = H.po.OracleVecEnv(_ora_consts(specs[q]), specs[q].tables, dict(m, eps_ind=None if eps_ind is None else eps_ind[q::S]), M,
                                    ep_index0=0)
            ora.set_noise_tape(tape[q::S])
            self.o.append(ora)
        self.F = self.o[0].obs_dim

    @staticmethod
    def _merge(parts):
        out = np.empty((N,) + parts[0].shape[1:], parts[0].dtype)
        for q in range(S):
            out[q::S] = parts[q]
        return out

    def reset(self):
        return self._merge([o.reset()[0] for o in self.o])

    def step(self, a):
        res = [o.step(a[q::S]) for q, o in enumerate(self.o)]
        return tuple(None if res[0][j] is None else self._merge([r[j] for r in res]) for j in range(5))

    def reset_env(self, e):
        return self.o[e % S].reset(e // S)[0][e // S]

    def state(self):
        st = [o.state() for o in self.o]
        return self._merge([s[0] for s in st]), self._merge([s[1] for s in st])

    def close(self):
        for o in self.o:
            o.close()


def _decode_edges():
    thr = [np.float32(x) for x in -1 + np.arange(6) * ((1 - (-1)) / 5)]
    vals = set(thr + [np.nextafter(x, np.float32(-np.inf)) for x in thr] + [np.nextafter(x, np.float32(np.inf)) for x in thr]
               + [np.float32(x) for x in (0.0, -0.0, 1.0, -1.0, -1.5, 1.5, np.inf, -np.inf)])
    return np.array(sorted(vals, key=float) + [np.float32(np.nan)], np.float32)


def _actions(K, n, continuous, seed):
    """held actions (partial and full load get reached); continuous: half of the draws are the decode thresholds and their neighbours"""
    rng = np.random.default_rng(seed)
    if not continuous:
        return H.sticky_tape(rng, K, n, p=1 / 8.0)
    edges = _decode_edges()
    draw = lambda: np.where(rng.random(n) < 0.5, edges[rng.integers(0, len(edges), n)], rng.uniform(-1.2, 1.2, n)).astype(np.float32)
    out, cur = [], draw()
    for _ in range(K):
        cur = np.where(rng.random(n) < 0.15, draw(), cur)
        out.append(cur.copy())
    return np.stack(out)


class _Run:
    """An engine in the split layout over the merged spec and the three oracles, driven side by side; every output row is checked."""

    def __init__(self, specs, out_dtype, noise, plan="spec", seed=41):
        from rl_ptg_amd.engine import HipEngine
        from rl_ptg_amd.prep import EnvSpec
        spec = EnvSpec.merge_scenarios(specs)
        c = spec.consts
        self.raw, self.P, self.sim_step = ("mod" if c["raw_modified"] else "raw"), int(c["price_ahead"]), int(c["sim_step"])
        self.continuous, self.evaluate = bool(c["action_type"]), bool(c["train_or_eval"])
        self.out_dtype = out_dtype
        self.rtol, self.atol = (H.RTOL64, H.ATOL64) if out_dtype == "float64" else (H.RTOL32, H.ATOL32)
        self.nh, self.nd = len(spec.markets[0]["el"]), len(spec.markets[0]["gas"])
        self.fm = _FlatMap(self.raw, self.P)
        self.sets = np.arange(N) % S
        self.eng = eng = HipEngine(c, spec.tables, spec.markets, N, device=0, out_dtype=out_dtype, obs_layout="split")
        assert eng.obs_dim == 16 and eng.n_sets == S
        eng.set_market_assignment(self.sets.astype(np.uint8))
        eps_ind = spec.eps_ind if isinstance(plan, str) else plan
        eng.set_episode_plan(eps_ind, N, N) if eps_ind is not None else eng.set_episode_plan(None, 0, 0)
        if noise == "tape":
            eng.fill_noise_tape(seed=seed, per_env_len=TAPE_L)
            tape = eng.get_noise_tape(TAPE_L)
        else:                                   # in-kernel RNG; the oracles read the same counter streams from a twin's tape
            eng.set_noise_rng(seed)
            twin = HipEngine(c, spec.tables, spec.markets, N, device=0, out_dtype=out_dtype, obs_layout="split")
            twin.fill_noise_tape(seed=seed, per_env_len=TAPE_L)
            tape = twin.get_noise_tape(TAPE_L)
            twin.close()
        self.ora = _Oracles(specs, tape, eps_ind)
        self.series = eng.market_feature_series()
        assert self.series["featA"].shape == (S, self.nh) and self.series["gas_n"].shape == (S, self.nd)      # the stride the indices assume
        assert all(v.dtype == np.float32 for v in self.series.values())
        self.ret, self.abs_ret, self.length = np.zeros(N), np.zeros(N), np.zeros(N, np.int64)
        self.fin_exp, self.fin_got = [], []
        self.n_done = 0
        self.n_resets = np.zeros(N, np.int64)
        self.E = 0 if eps_ind is None else len(eps_ind)
        self.worst = {"env": 0.0, "rebuilt": 0.0, "reward": 0.0}
        self.rec = {"rows": [], "flat": [], "rew": [], "done": []}          # every step's split rows / oracle flat rows, for the tests behind

    def close(self):
        self.eng.close()
        self.ora.close()

    def expected_idx(self, k, act_d, sets):
        """the two indices from the ORACLE's episode start and step count (its h_idx / d_idx, oracle/ptg_oracle.c step_one / reset_one:
        the row written by the step that raises the count to k holds the windows at time k * sim_step)"""
        return (sets * self.nh + act_d * 24 + (k * self.sim_step) // 3600, sets * self.nd + act_d + (k * self.sim_step) // 86400)

    def check_rows(self, tag, rows, o_ref, k, act_d, envs, keep=True):
        from rl_ptg_amd.policy_split import flat_rows_from_split
        fm, sets = self.fm, self.sets[envs]
        flat = fm.flat64(o_ref)
        assert rows.dtype == (np.float64 if self.out_dtype == "float64" else np.float32) and rows.shape == (len(envs), 16)
        assert np.array_equal(rows[:, :6], flat[:, fm.env_cols[:6]]), f"{tag}: METH_STATUS one-hot"
        ref = flat[:, fm.env_cols[6:]]
        tol = self.atol + self.rtol * np.abs(ref)
        self.worst["env"] = max(self.worst["env"], float((np.abs(rows[:, 6:14] - ref) / tol).max()))
        np.testing.assert_allclose(rows[:, 6:14], ref, rtol=self.rtol, atol=self.atol, err_msg=f"{tag}: env columns")
        hi, di = self.expected_idx(np.asarray(k), np.asarray(act_d), sets)
        assert np.array_equal(rows[:, 14], hi), f"{tag}: hour index {rows[:8, 14]} != {hi[:8]}"
        assert np.array_equal(rows[:, 15], di), f"{tag}: day index {rows[:8, 15]} != {di[:8]}"
        # no window reaches into the next set (from the engine's own numbers)
        assert np.all(rows[:, 14] - sets * self.nh >= 0) and np.all(rows[:, 14] - sets * self.nh + self.P <= self.nh), tag
        assert np.all(rows[:, 15] - sets * self.nd >= 0) and np.all(rows[:, 15] - sets * self.nd + 2 <= self.nd), tag
        # the market columns are float32 series values whatever the handle's dtype: float32 tolerance
        back = flat_rows_from_split(rows, self.series, self.raw, price_ahead=self.P)
        tol = H.ATOL32 + H.RTOL32 * np.abs(flat)
        self.worst["rebuilt"] = max(self.worst["rebuilt"], float((np.abs(back - flat) / tol).max()))
        np.testing.assert_allclose(back, flat, rtol=H.RTOL32, atol=H.ATOL32, err_msg=f"{tag}: rebuilt flat row")
        if keep:
            self.rec["rows"].append(rows.copy())
            self.rec["flat"].append(flat)

    def reset(self):
        rows = self.eng.reset().cpu().numpy()
        o_ref = self.ora.reset()
        self.n_resets += 1
        ints = self.ora.state()[0]
        assert np.all(ints[:, 8] == 0) and np.array_equal(ints[:, 10], 24 * ints[:, 11])
        self.check_rows("reset", rows, o_ref, ints[:, 8], ints[:, 11], np.arange(N))

    def partial_reset(self, mask):
        rows = self.eng.reset(mask).cpu().numpy()
        envs = np.flatnonzero(mask)
        o_ref = []
        for e in envs:
            # The reference has no partial reset: its envs share one episode counter and reset in env order.  The engine gives every env
            # its own pointer into eps_ind, (N + e + m N) mod E at the m-th reset (include/ptg_env.h, ptg_set_episode_plan), which is
            # that order while all envs end together; a masked reset takes the env's own next entry, so the oracle is pointed at it.
            if self.E:
                ptr = (N + e + self.n_resets[e] * N) % self.E
                assert ptr % S == e % S
                self.ora.o[e % S].ep_index = ptr // S
            o_ref.append(self.ora.reset_env(e))
            self.n_resets[e] += 1
        o_ref = np.stack(o_ref)
        ints = self.ora.state()[0]
        assert np.all(ints[envs, 8] == 0)
        self.check_rows("reset(mask)", rows[envs], o_ref, ints[envs, 8], ints[envs, 11], envs, keep=False)
        self.ret[envs], self.abs_ret[envs], self.length[envs] = 0.0, 0.0, 0

    def check(self, tag, rows, rew, done, a, final=None, info=None):
        pre = self.ora.state()[0]
        o_ref, r_ref, d_ref, f_ref, i_ref = self.ora.step(a)
        post = self.ora.state()[0]
        assert np.array_equal(post[:, 10], 24 * post[:, 11])                # act_ep_h = 24 act_ep_d: whole-day episode starts
        d = d_ref.astype(bool)
        assert np.array_equal(done.astype(bool), d), f"{tag}: done"
        H.assert_rewards(rew, r_ref, self.out_dtype, err_msg=f"{tag}: reward")
        nz = r_ref != 0
        if nz.any():
            self.worst["reward"] = max(self.worst["reward"], float((np.abs(rew[nz] - r_ref[nz]) / (self.atol + self.rtol * np.abs(r_ref[nz]))).max()))
        self.check_rows(tag, rows, o_ref, post[:, 8], post[:, 11], np.arange(N))
        if final is not None and d.any():                                   # the terminal row: the old episode's start, count k + 1
            self.check_rows(f"{tag}: terminal row", final[d], f_ref[d], pre[d, 8] + 1, pre[d, 11], np.flatnonzero(d), keep=False)
        if info is not None:
            np.testing.assert_allclose(info, i_ref, rtol=H.RTOL64, atol=H.ATOL64, err_msg=f"{tag}: info")
        self.rec["rew"].append(np.array(rew)); self.rec["done"].append(np.array(done))
        self.ret += r_ref
        self.abs_ret += np.abs(r_ref)
        self.length += 1
        for e in np.flatnonzero(d):
            self.fin_exp.append((int(e), int(self.length[e]), self.ret[e], self.abs_ret[e]))
        self.ret[d], self.abs_ret[d], self.length[d] = 0.0, 0.0, 0
        self.n_done += int(d.sum())
        self.n_resets[d] += 1
        return d

    def eager(self, acts, t0):
        """-> (hot launches recorded, steps on which an episode ended)"""
        eng, ends = self.eng, []
        eng.profile(True)
        for t in range(acts.shape[0]):
            o, r, d = eng.step(acts[t])
            eng.sync()
            info = eng.info.cpu().numpy() if self.evaluate else None
            if self.check(f"step {t0 + t}", o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), acts[t], final=eng.final_obs.cpu().numpy(),
                          info=info).any():
                ends.append(t0 + t)
        hot = len(eng.profile_read())
        eng.profile(False)
        self.collect()
        return hot, ends

    def fused(self, acts, t0, info=False):
        """-> hot launches recorded"""
        eng = self.eng
        eng.profile(True)
        res = eng.rollout_info(acts) if info else eng.rollout(acts)
        eng.sync()
        hot = len(eng.profile_read())
        eng.profile(False)
        o, r, d = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy()
        inf = res[3].cpu().numpy() if info else None
        for t in range(acts.shape[0]):
            self.check(f"rollout step {t0 + t}", o[t], r[t], d[t], acts[t], info=None if inf is None else inf[t])
        self.collect()
        return hot

    def collect(self):
        r, l, ids = self.eng.finished_episodes()
        self.fin_got.extend(zip(ids.tolist(), l.tolist(), r.tolist()))

    def check_state(self):
        ints, f64s = self.ora.state()
        eng = self.eng
        for col, name in enumerate(ORA_INT):
            assert np.array_equal(eng.get_state(name), ints[:, col]), name
        assert np.array_equal(eng.get_state("act_ep_d"), ints[:, 11])
        assert np.array_equal(eng.get_state("market_set"), self.sets)
        if self.E:
            assert np.array_equal(eng.get_state("ep_ptr"), (N + np.arange(N) + self.n_resets * N) % self.E)
        assert np.array_equal(eng.get_state("T_cat"), f64s[:, 2])
        assert np.all(np.abs(eng.get_state("cum_rew") - f64s[:, 1]) <= 1e-9 * self.abs_ret)
        assert int(eng.get_state("noise_count").max()) <= TAPE_L
        got, exp = sorted(self.fin_got), sorted(self.fin_exp)
        assert len(got) == len(exp)
        for (e1, l1, r1), (e2, l2, r2, a2) in zip(got, exp):
            assert e1 == e2 and l1 == l2 and abs(r1 - r2) <= 1e-9 * a2, (e1, l1, r1, r2)

    def report(self, name):
        print(f"{name}: worst error / tolerance -- env columns {self.worst['env']:.3f}, rebuilt flat row {self.worst['rebuilt']:.3f} "
              f"(float32 tolerance), nonzero rewards {self.worst['reward']:.3f}")

    def record(self):
        return {k: np.stack(v) for k, v in self.rec.items()} | {"series": self.series, "raw": self.raw, "P": self.P, "fm": self.fm,
                                                                "nh": self.nh, "nd": self.nd}


# ---------------------------------------------------------------------------------------------------------------- the main run
CASES = {
    "f32_mod_disc_p13_tape": dict(out_dtype="float32", raw="mod", action="discrete", P=13, noise="tape"),
    "f32_raw_cont_p13_rng": dict(out_dtype="float32", raw="raw", action="continuous", P=13, noise="rng"),
    "f64_mod_cont_p13_rng_penalty": dict(out_dtype="float64", raw="mod", action="continuous", P=13, noise="rng", penalty=0.3),
    "f64_raw_disc_p13_tape": dict(out_dtype="float64", raw="raw", action="discrete", P=13, noise="tape"),
    "f32_raw_disc_p6_tape": dict(out_dtype="float32", raw="raw", action="discrete", P=6, noise="tape"),
    "f64_mod_disc_p24_tape": dict(out_dtype="float64", raw="mod", action="discrete", P=24, noise="tape"),
}
_records = {}


def _drive(name, generic=False):
    """Reset rows; 20 eager steps; rollouts of 140 steps up to step 300 (every env terminates at step 283 and restarts at another
    act_ep_d); reset(mask) of every 7th env; 20 eager steps and a 40-step rollout on the de-synchronised batch.  Returns the record of
    every step's rows.  Routes: at price_ahead 13 a synchronised batch takes k_step_hot for step() and k_rollout_pc for rollout(),
    with the terminating step on the generic kernel (3 launches for the chunk that holds it); everything else -- another
    price_ahead, PTG_NO_HOT_KERNELS, the de-synchronised batch -- is one generic launch per step."""
    cfg = CASES[name]
    key = (name, generic)
    if key in _records:
        return _records[key]
    specs = _specs(cfg["raw"], cfg["action"], cfg["P"], cfg.get("penalty", 0.0))
    env = {"PTG_NO_HOT_KERNELS": "1"} if generic else {}
    os.environ.update(env)
    try:
        R = _Run(specs, cfg["out_dtype"], cfg["noise"])
        eng = R.eng
        hot = cfg["P"] == 13 and not generic
        R.reset()
        assert len(np.unique(eng.get_state("act_ep_d"))) > 10
        acts = _actions(360, N, R.continuous, seed=17)
        routes = {}
        routes["eager 0-19: hot launches"], ends = R.eager(acts[:20], 0)
        assert ends == []
        for t0 in (20, 160):
            routes[f"rollout {t0}-{t0 + 139}: rollout_launches"] = eng.rollout_launches(140)
            routes[f"rollout {t0}-{t0 + 139}: hot launches"] = R.fused(acts[t0:t0 + 140], t0)
        assert R.n_done == N and all(l == K_TERM + 1 for _, l, _, _ in R.fin_exp)
        d_all = np.stack(R.rec["done"])
        assert d_all[K_TERM].all() and d_all.sum() == N                    # all on the 283rd step, inside the second chunk
        day = np.stack(R.rec["rows"])[1:, :, 15]                            # (row 0 of the record is the reset row)
        assert np.all(day[143] - day[0] == 1)                               # the day index moved inside the episode (k = 144: one day)
        assert np.any(day[K_TERM] != day[K_TERM - 1] - 1)                   # ... and the restart is at another act_ep_d
        mask = (np.arange(N) % 7 == 0).astype(np.uint8)
        R.partial_reset(mask)
        assert eng.steps_to_episode_end() == 0
        assert set(np.unique(eng.get_state("k")).tolist()) == {0, 300 - (K_TERM + 1)}
        routes["desync eager 300-319: hot launches"], _ = R.eager(acts[300:320], 300)
        routes["desync rollout 320-359: rollout_launches"] = eng.rollout_launches(40)
        routes["desync rollout 320-359: hot launches"] = R.fused(acts[320:360], 320)
        print(f"{name}{' (PTG_NO_HOT_KERNELS)' if generic else ''} routes: {routes}")
        expect = {"eager 0-19: hot launches": 20 if hot else 0,
                  "rollout 20-159: rollout_launches": 1 if hot else 140, "rollout 20-159: hot launches": 1 if hot else 0,
                  "rollout 160-299: rollout_launches": 3 if hot else 140, "rollout 160-299: hot launches": 2 if hot else 0,
                  "desync eager 300-319: hot launches": 0, "desync rollout 320-359: rollout_launches": 40,
                  "desync rollout 320-359: hot launches": 0}
        assert routes == expect, routes
        R.check_state()
        eng.sync()                                                          # no PTG_E_* left behind
        R.report(name)
        _records[key] = R.record()
        R.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return _records[key]


@pytest.mark.parametrize("name", list(CASES))
def test_split_rows_of_three_market_sets_vs_three_oracles(name):
    _drive(name)


def test_generic_kernels_write_the_split_layout():
    """The first case again under PTG_NO_HOT_KERNELS=1: every step a generic k_step launch (ObsRow::put's split branch and put_idx),
    against the oracle and bit for bit against the hot run -- what lets tests/test_batch_edges.py compare split with the generic
    route like every other layout."""
    name = "f32_mod_disc_p13_tape"
    hot, gen = _drive(name), _drive(name, generic=True)
    for k in ("rows", "rew", "done"):
        assert hot[k].shape == gen[k].shape and np.array_equal(hot[k], gen[k]), k


@pytest.mark.parametrize("out_dtype", ["float64", "float32"])
def test_eval_mode_rollout_info_vs_three_oracles(out_dtype):
    """train_or_eval = 1 without an episode plan (every episode starts at offset 0): 60 steps of rollout_info on the mixed batch --
    float64 outputs take the fused kernel (info rows out of k_rollout_pc), float32 outputs 60 generic launches (rollout_impl; the
    fused kernel's info variant is launched without profile events and rollout_launches describes ptg_rollout, so of the two routes
    only the float32 one shows: no hot launch recorded on a batch that is hot-eligible).  Rows as in the main run, and all 24 info fields of every env and step against the oracles' (RTOL64: info rows are float64 in both)."""
    specs = _specs("mod", "discrete", 13, evaluate=True)
    R = _Run(specs, out_dtype, "tape", plan=None, seed=43)
    assert R.evaluate and R.eng.info is not None
    R.reset()
    assert np.all(R.eng.get_state("act_ep_d") == 0)
    acts = _actions(63, N, False, seed=23)
    assert R.eng.rollout_launches(60) == 1                                  # a synchronised batch at price_ahead 13: hot-eligible
    hot = R.fused(acts[:60], 0, info=True)
    print(f"eval {out_dtype}: rollout_launches(60) = 1, profiled hot launches of rollout_info(60) = {hot}")
    if out_dtype == "float32":
        assert hot == 0                                                     # float32 info rows: generic launches only
    hot, _ = R.eager(acts[60:], 60)                                         # step() with info rows: the generic kernel
    assert hot == 0
    R.check_state()
    R.eng.sync()
    R.report(f"eval {out_dtype}")
    R.close()


# The latest episode start (in days) at which a set's oracle completes an episode without "price index out of range", found on the CPU
# by starting one oracle env per set at 37, 36, ...  1-day episodes, because an episode starts at eps_ind entry x eps_len_d days
# and the entries are whole numbers: only then is every day a possible start.  All three traces are 38 days (911 usable hours); the
# last row of an episode is written at k = 139 (hour 23, day 0), so hour 24 * 36 + 23 + P <= 911 holds up to P = 24 (with equality)
# and day 36 + 2 <= 38 with equality; a start at day 37 fails in every set (d = 37).
SERIES_END_START = (36, 36, 36)
K_TERM_1D = 138


@pytest.mark.parametrize("out_dtype,raw,P", [("float32", "raw", 13), ("float64", "mod", 24)])
def test_series_end_last_whole_episode(out_dtype, raw, P):
    """Every env starts its episode at the last day from which a whole episode fits into its set's series, and runs through it: the
    windows of every set end at the last day (and, at P = 24, at the last hour) of that set's series, one element before the next
    set's.  Indices and rebuilt rows as in the main run, terminal rows on the step path included; no range error on either side;
    after the episode every env restarts at day 0."""
    from rl_ptg_amd.engine import PtgError
    specs = _specs(raw, "discrete", P, eps_len_d=1)
    start = np.array(SERIES_END_START, np.float64)[np.arange(N) % S]         # eps_ind entries: episode start = entry * eps_len_d days
    plan = np.concatenate([np.zeros(N), start, np.zeros(N)])                 # constructions, first reset, the reset after the episode
    # the hard-coded start is the latest: one day later the oracle raises
    for q in range(S):
        m = specs[q].markets[0]
        late = H.po.OracleVecEnv(_ora_consts(specs[q]), specs[q].tables, dict(m, eps_ind=np.array([0.0, SERIES_END_START[q] + 1.0, 0.0])), 1)
        with pytest.raises(RuntimeError, match="out of range"):
            late.reset()
            for t in range(K_TERM_1D + 1):
                late.step(np.array([1], np.int32))
        late.close()
    R = _Run(specs, out_dtype, "tape", plan=plan, seed=47)
    eng = R.eng
    R.reset()
    assert np.array_equal(eng.get_state("act_ep_d"), np.array(SERIES_END_START)[np.arange(N) % S])
    acts = _actions(K_TERM_1D + 6, N, False, seed=29)
    R.fused(acts[:130], 0)
    hot, ends = R.eager(acts[130:], 130)                                    # across the episode end: terminal rows compared
    assert ends == [K_TERM_1D] and R.n_done == N
    rows = np.stack(R.rec["rows"])[1:]
    last_d = rows[:K_TERM_1D, :, 15].max(axis=0) - R.sets * R.nd
    last_h = rows[:K_TERM_1D, :, 14].max(axis=0) - R.sets * R.nh
    assert np.all(last_d + 2 == R.nd) and np.all(last_h == 36 * 24 + 23)    # the last day window of every set
    assert np.all((last_h + P == R.nh) == (P == 24))                        # ... and at P = 24 the last hour window too
    assert np.all(eng.get_state("act_ep_d") == 0)
    R.check_state()
    try:
        eng.sync()                                                          # the range-error flag stayed clear
    except PtgError as e:
        raise AssertionError(f"the engine flagged {e} on an episode the oracle completes")
    R.report(f"series end {out_dtype} {raw} P={P}")
    R.close()


@pytest.mark.parametrize("name", ["f32_mod_disc_p13_tape", "f32_raw_cont_p13_rng"])
def test_the_comparison_can_fail(name):
    """Set q's rows decoded with the series slice of set (q + 1) % 3: the rebuilt rows miss the oracle by more than 1000 x the
    tolerance on some market column, in 'mod' and in 'raw' -- a wrong set stride cannot pass the comparison above."""
    from rl_ptg_amd.policy_split import flat_rows_from_split
    rec = _drive(name)
    fm, rows, flat = rec["fm"], rec["rows"][1:141], rec["flat"][1:141]
    sets = np.arange(N) % S
    for q in range(S):
        w = (q + 1) % S
        r = rows[:, sets == q].copy()
        r[..., 14] += (w - q) * rec["nh"]
        r[..., 15] += (w - q) * rec["nd"]
        back = flat_rows_from_split(r, rec["series"], rec["raw"], price_ahead=rec["P"])
        ref = flat[:, sets == q]
        miss = np.abs(back - ref) / (H.ATOL32 + H.RTOL32 * np.abs(ref))
        assert miss[..., fm.env_cols].max() <= 1.0                          # the env columns are untouched by the decode
        worst = miss[..., fm.market_cols].max(axis=(0, 1))
        print(f"{name}: set {q} decoded as set {w}: worst miss / tolerance per market column {np.array2string(worst, precision=0)}")
        assert worst.max() > 1000.0, (q, w, worst)
        if rec["raw"] == "raw":                                             # hourly AND daily columns: both strides matter
            P = rec["P"]
            src = fm.src[fm.market_cols]
            assert worst[src < P].max() > 1000.0 and worst[src >= P].max() > 1000.0, (q, w, worst)


def test_first_layer_split_on_engine_rows():
    """FirstLayerSplit on the device, float32 rows, series and weights, on the first rollout of the float32 'mod' case, against
    flatten_rows(oracle rows) @ W.T + b in float64.  Bound per output: the arithmetic bound of tests/test_policy_split_host.py,
    (width + 2) 2^-24 (|x| @ |W|.T + |b|), over inputs x that sit within the observation tolerance tol = ATOL32 + RTOL32 |flat| of
    the oracle's, i.e. |x| <= |flat| + tol; plus that tolerance propagated through the layer, tol @ |W|.T."""
    import torch
    from rl_ptg_amd.policy_split import FirstLayerSplit
    rec = _drive("f32_mod_disc_p13_tape")
    rows, flat = rec["rows"][21:161], rec["flat"][21:161]                   # the 140 steps of the first k_rollout_pc launch
    width, Hn = flat.shape[-1], 64
    g = np.random.default_rng(3)
    W32, b32 = g.normal(size=(Hn, width)).astype(np.float32), g.normal(size=Hn).astype(np.float32)
    fl = FirstLayerSplit(rec["series"], rec["raw"], device="cuda", price_ahead=rec["P"]).prepare(torch.from_numpy(W32).cuda(), torch.from_numpy(b32).cuda())
    y = fl(torch.from_numpy(rows).cuda())
    assert y.dtype == torch.float32
    y = y.cpu().numpy().astype(np.float64)
    W, b = W32.astype(np.float64), b32.astype(np.float64)
    ref = flat @ W.T + b
    tol = H.ATOL32 + H.RTOL32 * np.abs(flat)
    bound = (width + 2) * 2.0 ** -24 * ((np.abs(flat) + tol) @ np.abs(W).T + np.abs(b)) + tol @ np.abs(W).T
    print(f"engine-side first layer: worst error / bound {float((np.abs(y - ref) / bound).max()):.3f}")
    assert np.all(np.abs(y - ref) <= bound)
