"""A batch of mixed business scenarios (BASELINE.json config 5: env e in market set e % 3, sets BS1 / BS2 / BS3) against three CPU
oracles, one per scenario, each configured from its own single-scenario spec.  The per-env set lookup of every kernel family (generic
step, k_step_hot, the fused rollout, the state-change penalty of the finished return) and the per-set series then meet a reference
that does not share them -- the sharded / one-batch comparisons elsewhere are HIP against HIP.  Integers bit-exact; observations and
rewards within the float32 / float64 contract of tests/helpers.py."""
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
import sb3_flat_oracle as flat_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ["meth_state", "i", "j", "hot_cold", "standby_tid", "startup_tid", "partial_tid", "full_tid", "k", "current_action"]
S = 3                   # market sets
M = 1024                # envs per set
N = S * M               # 3 072 envs: twelve 256-env workgroups, sets interleaved within every wave
K_EAGER, K = 40, 600    # 2-day episodes (283 steps): every env terminates twice
L = 768                 # noise draws per env (>= one per step: the tape never wraps)

_specs = {}


def _specs_for(penalty):
    from rl_ptg_amd.prep import synthetic_spec
    if penalty not in _specs:
        _specs[penalty] = [synthetic_spec(scenario=q, operation="OP2", eps_len_d=2, state_change_penalty=penalty)[0] for q in (1, 2, 3)]
    return _specs[penalty]


def _oracle(spec, tape, eps_ind):
    """One scenario's M envs as the reference runs them: that spec's own consts and market scalars."""
    m = spec.markets[0]
    consts = dict(spec.consts, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])
    ora = H.po.OracleVecEnv(consts, spec.tables, dict(m, eps_ind=eps_ind), M, ep_index0=0)
    ora.set_noise_tape(tape)
    return ora


class _Oracles:
    """The three oracles behind the batch's env order: env e = 3 i + q is env i of oracle q."""

    def __init__(self, specs, tape, eps_ind):
        self.o = [_oracle(specs[q], tape[q::S], None if eps_ind is None else eps_ind[q::S]) for q in range(S)]

    def _merge(self, parts):
        out = np.empty((N,) + parts[0].shape[1:], parts[0].dtype)
        for q in range(S):
            out[q::S] = parts[q]
        return out

    def reset(self):
        return self._merge([o.reset()[0] for o in self.o])

    def step(self, a):
        res = [o.step(a[q::S])[:3] for q, o in enumerate(self.o)]
        return tuple(self._merge([r[j] for r in res]) for j in range(3))

    def reset_env(self, e):
        obs, _ = self.o[e % S].reset(e // S)
        return obs[e // S]

    def state(self):
        st = [o.state() for o in self.o]
        return self._merge([s[0] for s in st]), self._merge([s[1] for s in st])

    def close(self):
        for o in self.o:
            o.close()


def _sticky(rng, K, n):
    a = np.zeros((K, n), np.int32)
    cur = rng.integers(0, 5, n)
    for t in range(K):
        cur = np.where(rng.random(n) < 1 / 8, rng.integers(0, 5, n), cur)
        a[t] = cur
    return a


class _Run:
    """Drives the engine and the oracles side by side and compares every step."""

    def __init__(self, eng, ora, out_dtype, layout):
        self.eng, self.ora, self.out_dtype, self.layout = eng, ora, out_dtype, layout
        self.rtol, self.atol = (H.RTOL64, H.ATOL64) if out_dtype == "float64" else (H.RTOL32, H.ATOL32)
        self.ret = np.zeros(N)
        self.abs_ret = np.zeros(N)
        self.length = np.zeros(N, np.int64)
        self.fin_exp, self.fin_got = [], []
        self.rewards = []

    def rows(self, o):
        return flat_oracle.flatten_rows(o, "mod") if self.layout == "sb3_flat" else o

    def check(self, t, obs, rew, done, a):
        o_ref, r_ref, d_ref = self.ora.step(a)
        assert np.array_equal(done.astype(bool), d_ref.astype(bool)), f"done step {t}"
        H.assert_rewards(rew, r_ref, self.out_dtype, err_msg=f"reward step {t}")
        np.testing.assert_allclose(obs, self.rows(o_ref), rtol=self.rtol, atol=self.atol, err_msg=f"obs step {t}")
        self.rewards.append(r_ref)
        self.ret += r_ref
        self.abs_ret += np.abs(r_ref)
        self.length += 1
        for e in np.nonzero(d_ref)[0]:
            self.fin_exp.append((int(e), int(self.length[e]), self.ret[e], self.abs_ret[e]))
        d = d_ref.astype(bool)
        self.ret[d], self.abs_ret[d], self.length[d] = 0.0, 0.0, 0

    def eager(self, acts, t0):
        for t in range(acts.shape[0]):
            o, r, d = self.eng.step(acts[t])
            self.eng.sync()
            self.check(t0 + t, self.eng.rows(o).cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), acts[t])
        self.collect()

    def fused(self, acts, t0):
        o, r, d = self.eng.rollout(acts)
        self.eng.sync()
        o, r, d = self.eng.rows(o).cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
        for t in range(acts.shape[0]):
            self.check(t0 + t, o[t], r[t], d[t], acts[t])
        self.collect()

    def collect(self):
        r, l, ids = self.eng.finished_episodes()
        self.fin_got.extend(zip(ids.tolist(), l.tolist(), r.tolist()))

    def check_state(self):
        ints, f64s = self.ora.state()
        for col, name in enumerate(INT_FIELDS):
            assert np.array_equal(self.eng.get_state(name), ints[:, col]), name
        assert np.array_equal(self.eng.get_state("act_ep_d"), ints[:, 11])
        assert np.array_equal(self.eng.get_state("market_set"), np.arange(N) % S)
        assert np.array_equal(self.eng.get_state("T_cat"), f64s[:, 2])
        # cum_rew: float64 sums of rewards that agree to a few ulp (the float32 path's price-linear form included)
        assert np.all(np.abs(self.eng.get_state("cum_rew") - f64s[:, 1]) <= 1e-9 * self.abs_ret)
        got, exp = sorted(self.fin_got), sorted(self.fin_exp)
        assert len(got) == len(exp)
        for (e1, l1, r1), (e2, l2, r2, a2) in zip(got, exp):
            assert e1 == e2 and l1 == l2 and abs(r1 - r2) <= 1e-9 * a2, (e1, l1, r1, r2)


def _engine(specs, out_dtype, layout, noise, seed):
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import EnvSpec
    spec = EnvSpec.merge_scenarios(specs)
    eng = HipEngine(spec.consts, spec.tables, spec.markets, N, device=0, out_dtype=out_dtype, obs_layout=layout)
    eng.set_market_assignment(ptg_dist.mixed_scenario_assignment(N, 1, 0, S))
    if noise == "tape":
        eng.fill_noise_tape(seed=seed, per_env_len=L)
        tape = eng.get_noise_tape(L)
    else:
        eng.set_noise_rng(seed)
        twin = HipEngine(spec.consts, spec.tables, spec.markets, N, device=0, out_dtype=out_dtype, obs_layout=layout)
        twin.fill_noise_tape(seed=seed, per_env_len=L)          # the same counter streams (include/ptg_env.h)
        tape = twin.get_noise_tape(L)
        twin.close()
    return spec, eng, tape


@pytest.mark.parametrize("out_dtype,layout,noise,penalty", [
    ("float32", "row", "tape", 0.0), ("float32", "feature", "rng", 0.0), ("float32", "sb3_flat", "tape", 0.0),
    ("float32", "row", "rng", 0.3), ("float64", "row", "tape", 0.3)])
def test_mixed_scenario_batch_vs_three_oracles(out_dtype, layout, noise, penalty):
    """Episode plan over the shared eps_ind: env e = 3 i + q takes eps_ind[N + e] at its first reset, entry M + i of
    eps_ind[q::3], so oracle q gets that slice (DummyVecEnv order; all envs terminate on the same steps).  40 eager steps
    (k_step_hot), then fused chunks (k_rollout_pc, the two terminating steps on the generic kernel)."""
    specs = _specs_for(penalty)
    eps_ind = specs[0].eps_ind
    assert all(np.array_equal(s.eps_ind, eps_ind) for s in specs) and len(eps_ind) >= 3 * N
    spec, eng, tape = _engine(specs, out_dtype, layout, noise, seed=41)
    eng.set_episode_plan(eps_ind, N, N)
    ora = _Oracles(specs, tape, eps_ind)
    run = _Run(eng, ora, out_dtype, layout)
    rtol, atol = run.rtol, run.atol
    np.testing.assert_allclose(eng.rows(eng.reset()).cpu().numpy(), run.rows(ora.reset()), rtol=rtol, atol=atol)
    assert len(np.unique(eng.get_state("act_ep_d"))) > 10
    acts = _sticky(np.random.default_rng(17), K, N)
    run.eager(acts[:K_EAGER], 0)
    for t0 in range(K_EAGER, K, 140):
        run.fused(acts[t0:t0 + 140], t0)
    assert len(run.fin_exp) == 2 * N
    run.check_state()
    assert int(eng.get_state("noise_count").max()) <= L
    # the comparison can fail: set q's envs run on another set's scalars and series give other rewards (so a wrong
    # set lookup, or a scenario value leaking through the merged consts, cannot match the oracle of the right set)
    rew = np.array(run.rewards)
    for q in range(S):
        w = (q + 1) % S
        wrong = _oracle(specs[w], tape[q::S], eps_ind[q::S])
        wrong.reset()
        r_w = np.array([wrong.step(acts[t, q::S])[1] for t in range(60)])
        wrong.close()
        assert np.abs(r_w - rew[:60, q::S]).max() > 1e-3 * np.abs(rew[:60, q::S]).max(), (q, w)
    eng.close(); ora.close()


def test_mixed_scenario_batch_partial_reset_vs_three_oracles():
    """No episode plan (validation / test envs: every reset starts at offset 0, on both sides), 150 synchronised steps, then
    every 7th env reset mid-episode (eng.reset(mask) / the oracle's reset(e)) and 100 more steps: the batch is no longer
    synchronised, so the mixed sets run through the generic kernels with per-env step counts."""
    specs = _specs_for(0.0)
    spec, eng, tape = _engine(specs, "float32", "row", "tape", seed=43)
    eng.set_episode_plan(None, 0, 0)
    ora = _Oracles(specs, tape, None)
    run = _Run(eng, ora, "float32", "row")
    np.testing.assert_allclose(eng.reset().cpu().numpy(), ora.reset(), rtol=H.RTOL32, atol=H.ATOL32)
    assert np.all(eng.get_state("act_ep_d") == 0)
    acts = _sticky(np.random.default_rng(19), 250, N)
    run.eager(acts[:20], 0)
    run.fused(acts[20:150], 20)
    mask = (np.arange(N) % 7 == 0).astype(np.uint8)
    o = eng.reset(mask).cpu().numpy()
    for e in np.nonzero(mask)[0]:
        np.testing.assert_allclose(o[e], ora.reset_env(e), rtol=H.RTOL32, atol=H.ATOL32, err_msg=f"reset env {e}")
    run.ret[mask.astype(bool)] = 0.0
    run.abs_ret[mask.astype(bool)] = 0.0
    run.length[mask.astype(bool)] = 0
    k = eng.get_state("k")
    assert set(np.unique(k).tolist()) == {0, 150}
    run.eager(acts[150:170], 150)
    run.fused(acts[170:250], 170)
    run.check_state()
    eng.close(); ora.close()
