"""One constant at a time: for every constant that is live in a fixture recorded under an edited config_env.yaml
(tests/golden/traj_cfg_*.npz, `live_keys`), an engine built from that fixture's constants with THAT ONE constant back at its default,
against the CPU oracle built from the same constants -- 130 envs (two full waves and a ragged one) on small generated process tables,
40 single steps and one fused rollout of 100 steps, float32 and float64, on the hot kernels (k_step_hot, k_rollout_pc) and on the
generic ones.  The fixtures pin the oracle to the reference with every constant edited at once, and tests/test_config_liveness.py pins
it constant by constant; here every other constant is off its default while one is on it, so a route that reads the wrong field for a
constant (or bakes a default into a precomputed coefficient or a float32 record) fails under that constant's name."""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-11, 1e-13
RTOL32, ATOL32 = 2e-7, 1e-9
N, K1, K2, L = 130, 40, 100, 160
INT_FIELDS = ["meth_state", "i", "j", "hot_cold", "standby_tid", "startup_tid", "partial_tid", "full_tid", "k", "current_action"]
HOT_FIRST = ["cfg_a_bs2_op2_mod_disc", "cfg_b_bs1_op1_raw_cont", "cfg_c_bs3_op2_mod_disc"]          # price_ahead 13: the hot kernels run


def _case_of():
    """key -> the fixture it is live in, one the hot kernels can run on where there is one"""
    out = {}
    for c in HOT_FIRST + [c for c in H.CFG_CASES if c not in HOT_FIRST]:
        for k in H.load_traj(c)[0]["meta"]["live_keys"]:
            out.setdefault(k, c)
    return out


CASE_OF = _case_of()
_tables = {}


def _small_tables(S):
    if S not in _tables:
        _tables[S] = H.make_tables(np.random.default_rng(6100 + S), dict(grid=np.linspace(0.0, 598.7, 240), default_rows=(S + 5, 3 * S + 7)))
    return _tables[S]


def _tape(rng, K, n):
    """first half: start-up, then partial <-> full with holds of 1 .. 24 steps -- at 30 rows a step every threshold of both ladders lies
    between two of the `i + j * step_size` these reach -- a third of them after a first partial phase of 30 .. 85 steps (the two sides of
    time1_start_p_f); second half: sticky random actions (stand-by, cooldown and the restarts that meet the catalyst thresholds)"""
    a = np.zeros((K, n), np.int32)
    for e in range(n // 2):
        a[:4, e] = 2
        t, cur = 4, 3
        hold = int(rng.integers(30, 86)) if e % 3 == 0 else int(rng.integers(1, 25))
        while t < K:
            a[t:t + hold, e] = cur
            t, cur, hold = t + hold, 7 - cur, int(rng.integers(1, 25))
    a[:, n // 2:] = H.sticky_tape(rng, K, n - n // 2, 1 / 5.0)
    return a


def test_one_id_per_live_key():
    assert len(H.CFG_CASES) == 5 and len(CASE_OF) >= 60 and "time23_p_f_p" not in CASE_OF
    assert {CASE_OF[k] for k in CASE_OF} >= set(HOT_FIRST)


@pytest.mark.parametrize("key", sorted(CASE_OF))
def test_one_key_at_its_default_vs_oracle(key):
    from rl_ptg_amd.engine import HipEngine
    case = CASE_OF[key]
    tr, consts, _, market = H.load_traj(case)
    assert consts[key] != tr["meta"]["defaults"][key]
    consts = dict(consts, train_or_eval=0)                  # (eval mode would send every single step to the generic kernel)
    consts[key] = tr["meta"]["defaults"][key]
    S = consts["sim_step"] // consts["time_step_op"]
    tables = _small_tables(S)
    hot_possible = consts["price_ahead"] == 13
    eps_ind = market["eps_ind"]

    def engine(route, out_dtype):
        if route == "generic":
            os.environ["PTG_NO_HOT_KERNELS"] = "1"
        try:
            eng = HipEngine(consts, tables, H.market_for_engine(consts, market), N, device=0, out_dtype=out_dtype, obs_layout="row")
        finally:
            os.environ.pop("PTG_NO_HOT_KERNELS", None)
        if eps_ind is not None:
            eng.set_episode_plan(eps_ind, N, N)
        return eng

    def oracle(c, acts):
        ora = H.po.OracleVecEnv(c, tables, market, N, ep_index0=0)
        ora.set_noise_tape(tape)
        o0, _ = ora.reset()
        refs = [ora.step(acts[t])[:3] for t in range(K1 + K2)]
        ints, f64s = ora.state()
        assert not any(r[2].any() for r in refs)            # no episode ends inside: the hot kernels take every step
        assert max(ora.noise_count(e) for e in range(N)) <= L
        ora.close()
        return o0, refs, ints, f64s

    eng = engine("hot", "float32")                          # N(0, consts["noise"]) from the device generator: `noise` is read here
    eng.fill_noise_tape(seed=61, per_env_len=L)
    tape = eng.get_noise_tape(L)
    eng.close()
    assert abs(tape.std() - consts["noise"]) < 0.05 * consts["noise"]
    # the action tape: the first of 20 on which the ORACLE tells this key's default from its edited value beyond the float32 tolerance
    # (or in an integer) -- on such a tape a kernel that read another value for the key cannot pass
    edited = dict(consts, **{key: tr["meta"]["consts"][key]})
    for attempt in range(20):
        rng = np.random.default_rng(6200 + 100 * sorted(CASE_OF).index(key) + attempt)
        acts = _tape(rng, K1 + K2, N)
        if consts["action_type"]:
            acts = (-1 + 0.4 * (acts + 0.5) + rng.uniform(-0.19, 0.19, acts.shape)).astype(np.float32)
        o0, refs, ints, f64s = oracle(consts, acts)
        if key in ("noise", "time_step_op"):                # the noise tape's scale (asserted above); another window length: other tables
            break
        _, refs_e, ints_e, _ = oracle(edited, acts)
        if not np.array_equal(ints, ints_e) or any(not np.allclose(x[q], y[q], rtol=RTOL32, atol=ATOL32) for x, y in zip(refs, refs_e) for q in (0, 1)):
            break
    else:
        raise AssertionError(f"no tape on which {key} matters")
    for route in ("hot", "generic"):
        for out_dtype in ("float32", "float64"):
            rtol, atol = (RTOL64, ATOL64) if out_dtype == "float64" else (RTOL32, ATOL32)
            eng = engine(route, out_dtype)
            eng.set_noise_tape(tape)
            msg = f"{key} at its default ({case}), {route} route, {out_dtype}"
            np.testing.assert_allclose(eng.rows(eng.reset()).cpu().numpy(), o0, rtol=rtol, atol=atol, err_msg=msg)
            eng.profile(True)
            for t in range(K1):
                o, r, d = eng.step(acts[t])
                eng.sync()
                np.testing.assert_allclose(eng.rows(o).cpu().numpy(), refs[t][0], rtol=rtol, atol=atol, err_msg=f"{msg}: obs, step {t}")
                H.assert_rewards(r.cpu().numpy(), refs[t][1], out_dtype, err_msg=f"{msg}: reward, step {t}")
                assert not d.cpu().numpy().any()
            o, r, d = eng.rollout(acts[K1:])
            eng.sync()
            launched = len(eng.profile_read())
            eng.profile(False)
            assert launched == ((K1 + 1) if route == "hot" and hot_possible else 0), f"{msg}: {launched} hot launches"
            o, r = eng.rows(o).cpu().numpy(), r.cpu().numpy()
            for t in range(K2):
                np.testing.assert_allclose(o[t], refs[K1 + t][0], rtol=rtol, atol=atol, err_msg=f"{msg}: obs, fused step {t}")
                H.assert_rewards(r[t], refs[K1 + t][1], out_dtype, err_msg=f"{msg}: reward, fused step {t}")
            assert not d.cpu().numpy().any()
            for col, name in enumerate(INT_FIELDS):
                assert np.array_equal(eng.get_state(name), ints[:, col]), f"{msg}: {name}"
            assert np.array_equal(eng.get_state("T_cat"), f64s[:, 2]), msg
            np.testing.assert_allclose(eng.get_state("cum_rew"), f64s[:, 1], rtol=1e-11, atol=1e-9, err_msg=msg)
            eng.close()
