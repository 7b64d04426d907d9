"""Differential fuzz against the CPU oracle with constants OTHER than the reference's config_env.yaml defaults: a user of the reference
edits that file (thresholds of the partial / full-load ladders `config/config_env.yaml:133-155`, catalyst temperature thresholds `:130-131`,
noise `:28`, prices and species constants `:104-120`, normalisation bounds `:158-173`, step size `:27`), and every one of those values
reaches the kernels through `ptg_config`.  (The oracle is pinned to the reference off the defaults by the edited-config fixtures,
tests/golden/traj_cfg_*.npz, constant by constant: tests/test_config_liveness.py.)  Each seed draws a configuration, drives 65 .. 1 000 envs through the step path
(`ptg_step`: hot kernel, generic kernel on the terminating step) and the fused path (`ptg_rollout`) with actions that visit every handler,
and compares every observation, reward, done flag and the final integer state with `oracle/ptg_oracle.c` on the same action and noise tapes.
Integers bit-exact, floats within the tolerances below."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

RTOL64, ATOL64 = 1e-11, 1e-13
RTOL32, ATOL32 = 2e-7, 1e-9


def _draw_config(rng, consts, rng2):
    """rng: the draws this test has always made, in their order; rng2: the constants added later (a generator of their own, so that
    every value drawn before -- these constants, the noise tape, the actions -- is what it was)"""
    c = dict(consts)
    c["noise"] = float(rng.choice([0.0, 2.5, 10.0, 40.0]))
    cold = float(rng.uniform(40.0, 220.0))
    c["t_cat_startup_cold"] = cold
    c["t_cat_startup_hot"] = cold + float(rng.uniform(20.0, 260.0))
    c["t_cat_standby"] = float(rng.uniform(100.0, 420.0))
    # ladders: any integers are legal (the reference only compares); scaled copies of the defaults keep every rung reachable
    f = float(rng.uniform(0.4, 2.2))
    for k in ("time1_p_f_p", "time2_p_f_p", "time_p_f", "time3_p_f_p", "time34_p_f_p", "time4_p_f_p", "time45_p_f_p", "time5_p_f_p",
              "time23_p_f_p", "time2_start_f_p"):
        c[k] = max(1, int(round(consts[k] * f + rng.integers(-3, 4))))
    g = float(rng.uniform(0.4, 2.2))
    for k in ("time1_f_p_f", "time_f_p", "time2_f_p_f", "time23_f_p_f", "time3_f_p_f", "time34_f_p_f", "time4_f_p_f", "time45_f_p_f",
              "time5_f_p_f"):
        c[k] = max(1, int(round(consts[k] * g + rng.integers(-3, 4))))
    c["time1_start_p_f"] = int(rng.integers(200, 3000))
    c["i_fully_developed"] = int(rng.integers(2000, 20000))
    c["j_fully_developed"] = int(rng.integers(5, 160))
    for k in ("heat_price", "o2_price", "water_price", "eeg_el_price"):
        c[k] = float(consts[k] * rng.uniform(0.3, 2.0))
    c["eta_CHP"] = float(rng.uniform(0.2, 0.6))
    c["min_load_electrolyzer"] = float(rng.choice([0.032, 0.1, 0.3]))
    c["T_l_b"], c["T_u_b"] = float(rng.uniform(0, 20)), float(rng.uniform(500, 700))
    c["heat_u_b"] = float(rng.uniform(900, 2500))
    c["el_l_b"], c["el_u_b"] = float(rng.uniform(-30, 0)), float(rng.uniform(60, 120))
    c["state_change_penalty"] = float(rng.choice([0.0, 0.0, 0.25]))
    # ---- appended: the constants the draws above leave at their defaults.  Upper bounds stay above lower bounds and every range at
    # least half its default width, as for the edited-config fixtures (tests/golden/make_golden.py, edited_config)
    c["gas_l_b"], c["gas_u_b"] = float(rng2.uniform(0.0, 2.0)), float(rng2.uniform(20.0, 45.0))          # live with raw features only
    c["eua_l_b"], c["eua_u_b"] = float(rng2.uniform(5.0, 30.0)), float(rng2.uniform(80.0, 130.0))
    for k in ("h2", "ch4", "h2_res", "h2o"):              # the lower bounds default to 0: a normalisation that drops one is exact there
        c[f"{k}_u_b"] = float(consts[f"{k}_u_b"] * rng2.uniform(0.8, 1.3))
        c[f"{k}_l_b"] = float(consts[f"{k}_u_b"] * rng2.uniform(0.0, 0.2))
    c["heat_l_b"] = float(rng2.uniform(0.0, c["heat_u_b"] - 900.0))
    for k in ("H_u_CH4", "H_u_H2", "dt_water", "cp_water", "rho_water", "Molar_mass_CO2", "Molar_mass_H2O", "h_H2O_evap"):
        c[k] = float(consts[k] * rng2.uniform(0.85, 1.15))
    c["convert_mol_to_Nm3"] = float(consts["convert_mol_to_Nm3"] * rng2.uniform(0.9, 1.1))
    c["max_h2_volumeflow"] = c["convert_mol_to_Nm3"] * c["h2_u_b"]          # as EnvConfiguration derives it (src/rl_config_env.py:33)
    # (ch4_price_fix is no field of ptg_config: it reaches the kernels as the gas series of business scenario 2)
    return c


@pytest.mark.parametrize("seed", range(16))
def test_random_constants_vs_oracle(seed):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    rng = np.random.default_rng(7000 + seed)
    scenario = 1 + seed % 3
    operation = "OP1" if seed % 2 else "OP2"
    sim_step = int(rng.choice([60, 120, 300, 600, 1200]))
    raw_modified = "raw" if seed % 4 == 3 else "mod"
    action_type = "continuous" if seed % 3 == 1 else "discrete"
    out_dtype = "float64" if seed % 2 else "float32"
    layout = ["row", "feature", "row", "sb3_flat"][seed % 4] if out_dtype == "float32" else ["row", "feature"][(seed // 2) % 2]
    spec, _ = synthetic_spec(scenario=scenario, operation=operation, eps_len_d=4, sim_step=sim_step, raw_modified=raw_modified,
                             action_type=action_type, train_steps=60 * 8 * (4 * 86400 // sim_step))
    base = _draw_config(rng, spec.consts, np.random.default_rng(7100 + seed))
    n, K1, K2 = [512, 777, 65, 1000][(seed // 4) % 4], 150, 130      # ragged last waves / workgroups too
    m = spec.markets[0]
    eng = HipEngine(base, spec.tables, spec.markets, n, device=0, out_dtype=out_dtype, obs_layout=layout)
    eng.set_episode_plan(spec.eps_ind, n, n)
    tape = rng.normal(0.0, base["noise"], size=(n, 96)) if base["noise"] > 0 else np.zeros((n, 96))
    eng.set_noise_tape(tape)
    consts = dict(base, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])
    ora = H.po.OracleVecEnv(consts, spec.tables, dict(m, eps_ind=spec.eps_ind), n, ep_index0=0)
    ora.set_noise_tape(tape)
    rtol, atol = (RTOL64, ATOL64) if out_dtype == "float64" else (RTOL32, ATOL32)
    flat = layout == "sb3_flat"
    if flat:
        import sb3_flat_oracle as sfo      # oracle/ is on sys.path through helpers

    def ref_rows(o):
        return sfo.flatten_rows(o, raw_modified) if flat else o

    o_ref, _ = ora.reset()
    np.testing.assert_allclose(eng.rows(eng.reset()).cpu().numpy(), ref_rows(o_ref), rtol=rtol, atol=atol)
    abs_sum = np.zeros(n)                                    # sum of |reward| of each env's current episode: the cum_rew bound
    # actions: a start-up phase, then holds of random length over all five actions with a bias towards partial <-> full toggles
    warm = max(3, int(3600 * float(rng.uniform(0.5, 2.5)) / sim_step))
    hold = rng.integers(1, 14, n)
    cur = rng.integers(0, 5, n)

    def next_actions(t):
        nonlocal cur
        if t < warm:
            a = np.full(n, 2)
        else:
            flip = (t - warm) % hold == 0
            toggle = rng.random(n) < 0.6
            cur = np.where(flip, np.where(toggle & (cur >= 3), 7 - cur, rng.integers(0, 5, n)), cur)
            a = cur.copy()
        if action_type == "continuous":
            return (-1 + 0.4 * (a + 0.5) + rng.uniform(-0.19, 0.19, n)).astype(np.float32)
        return a.astype(np.int32)

    for t in range(K1):
        acts = next_actions(t)
        o, r, d = eng.step(acts)
        eng.sync()
        o_ref, r_ref, d_ref, _, _ = ora.step(acts)
        np.testing.assert_allclose(eng.rows(o).cpu().numpy(), ref_rows(o_ref), rtol=rtol, atol=atol, err_msg=f"obs step {t}")
        H.assert_rewards(r.cpu().numpy(), r_ref, out_dtype, err_msg=f"reward step {t}")
        assert np.array_equal(d.cpu().numpy().astype(bool), d_ref.astype(bool)), f"done step {t}"
        abs_sum = np.where(d_ref.astype(bool), 0.0, abs_sum + np.abs(r_ref))
    acts = np.stack([next_actions(K1 + t) for t in range(K2)])
    obs, rew, done = eng.rollout(acts)
    eng.sync()
    obs, rew, done = obs.cpu(), rew.cpu().numpy(), done.cpu().numpy()
    for t in range(K2):
        o_ref, r_ref, d_ref, _, _ = ora.step(acts[t])
        np.testing.assert_allclose(eng.rows(obs[t]).numpy(), ref_rows(o_ref), rtol=rtol, atol=atol, err_msg=f"obs fused step {t}")
        H.assert_rewards(rew[t], r_ref, out_dtype, err_msg=f"reward fused step {t}")
        assert np.array_equal(done[t].astype(bool), d_ref.astype(bool)), f"done fused step {t}"
        abs_sum = np.where(d_ref.astype(bool), 0.0, abs_sum + np.abs(r_ref))
    ints, f64s = ora.state()
    for col, name in [(0, "meth_state"), (1, "i"), (2, "j"), (3, "hot_cold"), (4, "standby_tid"), (5, "startup_tid"),
                      (6, "partial_tid"), (7, "full_tid"), (8, "k"), (9, "current_action"), (11, "act_ep_d")]:
        assert np.array_equal(eng.get_state(name), ints[:, col]), name
    assert np.array_equal(eng.get_state("T_cat"), f64s[:, 2])
    # float64 accumulation of rewards that agree to a few ulp: 1e-9 of the summed magnitudes in either output dtype
    assert np.all(np.abs(eng.get_state("cum_rew") - f64s[:, 1]) <= 1e-9 * abs_sum)
    eng.close(); ora.close()
