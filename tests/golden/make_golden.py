#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):   python tests/golden/make_golden.py
The reference is imported behind the stand-in `gymnasium` of oracle/refharness (gymnasium / SB3 are not
installable here; nothing was denied).  Outputs are data only: inputs (price series, action tapes, recorded
normal draws, constants) and the reference's outputs (integer state, float state, observations, info rows).

Files written
  market_real.npz            the reference's real price series as its loader returns them (3 splits)
  tables_OP{1,2}.npz  ->     written to rl_ptg_amd/data/ (the 17 process tables per load level; product input)
  prep_<mkt>_bs<k>_<op>.npz  per business scenario / load level: series the env sees, pot_rew / part_full,
                             bounds, r_level, T-OPT totals  (reference: load_data + Preprocessing)
  traj_<case>.npz            trajectories of n reference envs stepped in DummyVecEnv order
  units_<op>.npz             _get_index for every distinct T_cat x 6 destination tables
`make_golden.py tables` writes only the trajectories on generated process tables (synthetic_table_cases), `make_golden.py config`
only the fixtures under an edited config_env.yaml (edited_config_cases: traj_cfg_*, prep_cfg_*, cfg_liveness.json).
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle", "refharness"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import helpers as H                          # noqa: E402  (table generator, action tapes)
import ref_driver as rd                      # noqa: E402
import ptg_oracle as po                      # noqa: E402
from rl_ptg_amd.synthetic import synthetic_market_csv_units  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(ROOT, "rl_ptg_amd", "data")


def jsonable(d):
    out = {}
    for k, v in d.items():
        if isinstance(v, (np.floating, np.integer)):
            v = v.item()
        out[k] = v
    return out


def synth_markets():
    return {"train": synthetic_market_csv_units(38, 20250614),
            "val": synthetic_market_csv_units(9, 20250615),
            "test": synthetic_market_csv_units(9, 20250616)}


def sticky_tape(rng, K, n, p=1 / 12.0):
    """tests/helpers.sticky_tape (same draws), as the int64 the fixtures above were recorded with"""
    return H.sticky_tape(rng, K, n, p).astype(np.int64)


def toggler_tape(rng, K, n, max_hold=25, warm=None):
    """startup until production, then partial/full toggling with short random holds (+ rare detours)."""
    a = np.zeros((K, n), np.int64)
    for e in range(n):
        t = 0
        w = warm if warm is not None else int(rng.integers(150, 400))
        while t < K:
            a[t:t + w, e] = 2
            t += w
            seg_end = min(K, t + int(rng.integers(300, 900)))
            cur = 3
            first = True
            while t < seg_end:
                hold = int(rng.integers(1, max_hold + 1))
                if first and rng.random() < 0.5:
                    hold = int(rng.integers(30, 80))        # long first partial phase -> op3 branch later
                first = False
                a[t:t + hold, e] = cur
                t += hold
                cur = 7 - cur
            det = int(rng.integers(0, 2))                   # detour: standby or cooldown
            hold = int(rng.integers(5, 60))
            a[t:t + hold, e] = det
            t += hold
            w = int(rng.integers(20, 200))
    return a[:K]


def to_continuous(rng, a):
    """discrete tape -> float32 actions inside the matching interval, with the decode edge cases injected."""
    centers = -1 + 0.4 * (a + 0.5)
    x = (centers + rng.uniform(-0.19, 0.19, a.shape)).astype(np.float32)
    edges = np.array([-1.0, 1.0, np.nan, -1.5, 1.5, -0.6, -0.2, 0.2, 0.6, 0.99999994, -0.99999994,
                      np.nextafter(np.float32(-0.6), np.float32(1)), np.nextafter(np.float32(0.2), np.float32(-1)),
                      np.nextafter(np.float32(0.6), np.float32(-1)), 0.0, -0.0, 5.0, -5.0, np.inf, -np.inf],
                     dtype=np.float32)
    K, n = a.shape
    pos = rng.choice(K, size=min(K // 3, 6 * len(edges)), replace=False)
    for q, t in enumerate(np.sort(pos)):
        x[t, q % n] = edges[q % len(edges)]
    return x


def save_prep(name, setup, extra_meta):
    pre, price = setup.pre, setup.price
    kw = {s: setup.kwargs(s) for s in ("train", "val", "test")}
    arrs = {}
    for s in ("train", "val", "test"):
        arrs[f"el_{s}"] = price[f"el_price_{s}"].astype(np.float64)
        arrs[f"gas_{s}"] = np.asarray(price[f"gas_price_{s}"], dtype=np.float64)
        arrs[f"eua_{s}"] = np.asarray(price[f"eua_price_{s}"], dtype=np.float64)
        arrs[f"pot_rew_{s}"] = pre.dict_pot_r_b[f"pot_rew_{s}"].astype(np.float64)
        arrs[f"part_full_{s}"] = pre.dict_pot_r_b[f"part_full_b_{s}"].astype(np.int8)
        # cross-check the series folding used by every consumer of these fixtures
        c, t, m = po.split_reference_kwargs(kw[s], "train")
        P = kw[s]["price_ahead"]
        assert np.array_equal(m["el"], arrs[f"el_{s}"][:len(m["el"])]) and len(m["el"]) == len(arrs[f"el_{s}"]) - 1
        assert np.array_equal(m["pot_rew"], arrs[f"pot_rew_{s}"][:len(m["pot_rew"])])
        assert np.array_equal(m["part_full"], arrs[f"part_full_{s}"][:len(m["part_full"])].astype(float))
        assert np.array_equal(m["gas"], arrs[f"gas_{s}"]) and np.array_equal(m["eua"], arrs[f"eua_{s}"])
    consts, _, _ = po.split_reference_kwargs(kw["train"], "train")
    meta = dict(consts=jsonable(consts), r_level=float(pre.r_level[0]), n_eps=int(pre.n_eps),
                eps_sim_steps=dict(train=int(pre.eps_sim_steps_train), val=int(pre.eps_sim_steps_val),
                                   test=int(pre.eps_sim_steps_test)),
                rew_l_b=float(kw["train"]["rew_l_b"]), rew_u_b=float(kw["train"]["rew_u_b"]),
                operation=setup.EnvConfig.operation, scenario=int(setup.EnvConfig.scenario),
                seed_train=int(setup.TrainConfig.seed_train), train_steps=int(setup.TrainConfig.train_steps),
                **extra_meta)
    arrs["eps_ind"] = np.asarray(pre.eps_ind, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, f"prep_{name}.npz"), meta=json.dumps(meta), **arrs)
    print(f"  prep_{name}.npz  n_eps={pre.n_eps} eps_ind={len(pre.eps_ind)} r_level={pre.r_level[0]:.8f}")


def save_traj(case, setup, prep_name, split, train_or_eval, actions, seed, kw_over=None, note="", extra_meta=None, tables=None):
    """tables: a generated table set handed to the reference in place of the one it loaded; it is stored in the fixture (tab_<name>)"""
    kw = dict(setup.kwargs(split))
    kw.update(kw_over or {})
    kw.update(tables or {})
    out = rd.run_vector(kw, actions, seed=seed, train_or_eval=train_or_eval)
    consts, _, market = po.split_reference_kwargs(kw, train_or_eval)
    meta = dict(case=case, prep=prep_name, split=split, train_or_eval=train_or_eval, n_envs=int(actions.shape[1]),
                seed=int(seed), ep_index0=0, consts=jsonable(consts), operation=setup.EnvConfig.operation,
                int_cols=rd.INT_COLS, f64_cols=rd.F64_COLS, info_keys=rd.INFO_KEYS, note=note, **(extra_meta or {}))
    arrs = dict(actions=out["actions"], ints=out["ints"].astype(np.int32), f64s=out["f64s"], obs=out["obs"],
                done=out["done"], noise=out["noise"], noise_len=out["noise_len"], n_noise=out["n_noise"].astype(np.int32),
                reset_obs=out["reset_obs"], reset_int=out["reset_int"].astype(np.int32), reset_info=out["reset_info"],
                post_reset_obs=out["post_reset_obs"], post_reset_int=out["post_reset_int"].astype(np.int32),
                post_reset_at=out["post_reset_at"].astype(np.int32), ep_index_end=out["ep_index_end"],
                eps_ind=np.zeros(0) if market["eps_ind"] is None else market["eps_ind"])
    if "infos" in out:
        arrs["infos"] = out["infos"]
    arrs.update({f"tab_{k}": np.asarray(v, dtype=np.float64) for k, v in (tables or {}).items()})
    np.savez_compressed(os.path.join(OUT, f"traj_{case}.npz"), meta=json.dumps(meta), **arrs)
    ints = out["ints"]
    pt, ft = set(ints[..., 6].reshape(-1).tolist()), set(ints[..., 7].reshape(-1).tolist())
    print(f"  traj_{case}.npz K={actions.shape[0]} n={actions.shape[1]} dones={int(out['done'].sum())} "
          f"noise={out['noise_len'].tolist()} partial_tids={sorted(pt)} full_tids={sorted(ft)} "
          f"sum_rew={out['f64s'][..., 0].sum():.6f} zero_rew={(out['f64s'][..., 0] == 0).mean():.2f}")
    return out


def save_units(setup, op):
    kw = setup.kwargs("train")
    m = rd._import_reference()
    env = m["ptg"].PTGEnv(kw, "train")
    allT = np.unique(np.concatenate([kw[k][:, 1] for k in rd.TABLE_KEYS] + [np.array([16.0])]))
    dests = ["cooldown", "standby_up", "standby_down", "startup_cold", "startup_hot", "op1_start_p"]
    idx = np.zeros((len(dests), len(allT)), np.int32)
    for d, k in enumerate(dests):
        for q, T in enumerate(allT):
            idx[d, q] = env._get_index(kw[k], T)
    np.savez_compressed(os.path.join(OUT, f"units_{op}.npz"), T=allT, dests=np.array(dests), get_index=idx)
    print(f"  units_{op}.npz distinct_T={len(allT)}")


def save_tables(setup, op):
    os.makedirs(DATA, exist_ok=True)
    np.savez_compressed(os.path.join(DATA, f"tables_{op}.npz"), **{k: setup.op[k] for k in rd.TABLE_KEYS})
    print(f"  rl_ptg_amd/data/tables_{op}.npz rows={sum(len(setup.op[k]) for k in rd.TABLE_KEYS)}")


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(12345)

    # ---------------- real market data, default episode length (37 d), sim_step 600 ----------------
    print("real / BS2 / OP2")
    s = rd.RefSetup(dict(scenario=2, operation="OP2"))
    save_tables(s, "OP2")
    save_units(s, "OP2")
    save_prep("real_bs2_OP2", s, dict(market="real", eps_len_d=37, sim_step=600))
    # real price series before scenario overrides: BS1 leaves them untouched -> saved from the BS1 setup below
    save_traj("real_bs2_op2_mod_disc_train", s, "real_bs2_OP2", "train", "train",
              rng.integers(0, 5, (700, 3)), 3654, note="uniform-random actions; pins ep_index order (3 init + 3 reset)")
    save_traj("real_bs2_op2_mod_disc_evalval", s, "real_bs2_OP2", "val", "eval",
              sticky_tape(rng, 1500, 2), 605, note="sticky actions, eval mode (info rows)")
    save_traj("real_bs2_op2_raw_cont_test", s, "real_bs2_OP2", "test", "train",
              to_continuous(rng, sticky_tape(rng, 900, 2, 1 / 6.0)), 11, dict(raw_modified="raw", action_type="continuous"),
              note="raw features + continuous actions with decode edge cases")
    s.close()

    print("real / BS1 / OP1")
    s = rd.RefSetup(dict(scenario=1, operation="OP1"))
    save_tables(s, "OP1")
    save_units(s, "OP1")
    save_prep("real_bs1_OP1", s, dict(market="real", eps_len_d=37, sim_step=600))
    np.savez_compressed(os.path.join(OUT, "market_real.npz"),
                        **{f"{c}_{sp}": np.asarray(s.price[f"{c}_price_{sp}"], dtype=np.float64)
                           for c in ("el", "gas", "eua") for sp in ("train", "val", "test")})
    save_traj("real_bs1_op1_raw_cont_evalval", s, "real_bs1_OP1", "val", "eval",
              to_continuous(rng, sticky_tape(rng, 1500, 2)), 605, dict(raw_modified="raw", action_type="continuous"))
    save_traj("real_bs1_op1_mod_disc_train", s, "real_bs1_OP1", "train", "train", rng.integers(0, 5, (600, 2)), 467)
    s.close()

    print("real / BS3 / OP2")
    s = rd.RefSetup(dict(scenario=3, operation="OP2"))
    save_prep("real_bs3_OP2", s, dict(market="real", eps_len_d=37, sim_step=600))
    save_traj("real_bs3_op2_mod_cont_test", s, "real_bs3_OP2", "test", "eval",
              to_continuous(rng, sticky_tape(rng, 1200, 2)), 7, dict(action_type="continuous"))
    s.close()

    # ---------------- synthetic 38-day market (BASELINE.json configurations) ----------------
    sm = synth_markets()
    for scen, op in ((2, "OP2"), (1, "OP1"), (3, "OP2")):
        print(f"synthetic / BS{scen} / {op} / 32-day episodes")
        s = rd.RefSetup(dict(scenario=scen, operation=op, eps_len_d=32), synthetic_market=sm)
        for sp in ("train", "val", "test"):     # the reference's loader must see exactly what the product generator emits
            el, gas, eua = sm[sp]
            assert np.array_equal(s.price[f"el_price_{sp}"], el / 10)
            if scen == 1:
                assert np.array_equal(s.price[f"gas_price_{sp}"], gas / 10) and np.array_equal(s.price[f"eua_price_{sp}"], eua)
        save_prep(f"synth_bs{scen}_{op}", s, dict(market="synth", eps_len_d=32, sim_step=600))
        save_traj(f"synth_bs{scen}_{op.lower()}_mod_disc_train", s, f"synth_bs{scen}_{op}", "train", "train",
                  sticky_tape(rng, 800, 2), 100 + scen, note="BASELINE.json-style configuration (32-day episode, sticky actions)")
        s.close()

    # short episodes -> terminations, auto-reset order over the shared ep_index, state-change penalty
    print("synthetic / BS2 / OP2 / 2-day episodes, penalty")
    s = rd.RefSetup(dict(scenario=2, operation="OP2", eps_len_d=2, state_change_penalty=0.3), synthetic_market=sm,
                    train_steps=20000)
    out = save_traj("synth_bs2_op2_term_penalty", s, "synth_bs2_OP2", "train", "train", sticky_tape(rng, 900, 5, 1 / 5.0), 3654,
                    note="eps_len_d=2 (283-step episodes), 5 envs sharing ep_index, state_change_penalty=0.3")
    assert out["done"].sum() >= 10
    # an env set whose members terminate on different steps: different ep_index order
    s.close()

    # sim_step = 60 s (step_size 30): reaches every rung of the _partial / _full ladders
    for scen, op in ((2, "OP2"), (1, "OP1")):
        print(f"synthetic / BS{scen} / {op} / sim_step 60")
        s = rd.RefSetup(dict(scenario=scen, operation=op, eps_len_d=1, sim_step=60), synthetic_market=sm, train_steps=200000)
        out = save_traj(f"synth_bs{scen}_{op.lower()}_s60_toggle", s, f"synth_bs{scen}_{op}", "train", "train",
                        toggler_tape(rng, 2600, 2), 42 + scen, note="sim_step=60: all _partial/_full ladder rungs; eps_len_d=1 (1435-step episodes)")
        pt, ft = set(out["ints"][..., 6].reshape(-1).tolist()), set(out["ints"][..., 7].reshape(-1).tolist())
        assert pt >= {5, 8, 9, 10, 11, 12} and ft >= {6, 7, 13, 14, 15, 16}, (pt, ft)
        s.close()

    # ---------------- cells added later: each with its own generator, so the files above regenerate byte for byte ----------------
    print("real / BS2 / OP2 / val split, eval mode, one whole validation episode")
    s = rd.RefSetup(dict(scenario=2, operation="OP2"))
    t_end = int(s.pre.eps_sim_steps_val) - 6              # step index of the termination (8 634), then 10 post-reset steps
    n_val = t_end + 1 + 10
    out = save_traj("real_bs2_op2_mod_disc_evalval_full", s, "real_bs2_OP2", "val", "eval",
                    sticky_tape(np.random.default_rng(2001), n_val, 1), 605,
                    note="the whole validation episode: its last steps read gas / EUA day D with D + 2 == n_days")
    assert np.nonzero(out["done"][:, 0])[0].tolist() == [t_end], np.nonzero(out["done"][:, 0])[0]
    s.close()

    print("real / BS3 / OP2 / raw features")
    s = rd.RefSetup(dict(scenario=3, operation="OP2"))
    save_traj("real_bs3_op2_raw_disc_train", s, "real_bs3_OP2", "train", "train",
              np.random.default_rng(2002).integers(0, 5, (600, 2)), 3655, dict(raw_modified="raw"),
              note="BS3 gas / EUA are 0: the normalised raw features are negative constants")
    s.close()

    print("real / BS1 / OP1 / continuous actions")
    s = rd.RefSetup(dict(scenario=1, operation="OP1"))
    g = np.random.default_rng(2003)
    save_traj("real_bs1_op1_mod_cont_train", s, "real_bs1_OP1", "train", "train",
              to_continuous(g, sticky_tape(g, 700, 2)), 468, dict(action_type="continuous"))
    s.close()

    print("synthetic / BS1 / OP1 / sim_step 60, raw features, continuous actions")
    s = rd.RefSetup(dict(scenario=1, operation="OP1", eps_len_d=1, sim_step=60), synthetic_market=sm, train_steps=200000)
    g = np.random.default_rng(2004)
    out = save_traj("synth_bs1_op1_raw_cont_s60_toggle", s, "synth_bs1_OP1", "train", "train",
                    to_continuous(g, toggler_tape(g, 2600, 2)), 44, dict(raw_modified="raw", action_type="continuous"),
                    note="sim_step=60 toggler decoded from continuous actions, raw features: every ladder rung")
    pt, ft = set(out["ints"][..., 6].reshape(-1).tolist()), set(out["ints"][..., 7].reshape(-1).tolist())
    assert pt >= {5, 8, 9, 10, 11, 12} and ft >= {6, 7, 13, 14, 15, 16}, (pt, ft)
    s.close()

    # ---------------- price_ahead other than 13 (config/config_env.yaml:26): observation widths, e_r_b windows, T-OPT ----------------
    print("synthetic / BS2 / OP2 / price_ahead 6, 2-day episodes")
    s = rd.RefSetup(dict(scenario=2, operation="OP2", eps_len_d=2, price_ahead=6), synthetic_market=sm, train_steps=20000)
    save_prep("synth_bs2_OP2_pa6", s, dict(market="synth", eps_len_d=2, sim_step=600, price_ahead=6, t_opt=ref_t_opt(s)))
    g = np.random.default_rng(2005)
    out = save_traj("synth_bs2_op2_pa6_mod_disc_term", s, "synth_bs2_OP2_pa6", "train", "train", sticky_tape(g, 900, 5, 1 / 5.0), 3656,
                    note="price_ahead=6, eps_len_d=2 (283-step episodes): several terminations")
    assert out["done"].sum() >= 10
    s.close()

    print("real / BS1 / OP1 / price_ahead 24, raw features, continuous actions")
    s = rd.RefSetup(dict(scenario=1, operation="OP1", price_ahead=24))
    save_prep("real_bs1_OP1_pa24", s, dict(market="real", eps_len_d=37, sim_step=600, price_ahead=24, t_opt=ref_t_opt(s)))
    g = np.random.default_rng(2006)
    save_traj("real_bs1_op1_pa24_raw_cont_train", s, "real_bs1_OP1_pa24", "train", "train",
              to_continuous(g, sticky_tape(g, 700, 2, 1 / 6.0)), 469, dict(raw_modified="raw", action_type="continuous"),
              note="price_ahead=24, raw features, continuous actions with decode edge cases")
    s.close()

    print("real / BS3 / OP2 / price_ahead 1, raw features")
    s = rd.RefSetup(dict(scenario=3, operation="OP2", price_ahead=1))
    save_prep("real_bs3_OP2_pa1", s, dict(market="real", eps_len_d=37, sim_step=600, price_ahead=1, t_opt=ref_t_opt(s)))
    save_traj("real_bs3_op2_pa1_raw_disc_train", s, "real_bs3_OP2_pa1", "train", "train",
              np.random.default_rng(2007).integers(0, 5, (600, 3)), 3657, dict(raw_modified="raw"),
              note="price_ahead=1: the smallest window")
    s.close()

    print("real / BS2 / OP2 / price_ahead 25, val split, eval mode, one whole validation episode")
    s = rd.RefSetup(dict(scenario=2, operation="OP2", price_ahead=25))
    save_prep("real_bs2_OP2_pa25", s, dict(market="real", eps_len_d=37, sim_step=600, price_ahead=25, t_opt=ref_t_opt(s)))
    t_end = int(s.pre.eps_sim_steps_val) - 6
    n_val = t_end + 1 + 10
    out = save_traj("real_bs2_op2_pa25_mod_disc_evalval_full", s, "real_bs2_OP2_pa25", "val", "eval",
                    sticky_tape(np.random.default_rng(2008), n_val, 1), 606,
                    note="price_ahead=25, the whole validation episode: its last steps read the last hour the reference exposes")
    assert np.nonzero(out["done"][:, 0])[0].tolist() == [t_end], np.nonzero(out["done"][:, 0])[0]

    print("real / BS2 / OP2 / price_ahead 25, test split, eval mode: the reference raises before the episode ends")
    kw = s.kwargs("test")
    acts = sticky_tape(np.random.default_rng(2009), int(s.pre.eps_sim_steps_test), 1)
    t_fail, h_fail = ref_failing_step(kw, acts, 607, "eval")
    save_traj("real_bs2_op2_pa25_mod_disc_evaltest_end", s, "real_bs2_OP2_pa25", "test", "eval", acts[:t_fail], 607,
              note="price_ahead=25, whole test split: the reference raises IndexError on step fail_step (hour fail_h), "
                   "which is not part of the trajectory", extra_meta=dict(fail_step=t_fail, fail_h=h_fail, fail_action=int(acts[t_fail, 0])))
    s.close()
    synthetic_table_cases()
    edited_config_cases()
    print("done")


def synthetic_table_cases():
    """Process tables other than the shipped ones (tests/helpers.make_tables), handed to the unmodified reference: the oracle is pinned
    to it on tables shorter than one window, on exact ties of _get_index and with thresholds outside the temperature range.  Runs on its
    own too (`make_golden.py tables`): the files above are not touched."""
    sm = synth_markets()
    print("synthetic / BS2 / OP2 / generated tables around one window (S = 300), integer temperatures that tie")
    g = np.random.default_rng(3001)
    rows = dict(startup_cold=299, startup_hot=65, cooldown=601, standby_down=64, standby_up=63, op1_start_p=300, op2_start_f=301,
                op3_p_f=2, op4_p_f_p_5=1, op5_p_f_p_10=700, op6_p_f_p_15=300, op7_p_f_p_22=299, op8_f_p=301, op9_f_p_f_5=64,
                op10_f_p_f_10=1, op11_f_p_f_15=900, op12_f_p_f_20=65)
    even, odd = np.arange(0.0, 600.0, 2.0), np.arange(1.0, 600.0, 2.0)
    own = {k: (odd if k == "cooldown" or k not in H.DEST_KEYS else even) for k in rd.TABLE_KEYS}
    tables = H.make_tables(g, dict(rows=rows, grid=np.arange(0.0, 600.0), grid_of=own))
    tables["cooldown"] = tables["cooldown"][tables["cooldown"][:, 1] != 16.0]
    tables["cooldown"][-3:-1, 1] = (17.0, 15.0)
    # thresholds on temperatures the envs sit on: the last rows of cooldown (its only coldest), standby_up (its only hottest), op3_p_f, op8_f_p
    cd, su = tables["cooldown"], tables["standby_up"]
    cd[cd[:, 1] <= 1.0, 1] = 3.0
    cd[-1, 1] = 1.0
    su[su[:, 1] >= 598.0, 1] = 596.0
    su[-1, 1] = 598.0
    tables["op3_p_f"][-1, 1] = tables["op8_f_p"][-1, 1] = 251.0
    assert H.count_lookup_ties(tables) > 100
    s = rd.RefSetup(dict(scenario=2, operation="OP2", eps_len_d=2), synthetic_market=sm, train_steps=20000)
    acts = H.toggler_tape(g, 420, 4, warm=6)
    acts[:, 2:] = H.sticky_tape(g, 420, 2, 1 / 5.0)
    out = save_traj("synth_bs2_tables_short_ties", s, "synth_bs2_OP2", "train", "train", acts, 3660, dict(t_cat_startup_cold=1.0,
                    t_cat_startup_hot=598.0, t_cat_standby=251.0), tables=tables,
                    note="generated tables of 1 .. 2 S + 1 rows (S = 300) on integer temperatures: ties of _get_index, thresholds on table "
                         "temperatures, eps_len_d=2 (283-step episodes)")
    # (both start-up tables are shorter than one window: a start-up hands over to partial load within its first step)
    assert out["done"].sum() >= 4 and set(out["ints"][..., 0].reshape(-1).tolist()) == {0, 1, 3, 4}
    assert set(out["ints"][..., 3].reshape(-1).tolist()) == {0, 1}
    Tc, hc = out["f64s"][:-1, :, 2], out["ints"][:-1, :, 3]            # state a step starts from (no episode end in between matters here)
    n_cold, n_hot = int(((Tc == 1.0) & (hc == 1)).sum()), int(((Tc == 598.0) & (hc == 0)).sum())
    n_sb = int(((Tc == 251.0) & (out["ints"][:-1, :, 0] != 0) & (out["actions"][1:] == 0)).sum())
    print(f"  steps decided by equality with a threshold: cold {n_cold}, hot {n_hot}, stand-by {n_sb}")
    assert n_cold > 0 and n_hot > 0 and n_sb > 0
    s.close()

    print("synthetic / BS1 / OP1 / sim_step 60, generated tables around one window (S = 30), thresholds outside the temperature range")
    g = np.random.default_rng(3002)
    rows = dict(startup_cold=500, startup_hot=31, cooldown=61, standby_down=1, standby_up=2, op1_start_p=30, op2_start_f=63,
                op3_p_f=64, op4_p_f_p_5=65, op5_p_f_p_10=30, op6_p_f_p_15=31, op7_p_f_p_22=29, op8_f_p=500, op9_f_p_f_5=1,
                op10_f_p_f_10=2, op11_f_p_f_15=800, op12_f_p_f_20=64)
    tables = H.make_tables(g, dict(rows=rows, grid=np.linspace(0.0, 598.7, 300)))
    s = rd.RefSetup(dict(scenario=1, operation="OP1", eps_len_d=1, sim_step=60), synthetic_market=sm, train_steps=200000)
    acts = H.toggler_tape(g, 600, 3, warm=20)
    acts[:, 2:] = H.sticky_tape(g, 600, 1, 1 / 8.0)
    out = save_traj("synth_bs1_tables_s30_thresholds_outside", s, "synth_bs1_OP1", "train", "train", acts, 3661,
                    dict(t_cat_startup_cold=-5.0, t_cat_startup_hot=1000.0, t_cat_standby=-3.0), tables=tables,
                    note="generated tables of 1 .. 2 S + 1 rows (S = 30) beside three of 500 .. 800; every threshold outside the tables' temperatures: hot_cold stays 0, "
                         "stand-by always standby_down")
    assert set(out["ints"][..., 0].reshape(-1).tolist()) == {0, 1, 2, 3, 4}
    assert set(out["ints"][..., 3].reshape(-1).tolist()) == {0} and set(out["ints"][..., 4].reshape(-1).tolist()) == {3}
    s.close()


def edited_config():
    """config_env.yaml with every scalar numeric constant moved off its default (scenario, load level, step sizes, episode length and
    price_ahead are set per case).  Keys that share a default get different values -- the six ladder rungs 1, 2, 23, 3, 34, 4 of the two
    directions and time2_start_f_p, the five lower bounds that default to 0.  Kept valid: upper above lower bounds with every range at
    least half its default width, each ladder strictly increasing in the order the reference compares it, t_cat_startup_cold <
    t_cat_startup_hot, the [off, partial, full] entries of meth_stats_load ordered."""
    ov = dict(
        noise=7, state_change_penalty=0.15,
        ch4_price_fix=14.2, heat_price=5.1, o2_price=9.3, water_price=7.5, eeg_el_price=16.9,
        H_u_CH4=36.5, H_u_H2=10.5, h_H2O_evap=2300, dt_water=85, cp_water=4.3, rho_water=970, convert_mol_to_Nm3=0.0229,
        Molar_mass_CO2=46.0, Molar_mass_H2O=19.0, min_load_electrolyzer=0.2, eta_CHP=0.41,
        t_cat_standby=201.5, t_cat_startup_cold=172, t_cat_startup_hot=331,
        # each threshold is moved across a value `time_op = i + j * step_size` takes on the sim_step 60 tape (multiples of 30 from i = 0), so
        # that putting it back changes a decision
        time1_start_p_f=2400, time2_start_f_p=450,
        # partial -> full -> partial, in the order env/ptg_gym_env.py:649-679 walks it
        time1_p_f_p=65, time2_p_f_p=125, time_p_f=230, time23_p_f_p=250, time3_p_f_p=295, time34_p_f_p=395, time4_p_f_p=443,
        time45_p_f_p=575, time5_p_f_p=655,
        # full -> partial -> full (:715-745)
        time1_f_p_f=25, time_f_p=115, time2_f_p_f=159, time23_f_p_f=205, time3_f_p_f=309, time34_f_p_f=355, time4_f_p_f=459,
        time45_f_p_f=505, time5_f_p_f=595,
        i_fully_developed=11000, j_fully_developed=90,
        el_l_b=-12, el_u_b=95, gas_l_b=0.5, gas_u_b=30, eua_l_b=20, eua_u_b=105, T_l_b=8, T_u_b=620, h2_l_b=0.002, ch4_l_b=0.0005,
        h2_res_l_b=0.00002, h2o_l_b=0.05, heat_l_b=40, heat_u_b=1900,
        r_0_values=dict(el_price=[3], gas_price=[7], eua_price=[40]))
    import yaml
    with open(os.path.join(rd.REF, "config", "config_env.yaml")) as f:
        base = yaml.safe_load(f)
    msl = {}
    for op, d in base["meth_stats_load"].items():           # partial load x 1.07, full load x 0.93 (heating: x 1.02 / x 0.98, which keeps OP2's ordered)
        msl[op] = {k: list(v) for k, v in d.items()}
        for k in ("Meth_H2_flow", "Meth_CH4_flow", "Meth_H2_res_flow", "Meth_H2O_flow", "Meth_el_heating"):
            up, dn = (1.02, 0.98) if k == "Meth_el_heating" else (1.07, 0.93)
            msl[op][k] = [d[k][0], d[k][1] * up, d[k][2] * dn]
            assert msl[op][k][0] <= msl[op][k][1] <= msl[op][k][2], (op, k)
    ov["meth_stats_load"] = msl
    scalars = [k for k, v in base.items() if isinstance(v, (int, float)) and not isinstance(v, bool)
               and k not in ("scenario", "price_ahead", "time_step_op", "eps_len_d", "sim_step")]
    assert sorted(k for k in ov if k not in ("meth_stats_load", "r_0_values")) == sorted(scalars)
    assert all(ov[k] != base[k] for k in scalars)
    for grp in (["time1_p_f_p", "time2_p_f_p", "time_p_f", "time23_p_f_p", "time3_p_f_p", "time34_p_f_p", "time4_p_f_p", "time45_p_f_p",
                 "time5_p_f_p"], ["time1_f_p_f", "time_f_p", "time2_f_p_f", "time23_f_p_f", "time3_f_p_f", "time34_f_p_f", "time4_f_p_f",
                                  "time45_f_p_f", "time5_f_p_f"]):
        assert all(ov[a] < ov[b] for a, b in zip(grp, grp[1:])), grp
    ints = [ov[k] for k in scalars if k.startswith("time") or k.endswith("fully_developed")]
    assert len(set(ints)) == len(ints) == 22
    assert ov["t_cat_startup_cold"] < ov["t_cat_startup_hot"]
    for lo, hi in (("el_l_b", "el_u_b"), ("gas_l_b", "gas_u_b"), ("eua_l_b", "eua_u_b"), ("T_l_b", "T_u_b"), ("heat_l_b", "heat_u_b")):
        assert ov[hi] - ov[lo] >= 0.5 * (base[hi] - base[lo]), lo
    for op in msl:
        for lo, k in (("h2_l_b", "Meth_H2_flow"), ("ch4_l_b", "Meth_CH4_flow"), ("h2_res_l_b", "Meth_H2_res_flow"), ("h2o_l_b", "Meth_H2O_flow")):
            assert msl[op][k][2] - ov[lo] >= 0.5 * (base["meth_stats_load"][op][k][2] - base[lo]), (op, lo)
    return ov


# reference kwargs name of an oracle constant
_KW_OF = {"r_0": "reward_level"}
LIVE_SKIP = ("raw_modified", "action_type", "train_or_eval")


def _ref_outputs(kw, actions, seed, train_or_eval):
    out = rd.run_vector(kw, actions, seed=seed, train_or_eval=train_or_eval)
    return {k: np.asarray(out[k]) for k in ("ints", "f64s", "obs", "done", "n_noise", "infos", "post_reset_obs", "post_reset_int",
                                            "post_reset_at", "reset_obs", "reset_int", "reset_info") if k in out}


def liveness(kw, kw_default, actions, seed, train_or_eval):
    """Decided by the reference alone: for every constant of the env's input contract (src/rl_utils.py:337-405) whose value under the
    edited config differs from its value under the default config, the reference env runs again with that one constant put back
    (`prefix` steps of the tape) -> (defaults, {key: dict(max_rel, max_excess, int_changed)} of the keys with any recorded output changed).
    max_excess: the largest |change| / (ATOL32 + RTOL32 |value|) over observations, rewards and info rows."""
    c_e, _, _ = po.split_reference_kwargs(kw, train_or_eval)
    c_d, _, _ = po.split_reference_kwargs(kw_default, train_or_eval)
    keys = [k for k in po.CONST_KEYS if k not in LIVE_SKIP and c_e[k] != c_d[k]]
    base = _ref_outputs(kw, actions, seed, train_or_eval)
    defaults, live = {}, {}
    for k in keys:
        kk = _KW_OF.get(k, k)
        kw1 = dict(kw)
        kw1[kk] = kw_default[kk]
        defaults[k] = c_d[k]
        got = _ref_outputs(kw1, actions, seed, train_or_eval)
        if all(a.shape == got[q].shape and np.array_equal(a, got[q], equal_nan=True) for q, a in base.items()):
            continue
        int_changed = any(base[q].shape != got[q].shape or not np.array_equal(base[q], got[q])
                          for q in ("ints", "done", "n_noise", "post_reset_int", "post_reset_at", "reset_int"))
        rel = exc = 0.0
        for a, b in [(got[q], base[q]) for q in ("obs", "infos", "reset_obs") if q in base] + [(got["f64s"][..., 0], base["f64s"][..., 0])]:
            d = np.abs(a - b)
            nz = b != 0
            rel = max(rel, float(np.max(d[nz] / np.abs(b[nz]))) if nz.any() else 0.0)
            exc = max(exc, float(np.max(d / (H.ATOL32 + H.RTOL32 * np.abs(b)))))
        live[k] = dict(max_rel=rel, max_excess=exc, int_changed=bool(int_changed))
    return defaults, live


def edited_config_cases():
    """Trajectories and Preprocessing products of the unmodified reference under an edited config_env.yaml (`edited_config`), on the
    synthetic markets.  Runs on its own (`make_golden.py config`); the files above are not touched.  Each trajectory's meta carries the
    whole override dict (`env_overrides`), the default value of every constant the edits reach (`defaults`), the keys that are live in
    it (`live_keys`, `liveness`) and the tape prefix the liveness runs used (`live_prefix`); cfg_liveness.json lists the reached
    constants that are dead in every case."""
    sm = synth_markets()
    ov = edited_config()
    cases = [
        # (name, per-case config, train_steps, split, mode, traj kwargs, seed, tape maker, liveness prefix)
        ("a", dict(scenario=2, operation="OP2", eps_len_d=1, sim_step=60), 200000, "train", "train", {}, 4001,
         lambda g: toggler_tape(g, 2600, 2), 2600,
         "edited config, sim_step=60 toggler: every ladder rung with the edited ladders; eps_len_d=1 (1435-step episodes)"),
        ("b", dict(scenario=1, operation="OP1", eps_len_d=2, raw_modified="raw"), 20000, "train", "train", dict(action_type="continuous"), 4002,
         lambda g: to_continuous(g, sticky_tape(g, 700, 3, 1 / 5.0)), 700,
         "edited config, raw features (gas / EUA bounds live), continuous actions with decode edge cases, eps_len_d=2: terminations"),
        ("c", dict(scenario=3, operation="OP2", eps_len_d=32), 1500000, "val", "eval", {}, 4003,
         lambda g: sticky_tape(g, 700, 2, 1 / 6.0), 700,
         "edited config, BS3 (CHP / EEG path), val split in eval mode: the 24 info fields carry every revenue and cost term"),
        ("d", dict(scenario=1, operation="OP1", eps_len_d=2, time_step_op=3, sim_step=120, raw_modified="raw", price_ahead=9), 200000,
         "train", "train", {}, 4004, lambda g: H.toggler_tape(g, 900, 2, warm=70).astype(np.int64), 900,
         "edited config, time_step_op=3 with sim_step=120 (window 40), raw features, price_ahead=9"),
        ("e", dict(scenario=2, operation="OP2", eps_len_d=2, time_step_op=4, sim_step=300, price_ahead=5), 100000, "train", "train",
         dict(action_type="continuous"), 4005, lambda g: to_continuous(g, H.toggler_tape(g, 800, 2, warm=30).astype(np.int64)), 800,
         "edited config, time_step_op=4 with sim_step=300 (window 75), continuous actions, price_ahead=5, eps_len_d=2: a termination"),
    ]
    reached, live_any = set(), set()
    for name, cfg, train_steps, split, mode, kw_over, seed, tape, prefix, note in cases:
        scen, op = cfg["scenario"], cfg["operation"]
        full = dict(ov, **cfg)
        print(f"synthetic / edited config / case {name}: BS{scen} / {op} / {cfg}")
        s = rd.RefSetup(full, synthetic_market=sm, train_steps=train_steps)
        # the same case on the default constants (time_step_op is one of them: only the env reads it)
        s0 = rd.RefSetup({k: v for k, v in cfg.items() if k != "time_step_op"}, synthetic_market=sm, train_steps=train_steps)
        g = np.random.default_rng(seed)
        acts = tape(g)
        kw, kw0 = dict(s.kwargs(split), **kw_over), dict(s0.kwargs(split), **kw_over)
        defaults, live = liveness(kw, kw0, acts[:prefix], seed, mode)
        reached |= set(defaults)
        live_any |= set(live)
        for k, v in live.items():
            print(f"    live {k:24s} max_rel={v['max_rel']:.3e} max_excess={v['max_excess']:.3e} int_changed={v['int_changed']}")
        print(f"    dead here: {sorted(set(defaults) - set(live))}")
        pname = f"cfg_{name}_bs{scen}_{op}"
        pmeta = dict(market="synth", eps_len_d=cfg["eps_len_d"], sim_step=cfg.get("sim_step", 600), price_ahead=cfg.get("price_ahead", 13),
                     env_overrides=full, t_opt=ref_t_opt(s))
        save_prep(pname, s, pmeta)
        tname = f"cfg_{name}_bs{scen}_{op.lower()}_{cfg.get('raw_modified', 'mod')}_{'cont' if kw_over else 'disc'}"
        out = save_traj(tname, s, pname, split, mode, acts, seed, kw_over, note=note,
                        extra_meta=dict(env_overrides=full, defaults=jsonable(defaults), live_keys=sorted(live), liveness=live,
                                        live_prefix=int(prefix)))
        pt, ft = set(out["ints"][..., 6].reshape(-1).tolist()), set(out["ints"][..., 7].reshape(-1).tolist())
        if name == "a":
            assert pt >= {5, 8, 9, 10, 11, 12} and ft >= {6, 7, 13, 14, 15, 16}, (pt, ft)
            assert set(out["ints"][..., 0].reshape(-1).tolist()) == {0, 1, 2, 3, 4}
        if name in ("b", "e"):
            assert out["done"].sum() >= 1
        s.close(); s0.close()
    dead = sorted(reached - live_any)
    with open(os.path.join(OUT, "cfg_liveness.json"), "w") as f:
        json.dump(dict(reached=sorted(reached), dead_everywhere=dead), f, indent=1)
        f.write("\n")
    print(f"  cfg_liveness.json reached={len(reached)} dead_everywhere={dead}")


def ref_t_opt(setup):
    """T-OPT of each split as the reference prints it, unrounded: Meth_cum_reward_stats[-price_ahead] of its own calculate_optimum
    (src/rl_opt.py:145-147), which reads config_env.yaml relative to the working directory"""
    import src.rl_opt as rl_opt
    P = setup.EnvConfig.price_ahead
    cwd = os.getcwd()
    os.chdir(setup.wd)
    try:
        with rd._quiet():
            return {sp: float(rl_opt.calculate_optimum(setup.price[f"el_price_{sp}"], setup.price[f"gas_price_{sp}"],
                                                       setup.price[f"eua_price_{sp}"], sp, setup.EnvConfig.stats_names)
                              ["Meth_cum_reward_stats"][-P]) for sp in ("train", "val", "test")}
    finally:
        os.chdir(cwd)


def ref_failing_step(kw, actions, seed, train_or_eval):
    """Step one reference env (env 0 of run_vector: same seed, same actions) until it raises IndexError -> (step index, the hour
    index act_ep_h + h_step it asked e_r_b for, env/ptg_gym_env.py:442-446)."""
    ptg = rd._import_reference()["ptg"]
    ptg.ep_index = 0
    env = ptg.PTGEnv(kw, train_or_eval)
    env.reset(seed=seed)
    for t in range(actions.shape[0]):
        h = int(env.act_ep_h + math.floor((env.k + 1) * env.time_step_size_sim / 3600))
        try:
            env.step(int(actions[t, 0]))
        except IndexError as ex:
            print(f"  reference raised at step {t} (h = {h}): {ex}")
            assert h == np.asarray(kw["e_r_b"]).shape[2], (h, np.asarray(kw["e_r_b"]).shape)
            return t, h
    raise AssertionError("the reference finished without an IndexError")


if __name__ == "__main__":
    if sys.argv[1:] == ["tables"]:
        synthetic_table_cases()
    elif sys.argv[1:] == ["config"]:
        edited_config_cases()
    else:
        main()
