"""Shared fixture loading for the parity tests (test infrastructure; may import the oracle)."""
import atexit
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ptg_oracle as po  # noqa: E402

TRAJ_CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLD, "traj_*.npz")))
PREP_CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLD, "prep_*.npz")))

_cache = {}

# the reward contract: float64 outputs share the reference's operand order (a few ulp); float32 outputs are one rounding of the
# float64 value (2^-24 relative), so rtol 2e-7 with a floor far below the smallest nonzero reward of the fixtures (3.1e-6);
# an exact zero of the reference stays exactly zero in both
RTOL64, ATOL64 = 1e-11, 1e-13
RTOL32, ATOL32 = 2e-7, 1e-9


def assert_rewards(got, ref, out_dtype, err_msg=""):
    """Rewards of a HIP path against a float64 reference under the contract above.  With PTG_REWARD_ERR_LOG=<file>, the largest
    relative error over the nonzero reference rewards of each test is written to <file> when the process exits."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out_dtype in ("float32", "float64"), out_dtype
    rtol, atol = (RTOL64, ATOL64) if out_dtype == "float64" else (RTOL32, ATOL32)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=err_msg)
    z = ref == 0.0
    assert np.all(got[z] == 0.0), f"{err_msg}: nonzero reward where the reference has exactly 0.0: {got[z][got[z] != 0.0][:8]}"
    if os.environ.get("PTG_REWARD_ERR_LOG") and (~z).any():
        rel = float(np.max(np.abs(got[~z] - ref[~z]) / np.abs(ref[~z])))
        key = (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], out_dtype)
        if not _reward_err:
            atexit.register(_write_reward_err)
        _reward_err[key] = max(rel, _reward_err.get(key, 0.0))


_reward_err = {}


def _write_reward_err():
    with open(os.environ["PTG_REWARD_ERR_LOG"], "a") as f:
        for (test, dt), rel in sorted(_reward_err.items()):
            f.write(f"{test}\t{dt}\t{rel:.3e}\n")


def load_npz(path):
    if path not in _cache:
        z = np.load(path, allow_pickle=False)
        d = {k: z[k] for k in z.files}
        if "meta" in d:
            d["meta"] = json.loads(str(d["meta"]))
        _cache[path] = d
    return _cache[path]


def load_tables(op):
    z = load_npz(os.path.join(ROOT, "rl_ptg_amd", "data", f"tables_{op}.npz"))
    return {k: z[k] for k in po.TABLE_KEYS}


def load_prep(name):
    return load_npz(os.path.join(GOLD, f"prep_{name}.npz"))


def load_traj(case):
    """-> (traj dict, consts, tables, market) with market series taken from the referenced prep fixture, the hourly ones cut to the
    hours the reference env can index (what EnvSpec.from_dict_input makes of them)."""
    tr = load_npz(os.path.join(GOLD, f"traj_{case}.npz"))
    meta = tr["meta"]
    market = dict(_full_series(meta), eps_ind=tr["eps_ind"] if len(tr["eps_ind"]) else None)
    for k in ("el", "pot_rew", "part_full"):          # e_r_b covers all hours but the last, whatever P is
        market[k] = market[k][:-1]
    return tr, dict(meta["consts"]), load_tables(meta["operation"]), market


def _full_series(meta):
    """the split's whole series as Preprocessing makes them (what dict_env_kwargs passes as *_series)"""
    prep = load_prep(meta["prep"])
    sp = meta["split"]
    return dict(el=prep[f"el_{sp}"], pot_rew=prep[f"pot_rew_{sp}"], part_full=prep[f"part_full_{sp}"].astype(np.float64),
                gas=prep[f"gas_{sp}"], eua=prep[f"eua_{sp}"])


def make_oracle(case):
    tr, consts, tables, market = load_traj(case)
    env = po.OracleVecEnv(consts, tables, market, tr["meta"]["n_envs"], ep_index0=tr["meta"]["ep_index0"])
    env.set_noise_tape(tr["noise"])
    return tr, env


def market_for_engine(consts, market, prep_meta=None):
    """oracle-style market dict -> HipEngine market dict (adds the scenario-dependent scalars)."""
    m = {k: market[k] for k in ("el", "pot_rew", "part_full", "gas", "eua")}
    m.update(scenario=consts["scenario"], rew_l_b=consts["rew_l_b"], rew_u_b=consts["rew_u_b"], r_0=consts["r_0"])
    return m


def make_engine(case, out_dtype="float64", n_envs=None, obs_layout="row"):
    """HIP engine on cuda:0 configured exactly like the reference run that produced the fixture."""
    from rl_ptg_amd.engine import HipEngine
    tr, consts, tables, market = load_traj(case)
    n = tr["meta"]["n_envs"] if n_envs is None else n_envs
    eng = HipEngine(consts, tables, market_for_engine(consts, market), n, device=0, out_dtype=out_dtype, obs_layout=obs_layout)
    eng.set_noise_tape(tr["noise"])
    if market["eps_ind"] is not None:
        # DummyVecEnv order: n constructions consume eps_ind[0:n], the first vector reset takes eps_ind[n + e]
        eng.set_episode_plan(market["eps_ind"], first_ptr=n, stride=n)
    return tr, eng


def kwargs_from_fixture(case):
    """A reference-style env kwargs dict (src/rl_utils.py:337-405, price data as 1-D series) rebuilt from a trajectory fixture."""
    tr, consts, tables, market = load_traj(case)
    kw = {k: v for k, v in consts.items() if k not in ("raw_modified", "action_type", "train_or_eval", "r_0")}
    kw.update(raw_modified="mod" if consts["raw_modified"] else "raw",
              action_type="continuous" if consts["action_type"] else "discrete",
              reward_level=np.array([consts["r_0"]]), parallel="Singleprocessing", n_eps_loops=0,
              eps_ind=None if market["eps_ind"] is None else market["eps_ind"].astype(int),
              **{f"{k}_series": v for k, v in _full_series(tr["meta"]).items()})
    kw.update({f"ptg_{k}": i for i, k in enumerate(["standby", "cooldown", "startup", "partial_load", "full_load"])})
    kw.update(tables)
    return tr, kw
