"""Shared fixture loading for the parity tests (test infrastructure; may import the oracle)."""
import atexit
import contextlib
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
CFG_CASES = [c for c in TRAJ_CASES if c.startswith("cfg_")]          # recorded under an edited config_env.yaml (make_golden.py config)
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
    # a fixture made on generated process tables carries them (tab_<name>); the others use the shipped set of their load level
    tables = {k: tr[f"tab_{k}"] for k in po.TABLE_KEYS} if "tab_cooldown" in tr else load_tables(meta["operation"])
    return tr, dict(meta["consts"]), tables, market


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


# ------------------------------------------------------------------------------------------------ synthetic process tables
DEST_KEYS = ["cooldown", "standby_up", "standby_down", "startup_cold", "startup_hot", "op1_start_p"]      # _get_index destinations, lookup order
# magnitudes of the shipped tables' columns n_h2, n_ch4, n_h2_res, m_h2o, P_el (their largest entries; no row is copied)
COL_HI = np.array([0.0485, 0.0118, 0.0027, 1.55, 1750.0])
# (lowest, highest) fraction of COL_HI per column, by the role of a table
_LEVELS = {"startup": [(0.0, 0.15), (0.0, 0.14), (0.0, 0.04), (0.0, 0.001), (0.1, 1.0)],
           "idle": [(0.0, 0.08), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0006), (0.0, 0.4)],
           "partial": [(0.14, 0.45), (0.14, 0.42), (0.03, 0.6), (0.0, 0.6), (0.08, 0.37)],
           "full": [(0.4, 1.0), (0.4, 1.0), (0.1, 1.0), (0.3, 1.0), (0.1, 0.28)]}


def _role(key):
    if key.startswith("startup"):
        return "startup"
    if key in ("cooldown", "standby_down", "standby_up"):
        return "idle"
    return "partial" if key in ("op1_start_p", "op4_p_f_p_5", "op5_p_f_p_10", "op6_p_f_p_15", "op7_p_f_p_22", "op8_f_p") else "full"


def make_tables(rng, spec):
    """The 17 process tables as `[rows, 7]` float64 arrays (columns t, T_cat, n_h2, n_ch4, n_h2_res, m_h2o, P_el), generated.

    spec: rows      {table: rows}; tables not named get `default_rows` (an int, or (lo, hi) drawn per table)
          grid      1-D array of distinct catalyst temperatures.  With `cover` (default) every grid value occurs in at least one table,
                    so the number of distinct temperatures of the set is exactly len(grid) (+ 1 when 16.0, the reset temperature, is
                    not in the grid)
          grid_of   {table: 1-D array}: that table draws from its own values instead (tie families: destinations on even, sources on
                    odd integers); such tables take no part in the covering
          shape     {table: "rise" | "fall" | "tent"}; default: cooldown and standby_down fall, start-up tables and standby_up rise,
                    load tables go up and come back
    Like the shipped tables, a temperature column is not monotonic (neighbouring rows are swapped at random) and holds runs of equal
    values wherever a table has more rows than temperatures; flows and power follow slow waves at the shipped tables' magnitudes, low for
    the idle tables and high for the load tables, and the second half of cooldown draws no power at all (rewards of exactly zero)."""
    grid = np.unique(np.asarray(spec["grid"], dtype=np.float64))
    rows, own = dict(spec.get("rows", {})), spec.get("grid_of", {})
    dr = spec.get("default_rows", 2500)
    for k in po.TABLE_KEYS:
        if k not in rows:
            rows[k] = int(dr) if np.isscalar(dr) else int(rng.integers(dr[0], dr[1] + 1))
    # which temperatures each table uses
    vals = {}
    for k in po.TABLE_KEYS:
        src = np.unique(np.asarray(own[k], dtype=np.float64)) if k in own else grid
        m = max(1, min(int(rows[k] * rng.uniform(0.3, 0.7)), int(len(src) * rng.uniform(0.35, 1.0))))
        vals[k] = np.sort(rng.choice(src, size=m, replace=False))
    free = [k for k in po.TABLE_KEYS if k not in own]
    if spec.get("cover", True) and free:
        missing = np.setdiff1d(grid, np.concatenate([vals[k] for k in free]))
        for k in sorted(free, key=lambda k: len(vals[k]) - rows[k]):
            take = min(len(missing), rows[k] - len(vals[k]))
            vals[k] = np.union1d(vals[k], missing[:take])
            missing = missing[take:]
        if len(missing):
            raise ValueError(f"{len(missing)} temperatures of the grid do not fit into the tables' rows")
    out = {}
    for k in po.TABLE_KEYS:
        n, v = rows[k], vals[k]
        m = len(v)
        idx = np.sort(np.concatenate([np.arange(m), rng.integers(0, m, n - m)]))
        shape = spec.get("shape", {}).get(k) or ("fall" if k in ("cooldown", "standby_down") else
                                                "rise" if _role(k) == "startup" or k == "standby_up" else "tent")
        if shape == "fall":
            idx = idx[::-1].copy()
        elif shape == "tent":
            idx = np.concatenate([idx[::2], idx[1::2][::-1]])
        for p in np.flatnonzero(rng.random(max(n - 1, 0)) < 0.15):          # not monotonic
            idx[p], idx[p + 1] = idx[p + 1], idx[p]
        a = np.zeros((n, 7))
        a[:, 0] = 2.0 * np.arange(n)
        a[:, 1] = v[idx]
        u = np.arange(n) / max(n, 64)
        for c, (lo, hi) in enumerate(_LEVELS[_role(k)]):
            wave = 0.5 + 0.5 * np.sin(2 * np.pi * (rng.uniform(0.5, 3.0) * u + rng.random()))
            a[:, 2 + c] = COL_HI[c] * (lo + (hi - lo) * wave) * np.abs(1.0 + 0.02 * rng.normal(size=n))
        if k == "cooldown":
            a[n // 2:, 2:] = 0.0
        out[k] = a
    return out


def count_lookup_ties(tables, t_initial=16.0):
    """(keys x destination tables) pairs whose nearest temperature is tied between two DIFFERENT table temperatures, one on each side of
    the key: there `_get_index` depends on "the first minimum wins"."""
    keys = np.unique(np.concatenate([tables[k][:, 1] for k in po.TABLE_KEYS] + [np.array([t_initial])]))
    ties = 0
    for k in DEST_KEYS:
        col = np.unique(tables[k][:, 1])
        d = np.abs(col[None, :] - keys[:, None])
        ties += int(np.sum((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1))
    return ties


def sticky_tape(rng, K, n, p=1 / 12.0):
    a = np.zeros((K, n), np.int32)
    cur = rng.integers(0, 5, n)
    for t in range(K):
        cur = np.where(rng.random(n) < p, rng.integers(0, 5, n), cur)
        a[t] = cur
    return a


def toggler_tape(rng, K, n, warm):
    """start-up for `warm` steps, then holds of random length over all five actions with a bias towards partial <-> full toggles (the
    tape of test_fuzz_config.py as an array)"""
    a = np.zeros((K, n), np.int32)
    hold = rng.integers(1, 14, n)
    cur = rng.integers(0, 5, n)
    for t in range(K):
        if t < warm:
            a[t] = 2
            continue
        flip = (t - warm) % hold == 0
        toggle = rng.random(n) < 0.6
        cur = np.where(flip, np.where(toggle & (cur >= 3), 7 - cur, rng.integers(0, 5, n)), cur)
        a[t] = cur
    return a


# ------------------------------------------------------------------------------------------------ engine shells on the CPU
def host_engine(n, **attrs):
    """a HipEngine shell on the CPU: enough for the Python argument checks of the training ops, which run before anything touches the
    library (the tests assert `eng._L is None` after every refusal)"""
    import torch
    from rl_ptg_amd.engine import HipEngine
    eng = HipEngine.__new__(HipEngine)
    eng._torch, eng.n, eng.device, eng._h, eng._L = torch, n, torch.device("cpu"), None, None
    eng.out_dtype, eng.obs_dim, eng.feature_major, eng.pitch = torch.float32, 3, False, n
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


class RecordingLib:
    """stands in for the loaded library: every attribute is a function that stores (name, args) in `calls` and returns 0 --
    ptg_policy_loss_workspace returns the size the library computes (32 bytes + 88 per block of 256 rows, < 0 for a batch < 1)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if name == "ptg_policy_loss_workspace":
                return 32 + 88 * ((args[0] + 255) // 256) if args[0] >= 1 else -1
            return 0
        return f


class CpuTorch:
    """torch, except that cuda.device(...) is a null context"""

    class cuda:
        device = staticmethod(lambda *a, **kw: contextlib.nullcontext())

    def __getattr__(self, name):
        import torch
        return getattr(torch, name)


def recording_engine(n, **attrs):
    """host_engine whose accepted calls run on CPU tensors up to the library call, which a RecordingLib keeps in eng._L.calls"""
    return host_engine(n, _h="H", _L=RecordingLib(), _torch=CpuTorch(), _stream=lambda: None, **attrs)


def mlp_layers(fan_in, widths):
    """zero weights and biases of a net fan_in -> widths[0] -> widths[1] ..."""
    import torch
    ws, bs, k = [], [], fan_in
    for o in widths:
        ws.append(torch.zeros(o, k))
        bs.append(torch.zeros(o))
        k = o
    return ws, bs


def faulty_mlp_nets(B=6):
    """(exception, kwargs) for every faulty (x, x2, weights, biases, activations) that mlp_forward's argument checks are tested with
    (tests/test_mlp_host.py); mlp_backward must refuse each in the same words (tests/test_mlp_backward_host.py).  The good net under
    them: x [B, 40] and x2 [B, 1] into 41 -> 8 -> 8 -> 5"""
    import torch
    x, x2 = torch.zeros(B, 40), torch.zeros(B, 1)
    ws, bs = mlp_layers(41, [8, 8, 5])
    other = torch.device("meta")
    f = lambda **kw: {**dict(x=x, weights=ws, biases=bs, x2=x2), **kw}
    g = lambda x, net: dict(x=x, weights=net[0], biases=net[1])
    sub = lambda xs, l, t: xs[:l] + [t] + xs[l + 1:]
    t, v = TypeError, ValueError
    return [
        # what the values are
        (t, f(x=x.numpy())), (t, f(x=x.double())), (t, f(x=None)), (t, f(x2=x2.half())),
        (t, f(weights=ws[0])), (t, f(biases=None)), (t, f(weights=sub(ws, 1, ws[1].double()))),
        (t, f(biases=sub(bs, 2, bs[2].long()))), (t, f(weights=sub(ws, 0, None))),
        (t, f(x=torch.zeros(B, 2, 3), weights=sub(ws, 1, ws[1].double()))),        # TypeError before the ValueError of another argument
        (t, f(hidden_activation="gelu", x=x.double())),
        # the names, the counts
        (v, f(hidden_activation="gelu")), (v, f(hidden_activation=None)), (v, f(out_activation="sigmoid")),
        (v, f(weights=[], biases=[])), (v, f(biases=bs[:2])), (v, g(x, mlp_layers(40, [4] * 11))),
        # shapes, strides, devices
        (v, f(x=torch.zeros(B))), (v, f(x=torch.zeros(B, 2, 3))), (v, f(x=torch.zeros(40, B).t())),
        (v, f(x=torch.zeros(1, 40).expand(B, 40))), (v, f(x=torch.zeros(B, 40, device=other))),
        (v, f(x2=torch.zeros(B + 1, 1))), (v, f(x2=torch.zeros(B, 2))), (v, f(x2=None)),
        (v, f(x=x[:0], x2=x2[:0])), (v, f(x2=torch.zeros(B, 0))), (v, f(x=torch.zeros(B, 80)[:, ::2])),
        (v, g(torch.zeros(B, 1025), mlp_layers(1025, [4]))), (v, g(x, mlp_layers(40, [1025, 4]))), (v, g(x, mlp_layers(40, [4, 1025]))),
        (v, f(weights=sub(ws, 1, torch.zeros(8, 9)))), (v, f(weights=sub(ws, 0, torch.zeros(41, 8).t()))),
        (v, f(weights=sub(ws, 2, torch.zeros(5, 8, device=other)))), (v, f(biases=sub(bs, 0, torch.zeros(9)))),
        (v, f(biases=sub(bs, 0, torch.zeros(16)[::2]))), (v, f(biases=sub(bs, 1, torch.zeros(8, 1)))),
    ]
