"""Process tables OTHER than the two shipped sets against the CPU oracle.  Everything the kernels read is derived from the 17 tables
when a handle is created (`build_tables`: window records, the `_get_index` lookup, the sorted temperature list and the threshold keys,
the 16-bit lookup copy and whether it lives in LDS); the rest of the suite only ever hands it `tables_OP1.npz` / `tables_OP2.npz`.  The
families below are generated (`helpers.make_tables`) and each names the reference behaviour it is there for:

  short_S300, short_S30   tables of 1, 2, 63, 64, 65, S - 1, S, S + 1, 2 S + 1 rows: `_perform_sim_step` (env/ptg_gym_env.py:525-557) where a
                          table is shorter than one window -- `op_head` plus the `np.ones(...) * operation[-1]` padding, the start-up
                          hand-over `next_operation[:time_overhead]` reaching S - 1 rows into op1_start_p, op1_start_p of exactly S rows --
                          and `np.average` (:454-458) over such windows; `_get_index` (:514-523) over tables shorter than a wave;
                          short_S30 resets on the LAST row of cooldown
  tiny_nT                 five distinct temperatures: a lookup of 30 entries (one partly filled 1 KiB row in LDS); both start-up thresholds
                          and the stand-by threshold outside the temperature range (:339-342 never fires: hot_cold stays 0; :579
                          always picks standby_down)
  ties                    integer-spaced destination tables queried from the half-way temperatures of the other tables: `diff.argmin()`
                          keeps the FIRST minimum; 16.0, the reset temperature (:117), half-way between two cooldown rows; thresholds exactly
                          on table temperatures that envs sit on (the last rows of cooldown, standby_up, op3_p_f, op8_f_p), so the `<=` /
                          `>=` of :339-342 and :579 are decided by equality -- counted from the oracle's state (`_OnThreshold`)
  shipped_order           ~5 000 temperatures like the shipped sets, thresholds above every temperature (hot_cold stays 0, stand-by always
                          standby_up), the reset row the first row of cooldown
  nT_10000                the largest kind of lookup that still lives in LDS: 118 one-KiB rows staged by 16 workgroups, so the per-workgroup
                          rotation of the staging order (`rows / 32` = 3) is not 0 or 1 as on the shipped sets
  nT_14000, nT_32767      a lookup that cannot live in LDS beside the tiles; the largest temperature count the state word can hold;
                          t_cat_startup_hot below every temperature (hot_cold is 1 from the first step on)
  big_cooldown            70 000 rows of cooldown: `_get_index` results >= 65 536, so no 16-bit lookup copy exists; reset lands there
  big_full                70 000 rows of op3_p_f entered at i_fully_developed = 65 000 (:243, :276): row indices >= 65 536 with the 16-bit
                          lookup in place
  generic_pa6,            price_ahead = 6: every step, fused ones included, takes the generic kernel, which reads the int32 lookup and the
  big_cooldown_pa6        float64 records -- on the tie tables and on the 70 000-row cooldown

Every family runs through `ptg_step` (hot kernel, generic kernel on the terminating step) and `ptg_rollout` against `OracleVecEnv` on the
same action and noise tapes, all envs and all steps compared, and proves from the handle or from the oracle's state that it took the
branch it is named after."""
import numpy as np
import pytest

import helpers as H

RTOL64, ATOL64 = 1e-11, 1e-13          # the project's own tolerances (test_fuzz_config.py)
RTOL32, ATOL32 = 2e-7, 1e-9
TID = {k: i for i, k in enumerate(H.po.TABLE_KEYS)}
SPLICED = ("startup_cold", "startup_hot")

_SHORT300 = dict(startup_cold=299, startup_hot=65, cooldown=601, standby_down=64, standby_up=63, op1_start_p=300, op2_start_f=301,
                 op3_p_f=2, op4_p_f_p_5=1, op5_p_f_p_10=2500, op6_p_f_p_15=300, op7_p_f_p_22=299, op8_f_p=301, op9_f_p_f_5=64,
                 op10_f_p_f_10=1, op11_f_p_f_15=3000, op12_f_p_f_20=65)
_SHORT30 = dict(startup_cold=29, startup_hot=31, cooldown=61, standby_down=1, standby_up=2, op1_start_p=30, op2_start_f=63,
                op3_p_f=64, op4_p_f_p_5=65, op5_p_f_p_10=30, op6_p_f_p_15=31, op7_p_f_p_22=29, op8_f_p=2000, op9_f_p_f_5=1,
                op10_f_p_f_10=2, op11_f_p_f_15=3000, op12_f_p_f_20=64)
_TIES = dict(startup_cold=400, startup_hot=63, cooldown=1500, standby_down=65, standby_up=300, op1_start_p=700, op2_start_f=64,
             op3_p_f=900, op8_f_p=1100)

# the tie families' thresholds sit exactly on table temperatures that the trajectories reach (see _tables): the last row of cooldown is its
# only coldest one, the last row of standby_up its only hottest one, and op3_p_f / op8_f_p end on the stand-by threshold
_TIE_THRESHOLDS = dict(t_cat_startup_cold=1.0, t_cat_startup_hot=598.0, t_cat_standby=251.0)

# name -> (seed, n_envs, out_dtype, layout, synthetic_spec arguments, constants, what the handle / the oracle must show)
FAMILIES = {
    "short_S300": (1, 65, "float64", "row", dict(), dict(), dict(lds_lut=1, has_lut16=1)),
    # (sim_step = 60: a day has 1 440 steps; eps_sim_steps is set so that episodes end on the 141st step)
    "short_S30": (2, 512, "float32", "feature", dict(sim_step=60), dict(eps_sim_steps=146), dict(lds_lut=1, has_lut16=1, i_reset=60)),
    "tiny_nT": (3, 512, "float32", "row", dict(), dict(t_cat_startup_cold=-5.0, t_cat_startup_hot=1000.0, t_cat_standby=-3.0),
                dict(lds_lut=1, has_lut16=1, key_cold_max=-1, key_hot_min="nT", key_standby_max=-1, hot={0})),
    "ties": (4, 777, "float32", "row", dict(), _TIE_THRESHOLDS,
             dict(lds_lut=1, has_lut16=1, hot={0, 1}, ties=True)),
    "shipped_order": (5, 512, "float64", "feature", dict(), dict(t_cat_startup_cold=700.0, t_cat_startup_hot=800.0, t_cat_standby=700.0),
                      dict(lds_lut=1, has_lut16=1, key_cold_max="nT-1", key_standby_max="nT-1", hot={0}, i_reset=0)),
    "nT_10000": (11, 1000, "float32", "row", dict(), dict(), dict(lds_lut=1, has_lut16=1, hot={0, 1})),
    "nT_14000": (6, 1000, "float32", "sb3_flat", dict(), dict(t_cat_startup_cold=-1.0, t_cat_startup_hot=-0.5),
                 dict(lds_lut=0, has_lut16=1, key_cold_max=-1, key_hot_min=0, hot={1})),
    "nT_32767": (7, 65, "float32", "row", dict(), dict(), dict(lds_lut=0, has_lut16=1, nT=32767, hot={0, 1})),
    "big_cooldown": (8, 256, "float64", "row", dict(), dict(), dict(lds_lut=0, has_lut16=0, big_i="cooldown", hot={0, 1})),
    "big_full": (9, 512, "float32", "feature", dict(), dict(i_fully_developed=65000, j_fully_developed=2, time1_f_p_f=5000, time1_p_f_p=5000),
                 dict(lds_lut=1, has_lut16=1, big_i="op3_p_f")),
    "big_cooldown_pa6": (8, 130, "float64", "row", dict(price_ahead=6), dict(), dict(has_lut16=0, big_i="cooldown", hot={0, 1}, generic=True)),
    "generic_pa6": (10, 130, "float32", "row", dict(price_ahead=6), _TIE_THRESHOLDS,
                    dict(hot={0, 1}, ties=True, generic=True)),
}
_cache = {}


def _tables(name):
    """the family's tables (generated once per process)"""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(9000 + FAMILIES[name][0])
    lin = lambda g: np.linspace(0.0, 598.7, g)
    if name == "short_S300":
        t = H.make_tables(rng, dict(rows=_SHORT300, grid=np.append(lin(300), 16.0)))
    elif name == "short_S30":
        t = H.make_tables(rng, dict(rows=_SHORT30, grid=lin(300)))
        t["cooldown"][-1, 1] = 16.0                     # the reset row is the last row of cooldown
    elif name == "tiny_nT":
        t = H.make_tables(rng, dict(grid=[3.5, 120.0, 260.25, 400.0, 598.7], default_rows=(300, 2500)))
    elif name in ("ties", "generic_pa6"):
        even, odd = np.arange(0.0, 600.0, 2.0), np.arange(1.0, 600.0, 2.0)
        own = {k: (odd if k == "cooldown" or k not in H.DEST_KEYS else even) for k in H.po.TABLE_KEYS}
        t = H.make_tables(rng, dict(rows=_TIES, default_rows=(1, 65), grid=np.arange(0.0, 600.0), grid_of=own))
        t["cooldown"] = t["cooldown"][t["cooldown"][:, 1] != 16.0]
        t["cooldown"][-3:-1, 1] = (17.0, 15.0)          # the reset temperature half-way between two rows
        # an env that walks to the end of a table stays on its last row, so these temperatures are reached exactly, step after step
        cd, su = t["cooldown"], t["standby_up"]
        cd[cd[:, 1] <= 1.0, 1] = 3.0
        cd[-1, 1] = 1.0                                 # == t_cat_startup_cold, arrived at from above
        su[su[:, 1] >= 598.0, 1] = 596.0
        su[-1, 1] = 598.0                               # == t_cat_startup_hot, arrived at from below
        t["op3_p_f"][-1, 1] = t["op8_f_p"][-1, 1] = 251.0      # == t_cat_standby when stand-by is entered from the end of a load table
    elif name == "shipped_order":
        t = H.make_tables(rng, dict(grid=np.append(lin(5000)[lin(5000) > 16.0], 16.0), default_rows=(2000, 4000), shape=dict(cooldown="rise")))
        t["cooldown"][0, 1] = 16.0
    elif name == "nT_10000":
        t = H.make_tables(rng, dict(grid=lin(10000), default_rows=(2500, 4000)))
    elif name == "nT_14000":
        t = H.make_tables(rng, dict(grid=lin(14000), default_rows=(2500, 4000)))
    elif name == "nT_32767":
        t = H.make_tables(rng, dict(grid=lin(32766), default_rows=(2500, 3500)))
    elif name in ("big_cooldown", "big_cooldown_pa6"):
        t = H.make_tables(rng, dict(rows=dict(cooldown=70000), grid=lin(5000), default_rows=(2000, 3000)))
    elif name == "big_full":
        t = H.make_tables(rng, dict(rows=dict(op3_p_f=70000), grid=lin(300), default_rows=(2000, 3000)))
    _cache[name] = t
    return t


def _setup(name):
    """-> (spec, consts for the engine, consts for the oracle, tables, market of the oracle)"""
    from rl_ptg_amd.prep import synthetic_spec
    seed, n, out_dtype, layout, sargs, over, expect = FAMILIES[name]
    sim_step = sargs.get("sim_step", 600)
    spec, _ = synthetic_spec(scenario=1 + seed % 3, operation="OP2", eps_len_d=1, sim_step=sim_step, price_ahead=sargs.get("price_ahead", 13),
                             train_steps=60 * 8 * (86400 // sim_step))
    base = dict(spec.consts, noise=10.0, **over)
    m = spec.markets[0]
    consts = dict(base, scenario=m["scenario"], rew_l_b=m["rew_l_b"], rew_u_b=m["rew_u_b"], r_0=m["r_0"])
    return spec, base, consts, _tables(name), dict(m, eps_ind=spec.eps_ind)


def _tapes(name, K):
    seed, n = FAMILIES[name][:2]
    rng = np.random.default_rng(9100 + seed)
    sim_step = FAMILIES[name][4].get("sim_step", 600)
    acts = H.toggler_tape(rng, K, n, warm=max(3, 3600 // sim_step))
    acts[:, n // 2:] = H.sticky_tape(rng, K, n - n // 2, 1 / 6.0)
    return acts, rng.normal(0.0, 10.0, size=(n, 96))


K1, K2 = 150, 130          # steps through ptg_step, then through ptg_rollout: the 139th and the 278th step end an episode (eps_len_d = 1)


def _big_row(ints, which, S):
    """the largest window start i + (j - 1) S among the envs that are inside the 70 000-row table `which`, 0 if none is"""
    inside = (ints[:, 0] == 1) if which == "cooldown" else (ints[:, 0] == 4) & (ints[:, 7] == TID[which])
    row = ints[:, 1] + np.maximum(ints[:, 2] - 1, 0) * S
    row = row[inside & (row < 70000)]
    return int(row.max()) if len(row) else 0


def _prove_ties(tables):
    """NumPy alone, before a GPU is touched: the lookup holds exact ties, the reset temperature among them"""
    assert H.count_lookup_ties(tables) > 100
    cd = np.unique(tables["cooldown"][:, 1])
    assert 16.0 not in cd and 15.0 in cd and 17.0 in cd


class _OnThreshold:
    """Counts, from the oracle's state before each step, the env-steps on which a comparison with a threshold is decided by equality:
    T_cat == t_cat_startup_cold with hot_cold still 1 (`<=` of :339 turns it 0), T_cat == t_cat_startup_hot with hot_cold still 0 (`>=` of
    :341 turns it 1), and _standby entered with T_cat == t_cat_standby (`<=` of :579 picks standby_up)."""

    def __init__(self, consts):
        self.c, self.cold, self.hot, self.standby = consts, 0, 0, 0

    def before_step(self, ora, acts):
        ints, f64 = ora.state()
        T, hc, st = f64[:, 2], ints[:, 3], ints[:, 0]
        self.cold += int(np.sum((T == self.c["t_cat_startup_cold"]) & (hc == 1)))
        self.hot += int(np.sum((T == self.c["t_cat_startup_hot"]) & (hc == 0)))
        self.standby += int(np.sum((T == self.c["t_cat_standby"]) & (np.asarray(acts) == 0) & (st != 0)))

    def check(self):
        assert self.cold > 0 and self.hot > 0 and self.standby > 0, (self.cold, self.hot, self.standby)


def _np_argmin_lut(tables, T):
    return np.stack([np.argmin(np.abs(tables[k][:, 1][None, :] - T[:, None]), axis=1) for k in H.DEST_KEYS]).astype(np.int32)


def _np_window(tables, key, r, S):
    """the slice `_perform_sim_step` hands to step() for a window that starts at row r of `key` (r == n: every row the last one)"""
    tab = tables[key]
    n = len(tab)
    if r + S <= n:
        return tab[r:r + S]
    if r == n:
        return np.ones((S, 7)) * tab[-1]
    if key in SPLICED:
        return np.concatenate((tab[r:], tables["op1_start_p"][:r + S - n]), axis=0)
    return np.concatenate((tab[r:], np.ones((r + S - n, 7)) * tab[-1]), axis=0)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_runs_every_family(name):
    """The oracle takes every family to the end without an error code, and the family has what it is named after (NumPy and the oracle
    alone): ties in the lookup, both / one value of hot_cold, a row index >= 65 536, rewards of both signs and of exactly zero."""
    seed, n, out_dtype, layout, sargs, over, expect = FAMILIES[name]
    spec, base, consts, tables, market = _setup(name)
    assert sorted(tables) == sorted(H.po.TABLE_KEYS) and all(a.shape[1] == 7 and a.dtype == np.float64 for a in tables.values())
    if expect.get("ties"):
        _prove_ties(tables)
    on_thr = _OnThreshold(consts)
    n = min(n, 130)
    acts, tape = _tapes(name, K1 + K2)
    acts, tape = acts[:, -n:], tape[-n:]
    ora = H.po.OracleVecEnv(consts, tables, market, n, ep_index0=0)
    ora.set_noise_tape(tape)
    ora.reset()
    hot, rews, dones, imax = set(), [], 0, 0
    for t in range(K1 + K2):
        on_thr.before_step(ora, acts[t])
        _, r, d, _, _ = ora.step(acts[t])
        li, _ = ora.last()
        hot |= set(li[:, 3].tolist())
        if expect.get("big_i"):
            imax = max(imax, _big_row(li, expect["big_i"], consts["sim_step"] // consts["time_step_op"]))
        rews.append(r)
        dones += int(d.sum())
    ora.close()
    if expect.get("ties"):
        on_thr.check()
    rews = np.concatenate(rews)
    assert dones >= n                                      # an episode end falls inside
    assert rews.min() < 0 < rews.max()
    if "hot" in expect:
        assert hot == expect["hot"], hot
    if expect.get("big_i"):
        assert imax > 65535, imax
    if name in ("short_S300", "big_cooldown", "big_cooldown_pa6"):
        assert np.any(rews == 0.0)


def test_generated_tables_keep_the_shipped_tables_character():
    """not monotonic, runs of equal temperature, every grid temperature used (the count of distinct temperatures is exact)"""
    t = _tables("nT_14000")
    allT = np.unique(np.concatenate([a[:, 1] for a in t.values()] + [np.array([16.0])]))
    assert len(allT) == 14001
    for k, a in t.items():
        d = np.diff(a[:, 1])
        assert (d > 0).any() and (d < 0).any(), k
    assert any((np.diff(a[:, 1]) == 0).any() for a in t.values())
    assert len(np.unique(np.concatenate([a[:, 1] for a in _tables("nT_32767").values()] + [np.array([16.0])]))) == 32767


# ------------------------------------------------------------------------------------------------ GPU: what build_tables made
def _engine(name, n=None, out_dtype=None, layout=None):
    from rl_ptg_amd.engine import HipEngine
    seed, n0, dt0, lay0, sargs, over, expect = FAMILIES[name]
    spec, base, consts, tables, market = _setup(name)
    n = n or n0
    eng = HipEngine(base, tables, spec.markets, n, device=0, out_dtype=out_dtype or dt0, obs_layout=layout or lay0)
    eng.set_episode_plan(spec.eps_ind, n, n)
    return eng, H.po.OracleVecEnv(consts, tables, market, n, ep_index0=0)


def _check_plan(name, eng, tables):
    expect = FAMILIES[name][6]
    plan = eng.debug_table_plan()
    nT = plan["nT"]
    assert nT == len(np.unique(np.concatenate([a[:, 1] for a in tables.values()] + [np.array([16.0])])))
    for k in ("lds_lut", "has_lut16", "nT", "key_cold_max", "key_hot_min", "key_standby_max", "i_reset"):
        if k in expect:
            want = {"nT": nT, "nT-1": nT - 1}.get(expect[k], expect[k])
            assert plan[k] == want, (k, plan)
    if expect.get("ties"):          # each threshold IS a table temperature, and its key is that temperature's
        T = np.unique(np.concatenate([a[:, 1] for a in tables.values()] + [np.array([16.0])]))
        c = FAMILIES[name][5]
        assert T[plan["key_cold_max"]] == c["t_cat_startup_cold"] and T[plan["key_hot_min"]] == c["t_cat_startup_hot"]
        assert T[plan["key_standby_max"]] == c["t_cat_standby"]
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in FAMILIES if not k.endswith("_pa6")])
def test_device_built_lookup_and_records(name):
    """k_build_argmin == np.argmin(np.abs(T_col - Tq)) for every key x 6 destinations; k_build_records == np.average of the reference's
    slice, bit for bit, for EVERY start row 0 .. n of tables up to 700 rows and for both ends plus a stride of the longer ones; the reset
    state == the oracle's."""
    spec, base, consts, tables, market = _setup(name)
    if FAMILIES[name][6].get("ties"):
        _prove_ties(tables)
    eng, ora = _engine(name, n=64, out_dtype="float64", layout="row")
    S = consts["sim_step"] // consts["time_step_op"]
    plan = _check_plan(name, eng, tables)
    T, lut = eng.debug_get_index_lut()
    assert np.array_equal(T, np.unique(np.concatenate([a[:, 1] for a in tables.values()] + [np.array([16.0])])))
    ref = _np_argmin_lut(tables, T)
    assert np.array_equal(lut, ref), f"{int((lut != ref).sum())} lookup entries differ"
    assert (ref.max() > 65535) == (not plan["has_lut16"])
    for key in H.po.TABLE_KEYS:
        n = len(tables[key])
        starts = range(n + 1) if n <= 700 else sorted(set(list(range(0, 3)) + list(range(max(0, n - S - 2), n + 1)) + list(range(0, n, 997))))
        for r in starts:
            win = _np_window(tables, key, r, S)
            rec = eng.debug_window_record(TID[key], r)
            assert rec[0] == win[-1, 1], (key, r)
            assert T[int(rec[6])] == win[-1, 1], (key, r)
            for c in range(5):
                assert rec[1 + c] == np.average(win[:, 2 + c]), (key, r, c)
    o_ref, _ = ora.reset()
    np.testing.assert_allclose(eng.reset().cpu().numpy(), o_ref, rtol=RTOL64, atol=ATOL64)
    ints, f64s = ora.state()
    assert plan["i_reset"] == ints[0, 1] == int(np.argmin(np.abs(tables["cooldown"][:, 1] - 16.0)))
    for col, f in [(0, "meth_state"), (1, "i"), (2, "j"), (3, "hot_cold"), (8, "k")]:
        assert np.array_equal(eng.get_state(f), ints[:, col]), f
    assert np.array_equal(eng.get_state("T_cat"), f64s[:, 2])
    if name == "big_cooldown":
        assert plan["i_reset"] > 65535
    eng.close(); ora.close()


# ------------------------------------------------------------------------------------------------ GPU: trajectories
def _run(name, out_dtype=None, layout=None):
    seed, n, dt0, lay0, sargs, over, expect = FAMILIES[name]
    out_dtype, layout = out_dtype or dt0, layout or lay0
    spec, base, consts, tables, market = _setup(name)
    if expect.get("ties"):
        _prove_ties(tables)
    eng, ora = _engine(name, out_dtype=out_dtype, layout=layout)
    plan = _check_plan(name, eng, tables)
    on_thr = _OnThreshold(consts)
    acts, tape = _tapes(name, K1 + K2)
    eng.set_noise_tape(tape)
    ora.set_noise_tape(tape)
    rtol, atol = (RTOL64, ATOL64) if out_dtype == "float64" else (RTOL32, ATOL32)
    flat = layout == "sb3_flat"
    if flat:
        import sb3_flat_oracle as sfo
    conv = (lambda o: sfo.flatten_rows(o, "mod")) if flat else (lambda o: o)
    o_ref, _ = ora.reset()
    np.testing.assert_allclose(eng.rows(eng.reset()).cpu().numpy(), conv(o_ref), rtol=rtol, atol=atol)
    ret, abs_ret, length, fin_exp = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), []
    hot, imax = set(), 0

    def account(r_ref, d_ref):
        nonlocal ret, abs_ret, length, imax, hot
        li, _ = ora.last()
        hot |= set(li[:, 3].tolist())
        if expect.get("big_i"):
            imax = max(imax, _big_row(li, expect["big_i"], consts["sim_step"] // consts["time_step_op"]))
        ret += r_ref; abs_ret += np.abs(r_ref); length += 1
        for e in np.flatnonzero(d_ref):
            fin_exp.append((int(e), int(length[e]), ret[e], abs_ret[e]))
        w = d_ref.astype(bool)
        ret[w], abs_ret[w], length[w] = 0.0, 0.0, 0

    hot_route = not expect.get("generic")
    for t in range(K1):
        o, r, d = eng.step(acts[t])
        eng.sync()
        on_thr.before_step(ora, acts[t])
        o_ref, r_ref, d_ref, _, _ = ora.step(acts[t])
        np.testing.assert_allclose(eng.rows(o).cpu().numpy(), conv(o_ref), rtol=rtol, atol=atol, err_msg=f"obs step {t}")
        H.assert_rewards(r.cpu().numpy(), r_ref, out_dtype, err_msg=f"reward step {t}")
        assert np.array_equal(d.cpu().numpy().astype(bool), d_ref.astype(bool)), f"done step {t}"
        account(r_ref, d_ref)
        if expect.get("big_i"):
            assert np.array_equal(eng.get_state("i"), ora.state()[0][:, 1]), f"i after step {t}"
    assert (eng.rollout_launches(K2) < K2) == hot_route          # the generic kernels are launched once per step, the fused one is not
    obs, rew, done = eng.rollout(acts[K1:])
    eng.sync()
    obs, rew, done = obs.cpu(), rew.cpu().numpy(), done.cpu().numpy()
    for t in range(K2):
        on_thr.before_step(ora, acts[K1 + t])
        o_ref, r_ref, d_ref, _, _ = ora.step(acts[K1 + t])
        np.testing.assert_allclose(eng.rows(obs[t]).numpy(), conv(o_ref), rtol=rtol, atol=atol, err_msg=f"obs fused step {t}")
        H.assert_rewards(rew[t], r_ref, out_dtype, err_msg=f"reward fused step {t}")
        assert np.array_equal(done[t].astype(bool), d_ref.astype(bool)), f"done fused step {t}"
        account(r_ref, d_ref)
    ints, f64s = ora.state()
    for col, f in [(0, "meth_state"), (1, "i"), (2, "j"), (3, "hot_cold"), (4, "standby_tid"), (5, "startup_tid"), (6, "partial_tid"),
                   (7, "full_tid"), (8, "k"), (9, "current_action"), (11, "act_ep_d")]:
        assert np.array_equal(eng.get_state(f), ints[:, col]), f
    assert np.array_equal(eng.get_state("act_ep_d") * 24, ints[:, 10])
    assert np.array_equal(eng.get_state("noise_count"), [ora.noise_count(e) for e in range(n)])
    assert np.array_equal(eng.get_state("T_cat"), f64s[:, 2])
    # the five flows of the last step are columns of the last observation (compared above); cum_rew: float64 accumulation of rewards that
    # agree to a few ulp -- 1e-9 of the summed magnitudes (test_fuzz_config.py)
    assert np.all(np.abs(eng.get_state("cum_rew") - f64s[:, 1]) <= 1e-9 * abs_ret)
    r, l, ids = eng.finished_episodes()
    got, exp = sorted(zip(ids.tolist(), l.tolist(), r.tolist())), sorted(fin_exp)
    assert len(got) == len(exp) and len(exp) >= n
    for (e1, l1, r1), (e2, l2, r2, a2) in zip(got, exp):
        assert e1 == e2 and l1 == l2 and abs(r1 - r2) <= 1e-9 * a2, (e1, e2, l1, l2, r1, r2)
    if "hot" in expect:
        assert hot == expect["hot"], hot
    if expect.get("big_i"):
        assert imax > 65535, imax
    if expect.get("ties"):
        on_thr.check()
    eng.close(); ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_vs_oracle(name):
    _run(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,out_dtype,layout", [("short_S300", "float32", "feature"), ("ties", "float64", "row"),
                                                   ("big_cooldown", "float32", "row"), ("nT_14000", "float64", "feature")])
def test_family_vs_oracle_other_dtype(name, out_dtype, layout):
    """the other output type of the fused kernel (float32 <-> float64) on the families whose branch sits in the kernels themselves"""
    _run(name, out_dtype, layout)


# ------------------------------------------------------------------------------------------------ GPU: refusals
def _create_error(tables, **over):
    from rl_ptg_amd.engine import HipEngine, PtgError
    spec, base, consts, _, market = _setup("short_S300")
    with pytest.raises(PtgError) as ei:
        HipEngine(dict(base, **over), tables, spec.markets, 8, device=0, out_dtype="float64")
    assert ei.value.code == -1          # PTG_E_INVALID
    return str(ei.value)


@pytest.mark.gpu
def test_ptg_create_refuses_what_the_reference_cannot_run():
    good = _tables("short_S300")
    t = dict(good, op6_p_f_p_15=np.zeros((0, 7)))
    assert "table 10 is empty" in _create_error(t)
    t = dict(good, standby_up=good["standby_up"].copy())
    t["standby_up"][7, 1] = np.nan
    assert "NaN temperature in table 4 row 7" in _create_error(t)
    t = dict(good, op1_start_p=good["op1_start_p"][:299])
    assert "op1_start_p is shorter than one step" in _create_error(t)
    rng = np.random.default_rng(5)
    t = H.make_tables(rng, dict(grid=np.append(np.linspace(0.0, 598.7, 32766), 600.0), default_rows=(2500, 3500)))
    assert "more than 32767 distinct catalyst temperatures (32768)" in _create_error(t)
