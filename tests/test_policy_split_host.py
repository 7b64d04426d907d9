"""The consumer of the "split" observation layout (rl_ptg_amd/policy_split.py) on the CPU, against an independent construction of
SB3's flat row: canonical rows built from the definition of the observation (windows series[s, h : h + P], gas[s, d : d + 2], ...)
and flattened by oracle/sb3_flat_oracle.py -- not by policy_split.flat_columns, which is under test here.  More than one market set,
'mod' and 'raw', price_ahead 1 / 6 / 13 / 25, and the first and the last valid window of every set."""
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "oracle"))
import sb3_flat_oracle as flat_oracle  # noqa: E402

L_H, L_D = 64, 48            # hours / days per set (deliberately unrelated: a stride taken from the wrong series cannot fit)
U32 = 2.0 ** -24             # unit roundoff of float32


def _case(n_sets, raw_modified, P, seed):
    """-> (series dict of float64 [n_sets, L] arrays holding float32-representable values, canonical rows [N, F] float64,
    split rows [N, 16] float64, (set, hour, day) of every row)"""
    rng = np.random.default_rng(seed)
    f32 = lambda shape: rng.normal(size=shape).astype(np.float32).astype(np.float64)
    series = dict(featA=f32((n_sets, L_H)), featB=f32((n_sets, L_H)), gas_n=f32((n_sets, L_D)), eua_n=f32((n_sets, L_D)))
    sets, hours, days = [], [], []
    for s in range(n_sets):
        # the first and the last valid window of every set, in every combination; then random ones
        edge = [(0, 0), (L_H - P, L_D - 2), (0, L_D - 2), (L_H - P, 0)]
        rnd = [(int(rng.integers(0, L_H - P + 1)), int(rng.integers(0, L_D - 1))) for _ in range(9)]
        for h, d in edge + rnd:
            sets.append(s); hours.append(h); days.append(d)
    sets, hours, days = np.array(sets), np.array(hours), np.array(days)
    N = len(sets)
    status = np.arange(N) % 6                                    # every status value
    rng.shuffle(status)
    env = f32((N, 8))
    win = lambda a, lo, w: np.stack([a[s, l:l + w] for s, l in zip(sets, lo)])
    if raw_modified == "mod":
        market = [win(series["featA"], hours, P), win(series["featB"], hours, P)]
    else:
        market = [win(series["featA"], hours, P), win(series["gas_n"], days, 2), win(series["eua_n"], days, 2)]
    canon = np.concatenate(market + [status[:, None].astype(np.float64), env], axis=1)
    assert canon.shape[1] == sum(w for _, w in flat_oracle.reference_keys(raw_modified, P))
    split = np.zeros((N, 16))
    split[np.arange(N), status] = 1.0
    split[:, 6:14] = env
    split[:, 14] = sets * L_H + hours
    split[:, 15] = sets * L_D + days
    return series, canon, split, (sets, hours, days)


CASES = [(n_sets, rm, P) for n_sets in (1, 3) for rm in ("mod", "raw") for P in (1, 6, 13, 25)]


@pytest.mark.parametrize("n_sets,raw_modified,P", CASES)
def test_flat_rows_from_split_reproduces_the_flat_rows(n_sets, raw_modified, P):
    """Exact: the series and env values are float32-representable, so the float32 rows of flatten_rows and the float64 / float32
    rebuilds hold the same numbers.  NumPy and torch inputs, both dtypes.  And the comparison can fail: the series of another set
    (rolled by one set) or the hour and day indices swapped do not reproduce the rows."""
    import torch
    from rl_ptg_amd.policy_split import flat_rows_from_split
    series, canon, split, (sets, hours, days) = _case(n_sets, raw_modified, P, seed=100 * n_sets + P)
    for s in range(n_sets):                                      # the edges are really in the index set
        m = sets == s
        assert {0, L_H - P} <= set(hours[m].tolist()) and {0, L_D - 2} <= set(days[m].tolist())
    flat = flat_oracle.flatten_rows(canon, raw_modified, P)
    assert flat.dtype == np.float32 and flat.shape[1] == (2 * P + 14 if raw_modified == "mod" else P + 18)
    for dt in (np.float64, np.float32):
        ser = {k: v.astype(dt) for k, v in series.items()}
        rows = split.astype(dt)
        got = flat_rows_from_split(rows, ser, raw_modified, price_ahead=P)
        assert isinstance(got, np.ndarray) and got.dtype == dt and np.array_equal(got, flat.astype(dt))
        got_t = flat_rows_from_split(torch.from_numpy(rows), ser, raw_modified, price_ahead=P)
        assert torch.is_tensor(got_t) and got_t.dtype == torch.from_numpy(rows).dtype and np.array_equal(got_t.numpy(), flat.astype(dt))
        got_3d = flat_rows_from_split(rows.reshape(1, *rows.shape), ser, raw_modified, price_ahead=P)      # leading axes are kept
        assert np.array_equal(got_3d[0], flat.astype(dt))
    # can-fail 1: every set decoded with its neighbour's series
    if n_sets > 1:
        rolled = {k: np.roll(v, 1, axis=0) for k, v in series.items()}
        bad = flat_rows_from_split(split, rolled, raw_modified, price_ahead=P)
        assert not np.array_equal(bad, flat.astype(np.float64))
        assert (bad != flat).any(axis=1).all()                   # not one row survives the wrong set
    # can-fail 2: hour and day index swapped (rows whose swapped indices still lie inside the series)
    ok = (split[:, 14] + 2 <= n_sets * L_D) & (split[:, 15] + P <= n_sets * L_H) & (split[:, 14] != split[:, 15])
    assert ok.sum() >= 5
    swapped = split[ok].copy()
    swapped[:, [14, 15]] = swapped[:, [15, 14]]
    bad = flat_rows_from_split(swapped, series, raw_modified, price_ahead=P)
    assert (bad != flat[ok]).any(axis=1).all()


@pytest.mark.parametrize("n_sets,raw_modified,P", CASES)
def test_first_layer_split_equals_the_linear_layer_on_the_flat_rows(n_sets, raw_modified, P):
    """FirstLayerSplit.prepare(W, b)(rows) == flat @ W.T + b.

    float64: rtol = atol = 1e-12 (64 bits leave 4 decimal digits over the ~40 products).

    float32 series, rows and weights, against the float64 product of the same float32 numbers (exact to 1e-16): every output is
    a sum of `width` products and the bias, evaluated as a few partial dot products (env columns, hour table, day table) that are
    then added.  Whatever the order, a term goes through its product's rounding and at most `width` of the additions that join
    width + 1 terms, i.e. at most width + 1 roundings of relative size u = 2^-24 each:
        |y32 - y64| <= gamma_(width+1) * (|flat| @ |W|.T + |b|),   gamma_n = n u / (1 - n u) <= (n + 1) u  for n (n + 1) u <= 1,
    hence the bound (width + 2) * 2^-24 * (|flat| @ |W|.T + |b|) per output (width <= 64 here).  b = None drops the bias term."""
    import torch
    from rl_ptg_amd.policy_split import FirstLayerSplit
    series, canon, split, _ = _case(n_sets, raw_modified, P, seed=7 + 100 * n_sets + P)
    flat = flat_oracle.flatten_rows(canon, raw_modified, P).astype(np.float64)
    width, Hn = flat.shape[1], 24
    rng = np.random.default_rng(5 + P)
    W32 = rng.normal(size=(Hn, width)).astype(np.float32)
    b32 = rng.normal(size=Hn).astype(np.float32)
    W, b = W32.astype(np.float64), b32.astype(np.float64)
    worst64 = worst32 = 0.0
    for bias in (True, False):
        ref = flat @ W.T + (b if bias else 0.0)
        mag = np.abs(flat) @ np.abs(W).T + (np.abs(b) if bias else 0.0)
        # float64
        fl = FirstLayerSplit(series, raw_modified, price_ahead=P).prepare(torch.from_numpy(W), torch.from_numpy(b) if bias else None)
        y = fl(torch.from_numpy(split)).numpy()
        assert y.dtype == np.float64
        worst64 = max(worst64, float(np.abs(y - ref).max()))
        np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)
        # float32 against the derived bound
        ser32 = {k: v.astype(np.float32) for k, v in series.items()}
        fl = FirstLayerSplit(ser32, raw_modified, price_ahead=P).prepare(torch.from_numpy(W32), torch.from_numpy(b32) if bias else None)
        y = fl(torch.from_numpy(split.astype(np.float32))).numpy()
        assert y.dtype == np.float32
        bound = (width + 2) * U32 * mag
        worst32 = max(worst32, float((np.abs(y - ref) / bound).max()))
        assert np.all(np.abs(y - ref) <= bound), float((np.abs(y - ref) / bound).max())
    print(f"first layer n_sets={n_sets} {raw_modified} P={P}: float64 worst |err| {worst64:.2e}; float32 worst err / bound {worst32:.3f}")
    # a weight of another width is refused
    fl = FirstLayerSplit(series, raw_modified, price_ahead=P)
    for bad_width in (width - 1, width + 1):
        with pytest.raises(ValueError, match="input columns"):
            fl.prepare(torch.zeros((Hn, bad_width), dtype=torch.float64))
    if P != 13:                                                  # ... and so is the default-width weight at another price_ahead
        with pytest.raises(ValueError, match="input columns"):
            fl.prepare(torch.zeros((Hn, 40 if raw_modified == "mod" else 31), dtype=torch.float64))


def test_column_maps_of_consumer_and_oracle_agree():
    """flat_columns (the consumer's map) against the positions at which flatten_rows puts a marker per key"""
    from rl_ptg_amd.policy_split import SPLIT_ENV, env_columns, flat_columns
    for raw_modified in ("mod", "raw"):
        for P in (1, 6, 13, 25):
            keys = flat_oracle.reference_keys(raw_modified, P)
            cols, width = flat_columns(raw_modified, P)
            # canonical row whose every column holds the ordinal of its key (METH_STATUS: class 0 -> a one at its first column)
            canon = np.concatenate([np.full(w, 0.0 if k == "METH_STATUS" else 10.0 + j) for j, (k, w) in enumerate(keys)])[None]
            flat = flat_oracle.flatten_rows(canon, raw_modified, P)[0]
            assert flat.shape == (width,)
            for j, (k, w) in enumerate(keys):
                if k == "METH_STATUS":
                    assert flat[cols[k]] == 1.0 and np.all(flat[cols[k] + 1:cols[k] + 6] == 0.0)
                else:
                    assert np.all(flat[cols[k]:cols[k] + w] == 10.0 + j), (raw_modified, P, k)
            ec = env_columns(raw_modified, P)
            assert ec[:6] == list(range(cols["METH_STATUS"], cols["METH_STATUS"] + 6)) and ec[6:] == [cols[k] for k in SPLIT_ENV]
