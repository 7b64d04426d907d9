"""ptg_sde_resample_rows / ptg_sde_rsample / ptg_sde_rsample_backward, HipEngine.sde_resample_rows / sde_rsample / sde_rsample_backward,
rl_ptg_amd.SquashedSdeNoise and sde_squashed_rsample (include/ptg_env.h) -- gSDE's squashed head for SAC / TQC, its reparametrised sample
and the backward -- against the NumPy restatement (tests/sde_squash_restatement.py, pinned against torch autograd over SB3's expressions
by tests/test_sde_squash_host.py).

Tolerances, derived and not measured, by tests/test_sde.py's rules.  The kernels compute in float64 and round once on the store, and the
restatement adds in the kernels' own order, so against it only the last places of exp / log / sqrt / tanh / cos from two libraries show:
  float32 outputs   within one float32 spacing of the restatement rounded to float32
  float64 outputs   within 1e-12 * max(1, |ref|); the backward's gradients within 1e-12 * max(1, |B * ref|) / B (the incoming gradients
                    of the cases are of the order 1 / B, as a mean's are)
  a sum of n terms  within S(n) = (n * 2^-53 + 1e-12) * max(1, mean |term|): V (n = L, terms h^2 s^2), noise (n = L, terms h E), the
                    log_std gradient (n = B, terms h_ik * grad_latent_ik)
  E (resample_rows) an additional absolute 1e-12 * s_k, for the cosine near its zeros (tests/test_sde.py)
What lies behind a sum takes the sum's bound through its derivative, in addition to its own bound above.  With tn = S(L) of the noise,
relV = S(L) of V over V, d = 1 - a^2 and q = 2 a d / (d + 1e-6), tanh and the log correction as tests/test_actor.py has them (the
library functions' own last places are inside the float32 spacing / the 1e-12):
  action a = tanh(m + noise)      d * tn  (d a / d noise = d <= 1)
  log-prob                        (|noise| / V + |q|) * tn + relV * (noise^2 / (2 V) + 1 / 2)
  saved (noise, V)                tn, S(L) of V
The backward is FED THE OP'S OWN saved (noise, V), as tests/test_actor.py feeds ptg_rsample_backward the op's own noise, so that the
forward's sums are not counted a second time: the mean and latent gradients then carry their own bound only, and
  d loss / d log_std[k]           S(B) of its terms + sum_i |h_ik| * (the latent gradient's own bound)
Each test prints its measured maxima in units of its tolerance.

Shapes: tests/test_sde.py's -- L in {1, 2, 63, 64, 65, 127, 129, 233, 1024}, B in {1, 3, 4, 5, 63, 65, 255, 256, 257, 513}, thinned by
sde_restatement.grid() (every L with 5 and 257 rows, every B with L = 65, the diagonal); 4 100 and 9 000 rows for two and three rows a
wave and more than 1 000 blocks."""
import ctypes as C

import numpy as np
import pytest

import sde_restatement as sr
import sde_squash_restatement as sq

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
U53 = 2.0 ** -53
_specs = {}
_engines = {}


def _engine(n, fresh=False, eps_len_d=1):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if not fresh and n in _engines:
        return _engines[n]
    if eps_len_d not in _specs:
        _specs[eps_len_d] = synthetic_spec(scenario=2, operation="OP2", eps_len_d=eps_len_d, train_steps=200000, action_type="continuous")[0]
    s = _specs[eps_len_d]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[n] = eng
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _iv(dt):
    import torch
    return torch.int32 if np.dtype(dt) == np.float32 else torch.int64


def _padded(x, pad, rows=0):
    """host [n, L] -> (view [n, L] of a SENTINEL-filled [n + 2 rows, L + pad] device tensor, that tensor)"""
    import torch
    n, L = x.shape
    wide = torch.full((n + 2 * rows, L + pad), SENTINEL, dtype=_tdt(x.dtype), device="cuda")
    view = wide[rows:rows + n, :L]
    view.copy_(_t(x))
    return view, wide


def _guard_ok(view, wide, rows=0):
    n, L = view.shape
    ok = bool((wide[:, L:] == SENTINEL).all())
    return ok and (rows == 0 or (bool((wide[:rows] == SENTINEL).all()) and bool((wide[rows + n:] == SENTINEL).all())))


def _column(x):
    """host [n] -> column 0 of a [n, 2] device tensor (stride 2), column 1 SENTINEL"""
    import torch
    w = torch.full((x.shape[0], 2), SENTINEL, dtype=_tdt(x.dtype), device="cuda")
    w[:, 0] = _t(x)
    return w[:, 0], w


def S(n, abs_sum):
    """the bound of a sum of n terms with sum |term| = abs_sum"""
    return (n * U53 + 1e-12) * np.maximum(1.0, np.asarray(abs_sum, np.float64) / n)


def _err(got, ref64, extra=0.0, per_batch=None):
    """max error in units of the tolerance (<= 1 passes); NaN must meet NaN.  per_batch: B, for the gradients' float64 bound"""
    got = got.detach().cpu().numpy()
    ref64 = np.asarray(ref64, np.float64).reshape(got.shape)
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), (np.nonzero(np.isnan(got) != nan))
    if nan.all():
        return 0.0
    extra = np.broadcast_to(np.asarray(extra, np.float64), got.shape)
    if got.dtype == np.float32:
        ref = ref64.astype(np.float32)
        tol = np.spacing(np.abs(ref)).astype(np.float64) + extra
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    else:
        tol = (1e-12 * np.maximum(1.0, np.abs(ref64)) if per_batch is None else 1e-12 * np.maximum(1.0, np.abs(per_batch * ref64)) / per_batch) + extra
        d = np.abs(got - ref64)
    return float((d[~nan] / tol[~nan]).max())


def _own(ref, B, f32):
    """the own bound of a gradient entry, as _err applies it: for sum_i |h| * that bound in the log_std gradient"""
    ref = np.nan_to_num(np.asarray(ref, np.float64))
    return np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64) if f32 else 1e-12 * np.maximum(1.0, np.abs(B * ref)) / B


# ------------------------------------------------------------------------------------------------- one forward and one backward
def _fwd_errs(res, ref, L):
    with np.errstate(all="ignore"):
        ok = ~ref["bad"]
        z = lambda a: np.where(ok, a, 0.0)
        tn, dV = z(S(L, ref["abs_noise"])), z(S(L, ref["abs_V"]))
        V = np.where(ok, ref["V"], 1.0)
        relV, n = dV / V, z(ref["noise"])
        e = dict(act=_err(res.actions, ref["act"], z(ref["d"]) * tn))
        if res.step_actions is not None:
            e["step"] = _err(res.step_actions, ref["step_act"], z(ref["d"]) * tn)
        if res.log_prob is not None:
            e["logp"] = _err(res.log_prob, ref["logp"], (np.abs(n) / V + np.abs(z(ref["q"]))) * tn + relV * (n * n / (2 * V) + 0.5))
        if res.saved is not None:
            sv = res.saved.cpu().numpy()
            fin = np.isfinite(ref["saved"]).all(axis=1)
            e["saved"] = float(max((np.abs(sv[fin, 0] - ref["saved"][fin, 0]) / (1e-12 * np.maximum(1.0, np.abs(ref["saved"][fin, 0])) + tn[fin])).max(initial=0.0),
                                   (np.abs(sv[fin, 1] - ref["saved"][fin, 1]) / (1e-12 * np.maximum(1.0, np.abs(ref["saved"][fin, 1])) + dV[fin])).max(initial=0.0)))
    return e


def _bwd_errs(g, ref, latent, B):
    h = np.abs(np.nan_to_num(latent.astype(np.float64)))
    f32 = g.grad_mean.dtype.itemsize == 4
    e = dict(g_mu=_err(g.grad_mean, ref["grad_mean"], per_batch=B))
    if g.grad_latent is not None:
        e["g_lat"] = _err(g.grad_latent, ref["grad_latent"], per_batch=B)
    if g.grad_log_std is not None:
        L = h.shape[1]
        extra = S(B, ref["abs_gls"]) + (h * _own(ref["grad_latent"], B, f32)).sum(axis=0) if not ref["bad"].any() else np.zeros(L)
        e["g_ls"] = _err(g.grad_log_std, ref["grad_log_std"], extra, per_batch=B)
    return e


def _device_case(c, pad, shared, want_lat=True, want_ls=True):
    """the device tensors of a case: contiguous (pad 0), or the mean as a column of [B, 2], latent / E / the latent gradient in rows of
    L + pad between sentinel columns (E and the gradient between sentinel rows too), the mean gradient a column of a guarded [B + 2, 2]"""
    import torch
    B, L = c["latent"].shape
    dt = _tdt(c["latent"].dtype)
    d = dict(log_std=_t(c["log_std"]), grad_act=_t(c["grad_act"]), grad_logp=_t(c["grad_logp"]))
    d["latent"], d["latent_wide"] = _padded(c["latent"], pad)
    d["mean"], d["mean_wide"] = _column(c["mean"]) if pad else (_t(c["mean"]), None)
    if shared:
        d["E"], d["E_wide"], d["E_host"] = _t(c["row"]), None, c["row"]
    else:
        d["E"], d["E_wide"] = _padded(c["matrix"], pad, rows=1)
        d["E_host"] = c["matrix"]
    full = lambda *s: torch.full(s, SENTINEL, dtype=dt, device="cuda")
    if pad:
        d["gm_wide"] = full(B + 2, 2)
        gm = d["gm_wide"][1:B + 1, 0]
    else:
        d["gm_wide"], gm = None, full(B)
    g_lat, d["g_lat_wide"] = _padded(np.full((B, L), SENTINEL, c["latent"].dtype), pad, rows=1) if want_lat else (None, None)
    d["out_b"] = (gm, g_lat, full(L) if want_ls and shared else None)
    return d


def _guards(d):
    ok = _guard_ok(d["latent"], d["latent_wide"])
    if d["mean_wide"] is not None:
        ok = ok and bool((d["mean_wide"][:, 1] == SENTINEL).all()) and bool((d["gm_wide"][0] == SENTINEL).all()) and bool((d["gm_wide"][-1] == SENTINEL).all()) \
            and bool((d["gm_wide"][:, 1] == SENTINEL).all())
    if d["E_wide"] is not None:
        ok = ok and _guard_ok(d["E"], d["E_wide"], rows=1)
    if d["g_lat_wide"] is not None:
        ok = ok and _guard_ok(d["out_b"][1], d["g_lat_wide"], rows=1)
    return ok


def _ok(tag, worst):
    """print the measured maxima in units of their tolerances, then hold them to 1"""
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print(f"{tag}: max error / tolerance", {k: round(v, 4) for k, v in top})
    assert top[0][1] <= 1.0, dict(top)


def _run(eng, c, pad, shared, clip_mean=sq.CLIP_MEAN, want_lat=True, ga=True, gl=True, g_max=sq.G_MAX):
    """forward, then backward on the op's own saved pairs -> (errors in units of the tolerances, forward result, backward result, refs);
    g_max: the range the case must keep |g| in (None: a case that leaves it on purpose)"""
    B, L = c["latent"].shape
    d = _device_case(c, pad, shared, want_lat)
    f = eng.sde_rsample(d["mean"], d["latent"], d["log_std"], d["E"], clip_mean=clip_mean, want_step_actions=True)
    g = eng.sde_rsample_backward(d["mean"], d["latent"], d["log_std"], d["E"], f.saved, d["grad_act"] if ga else None, d["grad_logp"] if gl else None,
                                 clip_mean=clip_mean, out=d["out_b"])
    eng.sync()
    rf = sq.forward(c["mean"], c["latent"], c["log_std"], d["E_host"], clip_mean=clip_mean)
    rb = sq.backward(c["mean"], c["latent"], c["log_std"], d["E_host"], f.saved.cpu().numpy(), c["grad_act"] if ga else None, c["grad_logp"] if gl else None,
                     clip_mean=clip_mean)
    assert g_max is None or np.abs(np.where(rf["bad"], 0.0, rf["g"])).max() < g_max, np.abs(rf["g"]).max()
    e = _fwd_errs(f, rf, L)
    e.update(_bwd_errs(g, rb, c["latent"], B))
    assert _guards(d) and (g.grad_log_std is not None) == shared and (g.grad_latent is not None) == want_lat
    return e, f, g, rf, rb


@pytest.mark.parametrize("B,L", sq.grid())
def test_forward_and_backward_over_the_grid(B, L):
    """both dtypes x the shared row and the per-row matrix; float32 contiguous, float64 strided (the mean a column of [B, 2], latent, E and
    the latent gradient in padded rows between sentinels); the latent gradient left out on the float64 shared call; the deterministic
    forward without a matrix"""
    import torch
    eng = _engine(64)
    worst = {}
    for k, dt in enumerate(sq.DTYPES):
        c = sq.case(B, L, dt)
        for shared in (True, False):
            e, f, g, rf, _ = _run(eng, c, 3 * k, shared, want_lat=not (k == 1 and shared))
            assert f.actions.dtype == _tdt(dt) and f.step_actions.dtype == torch.float32 and not rf["bad"].any()
            worst.update({f"{key}{8 * dt().itemsize}{'s' if shared else 'm'}": v for key, v in e.items()})
        det = eng.sde_rsample(_t(c["mean"]), _t(c["latent"]), _t(c["log_std"]), None, deterministic=True, want_saved=False)
        eng.sync()
        worst.update({f"det_{key}{8 * dt().itemsize}": v for key, v in _fwd_errs(det, sq.forward(c["mean"], c["latent"], c["log_std"], deterministic=True), L).items()})
        assert det.saved is None and det.step_actions is None
    _ok(f"B={B} L={L}", worst)


@pytest.mark.parametrize("B,L", [(4100, 65), (9000, 233)])
def test_more_than_one_row_a_wave_and_more_than_one_block(B, L):
    eng = _engine(64)
    worst = {}
    for dt, pad, shared in ((np.float32, 0, True), (np.float64, 1, True), (np.float32, 0, False)):
        e, *_ = _run(eng, sq.case(B, L, dt), pad, shared)
        worst.update({f"{k}{8 * dt().itemsize}{'s' if shared else 'm'}": v for k, v in e.items()})
    _ok(f"B={B} L={L}", worst)


def test_the_trunk_output_of_a_train_mlp_is_read_in_place():
    """the latent is the OUTPUT of a TrainMLP trunk ending in its activation: [B, 37] float32, contiguous in the net's own buffer"""
    import torch
    from torch import nn
    from rl_ptg_amd import TrainMLP
    B, L = 65, 37
    eng = _engine(64)
    torch.manual_seed(3)
    trunk = TrainMLP(eng, nn.Sequential(nn.Linear(24, 48), nn.ReLU(), nn.Linear(48, L), nn.ReLU()).cuda(), batch=B)
    x = _t(np.random.default_rng(1).standard_normal((B, 24)).astype(np.float32))
    lat = trunk(x).detach()
    c = sq.case(B, L, np.float32)
    f = eng.sde_rsample(_t(c["mean"]), lat, _t(c["log_std"]), _t(c["row"]))
    eng.sync()
    w = _fwd_errs(f, sq.forward(c["mean"], lat.cpu().numpy(), c["log_std"], c["row"]), L)
    assert max(w.values()) <= 1.0 and float((lat == 0).float().mean()) > 0.1, w       # ReLU's zeros are part of the case


def test_clip_mean_at_and_around_its_ends_and_switched_off():
    import torch
    B, L = 70, 65
    eng = _engine(64)
    for dt in sq.DTYPES:
        c = sq.case(B, L, dt)
        two = dt(2.0)
        edge = [two, -two, np.nextafter(two, dt(0)), np.nextafter(two, dt(3)), np.nextafter(-two, dt(0)), np.nextafter(-two, dt(-3)), dt(2.5), dt(-7.0)]
        c["mean"][:8] = edge
        e, f, g, rf, rb = _run(eng, c, 0, True)
        assert max(e.values()) <= 1.0, e
        gm = g.grad_mean.cpu().numpy()
        assert (gm[[0, 1, 3, 5, 6, 7]] == 0).all() and (gm[[2, 4]] != 0).all() and (gm[8:] != 0).sum() == (np.abs(c["mean"][8:]) < 2).sum()
        assert np.array_equal(rf["m"][:8], [2, -2, edge[2], 2, edge[4], -2, 2, -2])
        # +Inf: the unclipped lines -- the forward is the clipped call's on means that lie inside, bit for bit, and every row has a gradient
        c["mean"][7] = -3.0                                  # unclipped, |g| must still stay below G_MAX
        e2, f2, g2, rf2, _ = _run(eng, c, 0, True, clip_mean=float("inf"))
        assert max(e2.values()) <= 1.0 and np.array_equal(rf2["m"], c["mean"].astype(np.float64)), e2
        inside = torch.from_numpy(np.abs(c["mean"]) < 2).cuda()
        assert torch.equal(f2.actions[inside].view(_iv(dt)), f.actions[inside].view(_iv(dt))) and bool((g2.grad_mean != 0).all())
        assert not torch.equal(f2.actions[~inside], f.actions[~inside])


def test_an_exactly_saturated_row_is_legal():
    """|g| = 25 and 40: tanh is +-1 exactly in float64, d = 0, q = 0; the log-prob is finite (log(1e-6) in the correction) and the
    gradients are the lines' values: 0 for the mean, the -gl * noise / V and variance paths for the latent and log_std"""
    import torch
    B, L = 9, 65
    eng = _engine(64)
    for dt in sq.DTYPES:
        c = sq.case(B, L, dt)
        c["mean"][2], c["mean"][5] = 25.0, -40.0
        e, f, g, rf, rb = _run(eng, c, 0, True, clip_mean=float("inf"), g_max=None)
        assert max(e.values()) <= 1.0, e
        a = f.actions.cpu().numpy()
        assert a[2] == 1.0 and a[5] == -1.0 and rf["d"][2] == 0.0 and rf["q"][5] == 0.0 and np.isfinite(f.log_prob.cpu().numpy()).all()
        assert g.grad_mean[2].item() == 0.0 and g.grad_mean[5].item() == 0.0 and bool(torch.isfinite(g.grad_latent).all()) and bool((g.grad_latent[2] != 0).any())
        assert bool(torch.isfinite(g.grad_log_std).all())
    eng.sync()


def test_bad_rows():
    """a NaN latent entry, an Inf mean, a NaN incoming gradient: NaN outputs on those rows and in every entry of the log_std gradient, the
    other rows' bits unchanged, PTG_E_NONFINITE once; a NaN and a +Inf log_std: every row"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    B, L = 300, 65
    eng = _engine(64)

    def expect():
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == _lib.E_NONFINITE
        eng.sync()

    def both(c, saved=None):
        d = _device_case(c, 0, True)
        f = eng.sde_rsample(d["mean"], d["latent"], d["log_std"], d["E"], want_step_actions=True)
        g = eng.sde_rsample_backward(d["mean"], d["latent"], d["log_std"], d["E"], f.saved if saved is None else saved, d["grad_act"], d["grad_logp"], out=d["out_b"])
        return f, g

    for dt in sq.DTYPES:
        iv = _iv(dt)
        c = sq.case(B, L, dt)
        f0, g0 = both(c)
        eng.sync()
        c["latent"][20, 64] = np.nan; c["mean"][277] = np.inf; c["latent"][101, 0] = -np.inf
        f, g = both(c)
        expect()
        rows = [20, 101, 277]
        assert np.nonzero(sq.forward(c["mean"], c["latent"], c["log_std"], c["row"])["bad"])[0].tolist() == rows
        keep = torch.ones(B, dtype=torch.bool, device="cuda"); keep[rows] = False
        for got, was in ((f.actions, f0.actions), (f.log_prob, f0.log_prob), (g.grad_mean, g0.grad_mean), (g.grad_latent, g0.grad_latent)):
            assert torch.equal(got[keep].view(iv), was[keep].view(iv)) and bool(torch.isnan(got[~keep]).all())
        assert torch.equal(f.step_actions[keep], f0.step_actions[keep]) and bool((f.step_actions[~keep] == 0).all())
        assert bool(torch.isnan(g.grad_log_std).all())
        # a NaN incoming gradient: the backward alone, on the clean forward's saved pairs
        c = sq.case(B, L, dt)
        c["grad_act"][7] = np.nan
        d = _device_case(c, 0, True)
        g = eng.sde_rsample_backward(d["mean"], d["latent"], d["log_std"], d["E"], f0.saved, d["grad_act"], d["grad_logp"], out=d["out_b"])
        expect()
        keep = torch.ones(B, dtype=torch.bool, device="cuda"); keep[7] = False
        for got, was in ((g.grad_mean, g0.grad_mean), (g.grad_latent, g0.grad_latent)):
            assert torch.equal(got[keep].view(iv), was[keep].view(iv)) and bool(torch.isnan(got[~keep]).all())
        assert bool(torch.isnan(g.grad_log_std).all())
        for bad_ls in (np.nan, np.inf):
            c = sq.case(B, L, dt)
            c["log_std"][7] = bad_ls
            d = _device_case(c, 0, True)
            f = eng.sde_rsample(d["mean"], d["latent"], d["log_std"], d["E"], want_step_actions=True)
            expect()
            assert bool(torch.isnan(f.actions).all()) and bool(torch.isnan(f.log_prob).all()) and bool((f.step_actions == 0).all())
            g = eng.sde_rsample_backward(d["mean"], d["latent"], d["log_std"], d["E"], f0.saved, d["grad_act"], d["grad_logp"], out=d["out_b"])
            expect()
            assert bool(torch.isnan(g.grad_mean).all()) and bool(torch.isnan(g.grad_latent).all()) and bool(torch.isnan(g.grad_log_std).all())
        # the training row: a NaN and a +Inf column, the others as they were
        c = sq.case(B, L, dt)
        cnt = eng.new_draw_counter()
        r0, r1 = torch.zeros(L, dtype=_tdt(dt), device="cuda"), torch.zeros(L, dtype=_tdt(dt), device="cuda")
        eng.sde_resample_rows(_t(c["log_std"]), cnt, r0, seed=1)
        eng.sync()
        c["log_std"][2] = np.nan; c["log_std"][64] = np.inf
        cnt.zero_()
        eng.sde_resample_rows(_t(c["log_std"]), cnt, r1, seed=1)
        expect()
        ok = torch.ones(L, dtype=torch.bool, device="cuda"); ok[[2, 64]] = False
        assert bool(torch.isnan(r1[~ok]).all()) and torch.equal(r1[ok].view(iv), r0[ok].view(iv))
    eng.sync()


def test_null_outputs_and_null_incoming_gradients():
    """grad_latent_dev = NULL leaves grad_log_std and grad_mean bit-identical; each incoming gradient alone is NULL (= 0)"""
    import torch
    B, L = 257, 129
    eng = _engine(64)
    for dt in sq.DTYPES:
        iv = _iv(dt)
        c = sq.case(B, L, dt)
        e, f, g, _, _ = _run(eng, c, 0, True)
        e2, f2, g2, _, _ = _run(eng, c, 0, True, want_lat=False)
        assert max(e.values()) <= 1.0 and max(e2.values()) <= 1.0 and g2.grad_latent is None
        assert torch.equal(g2.grad_log_std.view(iv), g.grad_log_std.view(iv)) and torch.equal(g2.grad_mean.view(iv), g.grad_mean.view(iv))
        for ga, gl in ((True, False), (False, True)):
            e3, *_ = _run(eng, c, 0, True, ga=ga, gl=gl)
            assert max(e3.values()) <= 1.0, (ga, gl, e3)


def test_the_two_noise_streams_of_a_squashed_sde_noise():
    """two reset_train_noise calls differ and advance only the training counter; the row is the restatement's under the derived seed and
    no row of the collecting matrix; the collecting matrix of a shard at global offset 4 000 still equals its slice of a 4 100-env
    engine's (ptg_sde_resample is unchanged); state_dict / load_state_dict carry both counters and both matrices"""
    import torch
    from rl_ptg_amd import SquashedSdeNoise
    N, L, SEED = 4100, 65, 77
    eng = _engine(N)
    ls_host = sq.case(4, L, np.float32)["log_std"]
    ls = _t(ls_host)
    noise = SquashedSdeNoise(eng, L, seed=SEED)
    noise.reset_train_noise(ls)
    eng.sync()
    a = noise.train_row.clone()
    noise.reset_train_noise(ls)
    eng.sync()
    b = noise.train_row.clone()
    assert int(noise.train_counter.item()) == 2 and int(noise.counter.item()) == 0 and not torch.equal(a, b) and bool((noise.matrix == 0).all())
    s = np.exp(ls_host.astype(np.float64))
    for k, row in enumerate((a, b)):
        assert _err(row, sq.resample_rows(ls_host, SEED ^ sq.TRAIN_SEED_XOR, k, 1)["E"][0], 1e-12 * s) <= 1.0
    noise.reset_noise(ls)
    eng.sync()
    assert int(noise.train_counter.item()) == 2 and int(noise.counter.item()) == 1 and torch.equal(noise.train_row, b)
    assert _err(noise.matrix, sr.resample(ls_host, SEED, 0, N)["E"], 1e-12 * s[None, :]) <= 1.0
    assert not bool((noise.matrix == a[None, :]).all(dim=1).any())
    shard = _engine(100, fresh=True)
    shard.set_global_env_offset(4000)
    sn = SquashedSdeNoise(shard, L, seed=SEED)
    sn.reset_noise(ls)
    sn.reset_train_noise(ls)
    shard.sync()
    assert torch.equal(sn.matrix.view(torch.int32), noise.matrix[4000:].view(torch.int32))
    assert torch.equal(sn.train_row.view(torch.int32), a.view(torch.int32))            # a batch row: no env offset
    sd = noise.state_dict()
    assert (sd["counter"], sd["train_counter"], sd["seed"]) == (1, 2, SEED) and torch.equal(sd["train_row"], b.cpu())
    other = SquashedSdeNoise(eng, L, seed=0)
    other.load_state_dict(sd)
    other.reset_train_noise(ls); noise.reset_train_noise(ls); other.reset_noise(ls); noise.reset_noise(ls)
    eng.sync()
    assert torch.equal(other.train_row, noise.train_row) and torch.equal(other.matrix, noise.matrix) and int(other.train_counter.item()) == 3
    shard.close()
    # rows: a [3, L] matrix with padded rows through sde_resample_rows
    m, mw = _padded(np.zeros((3, L), np.float32), 3, rows=1)
    cnt = eng.new_draw_counter()
    eng.sde_resample_rows(ls, cnt, m, seed=5)
    eng.sync()
    assert _err(m, sq.resample_rows(ls_host, 5, 0, 3)["E"], 1e-12 * s[None, :]) <= 1.0 and _guard_ok(m, mw, rows=1) and int(cnt.item()) == 1


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine(64)
    for B, L, dt in ((257, 129, np.float32), (4100, 65, np.float64)):
        c = sq.case(B, L, dt)
        runs = []
        for _ in range(2):
            _, f, g, _, _ = _run(eng, c, 0, True)
            runs.append([t.clone() for t in (f.actions, f.log_prob, g.grad_mean, g.grad_latent, g.grad_log_std)] + [f.saved.clone()])
        for a, b in zip(runs[0][:-1], runs[1][:-1]):
            assert torch.equal(a.view(_iv(dt)), b.view(_iv(dt)))
        assert torch.equal(runs[0][-1].view(torch.int64), runs[1][-1].view(torch.int64))


def test_on_a_side_stream():
    import torch
    eng = _engine(64)
    c = sq.case(257, 65, np.float64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e, *_ = _run(eng, c, 3, True)
        e2, *_ = _run(eng, c, 3, False)
    torch.cuda.current_stream().wait_stream(side)
    assert max(e.values()) <= 1.0 and max(e2.values()) <= 1.0, (e, e2)


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing (tests/test_sde.py's): the stream is busy with milliseconds of fused steps before the calls and still
    busy when they have returned, and torch's allocator hands out nothing in between.  Afterwards the engine's state equals a twin's."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls, L = 65536, 250, 8, 65
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    engs = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(5)
        e.vn_init()
        e.reset()
        engs.append(e)
    eng, twin = engs
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=gen)
    c = sq.case(n, L, np.float32)
    d = _device_case(c, 0, True)
    ws = eng.sde_rsample_backward_workspace(n, L)
    counter, row = eng.new_draw_counter(), torch.zeros(L, device="cuda")
    fo = (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros((n, 2), dtype=torch.float64, device="cuda"))
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")

    def ops():
        eng.sde_resample_rows(d["log_std"], counter, row, seed=3)
        f = eng.sde_rsample(d["mean"], d["latent"], d["log_std"], row, out=fo)
        return f, eng.sde_rsample_backward(d["mean"], d["latent"], d["log_std"], row, f.saved, d["grad_act"], d["grad_logp"], out=d["out_b"], workspace=ws)

    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    ops()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocated = torch.cuda.memory_allocated()
    f, g = ops()
    grown = torch.cuda.memory_allocated() - allocated
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    assert grown == 0, f"{grown} bytes allocated across the calls"
    eng.sync()
    E = row.cpu().numpy()
    w = _fwd_errs(f, sq.forward(c["mean"], c["latent"], c["log_std"], E), L)
    w.update(_bwd_errs(g, sq.backward(c["mean"], c["latent"], c["log_std"], E, f.saved.cpu().numpy(), c["grad_act"], c["grad_logp"]), c["latent"], n))
    w["E"] = _err(row, sq.resample_rows(c["log_std"], 3, 1, 1)["E"][0], 1e-12 * np.exp(c["log_std"].astype(np.float64)))
    assert max(w.values()) <= 1.0 and int(counter.item()) == 2, w
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    eng.close(); twin.close()
    print("65536 x 65: max error / tolerance", {k: round(v, 4) for k, v in w.items()})


# ------------------------------------------------------------------------------------------------- behind autograd, and captured
def test_one_sac_gradient_step_end_to_end():
    """TrainMLP trunk 24 -> 48 -> 65 (ReLU, ReLU as out_activation) -> a one-layer mu -> sde_squashed_rsample -> two TrainMLPGroup critics
    on (obs, action) -> sac_actor_loss -> backward(), B = 64, L = 65.  log_std.grad is the kernel's; mu's and the trunk's gradients equal,
    bit for bit, tests/mlp_backward_restatement.py's passes over the gradients the kernel hands back.  The no-grad call (the target's
    pass) with the same row gives the same bits and keeps nothing."""
    import torch
    from torch import nn
    import mlp_backward_restatement as mbr
    import mlp_restatement as mr
    from rl_ptg_amd import SquashedSdeNoise, TrainMLP, TrainMLPGroup, sac_actor_loss, sde_squashed_rsample
    B, L, F = 64, 65, 24
    eng = _engine(64)
    torch.manual_seed(9)
    trunk_m = nn.Sequential(nn.Linear(F, 48), nn.ReLU(), nn.Linear(48, L), nn.ReLU()).cuda()
    mu_m = nn.Sequential(nn.Linear(L, 1)).cuda()
    qfs = [nn.Sequential(nn.Linear(F + 1, 32), nn.ReLU(), nn.Linear(32, 1)).cuda() for _ in range(2)]
    trunk, mu, critics = TrainMLP(eng, trunk_m, batch=B), TrainMLP(eng, mu_m, batch=B), TrainMLPGroup(eng, qfs, batch=B)
    with torch.no_grad():
        mu_m[0].weight.mul_(12.0)                             # means on both sides of clip_mean
    x = _t(np.random.default_rng(2).standard_normal((B, F)).astype(np.float32))
    log_std = nn.Parameter(torch.full((L, 1), -2.5, device="cuda"))
    noise = SquashedSdeNoise(eng, L, seed=5)
    noise.reset_train_noise(log_std.detach())
    latent = trunk(x)
    mean = mu(latent)
    actions, log_prob = sde_squashed_rsample(noise, mean, latent, log_std)
    assert actions.shape == (B, 1) and log_prob.shape == (B, 1) and actions.grad_fn is not None
    q0, q1 = critics(x, x2=actions)
    loss, stats = sac_actor_loss(eng, [q0, q1], log_prob, ent_coef=sq.ENT_COEF)
    actions.retain_grad(); log_prob.retain_grad(); mean.retain_grad(); latent.retain_grad()
    loss.backward()
    eng.sync()
    lat_h, mean_h, ls_h, row_h = latent.detach().cpu().numpy(), mean.detach().cpu().numpy()[:, 0], log_std.detach().cpu().numpy()[:, 0], noise.train_row.cpu().numpy()
    assert (np.abs(mean_h) > 2).any() and (np.abs(mean_h) < 2).any()
    f = eng.sde_rsample(mean.detach(), latent.detach(), log_std.detach(), noise.train_row)
    g = eng.sde_rsample_backward(mean.detach(), latent.detach(), log_std.detach(), noise.train_row, f.saved, actions.grad.contiguous(), log_prob.grad.contiguous())
    eng.sync()
    assert torch.equal(f.actions, actions.detach()[:, 0]) and torch.equal(f.log_prob, log_prob.detach()[:, 0])
    rf = sq.forward(mean_h, lat_h, ls_h, row_h)
    assert np.abs(rf["g"]).max() < sq.G_MAX
    w = _fwd_errs(f, rf, L)
    rb = sq.backward(mean_h, lat_h, ls_h, row_h, f.saved.cpu().numpy(), actions.grad.cpu().numpy(), log_prob.grad.cpu().numpy())
    w.update(_bwd_errs(g, rb, lat_h, B))
    assert max(w.values()) <= 1.0, w
    assert torch.equal(log_std.grad[:, 0], g.grad_log_std) and torch.equal(mean.grad[:, 0], g.grad_mean)
    # mu: one Linear, its output gradient is the kernel's grad_mean
    gm = g.grad_mean.cpu().numpy().reshape(B, 1)
    wm, w_t = [m.weight.detach().cpu().numpy() for m in mu.linears], [m.weight.detach().cpu().numpy() for m in trunk.linears]
    dx, dws, dbs, _ = mbr.backward(gm, lat_h, wm, [], mean.detach().cpu().numpy(), hidden_act=mr.RELU, out_act=mr.NONE, want_dx=True)
    assert mr.same_bits(mu.linears[0].weight.grad.cpu().numpy(), dws[0]) and mr.same_bits(mu.linears[0].bias.grad.cpu().numpy(), dbs[0])
    # the trunk's output gradient: autograd's float32 sum of mu's dx and the kernel's grad_latent
    g_lat = latent.grad.cpu().numpy()
    assert mr.same_bits(g_lat, dx + g.grad_latent.cpu().numpy())
    hidden = [trunk.hidden[0].cpu().numpy()]
    _, dws, dbs, _ = mbr.backward(g_lat, x.cpu().numpy(), w_t, hidden, lat_h, hidden_act=mr.RELU, out_act=mr.RELU, want_dx=False)
    for l, m in enumerate(trunk.linears):
        assert mr.same_bits(m.weight.grad.cpu().numpy(), dws[l]) and mr.same_bits(m.bias.grad.cpu().numpy(), dbs[l]), l
    with torch.no_grad():
        a2, lp2 = sde_squashed_rsample(noise, mean.detach(), latent.detach(), log_std)
    assert a2.grad_fn is None and torch.equal(a2, actions.detach()) and torch.equal(lp2, log_prob.detach())
    print("SAC step: max error / tolerance", {k: round(v, 4) for k, v in w.items()})


def test_a_captured_collect_step_replayed_three_times():
    """DeviceMLP trunk obs -> 37 (ReLU as out_activation), DeviceMLP mu 37 -> 1 -> SquashedSdeNoise.act -> replay-proof step ->
    DeviceReplayBuffer.add at 64 envs, captured on a side stream.  One eager step, then three replays, reset_noise (not captured)
    between the second and the third.  After every step the env's action and the stored action are held to the restatement on that
    step's network outputs and matrix; the matrix to the restatement of its counter value."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, DeviceReplayBuffer, SquashedSdeNoise
    N, L, SEED = 64, 37, 21
    eng = _engine(N, fresh=True)
    eng.set_replay_proof(True)
    torch.manual_seed(5)
    trunk = DeviceMLP(eng, nn.Sequential(nn.Linear(eng.obs_dim, L), nn.ReLU()).cuda(), batch=N)
    mu = DeviceMLP(eng, nn.Sequential(nn.Linear(L, 1)).cuda(), batch=N)
    log_std = torch.full((L,), -2.0, device="cuda")
    ls_host = log_std.cpu().numpy()
    noise = SquashedSdeNoise(eng, L, seed=SEED)
    noise.reset_noise(log_std)
    buf = DeviceReplayBuffer(eng, 8 * N, columns={"actions": torch.float32}, seed=5)
    prev = eng.reset().clone()
    obs, rew, done, fin = eng.alloc_obs(zero=True), torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), eng.alloc_obs(zero=True)
    keep = {}

    def one():
        lat = trunk(prev)
        mean = mu(lat)
        head = noise.act(mean, lat, log_std)
        eng.step(head.step_actions, obs, rew, done, final_obs=fin)
        buf.add(prev, obs, rew, done, final_obs=fin, actions=head.actions)
        keep.update(lat=lat, mean=mean, head=head)
        prev.copy_(obs)

    worst, env_actions = {}, []

    def check(t, counter_value, obs_before):
        eng.sync()
        lat, mean, head = keep["lat"], keep["mean"], keep["head"]
        assert buf.cursor()[0] == t + 1 and int(noise.counter.item()) == counter_value + 1 and int(noise.train_counter.item()) == 0
        w = dict(E=_err(noise.matrix, sr.resample(ls_host, SEED, counter_value, N)["E"], 1e-12 * np.exp(ls_host.astype(np.float64))[None, :]))
        ref = sq.forward(mean.cpu().numpy()[:, 0], lat.cpu().numpy(), ls_host, noise.matrix.cpu().numpy())
        w.update(_fwd_errs(head, ref, L))
        assert head.log_prob is None and head.saved is None and torch.equal(buf.column("actions")[t], head.actions) and torch.equal(head.step_actions, head.actions)
        assert torch.equal(buf.observations[t], obs_before) and torch.equal(prev, obs)
        env_actions.append(head.actions.clone())
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)

    before = prev.clone()
    one()                                                   # eager once: code objects are loaded before the capture
    check(0, 0, before)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert buf.cursor()[0] == 1                              # capturing enqueued nothing
    for k in (1, 2, 3):
        if k == 3:
            noise.reset_noise(log_std)
        before = prev.clone()
        graph.replay()
        torch.cuda.synchronize()
        check(k, 1 if k == 3 else 0, before)
    eng.note_replays(2)                                     # three replays; the capture call counted as one step on the host
    assert not torch.equal(env_actions[1], env_actions[2]) and max(worst.values()) <= 1.0, worst
    eng.sync()
    eng.close()
    print("captured collect step: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    B, L = 300, 65
    eng = _engine(64)
    lib, h, stream = eng._L, eng._h, eng._stream()
    c = sq.case(B, L, np.float32)
    d = _device_case(c, 3, False)
    gm, g_lat, _ = d["out_b"]
    full = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device="cuda")
    row, g_ls, act, sact, lp, saved = _t(c["row"]), full(L), full(B), full(B), full(B), full(B, 2, dt=torch.float64)
    ws = eng.sde_rsample_backward_workspace(B, L)
    ws.fill_(0x5A)
    rows_m, rows_w = _padded(np.full((3, L), SENTINEL, np.float32), 3, rows=1)
    cnt = eng.new_draw_counter()
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    SH = _lib.SDE_RS_SHARED_E

    def rs(**kw):
        a = dict(flags=0, in_dtype=_lib.OUT_F32, latent_dim=L, batch=B, mean_dev=p(d["mean"]), mean_s_n=2, latent_dev=p(d["latent"]), latent_s_n=L + 3,
                 e_dev=p(d["E"]), e_s_n=L + 3, log_std_dev=p(d["log_std"]), clip_mean=2.0, act_dev=p(act), step_act_dev=p(sact), logp_dev=p(lp), saved_dev=p(saved),
                 grad_act_dev=p(d["grad_act"]), grad_logp_dev=p(d["grad_logp"]), grad_mean_dev=p(gm), gm_s_n=2, grad_latent_dev=p(g_lat), gl_s_n=L + 3,
                 grad_log_std_dev=None, ws_dev=p(ws))
        return _lib.PtgSdeRs(**{**a, **kw})

    def nz(**kw):
        return _lib.PtgSdeNoise(**{**dict(in_dtype=_lib.OUT_F32, latent_dim=L, log_std_dev=p(d["log_std"]), seed=1, counter_dev=p(cnt), e_dev=p(rows_m), e_s_n=L + 3), **kw})

    nan, inf = float("nan"), float("inf")
    common = [rs(mean_dev=None), rs(latent_dev=None), rs(log_std_dev=None), rs(e_dev=None), rs(flags=4), rs(flags=8), rs(in_dtype=2), rs(in_dtype=-1), rs(latent_dim=0),
              rs(latent_dim=1025), rs(batch=0), rs(batch=-3), rs(batch=2 ** 31 + 1), rs(mean_s_n=0), rs(latent_s_n=L - 1), rs(e_s_n=L - 1), rs(e_s_n=0), rs(clip_mean=0.0),
              rs(clip_mean=-2.0), rs(clip_mean=nan), rs(clip_mean=-inf), rs(saved_dev=p(saved) + 4)]
    bad = [(lib.ptg_sde_rsample, b"ptg_sde_rsample:", x) for x in common + [rs(act_dev=None)]]
    bad += [(lib.ptg_sde_rsample_backward, b"ptg_sde_rsample_backward:", x) for x in common + [
        rs(saved_dev=None), rs(grad_mean_dev=None), rs(ws_dev=None), rs(ws_dev=p(ws) + 4), rs(grad_act_dev=None, grad_logp_dev=None), rs(gm_s_n=0), rs(gl_s_n=L - 1),
        rs(grad_log_std_dev=p(g_ls)), rs(flags=_lib.SDE_RS_DETERMINISTIC, grad_log_std_dev=p(g_ls))]]
    for k, (fn, name, ds) in enumerate(bad):
        assert fn(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert name in lib.ptg_last_error(h), (k, lib.ptg_last_error(h))
        assert torch.cuda.current_stream().query() is True, k
    bad_n = [(nz(log_std_dev=None), 3), (nz(counter_dev=None), 3), (nz(e_dev=None), 3), (nz(in_dtype=2), 3), (nz(latent_dim=0), 3), (nz(latent_dim=1025), 3),
             (nz(e_s_n=L - 1), 3), (nz(), 0), (nz(), -1), (nz(), 2 ** 31 + 1)]
    for k, (ds, rows) in enumerate(bad_n):
        assert lib.ptg_sde_resample_rows(h, C.byref(ds), rows, stream) == _lib.E_INVALID and b"ptg_sde_resample_rows:" in lib.ptg_last_error(h), k
    assert lib.ptg_sde_resample_rows(h, None, 1, stream) == _lib.E_INVALID and lib.ptg_sde_resample_rows(None, C.byref(nz()), 1, stream) == _lib.E_INVALID
    for fn in (lib.ptg_sde_rsample, lib.ptg_sde_rsample_backward):
        assert fn(h, None, stream) == _lib.E_INVALID and fn(None, C.byref(rs()), stream) == _lib.E_INVALID
    W = lib.ptg_sde_rsample_backward_workspace
    assert W(0, L) < 0 and W(B, 0) < 0 and W(B, 1025) < 0
    assert torch.cuda.current_stream().query() is True
    untouched = [act, sact, lp, saved, g_ls, d["gm_wide"], d["g_lat_wide"], rows_w]
    assert all(bool((t == SENTINEL).all()) for t in untouched) and bool((ws == 0x5A).all()) and int(cnt.item()) == 0
    good = [(lib.ptg_sde_rsample, rs()), (lib.ptg_sde_rsample_backward, rs()),
            (lib.ptg_sde_rsample, rs(flags=SH, e_dev=p(row), e_s_n=0, clip_mean=inf, step_act_dev=None, logp_dev=None)),
            (lib.ptg_sde_rsample_backward, rs(flags=SH, e_dev=p(row), e_s_n=0, grad_log_std_dev=p(g_ls), grad_act_dev=None, grad_latent_dev=None, gl_s_n=0)),
            (lib.ptg_sde_rsample, rs(flags=_lib.SDE_RS_DETERMINISTIC, e_dev=None, e_s_n=0, saved_dev=None)), (lib.ptg_sde_rsample, rs(batch=1))]
    for k, (fn, ds) in enumerate(good):
        assert fn(h, C.byref(ds), stream) == 0, (k, lib.ptg_last_error(h))
    assert lib.ptg_sde_resample_rows(h, C.byref(nz()), 3, stream) == 0
    eng.sync()
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(g_ls).all()) and int(cnt.item()) == 1 and _guard_ok(rows_m, rows_w, rows=1) and _guards(d)
