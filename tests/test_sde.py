"""ptg_sde_resample / ptg_sde_act / ptg_sde_policy_loss, HipEngine.sde_*, rl_ptg_amd.SdeNoise and ppo_sde_loss / a2c_sde_loss
(include/ptg_env.h) -- gSDE's exploration matrix, its collecting head and its PPO / A2C loss -- against the NumPy restatement
(tests/sde_restatement.py, pinned against torch autograd over SB3's expressions by tests/test_sde_host.py).

Tolerances, derived and not measured.  The kernels compute in float64 and round once on the store, so against the float64 restatement
only the last-place differences between the device's and libm's exp / log / sqrt / cos and the order of the sums show:
  float32 outputs   within one float32 spacing of the restatement rounded to float32
  float64 outputs   within 1e-12 * max(1, |ref|); gradients of the loss within 1e-12 * max(1, |B * ref|) / B, as tests/test_policy_loss.py
  a sum of n terms  within S(n) = (n * 2^-53 + 1e-12) * max(1, mean |term|), on its own scale: the row sums V (n = L, terms h^2 s^2) and
                    noise (n = L, terms h E), the five means and the advantage moments (n = B), sum_i c_i h_ik^2 (n = B)
  E                 an additional absolute 1e-12 * s_k, for the cosine near its zeros
What lies behind a sum takes the sum's bound through its derivative, in addition to its own bound above.  With relV = S(L) / V:
  entropy, H          relV / 2
  log-prob (head)     |noise| * S(L) / V + relV * (noise^2 / (2 V) + 1 / 2);   raw and the action: S(L) of the noise
  log-prob lp (loss)  dlp = relV * (d^2 / (2 V) + 1 / 2);  the surrogate |g| * dlp;  approx_kl |r - 1| * dlp <= dlp (the cases keep
                      |log r| <= 0.5);  g itself (PPO: g = Ah * r) |g| * dlp
  d loss / d mu       |ref| * (relV + dlp [PPO])
  c_i                 dc = relV * (|g| * d^2 / V / (2 V) + |c|) + dlp [PPO] * |g| * |d^2 / V - 1| / (2 V)
  d loss / d h_ik     dc * 2 |h| s^2 / B;     d loss / d log_std[k]   (2 s^2 / B) * (S(B) of c_i h_ik^2 + sum_i dc_i * h_ik^2)
clip_fraction is exact: every case asserts that no ratio lies within 1e-9 of a clip edge.  Each test prints its measured maxima in
units of its tolerance.

Shapes: L in {1, 2, 63, 64, 65, 127, 129, 233, 1024} (one unit; lanes with and without a unit; the wave; one past it; lanes with one and
two units; 16 units a lane), N and B in {1, 3, 4, 5, 63, 65, 255, 256, 257, 513} (one wave of a block; a block's four; one past; the
moment kernel's 256-row blocks and one past), thinned diagonally by sde_restatement.grid() (31 of 90 pairs: every L with 5 and 257 rows,
every row count with L = 65, and the diagonal); 4 100 and 9 000 rows for more than one row a wave."""
import ctypes as C

import numpy as np
import pytest

import sde_restatement as sr

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


def _padded(x, pad, rows=0):
    """host [n, L] -> (view [n, L] of a SENTINEL-filled [n + 2 rows, L + pad] device tensor, that tensor)"""
    import torch
    n, L = x.shape
    wide = torch.full((n + 2 * rows, L + pad), SENTINEL, dtype=_tdt(x.dtype), device="cuda")
    view = wide[rows:rows + n, :L]
    view.copy_(_t(x))
    return view, wide


def _guard_ok(view, wide, rows=0):
    """the pad columns and guard rows of _padded's tensor still hold SENTINEL"""
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


# ------------------------------------------------------------------------------------------------- the matrix and the head
def _head_errs(res, ref, L):
    with np.errstate(all="ignore"):
        tn, relV = S(L, ref["abs_noise"]), S(L, ref["abs_V"]) / ref["V"]
        n2 = ref["noise"] * ref["noise"]
        return dict(act=_err(res.actions, ref["action"], tn), raw=_err(res.raw, ref["raw"], tn), ent=_err(res.entropy, ref["entropy"], relV / 2),
                    logp=_err(res.log_prob, ref["logp"], np.abs(ref["noise"]) * tn / ref["V"] + relV * (n2 / (2 * ref["V"]) + 0.5)))


def _resample_and_act(eng, n, L, dt, pad, counter, c_host, offset=0, clip=(-0.5, 0.5)):
    """one resample and two head calls (stochastic, deterministic) on the inputs of sr.head_case -> the worst errors"""
    import torch
    c = sr.head_case(n, L, dt)
    ls = _t(c["log_std"])
    E, Ew = _padded(np.zeros((n, L), dt), pad, rows=1)
    eng.sde_resample(ls, counter, E, seed=sr.SEED)
    eng.sync()
    r = sr.resample(c["log_std"], sr.SEED, c_host, n, offset)
    worst = dict(E=_err(E, r["E"], 1e-12 * r["s"][None, :]))
    assert _guard_ok(E, Ew, rows=1) and int(counter.item()) == c_host + 1
    lat, lw = _padded(c["latent"], pad)
    mean, mw = (_column(c["mean"]) if pad else (_t(c["mean"]), None))
    res = eng.sde_act(mean, lat, ls, E, clip=clip)
    eng.sync()
    E_host = E.cpu().numpy()                                 # the head is held to the matrix it was given
    ref = sr.act(c["mean"], c["latent"], c["log_std"], E_host, clip=clip)
    assert res.actions.dtype == torch.float32 and res.raw.dtype == _tdt(dt) and not ref["bad"].any()
    worst.update(_head_errs(res, ref, L))
    det = eng.sde_act(mean, lat, ls, None, clip=clip, deterministic=True, want_raw=False)
    eng.sync()
    dref = sr.act(c["mean"], c["latent"], c["log_std"], clip=clip, deterministic=True)
    assert det.raw is None
    worst["det"] = max(_err(det.actions, dref["action"]), _err(det.log_prob, dref["logp"], S(L, dref["abs_V"]) / dref["V"] / 2), _err(det.entropy, dref["entropy"], S(L, dref["abs_V"]) / dref["V"] / 2))
    assert _guard_ok(lat, lw) and (mw is None or bool((mw[:, 1] == SENTINEL).all()))
    return worst


@pytest.mark.parametrize("n,L", sr.grid())
def test_the_matrix_and_the_head_over_the_grid(n, L):
    """both dtypes; float32 contiguous, float64 with padded rows (latent and E with a row stride of L + 3, the means a column of an
    [N, 2] tensor) and sentinel guard rows around E; the deterministic mode without a matrix"""
    eng = _engine(n)
    counter = eng.new_draw_counter()
    worst = {}
    for k, dt in enumerate(sr.DTYPES):
        w = _resample_and_act(eng, n, L, dt, 3 * k, counter, k)
        worst.update({f"{key}{8 * dt().itemsize}": v for key, v in w.items()})
    assert max(worst.values()) <= 1.0, worst
    print(f"N={n} L={L}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


def test_more_than_one_row_a_wave_and_a_shard():
    """4 100 envs: two rows a wave in the head, five rows a block in resample; resample twice gives different matrices and an advanced
    counter; a shard of 100 envs at global offset 4 000 equals its slice of the big call, bit for bit"""
    import torch
    N, L = 4100, 65
    eng = _engine(N)
    counter = eng.new_draw_counter()
    w = _resample_and_act(eng, N, L, np.float32, 0, counter, 0)
    assert max(w.values()) <= 1.0, w
    ls = _t(sr.head_case(N, L, np.float32)["log_std"])
    a, b = torch.zeros(N, L, device="cuda"), torch.zeros(N, L, device="cuda")
    eng.sde_resample(ls, counter, a, seed=sr.SEED)
    eng.sde_resample(ls, counter, b, seed=sr.SEED)
    eng.sync()
    assert int(counter.item()) == 3 and not torch.equal(a, b) and float((a == b).float().mean()) < 1e-3
    shard = _engine(100, fresh=True)
    shard.set_global_env_offset(4000)
    cs = shard.new_draw_counter()
    cs.fill_(1)
    s = torch.zeros(100, L, device="cuda")
    shard.sde_resample(ls, cs, s, seed=sr.SEED)
    shard.sync()
    assert torch.equal(s.view(torch.int32), a[4000:].view(torch.int32))
    shard.close()
    print("4100 envs: max error / tolerance", {k: round(v, 4) for k, v in w.items()})


def test_the_kept_hidden_layer_of_a_device_mlp_is_read_in_place():
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, SdeNoise
    N, L = 65, 37                                            # rows of 37 floats padded to 40
    eng = _engine(N)
    torch.manual_seed(3)
    pi = nn.Sequential(nn.Linear(eng.obs_dim, L), nn.Tanh(), nn.Linear(L, 2)).cuda()
    policy = DeviceMLP(eng, pi, batch=N, hidden=True)
    eng.reset()
    out = policy(eng.obs)
    lat = policy.hidden[-1]
    assert lat.shape == (N, L) and lat.stride() == (40, 1)
    log_std = torch.full((L, 1), -1.25, device="cuda")
    noise = SdeNoise(eng, L, seed=11)
    noise.reset_noise(log_std)
    head = noise.act(out[:, 0], lat, log_std, clip=(-1.0, 1.0))
    eng.sync()
    ref = sr.act(out[:, 0].cpu().numpy(), lat.cpu().numpy(), log_std.cpu().numpy(), noise.matrix.cpu().numpy())
    w = _head_errs(head, ref, L)
    w["E"] = _err(noise.matrix, sr.resample(log_std.cpu().numpy(), 11, 0, N)["E"], 1e-12 * np.exp(-1.25))
    sd = noise.state_dict()
    assert sd["counter"] == 1 and sd["seed"] == 11 and torch.equal(sd["matrix"], noise.matrix.cpu())
    other = SdeNoise(eng, L, seed=0)
    other.load_state_dict(sd)
    other.reset_noise(log_std); noise.reset_noise(log_std)
    eng.sync()
    assert torch.equal(other.matrix, noise.matrix) and int(other.counter.item()) == 2 and not torch.equal(noise.matrix.cpu(), sd["matrix"])
    assert max(w.values()) <= 1.0, w
    print("DeviceMLP hidden layer: max error / tolerance", {k: round(v, 4) for k, v in w.items()})


# ------------------------------------------------------------------------------------------------- the loss
def _device_loss_case(c, pad, want_lat):
    import torch
    B, L = c["latent"].shape
    dt = _tdt(c["latent"].dtype)
    d = {k: _t(v) for k, v in c.items()}
    d["latent"], d["latent_wide"] = _padded(c["latent"], pad)
    full = lambda *s: torch.full(s, SENTINEL, dtype=dt, device="cuda")
    stats = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    if pad:                                                  # mean and value are columns of one [B, 2] output, and so are their gradients
        w = torch.stack([d["mean"], d["values"]], dim=1)
        d["mean"], d["values"] = w[:, 0], w[:, 1]
        guard = full(B + 2, 2)
        g_mu, g_val = guard[1:B + 1, 0], guard[1:B + 1, 1]
        d["guard"] = guard
    else:
        g_mu, g_val = full(B), full(B)
    g_lat = None
    if want_lat:
        g_lat, d["g_lat_wide"] = _padded(np.full((B, L), SENTINEL, c["latent"].dtype), pad, rows=1)
    d["out"] = (stats, g_mu, g_val, full(L), g_lat)
    return d


def _run(eng, kind, norm, cvf, d, ws=None):
    return eng.sde_policy_loss(kind, d["mean"], d["values"], d["latent"], d["log_std"], d["actions"], d["old_log_prob"] if kind == "ppo" else None,
                               d["advantages"], d["returns"], old_values=d["old_values"] if cvf is not None else None, out=d.get("out"), workspace=ws,
                               **sr.loss_kwargs(kind, norm, cvf))


def _ref(kind, norm, cvf, c):
    return sr.policy_loss(kind, c["mean"], c["values"], c["latent"], c["log_std"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
                          old_values=c["old_values"], **sr.loss_kwargs(kind, norm, cvf))


def _loss_errs(res, ref, c, kind):
    """the errors of one call in units of the tolerances the docstring derives"""
    h = c["latent"].astype(np.float64)
    B, L = h.shape
    ok = ~ref["bad"]
    with np.errstate(all="ignore"):
        s2 = np.exp(c["log_std"].astype(np.float64)) ** 2
        z = lambda a: np.where(ok, a, 0.0)
        relV = z(S(L, ref["abs_V"]) / ref["V"])
        dlp = relV * (0.5 * z(ref["d2V"]) + 0.5)
        gdep = dlp if kind == "ppo" else np.zeros(B)
        g, V, cc = np.abs(z(ref["g"])), np.where(ok, ref["V"], 1.0), np.abs(z(ref["c"]))
        dc = relV * (g * z(ref["d2V"]) / (2 * V) + cc) + gdep * g * np.abs(z(ref["d2V"]) - 1.0) / (2 * V)
        e = dict(g_mu=_err(res.grad_input, ref["grad_input"], np.abs(z(ref["grad_input"])) * (relV + gdep), per_batch=B),
                 g_val=_err(res.grad_values, ref["grad_values"], per_batch=B),
                 g_ls=_err(res.grad_log_std, ref["grad_log_std"], (2 * s2 / B) * (S(B, ref["abs_gls"]) + (dc[:, None] * h * h).sum(axis=0))))
        if res.grad_latent is not None:
            e["g_lat"] = _err(res.grad_latent, ref["grad_latent"], dc[:, None] * 2 * np.abs(h) * s2[None, :] / B, per_batch=B)
        got, want = res.stats.cpu().numpy(), ref["stats"]
        if ref["bad"].any():
            assert np.isnan(got[:6]).all()
            return e
        u, am = B * U53 + 1e-12, ref["abs_mean"]
        tol = {"policy_loss": u * max(1.0, am["policy_loss"]) + float((g * dlp).mean()), "value_loss": u * max(1.0, am["value_loss"]),
               "entropy_loss": u * max(1.0, am["entropy_loss"]) + float(relV.mean()) / 2, "approx_kl": u * max(1.0, am["approx_kl"]) + float(dlp.mean())}
        for i, k in ((1, "policy_loss"), (2, "value_loss"), (3, "entropy_loss"), (4, "approx_kl")):
            e[k] = abs(got[i] - want[i]) / tol[k]
        e["loss"] = abs(got[0] - want[0]) / (tol["policy_loss"] + abs(sr.ENT_COEF) * tol["entropy_loss"] + abs(sr.VF_COEF) * tol["value_loss"] + 4 * U53 * max(1.0, abs(want[0])))
        assert got[5] == want[5] and ref["margin"] > 1e-9, (got[5], want[5], ref["margin"])
        a64 = c["advantages"].astype(np.float64)
        e["adv_mean"] = abs(got[6] - want[6]) / (u * max(1.0, float(np.abs(a64).mean())))
        e["adv_std"] = abs(got[7] - want[7]) / (u * max(1.0, want[7]))
    return e


def _check_loss_case(eng, B, L, dt, pad, configs=sr.CONFIGS):
    worst = {}
    c = sr.loss_case(B, L, dt)
    for k, (kind, norm, cvf) in enumerate(configs):
        want_lat = k % 2 == 0
        d = _device_loss_case(c, pad, want_lat)
        res = _run(eng, kind, norm, cvf, d)
        eng.sync()
        assert (res.grad_latent is not None) == want_lat and res.grad_log_std.shape == (L,)
        for key, v in _loss_errs(res, _ref(kind, norm, cvf, c), c, kind).items():
            worst[key] = max(worst.get(key, 0.0), v)
        assert _guard_ok(d["latent"], d["latent_wide"])
        if pad:
            assert bool((d["guard"][0] == SENTINEL).all()) and bool((d["guard"][-1] == SENTINEL).all())
        if want_lat:
            assert _guard_ok(res.grad_latent, d["g_lat_wide"], rows=1)
    return worst


@pytest.mark.parametrize("B,L", sr.grid())
def test_both_losses_over_the_grid(B, L):
    """PPO and A2C x normalise x clip_range_vf (sr.CONFIGS), grad_latent present on every other configuration; float32 contiguous,
    float64 with the mean and the value as columns of one [B, 2] tensor (their gradients too, between sentinel rows), latent rows and
    latent gradients with a row stride of L + 3"""
    eng = _engine(64)
    worst = {}
    for k, dt in enumerate(sr.DTYPES):
        for key, v in _check_loss_case(eng, B, L, dt, 3 * k).items():
            worst[f"{key}{8 * dt().itemsize}"] = v
    assert max(worst.values()) <= 1.0, worst
    print(f"B={B} L={L}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("B,L", [(4100, 65), (9000, 358)])
def test_more_than_one_row_a_wave_in_the_loss(B, L):
    """two and three rows a wave (B above 4 096 and 8 192), 1 000 and more blocks: k_loss_final's threads walk four partials each"""
    eng = _engine(64)
    worst = _check_loss_case(eng, B, L, np.float32, 0, configs=sr.CONFIGS[:2])
    worst.update({k + "_64": v for k, v in _check_loss_case(eng, B, L, np.float64, 1, configs=sr.CONFIGS[4:5]).items()})
    assert max(worst.values()) <= 1.0, worst
    print(f"B={B} L={L}: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine(64)
    for B, L, dt in ((257, 129, np.float32), (4100, 65, np.float64)):
        c = sr.loss_case(B, L, dt)
        runs = []
        for _ in range(2):
            d = _device_loss_case(c, 0, True)
            res = _run(eng, "ppo", True, sr.CLIP_VF, d)
            eng.sync()
            runs.append([t.clone() for t in res])
        iv = torch.int32 if dt == np.float32 else torch.int64
        assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
        for a, b in zip(runs[0][1:], runs[1][1:]):
            assert torch.equal(a.view(iv), b.view(iv))


def test_bad_rows():
    """a planted NaN latent entry, an Inf mean, a non-finite sample: NaN gradients on those rows, the other rows' bits unchanged, NaN
    statistics and log_std gradient, PTG_E_NONFINITE once; a NaN and a +Inf log_std: every row.  The head and the matrix likewise."""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    B, L = 300, 65
    eng = _engine(B)

    def expect():
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == _lib.E_NONFINITE
        eng.sync()

    for dt in sr.DTYPES:
        iv = torch.int32 if dt == np.float32 else torch.int64
        c = sr.loss_case(B, L, dt)
        clean = _run(eng, "ppo", False, sr.CLIP_VF, _device_loss_case(c, 0, True))
        eng.sync()
        c["latent"][20, 64] = np.nan; c["mean"][277] = np.inf; c["actions"][100] = -np.inf; c["latent"][101, 0] = np.inf
        res = _run(eng, "ppo", False, sr.CLIP_VF, _device_loss_case(c, 0, True))
        expect()
        ref = _ref("ppo", False, sr.CLIP_VF, c)
        rows = [20, 100, 101, 277]
        assert np.nonzero(ref["bad"])[0].tolist() == rows
        keep = torch.from_numpy(~ref["bad"]).cuda()
        for got, was in ((res.grad_input, clean.grad_input), (res.grad_values, clean.grad_values), (res.grad_latent, clean.grad_latent)):
            assert torch.equal(got[keep].view(iv), was[keep].view(iv)) and bool(torch.isnan(got[~keep]).all())
        assert bool(torch.isnan(res.grad_log_std).all()) and bool(torch.isnan(res.stats[:6]).all())
        for bad_ls in (np.nan, np.inf):
            c = sr.loss_case(B, L, dt)
            c["log_std"][7] = bad_ls
            res = _run(eng, "a2c", False, None, _device_loss_case(c, 0, True))
            expect()
            assert bool(torch.isnan(res.grad_input).all()) and bool(torch.isnan(res.grad_values).all()) and bool(torch.isnan(res.grad_latent).all())
            assert bool(torch.isnan(res.grad_log_std).all())
        # the head: rows 3 (NaN latent) and 270 (-Inf mean); the matrix: a NaN and a +Inf column
        h = sr.head_case(B, L, dt)
        E = sr.resample(h["log_std"], 1, 0, B)["E"].astype(dt)
        good = eng.sde_act(_t(h["mean"]), _t(h["latent"]), _t(h["log_std"]), _t(E))
        eng.sync()
        good = [t.clone() for t in good]
        h["latent"][3, 5] = np.nan; h["mean"][270] = -np.inf
        res = eng.sde_act(_t(h["mean"]), _t(h["latent"]), _t(h["log_std"]), _t(E))
        expect()
        keep = torch.ones(B, dtype=torch.bool, device="cuda"); keep[[3, 270]] = False
        assert bool((res.actions[~keep] == 0).all()) and torch.equal(res.actions[keep], good[0][keep])
        for got, was in zip(res[1:], good[1:]):
            assert bool(torch.isnan(got[~keep]).all()) and torch.equal(got[keep].view(iv), was[keep].view(iv))
        h = sr.head_case(B, L, dt)
        cnt = eng.new_draw_counter()
        M0, M = torch.zeros(B, L, dtype=_tdt(dt), device="cuda"), torch.zeros(B, L, dtype=_tdt(dt), device="cuda")
        eng.sde_resample(_t(h["log_std"]), cnt, M0, seed=1)
        eng.sync()
        h["log_std"][2] = np.nan; h["log_std"][64] = np.inf
        cnt.zero_()
        eng.sde_resample(_t(h["log_std"]), cnt, M, seed=1)
        expect()
        ok = torch.ones(L, dtype=torch.bool, device="cuda"); ok[[2, 64]] = False
        assert bool(torch.isnan(M[:, ~ok]).all()) and torch.equal(M[:, ok].contiguous().view(iv), M0[:, ok].contiguous().view(iv))
        res = eng.sde_act(_t(h["mean"]), _t(h["latent"]), _t(h["log_std"]), _t(E))
        expect()
        assert bool((res.actions == 0).all()) and all(bool(torch.isnan(t).all()) for t in res[1:])
    eng.sync()


def test_on_a_side_stream():
    import torch
    eng = _engine(257)
    c = sr.loss_case(257, 65, np.float64)
    side = torch.cuda.Stream()
    counter = eng.new_draw_counter()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w = _resample_and_act(eng, 257, 65, np.float64, 3, counter, 0)
        d = _device_loss_case(c, 3, True)
        res = _run(eng, "ppo", True, None, d)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    w.update(_loss_errs(res, _ref("ppo", True, None, c), c, "ppo"))
    assert max(w.values()) <= 1.0, w


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they have
    returned, and torch's allocator hands out nothing in between.  Afterwards env state and vn statistics equal a twin's that made no call."""
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
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    c = sr.loss_case(n, L, np.float32)
    d = _device_loss_case(c, 0, True)
    ws = eng.sde_policy_loss_workspace(n, L)
    counter, E, head = eng.new_draw_counter(), torch.zeros(n, L, device="cuda"), eng.sde_act_outputs(torch.float32)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")

    def ops():
        eng.sde_resample(d["log_std"], counter, E, seed=3)
        eng.sde_act(d["mean"], d["latent"], d["log_std"], E, out=head)
        _run(eng, "ppo", True, sr.CLIP_VF, d, ws)

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
    ops()
    grown = torch.cuda.memory_allocated() - allocated
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    assert grown == 0, f"{grown} bytes allocated across the calls"
    eng.sync()
    res = _run(eng, "ppo", True, sr.CLIP_VF, d, ws)         # out= : the tensors the calls above wrote
    w = _loss_errs(res, _ref("ppo", True, sr.CLIP_VF, c), c, "ppo")
    ref = sr.act(c["mean"], c["latent"], c["log_std"], E.cpu().numpy())
    w.update(_head_errs(head, ref, L))
    w["E"] = _err(E, sr.resample(c["log_std"], 3, 1, n)["E"], 1e-12 * np.exp(c["log_std"].astype(np.float64))[None, :])
    assert max(w.values()) <= 1.0 and int(counter.item()) == 2, w
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    eng.close(); twin.close()
    print("65536 x 65: max error / tolerance", {k: round(v, 4) for k, v in w.items()})


# ------------------------------------------------------------------------------------------------- behind autograd, and captured
def test_loss_backward_fills_the_gradients_of_a_network_and_of_log_std():
    """TrainMLP obs -> 37 (tanh) -> [mean, value]; ppo_sde_loss on its output, its kept hidden layer as the latent (data: learn_features
    =False) and a log_std parameter; backward().  log_std.grad is the kernel's, held to the restatement; the network's gradients equal,
    bit for bit, tests/mlp_backward_restatement.py's pass over the gradients the kernel hands back for the same inputs.  Then with a
    latent that requires grad: its .grad is the kernel's grad_latent."""
    import torch
    from torch import nn
    import mlp_backward_restatement as mbr
    import mlp_restatement as mr
    from rl_ptg_amd import TrainMLP, a2c_sde_loss, ppo_sde_loss
    B, L = 203, 37
    eng = _engine(64)
    torch.manual_seed(9)
    pi = nn.Sequential(nn.Linear(24, L), nn.Tanh(), nn.Linear(L, 2)).cuda()
    net = TrainMLP(eng, pi, batch=B)
    rng = np.random.default_rng(2)
    x = _t(rng.standard_normal((B, 24)).astype(np.float32))
    log_std = nn.Parameter(torch.full((L, 1), -1.0, device="cuda"))
    out = net(x)
    lat = net.hidden[-1]
    c = sr.loss_case(B, L, np.float32)
    c.update(mean=out[:, 0].detach().cpu().numpy(), values=out[:, 1].detach().cpu().numpy(), latent=lat.cpu().numpy(), log_std=log_std.detach().cpu().numpy().reshape(-1))
    V, _ = sr.variance(c["latent"], c["log_std"])
    c["actions"] = (c["mean"] + np.sqrt(V) * rng.standard_normal(B)).astype(np.float32)
    c["old_log_prob"] = (sr.log_prob(c["mean"], c["latent"], c["log_std"], c["actions"]) - rng.uniform(-0.5, 0.5, B)).astype(np.float32)
    d = {k: _t(v) for k, v in c.items()}
    loss, stats = ppo_sde_loss(eng, out[:, 0], out[:, 1], lat, log_std, d["actions"], d["old_log_prob"], d["advantages"], d["returns"], clip_range=sr.CLIP,
                               clip_range_vf=sr.CLIP_VF, ent_coef=sr.ENT_COEF, vf_coef=sr.VF_COEF, old_values=d["old_values"])
    loss.backward()
    direct = eng.sde_policy_loss("ppo", out[:, 0].detach(), out[:, 1].detach(), lat, log_std.detach(), d["actions"], d["old_log_prob"], d["advantages"],
                                 d["returns"], old_values=d["old_values"], **sr.loss_kwargs("ppo", True, sr.CLIP_VF))
    eng.sync()
    ref = _ref("ppo", True, sr.CLIP_VF, c)
    w = _loss_errs(direct, ref, c, "ppo")
    assert max(w.values()) <= 1.0 and float(loss) == float(np.float32(stats[0].item())), w
    assert torch.equal(log_std.grad.reshape(-1), direct.grad_log_std) and direct.grad_latent is None
    gout = torch.stack([direct.grad_input, direct.grad_values], dim=1).cpu().numpy()
    ws_, bs_ = [m.weight.detach().cpu().numpy() for m in net.linears], [m.bias.detach().cpu().numpy() for m in net.linears]
    _, dws, dbs, _ = mbr.backward(gout, x.cpu().numpy(), ws_, [c["latent"]], out.detach().cpu().numpy(), hidden_act=mr.TANH, out_act=mr.NONE, want_dx=False)
    for l, m in enumerate(net.linears):
        assert mr.same_bits(m.weight.grad.cpu().numpy(), dws[l]) and mr.same_bits(m.bias.grad.cpu().numpy(), dbs[l]), l
    # learn_features=True: the latent as a leaf that requires grad
    leaf = lat.clone().requires_grad_(True)
    ls2 = log_std.detach().clone().requires_grad_(True)
    loss, _ = a2c_sde_loss(eng, out[:, 0].detach(), out[:, 1].detach(), leaf, ls2, d["actions"], d["advantages"], d["returns"], ent_coef=sr.ENT_COEF, vf_coef=sr.VF_COEF)
    (2.0 * loss).backward()
    eng.sync()
    direct2 = eng.sde_policy_loss("a2c", out[:, 0].detach(), out[:, 1].detach(), lat, log_std.detach(), d["actions"], None, d["advantages"], d["returns"],
                                  want_grad_latent=True, **sr.loss_kwargs("a2c", False, None))
    eng.sync()
    w2 = {k + "_a2c": v for k, v in _loss_errs(direct2, _ref("a2c", False, None, c), c, "a2c").items()}
    assert max(w2.values()) <= 1.0, w2
    assert torch.equal(leaf.grad, 2.0 * direct2.grad_latent) and torch.equal(ls2.grad.reshape(-1), 2.0 * direct2.grad_log_std)
    print("backward: max error / tolerance", {k: round(v, 4) for k, v in {**w, **w2}.items()})


def test_a_captured_collect_step_replayed_three_times():
    """DeviceMLP(hidden=True) obs -> 37 (tanh) -> [mean, value] -> SdeNoise.act -> replay-proof step -> DeviceRolloutBuffer.add at 64 envs,
    captured on a side stream at the default hardware-queue setting.  One eager step, then three replays, reset_noise (not captured)
    between the second and the third.  After every step the stored raw sample and log-prob and the env's action are held to the
    restatement on that step's network output, kept hidden layer and matrix; the matrix to the restatement of its counter value."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP, DeviceRolloutBuffer, SdeNoise
    N, L, T, SEED = 64, 37, 4, 21
    eng = _engine(N, fresh=True)
    eng.set_replay_proof(True)
    eng.reset()
    torch.manual_seed(5)
    pi = nn.Sequential(nn.Linear(eng.obs_dim, L), nn.Tanh(), nn.Linear(L, 2)).cuda()
    policy = DeviceMLP(eng, pi, batch=N, hidden=True)
    log_std = torch.full((L,), -0.5, device="cuda")
    ls_host = log_std.cpu().numpy()
    noise = SdeNoise(eng, L, seed=SEED)
    noise.reset_noise(log_std)
    buf = DeviceRolloutBuffer(eng, T, columns={"actions": torch.float32, "values": torch.float32, "log_probs": torch.float32})
    env_actions = []

    def one():
        out = policy(eng.obs)
        head = noise.act(out[:, 0], policy.hidden[-1], log_std)
        eng.step(head.actions)
        buf.add(eng.obs, eng.rew, eng.done, actions=head.raw, values=out[:, 1], log_probs=head.log_prob)
        return out, head

    worst = {}

    def check(t, counter_value):
        """row t of the buffer against the restatement on what the step's network call left"""
        eng.sync()
        assert buf.cursor() == (t + 1, 0) and int(noise.counter.item()) == counter_value + 1
        E = noise.matrix.cpu().numpy()
        w = dict(E=_err(noise.matrix, sr.resample(ls_host, SEED, counter_value, N)["E"], 1e-12 * np.exp(ls_host.astype(np.float64))[None, :]))
        ref = sr.act(out[:, 0].cpu().numpy(), policy.hidden[-1].cpu().numpy(), ls_host, E)
        got = type(head)(head.actions, buf.actions[t], buf.log_probs[t], head.entropy)
        w.update(_head_errs(got, ref, L))
        assert torch.equal(buf.values[t], out[:, 1]) and torch.equal(buf.storage.obs_rows[t + 1], eng.obs)
        env_actions.append(head.actions.clone())
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)

    buf.begin()
    out, head = one()                                       # eager once: code objects are loaded before the capture
    check(0, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert buf.cursor() == (1, 0)                           # capturing enqueued nothing
    for k in (1, 2, 3):
        if k == 3:
            noise.reset_noise(log_std)
        graph.replay()
        torch.cuda.synchronize()
        check(k, 1 if k == 3 else 0)
    eng.note_replays(2)                                     # three replays; the capture call counted as one step on the host
    assert not torch.equal(env_actions[1], env_actions[2]) and max(worst.values()) <= 1.0, worst
    eng.sync()
    eng.close()
    print("captured collect step: max error / tolerance", {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    N, L = 300, 65
    eng = _engine(N)
    lib, h, stream = eng._L, eng._h, eng._stream()
    c = sr.loss_case(N, L, np.float32)
    d = _device_loss_case(c, 3, True)
    stats, g_mu, g_val, g_ls, g_lat = d["out"]
    ws = eng.sde_policy_loss_workspace(N, L)
    ws.fill_(0x5A)
    E, Ew = _padded(np.full((N, L), SENTINEL, np.float32), 3, rows=1)
    cnt = eng.new_draw_counter()
    acts = torch.full((N,), SENTINEL, device="cuda")
    outs = [torch.full((N,), SENTINEL, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()

    def noise(**kw):
        return _lib.PtgSdeNoise(**{**dict(in_dtype=_lib.OUT_F32, latent_dim=L, log_std_dev=p(d["log_std"]), seed=1, counter_dev=p(cnt), e_dev=p(E), e_s_n=L + 3), **kw})

    def head(**kw):
        a = dict(flags=0, in_dtype=_lib.OUT_F32, latent_dim=L, act_kind=_lib.ACT_F32, mean_dev=p(d["mean"]), mean_s_n=2, latent_dev=p(d["latent"]), latent_s_n=L + 3,
                 e_dev=p(E), e_s_n=L + 3, log_std_dev=p(d["log_std"]), clip_lo=-1.0, clip_hi=1.0, act_dev=p(acts), raw_dev=p(outs[0]), logp_dev=p(outs[1]), ent_dev=p(outs[2]))
        return _lib.PtgSdeHead(**{**a, **kw})

    def loss(**kw):
        a = dict(kind=_lib.LOSS_PPO, flags=_lib.LOSS_NORM_ADV | _lib.LOSS_CLIP_VF, in_dtype=_lib.OUT_F32, latent_dim=L, batch=N, mean_dev=p(d["mean"]), mean_s_n=2,
                 val_dev=p(d["values"]), val_s_n=2, latent_dev=p(d["latent"]), latent_s_n=L + 3, log_std_dev=p(d["log_std"]), act_dev=p(d["actions"]),
                 old_logp_dev=p(d["old_log_prob"]), adv_dev=p(d["advantages"]), ret_dev=p(d["returns"]), old_val_dev=p(d["old_values"]), clip_range=0.2,
                 clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.5, stats_dev=p(stats), grad_in_dev=p(g_mu), g_s_n=2, grad_val_dev=p(g_val), gv_s_n=2,
                 grad_log_std_dev=p(g_ls), grad_latent_dev=p(g_lat), gl_s_n=L + 3, ws_dev=p(ws))
        return _lib.PtgSdeLoss(**{**a, **kw})

    nan = float("nan")
    bad = [(lib.ptg_sde_resample, b"ptg_sde_resample", x) for x in (
               noise(log_std_dev=None), noise(counter_dev=None), noise(e_dev=None), noise(in_dtype=2), noise(in_dtype=-1), noise(latent_dim=0), noise(latent_dim=1025),
               noise(e_s_n=L - 1), noise(e_s_n=0))]
    bad += [(lib.ptg_sde_act, b"ptg_sde_act", x) for x in (
                head(mean_dev=None), head(latent_dev=None), head(log_std_dev=None), head(act_dev=None), head(e_dev=None), head(flags=2), head(flags=4), head(in_dtype=2),
                head(latent_dim=0), head(latent_dim=1025), head(act_kind=_lib.ACT_I32), head(mean_s_n=0), head(latent_s_n=L - 1), head(e_s_n=L - 1),
                head(clip_lo=1.0, clip_hi=-1.0), head(clip_lo=nan))]
    bad += [(lib.ptg_sde_policy_loss, b"ptg_sde_policy_loss", x) for x in (
                loss(mean_dev=None), loss(val_dev=None), loss(latent_dev=None), loss(log_std_dev=None), loss(act_dev=None), loss(old_logp_dev=None), loss(adv_dev=None),
                loss(ret_dev=None), loss(stats_dev=None), loss(grad_in_dev=None), loss(grad_val_dev=None), loss(grad_log_std_dev=None), loss(ws_dev=None),
                loss(ws_dev=p(ws) + 4), loss(kind=2), loss(kind=-1), loss(flags=4), loss(batch=0), loss(batch=-3), loss(batch=2 ** 31 + 1), loss(in_dtype=2),
                loss(latent_dim=0), loss(latent_dim=1025), loss(mean_s_n=0), loss(g_s_n=0), loss(val_s_n=0), loss(gv_s_n=-1), loss(latent_s_n=L - 1), loss(gl_s_n=L - 1),
                loss(old_val_dev=None), loss(clip_range=nan), loss(clip_range=-0.1), loss(clip_range_vf=nan), loss(clip_range_vf=-1.0))]
    for k, (fn, name, ds) in enumerate(bad):
        assert fn(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert name in lib.ptg_last_error(h), k
        assert torch.cuda.current_stream().query() is True, k
    for fn, ds in ((lib.ptg_sde_resample, noise()), (lib.ptg_sde_act, head()), (lib.ptg_sde_policy_loss, loss())):
        assert fn(h, None, stream) == _lib.E_INVALID and fn(None, C.byref(ds), stream) == _lib.E_INVALID
    assert lib.ptg_sde_policy_loss_workspace(0, L) < 0 and lib.ptg_sde_policy_loss_workspace(N, 0) < 0 and lib.ptg_sde_policy_loss_workspace(N, 1025) < 0
    assert torch.cuda.current_stream().query() is True
    untouched = [stats, d["guard"], g_ls, d["g_lat_wide"], Ew, acts] + outs
    assert all(bool((t == SENTINEL).all()) for t in untouched) and bool((ws == 0x5A).all()) and int(cnt.item()) == 0
    good = [(lib.ptg_sde_resample, noise()), (lib.ptg_sde_act, head()), (lib.ptg_sde_act, head(flags=_lib.HEAD_DETERMINISTIC, e_dev=None, e_s_n=0, raw_dev=None)),
            (lib.ptg_sde_policy_loss, loss()), (lib.ptg_sde_policy_loss, loss(kind=_lib.LOSS_A2C, old_logp_dev=None, clip_range=nan)),
            (lib.ptg_sde_policy_loss, loss(flags=0, old_val_dev=None, clip_range_vf=nan, grad_latent_dev=None, gl_s_n=0)), (lib.ptg_sde_policy_loss, loss(batch=1))]
    for k, (fn, ds) in enumerate(good):
        assert fn(h, C.byref(ds), stream) == 0, (k, lib.ptg_last_error(h))
    eng.sync()
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(g_ls).all()) and int(cnt.item()) == 1 and _guard_ok(E, Ew, rows=1)
