"""ptg_rsample / ptg_rsample_backward / ptg_actor_loss, HipEngine.rsample / rsample_backward / smooth_target_action / actor_loss and
rl_ptg_amd.loss's squashed_rsample / sac_actor_loss / tqc_actor_loss / td3_actor_loss / ent_coef_loss (include/ptg_env.h) against the
NumPy restatement (tests/actor_restatement.py, pinned against torch autograd by tests/test_actor_host.py).

Bounds, derived and not measured.
  bit for bit, through integer views (no transcendental, no cross-lane sum): d loss / d q and d loss / d quantile; d loss / d log_prob
    (with a log alpha on the device the restatement is fed the alpha the kernel reports in stats[4], itself held to np.exp within 2
    float64 spacings: section 15's basis); the SMOOTH action given the noise; the noise itself between calls that draw the same
    (seed, counter, row) -- float32 and float64 calls, SQUASH and SMOOTH, and ptg_act's raw sample at mean 0, log_std 0 (0 + 1 * z)
  the noise against the restatement's z: 1e-12 * max(1, |z|) -- log, sqrt and cos come from two libraries (the cosine
    near its zeros).  So that this difference is not counted a second time, actions, log-probs and the backward's gradients are compared
    with the restatement FED THE OP'S OWN NOISE
  actions, log-probs, the backward's gradients (exp, tanh, log): float32 within one float32 spacing of the rounded restatement; float64
    within 1e-12 * max(1, |ref|) + 1e-12 * sigma
  every mean: (B * 2^-53 + 1e-12) * max(1, mean |term|); the entropy-coefficient loss is log alpha times such a mean
Each test prints its measured maxima in units of its bound.

The grid is thinned diagonally as tests/test_quantile_loss.py's is: at every B the six (K, Q) pairs are all run, and dtype, layout
(contiguous / stride 2 or row stride Q + 1 with guard columns and guard rows), alpha form (host, device, device log) and the nullable parts
(grad_log_prob, the entropy-coefficient part) walk diagonally over them, shifted by B's position; at B = 290 and B = 470 dtype x layout is
run in full for every (K, Q) with the alpha forms cycling, so every value of every axis appears there."""
import ctypes as C

import numpy as np
import pytest

import act_restatement as ar
import actor_restatement as at

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
ALPHA, LOG_ALPHA = 0.2173, -1.3125
ALPHA_FORMS = ["host", "dev", "log"]
_engines = {}
_spec = []
_worst = {"exp_spacings": 0.0, "noise": 0.0}


def _engine(n=64, fresh=False):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if not fresh and n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])      # 139-step episodes
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[n] = eng
    return eng


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _full(shape, dt):
    import torch
    return torch.full(shape, SENTINEL, dtype=dt, device="cuda")


def _h(t):
    return t.detach().cpu().numpy()


def _same_bits(got, ref64):
    """an output against the restatement rounded once to the output's dtype, through integer views; a NaN must meet a NaN"""
    got = _h(got)
    ref = np.asarray(ref64, np.float64).reshape(got.shape).astype(got.dtype)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    iv = np.int32 if got.dtype == np.float32 else np.int64
    assert np.array_equal(got[~nan].view(iv), ref[~nan].view(iv)), float(np.abs(got[~nan].astype(np.float64) - ref[~nan]).max())


def _float_err(got, ref64, sigma):
    """max error of a float output in units of its bound: one float32 spacing of the rounded restatement, or 1e-12 * max(1, |ref|) +
    1e-12 * sigma"""
    got = _h(got).reshape(-1)
    ref = np.asarray(ref64, np.float64).reshape(-1)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    if got.dtype == np.float32:
        r32 = ref.astype(np.float32)
        return float((np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)).max())
    return float((np.abs(got - ref) / (1e-12 * np.maximum(1.0, np.abs(ref)) + 1e-12 * sigma)).max())


def _noise_err(noise, seed, c):
    z = at.draw(seed, c, noise.shape[0])
    e = float((np.abs(noise - z) / (1e-12 * np.maximum(1.0, np.abs(z)))).max())
    _worst["noise"] = max(_worst["noise"], e)
    return e


def _strided(x, stride2):
    """a host array [B] as a device tensor: contiguous, or column 0 of a [B, 2] tensor whose column 1 is a guard"""
    if not stride2:
        return _t(x), None
    w = _full((x.shape[0], 2), _t(x[:1]).dtype)
    w[:, 0] = _t(x)
    return w[:, 0], w


def _guarded(B, dt, stride2):
    """an output [B]: rows 1 .. B of a [B + 2] tensor (guard rows), or of column 0 of a [B + 2, 2] tensor (guard rows and a guard column)"""
    g = _full((B + 2, 2) if stride2 else (B + 2,), dt)
    return (g[1:B + 1, 0] if stride2 else g[1:B + 1]), g


def _guards_intact(g, B, stride2):
    ok = bool((g[0] == SENTINEL).all()) and bool((g[B + 1] == SENTINEL).all())
    return ok and (not stride2 or bool((g[:, 1] == SENTINEL).all()))


# ------------------------------------------------------------------------------------------------- rsample, its backward, the smoothed action
def _check_rsample(eng, B, dt, stride2, c, parts):
    """one forward and one backward at counter value c; parts: which nullable parts are present (logp, noise-less second call, ga, gl)"""
    import torch
    z_host = at.draw(at.SEED, c, B)
    mean, ls = at.rs_case(B, dt, z_host)
    ga, gl = at.grads_case(B, dt)
    m_d, m_w = _strided(mean, stride2)
    l_d, l_w = _strided(ls, stride2)
    tdt = m_d.dtype
    counter = torch.full((1,), c, dtype=torch.int64, device="cuda")
    act, act_g = _guarded(B, tdt, False)
    logp, logp_g = _guarded(B, tdt, False)
    noise, noise_g = _guarded(B, torch.float64, False)
    res = eng.rsample(m_d, l_d, counter, seed=at.SEED, out=(act, logp if parts["logp"] else None, noise))
    eng.sync()
    assert int(counter) == c + 1 and res.actions is act and (res.log_prob is None) == (not parts["logp"])
    z = _h(noise).copy()
    e_noise = _noise_err(z, at.SEED, c)
    ref = at.rsample(mean, ls, z)
    assert not ref["bad"].any()
    errs = [_float_err(act, ref["act"], ref["sigma"])]
    if parts["logp"]:
        errs.append(_float_err(logp, ref["logp"], ref["sigma"]))
    else:
        assert bool((logp_g == SENTINEL).all())
    for g in (act_g, logp_g, noise_g):
        assert _guards_intact(g, B, False)
    if stride2:
        assert bool((m_w[:, 1] == SENTINEL).all()) and bool((l_w[:, 1] == SENTINEL).all())
    # backward, its outputs strided like the inputs
    gm, gm_g = _guarded(B, tdt, stride2)
    gs, gs_g = _guarded(B, tdt, stride2)
    ga_d, gl_d = (_t(ga) if parts["ga"] else None), (_t(gl) if parts["gl"] else None)
    out = eng.rsample_backward(m_d, l_d, noise, ga_d, gl_d, out=(gm, gs))
    eng.sync()
    rb = at.rsample_backward(mean, ls, z, ga if parts["ga"] else None, gl if parts["gl"] else None)
    assert out.grad_mean is gm and not rb["bad"].any()
    errs += [_float_err(gm, rb["grad_mean"], ref["sigma"]), _float_err(gs, rb["grad_log_std"], ref["sigma"])]
    assert float(gs[1]) == 0.0 if B > 1 else True             # one spacing below -20: outside the clamp
    assert float(gs[3]) == 0.0 if B > 3 else True
    assert _guards_intact(gm_g, B, stride2) and _guards_intact(gs_g, B, stride2)
    return max(errs), e_noise


@pytest.mark.parametrize("B", at.BS)
def test_rsample_forward_and_backward_over_every_shape(B):
    """B at 1, around the wave, around the 256-thread block, TQC's 290 and SAC's 470; float32 / float64; stride 1 / 2 with guard columns and
    guard rows; each nullable part present and absent (walked diagonally, all of them at B = 290 and 470); the planted clamp-edge rows"""
    eng = _engine()
    ib = at.BS.index(B)
    worst, worst_z, c = 0.0, 0.0, 0
    full = B in (290, 470)
    for i, dt in enumerate(at.DTYPES):
        for j, stride2 in enumerate((False, True)):
            combos = [dict(logp=True, ga=True, gl=True), dict(logp=False, ga=True, gl=False), dict(logp=True, ga=False, gl=True)]
            for k, parts in enumerate(combos):
                if not full and k != (i + j + ib) % 3:
                    continue
                e, ez = _check_rsample(eng, B, dt, stride2, c % 4, parts)
                worst, worst_z, c = max(worst, e), max(worst_z, ez), c + 1
    print(f"rsample B={B}: outputs, max error / bound {worst:.4f}; noise against the restatement's z {worst_z:.4f}")
    assert worst <= 1.0 and worst_z <= 1.0


def test_a_deterministic_call_the_counter_and_the_same_noise_in_every_call_that_draws_it():
    """z = 0 exactly and the counter untouched when deterministic; one step per stochastic call; the same (seed, counter) repeats and two
    calls differ; the noise of a float32 call, a float64 call, a SMOOTH call (through its action at mean 0, sigma_t 1, wide clips) and
    ptg_act's raw sample at mean 0, log_std 0 on an engine with n_envs = B are the same bits; with log_std inside the clamp rsample gives
    the bits of act_gaussian(squash=True)"""
    import torch
    B = 65
    eng = _engine(B)
    assert eng._L.ptg_set_global_env_offset(eng._h, 0) == 0
    mean, ls = ar.gaussian_case(B, np.float32, True)
    m, l = _t(mean), _t(ls)
    counter = eng.new_draw_counter()
    det = eng.rsample(m, l, None, deterministic=True)
    det2 = eng.rsample(m, l, counter, deterministic=True)
    eng.sync()
    assert int(counter) == 0 and bool((det.noise == 0).all()) and torch.equal(det.actions, det2.actions)
    ref = at.rsample(mean, ls, np.zeros(B))
    assert _float_err(det.actions, ref["act"], ref["sigma"]) <= 1.0 and _float_err(det.log_prob, ref["logp"], ref["sigma"]) <= 1.0
    r0 = eng.rsample(m, l, counter, seed=11)
    r1 = eng.rsample(m, l, counter, seed=11)
    eng.sync()
    assert int(counter) == 2 and not torch.equal(r0.noise, r1.noise) and not torch.equal(r0.actions, r1.actions)
    counter.zero_()
    r0b = eng.rsample(m.double(), l.double(), counter, seed=11)
    eng.sync()
    assert torch.equal(r0b.noise.view(torch.int64), r0.noise.view(torch.int64)) and int(counter) == 1
    assert _noise_err(_h(r0.noise), 11, 0) <= 1.0 and _noise_err(_h(r1.noise), 11, 1) <= 1.0
    other = eng.rsample(m, l, torch.zeros_like(counter), seed=12)
    assert not torch.equal(other.noise, r0.noise)
    # the collecting head at the same (seed, counter): bit for bit
    counter.zero_()
    head = eng.act_gaussian(m, l, counter, squash=True, seed=11)
    eng.sync()
    assert torch.equal(head.actions.view(torch.int32), r0.actions.view(torch.int32)) and torch.equal(head.log_prob.view(torch.int32), r0.log_prob.view(torch.int32))
    counter.zero_()
    zero = torch.zeros(B, dtype=torch.float64, device="cuda")
    raw = eng.act_gaussian(zero, zero[:1], counter, seed=11).raw
    counter.zero_()
    sm = eng.smooth_target_action(zero, counter, 1.0, 100.0, clip=(-100.0, 100.0), seed=11)
    eng.sync()
    assert torch.equal(raw.view(torch.int64), r0.noise.view(torch.int64)) and torch.equal(sm.view(torch.int64), r0.noise.view(torch.int64))
    assert int(counter) == 1


@pytest.mark.parametrize("B", at.BS)
def test_the_smoothed_target_action_bit_for_bit(B):
    """TD3's target action at the reference's noise (0.2 clipped to 0.5) and with a clip that bites, float32 / float64, stride 1 / 2: the
    bits of the restatement given the noise of the same (seed, counter), which a SQUASH call hands out"""
    import torch
    eng = _engine()
    for dt in at.DTYPES:
        for stride2 in (False, True):
            mean = np.random.default_rng([29, B]).uniform(-1.3, 1.3, B).astype(dt)
            m_d, m_w = _strided(mean, stride2)
            counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
            z = _h(eng.rsample(m_d, m_d, counter, seed=at.SEED).noise)
            for sd, c, clip in ((0.2, 0.5, (-1.0, 1.0)), (1.0, 0.25, (-0.5, 0.75)), (0.0, 0.0, (-1.0, 1.0))):
                counter.fill_(5)
                out, g = _guarded(B, m_d.dtype, False)
                got = eng.smooth_target_action(m_d, counter, sd, c, clip=clip, seed=at.SEED, out=out)
                eng.sync()
                assert got is out and int(counter) == 6 and _guards_intact(g, B, False)
                _same_bits(out, at.smooth(mean, z, sd, c, *clip)["act"])
            if stride2:
                assert bool((m_w[:, 1] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- the losses
def _alpha_kw(form):
    import torch
    if form == "host":
        return dict(ent_coef=ALPHA), ALPHA, None
    if form == "dev":
        return dict(ent_coef=torch.tensor([ALPHA], dtype=torch.float64, device="cuda")), ALPHA, None
    return dict(log_ent_coef=torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")), None, LOG_ALPHA


def _alpha_of(stats, alpha, log_alpha):
    """the alpha the restatement is fed: the given one, which stats[4] must equal -- or, for a log alpha, the kernel's own stats[4], held
    to np.exp within 2 float64 spacings"""
    got = float(stats[4])
    if log_alpha is None:
        assert got == alpha
        return alpha
    want = float(np.exp(log_alpha))
    dist = abs(got - want) / float(np.spacing(want))
    _worst["exp_spacings"] = max(_worst["exp_spacings"], dist)
    assert dist <= 2.0, (got, want)
    return got


def _means_err(stats, ref, B, log_alpha=None):
    got, want, am = _h(stats), ref["stats"], ref["abs_mean"]
    u = B * 2.0 ** -53 + 1e-12
    e = [abs(got[0] - want[0]) / (u * max(1.0, am["loss"])), abs(got[2] - want[2]) / (u * max(1.0, am["lp"])), abs(got[3] - want[3]) / (u * max(1.0, am["m"]))]
    if log_alpha is not None and want[1] != 0.0:
        e.append(abs(got[1] - want[1]) / (u * max(1.0, abs(log_alpha) * am["s"])))
        e.append(abs(got[5] - want[5]) / (u * max(1.0, am["s"])))
    else:
        assert got[1] == 0.0 and got[5] == 0.0
    assert got[6] == 0.0 and got[7] == 0.0, got
    return max(e)


def _check_loss(eng, B, K, Q, dt, wide, form, want_glp=True, ent_coef_part=False, kind=None, seed=0, ws=None):
    """one actor_loss call against the restatement.  kind None: "sac" for Q = 1, "tqc" else; wide: critics as columns of one [B, K] tensor
    with the gradients in a guarded [B + 2, K + 1] one (sac) / a list of [B, Q] views with row stride Q + 1 and guard rows (tqc); else
    SB3's tuple of [B, 1] tensors (sac) / the stacked contiguous [B, K, Q] tensor (tqc)"""
    import torch
    c = at.al_case(B, K, Q, dt, seed)
    kind = kind or ("sac" if Q == 1 else "tqc")
    kw, alpha, log_alpha = _alpha_kw(form)
    if ent_coef_part and form != "log":
        ent_coef_part = False
    lp = _t(c["lp"]).view(-1, 1)
    tdt = lp.dtype
    stats = _full((8,), torch.float64)
    guards = []
    if kind == "sac":
        if wide:
            Qd = _t(np.concatenate(c["q"], axis=1))
            g = _full((B + 2, K + 1), tdt)
            q, gq = [Qd[:, k] for k in range(K)], [g[1:B + 1, k] for k in range(K)]
            guards.append((g, lambda g: bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all()) and bool((g[:, K] == SENTINEL).all())))
        else:
            q, gq = [_t(x) for x in c["q"]], [_full((B, 1), tdt) if k % 2 == 0 else _full((B,), tdt) for k in range(K)]
        ref_q, ref_kind = at.al_flat(c), "min"
    else:
        if wide:
            q, gq = [], []
            for k in range(K):
                w = _full((B, Q + 1), tdt)
                w[:, :Q] = _t(c["q"][k])
                g = _full((B + 2, Q + 1), tdt)
                q.append(w[:, :Q]); gq.append(g[1:B + 1, :Q])
                guards.append((g, lambda g: bool((g[0] == SENTINEL).all()) and bool((g[-1] == SENTINEL).all()) and bool((g[:, Q] == SENTINEL).all())))
                guards.append((w, lambda w: bool((w[:, Q] == SENTINEL).all())))
        else:
            q, gq = _t(np.stack(c["q"], axis=1)), _full((B, K, Q), tdt)
        ref_q, ref_kind = c["q"], "mean"
    glp = _full((B, 1), tdt) if want_glp else None
    gla = _full((1,), torch.float64) if ent_coef_part else None
    res = eng.actor_loss(kind, q, lp, target_entropy=at.H_T if ent_coef_part else None, out=(stats, gq, glp, gla), workspace=ws, **kw)
    eng.sync()
    a_used = _alpha_of(stats, alpha, log_alpha)
    ref = at.actor_loss(ref_kind, ref_q, c["lp"], alpha=a_used, log_alpha=log_alpha if ent_coef_part else None, target_entropy=at.H_T if ent_coef_part else None)
    assert not ref["bad"].any() and res.stats is stats and res.grad_q is gq
    for k in range(K):
        _same_bits(gq[k] if isinstance(gq, list) else gq[:, k], ref["grad_q"][k])
    if want_glp:
        _same_bits(glp, ref["grad_lp"])
    if ent_coef_part:
        assert float(gla[0]) == float(stats[5])
    for g, ok in guards:
        assert ok(g)
    return _means_err(stats, ref, B, log_alpha if ent_coef_part else None)


def _loss_sweep(eng, B, shift, full):
    worst = 0.0
    for i, (K, Q) in enumerate(at.KQ):
        for a, dt in enumerate(at.DTYPES):
            for b, wide in enumerate((False, True)):
                if not full and (a, b) != ((i + shift) % 2, ((i + shift) // 2) % 2):
                    continue
                n = i + a + b + shift
                worst = max(worst, _check_loss(eng, B, K, Q, dt, wide, ALPHA_FORMS[n % 3], want_glp=n % 2 == 0, ent_coef_part=n % 3 == 2))
        if Q == 1:                                           # the MEAN kind at Q = 1 (TD3's shape) beside the MIN kind
            worst = max(worst, _check_loss(eng, B, K, 1, at.DTYPES[(i + shift) % 2], False, ALPHA_FORMS[(i + shift) % 3], kind="tqc"))
    return worst


@pytest.mark.parametrize("B", at.BS)
def test_actor_loss_over_every_shape(B):
    eng = _engine()
    worst = _loss_sweep(eng, B, at.BS.index(B), B in (290, 470))
    # TD3 (no entropy term) and the entropy-coefficient loss alone
    import torch
    for dt in at.DTYPES:
        c = at.al_case(B, 1, 1, dt)
        stats, gq = _full((8,), torch.float64), _full((B, 1), _t(c["lp"]).dtype)
        res = eng.actor_loss("td3", _t(c["q"][0]), out=(stats, gq, None, None))
        eng.sync()
        ref = at.actor_loss("mean", [c["q"][0]])
        _same_bits(gq, ref["grad_q"][0])
        assert float(stats[4]) == 0.0 and float(stats[2]) == 0.0 and res.grad_log_prob is None
        worst = max(worst, _means_err(stats, ref, B))
        la = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
        for want_gla in (True, False):
            stats, gla = _full((8,), torch.float64), _full((1,), torch.float64)
            res = eng.actor_loss("ent_coef", log_prob=_t(c["lp"]), log_ent_coef=la, target_entropy=at.H_T, out=(stats, None, None, gla if want_gla else None))
            eng.sync()
            a_used = _alpha_of(stats, None, LOG_ALPHA)
            ref = at.actor_loss("alpha_only", None, c["lp"], alpha=a_used, log_alpha=LOG_ALPHA, target_entropy=at.H_T)
            assert float(stats[0]) == 0.0 and float(stats[3]) == 0.0 and float(gla[0]) == (float(stats[5]) if want_gla else SENTINEL)
            worst = max(worst, _means_err(stats, ref, B, LOG_ALPHA))
    print(f"actor_loss B={B}: means, max error / bound {worst:.4f}; exp(log alpha) against np.exp: {_worst['exp_spacings']:.2f} spacings")
    assert worst <= 1.0


def test_a_batch_that_crosses_the_partial_boundaries():
    """65 793 rows = 258 blocks of 256: the final kernel's 256 threads walk the block partials in laps of 256, so two threads take a second
    partial; the last block holds one row"""
    eng = _engine()
    ws = eng.actor_loss_workspace(at.B_BIG)
    worst = max(_check_loss(eng, at.B_BIG, 2, 1, np.float32, True, "log", ent_coef_part=True, ws=ws),
                _check_loss(eng, at.B_BIG, 2, 25, np.float64, False, "dev", ws=ws),
                _check_loss(eng, at.B_BIG, 1, 1, np.float64, False, "host", kind="tqc", ws=ws))
    e_rs, e_z = _check_rsample(eng, at.B_BIG, np.float32, True, 2, dict(logp=True, ga=True, gl=True))
    print(f"B={at.B_BIG}: means, max error / bound {worst:.4f}; rsample outputs {e_rs:.4f}, noise {e_z:.4f}")
    assert worst <= 1.0 and e_rs <= 1.0 and e_z <= 1.0


def test_thread_0_of_the_final_pass_adds_two_partials():
    """the same 65 793 rows (256 * 257 + 1) in float32 with one critic, the smallest K of the sweeps, and a fresh workspace: thread 0 of
    the final kernel adds the partials of blocks 0 and 256 before the block's tree"""
    eng = _engine()
    worst = _check_loss(eng, at.B_BIG, 1, 1, np.float32, False, "host")
    print(f"B={at.B_BIG}, K=1, float32: means, max error / bound {worst:.4f}")
    assert worst <= 1.0


def test_two_runs_give_identical_bits():
    import torch
    eng = _engine()
    for B in (470, at.B_BIG):
        c = at.al_case(B, 2, 30, np.float32)
        q, lp = _t(np.stack(c["q"], axis=1)), _t(c["lp"])
        la = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
        runs = []
        for _ in range(2):
            r = eng.actor_loss("tqc", q, lp, log_ent_coef=la, target_entropy=at.H_T)
            eng.sync()
            runs.append((r.stats.clone(), r.grad_q.clone(), r.grad_log_prob.clone(), r.grad_log_ent_coef.clone()))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs)) and bool(torch.isfinite(runs[0][0]).all())


# ------------------------------------------------------------------------------------------------- the autograd wrappers
def _typed_action_log_prob(mean, log_std, z):
    """SB3's Actor.action_log_prob on the device, the noise given"""
    import torch
    log_std = torch.clamp(log_std, at.LS_MIN, at.LS_MAX)
    std = torch.ones_like(mean) * log_std.exp()
    g = mean + std * z
    a = torch.tanh(g)
    lp = torch.distributions.Normal(mean, std).log_prob(g).sum(dim=1) - torch.log(1 - a ** 2 + 1e-6).sum(dim=1)
    return a, lp.reshape(-1, 1)


def _grad_share(got, ref):
    return max(float((g - r).abs().max()) / (1e-12 * max(1.0, float(r.abs().max()))) for g, r in zip(got, ref))


def test_the_wrappers_drive_networks_as_torch_autograd_does():
    """a float64 Linear(40, 2) actor (mean and log_std columns), two Linear(41, 1) critics and a Linear(41, 2 * 30) quantile critic:
    squashed_rsample + sac / tqc / td3 actor loss + ent_coef_loss, after backward(), leave the parameter gradients of SB3's lines under
    torch autograd on the device, fed the op's own noise, within 1e-12 * max(1, max |ref|); the losses within 1e-12 * max(1, |ref|)"""
    import torch
    from rl_ptg_amd import ent_coef_loss, sac_actor_loss, squashed_rsample, td3_actor_loss, tqc_actor_loss
    eng = _engine()
    B = 470
    torch.manual_seed(5)
    f64 = dict(dtype=torch.float64, device="cuda")
    obs = torch.randn(B, 40, **f64)
    actor = torch.nn.Linear(40, 2).double().cuda()
    with torch.no_grad():
        actor.weight.mul_(0.3); actor.bias[1] = -1.5         # log_std around -1.5: |g| stays small (section 12's conditioning)
    critics = [torch.nn.Linear(41, 1).double().cuda() for _ in range(2)]
    qnet = torch.nn.Linear(41, 60).double().cuda()
    log_alpha = torch.tensor([LOG_ALPHA], requires_grad=True, **f64)
    params = list(actor.parameters())
    counter = eng.new_draw_counter()
    worst = 0.0
    for kind in ("sac", "tqc", "td3"):
        counter.zero_()

        def forward(z=None):
            ml = actor(obs)
            mean, log_std = ml[:, :1], ml[:, 1:]
            if z is None:
                a, lp = squashed_rsample(eng, mean, log_std, counter, seed=3)
            else:
                a, lp = _typed_action_log_prob(mean, log_std, z)
            sa = torch.cat([obs, a], dim=1)
            return a, lp, sa

        for p in params + [log_alpha]:
            p.grad = None
        a, lp, sa = forward()
        assert a.shape == (B, 1) and lp.shape == (B, 1) and a.requires_grad and lp.requires_grad
        z = a.grad_fn.noise.clone() if hasattr(a.grad_fn, "noise") else None
        assert z is not None and z.shape == (B, 1)
        alpha = log_alpha.detach().exp()
        if kind == "sac":
            loss, stats = sac_actor_loss(eng, [c(sa) for c in critics], lp, log_ent_coef=log_alpha)
        elif kind == "tqc":
            loss, stats = tqc_actor_loss(eng, qnet(sa).view(B, 2, 30), lp, ent_coef=alpha)
        else:
            loss, stats = td3_actor_loss(eng, critics[0](sa))
        el, el_stats = ent_coef_loss(eng, lp, log_alpha, target_entropy=at.H_T)
        assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.requires_grad and not stats.requires_grad and el.requires_grad
        (loss + el).backward()
        eng.sync()
        got = [p.grad.clone() for p in params + [log_alpha]]
        got_loss, got_el = float(loss.detach()), float(el.detach())
        assert float(stats[0]) == got_loss and float(el_stats[1]) == got_el
        for p in params + [log_alpha]:
            p.grad = None
        a2, lp2, sa2 = forward(z)
        if kind == "sac":
            ref_loss = (alpha * lp2 - torch.min(torch.cat([c(sa2) for c in critics], dim=1), dim=1, keepdim=True)[0]).mean()
        elif kind == "tqc":
            ref_loss = (alpha * lp2 - qnet(sa2).view(B, 2, 30).mean(dim=2).mean(dim=1, keepdim=True)).mean()
        else:
            ref_loss = -critics[0](sa2).mean()
        ref_el = -(log_alpha * (lp2 + at.H_T).detach()).mean()
        (ref_loss + ref_el).backward()
        ref = [p.grad.clone() for p in params + [log_alpha]]
        worst = max(worst, _grad_share(got, ref))
        assert abs(got_loss - float(ref_loss.detach())) <= 1e-12 * max(1.0, abs(float(ref_loss.detach()))), kind
        assert abs(got_el - float(ref_el.detach())) <= 1e-12 * max(1.0, abs(float(ref_el.detach()))), kind
        assert float((a.detach() - a2.detach()).abs().max()) <= 1e-12 and float((lp.detach() - lp2.detach()).abs().max()) <= 1e-11
    print(f"parameter gradients: max error / tolerance {worst:.4f}")
    assert worst <= 1.0
    with torch.no_grad():                                    # the critic target's call: nothing is kept
        a, lp = squashed_rsample(eng, actor(obs)[:, :1], actor(obs)[:, 1:], counter, seed=3)
    eng.sync()
    assert not a.requires_grad and not lp.requires_grad


# ------------------------------------------------------------------------------------------------- a whole captured step
@pytest.mark.parametrize("B", [64, 470])
def test_a_full_sac_step_captured_and_replayed_three_times(B):
    """DeviceReplayBuffer.add -> sample -> actor -> squashed_rsample (no_grad on the next observations, with a graph on the current ones)
    -> ent_coef_loss -> sac_critic_loss -> DeviceOptimizer.step(tau=0.005) -> sac_actor_loss -> the actor's and log alpha's steps, in SB3's
    order, captured once on a side stream at the default hardware-queue setting and replayed three times with the step's inputs
    rewritten; one launch per loss at B = 64, two at 470.  After every replay the step's own tensors are held to the restatement: fresh
    noise (the counter moved on), the sample, the three losses with the alpha from BEFORE the alpha step, moved parameters and targets."""
    import torch
    from rl_ptg_amd import DeviceOptimizer, DeviceReplayBuffer, ent_coef_loss, sac_actor_loss, sac_critic_loss, squashed_rsample
    import td_loss_restatement as tr
    N, T = 64, 12
    eng = _engine(N, fresh=True)
    F = eng.obs_dim
    buf = DeviceReplayBuffer(eng, 16 * N, columns={"actions": torch.float32}, seed=3)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    prev0 = eng.rows(eng.reset()).clone()
    obs, rew, done = eng.rollout(torch.randint(0, 5, (T, N), dtype=torch.int64, device="cuda", generator=g))
    cont = torch.rand((T, N), device="cuda", generator=g) * 2 - 1
    buf.add(prev0, obs[:8], rew[:8], done[:8], actions=cont[:8])             # 512 transitions before the step
    prev_s, obs_s, rew_s, done_s, act_s = obs[7].clone(), obs[8].clone(), rew[8].clone(), done[8].clone(), cont[8].clone()
    torch.manual_seed(13)
    actor = torch.nn.Linear(F, 2).cuda()
    with torch.no_grad():
        actor.weight.mul_(0.05); actor.bias[1] = -1.5
    critics = [torch.nn.Linear(F + 1, 1).cuda() for _ in range(2)]
    targets = [torch.nn.Linear(F + 1, 1).cuda() for _ in range(2)]
    log_alpha = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda", requires_grad=True)
    ap, cp, tp = list(actor.parameters()), [p for m in critics for p in m.parameters()], [p for m in targets for p in m.parameters()]
    opt_a = DeviceOptimizer(eng, ap, kind="adam", lr=3e-4, zero_grad=True)
    opt_c = DeviceOptimizer(eng, cp, kind="adam", lr=3e-4, targets=tp, tau=0.005, zero_grad=True)
    opt_l = DeviceOptimizer(eng, [log_alpha], kind="adam", lr=1e-2, zero_grad=True)
    counter = eng.new_draw_counter()
    raw = eng.replay_sample(buf.storage, batch_size=B, seed=buf.seed)
    gamma = tr.GAMMA["sac"]
    keep = {}

    def step():
        buf.add(prev_s, obs_s, rew_s, done_s, actions=act_s)
        s = buf.sample(B, out=raw)
        with torch.no_grad():
            nml = actor(s.next_observations)
            na, nlp = squashed_rsample(eng, nml[:, :1], nml[:, 1:], counter, seed=21)
            nq = [m(torch.cat([s.next_observations, na], dim=1)) for m in targets]
        ml = actor(s.observations)
        a, lp = squashed_rsample(eng, ml[:, :1], ml[:, 1:], counter, seed=21)
        el, el_stats = ent_coef_loss(eng, lp, log_alpha, target_entropy=at.H_T)
        alpha = el_stats[4:5]                                # the alpha from before the alpha step, on the device
        el.backward()
        q = [m(torch.cat([s.observations, s.actions], dim=1)) for m in critics]
        cl, c_stats = sac_critic_loss(eng, q, nq, s.rewards, s.dones, nlp, gamma=gamma, ent_coef=alpha)
        cl.backward()
        opt_c.step()
        q_pi = [m(torch.cat([s.observations, a], dim=1)) for m in critics]
        al, a_stats = sac_actor_loss(eng, q_pi, lp, ent_coef=alpha)
        for p, gr in zip(ap, torch.autograd.grad(al, ap)):  # the actor's parameters alone, as SB3's actor optimiser sees them
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(gr)
        opt_a.step()
        opt_l.step()
        keep.update(ml=ml.detach(), nml=nml, a=a.detach(), lp=lp.detach(), nlp=nlp, noise=a.grad_fn.noise, q=[t.detach() for t in q], nq=nq,
                    q_pi=[t.detach() for t in q_pi], el=el_stats, cs=c_stats, as_=a_stats, s=s)

    def check(k, c0, la_before):
        eng.sync()
        assert int(counter) == c0 + 2 and buf.cursor()[0] == 8 + k + 1
        ml, z = _h(keep["ml"]), _h(keep["noise"]).reshape(-1)
        assert _noise_err(z, 21, c0 + 1) <= 1.0
        ref = at.rsample(ml[:, 0], ml[:, 1], z)
        assert not ref["bad"].any() and np.abs(ref["g"]).max() < 4.0
        e = [_float_err(keep["a"], ref["act"], ref["sigma"]), _float_err(keep["lp"], ref["logp"], ref["sigma"])]
        lp = _h(keep["lp"]).reshape(-1)
        a_used = float(keep["el"][4])
        assert abs(a_used - np.exp(la_before)) <= 2 * np.spacing(np.exp(la_before)) and float(keep["as_"][4]) == a_used and float(keep["cs"][5]) == a_used
        r_el = at.actor_loss("alpha_only", None, lp, alpha=a_used, log_alpha=la_before, target_entropy=at.H_T)
        r_al = at.actor_loss("min", [_h(t).reshape(-1) for t in keep["q_pi"]], lp, alpha=a_used)
        e += [_means_err(keep["el"], r_el, B, la_before), _means_err(keep["as_"], r_al, B)]
        s = keep["s"]
        r_c = tr.td_loss("sac", [_h(t).reshape(-1) for t in keep["q"]], [_h(t).reshape(-1) for t in keep["nq"]], _h(s.rewards), _h(s.dones), gamma,
                         next_log_prob=_h(keep["nlp"]).reshape(-1), alpha=a_used)
        u = B * 2.0 ** -53 + 1e-12
        e.append(abs(float(keep["cs"][0]) - r_c["stats"][0]) / (u * max(1.0, r_c["abs_mean"]["loss"])))
        assert max(e) <= 1.0, (k, e)
        return max(e)

    la0 = float(log_alpha.detach())
    step()                                                   # eager once: code objects are loaded, the gradients and the optimisers' tables exist
    worst = check(0, 0, la0)
    before = [p.detach().clone() for p in ap + cp + tp + [log_alpha]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(counter) == 2 and buf.cursor()[0] == 9 and all(torch.equal(p.detach(), b) for p, b in zip(ap + cp + tp + [log_alpha], before))      # capturing enqueued nothing
    for k in (1, 2, 3):
        prev_s.copy_(obs[7 + k]); obs_s.copy_(obs[8 + k]); rew_s.copy_(rew[8 + k]); done_s.copy_(done[8 + k]); act_s.copy_(cont[8 + k])
        if k == 2:
            with torch.no_grad():
                log_alpha.fill_(-0.25)                       # a moved log alpha, beside the optimiser's own steps
        la_before = float(log_alpha.detach())
        graph.replay()
        torch.cuda.synchronize()
        worst = max(worst, check(k, 2 * k, la_before))
        assert float(log_alpha.detach()) != la_before
    after = [p.detach() for p in ap + cp + tp]
    assert all(not torch.equal(a, b) for a, b in zip(after, before[:-1])) and all(bool(torch.isfinite(a).all()) for a in after)
    print(f"captured SAC step B={B}: max error / bound over the eager step and three replays {worst:.4f}")
    eng.close()


# ------------------------------------------------------------------------------------------------- streams, synchronisation, state
def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they have
    returned; with out= and workspace= the allocator hands out nothing during them.  Afterwards env state, finished ring, vn statistics
    and a replay cursor equal a twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
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
    buf = DeviceReplayBuffer(eng, 2 * n)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    z_host = at.draw(9, 0, n)
    mean, ls = at.rs_case(n, np.float32, z_host)
    ga, gl = at.grads_case(n, np.float32)
    m, l, ga_d, gl_d = _t(mean), _t(ls), _t(ga), _t(gl)
    c = at.al_case(n, 2, 1, np.float32)
    q, lp = [_t(x) for x in c["q"]], _t(c["lp"])
    la = torch.tensor([LOG_ALPHA], dtype=torch.float64, device="cuda")
    counter = eng.new_draw_counter()
    f32 = lambda *s: torch.empty(s, device="cuda")
    rs_out = (f32(n), f32(n), torch.empty(n, dtype=torch.float64, device="cuda"))
    bw_out, sm_out = (f32(n), f32(n)), f32(n)
    al_out = (torch.empty(8, dtype=torch.float64, device="cuda"), [f32(n, 1), f32(n, 1)], f32(n), torch.empty(1, dtype=torch.float64, device="cuda"))
    ws = eng.actor_loss_workspace(n)

    def ops():
        eng.rsample(m, l, counter, seed=9, out=rs_out)
        eng.rsample_backward(m, l, rs_out[2], ga_d, gl_d, out=bw_out)
        eng.smooth_target_action(m, counter, 0.2, 0.5, seed=9, out=sm_out)
        eng.actor_loss("sac", q, lp, log_ent_coef=la, target_entropy=at.H_T, out=al_out, workspace=ws)

    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                            # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    ops()
    torch.cuda.synchronize()
    counter.zero_()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    ops()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    assert allocs_after == allocs, "a call with out= and workspace= allocated device memory"
    eng.sync()
    z = _h(rs_out[2])
    ref = at.rsample(mean, ls, z)
    assert _noise_err(z, 9, 0) <= 1.0 and _float_err(rs_out[0], ref["act"], ref["sigma"]) <= 1.0 and int(counter) == 2
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


def test_on_a_side_stream():
    import torch
    eng = _engine()
    B = 257
    c = at.al_case(B, 2, 1, np.float64)
    side = torch.cuda.Stream()
    q, lp = [_t(x) for x in c["q"]], _t(c["lp"])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = eng.actor_loss("sac", q, lp, ent_coef=ALPHA)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    ref = at.actor_loss("min", at.al_flat(c), c["lp"], alpha=ALPHA)
    for k in range(2):
        _same_bits(res.grad_q[k], ref["grad_q"][k])
    assert _means_err(res.stats, ref, B) <= 1.0


# ------------------------------------------------------------------------------------------------- bad rows and refusals
def test_bad_rows():
    """planted as data, which the kernels must classify: a NaN and an infinite mean, a NaN log_std (an infinite one clamps and is legal);
    in the backward also a non-finite noise value and incoming gradient; a NaN critic, a -Inf minimum, a non-finite log-prob, a
    non-finite quantile, alpha = NaN in its three forms; NaN outputs on those rows, the other rows correct, PTG_E_NONFINITE once, and a
    clean call syncs clean"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    eng = _engine()
    B = 300                                                  # two blocks: the two-launch route of the loss

    def expect():
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == _lib.E_NONFINITE
        eng.sync()

    for dt in at.DTYPES:
        z_host = at.draw(at.SEED, 3, B)                      # a counter value whose rows the host test has vetted
        mean, ls = at.rs_case(B, dt, z_host)
        mean[20] = np.nan; mean[277] = np.inf; ls[30] = np.nan
        ls[40] = np.inf; ls[50] = -np.inf                     # legal: they clamp
        mean[40] = dt(0.3 - np.exp(2.0) * z_host[40])
        counter = torch.full((1,), 3, dtype=torch.int64, device="cuda")
        res = eng.rsample(_t(mean), _t(ls), counter, seed=at.SEED)
        expect()
        z = _h(res.noise)
        ref = at.rsample(mean, ls, z)
        bad = [20, 30, 277]
        assert np.nonzero(ref["bad"])[0].tolist() == bad and np.isfinite(z).all()
        assert np.nonzero(np.isnan(_h(res.actions)))[0].tolist() == bad and np.nonzero(np.isnan(_h(res.log_prob)))[0].tolist() == bad
        ok = ~ref["bad"]
        assert _float_err(res.actions[_t(ok)], ref["act"][ok], ref["sigma"][ok]) <= 1.0 and _float_err(res.log_prob[_t(ok)], ref["logp"][ok], ref["sigma"][ok]) <= 1.0
        sm = eng.smooth_target_action(_t(mean), counter, 0.2, 0.5, seed=at.SEED)
        expect()
        assert np.nonzero(np.isnan(_h(sm)))[0].tolist() == [20, 277]
        ga, gl = at.grads_case(B, dt)
        ga[60] = np.inf; gl[70] = np.nan
        noise = res.noise.clone(); noise[80] = float("inf")
        out = eng.rsample_backward(_t(mean), _t(ls), noise, _t(ga), _t(gl))
        expect()
        rb = at.rsample_backward(mean, ls, _h(noise), ga, gl)
        bad = [20, 30, 60, 70, 80, 277]
        assert np.nonzero(rb["bad"])[0].tolist() == bad
        assert np.nonzero(np.isnan(_h(out.grad_mean)))[0].tolist() == bad and np.nonzero(np.isnan(_h(out.grad_log_std)))[0].tolist() == bad
        assert float(out.grad_log_std[40]) == 0.0 and float(out.grad_log_std[50]) == 0.0
        ok = ~rb["bad"]
        assert _float_err(out.grad_mean[_t(ok)], rb["grad_mean"][ok], ref["sigma"][ok]) <= 1.0
        # the losses
        c = at.al_case(B, 2, 1, dt)
        q = at.al_flat(c)
        q[1][20] = np.nan; q[0][277] = np.nan; q[1][30] = -np.inf; c["lp"][40] = np.inf
        q[0][50] = np.inf                                     # legal beside a smaller value
        res = eng.actor_loss("sac", [_t(x) for x in q], _t(c["lp"]), ent_coef=ALPHA)
        expect()
        ref = at.actor_loss("min", q, c["lp"], alpha=ALPHA)
        assert np.nonzero(ref["bad"])[0].tolist() == [20, 30, 40, 277]
        for k in range(2):
            _same_bits(res.grad_q[k], ref["grad_q"][k])
        _same_bits(res.grad_log_prob, ref["grad_lp"])
        assert bool(torch.isnan(res.stats[[0, 1, 2, 3, 5]]).all()) and float(res.stats[4]) == ALPHA and float(res.grad_q[1][50]) == float(dt(-1.0 / B))
        c = at.al_case(B, 2, 30, dt)
        c["q"][1][20, 29] = np.inf; c["q"][0][277, 0] = np.nan
        res = eng.actor_loss("tqc", _t(np.stack(c["q"], axis=1)), _t(c["lp"]), ent_coef=ALPHA)
        expect()
        ref = at.actor_loss("mean", c["q"], c["lp"], alpha=ALPHA)
        assert np.nonzero(ref["bad"])[0].tolist() == [20, 277]
        for k in range(2):
            _same_bits(res.grad_q[:, k], ref["grad_q"][k])
        c = at.al_case(B, 2, 1, dt)                           # alpha = NaN: every row
        nan64 = torch.tensor([np.nan], dtype=torch.float64, device="cuda")
        for kw in (dict(ent_coef=float("nan")), dict(ent_coef=nan64), dict(log_ent_coef=nan64), dict(log_ent_coef=nan64, target_entropy=at.H_T)):
            res = eng.actor_loss("sac", [_t(x) for x in c["q"]], _t(c["lp"]), **kw)
            expect()
            assert all(bool(torch.isnan(g).all()) for g in res.grad_q) and bool(torch.isnan(res.grad_log_prob).all()) and bool(torch.isnan(res.stats[:6]).all())
            assert res.grad_log_ent_coef is None or bool(torch.isnan(res.grad_log_ent_coef).all())
        res = eng.actor_loss("ent_coef", log_prob=_t(c["lp"]), log_ent_coef=torch.tensor([-np.inf], dtype=torch.float64, device="cuda"), target_entropy=at.H_T)
        expect()
        assert bool(torch.isnan(res.stats[[1, 2, 5]]).all()) and float(res.stats[4]) == 0.0
    res = eng.actor_loss("td3", _t(c["q"][0]))               # a clean call syncs clean
    eng.sync()
    assert bool(torch.isfinite(res.stats).all())


def test_refused_descriptors_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B = 300
    L, h, stream = eng._L, eng._h, eng._stream()
    f32 = lambda *s: _full(s, torch.float32)
    mean, ls, act, logp, ga, gm, gs = (f32(B) for _ in range(7))
    noise, stats, a64, gla = _full((B,), torch.float64), _full((8,), torch.float64), torch.tensor([ALPHA], dtype=torch.float64, device="cuda"), _full((1,), torch.float64)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    q, gq, glp = f32(B, 2, 30), f32(B, 2, 30), f32(B)
    ws = eng.actor_loss_workspace(B)
    ws.fill_(0x5A)
    torch.cuda.synchronize()

    def fill(ds, kw):
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for j, x in enumerate(v):
                    getattr(ds, k)[j] = x
            else:
                setattr(ds, k, v)
        return ds

    p = lambda t, off=0: t.data_ptr() + off

    def fwd(**kw):
        a = dict(kind=_lib.RS_SQUASH, q_dtype=_lib.OUT_F32, batch=B, mean_dev=p(mean), mean_s_n=1, log_std_dev=p(ls), log_std_s_n=1, seed=1, counter_dev=p(counter),
                 act_dev=p(act), logp_dev=p(logp), noise_dev=p(noise))
        a.update(kw)
        return fill(_lib.PtgRs(), a)

    def smooth(**kw):
        return fwd(**{**dict(kind=_lib.RS_SMOOTH, log_std_dev=None, log_std_s_n=0, logp_dev=None, noise_std=0.2, noise_clip=0.5, clip_lo=-1.0, clip_hi=1.0), **kw})

    def bwd(**kw):
        a = dict(kind=_lib.RS_SQUASH, q_dtype=_lib.OUT_F32, batch=B, mean_dev=p(mean), mean_s_n=1, log_std_dev=p(ls), log_std_s_n=1, noise_dev=p(noise),
                 grad_act_dev=p(ga), grad_logp_dev=p(ga), grad_mean_dev=p(gm), gm_s_n=1, grad_log_std_dev=p(gs), gl_s_n=1)
        a.update(kw)
        return fill(_lib.PtgRs(), a)

    def al(**kw):
        a = dict(kind=_lib.AL_MEAN, flags=_lib.AL_ENTROPY | _lib.AL_LOG_ALPHA | _lib.AL_ENT_COEF, n_critics=2, n_quantiles=30, q_dtype=_lib.OUT_F32, batch=B,
                 q_dev=[p(q), p(q, 120)], q_s_n=[60, 60], logp_dev=p(mean), alpha_dev=p(a64), target_entropy=-1.0, stats_dev=p(stats),
                 grad_q_dev=[p(gq), p(gq, 120)], g_s_n=[60, 60], grad_logp_dev=p(glp), grad_log_alpha_dev=p(gla), ws_dev=p(ws))
        a.update(kw)
        return fill(_lib.PtgAl(), a)

    inf, nan = float("inf"), float("nan")
    bad_f = [fwd(kind=2), fwd(kind=-1), fwd(flags=2), fwd(q_dtype=2), fwd(batch=0), fwd(batch=2 ** 31 + 1), fwd(mean_dev=None), fwd(mean_s_n=0), fwd(log_std_dev=None),
             fwd(log_std_s_n=0), fwd(act_dev=None), fwd(counter_dev=None), fwd(noise_dev=p(noise, 4)), smooth(logp_dev=p(logp)), smooth(noise_std=-0.1), smooth(noise_std=inf),
             smooth(noise_std=nan), smooth(noise_clip=-1.0), smooth(noise_clip=nan), smooth(clip_lo=1.0, clip_hi=-1.0), smooth(clip_lo=nan), smooth(counter_dev=None)]
    bad_b = [bwd(kind=_lib.RS_SMOOTH), bwd(noise_dev=None), bwd(noise_dev=p(noise, 4)), bwd(grad_act_dev=None, grad_logp_dev=None), bwd(grad_mean_dev=None),
             bwd(grad_log_std_dev=None), bwd(gm_s_n=0), bwd(gl_s_n=-1), bwd(q_dtype=-1), bwd(batch=0), bwd(mean_dev=None), bwd(log_std_dev=None), bwd(flags=4)]
    E, LA, EC = _lib.AL_ENTROPY, _lib.AL_LOG_ALPHA, _lib.AL_ENT_COEF
    bad_l = [al(kind=3), al(kind=-1), al(flags=8), al(flags=15), al(q_dtype=2), al(batch=0), al(batch=2 ** 31 + 1), al(stats_dev=None), al(ws_dev=None), al(ws_dev=p(ws, 4)),
             al(n_critics=0), al(n_critics=5), al(n_quantiles=0), al(n_quantiles=65), al(q_dev=[p(q), None]), al(grad_q_dev=[None, p(gq)]), al(q_s_n=[60, 29]),
             al(g_s_n=[29, 60]), al(kind=_lib.AL_MIN, q_s_n=[0, 1]), al(kind=_lib.AL_MIN, g_s_n=[1, -1]), al(logp_dev=None), al(alpha_dev=None), al(flags=E | EC),
             al(flags=LA), al(flags=E | LA | EC, target_entropy=nan), al(target_entropy=inf), al(flags=0, grad_log_alpha_dev=None), al(flags=E, grad_logp_dev=p(glp)),
             al(flags=E | LA, grad_logp_dev=None), al(grad_log_alpha_dev=p(gla, 4)), al(kind=_lib.AL_ALPHA_ONLY), al(kind=_lib.AL_ALPHA_ONLY, flags=LA, grad_logp_dev=None, grad_log_alpha_dev=None),
             al(kind=_lib.AL_ALPHA_ONLY, flags=E | LA, grad_log_alpha_dev=None)]
    for fn, name, group in ((L.ptg_rsample, b"ptg_rsample", bad_f), (L.ptg_rsample_backward, b"ptg_rsample_backward", bad_b), (L.ptg_actor_loss, b"ptg_actor_loss", bad_l)):
        for k, ds in enumerate(group):
            assert fn(h, C.byref(ds), stream) == _lib.E_INVALID, (name, k)
            assert name in L.ptg_last_error(h)
            assert torch.cuda.current_stream().query() is True, (name, k)
        assert fn(h, None, stream) == _lib.E_INVALID and fn(None, C.byref(group[0]), stream) == _lib.E_INVALID
    assert torch.cuda.current_stream().query() is True
    for t in (act, logp, gm, gs, noise, stats, gla, gq, glp):
        assert bool((t == SENTINEL).all())
    assert bool((ws == 0x5A).all()) and int(counter) == 0
    good_f = [fwd(), fwd(logp_dev=None, noise_dev=None), fwd(flags=_lib.RS_DETERMINISTIC, counter_dev=None), fwd(batch=1), smooth(), smooth(noise_std=0.0, noise_clip=inf),
              smooth(flags=_lib.RS_DETERMINISTIC, counter_dev=None)]
    good_b = [bwd(), bwd(grad_act_dev=None), bwd(grad_logp_dev=None), bwd(noise_std=nan, clip_lo=2.0, clip_hi=1.0, act_dev=None, counter_dev=None)]
    good_l = [al(), al(grad_logp_dev=None, grad_log_alpha_dev=None), al(flags=E, alpha_dev=None, alpha=0.2, grad_log_alpha_dev=None), al(flags=E, grad_log_alpha_dev=None),
              al(flags=0, grad_logp_dev=None, grad_log_alpha_dev=None, logp_dev=None, alpha_dev=None), al(kind=_lib.AL_MIN, n_quantiles=99),
              al(kind=_lib.AL_ALPHA_ONLY, flags=LA | EC, grad_logp_dev=None, n_critics=77, q_dev=[None, None]), al(n_critics=1, q_dev=[p(q), None])]
    mean.uniform_(-1, 1); ls.uniform_(-3, -1); ga.uniform_(-1, 1); q.uniform_(-1, 1)
    torch.cuda.synchronize()
    for fn, group in ((L.ptg_rsample, good_f), (L.ptg_rsample_backward, good_b), (L.ptg_actor_loss, good_l)):
        for k, ds in enumerate(group):
            assert fn(h, C.byref(ds), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(act).all()) and bool(torch.isfinite(gm).all()) and int(counter) == 5
