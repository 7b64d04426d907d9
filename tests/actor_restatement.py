"""ptg_rsample / ptg_rsample_backward / ptg_actor_loss (include/ptg_env.h states the lines) restated in float64 NumPy for
tests/test_actor_host.py and tests/test_actor.py: SB3 2.0.0a13's Actor.action_log_prob (the log_std clamp, the reparametrised sample,
tanh, the Gaussian log-density and the tanh correction) with its closed-form backward, TD3's target-policy smoothing, and the actor and
entropy-coefficient losses of SAC, TQC and TD3 with their gradients.  The draw is tests/act_restatement.py's (words / normal), keyed
(seed, counter, row) with no env offset.  Operand order is the header's, so everything that holds no transcendental and no cross-lane
sum is the kernel's bit for bit; sums are NumPy's (the tests' tolerance for a mean covers any order).
The second half builds the inputs the GPU tests use, so that the host test can vet them."""
import numpy as np

import act_restatement as ar

HALF_LOG_2PI = 0.9189385332046727
LS_MIN, LS_MAX = -20.0, 2.0
H_T = -1.0                                                  # SB3's target_entropy = -dim(action space)


def _f(a):
    return np.asarray(a).astype(np.float64)


def draw(seed, c, B):
    """z of rows 0 .. B - 1 of the c-th call under seed"""
    w0, w1 = ar.words(seed, c, np.arange(B))
    return ar.normal(w0, w1)


def clamp_log_std(l):
    """-> (ls, pass): compare-selects that fall through, so a NaN stays NaN; pass is torch's clamp gradient, inclusive at both ends"""
    with np.errstate(invalid="ignore"):
        ls = np.where(l < LS_MIN, LS_MIN, np.where(l > LS_MAX, LS_MAX, l))
        return ls, (LS_MIN <= l) & (l <= LS_MAX)


def rsample(mean, log_std, z):
    """-> dict(act, logp (NaN on a bad row), bad, g, sigma)"""
    mu, l, z = _f(mean).reshape(-1), _f(log_std).reshape(-1), _f(z).reshape(-1)
    bad = ~np.isfinite(mu) | np.isnan(l)
    ls, _ = clamp_log_std(l)
    with np.errstate(all="ignore"):
        sigma = np.exp(ls)
        g = mu + sigma * z
        a = np.tanh(g)
        lp = (((-(z * z)) / 2.0 - ls) - HALF_LOG_2PI) - np.log((1.0 - a * a) + 1e-6)
    return dict(act=np.where(bad, np.nan, a), logp=np.where(bad, np.nan, lp), bad=bad, g=g, sigma=sigma)


def rsample_backward(mean, log_std, z, grad_act=None, grad_logp=None):
    """-> dict(grad_mean, grad_log_std (NaN on a bad row), bad)"""
    mu, l, z = _f(mean).reshape(-1), _f(log_std).reshape(-1), _f(z).reshape(-1)
    ga = np.zeros_like(mu) if grad_act is None else _f(grad_act).reshape(-1)
    gl = np.zeros_like(mu) if grad_logp is None else _f(grad_logp).reshape(-1)
    bad = ~np.isfinite(mu) | np.isnan(l) | ~np.isfinite(z) | ~np.isfinite(ga) | ~np.isfinite(gl)
    ls, ok = clamp_log_std(l)
    with np.errstate(all="ignore"):
        sigma = np.exp(ls)
        a = np.tanh(mu + sigma * z)
        d = 1.0 - a * a
        sz = sigma * z
        q = ((2.0 * a) * d) / (d + 1e-6)
        gm = ga * d + gl * q
        gs = np.where(ok, ga * (d * sz) + gl * (q * sz - 1.0), 0.0)
    return dict(grad_mean=np.where(bad, np.nan, gm), grad_log_std=np.where(bad, np.nan, gs), bad=bad)


def smooth(mean, z, noise_std, noise_clip, lo=-1.0, hi=1.0):
    """TD3's target action; -> dict(act, bad)"""
    mu, z = _f(mean).reshape(-1), _f(z).reshape(-1)
    bad = ~np.isfinite(mu)
    with np.errstate(invalid="ignore"):
        n = noise_std * z
        nc = np.where(n < -noise_clip, -noise_clip, np.where(n > noise_clip, noise_clip, n))
        x = mu + nc
        x = np.where(x < lo, lo, np.where(x > hi, hi, x))
    return dict(act=np.where(bad, np.nan, x), bad=bad)


def actor_loss(kind, q=None, lp=None, alpha=0.0, log_alpha=None, target_entropy=None, entropy=None):
    """kind "min": q a list of K arrays [B]; "mean": a list of K arrays [B, Q]; "alpha_only": no q.  alpha: the coefficient AS USED
    (the caller takes np.exp of a log alpha, or the kernel's stats[4]); log_alpha and target_entropy: the entropy-coefficient loss is
    emitted too.  entropy: the alpha * lp term (default: whenever lp is given and kind is not alpha_only).
    -> dict(stats [8], grad_q (list of K arrays shaped like q[k]), grad_lp [B], grad_la, bad [B], m, abs_mean {name: mean |term|})"""
    only = kind == "alpha_only"
    ec = target_entropy is not None
    if entropy is None:
        entropy = lp is not None and not only
    reads_lp = entropy or ec
    with np.errstate(all="ignore"):
        if only:
            lpv = _f(lp).reshape(-1)
            B = lpv.shape[0]
            m, ks, K, Q = np.zeros(B), None, 0, 1
        else:
            xs = [_f(t) for t in q]
            K, B = len(xs), xs[0].shape[0]
            lpv = _f(lp).reshape(-1) if reads_lp else np.zeros(B)
            if kind == "min":
                xs = [t.reshape(-1) for t in xs]
                Q = 1
                m, ks = xs[0].copy(), np.zeros(B, np.int64)
                for k in range(1, K):
                    l = xs[k]
                    take = (l < m) | np.isnan(l)
                    m, ks = np.where(take, l, m), np.where(take, k, ks)
            else:
                Q = xs[0].shape[1]
                s = np.zeros(B)
                for k in range(K):
                    t = np.zeros(B)
                    for i in range(Q):
                        t = t + xs[k][:, i]
                    s = s + t / float(Q)
                m = s / float(K)
        Bd = float(B)
        a_ok = np.isfinite(alpha) and (log_alpha is None or np.isfinite(log_alpha))
        bad = ~np.isfinite(m) | ~np.isfinite(lpv) | (not a_ok)
        term = alpha * lpv - m if entropy else -m
        grad_q = None
        if kind == "min":
            gq = (-1.0) / Bd
            grad_q = [np.where(bad, np.nan, np.where(ks == k, gq, 0.0)) for k in range(K)]
        elif kind == "mean":
            gq = (-1.0) / ((Bd * float(K)) * float(Q))
            grad_q = [np.where(bad[:, None], np.nan, np.full((B, Q), gq)) for k in range(K)]
        grad_lp = np.where(bad, np.nan, alpha / Bd)
        any_bad = bool(bad.any())
        stats = np.zeros(8)
        stats[4] = alpha if reads_lp else 0.0
        if not only:
            stats[0], stats[3] = term.sum() / Bd, m.sum() / Bd
        if reads_lp:
            stats[2] = lpv.sum() / Bd
        grad_la = None
        if ec:
            sb = (lpv + target_entropy).sum() / Bd
            stats[1], stats[5] = -(log_alpha * sb), -sb
            grad_la = np.nan if any_bad else stats[5]
        if any_bad:
            stats[[0, 1, 2, 3, 5]] = np.nan
        ok = ~bad
        am = lambda t: float(np.abs(t[ok]).mean()) if ok.any() else 0.0
        return dict(stats=stats, grad_q=grad_q, grad_lp=grad_lp, grad_la=grad_la, bad=bad, m=m,
                    abs_mean=dict(loss=am(term), lp=am(lpv), m=am(m), s=am(lpv + (target_entropy or 0.0))))


# ------------------------------------------------------------------------------------------------- the inputs of the tests
BS = [1, 63, 64, 65, 256, 257, 290, 470]              # the wave edges, the edge between the one- and the two-launch route, TQC's and SAC's batches
B_BIG = 65793                                         # 258 block partials: the final pass crosses its 256-thread lap
KQ = [(1, 1), (2, 1), (4, 1), (2, 30), (2, 25), (4, 64)]
DTYPES = [np.float32, np.float64]
SEED = 0xAC7020C0FFEE5EED
PLANTED_RS = ("log_std = -20", "one spacing below -20", "log_std = 2", "one spacing above 2")
N_PLANTED_RS = 4


def rs_case(B, dt, z):
    """means in [-1, 1], log_std in [-3, -0.5] as tests/act_restatement.gaussian_case (|g| < 4 on the rows drawn: asserted on the host),
    with the planted rows 0 .. 3 (as many as fit).  The rows at the upper clamp edge have sigma = e^2 = 7.39, so their means are set to
    0.3 - sigma * z for the z THIS call will draw: g stays near 0.3 and 1 - tanh(g)^2 + 1e-6 well conditioned there too.  The rows at
    the lower edge have sigma = e^-20 = 2e-9 and mean exactly 0: SB3's Normal.log_prob recovers z as (g - mean) / sigma, which beside a
    mean of order 1 would lose eight digits of z in torch's own lines (the header's lines keep z and lose none)."""
    rng = np.random.default_rng([17, B, np.dtype(dt).itemsize])
    mean = rng.uniform(-1.0, 1.0, B).astype(dt)
    ls = rng.uniform(-3.0, -0.5, B).astype(dt)
    plant = [dt(LS_MIN), np.nextafter(dt(LS_MIN), dt(-np.inf)), dt(LS_MAX), np.nextafter(dt(LS_MAX), dt(np.inf))]
    for r, v in enumerate(plant):
        if r < B:
            ls[r] = v
            mean[r] = dt(0.3 - np.exp(LS_MAX) * float(z[r])) if r >= 2 else dt(0.0)
    return mean, ls


def grads_case(B, dt):
    """incoming gradients of the backward, |.| <= 4"""
    rng = np.random.default_rng([19, B, np.dtype(dt).itemsize])
    return rng.uniform(-4.0, 4.0, B).astype(dt), rng.uniform(-4.0, 4.0, B).astype(dt)


def al_case(B, K, Q, dt, seed=0):
    """K critics' outputs in [-8, 8] ([B] each for Q = 1 when `flat`, see al_flat), log-probs in [-4, 1]; planted: row 0 equal critics
    (the first index wins), row 1 the minimum in the last critic"""
    rng = np.random.default_rng([23, B, K, Q, seed])
    q = [rng.uniform(-8.0, 8.0, (B, Q)).astype(dt) for _ in range(K)]
    lp = rng.uniform(-4.0, 1.0, B).astype(dt)
    for k in range(K):
        q[k][0] = dt(1.25)
        if B > 1:
            q[k][1] = dt(-9.0) if k == K - 1 else dt(3.0 + k)
    return dict(q=q, lp=lp)


def al_flat(c):
    """the [B, 1] critics of an al_case with Q = 1 as [B] arrays: PTG_AL_MIN's form"""
    return [t[:, 0] for t in c["q"]]


# ------------------------------------------------------------------------------------------------- SB3's lines, typed out
def sb3_action_log_prob(mean, log_std, z, grad_act=None, grad_logp=None):
    """Actor.action_log_prob on float64 CPU tensors with the noise given: clamp, Normal(mean, std).log_prob of the pre-squash sample,
    the tanh correction; with incoming gradients also autograd's d / d mean and d / d log_std -> (act, logp, grad_mean, grad_log_std)"""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64).reshape(-1))
    mean_actions, ls_raw = t(mean).requires_grad_(True), t(log_std).requires_grad_(True)
    log_std_c = torch.clamp(ls_raw, LS_MIN, LS_MAX)
    action_std = torch.ones_like(mean_actions) * log_std_c.exp()
    dist = torch.distributions.Normal(mean_actions, action_std)
    gaussian_actions = mean_actions + action_std * t(z)                     # rsample with the noise given
    actions = torch.tanh(gaussian_actions)
    log_prob = dist.log_prob(gaussian_actions)
    log_prob = log_prob - torch.log(1 - actions ** 2 + 1e-6)
    gm = gs = None
    if grad_act is not None or grad_logp is not None:
        tot = 0.0
        if grad_act is not None:
            tot = tot + (actions * t(grad_act)).sum()
        if grad_logp is not None:
            tot = tot + (log_prob * t(grad_logp)).sum()
        tot.backward()
        gm, gs = mean_actions.grad.numpy(), ls_raw.grad.numpy()
    return actions.detach().numpy(), log_prob.detach().numpy(), gm, gs


def sb3_actor_lines(kind, q, lp=None, alpha=None):
    """the actor loss of SAC ("sac": q a list of K [B]), TQC ("tqc": K arrays [B, Q]) or TD3 ("td3": one [B]) on float64 CPU tensors
    -> (loss, [d loss / d q_k], d loss / d lp or None)"""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    qs = [t(x).requires_grad_(True) for x in q]
    log_prob = None if lp is None else t(lp).reshape(-1, 1).requires_grad_(True)
    if kind == "sac":
        q_values_pi = torch.cat([x.reshape(-1, 1) for x in qs], dim=1)
        min_qf_pi, _ = torch.min(q_values_pi, dim=1, keepdim=True)
        actor_loss = (alpha * log_prob - min_qf_pi).mean()
    elif kind == "tqc":
        quantiles = torch.stack(qs, dim=1)                                 # [B, K, Q]
        qf_pi = quantiles.mean(dim=2).mean(dim=1, keepdim=True)
        actor_loss = (alpha * log_prob - qf_pi).mean()
    else:
        actor_loss = -qs[0].reshape(-1, 1).mean()
    actor_loss.backward()
    return float(actor_loss.detach()), [x.grad.numpy() for x in qs], None if lp is None else log_prob.grad.numpy().reshape(-1)


def sb3_ent_coef_lines(lp, log_alpha, target_entropy):
    """-> (ent_coef_loss, d / d log_ent_coef, ent_coef = exp(log_ent_coef.detach()))"""
    import torch
    log_ent_coef = torch.tensor([float(log_alpha)], dtype=torch.float64, requires_grad=True)
    log_prob = torch.from_numpy(np.asarray(lp).astype(np.float64)).reshape(-1, 1)
    ent_coef = torch.exp(log_ent_coef.detach())
    ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
    ent_coef_loss.backward()
    return float(ent_coef_loss.detach()), float(log_ent_coef.grad[0]), float(ent_coef[0])
