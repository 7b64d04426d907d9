"""ptg_sde_resample / ptg_sde_act / ptg_sde_policy_loss (include/ptg_env.h states the lines) restated in float64 NumPy for
tests/test_sde_host.py and tests/test_sde.py: SB3 2.0.0a13's StateDependentNoiseDistribution with its on-policy defaults (full_std,
no expln, no squashing, learn_features=False, epsilon 1e-6, D = 1).  The draw is act_restatement's (words, normal).  The advantage,
PPO / A2C, value and "means" lines are policy_loss_restatement's, which offers them only behind its own heads: lines() below types them
out as a function of a row's (lp, H), and tests/test_sde_host.py holds it to policy_loss_restatement.policy_loss bit for bit on that
module's Gaussian case.  Operand order is the header's; sums over k and over the batch are NumPy's, and every reduced quantity comes
with sum |term| so that a test can put its tolerance on the sum's own scale.
The second half builds the inputs the GPU tests use."""
import numpy as np

import act_restatement as ar
import policy_loss_restatement as plr

HALF_LOG_2PI = 0.9189385332046727
EPS = 1e-6
KEY_STRIDE = 1024                                            # PTG_MLP_MAX_WIDTH: the key of (e, k) does not depend on L


def f64(a):
    return np.asarray(a).astype(np.float64)


def keys(n, L, offset=0):
    """[n, L] uint64 keys of the rows with global env indices offset .. offset + n"""
    return (np.arange(offset, offset + n, dtype=np.uint64)[:, None] * np.uint64(KEY_STRIDE) + np.arange(L, dtype=np.uint64)[None, :])


def resample(log_std, seed, c, n, offset=0):
    """-> dict(E [n, L] float64, s [L], bad_cols [L] bool): E[e][k] = s_k * z(seed, c, (offset + e) * 1024 + k); a NaN or +Inf log_std makes
    its column NaN"""
    ls = f64(log_std).reshape(-1)
    L = ls.shape[0]
    w0, w1 = ar.words(seed, c, keys(n, L, offset).reshape(-1))
    z = ar.normal(w0, w1).reshape(n, L)
    bad = np.isnan(ls) | (ls == np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.exp(ls)
        E = np.where(bad[None, :], np.nan, s[None, :] * z)
    return dict(E=E, s=s, bad_cols=bad, z=z)


def variance(latent, log_std):
    """-> (V [n], sum |term| [n]): V = (sum_k (h_k * h_k) * (s_k * s_k)) + 1e-6"""
    h, ls = f64(latent), f64(log_std).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.exp(ls)
        terms = (h * h) * (s * s)[None, :]
        return terms.sum(axis=1) + EPS, np.abs(terms).sum(axis=1)


def act(mean, latent, log_std, E=None, clip=(-1.0, 1.0), deterministic=False):
    """-> dict(action (float64, clipped: round it to float32), raw, logp, entropy, bad [n], V, noise, abs_V, abs_noise)"""
    mu, h, ls = f64(mean).reshape(-1), f64(latent), f64(log_std).reshape(-1)
    n = mu.shape[0]
    bad = ~np.isfinite(mu) | ~np.isfinite(h).all(axis=1) | (np.isnan(ls) | (ls == np.inf)).any()
    with np.errstate(all="ignore"):
        V, abs_V = variance(h, ls)
        if deterministic:
            noise, abs_noise = np.zeros(n), np.zeros(n)
        else:
            t = h * f64(E)
            noise, abs_noise = t.sum(axis=1), np.abs(t).sum(axis=1)
        lsd = np.log(np.sqrt(V))
        g = mu + noise
        lo, hi = clip
        x = np.where(g < lo, lo, np.where(g > hi, hi, g))
        lp = ((-(noise * noise)) / (2.0 * V)) - lsd - HALF_LOG_2PI
        ent = 1.4189385332046727 + lsd
    nan = lambda a: np.where(bad, np.nan, a)
    return dict(action=np.where(bad, 0.0, x), raw=nan(g), logp=nan(lp), entropy=nan(ent), bad=bad, V=V, noise=noise, abs_V=abs_V, abs_noise=abs_noise)


def log_prob(mean, latent, log_std, actions):
    V, _ = variance(latent, log_std)
    d = f64(actions) - f64(mean).reshape(-1)
    return ((-(d * d)) / (2.0 * V)) - np.log(np.sqrt(V)) - HALF_LOG_2PI


def lines(kind, lp, H, head_bad, values, old_log_prob, advantages, returns, clip_range=0.0, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5,
          normalize_advantage=None, old_values=None):
    """policy_loss_restatement.policy_loss's lines behind the head, for rows with log-probability lp and entropy H -> dict(stats [8],
    grad_values, g [B] the surrogate's derivative, bad [B], abs_mean, margin)"""
    ppo = kind == "ppo"
    v, adv, ret = f64(values).reshape(-1), f64(advantages), f64(returns)
    B = v.shape[0]
    Bd = float(B)
    old = f64(old_log_prob) if ppo else np.zeros(B)
    clipv = clip_range_vf is not None
    ov = f64(old_values) if clipv else np.zeros(B)
    norm = (ppo if normalize_advantage is None else normalize_advantage) and B > 1
    bad = ~np.isfinite(v) | ~np.isfinite(adv) | ~np.isfinite(ret) | ~np.isfinite(old) | ~np.isfinite(ov) | head_bad | ~np.isfinite(lp)
    with np.errstate(all="ignore"):
        if ppo:
            d = lp - old
            r = np.exp(d)
            bad |= ~np.isfinite(r)
        mean, std = 0.0, 1.0
        if norm:
            mean = adv.mean()
            std = np.sqrt(((adv - mean) ** 2).sum() / (Bd - 1.0))
            ah = (adv - mean) / (std + 1e-8)
        else:
            ah = adv
        margin = np.inf
        if ppo:
            lo, hi = 1.0 - clip_range, 1.0 + clip_range
            c = np.where(r < lo, lo, np.where(r > hi, hi, r))
            t1, t2 = ah * r, ah * c
            surr = np.where(np.isnan(t1) | np.isnan(t2), np.nan, np.where(t2 < t1, t2, t1))
            g = np.where((t1 < t2) | ((r >= lo) & (r <= hi)), t1, 0.0)
            kl = (r - 1.0) - d
            cf = (np.abs(r - 1.0) > clip_range).astype(np.float64)
            if (~bad).any():
                margin = float(np.minimum(np.abs(r[~bad] - lo), np.abs(r[~bad] - hi)).min())
        else:
            surr, g, kl, cf = ah * lp, ah, np.zeros(B), np.zeros(B)
        if clipv:
            dv = v - ov
            vh = ov + np.where(dv < -clip_range_vf, -clip_range_vf, np.where(dv > clip_range_vf, clip_range_vf, dv))
            passes = (dv >= -clip_range_vf) & (dv <= clip_range_vf)
        else:
            vh, passes = v, np.ones(B, bool)
        dq = ret - vh
        q = dq * dq
        h = np.where(passes, 2.0 * (vh - ret), 0.0)
        terms = {k: np.where(bad, np.nan, t) for k, t in (("policy_loss", surr), ("value_loss", q), ("entropy_loss", H), ("approx_kl", kl), ("clip_fraction", cf))}
        pl, vl, el = -(terms["policy_loss"].sum() / Bd), terms["value_loss"].sum() / Bd, -(terms["entropy_loss"].sum() / Bd)
        stats = np.array([(pl + ent_coef * el) + vf_coef * vl, pl, vl, el, terms["approx_kl"].sum() / Bd, terms["clip_fraction"].sum() / Bd, mean, std])
    return dict(stats=stats, grad_values=np.where(bad, np.nan, (vf_coef * h) / Bd), g=g, bad=bad, margin=margin,
                abs_mean={k: float(np.abs(t[~bad]).mean()) if (~bad).any() else 0.0 for k, t in terms.items()})


def policy_loss(kind, mean, values, latent, log_std, actions, old_log_prob, advantages, returns, clip_range=0.0, clip_range_vf=None, ent_coef=0.0,
                vf_coef=0.5, normalize_advantage=None, old_values=None):
    """-> dict(stats [8], grad_input (d loss / d mean), grad_values, grad_log_std [L], grad_latent [B, L], bad [B], abs_mean: {name: mean
    |term|}, abs_V [B]: sum_k |term| of V, abs_gls [L]: sum_i |c_i * h_ik^2|, margin, c [B], V [B], g [B], d2V [B] = (d * d) / V: what a test needs to
    carry V's summation bound into the quantities behind it); gradients of bad rows are NaN"""
    mu, h, ls, a = f64(mean).reshape(-1), f64(latent), f64(log_std).reshape(-1), f64(actions)
    Bd = float(h.shape[0])
    with np.errstate(all="ignore"):
        V, abs_V = variance(h, ls)
        lsd = np.log(np.sqrt(V))
        d = a - mu
        lp = ((-(d * d)) / (2.0 * V)) - lsd - HALF_LOG_2PI
        H = 1.4189385332046727 + lsd
        ln = lines(kind, lp, H, ~np.isfinite(mu) | ~np.isfinite(V), values, old_log_prob, advantages, returns, clip_range, clip_range_vf, ent_coef, vf_coef,
                   normalize_advantage, old_values)
        g, bad = ln["g"], ln["bad"]
        c = np.where(bad, np.nan, (((-g) * (((d * d) / V) - 1.0)) - ent_coef) / (2.0 * V))
        s2 = np.exp(ls) * np.exp(ls)
        t = c[:, None] * (h * h)
        g_ls = ((2.0 * s2) * t.sum(axis=0)) / Bd
        g_lat = ((c[:, None] * (2.0 * h)) * s2[None, :]) / Bd
        g_mu = np.where(bad, np.nan, ((-g) * (d / V)) / Bd)
    return dict(stats=ln["stats"], grad_input=g_mu, grad_values=ln["grad_values"], grad_log_std=g_ls, grad_latent=g_lat,
                bad=bad, abs_mean=ln["abs_mean"], abs_V=abs_V, abs_gls=np.abs(t).sum(axis=0), margin=ln["margin"], c=c, V=V, g=g, d2V=(d * d) / V)


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
LS = [1, 2, 63, 64, 65, 127, 129, 233, 1024]
NS = [1, 3, 4, 5, 63, 65, 255, 256, 257, 513]
DTYPES = [np.float32, np.float64]
SEED = 0x5DE5EED0C0FFEE11
CLIP, CLIP_VF, ENT_COEF, VF_COEF = plr.CLIP, plr.CLIP_VF, plr.ENT_COEF, plr.VF_COEF
# PPO and A2C x normalise x clip_range_vf, as tests/test_policy_loss.py's CONFIGS
CONFIGS = [("ppo", True, None), ("ppo", True, CLIP_VF), ("ppo", False, None), ("ppo", False, CLIP_VF), ("a2c", False, None), ("a2c", True, None)]


def grid():
    """The thinned (n, L) grid of the sweeps, n a row count (N or B).  Every L meets n = 5 and n = 257 (one block and its ragged last
    wave; more than 256 rows: a second moment block), every n meets L = 65 (two units on lane 0, one elsewhere); beyond those two lines
    the diagonal pairs the i-th n with the i-th L.  31 of the 90 pairs."""
    pairs = {(n, 65) for n in NS} | {(5, L) for L in LS} | {(257, L) for L in LS} | {(NS[i], LS[i % len(LS)]) for i in range(len(NS))}
    return sorted(pairs)


def head_case(n, L, dtype, seed=0):
    """means in [-1, 1], latent = tanh-like values in (-1, 1) [n, L] (what a Tanh policy leaves), log_std in [-3, -1] [L]"""
    rng = np.random.default_rng([n, L, np.dtype(dtype).itemsize, 23, seed])
    return dict(mean=rng.uniform(-1.0, 1.0, n).astype(dtype), latent=np.tanh(rng.standard_normal((n, L))).astype(dtype),
                log_std=rng.uniform(-3.0, -1.0, L).astype(dtype))


def loss_case(B, L, dtype, seed=0):
    """a minibatch: head_case plus stored samples a = mu + sd * z, old_log_prob = lp - delta with delta in [-0.5, 0.5] (ratios on both
    clip sides and inside at eps = 0.2), advantages, returns, values and old values with differences inside and outside eps_v = 0.3"""
    c = head_case(B, L, dtype, seed)
    rng = np.random.default_rng([B, L, np.dtype(dtype).itemsize, 29, seed])
    V, _ = variance(c["latent"], c["log_std"])
    c["actions"] = (c["mean"].astype(np.float64) + np.sqrt(V) * rng.standard_normal(B)).astype(dtype)
    lp = log_prob(c["mean"], c["latent"], c["log_std"], c["actions"])
    c["old_log_prob"] = (lp - rng.uniform(-0.5, 0.5, B)).astype(dtype)
    ov = rng.standard_normal(B)
    c["advantages"] = rng.standard_normal(B).astype(dtype)
    c["returns"] = (ov + rng.standard_normal(B)).astype(dtype)
    c["values"] = (ov + rng.uniform(-0.6, 0.6, B)).astype(dtype)
    c["old_values"] = ov.astype(dtype)
    return c


def loss_kwargs(kind, norm, cvf):
    kw = dict(ent_coef=ENT_COEF, vf_coef=VF_COEF, normalize_advantage=norm, clip_range_vf=cvf)
    if kind == "ppo":
        kw["clip_range"] = CLIP
    return kw


def torch_reference(kind, c, clip_range=CLIP, clip_range_vf=None, ent_coef=ENT_COEF, vf_coef=VF_COEF, normalize_advantage=None):
    """SB3's own expressions in float64 torch on the CPU, gradients by autograd: Normal(mean, sqrt((latent ** 2) @ (exp(log_std) ** 2) +
    1e-6)), log_prob and entropy (distributions.py), then policy_loss_restatement.torch_reference's loss lines (ppo.py / a2c.py)
    -> dict(stats [6], grad_input, grad_values, grad_log_std [L], grad_latent [B, L])"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    mean, values = t(c["mean"]).requires_grad_(True), t(c["values"]).requires_grad_(True)
    latent, log_std = t(c["latent"]).requires_grad_(True), t(c["log_std"]).reshape(-1, 1).requires_grad_(True)
    advantages, returns = t(c["advantages"]), t(c["returns"])
    std = torch.exp(log_std)
    variance_ = torch.mm(latent ** 2, std ** 2)
    dist = torch.distributions.Normal(mean.reshape(-1, 1), torch.sqrt(variance_ + 1e-6))
    log_prob_, entropy = dist.log_prob(t(c["actions"]).reshape(-1, 1)).sum(dim=1), dist.entropy().sum(dim=1)
    ppo = kind == "ppo"
    if (ppo if normalize_advantage is None else normalize_advantage) and len(advantages) > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    kl = cf = torch.zeros((), dtype=torch.float64)
    if ppo:
        ratio = torch.exp(log_prob_ - t(c["old_log_prob"]))
        policy_loss_ = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
        cf = torch.mean((torch.abs(ratio - 1) > clip_range).double())
        log_ratio = log_prob_ - t(c["old_log_prob"])
        kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
    else:
        policy_loss_ = -(advantages * log_prob_).mean()
    values_pred = values if clip_range_vf is None else t(c["old_values"]) + torch.clamp(values - t(c["old_values"]), -clip_range_vf, clip_range_vf)
    value_loss = F.mse_loss(returns, values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss_ + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    n = lambda a: a.detach().numpy()
    return dict(stats=np.array([n(a_).item() for a_ in (loss, policy_loss_, value_loss, entropy_loss, kl, cf)]), grad_input=n(mean.grad),
                grad_values=n(values.grad), grad_log_std=n(log_std.grad).reshape(-1), grad_latent=n(latent.grad))
