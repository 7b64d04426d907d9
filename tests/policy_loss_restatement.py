"""ptg_policy_loss (include/ptg_env.h states the lines) restated in float64 NumPy for tests/test_policy_loss_host.py and
tests/test_policy_loss.py: SB3 2.0.0a13's evaluate_actions and the loss lines of PPO.train / A2C.train with the closed-form
gradients with respect to the logits (or means), the values and log_std.  Operand order is the header's; sums are NumPy's (the
tests' tolerance for a mean covers any order).  Besides the results it returns what the tolerances need: mean_i |term_i| of every
mean and the smallest distance of a PPO ratio from 1 - eps or 1 + eps.
The second half builds the inputs the GPU tests use, so that the host test can vet them."""
import numpy as np

HALF_LOG_2PI = 0.9189385332046727
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")


def _categorical(l, act):
    """-> lp [B], H [B], p [B, A], logp [B, A], e [B, A], bad [B] (row maximum not finite), oob [B] (action outside [0, A))"""
    B, A = l.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = l.max(axis=1)
        bad = ~np.isfinite(m)
        d = l - m[:, None]
        e = np.exp(d)
        s = np.zeros(B)
        for j in range(A):                                   # s = e_0 + e_1 + ... in index order
            s = s + e[:, j]
        logp = d - np.log(s)[:, None]
        ent = np.zeros(B)
        for j in range(A):
            ent = np.where(e[:, j] != 0, ent + (e[:, j] / s) * logp[:, j], ent)
        p = e / s[:, None]
    oob = (act < 0) | (act >= A)
    lp = logp[np.arange(B), np.where(oob, 0, act)]
    return lp, -ent, p, logp, e, bad, oob


def policy_loss(kind, head_input, values, actions, old_log_prob, advantages, returns, clip_range=0.0, clip_range_vf=None, ent_coef=0.0,
                vf_coef=0.5, normalize_advantage=None, old_values=None, log_std=None):
    """-> dict(stats [8], grad_input, grad_values, grad_log_std (Gaussian), bad, oob [B] bool, abs_mean: {name: mean |term|},
    margin: smallest |r - (1 -+ eps)| over the good rows (inf for A2C)).  Gradients of oob rows are NaN here and must be ignored
    (the kernel leaves them untouched); gradients of bad rows are NaN as the kernel's are."""
    ppo = kind == "ppo"
    f = lambda a: np.asarray(a).astype(np.float64)
    x, v, adv, ret = f(head_input), f(values).reshape(-1), f(advantages), f(returns)
    B = v.shape[0]
    Bd = float(B)
    old = f(old_log_prob) if ppo else np.zeros(B)
    clipv = clip_range_vf is not None
    ov = f(old_values) if clipv else np.zeros(B)
    gauss = log_std is not None
    norm = (ppo if normalize_advantage is None else normalize_advantage) and B > 1
    bad = ~np.isfinite(v) | ~np.isfinite(adv) | ~np.isfinite(ret) | ~np.isfinite(old) | ~np.isfinite(ov)
    with np.errstate(all="ignore"):
        if gauss:
            mu, ls, a = x.reshape(-1), float(np.asarray(log_std).astype(np.float64).reshape(-1)[0]), f(actions)
            oob = np.zeros(B, bool)
            bad |= ~np.isfinite(mu) | np.isnan(ls) | (ls == np.inf)
            sigma = np.exp(ls)
            z = (a - mu) / sigma
            lp = ((-(z * z) / 2.0) - ls) - HALF_LOG_2PI
            H = np.full(B, 1.4189385332046727 + ls)
        else:
            act = np.asarray(actions).astype(np.int64)
            lp, H, p, logp, e, bad_row, oob = _categorical(x, act)
            bad |= bad_row
        bad |= ~np.isfinite(lp)
        if ppo:
            d = lp - old
            r = np.exp(d)
            bad |= ~np.isfinite(r)                           # a ratio that overflows
        bad &= ~oob
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
            ok = ~bad & ~oob
            if ok.any():
                margin = float(np.minimum(np.abs(r[ok] - lo), np.abs(r[ok] - hi)).min())
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
        poison = bad | oob
        terms = {k: np.where(poison, np.nan, t) for k, t in (("policy_loss", surr), ("value_loss", q), ("entropy_loss", H), ("approx_kl", kl), ("clip_fraction", cf))}
        pl, vl, el = -(terms["policy_loss"].sum() / Bd), terms["value_loss"].sum() / Bd, -(terms["entropy_loss"].sum() / Bd)
        stats = np.array([(pl + ent_coef * el) + vf_coef * vl, pl, vl, el, terms["approx_kl"].sum() / Bd, terms["clip_fraction"].sum() / Bd, mean, std])
        gv = np.where(poison, np.nan, (vf_coef * h) / Bd)
        out = dict(stats=stats, grad_values=gv, bad=bad, oob=oob, margin=margin, ratio=r if ppo else None,
                   abs_mean={k: float(np.abs(t[~poison]).mean()) if (~poison).any() else 0.0 for k, t in terms.items()})
        if gauss:
            out["grad_input"] = np.where(poison, np.nan, ((-g) * (z / sigma)) / Bd)
            out["grad_log_std"] = (-(np.where(poison, np.nan, g * ((z * z) - 1.0)).sum()) / Bd) - ent_coef
        else:
            onehot = (np.arange(x.shape[1])[None, :] == np.where(oob, -1, act)[:, None]).astype(np.float64)
            gr = (-g)[:, None] * (onehot - p)
            gr = np.where(e != 0, gr + ent_coef * (p * (logp + H[:, None])), gr)
            out["grad_input"] = np.where(poison[:, None], np.nan, gr / Bd)
    return out


def log_prob(head_input, actions, log_std=None):
    """the log-probability the restatement gives the actions (what a collect step would have stored as old_log_prob)"""
    x = np.asarray(head_input).astype(np.float64)
    if log_std is None:
        return _categorical(x, np.asarray(actions).astype(np.int64))[0]
    ls = float(np.asarray(log_std).astype(np.float64).reshape(-1)[0])
    z = (np.asarray(actions).astype(np.float64) - x.reshape(-1)) / np.exp(ls)
    return ((-(z * z) / 2.0) - ls) - HALF_LOG_2PI


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
BS = [1, 2, 63, 64, 65, 203, 257, 4097]
AS = [2, 5, 32]
DTYPES = [np.float32, np.float64]
B_BIG = 70001             # 274 blocks of 256 rows: k_loss_final's 256 threads each walk two partials (blocks t and t + 256: one lap boundary),
#                           and k_vn_merge's 64 lanes five moment partials each (laps at 64, 128, 192, 256 blocks)
CLIP, CLIP_VF, ENT_COEF, VF_COEF = 0.2, 0.3, 0.01, 0.5


def case(B, A, dtype, seed=0):
    """dict of host arrays for a categorical minibatch: logits uniform in [-8, 8] [B, A], values, actions, old_log_prob, advantages,
    returns, old_values in dtype.  old_log_prob = lp - delta with delta uniform in [-0.5, 0.5], so the ratios exp(delta) lie in
    [0.6, 1.65]: both clip sides and the inside are populated at eps = 0.2.  Planted rows (those that fit B): 0 all logits equal;
    1 a -Inf logit on a column that was not chosen; 2 underflow everywhere but the chosen maximum; 3 advantage exactly 0; 4 ratio
    exactly 1 (an underflow row, whose lp is exactly 0, with old = 0: exact in float32 too); 5 / 6 clipped above (ratio e^0.4) with
    advantage > 0 / < 0; 7 / 8 clipped below (e^-0.4) with advantage > 0 / < 0; 9 value difference inside +-eps_v = 0.3; 10 / 11
    outside it on either side."""
    rng = np.random.default_rng([B, A, np.dtype(dtype).itemsize, seed])
    x = rng.uniform(-8.0, 8.0, (B, A)).astype(dtype)
    act = rng.integers(0, A, B)
    if B > 0:
        x[0] = dtype(1.25)
    if B > 1:
        x[1, (act[1] + 1) % A] = -np.inf
    if B > 2:
        x[2] = dtype(-800.0); act[2] = A - 1; x[2, A - 1] = dtype(2.0)
    if B > 4:
        x[4] = dtype(-800.0); act[4] = 0; x[4, 0] = dtype(3.0)
    lp = log_prob(x, act)
    delta = rng.uniform(-0.5, 0.5, B)
    adv = rng.standard_normal(B)
    for r_, dl, sgn in ((5, 0.4, 1.0), (6, 0.4, -1.0), (7, -0.4, 1.0), (8, -0.4, -1.0)):
        if B > r_:
            delta[r_] = dl
            adv[r_] = sgn * (0.5 + abs(adv[r_]))
    if B > 3:
        adv[3] = 0.0
    if B > 4:
        delta[4] = 0.0
    old = (lp - delta).astype(dtype)
    ov = rng.standard_normal(B)
    dv = rng.uniform(-0.6, 0.6, B)
    for r_, val in ((9, 0.1), (10, 0.5), (11, -0.5)):
        if B > r_:
            dv[r_] = val
    return dict(logits=x, actions=act.astype(np.int64), old_log_prob=old, advantages=adv.astype(dtype), returns=(ov + rng.standard_normal(B)).astype(dtype),
                values=(ov + dv).astype(dtype), old_values=ov.astype(dtype))


def ratio_one_rows(c):
    """rows of a case whose stored old log-prob equals the restatement's lp bit for bit (ratio exactly 1): the planted row 4"""
    lp = log_prob(c["logits"], c["actions"])
    return np.nonzero(c["old_log_prob"].astype(np.float64) == lp)[0]


def gaussian_case(B, dtype, seed=0):
    rng = np.random.default_rng([B, np.dtype(dtype).itemsize, 7, seed])
    mean = rng.uniform(-1.0, 1.0, B).astype(dtype)
    ls = np.array([-0.7], dtype)
    a = (mean.astype(np.float64) + np.exp(-0.7) * rng.standard_normal(B)).astype(dtype)
    lp = log_prob(mean, a, ls)
    old = (lp - rng.uniform(-0.5, 0.5, B)).astype(dtype)
    ov = rng.standard_normal(B)
    return dict(mean=mean, log_std=ls, actions=a, old_log_prob=old, advantages=rng.standard_normal(B).astype(dtype),
                returns=(ov + rng.standard_normal(B)).astype(dtype), values=(ov + rng.uniform(-0.6, 0.6, B)).astype(dtype), old_values=ov.astype(dtype))


def torch_reference(kind, c, A=None, clip_range=CLIP, clip_range_vf=None, ent_coef=ENT_COEF, vf_coef=VF_COEF, normalize_advantage=None, device="cpu"):
    """SB3's own lines (distributions.py log_prob / entropy, ppo.py / a2c.py train) typed out in float64 torch on leaf tensors;
    -> dict(stats [6] np, grad_input, grad_values, grad_log_std) by autograd"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64)).to(device)
    gauss = "mean" in c
    x = t(c["mean"] if gauss else c["logits"]).requires_grad_(True)
    values = t(c["values"]).requires_grad_(True)
    advantages, returns = t(c["advantages"]), t(c["returns"])
    if gauss:
        log_std = t(c["log_std"]).requires_grad_(True)
        dist = torch.distributions.Normal(x, torch.ones_like(x) * log_std.exp())
        log_prob_, entropy = dist.log_prob(t(c["actions"])), dist.entropy()
    else:
        dist = torch.distributions.Categorical(logits=x)
        log_prob_, entropy = dist.log_prob(torch.from_numpy(c["actions"]).to(device)), dist.entropy()
    ppo = kind == "ppo"
    if (ppo if normalize_advantage is None else normalize_advantage) and len(advantages) > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    kl = cf = torch.zeros((), dtype=torch.float64)
    if ppo:
        ratio = torch.exp(log_prob_ - t(c["old_log_prob"]))
        policy_loss_1 = advantages * ratio
        policy_loss_2 = advantages * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
        policy_loss_ = -torch.min(policy_loss_1, policy_loss_2).mean()
        cf = torch.mean((torch.abs(ratio - 1) > clip_range).double())
        log_ratio = log_prob_ - t(c["old_log_prob"])
        kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
    else:
        policy_loss_ = -(advantages * log_prob_).mean()
    if clip_range_vf is None:
        values_pred = values
    else:
        values_pred = t(c["old_values"]) + torch.clamp(values - t(c["old_values"]), -clip_range_vf, clip_range_vf)
    value_loss = F.mse_loss(returns, values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss_ + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    n = lambda a: a.detach().cpu().numpy()
    return dict(stats=np.array([n(a_).item() for a_ in (loss, policy_loss_, value_loss, entropy_loss, kl, cf)]),
                grad_input=n(x.grad), grad_values=n(values.grad), grad_log_std=n(log_std.grad) if gauss else None)
