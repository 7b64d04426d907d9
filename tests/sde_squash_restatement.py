"""ptg_sde_resample_rows / ptg_sde_rsample / ptg_sde_rsample_backward (include/ptg_env.h states the lines) restated in float64 NumPy
for tests/test_sde_squash_host.py and tests/test_sde_squash.py: SB3 2.0.0a13's StateDependentNoiseDistribution as sac/policies.py::Actor
builds it with use_sde (full_std, no expln, squash_output, learn_features, epsilon 1e-6, D = 1, Hardtanh(+-clip_mean) on the mean).
Operand order is the header's, and so is the order of the sums: unit k belongs to lane k mod 64, a lane adds its terms ascending in k
from 0.0, the 64 lane sums meet in the shuffle tree (offsets 32, 16, ..., 1); the batch sum of the log_std gradient runs per wave over
its rows ascending, the block's four waves in wave order, the blocks ascending.  Every reduced quantity comes with sum |term| so that a
test can put its tolerance on the sum's own scale.  The draw is act_restatement's (words, normal); sde_restatement gives the keys.
The second half builds the inputs the tests use and SB3's own expressions under torch autograd."""
import numpy as np

import sde_restatement as sr

HALF_LOG_2PI = sr.HALF_LOG_2PI
EPS = sr.EPS
TRAIN_SEED_XOR = 0x9E3779B97F4A7C15                          # rl_ptg_amd.sde: the training row's seed is the collecting seed XOR this
f64 = sr.f64


def resample_rows(log_std, seed, c, rows):
    """sde_restatement.resample without an env offset: row r, unit k takes the key r * 1024 + k"""
    return sr.resample(log_std, seed, c, rows, offset=0)


def wave_sum(terms):
    """[n, L] terms -> [n]: the kernel's sum over k (lane partials ascending from 0.0, then the xor tree)"""
    t = f64(terms)
    n, L = t.shape
    J = (L + 63) // 64
    pad = np.zeros((n, J * 64))
    pad[:, :L] = t
    pad = pad.reshape(n, J, 64)
    p = np.zeros((n, 64))
    for j in range(J):
        p = p + pad[:, j, :]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, idx ^ off]
    return p[:, 0]


def batch_sum(terms):
    """[B, L] terms -> [L]: the kernel's sum over the batch.  R = ceil(B / 4096) rows a wave; block b owns rows [4 R b, 4 R (b + 1));
    wave w adds rows 4 R b + w, + 4, ... from 0.0; the waves in wave order; the blocks ascending"""
    t = f64(terms)
    B, L = t.shape
    R = (B - 1) // 4096 + 1
    per = 4 * R
    nblk = (B - 1) // per + 1
    pad = np.zeros((nblk * per, L))
    pad[:B] = t
    pad = pad.reshape(nblk, R, 4, L)                        # row = 4 R b + 4 t + w
    acc = np.zeros((nblk, 4, L))
    for r in range(R):
        acc = acc + pad[:, r]
    blk = acc[:, 0]
    for w in range(1, 4):
        blk = blk + acc[:, w]
    s = blk[0]
    for b in range(1, nblk):
        s = s + blk[b]
    return s


def hardtanh(mu, c):
    return np.where(mu < -c, -c, np.where(mu > c, c, mu))


def forward(mean, latent, log_std, E=None, clip_mean=2.0, deterministic=False):
    """E: one shared row [L] or a matrix [B, L]; -> dict(act, step_act (act, 0 on bad rows: round it to float32), logp, saved [B, 2],
    bad [B], V, noise, abs_V, abs_noise, m, g, d, q)"""
    mu, h, ls = f64(mean).reshape(-1), f64(latent), f64(log_std).reshape(-1)
    B = mu.shape[0]
    with np.errstate(all="ignore"):
        s = np.exp(ls)
        tv = (h * h) * (s * s)[None, :]
        V, abs_V = wave_sum(tv) + EPS, np.abs(tv).sum(axis=1)
        if deterministic:
            noise, abs_noise = np.zeros(B), np.zeros(B)
        else:
            Em = f64(E)
            tn = h * (Em[None, :] if Em.ndim == 1 else Em)
            noise, abs_noise = wave_sum(tn), np.abs(tn).sum(axis=1)
        bad = ~np.isfinite(mu) | ~np.isfinite(h).all(axis=1) | ~np.isfinite(V) | ~np.isfinite(noise) | (np.isnan(ls) | (ls == np.inf)).any()
        m = hardtanh(mu, clip_mean)
        lsd = np.log(np.sqrt(V))
        g = m + noise
        a = np.tanh(g)
        d = 1.0 - a * a
        logp = ((((-(noise * noise)) / (2.0 * V)) - lsd) - HALF_LOG_2PI) - np.log(d + EPS)
        q = ((2.0 * a) * d) / (d + EPS)
    nan = lambda x: np.where(bad, np.nan, x)
    return dict(act=nan(a), step_act=np.where(bad, 0.0, a), logp=nan(logp), saved=np.stack([noise, V], axis=1), bad=bad, V=V, noise=noise,
                abs_V=abs_V, abs_noise=abs_noise, m=m, g=g, d=d, q=q)


def backward(mean, latent, log_std, E, saved, grad_act, grad_logp, clip_mean=2.0, deterministic=False):
    """E: the shared row [L], a matrix [B, L] or None (deterministic); saved [B, 2] = (noise, V) as the forward left them
    -> dict(grad_mean [B], grad_latent [B, L], grad_log_std [L], variance_path [L], matrix_path [L] (summed apart, NumPy's order),
    abs_gls [L] = sum_i |h_ik * grad_latent_ik|, bad [B], t, n, cV)"""
    mu, h, ls, sv = f64(mean).reshape(-1), f64(latent), f64(log_std).reshape(-1), f64(saved)
    B, L = h.shape
    ga = np.zeros(B) if grad_act is None else f64(grad_act).reshape(-1)
    gl = np.zeros(B) if grad_logp is None else f64(grad_logp).reshape(-1)
    noise, V = sv[:, 0], sv[:, 1]
    c = clip_mean
    with np.errstate(all="ignore"):
        s2 = np.exp(ls) * np.exp(ls)
        bad = (~np.isfinite(mu) | ~np.isfinite(h).all(axis=1) | ~np.isfinite(noise) | ~np.isfinite(V) | ~np.isfinite(ga) | ~np.isfinite(gl)
               | (np.isnan(ls) | (ls == np.inf)).any())
        a = np.tanh(hardtanh(mu, c) + noise)
        d = 1.0 - a * a
        q = ((2.0 * a) * d) / (d + EPS)
        t = ga * d + gl * q
        g_mu = np.where(bad, np.nan, np.where((-c < mu) & (mu < c), t, 0.0))
        n = np.where(bad, np.nan, t - gl * (noise / V))
        cV = np.where(bad, np.nan, (gl * (((noise * noise) / V) - 1.0)) / (2.0 * V))
        if deterministic or E is None:
            Em = np.zeros((1, L))
        else:
            Em = f64(E)
            Em = Em[None, :] if Em.ndim == 1 else Em
        g_lat = (n[:, None] * Em) + ((cV[:, None] * (2.0 * h)) * s2[None, :])
        terms = h * g_lat
        g_ls = batch_sum(terms)
        var_path = (2.0 * s2) * (cV[:, None] * (h * h)).sum(axis=0)
        mat_path = (Em[0] if Em.shape[0] == 1 else np.full(L, np.nan)) * (n[:, None] * h).sum(axis=0)
    return dict(grad_mean=g_mu, grad_latent=g_lat, grad_log_std=g_ls, variance_path=var_path, matrix_path=mat_path, abs_gls=np.abs(terms).sum(axis=0),
                bad=bad, t=t, n=n, cV=cV)


# ---------------------------------------------------------------------------------------------------- the tests' inputs
LS, NS, DTYPES, SEED = sr.LS, sr.NS, sr.DTYPES, sr.SEED
grid = sr.grid
CLIP_MEAN = 2.0
ENT_COEF = 0.2173


G_MAX = 4.0


def case(B, L, dtype, seed=0):
    """unclipped means in [-2.5, 2.5] (both sides of clip_mean = 2 and inside), latent = tanh-like values in (-1, 1), log_std in
    [-1.5, -0.5] - log(L) / 2, so that V is of the order 0.05 whatever L and |g| = |m + noise| stays below G_MAX = 4 (the tests assert
    it): there 1 - a^2 >= 1.3e-3, and two last places of tanh move log(1 - a^2 + 1e-6) by 4 * 2^-53 / 1.3e-3 = 3.3e-13, inside the 1e-12
    that tests/test_actor.py allows ptg_rsample on the same range.  The shared row E = s * z with z from a NumPy generator, cut at +-2.5
    (the op takes E as data), a matrix of B such rows, and incoming gradients: grad_logp = ent_coef / B, grad_act = -w / B with random
    w, what (ent_coef * logp - w * a).mean() sends back"""
    rng = np.random.default_rng([B, L, np.dtype(dtype).itemsize, 31, seed])
    ls = rng.uniform(-1.5, -0.5, L) - 0.5 * np.log(L)
    c = dict(mean=rng.uniform(-2.5, 2.5, B).astype(dtype), latent=np.tanh(rng.standard_normal((B, L))).astype(dtype), log_std=ls.astype(dtype))
    s = np.exp(c["log_std"].astype(np.float64))
    c["row"] = (s * np.clip(rng.standard_normal(L), -2.5, 2.5)).astype(dtype)
    c["matrix"] = (s[None, :] * np.clip(rng.standard_normal((B, L)), -2.5, 2.5)).astype(dtype)
    c["w"] = rng.standard_normal(B)
    c["grad_act"] = (-c["w"] / B).astype(dtype)
    c["grad_logp"] = np.full(B, ENT_COEF / B).astype(dtype)
    return c


def torch_reference(c, E, clip_mean=CLIP_MEAN, ent_coef=ENT_COEF, shared=True):
    """SB3's own expressions in float64 torch on the CPU, gradients by autograd (distributions.py: StateDependentNoiseDistribution with
    squash_output and learn_features, TanhBijector; sac/policies.py: Actor.action_log_prob).  The matrix row is weights_dist.rsample()
    = 0 + std * eps with the eps that makes it E, so the path from log_std through the row is autograd's.  log_prob(actions) goes the
    round trip atanh(clamp(tanh(g), +-(1 - eps64))).  Loss (ent_coef * logp - w * a).mean().
    -> dict(act, logp, grad_mean, grad_latent, grad_log_std)"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    mean_raw, latent = t(c["mean"]).reshape(-1, 1).requires_grad_(True), t(c["latent"]).requires_grad_(True)
    log_std = t(c["log_std"]).reshape(-1, 1).requires_grad_(True)
    B, L = latent.shape
    std = torch.exp(log_std)                                 # get_std: full_std, no expln
    weights_dist = torch.distributions.Normal(torch.zeros_like(std), std)
    if shared:
        eps = t(E).reshape(L, 1) / std.detach()
        exploration_mat = weights_dist.loc + weights_dist.scale * eps                      # rsample() with this eps: [L, 1]
    else:
        eps = t(E).reshape(B, L, 1) / std.detach().reshape(1, L, 1)
        exploration_matrices = weights_dist.loc.reshape(1, L, 1) + weights_dist.scale.reshape(1, L, 1) * eps      # rsample((B,)): [B, L, 1]
    mean_actions = F.hardtanh(mean_raw, -clip_mean, clip_mean) if np.isfinite(clip_mean) else mean_raw
    variance = torch.mm(latent ** 2, std ** 2)               # learn_features: latent not detached
    distribution = torch.distributions.Normal(mean_actions, torch.sqrt(variance + 1e-6))
    if shared:
        noise = torch.mm(latent, exploration_mat)            # get_noise, the mm branch
    else:
        noise = torch.bmm(latent.unsqueeze(dim=1), exploration_matrices).squeeze(dim=1)    # the bmm branch
    actions = torch.tanh(distribution.mean + noise)          # sample(): bijector.forward
    e64 = torch.finfo(torch.float64).eps
    y = actions.clamp(min=-1.0 + e64, max=1.0 - e64)         # TanhBijector.inverse
    gaussian_actions = 0.5 * (y.log1p() - (-y).log1p())
    log_prob = distribution.log_prob(gaussian_actions).sum(dim=-1)
    log_prob = log_prob - torch.sum(torch.log(1.0 - actions ** 2 + 1e-6), dim=1)
    loss = (ent_coef * log_prob - t(c["w"]) * actions[:, 0]).mean()
    loss.backward()
    n = lambda a: a.detach().numpy()
    return dict(act=n(actions)[:, 0], logp=n(log_prob), grad_mean=n(mean_raw.grad)[:, 0], grad_latent=n(latent.grad), grad_log_std=n(log_std.grad).reshape(-1))
