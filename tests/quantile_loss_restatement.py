"""ptg_quantile_loss (include/ptg_env.h states the lines) restated in float64 NumPy for tests/test_quantile_loss_host.py and
tests/test_quantile_loss.py: the critic lines of sb3_contrib's TQC.train -- the sort over the target critics' quantiles, the drop of
the top d per net, the entropy term, the TD targets -- and quantile_huber_loss(sum_over_quantiles=False) with the closed-form
gradients with respect to the current quantiles.  Vectorised over (b, k, i) with a Python loop over the targets j, so the j order and
the operand order are the header's and the per-row outputs (y and the gradients) are the kernel's bit for bit; sums are NumPy's (the
tests' tolerance for a mean covers any order).  Besides the results it returns the bad-row classification and mean |term| and the
number of summands of every mean, which the tolerances need.
The second half builds the inputs the GPU tests use, so that the host test can vet them."""
import numpy as np

GAMMA, ALPHA = 0.9639, 0.00047                        # the reference's config/config_agent.yaml (TQC)
SHAPES = [(1, 1, 0), (2, 30, 2), (2, 25, 2), (3, 33, 5), (4, 64, 0), (1, 64, 63)]      # (K, Q, d): the reference's, SB3's defaults, the edges
DTYPES = [np.float32, np.float64]


def _f(a):
    return np.asarray(a).astype(np.float64)


def stack(x):
    """a [B, K, Q] array or a list of K [B, Q] arrays -> [B, K, Q] float64"""
    return np.stack([_f(t) for t in x], axis=1) if isinstance(x, (list, tuple)) else _f(x)


def quantile_loss(quantiles, next_quantiles, rewards, dones, next_log_prob, gamma, drop, alpha):
    """alpha: the entropy coefficient AS USED (the caller takes np.exp of a log alpha, or the kernel's stats[5]).
    -> dict(stats [8], grad [B, K, Q], y [B, M], bad [B] bool, abs_mean {name: mean |term|}, count {name: summands}).  A bad row has NaN
    gradients and its y as computed, as in the kernel."""
    cur, nxt = stack(quantiles), stack(next_quantiles)
    r, dn, lp = _f(rewards).reshape(-1), _f(dones).reshape(-1), _f(next_log_prob).reshape(-1)
    B, K, Q = cur.shape
    M = K * (Q - drop)
    a_used = float(alpha)
    with np.errstate(all="ignore"):
        s = np.sort(nxt.reshape(B, K * Q), axis=1, kind="stable")[:, :M]       # NaN last, as torch.sort; equal values keep their flat order
        t = s - (a_used * lp)[:, None]
        y = r[:, None] + ((1.0 - dn) * gamma)[:, None] * t
        tau = ((np.arange(Q, dtype=np.float64) + 0.5) / float(Q))[None, None, :]
        acc, ls, ad, gt = np.zeros((B, K, Q)), np.zeros((B, K, Q)), np.zeros((B, K, Q)), np.zeros((B, K, Q))
        for j in range(M):
            dl = y[:, j][:, None, None] - cur
            ab = np.abs(dl)
            w = np.abs(tau - np.where(dl < 0.0, 1.0, 0.0))
            h = np.where(ab > 1.0, ab - 0.5, 0.5 * (dl * dl))
            c = np.where(dl < -1.0, -1.0, np.where(dl > 1.0, 1.0, dl))
            acc = acc + w * c
            ls = ls + w * h
            ad = ad + ab
            gt = gt + (ab > 1.0)
        n = ((float(B) * float(K)) * float(Q)) * float(M)
        bad = ~np.isfinite(y).all(axis=1) | ~np.isfinite(cur).all(axis=(1, 2))
        grad = (-acc) / n
        grad[bad] = np.nan
        poison = lambda x: np.where(bad.reshape((B,) + (1,) * (x.ndim - 1)), np.nan, x).sum()
        stats = np.array([poison(ls) / n, poison(cur) / ((float(B) * float(K)) * float(Q)), poison(y) / (float(B) * float(M)), poison(ad) / n,
                          poison(gt) / n, a_used, 0.0, 0.0])
        ok = ~bad
        am = lambda x, per=1.0: float(np.abs(x[ok]).mean() / per) if ok.any() else 0.0
    return dict(stats=stats, grad=grad, y=y, bad=bad,
                abs_mean=dict(loss=am(ls, float(M)), q=am(cur), y=am(y), abs_delta=am(ad, float(M))),
                count=dict(loss=n, q=float(B * K * Q), y=float(B * M), abs_delta=n))


# ------------------------------------------------------------------------------------------------- the inputs of the tests
BS = [1, 2, 3, 4, 5, 8, 9, 290, 1029]                 # the one-block edge (4 | 5), the block edges, the reference batch, 258 partials
GPU_SHAPES = SHAPES + [(2, 32, 0)]                    # exactly 64 pairs
PLANTED = ("delta = 0", "delta = -1", "delta = +1", "|delta| just above 1", "|delta| just below 1", "|delta| just above 1, the other sign",
           "equal next quantiles across the critics", "done = 1", "a NaN among the dropped tops", "a +Inf among the dropped tops")


def case(B, K, Q, drop, dt, seed=0, rdt=np.float32, ddt=np.float32):
    """quantiles in [-3, 3], rewards in [-3, 3], log-probs in [-4, 1], about a tenth of the rows done, and the PLANTED rows (as many as
    fit): rows 0 .. 5 are done with r = 0.5 -- every y_j is 0.5 exactly: (1 - 1) * gamma * t_j = 0 -- and their first current quantile is
    0.5 - delta; row 6 gives every critic the same next quantiles; row 7 is done; rows 8 and 9 (when something is dropped) hold a NaN /
    a +Inf that the sort must put among the dropped tops"""
    rng = np.random.default_rng([17, B, K, Q, drop, seed])
    cur = rng.uniform(-3, 3, (B, K, Q)).astype(dt)
    nxt = rng.uniform(-3, 3, (B, K, Q)).astype(dt)
    lp = rng.uniform(-4, 1, B).astype(dt)
    r = rng.uniform(-3, 3, B).astype(rdt)
    d = (rng.random(B) < 0.1).astype(ddt)
    one = dt(1.5)
    vals = [dt(0.5), one, dt(-0.5), np.nextafter(one, dt(2)), np.nextafter(one, dt(1)), np.nextafter(dt(-0.5), dt(-1))]
    for i, v in enumerate(vals):
        if i < B:
            cur[i, 0, 0] = v
            r[i], d[i] = 0.5, 1.0
    if 6 < B:
        d[6] = 0.0
        nxt[6] = nxt[6, 0]
    if 7 < B:
        d[7] = 1.0
    if drop > 0:
        if 8 < B:
            d[8] = 0.0
            nxt[8, K - 1, Q // 2] = np.nan
        if 9 < B:
            d[9] = 0.0
            nxt[9, 0, 0] = np.inf
    return dict(quantiles=cur, next_quantiles=nxt, next_log_prob=lp, rewards=r, dones=d)


def sb3_tqc_lines(c, gamma, alpha, drop, device="cpu"):
    """sb3_contrib's TQC.train critic lines and quantile_huber_loss(sum_over_quantiles=False) typed out on float64 tensors, cum_prob
    in float64 -> (loss, d loss / d quantiles [B, K, Q], y [B, M])"""
    import torch as th
    t = lambda a: th.from_numpy(np.asarray(a).astype(np.float64)).to(device)
    current_quantiles = t(c["quantiles"]).requires_grad_(True)
    batch_size, n_critics, n_quantiles = current_quantiles.shape
    n_target_quantiles = n_critics * n_quantiles - drop * n_critics
    loss, target_quantiles = tqc_lines(th, current_quantiles, t(c["next_quantiles"]), t(c["rewards"]).reshape(-1, 1), t(c["dones"]).reshape(-1, 1),
                                       t(c["next_log_prob"]), gamma, alpha, n_target_quantiles)
    loss.backward()
    return float(loss.detach()), current_quantiles.grad.cpu().numpy(), target_quantiles.cpu().numpy().reshape(batch_size, -1)


def tqc_lines(th, current_quantiles, next_quantiles, rewards, dones, next_log_prob, gamma, ent_coef, n_target_quantiles):
    """the lines themselves, on tensors of any device -> (critic_loss, target_quantiles [B, 1, M])"""
    with th.no_grad():
        batch_size = next_quantiles.shape[0]
        next_quantiles, _ = th.sort(next_quantiles.reshape(batch_size, -1))
        next_quantiles = next_quantiles[:, :n_target_quantiles]
        target_quantiles = next_quantiles - ent_coef * next_log_prob.reshape(-1, 1)
        target_quantiles = rewards + (1 - dones) * gamma * target_quantiles
        target_quantiles = target_quantiles.unsqueeze(dim=1)
    # quantile_huber_loss(current_quantiles, target_quantiles, sum_over_quantiles=False)
    n_quantiles = current_quantiles.shape[-1]
    cum_prob = (th.arange(n_quantiles, device=current_quantiles.device, dtype=th.float64) + 0.5) / n_quantiles
    cum_prob = cum_prob.view(1, 1, -1, 1)
    pairwise_delta = target_quantiles.unsqueeze(-2) - current_quantiles.unsqueeze(-1)
    abs_pairwise_delta = th.abs(pairwise_delta)
    huber_loss = th.where(abs_pairwise_delta > 1, abs_pairwise_delta - 0.5, pairwise_delta ** 2 * 0.5)
    loss = th.abs(cum_prob - (pairwise_delta.detach() < 0).double()) * huber_loss
    return loss.mean(), target_quantiles
