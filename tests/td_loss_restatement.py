"""ptg_td_loss (include/ptg_env.h states the lines) restated in float64 NumPy for tests/test_td_loss_host.py and
tests/test_td_loss.py: the TD target and the loss lines of SB3 2.0.0a13's DQN.train, TD3.train and SAC.train with the closed-form
gradients with respect to the current Q-values.  Operand order is the header's, so the per-row outputs (y and the gradients) are the
kernel's bit for bit; sums are NumPy's (the tests' tolerance for a mean covers any order).  Besides the results it returns the
bad-row classification and mean_i |term_i| of every mean, which the tolerances need.
The second half builds the inputs the GPU tests use, so that the host test can vet them."""
import numpy as np

STAT_NAMES = ("loss", "q", "y", "abs_delta", "share_ge_1", "alpha")
GAMMA = {"dqn": 0.9728, "td3": 0.9595, "sac": 0.9628}           # the reference's config/config_agent.yaml
SCALE = {"td3": 1.0, "sac": 0.5}


def _f(a):
    return np.asarray(a).astype(np.float64)


def td_loss(kind, q, next_q, rewards, dones, gamma, actions=None, next_log_prob=None, alpha=None):
    """kind "dqn": q, next_q [B, A]; "td3" / "sac": lists of K arrays [B].  alpha: SAC's entropy coefficient AS USED (the caller takes
    np.exp of a log alpha, or the kernel's stats[5]).
    -> dict(stats [8], grad_q ([B, A], or a list of K [B]), y [B], bad, oob [B] bool, abs_mean {name: mean |term|}, delta).  Of an oob
    row (action outside [0, A)) gradients and y are NaN here and must be ignored: the kernel leaves them untouched.  A bad row has
    NaN gradients and its y as computed, as in the kernel."""
    r, d = _f(rewards).reshape(-1), _f(dones).reshape(-1)
    B = r.shape[0]
    Bd = float(B)
    with np.errstate(all="ignore"):
        if kind == "dqn":
            x, nx = _f(q), _f(next_q)
            A = x.shape[1]
            act = np.asarray(actions).astype(np.int64)
            m = nx[:, 0]
            for j in range(1, A):
                l = nx[:, j]
                m = np.where((l > m) | np.isnan(l), l, m)
            y = r + ((1.0 - d) * gamma) * m
            oob = (act < 0) | (act >= A)
            safe = np.where(oob, 0, act)
            qa = x[np.arange(B), safe]
            bad = (~np.isfinite(y) | ~np.isfinite(qa)) & ~oob
            poison = bad | oob
            dl = qa - y
            ad = np.abs(dl)
            term = np.where(ad < 1.0, 0.5 * (dl * dl), ad - 0.5)
            gc = np.where(dl < -1.0, -1.0, np.where(dl > 1.0, 1.0, dl)) / Bd
            grad = np.zeros((B, A))
            grad[np.arange(B), safe] = gc
            grad[poison] = np.nan
            n = Bd
            sums = [np.where(poison, np.nan, t).sum() for t in (term, qa, y, ad, (ad >= 1.0).astype(np.float64))]
            stats = np.array([sums[0] / Bd, sums[1] / n, sums[2] / Bd, sums[3] / n, sums[4] / n, 0.0, 0.0, 0.0])
            ok = ~poison
            am = lambda t: float(np.abs(t[ok]).mean()) if ok.any() else 0.0
            return dict(stats=stats, grad_q=grad, y=np.where(oob, np.nan, y), bad=bad, oob=oob, delta=dl,
                        abs_mean=dict(loss=am(term), q=am(qa), y=am(y), abs_delta=am(ad)))
        c = SCALE[kind]
        xs, nxs = [_f(t).reshape(-1) for t in q], [_f(t).reshape(-1) for t in next_q]
        K = len(xs)
        m = nxs[0]
        for k in range(1, K):
            l = nxs[k]
            m = np.where((l < m) | np.isnan(l), l, m)
        a_used = 0.0
        if kind == "sac":
            a_used = float(alpha)
            m = m - a_used * _f(next_log_prob).reshape(-1)
        y = r + ((1.0 - d) * gamma) * m
        bad = ~np.isfinite(y)
        for k in range(K):
            bad = bad | ~np.isfinite(xs[k])
        term, sq, sad, sge = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
        grads, deltas = [], []
        c2 = c * 2.0
        for k in range(K):
            dl = xs[k] - y
            ad = np.abs(dl)
            grads.append(np.where(bad, np.nan, (c2 * dl) / Bd))
            term = term + dl * dl
            sq = sq + xs[k]
            sad = sad + ad
            sge = sge + (ad >= 1.0).astype(np.float64)
            deltas.append(dl)
        n = Bd * float(K)
        sums = [np.where(bad, np.nan, t).sum() for t in (term, sq, y, sad, sge)]
        stats = np.array([(c * sums[0]) / Bd, sums[1] / n, sums[2] / Bd, sums[3] / n, sums[4] / n, a_used, 0.0, 0.0])
        ok = ~bad
        am = lambda t, by=1.0: float(np.abs(t[ok]).mean() / by) if ok.any() else 0.0
        return dict(stats=stats, grad_q=grads, y=y, bad=bad, oob=np.zeros(B, bool), delta=deltas,
                    abs_mean=dict(loss=am(c * term), q=float(np.mean([am(t) for t in xs])), y=am(y), abs_delta=am(sad, float(K))))


# ------------------------------------------------------------------------------------------------- the inputs of the tests
BS = [1, 2, 63, 64, 65, 255, 256, 257, 544, 4097]     # the wave edges, the edge between the one- and the two-launch route, a ragged last block
B_BIG = 70001                                         # 274 blocks: the final pass crosses a lap of 256 partials
AS = [2, 5, 32]
KS = [1, 2, 4]
DTYPES = [np.float32, np.float64]
PLANTED = ("delta = 0", "delta = +1", "delta = -1", "delta just above 1", "delta just below 1", "delta just below -1", "a tie in the extremum",
           "done = 1")


def _plant(qcol, nq_cols, r, d, dt):
    """rows 0 .. 7 (as many as fit) made what PLANTED says: rows 0 .. 5 are done (y = r = 0.5 exactly: (1 - 1) * gamma * m = 0) with the
    current Q at 0.5 + delta; row 6 has two equal next-Q extremes; row 7 is done.  qcol: the column of the current Q that the row reads"""
    B = r.shape[0]
    one = dt(1.5)
    vals = [dt(0.5), one, dt(-0.5), np.nextafter(one, dt(2)), np.nextafter(one, dt(1)), np.nextafter(dt(-0.5), dt(-1))]
    for i, v in enumerate(vals):
        if i < B:
            qcol[i] = v
            r[i], d[i] = 0.5, 1.0
    if 6 < B:
        d[6] = 0.0
        nq_cols(6)
    if 7 < B:
        d[7] = 1.0


def dqn_case(B, A, dt, seed=0, rdt=np.float32, ddt=np.float32, adt=np.int64):
    """uniform Q in [-8, 8], rewards in [-3, 3], about a tenth of the rows done, the planted rows"""
    rng = np.random.default_rng([11, B, A, seed])
    q = rng.uniform(-8, 8, (B, A)).astype(dt)
    nq = rng.uniform(-8, 8, (B, A)).astype(dt)
    act = rng.integers(0, A, B).astype(adt)
    r = rng.uniform(-3, 3, B).astype(rdt)
    d = (rng.random(B) < 0.1).astype(ddt)
    chosen = q[np.arange(B), act].copy()

    def tie(i):
        nq[i] = dt(-2.0)
        nq[i, 0] = nq[i, A - 1] = dt(7.25)                  # the maximum twice, first and last column

    _plant(chosen, tie, r, d, dt)
    q[np.arange(B), act] = chosen
    return dict(q=q, next_q=nq, actions=act, rewards=r, dones=d)


def critics_case(B, K, dt, seed=0, rdt=np.float32, ddt=np.float32):
    rng = np.random.default_rng([13, B, K, seed])
    q = [rng.uniform(-8, 8, B).astype(dt) for _ in range(K)]
    nq = [rng.uniform(-8, 8, B).astype(dt) for _ in range(K)]
    lp = rng.uniform(-4, 1, B).astype(dt)
    r = rng.uniform(-3, 3, B).astype(rdt)
    d = (rng.random(B) < 0.1).astype(ddt)

    def tie(i):
        for k in range(K):
            nq[k][i] = dt(5.0)
        nq[0][i] = nq[K - 1][i] = dt(-7.25)                 # the minimum twice (K = 1: once)

    _plant(q[0], tie, r, d, dt)
    return dict(q=q, next_q=nq, next_log_prob=lp, rewards=r, dones=d)


def sb3_dqn_lines(c, gamma):
    """SB3's DQN.train lines typed out on float64 CPU tensors -> (loss, d loss / d q, y)"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    q = t(c["q"]).requires_grad_(True)
    with torch.no_grad():
        next_q_values = t(c["next_q"])
        next_q_values, _ = next_q_values.max(dim=1)
        next_q_values = next_q_values.reshape(-1, 1)
        target_q_values = t(c["rewards"]).reshape(-1, 1) + (1 - t(c["dones"]).reshape(-1, 1)) * gamma * next_q_values
    current_q_values = torch.gather(q, dim=1, index=torch.from_numpy(np.asarray(c["actions"]).astype(np.int64)).reshape(-1, 1))
    loss = F.smooth_l1_loss(current_q_values, target_q_values)
    loss.backward()
    return float(loss.detach()), q.grad.numpy(), target_q_values.numpy().reshape(-1)


def sb3_critic_lines(kind, c, gamma, alpha=None):
    """SB3's TD3.train / SAC.train critic lines on float64 CPU tensors -> (loss, [d loss / d q_k], y)"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64)).reshape(-1, 1)
    qs = [t(x).requires_grad_(True) for x in c["q"]]
    with torch.no_grad():
        next_q_values = torch.cat([t(x) for x in c["next_q"]], dim=1)
        next_q_values, _ = torch.min(next_q_values, dim=1, keepdim=True)
        if kind == "sac":
            next_q_values = next_q_values - alpha * t(c["next_log_prob"])
        target_q_values = t(c["rewards"]) + (1 - t(c["dones"])) * gamma * next_q_values
    critic_loss = sum(F.mse_loss(current_q, target_q_values) for current_q in qs)
    if kind == "sac":
        critic_loss = 0.5 * critic_loss
    critic_loss.backward()
    return float(critic_loss.detach()), [x.grad.numpy().reshape(-1) for x in qs], target_q_values.numpy().reshape(-1)
