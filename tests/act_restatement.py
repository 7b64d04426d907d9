"""The action heads of ptg_act (include/ptg_env.h states the lines) restated in NumPy for tests/test_act_host.py and tests/test_act.py:
SB3 2.0.0a13's CategoricalDistribution sample / log_prob / entropy, DQN's epsilon-greedy and the Gaussian heads, with the device's
counter-keyed draw.  Integers are uint64 masked to 32 bits; the finaliser is tests/replay_restatement.py's, so one definition serves
the replay draw and this one.  All floating point is float64 in the header's operand order; a caller rounds to the output dtype.
The second half builds the inputs the GPU tests use, so that the host test can vet every one of them (no ambiguous row)."""
import numpy as np

import replay_restatement as rr

M32 = np.uint64(0xFFFFFFFF)
U = np.uint64
HALF_LOG_2PI = 0.9189385332046727
TWO_PI = 6.283185307179586


def words(seed, c, g):
    """(w0, w1) of the rows with global env indices g (array) in the c-th call under seed: ptg_replay_sample's chain keyed (seed, c, g)"""
    h = rr.lowbias32
    g = np.atleast_1d(np.asarray(g)).astype(np.uint64)
    k = h((seed & 0xFFFFFFFF) ^ 0x9E3779B9)                  # Python integers up to here: the key's scalar part
    k = h(k + ((seed >> 32) & 0xFFFFFFFF))
    k = h(k ^ (c & 0xFFFFFFFF))
    k = h(k + ((c >> 32) & 0xFFFFFFFF))
    k = h(U(k) ^ (g & M32))
    k = h(k + (g >> U(32)))
    return h(k ^ U(0x85EBCA6B)), h(k ^ U(0xC2B2AE35))


def uniform53(w0, w1):
    return ((w0 << U(21)) | (w1 >> U(11))).astype(np.float64) * 2.0 ** -53


def _row_max(x):
    """(m, first index of m, bad): bad = the maximum is not finite (a NaN or +Inf entry, or -Inf everywhere)"""
    with np.errstate(invalid="ignore"):
        m = x.max(axis=1)
    bad = ~np.isfinite(m)
    jm = np.where(bad, 0, np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1))
    return m, jm, bad


def categorical(logits, w0=None, w1=None, deterministic=False):
    """-> dict(action int64, logp, entropy float64, bad, ambiguous bool) for logits [N, A] (any float dtype)"""
    l = np.asarray(logits).astype(np.float64)
    N, A = l.shape
    m, jm, bad = _row_max(l)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = l - m[:, None]
        e = np.exp(d)
        c = np.zeros((N, A))
        s = np.zeros(N)
        for j in range(A):                                   # s = e_0 + e_1 + ... in index order; c_j its partial sums
            s = s + e[:, j]
            c[:, j] = s
        logp = d - np.log(s)[:, None]
        ent = np.zeros(N)
        for j in range(A):
            ent = np.where(e[:, j] != 0, ent + (e[:, j] / s) * logp[:, j], ent)
        ent = -ent
        if deterministic:
            action = jm.copy()
            ambiguous = np.zeros(N, bool)
        else:
            us = uniform53(w0, w1) * s
            lt = us[:, None] < c
            action = np.where(lt.any(axis=1), lt.argmax(axis=1), A - 1)
            ambiguous = (np.abs(us[:, None] - c) <= 2.0 ** -40 * s[:, None]).any(axis=1) & ~bad
    lp = logp[np.arange(N), np.where(bad, 0, action)]
    action = np.where(bad, 0, action).astype(np.int64)
    return dict(action=action, logp=np.where(bad, np.nan, lp), entropy=np.where(bad, np.nan, ent), bad=bad, ambiguous=ambiguous)


def eps_threshold(eps):
    return int(eps * 4294967296.0)                           # (uint64)(eps * 2^32)


def eps_greedy(q, eps=None, w0=None, w1=None, deterministic=False):
    """-> dict(action int64, explore bool, bad bool); integers only past the row maximum"""
    x = np.asarray(q).astype(np.float64)
    N, A = x.shape
    m, jm, bad = _row_max(x)
    action, explore = jm.astype(np.int64), np.zeros(N, bool)
    if not deterministic:
        if not (0.0 <= eps <= 1.0):                          # NaN included
            bad = np.ones(N, bool)
        else:
            explore = w0 < U(eps_threshold(eps))
            action = np.where(explore, ((w1 * U(A)) >> U(32)).astype(np.int64), action)
    return dict(action=np.where(bad, 0, action), explore=explore, bad=bad)


def normal(w0, w1):
    u1 = (w0.astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = w1.astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def gaussian(mean, log_std, w0=None, w1=None, clip=(-1.0, 1.0), squash=False, deterministic=False):
    """-> dict(action (float64, clipped: round it to float32), raw, logp, entropy (None when squashed), bad, sigma)"""
    mu = np.asarray(mean).astype(np.float64).reshape(-1)
    ls = np.broadcast_to(np.asarray(log_std).astype(np.float64).reshape(-1), mu.shape)
    bad = ~np.isfinite(mu) | np.isnan(ls) | (ls == np.inf)
    z = np.zeros(mu.shape) if deterministic else normal(w0, w1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sigma = np.exp(ls)
        g = mu + sigma * z
        lp = ((-(z * z) / 2.0) - ls) - HALF_LOG_2PI
        x = g
        if squash:
            x = np.tanh(g)
            lp = lp - np.log((1.0 - x * x) + 1e-6)
        lo, hi = clip
        x = np.where(x < lo, lo, np.where(x > hi, hi, x))
        ent = None if squash else np.where(bad, np.nan, 1.4189385332046727 + ls)
    return dict(action=np.where(bad, 0.0, x), raw=np.where(bad, np.nan, g), logp=np.where(bad, np.nan, lp), entropy=ent, bad=bad, sigma=sigma)


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
NS = [1, 63, 64, 65, 257]
AS = [2, 5, 32]
DTYPES = [np.float32, np.float64]
SEED = 0x5EED0F00DCAFE123                                    # the draw seed of the shape sweep


def logits_case(N, A, dtype):
    """uniform in [-30, 30] with planted rows (those that fit N): 0 all equal, 1 one -Inf, 2 all but one -Inf, 3 exp underflows
    for every entry but the maximum, 4 a tie of two maxima"""
    rng = np.random.default_rng([N, A, np.dtype(dtype).itemsize])
    x = rng.uniform(-30.0, 30.0, (N, A)).astype(dtype)
    plant = [np.full(A, 1.25), None, None, None, None]
    plant[1] = x[min(1, N - 1)].copy(); plant[1][A // 2] = -np.inf
    plant[2] = np.full(A, -np.inf); plant[2][A - 1] = -3.0
    plant[3] = np.full(A, -800.0); plant[3][0] = 2.0
    plant[4] = x[min(4, N - 1)].copy(); plant[4][[0, A - 1]] = 31.0
    for r, row in enumerate(plant):
        if r < N:
            x[r] = row.astype(dtype)
    return x


def sweep_cases():
    """every (N, A, dtype) of the GPU sweep with its draw counter value: the order the GPU test makes its stochastic calls in.  Each
    case is drawn twice on one counter (row stride A with int32 actions, then A + 1 with int64), so the counter advances by 2."""
    out, c = [], {}
    for N in NS:
        c[N] = 0
        for A in AS:
            for dt in DTYPES:
                out.append((N, A, dt, c[N]))
                c[N] += 2
    return out


def gaussian_case(N, dtype, per_env):
    """means in [-1, 1], log_std in [-3, -0.5] (sigma <= 0.61): |g| <= 1 + 0.61 * 6.66 = 5.1 at the very worst, and below 4 for the
    rows the tests draw (asserted on the host): the squashed log-prob's 1 - tanh(g)^2 + 1e-6 stays above 1e-3, where a last-place
    difference between two tanh implementations moves its log by less than 1e-12"""
    rng = np.random.default_rng([N, np.dtype(dtype).itemsize, int(per_env)])
    mean = rng.uniform(-1.0, 1.0, N).astype(dtype)
    ls = rng.uniform(-3.0, -0.5, N if per_env else 1).astype(dtype)
    return mean, ls


def capture_case(N, A):
    """four [N, A + 1] float32 actor-critic outputs (logits and a value column) for the captured collect step"""
    rng = np.random.default_rng(12)
    return [rng.uniform(-3, 3, (N, A + 1)).astype(np.float32) for _ in range(4)]


def other_categorical_draws():
    """(logits, seed, counter, global offset of row 0) of every categorical draw tests/test_act.py compares exactly outside its sweep"""
    out = []
    x200 = logits_case(200, 5, np.float32)
    for c in range(2):
        out.append((x200, 11, c, 0))
    out.append((x200[100:], 11, 0, 100))
    clean = logits_case(65, 5, np.float32)
    out += [(clean, 5, c, 0) for c in range(12)]             # the bad-row test: its own rows are not compared, the clean ones are
    out += [(x[:, :5], 21, k, 0) for k, x in enumerate(capture_case(70, 5))]
    out.append((logits_case(257, 5, np.float64), SEED, 0, 0))
    out.append((nosync_case(), 0, 3, 0))
    return out


def nosync_case():
    """[65 536, 5] float32 logits of the no-synchronisation test"""
    return np.random.default_rng(77).standard_normal((65536, 5)).astype(np.float32)
