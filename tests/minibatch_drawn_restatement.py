"""The permutation that ptg_minibatch_drawn draws its minibatches from, and the rule of its cursor, restated in Python integers from
the text of include/ptg_env.h (ptg_minibatch_drawn) -- not from the kernel.  There is no SB3 line to restate: SB3 draws
np.random.permutation(T * N) on the host, and that stream is not reproduced (nor was it by HipEngine.minibatches, which takes any
permutation).  What is restated is a keyed bijection of [0, TN): a balanced-as-possible Feistel network over the n = max(2,
bit_length(TN - 1)) bits of a position, cycle-walked into range.  It is NOT a uniform draw from the TN! orders."""
import numpy as np

from replay_restatement import M32, lowbias32

ROUNDS = 6                               # PTG_MB_PERM_ROUNDS
MAX_ROWS = 1 << 48                       # PTG_MB_DRAWN_MAX_ROWS


def draw_word(seed, c, b):
    """the 64-bit word (w0 << 32) | w1 of ptg_replay_sample's keying, here with (c, b) = (epoch, round)"""
    h = lowbias32
    k = h((seed & M32) ^ 0x9E3779B9)
    k = h(k + ((seed >> 32) & M32))
    k = h(k ^ (c & M32))
    k = h(k + ((c >> 32) & M32))
    k = h(k ^ (b & M32))
    k = h(k + ((b >> 32) & M32))
    return (h(k ^ 0x85EBCA6B) << 32) | h(k ^ 0xC2B2AE35)


def width(TN):
    """(a, b): the bits of the low and of the high half"""
    n = max(2, (TN - 1).bit_length())
    a = n // 2
    return a, n - a


def round_keys(seed, epoch, rounds=ROUNDS):
    return [draw_word(seed, epoch, r) >> 32 for r in range(rounds)]


def rounds_forward(x, keys, a, b):
    """one application of the round function to x in [0, 2^(a + b))"""
    mask_a, mask_b = (1 << a) - 1, (1 << b) - 1
    lo, hi = x & mask_a, (x >> a) & mask_b
    for r, k in enumerate(keys):
        if r % 2 == 0:
            hi ^= lowbias32(lo ^ k) & mask_b
        else:
            lo ^= lowbias32(hi ^ k) & mask_a
    return (hi << a) | lo


def rounds_backward(x, keys, a, b):
    """its inverse: every round is an involution, so the rounds run in the opposite order"""
    mask_a, mask_b = (1 << a) - 1, (1 << b) - 1
    lo, hi = x & mask_a, (x >> a) & mask_b
    for r in reversed(range(len(keys))):
        if r % 2 == 0:
            hi ^= lowbias32(lo ^ keys[r]) & mask_b
        else:
            lo ^= lowbias32(hi ^ keys[r]) & mask_a
    return (hi << a) | lo


def perm_at(i, TN, keys, count=None):
    """perm(i) for 0 <= i < TN under the round keys of one epoch: the round function applied until the result is below TN.  count: a
    list that receives the number of applications"""
    assert 0 <= i < TN <= MAX_ROWS
    a, b = width(TN)
    x, k = rounds_forward(i, keys, a, b), 1
    while x >= TN:
        x, k = rounds_forward(x, keys, a, b), k + 1
    if count is not None:
        count.append(k)
    return x


def position_of(v, TN, keys):
    """perm's inverse: the backward rounds applied until the result is below TN"""
    a, b = width(TN)
    x = rounds_backward(v, keys, a, b)
    while x >= TN:
        x = rounds_backward(x, keys, a, b)
    return x


def perm(TN, seed, epoch, rounds=ROUNDS):
    """the whole order of epoch `epoch`: int64 [TN], value i = env * T + step (SB3's swap_and_flatten index)"""
    keys = round_keys(seed, epoch, rounds)
    return np.array([perm_at(i, TN, keys) for i in range(TN)], dtype=np.int64)


def batch(TN, B, seed, epoch, j):
    """the indices of batch j of epoch `epoch`: positions j * B ... j * B + B - 1"""
    assert TN % B == 0 and 0 <= j < TN // B
    keys = round_keys(seed, epoch)
    return np.array([perm_at(j * B + l, TN, keys) for l in range(B)], dtype=np.int64)


# ---- the cursor {epochs finished, batches drawn in this epoch}
def advance(epoch, j, batches):
    """behind a drawn batch; batches = TN / B"""
    j += 1
    if j >= batches:
        epoch, j = epoch + 1, 0
    return epoch, j


def end_epoch(epoch, j):
    """ptg_minibatch_end_epoch: an epoch cut short ends here; a fresh one (j == 0) is left alone"""
    if j != 0:
        epoch, j = epoch + 1, 0
    return epoch, j
