"""What the GPU tests of the drawn minibatches (tests/test_minibatch_drawn.py) compare against, pinned without a GPU: the Python-integer
restatement of ptg_minibatch_drawn's permutation and cursor rule (tests/minibatch_drawn_restatement.py, written from the text of
include/ptg_env.h) -- one typed-out example, bijection and inverse at every size class, distinct keys, the bucket test that sets the
number of rounds -- and the Python-level refusals of HipEngine.minibatch_drawn / minibatch_end_epoch and of DeviceRolloutBuffer's
epoch cursor on CPU tensors, with the library not reached, and what reaches the library."""
import re
import os

import numpy as np
import pytest

import minibatch_drawn_restatement as md
import replay_restatement as rr
from helpers import host_engine, recording_engine
from rl_ptg_amd.rollout_buffer import DeviceRolloutBuffer, RolloutBufferSamples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 203, 1218, 4095, 4096, 4097, 25578]
CHI2_49_999 = 85.4                       # the 99.9 % quantile of a chi-square of 49 degrees of freedom (85.35): a property of the statistic


def test_one_typed_out_example():
    """TN = 5 under seed 11, epoch 2: n = 3 bits, one low and two high; the six round keys and all five indices"""
    assert md.width(5) == (1, 2)
    assert md.round_keys(11, 2) == [61604379, 2206688443, 1405373292, 1078391092, 516289661, 635487353]
    assert md.perm(5, 11, 2).tolist() == [4, 2, 1, 0, 3]
    assert md.batch(5, 5, 11, 2, 0).tolist() == [4, 2, 1, 0, 3]
    assert [md.batch(9, 3, 11, 0, j).tolist() for j in range(3)] == [[4, 0, 2], [8, 3, 5], [7, 6, 1]]
    # the keying is ptg_replay_sample's: the index it draws out of 2^64 "transitions" is the word itself
    assert md.draw_word(11, 2, 3) == rr.draw_index(11, 2, 3, 1 << 64) and md.draw_word(11, 2, 3) >> 32 == 1078391092


def test_the_header_states_the_constants_of_the_restatement():
    from rl_ptg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert int(re.search(r"#define PTG_MB_PERM_ROUNDS (\d+)", hdr).group(1)) == md.ROUNDS == _lib.MB_PERM_ROUNDS == 6
    assert re.search(r"#define PTG_MB_DRAWN_MAX_ROWS \(\(uint64_t\)1 << (\d+)\)", hdr).group(1) == "48"
    assert md.MAX_ROWS == _lib.MB_DRAWN_MAX_ROWS == 1 << 48 >= 1 << 40


@pytest.mark.parametrize("TN", SIZES)
def test_a_bijection_with_an_inverse_at_every_size_class(TN):
    """1; around the powers of two where the width and the split of the halves change; PPO's batch and window; every value once,
    the backward rounds return the position, and a walk is short"""
    a, b = md.width(TN)
    assert a + b == max(2, (TN - 1).bit_length()) and a == (a + b) // 2 and (1 << (a + b)) >= TN
    for seed, epoch in ((0, 0), (5, 1), (2 ** 64 - 1, 2 ** 40 + 3)):
        keys = md.round_keys(seed, epoch)
        walks = []
        p = [md.perm_at(i, TN, keys, walks) for i in range(TN)]
        assert sorted(p) == list(range(TN))
        step = max(1, TN // 257)
        assert all(md.position_of(p[i], TN, keys) == i for i in range(0, TN, step))
        assert max(walks) <= 64
        if TN > 2:
            assert np.mean(walks) <= 2.5                     # 2^n < 2 TN: geometric with p > 1 / 2
        assert np.array_equal(md.perm(TN, seed, epoch), p)


@pytest.mark.parametrize("TN", [2 ** 32 + 12345, 65537 * 65536, 2 ** 40 + 1, 2 ** 48])
def test_above_32_bits_sampled(TN):
    """a few thousand positions -- the first, the last, those around 2^32 and random ones -- give distinct values below TN, and the
    backward rounds return them"""
    rng = np.random.default_rng(TN % 1000)
    pos = {0, 1, TN - 1, TN - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 31, TN // 2} | {int(v) for v in rng.integers(0, TN, 3000)}
    pos = sorted(v for v in pos if v < TN)
    keys = md.round_keys(9, 4)
    vals = [md.perm_at(i, TN, keys) for i in pos]
    assert len(set(vals)) == len(pos) and 0 <= min(vals) and max(vals) < TN
    assert all(md.position_of(v, TN, keys) == i for i, v in zip(pos[:300], vals[:300]))
    assert TN < 2 ** 33 or max(vals) >= 2 ** 32             # the bits past 32 are alive
    with pytest.raises(AssertionError):
        md.perm_at(0, 2 ** 48 + 1, keys)


def test_two_epochs_and_two_seeds_give_different_orders():
    for TN in (203, 1218):
        orders = {(s, e): md.perm(TN, s, e).tolist() for s in (0, 1) for e in (0, 1)}
        assert len({tuple(o) for o in orders.values()}) == 4
        assert orders[(0, 0)] != list(range(TN))
        # and not merely shifted or relabelled: two orders agree at about TN / TN = 1 position
        assert sum(a == b for a, b in zip(orders[(0, 0)], orders[(0, 1)])) < 10


def _bucket_chi_square(TN, seed, rounds, epochs=400):
    """position octile x value octile over `epochs` orders, against the counts of uniform orders; 7 x 7 free cells"""
    pos = np.arange(TN) * 8 // TN
    seen = np.zeros((8, 8))
    for e in range(epochs):
        np.add.at(seen, (pos, md.perm(TN, seed, e, rounds) * 8 // TN), 1)
    n = np.bincount(pos, minlength=8).astype(np.float64)
    expected = epochs * np.outer(n, n) / TN
    return float(((seen - expected) ** 2 / expected).sum())


@pytest.mark.parametrize("TN,recorded", [(203, 49.3), (1218, 52.4), (4097, 59.0)])
def test_the_bucket_test_that_sets_the_number_of_rounds(TN, recorded):
    """seed 5, 400 epochs.  The bound is the statistic's own 99.9 % quantile.  Two rounds miss it many times over; four stay
    below it (73.0 at TN = 1218) but read 50.4 in the mean of 16 seeds where NumPy's permutations read 43.4 and six rounds 43.0
    (include/ptg_env.h), so six are used."""
    chi = _bucket_chi_square(TN, 5, md.ROUNDS)
    print(f"TN={TN}: chi-square {chi:.1f} (recorded {recorded}), bound {CHI2_49_999}")
    assert chi < CHI2_49_999
    assert abs(chi - recorded) < 0.06                       # the figures written down with the scheme are this restatement's
    if TN == 1218:                                          # the test can tell: two rounds, a quarter of the epochs
        assert _bucket_chi_square(TN, 5, 2, epochs=100) > 5 * CHI2_49_999


def test_the_cursor_rule():
    c = (0, 0)
    seen = []
    for _ in range(7):
        c = md.advance(*c, batches=3)
        seen.append(c)
    assert seen == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)]
    assert md.advance(4, 0, batches=1) == (5, 0)             # A2C: every batch is an epoch
    assert md.advance(4, 7, batches=3) == (5, 0)             # a cursor past its epoch starts the next one
    assert md.end_epoch(4, 0) == (4, 0) and md.end_epoch(4, 1) == (5, 0) and md.end_epoch(0, 2) == (1, 0)
    assert md.end_epoch(*md.end_epoch(3, 2)) == (4, 0)       # twice is once


# ---------------------------------------------------------------------------------------------- the Python layer, on the CPU
def _rollout(T, N, F):
    import torch
    return torch.zeros((T, N, F)), [torch.zeros((T, N)), torch.zeros((T, N), dtype=torch.uint8)]


def test_python_refusals_never_reach_the_library():
    import torch
    N, T, F, B = 6, 4, 3, 8
    eng = host_engine(N, obs_dim=F)
    obs, cols = _rollout(T, N, F)
    cur = eng.new_epoch_cursor()
    assert cur.dtype == torch.int64 and cur.tolist() == [0, 0]
    out, outs, io = torch.zeros((B, F)), [torch.zeros(B), torch.zeros(B, dtype=torch.uint8)], torch.zeros(B, dtype=torch.int64)
    d = lambda **kw: eng.minibatch_drawn(kw.pop("cursor", cur), kw.pop("batch_size", B), kw.pop("obs", obs), kw.pop("columns", cols),
                                         obs_out=kw.pop("obs_out", out), columns_out=kw.pop("columns_out", outs), idx_out=kw.pop("idx_out", io), **kw)
    refused = [
        (ValueError, lambda: d(batch_size=5, obs_out=torch.zeros((5, F)), columns_out=[torch.zeros(5), torch.zeros(5, dtype=torch.uint8)],
                               idx_out=torch.zeros(5, dtype=torch.int64))),                 # 5 does not divide 24
        (ValueError, lambda: d(batch_size=48, obs_out=torch.zeros((48, F)), columns_out=[torch.zeros(48), torch.zeros(48, dtype=torch.uint8)],
                               idx_out=torch.zeros(48, dtype=torch.int64))),                # nor does a batch larger than the rollout
        (ValueError, lambda: d(batch_size=0)),
        (TypeError, lambda: d(batch_size=None)),
        (TypeError, lambda: d(cursor=None)),
        (TypeError, lambda: d(cursor=cur.float())),
        (TypeError, lambda: d(cursor=cur.int())),
        (TypeError, lambda: d(cursor=torch.zeros(1, dtype=torch.int64))),                    # a draw counter is not an epoch cursor
        (TypeError, lambda: d(cursor=torch.zeros(3, dtype=torch.int64))),
        (TypeError, lambda: d(cursor=[0, 0])),
        (ValueError, lambda: d(cursor=torch.zeros(4, dtype=torch.int64)[::2])),
        (ValueError, lambda: d(cursor=torch.zeros((2, 1), dtype=torch.int64)[:, 0].reshape(1, 2))),
        (ValueError, lambda: d(idx_out=io.int())),
        (ValueError, lambda: d(idx_out=io.double())),
        (ValueError, lambda: d(idx_out=io[:B - 1])),
        (ValueError, lambda: d(idx_out=torch.zeros((B, 1), dtype=torch.int64))),
        (ValueError, lambda: d(idx_out=torch.zeros(2 * B, dtype=torch.int64)[::2])),
        # minibatch's own checks, in minibatch's words
        (ValueError, lambda: d(obs=None, columns=[], obs_out=None, columns_out=None)),
        (ValueError, lambda: d(obs=obs[:, :N - 1])),
        (TypeError, lambda: d(obs=obs.half())),
        (ValueError, lambda: d(columns=[cols[0].t()], columns_out=[outs[0]])),
        (ValueError, lambda: d(obs_out=out[:B - 1])),
        (ValueError, lambda: d(obs_out=out.double())),
        (ValueError, lambda: d(columns_out=[outs[0]])),
        (ValueError, lambda: d(columns_out=[outs[0], outs[1].float()])),
        (ValueError, lambda: d(columns=cols * 5, columns_out=outs * 5)),
        (ValueError, lambda: d(obs=None, obs_out=out)),
        (TypeError, lambda: eng.minibatch_end_epoch(None)),
        (TypeError, lambda: eng.minibatch_end_epoch(cur.float())),
        (TypeError, lambda: eng.minibatch_end_epoch(torch.zeros(1, dtype=torch.int64))),
    ]
    for k, (exc, call) in enumerate(refused):
        with pytest.raises(exc) as ei:
            call()
        assert "minibatch_drawn" in str(ei.value) or "minibatch_end_epoch" in str(ei.value) or k == 3, (k, str(ei.value))
        assert eng._L is None and cur.tolist() == [0, 0]
    gpu = host_engine(N, obs_dim=F, device=torch.device("cuda", 0))      # an engine elsewhere: the CPU cursor is on the wrong device
    with pytest.raises(ValueError, match="lives on"):
        gpu.minibatch_end_epoch(cur)
    assert gpu._L is None


def test_what_reaches_the_library():
    import torch
    N, T, F, B = 6, 4, 3, 8
    eng = recording_engine(N, obs_dim=F)
    obs, cols = _rollout(T, N, F)
    cur = eng.new_epoch_cursor()
    io = torch.zeros(B, dtype=torch.int64)
    o, outs, got_io = eng.minibatch_drawn(cur, B, obs, cols, seed=-1, idx_out=io)
    assert o.shape == (B, F) and [x.shape for x in outs] == [(B,), (B,)] and outs[1].dtype == torch.uint8 and got_io is io
    eng.minibatch(io, obs, cols, obs_out=o, columns_out=outs)
    eng.minibatch_end_epoch(cur)
    (n0, a0), (n1, a1), (n2, a2) = eng._L.calls
    assert (n0, n1, n2) == ("ptg_minibatch_drawn", "ptg_minibatch", "ptg_minibatch_end_epoch")
    assert a0[0] == "H" and a0[1].value == cur.data_ptr() and a0[2] == 2 ** 64 - 1 and a0[3].value == io.data_ptr() and a0[4:6] == (B, T)
    assert a1[1].value == io.data_ptr() and a1[2:5] == (8, B, T)
    # from obs_dev on the two calls pass the same things
    assert len(a0) - 6 == len(a1) - 5 == 12 and a0[-1] is None
    for x, y in zip(a0[6:-1], a1[5:-1]):
        if hasattr(x, "value"):
            assert x.value == y.value
        elif hasattr(x, "_length_"):
            assert list(x) == list(y)
        else:
            assert x == y
    assert a0[7:11] == (N * F, F, 1, F)
    assert a2 == ("H", a2[1], None) and a2[1].value == cur.data_ptr()
    assert eng.minibatch_drawn(cur, T * N, None, cols[:1])[2] is None     # columns only, one batch of everything, no idx_out


def test_the_buffer_owns_an_epoch_cursor():
    import torch
    N, T, F = 6, 4, 3
    eng = recording_engine(N, obs_dim=F, action_type=0)
    eng.obs = torch.zeros((N, F))
    buf = DeviceRolloutBuffer(eng, T, seed=77)
    assert buf.seed == 77 and DeviceRolloutBuffer(eng, T).seed == 0
    assert buf.epoch.dtype == torch.int64 and buf.epoch_cursor() == (0, 0) and buf.epoch.data_ptr() != buf.storage.cursor.data_ptr()
    buf.set_epoch_cursor(3, 2)
    assert buf.epoch_cursor() == (3, 2) and buf.cursor() == (0, 0)
    buf.begin()                                              # a new window leaves the epoch cursor alone
    assert buf.epoch_cursor() == (3, 2)
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            buf.set_epoch_cursor(*bad)
    eng._L.calls.clear()
    b = buf.next_batch(8)
    assert isinstance(b, RolloutBufferSamples) and b.observations.shape == (8, F) and b.actions.dtype == torch.int64
    again = buf.next_batch(8, out=b)
    assert all(x is y for x, y in zip(b, again))
    whole = buf.next_batch()
    assert whole.returns.shape == (T * N,)
    buf.end_epoch()
    assert [n for n, _ in eng._L.calls] == ["ptg_minibatch_drawn"] * 3 + ["ptg_minibatch_end_epoch"]
    a = eng._L.calls[1][1]
    assert a[1].value == buf.epoch.data_ptr() and a[2] == 77 and a[3] is None and a[4:6] == (8, T) and a[12].value == b.observations.data_ptr()
    assert list(a[14])[:5] == [x.data_ptr() for x in (buf.actions, buf.values, buf.log_probs, buf.advantages, buf.returns)]
    assert list(a[16])[:5] == [x.data_ptr() for x in b[1:]]
    assert eng._L.calls[2][1][4] == T * N
    eng._L.calls.clear()
    assert len(list(buf.get(8, drawn=True))) == 3 and len(list(buf.get(drawn=True))) == 1
    assert [n for n, _ in eng._L.calls] == ["ptg_minibatch_drawn"] * 4
    for kw in (dict(batch_size=5, drawn=True), dict(batch_size=0, drawn=True), dict(batch_size=8, drawn=True, perm=torch.arange(T * N))):
        with pytest.raises(ValueError):
            next(buf.get(**kw))
    with pytest.raises(ValueError):
        buf.next_batch(5)
    with pytest.raises(ValueError):
        buf.next_batch(8, out=(b.observations,))
    with pytest.raises(ValueError):
        buf.next_batch(8, out=b._replace(returns=b.returns.double()))
    assert len(eng._L.calls) == 4
    bare = DeviceRolloutBuffer(eng, T, columns={"actions": torch.int64})
    with pytest.raises(ValueError, match=r"next_batch needs the columns \['values', 'log_probs'\]"):
        bare.next_batch()
    eng._L.calls.clear()
    assert len(list(buf.get(8, perm=torch.arange(T * N)))) == 3             # today's route, as before
    assert [n for n, _ in eng._L.calls] == ["ptg_minibatch"] * 3
