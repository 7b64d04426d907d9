"""What the GPU tests of the device replay buffer (tests/test_replay.py) compare against, pinned without a GPU: the NumPy
restatement of SB3's ReplayBuffer (tests/replay_restatement.py) against a typed-out case, and the restated device index draw's
range, determinism and spread; the entry points' refusal of a NULL handle (the library loads without a device)."""
import ctypes as C

import numpy as np
import pytest

import replay_restatement as rr


def _window(T, N, F, first):
    """obs[t, e, f] = 100 (first + t) + 10 e + f: step `first + t`'s new observation"""
    t, e, f = np.meshgrid(np.arange(T), np.arange(N), np.arange(F), indexing="ij")
    return (100 * (first + t) + 10 * e + f).astype(np.int32)


def test_known_answer_three_rows_two_envs_five_adds():
    """S = 3 (buffer_size 7 // 2 envs), five adds: steps 0, 1, 2 fill the rows, `full` turns true on the third add, steps 3 and 4
    overwrite rows 0 and 1; row 2 survives with step 2"""
    rb = rr.ReplayBuffer(7, 2, 2, np.int32, [np.int32, np.int32])
    assert rb.buffer_size == 3
    obs = _window(5, 2, 2, 1)                                # step t's new observation is "observation number t + 1"
    prev = _window(1, 2, 2, 0)[0]                            # observation number 0
    act = np.arange(10, dtype=np.int32).reshape(5, 2) + 50   # act[t, e] = 50 + 2 t + e
    done = np.zeros((5, 2), np.uint8); done[3, 1] = 1
    fin = -_window(5, 2, 2, 1)
    seen = []
    for t in range(5):
        rr.store_window(rb, prev if t == 0 else obs[t - 1], obs[t:t + 1], done[t:t + 1], [act[t:t + 1], None], fin[t:t + 1], done_col=1)
        seen.append((rb.pos, rb.full, rb.size()))
    assert seen == [(1, False, 1), (2, False, 2), (0, True, 3), (1, True, 3), (2, True, 3)]
    # rows hold steps 3, 4, 2: observation of step t is observation number t, its next observation number t + 1
    np.testing.assert_array_equal(rb.observations[:, :, 0], [[300, 310], [400, 410], [200, 210]])
    np.testing.assert_array_equal(rb.next_observations[:, :, 1], [[401, -411], [501, 511], [301, 311]])     # env 1 ended on step 3
    np.testing.assert_array_equal(rb.columns[0], [[56, 57], [58, 59], [54, 55]])
    np.testing.assert_array_equal(rb.columns[1].view(np.float32), [[0, 1], [0, 0], [0, 0]])
    o, n, (a, d) = rb.get_flat([5, 0, 1, 1])                 # flat index = row * 2 + env; repeats are legal
    np.testing.assert_array_equal(o, [[210, 211], [300, 301], [310, 311], [310, 311]])
    np.testing.assert_array_equal(n, [[310, 311], [400, 401], [-410, -411], [-410, -411]])
    np.testing.assert_array_equal(a, [55, 56, 57, 57])
    np.testing.assert_array_equal(d.view(np.float32), [0, 0, 1, 1])


def test_a_window_is_its_steps_one_by_one_and_without_final_obs_the_reset_observation_stays():
    rng = np.random.default_rng(0)
    T, N, F = 7, 3, 4
    obs, prev = rng.integers(0, 1 << 30, (T, N, F), dtype=np.int32), rng.integers(0, 1 << 30, (N, F), dtype=np.int32)
    col = rng.integers(0, 1 << 30, (T, N), dtype=np.int32)
    done = (rng.random((T, N)) < 0.3).astype(np.uint8)
    a, b = rr.ReplayBuffer(5 * N, N, F, np.int32, [np.int32]), rr.ReplayBuffer(5 * N, N, F, np.int32, [np.int32])
    rr.store_window(a, prev, obs[:5], done[:5], [col[:5]])
    rr.store_window(a, obs[4], obs[5:], done[5:], [col[5:]])
    for t in range(T):
        rr.store_window(b, prev if t == 0 else obs[t - 1], obs[t:t + 1], done[t:t + 1], [col[t:t + 1]])
    for x, y in [(a.observations, b.observations), (a.next_observations, b.next_observations), (a.columns[0], b.columns[0])]:
        np.testing.assert_array_equal(x, y)
    assert (a.pos, a.full) == (2, True)
    np.testing.assert_array_equal(a.next_observations[1], obs[6])           # no final_obs: next_obs is the new observation, done or not
    np.testing.assert_array_equal(a.observations[1], obs[5])


def test_one_row_buffer():
    rb = rr.ReplayBuffer(1, 4, 1, np.int32, [])
    assert rb.buffer_size == 1                               # max(1 // 4, 1)
    rr.store_window(rb, np.zeros((4, 1), np.int32), np.ones((1, 4, 1), np.int32), np.zeros((1, 4), np.uint8), [])
    assert (rb.pos, rb.full, rb.size()) == (0, True, 1)


def test_lowbias32_known_values():
    assert rr.lowbias32(0) == 0
    x = 1                                                    # the finaliser's lines by hand for x = 1
    x ^= x >> 16; x = (x * 0x7feb352d) % 2 ** 32; x ^= x >> 15; x = (x * 0x846ca68b) % 2 ** 32; x ^= x >> 16
    assert rr.lowbias32(1) == x and 0 < x < 2 ** 32
    assert len({rr.lowbias32(v) for v in range(4096)}) == 4096


@pytest.mark.parametrize("total", [1, 2, 192, 12345, 2 ** 33 + 5])
def test_the_draw_stays_in_range_and_is_deterministic(total):
    a = rr.draw(7, 0, 2000, total)
    assert a.min() >= 0 and a.max() < total
    assert np.array_equal(a, rr.draw(7, 0, 2000, total))
    if total > 100:
        assert not np.array_equal(a, rr.draw(7, 1, 2000, total))            # the next batch
        assert not np.array_equal(a, rr.draw(8, 0, 2000, total))            # another seed
        assert not np.array_equal(a, rr.draw(7 + 2 ** 32, 0, 2000, total))  # the seed's high half
        assert not np.array_equal(a, rr.draw(7, 2 ** 32, 2000, total))      # the counter's high half
    if total > 2 ** 32:
        assert a.max() > 2 ** 32                             # the low word matters there


def test_the_draw_spreads_over_192_cells():
    """the GPU test's bound on the restatement itself: B = 65 536 over 192 cells, every count within 341 +- 111 (6 sigma)"""
    counts = np.bincount(rr.draw(3, 5, 65536, 192), minlength=192)
    assert counts.sum() == 65536 and np.abs(counts - 65536 / 192).max() <= 111, (counts.min(), counts.max())


def test_the_entry_points_refuse_a_null_handle():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    d = _lib.PtgReplay()
    assert L.ptg_replay_add(None, C.byref(d), None, None, 0, 0, 0, None, None, -1, 0, None, 1, None) == _lib.E_INVALID
    assert L.ptg_replay_sample(None, C.byref(d), None, 1, 0, None, None, None, -1, None, None) == _lib.E_INVALID
    assert L.ptg_abi_version() >= 11
