"""What the GPU tests of ptg_minibatch (tests/test_minibatch.py) compare against, pinned without a GPU: the NumPy restatement of
SB3's swap_and_flatten / RolloutBuffer.get (tests/minibatch_restatement.py) against a typed-out example and the identities that
define it, and the entry point's refusal of a NULL handle (the library loads without a device, tests/test_cabi.py)."""
import ctypes as C

import numpy as np
import pytest

import minibatch_restatement as mr


def test_known_answer_three_steps_two_envs_two_features():
    """x[t, n] = (10 t + n, -(10 t + n)); the flat order is env 0's steps 0 1 2, then env 1's"""
    x = np.array([[[0, -0], [1, -1]], [[10, -10], [11, -11]], [[20, -20], [21, -21]]], np.float32)
    assert x.shape == (3, 2, 2)
    flat = mr.swap_and_flatten(x)
    np.testing.assert_array_equal(flat, np.array([[0, 0], [10, -10], [20, -20], [1, -1], [11, -11], [21, -21]], np.float32))
    col = np.array([[0, 1], [10, 11], [20, 21]], np.int64)
    np.testing.assert_array_equal(mr.swap_and_flatten(col), np.array([[0], [10], [20], [1], [11], [21]], np.int64))
    idx = np.array([5, 0, 3, 3, 2])
    np.testing.assert_array_equal(mr.gather(x, idx), np.array([[21, -21], [0, 0], [1, -1], [1, -1], [20, -20]], np.float32))
    np.testing.assert_array_equal(mr.gather(col, idx), np.array([21, 0, 1, 1, 20], np.int64))
    assert mr.gather(col, idx).dtype == np.int64 and mr.gather(x, idx).dtype == np.float32


@pytest.mark.parametrize("T,N,F", [(1, 1, 3), (7, 5, 4), (64, 3, 1), (5, 65, 2)])
def test_flat_row_n_T_plus_t_is_x_t_n(T, N, F):
    rng = np.random.default_rng([T, N, F])
    x = rng.normal(size=(T, N, F))
    c = rng.integers(0, 1 << 30, (T, N))
    flat, flat_c = mr.swap_and_flatten(x), mr.swap_and_flatten(c)
    assert flat.shape == (T * N, F) and flat_c.shape == (T * N, 1)
    for n in range(N):
        for t in range(T):
            assert np.array_equal(flat[n * T + t], x[t, n]) and flat_c[n * T + t, 0] == c[t, n]
    idx = rng.integers(0, T * N, 50)
    np.testing.assert_array_equal(mr.gather(x, idx), x[idx % T, idx // T])
    np.testing.assert_array_equal(mr.gather(c, idx), c[idx % T, idx // T])


def test_arange_is_the_transposition():
    T, N, F = 6, 4, 3
    x = np.arange(T * N * F, dtype=np.float64).reshape(T, N, F)
    c = np.arange(T * N, dtype=np.int32).reshape(T, N)
    np.testing.assert_array_equal(mr.gather(x, np.arange(T * N)).reshape(N, T, F), x.transpose(1, 0, 2))
    np.testing.assert_array_equal(mr.gather(c, np.arange(T * N)).reshape(N, T), c.T)


@pytest.mark.parametrize("T,N,bs", [(7, 5, 4), (21, 6, 203), (3, 3, 9), (10, 4, 1), (658, 6, 203)])
def test_slices_of_a_permutation_cover_every_row_once(T, N, bs):
    perm = np.random.default_rng(3).permutation(T * N)
    c = np.arange(T * N).reshape(T, N)                       # c[t, n] names (t, n)
    batches = list(mr.minibatches(perm, bs, None, [c]))
    sizes = [len(b[1][0]) for b in batches]
    assert len(batches) == -(-T * N // bs) and all(s == bs for s in sizes[:-1])
    assert sizes[-1] == (T * N - 1) % bs + 1                 # the short last batch (a full one when bs divides T * N)
    assert all(b[0] is None for b in batches)
    seen = np.concatenate([b[1][0] for b in batches])
    assert np.array_equal(np.sort(seen), np.arange(T * N))
    assert np.array_equal(seen, c[perm % T, perm // T])


def test_batch_size_none_is_one_batch():
    T, N = 9, 4
    perm = np.random.default_rng(4).permutation(T * N)
    x = np.random.default_rng(5).normal(size=(T, N, 2))
    batches = list(mr.minibatches(perm, None, x, [x[..., 0]]))
    assert len(batches) == 1
    np.testing.assert_array_equal(batches[0][0], x[perm % T, perm // T])
    np.testing.assert_array_equal(batches[0][1][0], x[perm % T, perm // T, 0])
    assert [len(s) for s in mr.get_slices(perm)] == [T * N]


def test_null_handle_is_invalid():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.ptg_minibatch(None, p, 4, 1, 1, p, 1, 1, 1, 1, 4, p, 0, None, None, None, None) == _lib.E_INVALID
    assert "ptg_minibatch" in _lib.EXPORTS and _lib.E_INDEX == -5
