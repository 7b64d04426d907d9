"""What the GPU tests of ptg_gae (tests/test_gae.py) compare against, pinned without a GPU: the NumPy restatement of SB3's
RolloutBuffer.compute_returns_and_advantage (tests/gae_restatement.py) against a hand-computed answer and two closed forms, and
the entry point's refusal of a NULL handle (the library loads without a device, tests/test_cabi.py)."""
import ctypes as C

import numpy as np
import pytest

import gae_restatement as gr

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_three_steps_two_envs(dtype):
    """gamma = gae_lambda = 0.5, so gamma * gae_lambda = 0.25; every number below is a dyadic fraction, exact in float32.
    env 0, no done:  rew 1 2 3, val 0.5 1 2, last value 4
      t=2: delta = 3 + 0.5*4*1 - 2   = 3     last = 3                   ret = 3 + 2        = 5
      t=1: delta = 2 + 0.5*2*1 - 1   = 2     last = 2 + 0.25*1*3        = 2.75     ret = 3.75
      t=0: delta = 1 + 0.5*1*1 - 0.5 = 1     last = 1 + 0.25*1*2.75     = 1.6875   ret = 2.1875
    env 1, done on t=1:  rew -1 4 0.5, val 2 -1 8, last value -2
      t=2: delta = 0.5 + 0.5*(-2)*1 - 8 = -8.5   last = -8.5                        ret = -0.5
      t=1: delta = 4 + 0.5*8*0 - (-1)   = 5      last = 5 + 0.25*0*(-8.5) = 5       ret = 4      (the episode ended here: nothing
                                                                                                   of t=2 reaches this step)
      t=0: delta = -1 + 0.5*(-1)*1 - 2  = -3.5   last = -3.5 + 0.25*1*5   = -2.25   ret = -0.25"""
    rew = np.array([[1.0, -1.0], [2.0, 4.0], [3.0, 0.5]])
    val = np.array([[0.5, 2.0], [1.0, -1.0], [2.0, 8.0]])
    done = np.array([[0, 0], [0, 1], [0, 0]], np.uint8)
    last = np.array([4.0, -2.0])
    adv, ret = gr.gae(rew, val, done, last, 0.5, 0.5, dtype)
    assert adv.dtype == dtype and ret.dtype == dtype
    np.testing.assert_array_equal(adv, np.array([[1.6875, -2.25], [2.75, 5.0], [3.0, -8.5]], dtype))
    np.testing.assert_array_equal(ret, np.array([[2.1875, -0.25], [3.75, 4.0], [5.0, -0.5]], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lambda_zero_gives_the_one_step_td_error(dtype):
    rng = np.random.default_rng(1)
    T, N, gamma = 40, 33, 0.973
    rew, val = rng.normal(0, 1, (T, N)).astype(dtype), rng.normal(0, 1, (T, N)).astype(dtype)
    last = rng.normal(0, 1, N).astype(dtype)
    done = (rng.random((T, N)) < 0.1).astype(np.uint8)
    adv, ret = gr.gae(rew, val, done, last, gamma, 0.0, dtype)
    nv = np.concatenate([val[1:], last[None]])
    delta = rew + gamma * nv * (1.0 - done.astype(dtype)) - val
    assert delta.dtype == dtype
    np.testing.assert_array_equal(adv, delta)
    np.testing.assert_array_equal(ret, delta + val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gamma_lambda_one_without_done_gives_the_reward_to_go(dtype):
    """small integers: every sum is exact, so ret[t] = sum of rew[t:] + last value holds to the bit"""
    rng = np.random.default_rng(2)
    T, N = 50, 17
    rew, val = rng.integers(-8, 9, (T, N)).astype(dtype), rng.integers(-8, 9, (T, N)).astype(dtype)
    last = rng.integers(-8, 9, N).astype(dtype)
    adv, ret = gr.gae(rew, val, np.zeros((T, N), np.uint8), last, 1.0, 1.0, dtype)
    to_go = np.cumsum(rew[::-1], axis=0)[::-1] + last
    np.testing.assert_array_equal(ret, to_go.astype(dtype))
    np.testing.assert_array_equal(adv, (to_go - val).astype(dtype))


def test_one_row_input_is_one_step():
    adv, ret = gr.gae(np.array([1.0, 2.0]), np.array([0.5, 0.25]), np.array([0, 1]), np.array([2.0, 100.0]), 0.5, 0.9, np.float32)
    np.testing.assert_array_equal(adv, np.array([[1.5, 1.75]], np.float32))
    np.testing.assert_array_equal(ret, np.array([[2.0, 2.0]], np.float32))


def test_null_handle_is_invalid():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.ptg_gae(None, p, p, p, p, 1, _lib.OUT_F32, 0.99, 0.95, p, p, None) == -1      # PTG_E_INVALID
    assert "ptg_gae" in _lib.EXPORTS
