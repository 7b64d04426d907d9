"""Generalised advantage estimation as stable-baselines3 2.0.0a13 computes it (common/buffers.py,
RolloutBuffer.compute_returns_and_advantage -- what the reference's A2C and PPO run after every collect), restated in NumPy
for the tests of ptg_gae.  The loop body is SB3's, line for line, with `self.` dropped; the arrays are of ONE float dtype and
gamma / gae_lambda are Python floats, so NumPy itself fixes every rounding and scalar cast:
  gamma * next_values                 the Python float meets a float32 array as float32(gamma)
  gamma * gae_lambda * ...            the product of the two Python floats is taken in double first
  ... * next_non_terminal             a multiplication: NaN / Inf next values at a finished step propagate
`done` follows the project's rollout convention (done[t] != 0: the episode ended on step t): SB3's episode_starts[t + 1] is
done[t] and the `dones` argument of the method is done[T - 1].  Both are held in the arrays' dtype here, as SB3 holds
episode_starts; SB3 itself receives `dones` as a bool array, whose `1.0 - dones` NumPy makes float64 -- the restatement keeps
the buffer's precision on the last step too, which is the recurrence include/ptg_env.h states."""
import numpy as np


def compute_returns_and_advantage(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """rewards, values, episode_starts [T, N], last_values, dones [N], all of one dtype -> (advantages, returns) of that dtype."""
    buffer_size = rewards.shape[0]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(buffer_size)):
        if step == buffer_size - 1:
            next_non_terminal = 1.0 - dones
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    returns = advantages + values
    return advantages, returns


def gae(rew, val, done, last_val, gamma, gae_lambda, dtype):
    """The project's convention in, SB3's buffers out: rew, val [T, N] (or [N]), done [T, N] of any integer / bool type,
    last_val [N] -> (adv, ret) [T, N] of `dtype`.  The inputs must already be representable in `dtype` (astype is a no-op then)."""
    dtype = np.dtype(dtype)
    rew, val, done = (np.atleast_2d(np.asarray(x)) for x in (rew, val, done))
    rewards, values, last_values = rew.astype(dtype), val.astype(dtype), np.asarray(last_val).astype(dtype)
    flags = (done != 0).astype(dtype)
    episode_starts = np.zeros_like(flags)
    episode_starts[1:] = flags[:-1]                         # row 0 (did the window open on a fresh episode) is never read
    with np.errstate(all="ignore"):                         # NaN / Inf inputs are part of the tests
        adv, ret = compute_returns_and_advantage(rewards, values, episode_starts, last_values, flags[-1],
                                                 float(gamma), float(gae_lambda))
    assert adv.dtype == dtype and ret.dtype == dtype
    return adv, ret
