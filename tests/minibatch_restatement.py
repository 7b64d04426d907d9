"""How stable-baselines3 2.0.0a13 hands a rollout to PPO / A2C (common/buffers.py: BaseBuffer.swap_and_flatten, RolloutBuffer.get
and _get_samples -- every training batch of the reference's algorithms goes through them), restated in NumPy for the tests of
ptg_minibatch.  swap_and_flatten and the slicing loop are SB3's lines with `self.` dropped; the permutation is an argument (SB3
draws np.random.permutation(buffer_size * n_envs); its stream is not part of what is restated)."""
import numpy as np


def swap_and_flatten(arr):
    """[n_steps, n_envs, ...] -> [n_steps * n_envs, ...], env-major: flat row n * n_steps + t is arr[t, n]."""
    shape = arr.shape
    if len(shape) < 3:
        shape = (*shape, 1)
    return arr.swapaxes(0, 1).reshape(shape[0] * shape[1], *shape[2:])


def get_slices(indices, batch_size=None):
    """RolloutBuffer.get's loop over a drawn permutation: consecutive slices of batch_size, the last one short; None = one batch."""
    total = len(indices)
    if batch_size is None:
        batch_size = total
    start_idx = 0
    while start_idx < total:
        yield indices[start_idx:start_idx + batch_size]
        start_idx += batch_size


def gather(x, idx):
    """_get_samples for one buffer: x [T, N] or [T, N, F], idx flat indices -> [B] or [B, F] (SB3 keeps [B, 1] for the former; the
    project's columns are [B])."""
    flat = swap_and_flatten(np.asarray(x))
    out = flat[np.asarray(idx)]
    return out[:, 0] if np.asarray(x).ndim == 2 else out


def minibatches(perm, batch_size, obs=None, columns=()):
    """What HipEngine.minibatches yields, on host arrays: (obs rows or None, [column entries]) per slice of perm."""
    for idx in get_slices(np.asarray(perm), batch_size):
        yield (None if obs is None else gather(obs, idx)), [gather(c, idx) for c in columns]
