"""The replay buffer of stable-baselines3 2.0.0a13 (common/buffers.py: ReplayBuffer.__init__, add, sample, _get_samples with
optimize_memory_usage off, as DictReplayBuffer requires; common/off_policy_algorithm.py: _store_transition's terminal observation),
from which the reference's DQN, TD3, SAC and TQC train, restated in NumPy for the tests of ptg_replay_add / ptg_replay_sample.
The lines are SB3's with `self.` kept and the dtype handling dropped: arrays are stored as integer BIT PATTERNS of the payload's
element size, so every comparison is byte for byte.  `timeouts` is identically 0 in the reference (env/ptg_gym_env.py:478-481
never truncates) and is left out.  SB3 draws the sample indices with np.random.randint; that stream is not restated -- the
device's own draw is, in integer arithmetic, from the keying written in include/ptg_env.h."""
import numpy as np

M32 = 0xFFFFFFFF


class ReplayBuffer:
    def __init__(self, buffer_size, n_envs, obs_dim, obs_dtype, col_dtypes):
        self.buffer_size = max(buffer_size // n_envs, 1)
        self.n_envs = n_envs
        self.pos = 0
        self.full = False
        self.observations = np.zeros((self.buffer_size, n_envs, obs_dim), dtype=obs_dtype)
        self.next_observations = np.zeros((self.buffer_size, n_envs, obs_dim), dtype=obs_dtype)
        self.columns = [np.zeros((self.buffer_size, n_envs), dtype=dt) for dt in col_dtypes]      # actions, rewards, dones, ...

    def size(self):
        return self.buffer_size if self.full else self.pos

    def add(self, obs, next_obs, cols):
        """one vector step: obs, next_obs [n_envs, obs_dim]; cols: one [n_envs] array per column"""
        self.observations[self.pos] = np.array(obs).copy()
        self.next_observations[self.pos] = np.array(next_obs).copy()
        for ring, c in zip(self.columns, cols):
            ring[self.pos] = np.array(c).copy()
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True
            self.pos = 0

    def _get_samples(self, batch_inds, env_indices):
        return (self.observations[batch_inds, env_indices, :], self.next_observations[batch_inds, env_indices, :],
                [ring[batch_inds, env_indices] for ring in self.columns])

    def get_flat(self, idx):
        """_get_samples at the flat indices i = slot * n_envs + env of the device interface"""
        idx = np.asarray(idx, dtype=np.int64)
        assert ((idx >= 0) & (idx < self.size() * self.n_envs)).all()          # NumPy would wrap a negative index, the device refuses it
        return self._get_samples(idx // self.n_envs, idx % self.n_envs)


def store_window(rb, prev_obs, obs, done, cols, final_obs=None, done_col=None):
    """OffPolicyAlgorithm._store_transition over a window of T vector steps: the observation of step t is the next observation of
    step t - 1 (prev_obs for t = 0); next_obs = deepcopy(new_obs) with next_obs[i] = infos[i]["terminal_observation"] where
    done[i] (final_obs given), else the post-reset observation stays; column done_col holds float32(done)."""
    T = obs.shape[0]
    for t in range(T):
        next_obs = obs[t].copy()
        if final_obs is not None:
            for i in np.nonzero(done[t])[0]:
                next_obs[i] = final_obs[t, i]
        step_cols = [np.float32(done[t] != 0).view(np.int32) if c == done_col else cols[c][t] for c in range(len(cols))]
        rb.add(prev_obs if t == 0 else obs[t - 1], next_obs, step_cols)


def lowbias32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw_index(seed, c, b, total):
    """row b of the c-th device-drawn batch under seed, out of `total` = size * n_envs transitions (Python integers)"""
    h = lowbias32
    k = h((seed & M32) ^ 0x9E3779B9)
    k = h(k + ((seed >> 32) & M32))
    k = h(k ^ (c & M32))
    k = h(k + ((c >> 32) & M32))
    k = h(k ^ (b & M32))
    k = h(k + ((b >> 32) & M32))
    w0, w1 = h(k ^ 0x85EBCA6B), h(k ^ 0xC2B2AE35)
    return (((w0 << 32) | w1) * total) >> 64


def draw(seed, c, batch, total):
    return np.array([draw_index(seed, c, b, total) for b in range(batch)], dtype=np.int64)
