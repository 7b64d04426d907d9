"""How stable-baselines3 2.0.0a13 stores an on-policy collect (common/buffers.py: RolloutBuffer.reset / add; common/
on_policy_algorithm.py: collect_rollouts -- what the reference's PPO and A2C run every step), restated in NumPy for the tests of
ptg_rollout_buffer_begin / ptg_rollout_buffer_add and rl_ptg_amd.DeviceRolloutBuffer.

RolloutBuffer is SB3's: reset and add are its lines with the torch / device conversions dropped (arrays in, arrays kept; dtypes are
arguments, because the device buffer moves raw bytes of any element size).  collect_step is collect_rollouts' two lines around
add: the buffer receives the observation the action was chosen FROM and the episode_starts that came with it.

DeviceRows is the layout the device buffer keeps instead, with the mapping between the two:
  row t + 1 <- the new observation of add number t (row 0 <- begin's observation), so rows[:T] == SB3's observations and rows[T] is
              new_obs, what last_values is computed from;
  dones[t]  =  SB3's episode_starts[t + 1] (dones[T - 1] is the `dones` argument of compute_returns_and_advantage);
  an add past T raises IndexError, where SB3's `self.observations[self.pos] = ...` raises it."""
import numpy as np


class RolloutBuffer:
    """SB3's RolloutBuffer: observations [T, N, F], actions, rewards, episode_starts, values, log_probs [T, N]"""

    def __init__(self, buffer_size, n_envs, obs_dim, obs_dtype=np.float32, action_dtype=np.float32, float_dtype=np.float32):
        self.buffer_size, self.n_envs, self.obs_dim = buffer_size, n_envs, obs_dim
        self.obs_dtype, self.action_dtype, self.float_dtype = obs_dtype, action_dtype, float_dtype
        self.reset()

    def reset(self):
        self.observations = np.zeros((self.buffer_size, self.n_envs, self.obs_dim), dtype=self.obs_dtype)
        self.actions = np.zeros((self.buffer_size, self.n_envs), dtype=self.action_dtype)
        self.rewards = np.zeros((self.buffer_size, self.n_envs), dtype=self.float_dtype)
        self.episode_starts = np.zeros((self.buffer_size, self.n_envs), dtype=self.float_dtype)
        self.values = np.zeros((self.buffer_size, self.n_envs), dtype=self.float_dtype)
        self.log_probs = np.zeros((self.buffer_size, self.n_envs), dtype=self.float_dtype)
        self.pos = 0
        self.full = False

    def add(self, obs, action, reward, episode_start, value, log_prob):
        self.observations[self.pos] = np.array(obs).copy()
        self.actions[self.pos] = np.array(action).copy()
        self.rewards[self.pos] = np.array(reward).copy()
        self.episode_starts[self.pos] = np.array(episode_start).copy()
        self.values[self.pos] = np.array(value).copy().flatten()
        self.log_probs[self.pos] = np.array(log_prob).copy()
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True


class Collector:
    """collect_rollouts' state around an SB3 buffer: _last_obs and _last_episode_starts"""

    def __init__(self, buffer, first_obs):
        self.buffer = buffer
        self.last_obs = np.array(first_obs).copy()
        self.last_episode_starts = np.ones(buffer.n_envs, dtype=bool)      # OnPolicyAlgorithm._setup_learn

    def collect_step(self, action, value, log_prob, new_obs, reward, done):
        """the action, value and log-prob were computed from self.last_obs; the env answered new_obs, reward, done"""
        self.buffer.add(self.last_obs, action, reward, self.last_episode_starts, value, log_prob)
        self.last_obs = np.array(new_obs).copy()
        self.last_episode_starts = np.asarray(done) != 0


class DeviceRows:
    """what the device buffer keeps: rows [T + 1, ...block...] and any columns [T, N], as raw integers of the elements' sizes; a block
    has whatever shape the caller's has ([N, F] or [F, N])"""

    def __init__(self, n_steps, block_shape, obs_dtype, col_dtypes, n_envs, fill=0):
        self.n_steps = n_steps
        self.rows = np.full((n_steps + 1,) + tuple(block_shape), fill, dtype=obs_dtype)
        self.columns = [np.full((n_steps, n_envs), fill, dtype=dt) for dt in col_dtypes]
        self.pos = 0

    def begin(self, obs):
        self.rows[0] = obs
        self.pos = 0

    def add(self, obs, cols):
        if self.pos >= self.n_steps:
            raise IndexError(f"index {self.pos} is out of bounds for axis 0 with size {self.n_steps}")
        self.rows[self.pos + 1] = obs
        for ring, c in zip(self.columns, cols):
            ring[self.pos] = c
        self.pos += 1

    @property
    def full(self):
        return self.pos >= self.n_steps

    observations = property(lambda self: self.rows[:self.n_steps])
    last_obs = property(lambda self: self.rows[self.n_steps])


def episode_starts_of(dones, first):
    """SB3's episode_starts [T, N] from the device buffer's dones [T, N] and the flags the window opened with"""
    out = np.empty(dones.shape, dtype=bool)
    out[0] = first
    out[1:] = dones[:-1] != 0
    return out
