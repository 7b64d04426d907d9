"""DeviceRolloutBuffer: the rollout buffer the reference's on-policy algorithms (PPO, A2C) collect into, resident on the GPU.

It restates stable-baselines3 2.0.0a13 common/buffers.py RolloutBuffer over torch tensors that never leave the device: begin() and
add() enqueue kernels of csrc/ptg_train.hip (ptg_rollout_buffer_begin: one; ptg_rollout_buffer_add: the copy and the one-thread cursor
kernel behind it; include/ptg_env.h) on the current stream, without synchronisation, so a collect step -- DeviceMLP -> act_* ->
HipEngine.step() -> add() -- can be captured into one graph and replayed: the row number lives on the device (cursor), like the step count of the hot kernels, so every replay stores
at the next row.  compute_returns_and_advantage() and get() are HipEngine.gae / vn_normalize / minibatches over the same storage.

Row layout: obs_rows[0] is the observation the window's first action is chosen from (begin() puts it there), add() number t writes
obs_rows[t + 1] and row t of every column.  After T adds obs_rows[:T] are SB3's `observations`, obs_rows[T] is `new_obs` -- what
last_values is computed from -- and SB3's episode_starts[t + 1] is dones[t].  There is no state_dict: SB3 does not checkpoint rollout
buffers."""
import collections

RolloutStorage = collections.namedtuple("RolloutStorage", ["obs_rows", "col_rows", "cursor"])
RolloutBufferSamples = collections.namedtuple("RolloutBufferSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])


class DeviceRolloutBuffer:
    def __init__(self, engine, n_steps, columns=None):
        """n_steps vector steps of engine.n envs per window.  columns: name -> torch dtype of the per-step columns beside the
        observations; "actions" is required (default: actions int64 for a discrete engine, float32 for a continuous one, values
        float32, log_probs float32), "rewards" (the engine's out_dtype) and "dones" (uint8, step()'s own flags, which gae takes) are
        always kept; at most 8 in all.  compute_returns_and_advantage() needs a float32 or float64 "values" column -- advantages and
        returns [T, N] of its dtype are allocated here when there is one -- and get() needs "values" and "log_probs" as well."""
        from . import _lib
        torch = self._torch = engine._torch
        self.engine = engine
        self.n_envs = engine.n
        self.n_steps = int(n_steps)
        if self.n_steps < 1:
            raise ValueError(f"DeviceRolloutBuffer: n_steps must be >= 1, got {n_steps}")
        cols = dict(columns) if columns is not None else {"actions": torch.float32 if engine.action_type == 1 else torch.int64,
                                                          "values": torch.float32, "log_probs": torch.float32}
        if "actions" not in cols:
            raise ValueError("DeviceRolloutBuffer: columns must name 'actions'")
        if "rewards" in cols or "dones" in cols:
            raise ValueError("DeviceRolloutBuffer: 'rewards' and 'dones' are kept by the buffer itself")
        cols["rewards"] = engine.out_dtype
        cols["dones"] = torch.uint8
        if len(cols) > _lib.MB_MAX_COLS:
            raise ValueError(f"DeviceRolloutBuffer: at most {_lib.MB_MAX_COLS} columns with 'rewards' and 'dones', got {len(cols)}")
        self.columns = cols
        self.names = list(cols)
        T, N = self.n_steps, engine.n
        with torch.cuda.device(engine.device):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=engine.device)
            self.storage = RolloutStorage(engine.alloc_obs(T + 1, zero=True), [z((T, N), dt) for dt in cols.values()], z((2,), torch.int64))
            self.advantages = self.returns = None
            if "values" in cols:
                self.advantages, self.returns = z((T, N), cols["values"]), z((T, N), cols["values"])

    # views with SB3's names
    observations = property(lambda self: self.storage.obs_rows[:self.n_steps])
    last_obs = property(lambda self: self.storage.obs_rows[self.n_steps])
    actions = property(lambda self: self.column("actions"))
    values = property(lambda self: self.column("values"))
    log_probs = property(lambda self: self.column("log_probs"))
    rewards = property(lambda self: self.column("rewards"))
    dones = property(lambda self: self.column("dones"))

    def _need(self, who, *names):
        missing = [k for k in names if k not in self.names]
        if missing:
            raise ValueError(f"DeviceRolloutBuffer.{who} needs the columns {list(names)}; this buffer was built without {missing} (kept: {self.names})")

    def column(self, name):
        if name not in self.names:
            raise ValueError(f"DeviceRolloutBuffer: no column {name!r} (kept: {self.names})")
        return self.storage.col_rows[self.names.index(name)]

    def begin(self, obs=None):
        """SB3's reset(): obs (default engine.obs, what reset() or the last step() left) becomes row 0, the observation the window's
        first action is chosen from, and the cursor returns to 0.  Enqueues on the current stream; nothing is copied to the host."""
        self.engine.rollout_buffer_begin(self.storage, self.engine.obs if obs is None else obs)

    def add(self, obs, rewards, dones, **columns):
        """Store one step: obs, rewards, dones as HipEngine.step() left them ([N]-shaped, obs an engine-layout block), columns the
        other columns by name, [N] each with any stride >= 1 (values=out[:, A] reads a network's value column in place).  Enqueues two
        kernels on the current stream (the copy, then the cursor's advance); the row is the device cursor's, so a captured add() stores
        at the next row on every replay.
        On a full buffer nothing is stored and the engine's next sync() raises PtgError (PTG_E_INDEX), where SB3 raises IndexError."""
        extra = sorted(set(columns) ^ set(self.names[:-2]))
        if extra:
            raise ValueError(f"DeviceRolloutBuffer.add: columns given and columns kept differ in {extra}")
        self.engine.rollout_buffer_add(self.storage, obs, [columns[k] for k in self.names[:-2]] + [rewards, dones])

    def compute_returns_and_advantage(self, last_values, gamma, gae_lambda, normalize_reward=False):
        """SB3's compute_returns_and_advantage into the preallocated advantages / returns: HipEngine.gae over the rewards, values and
        dones columns with last_values [N] = V(last_obs).  normalize_reward: HipEngine.vn_normalize(training=True) over the reward
        column first (VecNormalize sits before SB3's buffer); the column itself keeps the raw rewards, and the normalised copy is a
        fresh tensor.  Rewards of another dtype than the values are cast, which allocates too.  Does not synchronise and does not
        check that the window is full: rows not yet added hold the previous window's values."""
        self._need("compute_returns_and_advantage", "values")
        eng = self.engine
        rew = self.rewards
        if normalize_reward:
            rew = eng.vn_normalize(rew, self.dones)
        if rew.dtype != self.values.dtype:
            rew = rew.to(self.values.dtype)
        eng.gae(rew, self.values, self.dones, last_values, gamma, gae_lambda, adv=self.advantages, ret=self.returns)
        return self.advantages, self.returns

    def get(self, batch_size=None, perm=None):
        """SB3's get(): yields RolloutBufferSamples(observations [B, F], actions, old_values, old_log_prob, advantages, returns [B]
        each) through HipEngine.minibatches over a permutation of T * N (perm, or a fresh torch.randperm on the device); batch_size
        None: one batch of everything (A2C).  Does not synchronise and does not check that the window is full."""
        self._need("get", "values", "log_probs")
        torch = self._torch
        if perm is None:
            with torch.cuda.device(self.engine.device):
                perm = torch.randperm(self.n_steps * self.n_envs, device=self.engine.device)
        cols = [self.actions, self.values, self.log_probs, self.advantages, self.returns]
        for obs, outs in self.engine.minibatches(perm, batch_size, obs=self.observations, columns=cols):
            yield RolloutBufferSamples(obs, *outs)

    def cursor(self):
        """(rows added in this window, the reserved second word: 0); synchronises"""
        a, c = self.storage.cursor.cpu().tolist()
        return int(a), int(c)

    @property
    def pos(self):
        return self.cursor()[0]

    @property
    def full(self):
        return self.cursor()[0] >= self.n_steps
