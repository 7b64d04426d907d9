"""DeviceRolloutBuffer: the rollout buffer the reference's on-policy algorithms (PPO, A2C) collect into, resident on the GPU.

It restates stable-baselines3 2.0.0a13 common/buffers.py RolloutBuffer over torch tensors that never leave the device: begin() and
add() enqueue kernels of csrc/ptg_train.hip (ptg_rollout_buffer_begin: one; ptg_rollout_buffer_add: the copy and the one-thread cursor
kernel behind it; include/ptg_env.h) on the current stream, without synchronisation, so a collect step -- DeviceMLP -> act_* ->
HipEngine.step() -> add() -- can be captured into one graph and replayed: the row number lives on the device (cursor), like the step count of the hot kernels, so every replay stores
at the next row.  compute_returns_and_advantage() and get() are HipEngine.gae / vn_normalize / minibatches over the same storage.
next_batch() is HipEngine.minibatch_drawn over it: the minibatch is named by a second device cursor {epochs finished, batches drawn
in this epoch} and its indices are computed in the gather, so a captured gradient step -- next_batch -> networks -> loss -> backward
-> optimiser -- replays through every minibatch of every epoch.

Row layout: obs_rows[0] is the observation the window's first action is chosen from (begin() puts it there), add() number t writes
obs_rows[t + 1] and row t of every column.  After T adds obs_rows[:T] are SB3's `observations`, obs_rows[T] is `new_obs` -- what
last_values is computed from -- and SB3's episode_starts[t + 1] is dones[t].  There is no state_dict: SB3 does not checkpoint rollout
buffers."""
import collections

RolloutStorage = collections.namedtuple("RolloutStorage", ["obs_rows", "col_rows", "cursor"])
RolloutBufferSamples = collections.namedtuple("RolloutBufferSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])


class DeviceRolloutBuffer:
    def __init__(self, engine, n_steps, columns=None, seed=0):
        """n_steps vector steps of engine.n envs per window; seed keys the minibatch orders that next_batch() draws.  columns: name -> torch dtype of the per-step columns beside the
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
        self.seed = int(seed)
        T, N = self.n_steps, engine.n
        with torch.cuda.device(engine.device):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=engine.device)
            self.storage = RolloutStorage(engine.alloc_obs(T + 1, zero=True), [z((T, N), dt) for dt in cols.values()], z((2,), torch.int64))
            self.advantages = self.returns = None
            if "values" in cols:
                self.advantages, self.returns = z((T, N), cols["values"]), z((T, N), cols["values"])
            self.epoch = engine.new_epoch_cursor()

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
        first action is chosen from, and the cursor returns to 0.  Enqueues on the current stream; nothing is copied to the host.
        The epoch cursor of next_batch() is left alone, so successive windows draw under successive epoch numbers."""
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

    def _batch_columns(self):
        return [self.actions, self.values, self.log_probs, self.advantages, self.returns]

    def next_batch(self, batch_size=None, out=None):
        """The next minibatch of the current epoch as RolloutBufferSamples, through HipEngine.minibatch_drawn: its indices are computed
        on the device from (seed, epoch cursor) and the cursor advances behind the gather -- past the epoch's last batch to the next
        epoch.  batch_size must divide T * N; None: one batch of everything (A2C).  out: the RolloutBufferSamples of an earlier
        call, written again -- then nothing is allocated and the call may be captured into a graph and replayed, every replay
        giving the next batch.  Does not synchronise and does not check that the window is full."""
        self._need("next_batch", "values", "log_probs")
        B = self.n_steps * self.n_envs if batch_size is None else batch_size
        if out is not None and (not isinstance(out, tuple) or len(out) != len(RolloutBufferSamples._fields)):
            raise ValueError("DeviceRolloutBuffer.next_batch: out must be the RolloutBufferSamples of an earlier call")
        obs, outs, _ = self.engine.minibatch_drawn(self.epoch, B, obs=self.observations, columns=self._batch_columns(), seed=self.seed,
                                                   obs_out=None if out is None else out[0], columns_out=None if out is None else list(out[1:]))
        return RolloutBufferSamples(obs, *outs)

    def end_epoch(self):
        """End an epoch that was cut short (PPO's target_kl): the next next_batch() is batch 0 of the next epoch; after a whole epoch,
        or before the first batch, nothing changes.  Enqueues one kernel; does not synchronise."""
        self.engine.minibatch_end_epoch(self.epoch)

    def epoch_cursor(self):
        """(epochs finished, batches drawn in this epoch); synchronises"""
        c, j = self.epoch.cpu().tolist()
        return int(c), int(j)

    def set_epoch_cursor(self, epochs, batches):
        """restore epoch_cursor() from a checkpoint; the batch size that goes with `batches` is the caller's to keep"""
        epochs, batches = int(epochs), int(batches)
        if epochs < 0 or batches < 0:
            raise ValueError(f"DeviceRolloutBuffer.set_epoch_cursor: ({epochs}, {batches}) must not be negative")
        self.epoch.copy_(self._torch.tensor([epochs, batches], dtype=self._torch.int64))

    def get(self, batch_size=None, perm=None, drawn=False):
        """SB3's get(): yields RolloutBufferSamples(observations [B, F], actions, old_values, old_log_prob, advantages, returns [B]
        each) through HipEngine.minibatches over a permutation of T * N (perm, or a fresh torch.randperm on the device); batch_size
        None: one batch of everything (A2C).  drawn=True: no permutation is made; the T * N / batch_size batches of one epoch come
        from next_batch() with fresh outputs each, from the epoch cursor on (batch_size must divide T * N).  Does not synchronise and does not check that the window is full."""
        self._need("get", "values", "log_probs")
        torch = self._torch
        if drawn:
            if perm is not None:
                raise ValueError("DeviceRolloutBuffer.get: perm and drawn=True exclude each other")
            total = self.n_steps * self.n_envs
            B = total if batch_size is None else int(batch_size)
            if B < 1 or total % B:
                raise ValueError(f"DeviceRolloutBuffer.get: drawn=True needs a batch_size that divides {total}, got {batch_size}")
            for _ in range(total // B):
                yield self.next_batch(B)
            return
        if perm is None:
            with torch.cuda.device(self.engine.device):
                perm = torch.randperm(self.n_steps * self.n_envs, device=self.engine.device)
        for obs, outs in self.engine.minibatches(perm, batch_size, obs=self.observations, columns=self._batch_columns()):
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
