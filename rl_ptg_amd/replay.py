"""DeviceReplayBuffer: the replay buffer the reference's off-policy algorithms (DQN, TD3, SAC, TQC) train from, resident on the GPU.

It restates stable-baselines3 2.0.0a13 common/buffers.py ReplayBuffer (optimize_memory_usage off) over torch tensors that never leave
the device: add() and sample() each enqueue kernels of csrc/ptg_train.hip (ptg_replay_add, ptg_replay_sample in include/ptg_env.h) on
the current stream, without synchronisation, so a collect -> store -> sample step can be captured into one graph behind
HipEngine.step().  The write position lives on the device (cursor), like the step count of the hot kernels.
"""
import collections

ReplayStorage = collections.namedtuple("ReplayStorage", ["obs_ring", "next_ring", "col_rings", "cursor"])
ReplaySamples = collections.namedtuple("ReplaySamples", ["observations", "actions", "next_observations", "dones", "rewards"])


class DeviceReplayBuffer:
    def __init__(self, engine, buffer_size, columns=None, seed=0):
        """buffer_size transitions over engine.n envs: S = max(buffer_size // n_envs, 1) rows (SB3's rule).  columns: name -> torch
        dtype of the per-transition columns beside the observations; "actions" is required (default: int64 for a discrete engine,
        float32 for a continuous one), "rewards" (the engine's out_dtype, stored raw) and "dones" (float32 0 / 1, SB3's dtype) are
        always kept; at most 8 in all.  seed keys the device-drawn sample indices."""
        import torch
        self._torch = torch
        self.engine = engine
        self.n_envs = engine.n
        self.buffer_size = max(int(buffer_size) // engine.n, 1)
        self.seed = int(seed)
        cols = dict(columns) if columns is not None else {"actions": torch.float32 if engine.action_type == 1 else torch.int64}
        if "actions" not in cols:
            raise ValueError("DeviceReplayBuffer: columns must name 'actions'")
        if "rewards" in cols or "dones" in cols:
            raise ValueError("DeviceReplayBuffer: 'rewards' and 'dones' are kept by the buffer itself")
        cols["rewards"] = engine.out_dtype
        cols["dones"] = torch.float32
        self.columns = cols
        self.names = list(cols)
        S, N, F = self.buffer_size, engine.n, engine.obs_dim
        with torch.cuda.device(engine.device):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=engine.device)
            self.storage = ReplayStorage(z((S, N, F), engine.out_dtype), z((S, N, F), engine.out_dtype),
                                         [z((S, N), dt) for dt in cols.values()], z((2,), torch.int64))
        self._done_col = self.names.index("dones")
        self._rew_col = self.names.index("rewards")

    # views with SB3's names
    observations = property(lambda self: self.storage.obs_ring)
    next_observations = property(lambda self: self.storage.next_ring)

    def column(self, name):
        return self.storage.col_rings[self.names.index(name)]

    def add(self, prev_obs, obs, rewards, dones, final_obs=None, **columns):
        """Store the steps HipEngine.step() (tensors [N]-shaped, obs an engine-layout [N, F] / [F, N] buffer) or rollout() ([T, N],
        [T, ...]) left: prev_obs is the observation the (first) action was chosen from, final_obs the terminal observations (step()'s
        final_obs; without it a finished env's next observation is the post-reset one), columns the other columns by name.
        Enqueues on the current stream; nothing is copied to the host."""
        eng = self.engine
        one = obs.dim() == 2
        lift = lambda x: x.unsqueeze(0) if one and x is not None else x
        extra = sorted(set(columns) ^ set(self.names[:-2]))
        if extra:
            raise ValueError(f"DeviceReplayBuffer.add: columns given and columns kept differ in {extra}")
        for x in (prev_obs, obs) + ((final_obs,) if final_obs is not None else ()):
            eng._check_obs(x)
        cols = [lift(columns[k]) for k in self.names[:-2]] + [lift(rewards), None]
        eng.replay_add(self.storage, eng.rows(prev_obs), eng.rows(lift(obs)), cols, done=lift(dones),
                       final_obs=None if final_obs is None else eng.rows(lift(final_obs)), done_col=self._done_col)

    def sample(self, batch_size=None, idx=None, normalize_reward=False, extras=False, out=None):
        """SB3's ReplayBuffer.sample: a ReplaySamples of observations, next_observations [B, F] and actions, dones, rewards [B, 1].
        idx: explicit int64 flat indices (slot * n_envs + env); without it batch_size indices are drawn on the device, a fresh
        batch per call (and per replay of a captured call).  normalize_reward: SB3's _normalize_reward with the engine's current
        vn_* statistics.  extras: also return a dict of the other columns ([B, 1]) and "indices" ([B]).  out: the raw output tuple
        of an earlier call's HipEngine.replay_sample to write into."""
        o0, o1, outs, io = self.engine.replay_sample(self.storage, batch_size, idx, seed=self.seed, want_idx=extras,
                                                    norm_col=self._rew_col if normalize_reward else -1, out=out)
        by = {k: x.view(-1, 1) for k, x in zip(self.names, outs)}
        res = ReplaySamples(o0, by["actions"], o1, by["dones"], by["rewards"])
        if not extras:
            return res
        rest = {k: v for k, v in by.items() if k not in ("actions", "dones", "rewards")}
        rest["indices"] = io
        return res, rest

    def cursor(self):
        """(vector steps added since creation, batches drawn on the device); synchronises"""
        a, c = self.storage.cursor.cpu().tolist()
        return int(a), int(c)

    def size(self):
        """live rows (of n_envs transitions each): SB3's `buffer_size if full else pos`; synchronises"""
        return min(self.cursor()[0], self.buffer_size)

    @property
    def pos(self):
        return self.cursor()[0] % self.buffer_size

    @property
    def full(self):
        return self.cursor()[0] >= self.buffer_size

    def state_dict(self):
        """What save_replay_buffer pickles: the rings and the position, as NumPy arrays / plain numbers (synchronises)."""
        st = self.storage
        return {"buffer_size": self.buffer_size, "n_envs": self.n_envs, "seed": self.seed, "cursor": list(self.cursor()),
                "observations": st.obs_ring.cpu().numpy(), "next_observations": st.next_ring.cpu().numpy(),
                "columns": {k: x.cpu().numpy() for k, x in zip(self.names, st.col_rings)}}

    def load_state_dict(self, sd):
        """Inverse of state_dict() on a buffer built with the same engine shape, size and columns."""
        torch = self._torch
        st = self.storage
        if sd["buffer_size"] != self.buffer_size or sd["n_envs"] != self.n_envs or list(sd["columns"]) != self.names:
            raise ValueError("DeviceReplayBuffer.load_state_dict: the checkpoint's shape or columns differ from this buffer's")
        st.obs_ring.copy_(torch.from_numpy(sd["observations"]))
        st.next_ring.copy_(torch.from_numpy(sd["next_observations"]))
        for k, x in zip(self.names, st.col_rings):
            x.copy_(torch.from_numpy(sd["columns"][k]))
        st.cursor.copy_(torch.tensor(sd["cursor"], dtype=torch.int64))
        self.seed = int(sd["seed"])
