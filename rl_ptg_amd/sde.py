"""SdeNoise: the exploration state of gSDE (SB3's `use_sde`, the reference's agent switch `gSDE : True`) for the on-policy algorithms,
resident on the GPU.

It holds what stable-baselines3 2.0.0a13 common/distributions.py StateDependentNoiseDistribution keeps between steps -- the exploration
matrices, one [L] row per env, since the env's Box has one dimension -- and the device counter their draws are keyed by.  reset_noise()
is sample_weights (HipEngine.sde_resample; include/ptg_env.h: ptg_sde_resample), act() is proba_distribution followed by sample / mode,
log_prob and entropy in one launch (HipEngine.sde_act; ptg_sde_act).  Both enqueue on the current stream without synchronisation or
allocation, so a collect step -- DeviceMLP(hidden=True) -> act() -> HipEngine.step() -> DeviceRolloutBuffer.add() -- can be captured
into one graph and replayed; reset_noise() between replays refills the matrix in place.  When to call it (the start of every rollout and
every sde_sample_freq steps) stays the caller's schedule.  Training is rl_ptg_amd.ppo_sde_loss / a2c_sde_loss.

SquashedSdeNoise is the same for SAC and TQC, whose actor (sac/policies.py::Actor with use_sde) squashes the sample, clips the mean with
a Hardtanh at clip_mean and learns the features: besides the per-env matrix it holds the ONE [L] row that SAC.train / TQC.train
resample once per gradient step (actor.reset_noise() with batch_size 1), with a counter of its own and the seed
(seed XOR 0x9E3779B97F4A7C15), so that at equal seed the training row never repeats a collecting row.  Training is
rl_ptg_amd.sde_squashed_rsample."""

TRAIN_SEED_XOR = 0x9E3779B97F4A7C15                         # the training row's key stream: its own counter and seed ^ this constant


class SdeNoise:
    def __init__(self, engine, latent_dim, seed=0, dtype=None):
        """latent_dim: the width L of the policy's last hidden layer, 1 to 1024; dtype: torch.float32 (the default: what DeviceMLP
        leaves) or torch.float64, the dtype of the means, the latent and log_std"""
        from . import _lib
        torch = self._torch = engine._torch
        self.engine = engine
        self.latent_dim = int(latent_dim)
        if not 1 <= self.latent_dim <= _lib.MLP_MAX_WIDTH:
            raise ValueError(f"SdeNoise: latent_dim must be in [1, {_lib.MLP_MAX_WIDTH}], got {latent_dim}")
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"SdeNoise: dtype must be torch.float32 or torch.float64, got {dtype}")
        self.seed = int(seed) & (2 ** 64 - 1)
        with torch.cuda.device(engine.device):
            self.matrix = torch.zeros((engine.n, self.latent_dim), dtype=self.dtype, device=engine.device)
            self.counter = engine.new_draw_counter()
            self._out = engine.sde_act_outputs(self.dtype)

    def reset_noise(self, log_std):
        """SB3's reset_noise(): refill the exploration matrix from log_std [L] / [L, 1] as it is on the device now; the counter moves on"""
        self.engine.sde_resample(log_std, self.counter, self.matrix, seed=self.seed)

    def act(self, mean, latent, log_std, deterministic=False, clip=(-1.0, 1.0)):
        """-> SdeAct(actions float32 [N] clipped for step(), raw (unclipped: what the rollout buffer stores), log_prob, entropy) of the
        policy's means [N] / [N, 1] and its latent [N, L]; the four tensors are this object's own and the next call overwrites them"""
        return self.engine.sde_act(mean, latent, log_std, None if deterministic else self.matrix, clip=clip, deterministic=deterministic, out=self._out)

    def state_dict(self):
        """seed, counter and matrix on the host; synchronises"""
        return {"seed": self.seed, "counter": int(self.counter.item()), "matrix": self.matrix.cpu()}

    def load_state_dict(self, state):
        m = state["matrix"]
        if tuple(m.shape) != tuple(self.matrix.shape) or m.dtype != self.matrix.dtype:
            raise ValueError(f"SdeNoise.load_state_dict: matrix must be {tuple(self.matrix.shape)} of {self.matrix.dtype}, got {tuple(m.shape)} of {m.dtype}")
        self.seed = int(state["seed"]) & (2 ** 64 - 1)
        self.counter.fill_(int(state["counter"]))
        self.matrix.copy_(m)


class SquashedSdeNoise:
    def __init__(self, engine, latent_dim, seed=0, clip_mean=2.0, dtype=None):
        """latent_dim: the width L of the actor's trunk, 1 to 1024; clip_mean: SB3's default 2.0, float("inf") for none; dtype:
        torch.float32 (the default) or torch.float64, the dtype of the means, the latent and log_std"""
        from . import _lib
        torch = self._torch = engine._torch
        self.engine = engine
        self.latent_dim = int(latent_dim)
        if not 1 <= self.latent_dim <= _lib.MLP_MAX_WIDTH:
            raise ValueError(f"SquashedSdeNoise: latent_dim must be in [1, {_lib.MLP_MAX_WIDTH}], got {latent_dim}")
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"SquashedSdeNoise: dtype must be torch.float32 or torch.float64, got {dtype}")
        self.clip_mean = float(clip_mean)
        if not self.clip_mean > 0.0:
            raise ValueError(f"SquashedSdeNoise: clip_mean must be > 0 (float('inf'): no clipping), got {clip_mean}")
        self.seed = int(seed) & (2 ** 64 - 1)
        with torch.cuda.device(engine.device):
            self.matrix = torch.zeros((engine.n, self.latent_dim), dtype=self.dtype, device=engine.device)
            self.train_row = torch.zeros(self.latent_dim, dtype=self.dtype, device=engine.device)
            self.counter = engine.new_draw_counter()
            self.train_counter = engine.new_draw_counter()
            self._out = (torch.zeros(engine.n, dtype=self.dtype, device=engine.device), torch.zeros(engine.n, dtype=torch.float32, device=engine.device), None, None)

    @property
    def train_seed(self):
        return self.seed ^ TRAIN_SEED_XOR

    def reset_noise(self, log_std):
        """SB3's reset_noise(n_envs) while collecting: refill the per-env matrix from log_std [L] / [L, 1]; the collecting counter moves on"""
        self.engine.sde_resample(log_std, self.counter, self.matrix, seed=self.seed)

    def reset_train_noise(self, log_std):
        """SB3's actor.reset_noise() in SAC.train / TQC.train: redraw the one row every batch row shares; the training counter moves on"""
        self.engine.sde_resample_rows(log_std, self.train_counter, self.train_row, seed=self.train_seed)

    def act(self, mean, latent, log_std, deterministic=False):
        """the collecting head -> SdeRSample(actions [N] in dtype, step_actions float32 [N]: what step() takes, None, None) of the actor's
        unclipped means [N] / [N, 1] and its latent [N, L]; the tensors are this object's own and the next call overwrites them"""
        return self.engine.sde_rsample(mean, latent, log_std, None if deterministic else self.matrix, clip_mean=self.clip_mean,
                                       deterministic=deterministic, out=self._out)

    def state_dict(self):
        """seed, both counters and both matrices on the host; synchronises"""
        return {"seed": self.seed, "counter": int(self.counter.item()), "matrix": self.matrix.cpu(),
                "train_counter": int(self.train_counter.item()), "train_row": self.train_row.cpu()}

    def load_state_dict(self, state):
        for name, own in (("matrix", self.matrix), ("train_row", self.train_row)):
            m = state[name]
            if tuple(m.shape) != tuple(own.shape) or m.dtype != own.dtype:
                raise ValueError(f"SquashedSdeNoise.load_state_dict: {name} must be {tuple(own.shape)} of {own.dtype}, got {tuple(m.shape)} of {m.dtype}")
        self.seed = int(state["seed"]) & (2 ** 64 - 1)
        self.counter.fill_(int(state["counter"]))
        self.train_counter.fill_(int(state["train_counter"]))
        self.matrix.copy_(state["matrix"])
        self.train_row.copy_(state["train_row"])
