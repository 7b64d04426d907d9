"""HipEngine: the batched PtG env state on one MI355X, driven through the C ABI (include/ptg_env.h).

PyTorch is plumbing here: it owns the observation / reward / done / action buffers (ROCm tensors whose
data_ptr() is handed to the library) and the HIP stream; all env arithmetic runs in the hand-written
kernels of csrc/ptg_env.hip.  There is no CPU path: constructing an engine without the extension or
without a GPU raises.

`consts` uses the key names of the reference's env kwargs (src/rl_utils.py:345-365) with the two strings
already mapped to ints: raw_modified {0 raw, 1 mod}, action_type {0 discrete, 1 continuous},
train_or_eval {0 train, 1 eval}.  `markets` is a list (one per business scenario in the batch) of dicts
with el, pot_rew, part_full, gas, eua (1-D float64), scenario, rew_l_b, rew_u_b, r_0.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib

TABLE_KEYS = ["startup_cold", "startup_hot", "cooldown", "standby_down", "standby_up",
              "op1_start_p", "op2_start_f", "op3_p_f", "op4_p_f_p_5", "op5_p_f_p_10",
              "op6_p_f_p_15", "op7_p_f_p_22", "op8_f_p", "op9_f_p_f_5", "op10_f_p_f_10",
              "op11_f_p_f_15", "op12_f_p_f_20"]
ACTIONS = ["standby", "cooldown", "startup", "partial_load", "full_load"]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# what the action heads return: device tensors [N]; a field that was not asked for (or that the head does not have) is None
CategoricalAct = collections.namedtuple("CategoricalAct", "actions log_prob entropy")
EpsGreedyAct = collections.namedtuple("EpsGreedyAct", "actions")
GaussianAct = collections.namedtuple("GaussianAct", "actions raw log_prob entropy")
# what policy_loss returns: stats float64 [8], the gradients w.r.t. the head's input, the values and (Gaussian head) log_std
PolicyLoss = collections.namedtuple("PolicyLoss", "stats grad_input grad_values grad_log_std")


class PtgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libptg_env error {code}: {msg}")
        self.code = code


class HipEngine:
    def __init__(self, consts, tables, markets, n_envs, device=0, out_dtype="float32", obs_layout="row", obs_pitch=None):
        """obs_pitch (obs_layout="feature" only): elements between two feature planes of the observation buffers -- None: n_envs (planes
        back to back, `[F, N]` contiguous); an int >= n_envs; or "auto": n_envs + 1 KiB worth of elements for float64 outputs whose plane
        stride would be a multiple of 64 KiB (power-of-two batches: planes 2^19 bytes apart run at 0.59 of the HBM peak, 0.70 with the
        pitch; float32 planes do not need it and run slower with one -- profiles/r03_fm_pitch.txt; include/ptg_env.h ptg_set_feature_pitch).  With a pitch the observation tensors are `[F, N]` VIEWS of `[F, pitch]` storage."""
        import torch
        self._torch = torch
        self._L = _lib.lib()                      # raises if the extension is missing
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs a ROCm GPU (torch.cuda.is_available() is False); rl_ptg_amd has no CPU path")
        self.n = int(n_envs)
        self._fin_buf = None
        self.device = torch.device("cuda", int(device))
        self.out_dtype = {"float32": torch.float32, "float64": torch.float64}[out_dtype]
        cfg = _lib.PtgConfig()
        c = dict(consts)
        c.setdefault("t_cat_initial", 16.0)
        c["out_dtype"] = _lib.OUT_F64 if out_dtype == "float64" else _lib.OUT_F32
        c["obs_layout"] = {"row": _lib.OBS_ROW_MAJOR, "feature": _lib.OBS_FEATURE_MAJOR, "sb3_flat": _lib.OBS_SB3_FLAT,
                           "split": _lib.OBS_SPLIT}[obs_layout]
        self.feature_major = obs_layout == "feature"
        for k in _lib.CONFIG_KEYS:
            setattr(cfg, k, c[k])
        self.consts = c
        self._keep = []
        tb = _lib.PtgTables()
        for t, k in enumerate(TABLE_KEYS):
            a = np.ascontiguousarray(tables[k], dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 7:
                raise ValueError(f"table {k}: expected [rows, 7], got {a.shape}")
            self._keep.append(a)
            tb.data_host[t] = _dp(a)
            tb.rows[t] = a.shape[0]
        if isinstance(markets, dict):
            markets = [markets]
        mk = (_lib.PtgMarket * len(markets))()
        for s, m in enumerate(markets):
            arrs = {k: np.ascontiguousarray(m[k], dtype=np.float64) for k in ("el", "pot_rew", "part_full", "gas", "eua")}
            if not (len(arrs["el"]) == len(arrs["pot_rew"]) == len(arrs["part_full"])) or len(arrs["gas"]) != len(arrs["eua"]):
                raise ValueError("market series lengths differ")
            self._keep.extend(arrs.values())
            mk[s].n_hours, mk[s].n_days = len(arrs["el"]), len(arrs["gas"])
            mk[s].el_host, mk[s].pot_rew_host, mk[s].part_full_host = _dp(arrs["el"]), _dp(arrs["pot_rew"]), _dp(arrs["part_full"])
            mk[s].gas_host, mk[s].eua_host = _dp(arrs["gas"]), _dp(arrs["eua"])
            mk[s].scenario = int(m["scenario"])
            mk[s].rew_l_b, mk[s].rew_u_b, mk[s].r_0 = float(m["rew_l_b"]), float(m["rew_u_b"]), float(m["r_0"])
        self.n_sets = len(markets)
        h = C.c_void_p()
        rc = self._L.ptg_create(C.byref(cfg), C.byref(tb), mk, len(markets), self.n, int(device), C.byref(h))
        if rc != 0:
            raise PtgError(rc, self._L.ptg_last_error(None).decode())
        self._h = h
        self.obs_dim = self._L.ptg_obs_dim(h)
        osz = 8 if out_dtype == "float64" else 4
        if obs_pitch == "auto":
            pad = 1024                                                    # bytes (profiles/r03_fm_pitch.txt)
            obs_pitch = self.n + pad // osz if (self.feature_major and osz == 8 and (self.n * osz) % 65536 == 0) else None
        self.pitch = self.n if obs_pitch is None else int(obs_pitch)
        if self.pitch != self.n:
            if not self.feature_major:
                raise ValueError("obs_pitch applies to obs_layout='feature' only")
            self._chk(self._L.ptg_set_feature_pitch(h, self.pitch))
        self.action_type = int(c["action_type"])
        self.eval_mode = bool(c["train_or_eval"])
        with torch.cuda.device(self.device):
            self.obs = self.alloc_obs(zero=True)
            self.final_obs = self.alloc_obs(zero=True)
            self.rew = torch.zeros(self.n, dtype=self.out_dtype, device=self.device)
            self.done = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            self.info = torch.zeros((self.n, _lib.N_INFO), dtype=torch.float64, device=self.device) if self.eval_mode else None

    # ------------------------------------------------------------------ plumbing
    def alloc_obs(self, T=None, zero=False):
        """An observation buffer in this engine's layout: [N, F] row-major, [F, N] feature-major (a view of [F, pitch] storage when the
        engine has a pitch); with T: [T, ...] for a rollout."""
        torch = self._torch
        make = torch.zeros if zero else torch.empty
        lead = () if T is None else (int(T),)
        if not self.feature_major:
            return make(lead + (self.n, self.obs_dim), dtype=self.out_dtype, device=self.device)
        t = make(lead + (self.obs_dim, self.pitch), dtype=self.out_dtype, device=self.device)
        return t[..., :self.n] if self.pitch != self.n else t

    def _check_obs(self, obs):
        """a caller-supplied feature-major buffer must have the engine's plane pitch (and a contiguous env axis)"""
        if self.feature_major:
            ok = obs.stride(-1) == 1 and obs.stride(-2) == self.pitch and (obs.dim() == 2 or obs.stride(0) == self.obs_dim * self.pitch)
        else:
            ok = obs.is_contiguous()
        if not ok:
            raise ValueError(f"observation buffer strides {tuple(obs.stride())} do not match the engine's layout (pitch {self.pitch}); use alloc_obs()")

    def close(self):
        if getattr(self, "_h", None):
            self._L.ptg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise PtgError(rc, self._L.ptg_last_error(self._h).decode())

    def rows(self, obs):
        """[N, F] (or [T, N, F]) view of an observation buffer in either layout (a transpose view for feature-major)."""
        return obs.transpose(-1, -2) if self.feature_major else obs

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _action_kind(self, t):
        torch = self._torch
        if t.dtype == torch.int32:
            return _lib.ACT_I32
        if t.dtype == torch.int64:
            return _lib.ACT_I64
        if t.dtype == torch.float32:
            return _lib.ACT_F32
        raise TypeError(f"actions must be int32 / int64 / float32, got {t.dtype}")

    def as_device_actions(self, actions):
        """numpy / torch actions -> contiguous device tensor of a dtype the kernels read."""
        torch = self._torch
        if not torch.is_tensor(actions):
            a = np.asarray(actions)
            a = a.astype(np.float32) if self.action_type == 1 else a.astype(np.int32)
            actions = torch.from_numpy(np.ascontiguousarray(a))
        if actions.device != self.device:
            actions = actions.to(self.device, non_blocking=True)
        if self.action_type == 1 and actions.dtype != torch.float32:
            actions = actions.float()
        return actions.contiguous()

    # ------------------------------------------------------------------ configuration
    def set_market_assignment(self, set_of_env):
        a = np.ascontiguousarray(set_of_env, dtype=np.uint8)
        assert a.shape == (self.n,)
        self._chk(self._L.ptg_set_market_assignment(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_episode_plan(self, eps_ind, first_ptr, stride):
        if eps_ind is None or len(eps_ind) == 0:
            self._chk(self._L.ptg_set_episode_plan(self._h, None, 0, 0, 0))
            return
        a = np.ascontiguousarray(eps_ind, dtype=np.float64)
        self._chk(self._L.ptg_set_episode_plan(self._h, _dp(a), len(a), int(first_ptr), int(stride)))

    def set_noise_tape(self, tape):
        if tape is None:
            self._chk(self._L.ptg_set_noise_tape(self._h, None, 0))
            self._noise_cfg = {"mode": "none"}
            return
        a = np.ascontiguousarray(tape, dtype=np.float64)
        assert a.ndim == 2 and a.shape[0] == self.n
        self._chk(self._L.ptg_set_noise_tape(self._h, _dp(a), a.shape[1]))
        self._noise_cfg = {"mode": "tape", "per_env_len": int(a.shape[1])}

    def set_noise_rng(self, seed):
        """Draw the state-change noise inside the kernels from the counter-based generator (no tape)."""
        self._chk(self._L.ptg_set_noise_rng(self._h, int(seed) & (2 ** 64 - 1)))
        self._noise_cfg = {"mode": "rng", "seed": int(seed) & (2 ** 64 - 1)}

    def set_global_env_offset(self, offset):
        self._chk(self._L.ptg_set_global_env_offset(self._h, int(offset)))
        self._env_offset = int(offset)

    def fill_noise_tape(self, seed, per_env_len):
        self._chk(self._L.ptg_fill_noise_tape(self._h, int(seed) & (2 ** 64 - 1), int(per_env_len), self._stream()))
        self.tape_len = int(per_env_len)
        self._noise_cfg = {"mode": "tape", "per_env_len": int(per_env_len)}

    def get_noise_tape(self, per_env_len):
        out = np.zeros((self.n, per_env_len))
        self._chk(self._L.ptg_get_noise_tape(self._h, _dp(out)))
        return out

    # ------------------------------------------------------------------ hot path
    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert m.shape == (self.n,)
        with self._torch.cuda.device(self.device):
            self._chk(self._L.ptg_reset(self._h, None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        C.c_void_p(self.obs.data_ptr()), self._stream()))
        return self.obs

    def step(self, actions, obs=None, rew=None, done=None, final_obs=None, want_final=True):
        """Enqueue one vector step on the current stream; returns (obs, rew, done) device tensors (no sync)."""
        a = self.as_device_actions(actions)
        assert a.numel() == self.n
        if obs is not None:
            self._check_obs(obs)
        if final_obs is not None:
            self._check_obs(final_obs)
        obs = self.obs if obs is None else obs
        rew = self.rew if rew is None else rew
        done = self.done if done is None else done
        fo = (self.final_obs if final_obs is None else final_obs) if want_final else None
        with self._torch.cuda.device(self.device):
            self._chk(self._L.ptg_step(self._h, C.c_void_p(a.data_ptr()), self._action_kind(a), C.c_void_p(obs.data_ptr()),
                                       C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()),
                                       C.c_void_p(fo.data_ptr()) if fo is not None else None,
                                       C.c_void_p(self.info.data_ptr()) if self.info is not None else None, self._stream()))
        return obs, rew, done

    def rollout(self, actions, obs=None, rew=None, done=None):
        """T fused steps in one launch: actions [T, N] -> obs [T, N, F] ([T, F, N] feature-major), rew [T, N], done [T, N]."""
        torch = self._torch
        a = self.as_device_actions(actions)
        assert a.dim() == 2 and a.shape[1] == self.n
        T = a.shape[0]
        with torch.cuda.device(self.device):
            if obs is None:
                obs = self.alloc_obs(T)
            else:
                self._check_obs(obs)
            if rew is None:
                rew = torch.empty((T, self.n), dtype=self.out_dtype, device=self.device)
            if done is None:
                done = torch.empty((T, self.n), dtype=torch.uint8, device=self.device)
            self._chk(self._L.ptg_rollout(self._h, C.c_void_p(a.data_ptr()), self._action_kind(a), T, C.c_void_p(obs.data_ptr()),
                                          C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), self._stream()))
        return obs, rew, done

    def rollout_info(self, actions):
        """T steps with the 24 `_get_info` fields of every step recorded on the device: returns (obs, rew, done, info) with
        info [T, N, 24] float64 in the key order of rl_ptg_amd.vec_env.INFO_KEYS (what Postprocessing.test_performance gathers
        from per-step info dicts, src/rl_utils.py:528-565)."""
        torch = self._torch
        a = self.as_device_actions(actions)
        assert a.dim() == 2 and a.shape[1] == self.n
        T = a.shape[0]
        with torch.cuda.device(self.device):
            obs = self.alloc_obs(T)
            rew = torch.empty((T, self.n), dtype=self.out_dtype, device=self.device)
            done = torch.empty((T, self.n), dtype=torch.uint8, device=self.device)
            info = torch.empty((T, self.n, 24), dtype=torch.float64, device=self.device)
            self._chk(self._L.ptg_rollout_info(self._h, C.c_void_p(a.data_ptr()), self._action_kind(a), T, C.c_void_p(obs.data_ptr()),
                                               C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), C.c_void_p(info.data_ptr()), self._stream()))
        return obs, rew, done, info

    def rollout_launches(self, n_steps):
        """Kernel launches a rollout of n_steps would issue from the envs' current position (per-launch timing)."""
        k = self._L.ptg_rollout_launches(self._h, int(n_steps))
        if k < 0:
            self._chk(k)
        return k

    def profile(self, enable=True):
        """Start / stop collecting the device time of every hot-kernel launch (kernel-attached HIP events)."""
        self._chk(self._L.ptg_profile(self._h, 1 if enable else 0))

    def profile_read(self, cap=65536):
        """Durations [us] of the launches recorded since profile(True), in launch order; waits for them and clears the list."""
        out = np.zeros(cap)
        cnt = C.c_int(0)
        self._chk(self._L.ptg_profile_read(self._h, _dp(out), cap, C.byref(cnt)))
        return out[:cnt.value].copy()

    def profile_read_ex(self, cap=65536):
        """profile_read with each launch's helper kernel (the table refresher beside it) accounted for: (us, helper_us, span_us),
        span = first start to last end of the launch and its helper (include/ptg_env.h, ptg_profile_read_ex)."""
        us, hp, sp = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        cnt = C.c_int(0)
        self._chk(self._L.ptg_profile_read_ex(self._h, _dp(us), _dp(hp), _dp(sp), cap, C.byref(cnt)))
        n = cnt.value
        return us[:n].copy(), hp[:n].copy(), sp[:n].copy()

    def finished_dropped(self):
        """Finished episodes that were never handed out (ring overflow / a query's cap) since the engine was created."""
        d = C.c_uint64(0)
        self._chk(self._L.ptg_finished_dropped(self._h, C.byref(d)))
        return int(d.value)

    def steps_to_episode_end(self):
        """Vector steps from now up to and including the one on which a synchronised batch's episodes end; 0 = unknown to the
        host (de-synchronised batch).  Pure host bookkeeping: no device call."""
        s = C.c_int(0)
        self._chk(self._L.ptg_steps_to_episode_end(self._h, C.byref(s)))
        return int(s.value)

    def note_replays(self, n_steps):
        """Tell the handle how far replays of captured launches advanced the batch (include/ptg_env.h, "hipGraph capture"): `n_steps` =
        the vector steps of ALL replays minus those of one replay, because the capture call already counted as one execution -- R replays
        of a captured step: R - 1; R replays of a captured T-step rollout: (R - 1) * T.  step() / rollout() captured into a graph can be
        replayed because the kernels read the step count from the device state; the host-side count that routes an episode's terminating
        step only sees eager calls and the capture itself.  On a de-synchronised batch it only marks finished episodes as possible."""
        self._chk(self._L.ptg_note_replays(self._h, int(n_steps)))

    def set_replay_proof(self, enable=True):
        """A step() captured into a graph AFTER this call replays across episode ends by itself (hot kernel + generic kernel, one of them a
        no-op per step: +1.5-2 us); without it a captured step must stop before the episode's terminating step (include/ptg_env.h)."""
        self._chk(self._L.ptg_set_replay_proof(self._h, 1 if enable else 0))

    def sync(self):
        self._chk(self._L.ptg_sync(self._h, self._stream()))

    # ------------------------------------------------------------------ state access
    def get_state(self, name):
        f = _lib.STATE_FIELDS[name]
        out = np.zeros(self.n, np.float64 if f >= 32 else np.int32)
        self._chk(self._L.ptg_get_state(self._h, f, C.c_void_p(out.ctypes.data)))
        return out

    def set_state(self, name, values):
        f = _lib.STATE_FIELDS[name]
        a = np.ascontiguousarray(values, dtype=np.float64 if f >= 32 else np.int32)
        assert a.shape == (self.n,)
        self._chk(self._L.ptg_set_state(self._h, f, C.c_void_p(a.ctypes.data)))

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        """Everything a resumed run needs beyond the constructor arguments and the episode plan: every per-env state field,
        the noise source, the global env offset and -- if started -- the reward normaliser with its hyper-parameters (NumPy arrays /
        plain numbers; synchronises).  Not included: the list of finished episodes not yet collected (ptg_finished_episodes)."""
        sd = {"fields": {k: self.get_state(k) for k in _lib.STATE_FIELDS}, "n": self.n,
              "env_offset": self.__dict__.get("_env_offset", 0)}       # keys the in-kernel RNG streams (global env index)
        sd["noise"] = dict(self.__dict__.get("_noise_cfg", {"mode": "none"}))
        if sd["noise"].get("mode") == "tape":
            sd["noise"]["tape"] = self.get_noise_tape(sd["noise"]["per_env_len"])
        try:
            st, ret = self.vn_get()
            sd["vn"] = {"stats": st, "returns": ret, "hyper": dict(self.__dict__.get("_vn_hyper", {}))}
        except PtgError:
            pass
        return sd

    def load_state_dict(self, sd):
        """Inverse of state_dict() on an engine built with the same arguments (reset() first, then the episode plan)."""
        assert sd["n"] == self.n
        if "env_offset" in sd:
            self.set_global_env_offset(sd["env_offset"])
        nz = sd.get("noise", {})
        if nz.get("mode") == "rng":
            self.set_noise_rng(nz["seed"])
        elif nz.get("mode") == "tape":
            self.set_noise_tape(nz["tape"])
        for k, v in sd["fields"].items():
            if k != "k":
                self.set_state(k, v)
        self.set_state("k", sd["fields"]["k"])              # last: equal step counts mark the batch as synchronised again
        if "vn" in sd:
            hyper = sd["vn"].get("hyper") or {}
            if hyper and hyper != self.__dict__.get("_vn_hyper"):
                self.vn_init(**hyper)                           # the checkpoint's gamma / epsilon / clip_reward
            else:
                try:
                    self.vn_get()
                except PtgError:
                    self.vn_init()
            self.vn_set(stats=sd["vn"]["stats"], returns=sd["vn"]["returns"])

    def finished_episodes(self, cap=None):
        cap = max(2 * self.n, 1024) if cap is None else int(cap)          # the library's ring holds max(2 n, 1024) entries
        buf = self._fin_buf
        if buf is None or buf[0].shape[0] < cap:                          # receive buffers kept across calls (2 MB at 65 536 envs)
            buf = self._fin_buf = (np.zeros(cap), np.zeros(cap, np.int32), np.zeros(cap, np.int32))
        r, l, ids = buf
        cnt = C.c_int(0)
        self._chk(self._L.ptg_finished_episodes(self._h, _dp(r), l.ctypes.data_as(C.POINTER(C.c_int32)),
                                                ids.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(cnt)))
        n = cnt.value
        return r[:n].copy(), l[:n].copy(), ids[:n].copy()

    def finished_episodes_dev(self, block=None, append=False):
        """The device route out of the finished-episode ring: enqueue, on the current stream, the hand-over of the episodes finished
        since the last drain (or host query) into a rl_ptg_amd.dist.FinishedBlock on this GPU -- no synchronisation, no host copy, so
        it can be captured into a graph behind a replay-proof step().  block None: the engine's own block of cap n_envs, allocated
        once and reused (the fixed N/G of SURVEY.md 8e); append: entries go behind the block's count instead of replacing the list.
        Returns the block; its counts are valid once the stream has run (fin.count() synchronises).  finished_episodes() is the
        host query of the same ring: an episode leaves through whichever is called first."""
        from . import dist as ptg_dist
        if block is None:
            if self.__dict__.get("_fin_dev") is None:
                self._fin_dev = ptg_dist.FinishedBlock.empty(self.n, self.device)
            block = self._fin_dev
        if block.block.device != self.device:
            raise ValueError(f"the block lives on {block.block.device}, the engine on {self.device}")
        with self._torch.cuda.device(self.device):
            self._chk(self._L.ptg_finished_episodes_dev(self._h, C.c_void_p(block.returns.data_ptr()), C.c_void_p(block.lengths.data_ptr()),
                                                        C.c_void_p(block.env_ids.data_ptr()), block.cap, C.c_void_p(block.counts.data_ptr()),
                                                        1 if append else 0, self._stream()))
        return block

    def episode_stats_dev(self, fin, stats=None, accumulate=False):
        """Enqueue Monitor's statistic of a device list: float64[6] = {count, sum r, sum r^2, sum len, min r, max r} of `fin` (a
        FinishedBlock), written to `stats` (None: the engine's own tensor, which starts as the empty statistic) or, with accumulate,
        merged into it.  Deterministic (fixed reduction order).  ep_rew_mean = stats[1] / stats[0]."""
        torch = self._torch
        if stats is None:
            if self.__dict__.get("_fin_stats") is None:
                self._fin_stats = torch.tensor([0.0, 0.0, 0.0, 0.0, float("inf"), float("-inf")], dtype=torch.float64, device=self.device)
            stats = self._fin_stats
        assert stats.dtype == torch.float64 and stats.numel() == 6 and stats.is_contiguous() and stats.device == self.device
        with torch.cuda.device(self.device):
            self._chk(self._L.ptg_episode_stats_dev(self._h, C.c_void_p(fin.returns.data_ptr()), C.c_void_p(fin.lengths.data_ptr()),
                                                    C.c_void_p(fin.counts.data_ptr()), C.c_void_p(stats.data_ptr()),
                                                    1 if accumulate else 0, self._stream()))
        return stats

    # ------------------------------------------------------------------ VecNormalize(norm_obs=False) on the device
    def vn_init(self, gamma=0.99, epsilon=1e-8, clip_reward=10.0):
        """Start reward normalisation as the reference wraps its envs (src/rl_utils.py:453, SB3 defaults)."""
        self._chk(self._L.ptg_vn_init(self._h, float(gamma), float(epsilon), float(clip_reward)))
        self._vn_hyper = {"gamma": float(gamma), "epsilon": float(epsilon), "clip_reward": float(clip_reward)}

    def vn_normalize(self, rew, done, training=True, out=None, group=None):
        """Normalise a [T, N] (or [N]) reward tensor in place of VecNormalize.step_wait: advances the discounted returns,
        updates the running moments step by step (training=True) and returns the clipped, scaled rewards.  With an
        initialised torch.distributed process group the per-step moments of all ranks' envs are merged first (one
        all-gather per call), so every rank holds the statistics of the whole job."""
        torch = self._torch
        from . import dist as ptg_dist
        r2 = rew if rew.dim() == 2 else rew.unsqueeze(0)
        d2 = done if done.dim() == 2 else done.unsqueeze(0)
        T = r2.shape[0]
        assert r2.shape == (T, self.n) and d2.shape == (T, self.n) and r2.is_contiguous() and d2.is_contiguous()
        assert r2.dtype == self.out_dtype and d2.element_size() == 1, (r2.dtype, d2.dtype)    # what the kernels read
        res = torch.empty_like(r2) if out is None else (out if out.dim() == 2 else out.unsqueeze(0))
        with torch.cuda.device(self.device):
            mom = None
            if training:
                mom = torch.empty((T, 3), dtype=torch.float64, device=self.device)
                self._chk(self._L.ptg_vn_batch_moments(self._h, C.c_void_p(r2.data_ptr()), C.c_void_p(d2.data_ptr()), T,
                                                       C.c_void_p(mom.data_ptr()), self._stream()))
                mom = ptg_dist.all_merge_moments(mom, group=group)
            self._chk(self._L.ptg_vn_apply(self._h, C.c_void_p(r2.data_ptr()), T, C.c_void_p(mom.data_ptr()) if mom is not None else None,
                                           C.c_void_p(res.data_ptr()), 1 if training else 0, self._stream()))
            if not training:                                # frozen statistics: returns[done] = 0 all the same (SB3 step_wait)
                self._chk(self._L.ptg_vn_clear_done(self._h, C.c_void_p(d2.data_ptr()), T, self._stream()))
        return res if rew.dim() == 2 else res[0]

    def vn_get(self):
        st, ret = np.zeros(3), np.zeros(self.n)
        self._chk(self._L.ptg_vn_get(self._h, _dp(st), _dp(ret)))
        return dict(mean=st[0], var=st[1], count=st[2]), ret

    def vn_set(self, stats=None, returns=None):
        st = None if stats is None else np.array([stats["mean"], stats["var"], stats["count"]], dtype=np.float64)
        rt = None if returns is None else np.ascontiguousarray(returns, dtype=np.float64)
        self._chk(self._L.ptg_vn_set(self._h, None if st is None else _dp(st), None if rt is None else _dp(rt)))

    # ------------------------------------------------------------------ RolloutBuffer.compute_returns_and_advantage on the device
    def gae(self, rew, values, done, last_values, gamma, gae_lambda, adv=None, ret=None):
        """Enqueue, on the current stream, the advantages and returns of a rollout in place of SB3's
        RolloutBuffer.compute_returns_and_advantage (include/ptg_env.h: ptg_gae): rew, values [T, N] (or [N] for T = 1) and
        last_values [N] of ONE float dtype (float32 or float64, whatever the engine's out_dtype), done [T, N] of a 1-byte dtype with
        rollout()'s meaning (done[t] != 0: the episode ended on step t), values[t] = V of the observation step t's action was chosen
        from, last_values = V of the observation after step T - 1.  Returns (adv, ret), allocated when not given; adv may be rew and
        ret may be values.  No synchronisation; bit for bit what NumPy computes with SB3's lines on arrays of that dtype."""
        torch = self._torch
        one = rew.dim() == 1
        r2, v2, d2 = (x.unsqueeze(0) if one and x.dim() == 1 else x for x in (rew, values, done))
        T = r2.shape[0] if r2.dim() == 2 else -1
        if r2.shape != (T, self.n) or v2.shape != (T, self.n) or d2.shape != (T, self.n) or last_values.shape != (self.n,):
            raise ValueError(f"gae: expected rew / values / done [T, {self.n}] and last_values [{self.n}], got {tuple(rew.shape)}, "
                             f"{tuple(values.shape)}, {tuple(done.shape)}, {tuple(last_values.shape)}")
        if r2.dtype not in (torch.float32, torch.float64) or v2.dtype != r2.dtype or last_values.dtype != r2.dtype:
            raise TypeError(f"gae: rew, values and last_values must share float32 or float64, got {r2.dtype}, {v2.dtype}, {last_values.dtype}")
        if d2.element_size() != 1:
            raise TypeError(f"gae: done must have a 1-byte dtype, got {d2.dtype}")
        a2 = torch.empty_like(r2) if adv is None else (adv.unsqueeze(0) if one and adv.dim() == 1 else adv)
        t2 = torch.empty_like(r2) if ret is None else (ret.unsqueeze(0) if one and ret.dim() == 1 else ret)
        for name, x in (("adv", a2), ("ret", t2)):
            if x.shape != (T, self.n) or x.dtype != r2.dtype:
                raise ValueError(f"gae: {name} must be [{T}, {self.n}] of {r2.dtype}, got {tuple(x.shape)} of {x.dtype}")
        for name, x in (("rew", r2), ("values", v2), ("done", d2), ("last_values", last_values), ("adv", a2), ("ret", t2)):
            if not x.is_contiguous() or x.device != self.device:
                raise ValueError(f"gae: {name} must be a contiguous tensor on {self.device}")
        with torch.cuda.device(self.device):
            self._chk(self._L.ptg_gae(self._h, C.c_void_p(r2.data_ptr()), C.c_void_p(v2.data_ptr()), C.c_void_p(d2.data_ptr()),
                                      C.c_void_p(last_values.data_ptr()), T, _lib.OUT_F64 if r2.dtype == torch.float64 else _lib.OUT_F32,
                                      float(gamma), float(gae_lambda), C.c_void_p(a2.data_ptr()), C.c_void_p(t2.data_ptr()), self._stream()))
        return (a2[0], t2[0]) if one else (a2, t2)

    # ------------------------------------------------------------------ RolloutBuffer.get on the device
    def minibatch(self, idx, obs=None, columns=(), obs_out=None, columns_out=None):
        """Enqueue, on the current stream, the gather of ONE minibatch in place of SB3's RolloutBuffer._get_samples
        (include/ptg_env.h: ptg_minibatch): idx [B] int32 / int64 sample indices in swap_and_flatten's order, i = env * T + step,
        0 <= i < T * N (slices of a torch.randperm(T * N)); obs a rollout's observation buffer as alloc_obs(T) / rollout() make it
        ([T, N, F], or [T, F, N] feature-major with the engine's pitch); columns up to 8 contiguous [T, N] tensors of 1-, 2-, 4- or
        8-byte elements (actions, values, log-probs, advantages, returns, done flags ...).  Returns (obs_out [B, F] or None,
        [column outputs [B]]), allocated when not given; row b is source row (idx[b] % T, idx[b] // T), byte for byte.  Outputs must
        not overlap inputs (not checked).  No synchronisation; an index out of range leaves its row untouched and makes the next
        sync() raise PtgError with code PTG_E_INDEX."""
        torch = self._torch
        columns = list(columns)
        if not torch.is_tensor(idx) or idx.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"minibatch: idx must be an int32 or int64 tensor, got {getattr(idx, 'dtype', type(idx))}")
        if idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError(f"minibatch: idx must be 1-D and contiguous, got shape {tuple(idx.shape)}, strides {tuple(idx.stride())}")
        if obs is None and not columns:
            raise ValueError("minibatch: neither observations nor columns given")
        if len(columns) > _lib.MB_MAX_COLS:
            raise ValueError(f"minibatch: at most {_lib.MB_MAX_COLS} columns, got {len(columns)}")
        B = idx.shape[0]
        F = s_t = s_n = s_f = 0
        if obs is not None:
            if obs.dim() != 3 or obs.shape[1:] != ((self.obs_dim, self.n) if self.feature_major else (self.n, self.obs_dim)):
                raise ValueError(f"minibatch: obs must be a [T, ...] buffer of alloc_obs(T), got shape {tuple(obs.shape)}")
            if obs.element_size() not in (4, 8):
                raise TypeError(f"minibatch: obs must have 4- or 8-byte elements, got {obs.dtype}")
            self._check_obs(obs)
            T, F = obs.shape[0], self.obs_dim
            s_t, (s_n, s_f) = obs.stride(0), ((obs.stride(2), obs.stride(1)) if self.feature_major else (obs.stride(1), obs.stride(2)))
        else:
            T = columns[0].shape[0] if columns[0].dim() == 2 else -1
        for c, x in enumerate(columns):
            if x.shape != (T, self.n) or not x.is_contiguous():
                raise ValueError(f"minibatch: column {c} must be a contiguous [{T}, {self.n}] tensor, got shape {tuple(x.shape)}, strides {tuple(x.stride())}")
            if x.element_size() not in (1, 2, 4, 8):
                raise TypeError(f"minibatch: column {c} must have 1-, 2-, 4- or 8-byte elements, got {x.dtype}")
        if columns_out is not None and len(columns_out) != len(columns):
            raise ValueError(f"minibatch: {len(columns)} columns but {len(columns_out)} column outputs")
        if obs is None and obs_out is not None:
            raise ValueError("minibatch: obs_out given without obs")
        for name, x in [("idx", idx)] + ([("obs", obs)] if obs is not None else []) + [(f"column {c}", x) for c, x in enumerate(columns)]:
            if x.device != self.device:
                raise ValueError(f"minibatch: {name} lives on {x.device}, the engine on {self.device}")
        with torch.cuda.device(self.device):
            if obs is not None and obs_out is None:
                obs_out = torch.empty((B, F), dtype=obs.dtype, device=self.device)
            outs = [torch.empty((B,), dtype=x.dtype, device=self.device) for x in columns] if columns_out is None else list(columns_out)
            if obs is not None and (obs_out.shape != (B, F) or obs_out.dtype != obs.dtype or not obs_out.is_contiguous() or obs_out.device != self.device):
                raise ValueError(f"minibatch: obs_out must be a contiguous [{B}, {F}] tensor of {obs.dtype} on {self.device}, got "
                                 f"{tuple(obs_out.shape)} of {obs_out.dtype} on {obs_out.device}")
            for c, (x, o) in enumerate(zip(columns, outs)):
                if o.shape != (B,) or o.dtype != x.dtype or not o.is_contiguous() or o.device != self.device:
                    raise ValueError(f"minibatch: output of column {c} must be a contiguous [{B}] tensor of {x.dtype} on {self.device}, got "
                                     f"{tuple(o.shape)} of {o.dtype} on {o.device}")
            k = len(columns)
            src = (C.c_void_p * max(k, 1))(*[x.data_ptr() for x in columns])
            dst = (C.c_void_p * max(k, 1))(*[o.data_ptr() for o in outs])
            size = (C.c_int32 * max(k, 1))(*[x.element_size() for x in columns])
            self._chk(self._L.ptg_minibatch(self._h, C.c_void_p(idx.data_ptr()), idx.element_size(), B, T,
                                            C.c_void_p(obs.data_ptr()) if obs is not None else None, s_t, s_n, s_f, F,
                                            obs.element_size() if obs is not None else 0,
                                            C.c_void_p(obs_out.data_ptr()) if obs is not None else None, k, src, size, dst, self._stream()))
        return obs_out, outs

    def minibatches(self, perm, batch_size, obs=None, columns=()):
        """SB3's RolloutBuffer.get loop: yields minibatch(perm[start : start + batch_size], obs, columns) for start = 0, batch_size,
        ... -- the last slice short when batch_size does not divide len(perm); batch_size None: one batch of all of perm (A2C).
        perm: a permutation of T * N on the device, e.g. torch.randperm(T * N, device=...).  Every yield has fresh outputs."""
        total = perm.shape[0]
        if batch_size is None:
            batch_size = total
        if int(batch_size) < 1:
            raise ValueError(f"minibatches: batch_size must be >= 1 or None, got {batch_size}")
        start = 0
        while start < total:
            yield self.minibatch(perm[start:start + int(batch_size)], obs, columns)
            start += int(batch_size)

    # ------------------------------------------------------------------ ReplayBuffer.add / sample on the device
    def _replay_desc(self, st, who):
        """the ptg_replay descriptor of a storage object (rl_ptg_amd.replay.ReplayStorage: obs_ring, next_ring [S, N, F], col_rings
        [S, N] each, cursor uint64-as-int64 [2]), its tensors checked"""
        torch = self._torch
        o, nx, cols, cur = st.obs_ring, st.next_ring, list(st.col_rings), st.cursor
        if o.dim() != 3 or o.shape[1] != self.n or o.shape[0] < 1 or o.shape[2] < 1:
            raise ValueError(f"{who}: obs_ring must be [S, {self.n}, F], got shape {tuple(o.shape)}")
        if nx.shape != o.shape or nx.dtype != o.dtype:
            raise ValueError(f"{who}: next_ring must match obs_ring, got {tuple(nx.shape)} of {nx.dtype}")
        if o.element_size() not in (4, 8):
            raise TypeError(f"{who}: the observation rings must have 4- or 8-byte elements, got {o.dtype}")
        if len(cols) > _lib.MB_MAX_COLS:
            raise ValueError(f"{who}: at most {_lib.MB_MAX_COLS} column rings, got {len(cols)}")
        for c, x in enumerate(cols):
            if x.shape != o.shape[:2]:
                raise ValueError(f"{who}: column ring {c} must be [{o.shape[0]}, {self.n}], got shape {tuple(x.shape)}")
            if x.element_size() not in (1, 2, 4, 8):
                raise TypeError(f"{who}: column ring {c} must have 1-, 2-, 4- or 8-byte elements, got {x.dtype}")
        if cur.dtype != torch.int64 or cur.shape != (2,):
            raise TypeError(f"{who}: cursor must be an int64 tensor of 2 elements, got {cur.dtype} {tuple(cur.shape)}")
        for name, x in [("obs_ring", o), ("next_ring", nx), ("cursor", cur)] + [(f"column ring {c}", x) for c, x in enumerate(cols)]:
            if x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous tensor on {self.device}")
        d = _lib.PtgReplay()
        d.capacity, d.obs_dim, d.obs_bytes = o.shape[0], o.shape[2], o.element_size()
        d.obs_ring, d.next_ring, d.n_cols, d.cursor_dev = o.data_ptr(), nx.data_ptr(), len(cols), cur.data_ptr()
        for c, x in enumerate(cols):
            d.col_bytes[c], d.col_ring[c] = x.element_size(), x.data_ptr()
        return d

    def replay_add(self, storage, prev_obs, obs, columns=(), done=None, final_obs=None, done_col=-1):
        """Enqueue, on the current stream, SB3's ReplayBuffer.add for a window of T vector steps (include/ptg_env.h: ptg_replay_add).
        obs is the ROW VIEW [T, N, F] of the window's observations -- rows(buffer) for a feature-major engine; any non-negative
        strides -- prev_obs [N, F] the observation the first action was chosen from and final_obs (optional, [T, N, F]) the terminal
        observations, both with obs's strides; columns one contiguous [T, N] tensor per column ring, of the ring's dtype (None at
        done_col, which is written as float32 0 / 1 from done); done [T, N] of a 1-byte dtype.  Step t goes to slot
        (cursor[0] + t) % S; the cursor advances on the device.  No synchronisation."""
        torch = self._torch
        d = self._replay_desc(storage, "replay_add")
        columns = list(columns)
        F, ring_dt = storage.obs_ring.shape[2], storage.obs_ring.dtype
        if not torch.is_tensor(obs) or obs.dim() != 3 or obs.shape[1:] != (self.n, F):
            raise ValueError(f"replay_add: obs must be a [T, {self.n}, {F}] row view, got shape {tuple(getattr(obs, 'shape', ()))}")
        T = obs.shape[0]
        if T < 1 or T > storage.obs_ring.shape[0]:
            raise ValueError(f"replay_add: a window of {T} steps does not fit a buffer of {storage.obs_ring.shape[0]} rows (1 <= T <= S)")
        if not torch.is_tensor(prev_obs) or prev_obs.shape != (self.n, F) or tuple(prev_obs.stride()) != tuple(obs.stride()[1:]):
            raise ValueError(f"replay_add: prev_obs must be [{self.n}, {F}] with obs's strides {tuple(obs.stride()[1:])}, got "
                             f"{tuple(getattr(prev_obs, 'shape', ()))}, strides {tuple(prev_obs.stride()) if torch.is_tensor(prev_obs) else None}")
        if final_obs is not None and (final_obs.shape != obs.shape or tuple(final_obs.stride())[T == 1:] != tuple(obs.stride())[T == 1:]):
            raise ValueError(f"replay_add: final_obs must have obs's shape and strides, got {tuple(final_obs.shape)}, {tuple(final_obs.stride())}")
        views = [("obs", obs), ("prev_obs", prev_obs)] + ([("final_obs", final_obs)] if final_obs is not None else [])
        for name, x in views:
            if x.dtype != ring_dt:
                raise TypeError(f"replay_add: {name} is {x.dtype}, the rings hold {ring_dt}")
            if min(x.stride()) < 0:
                raise ValueError(f"replay_add: {name} has a negative stride")
        if len(columns) != len(storage.col_rings):
            raise ValueError(f"replay_add: {len(storage.col_rings)} column rings but {len(columns)} columns")
        if not -1 <= done_col < len(columns):
            raise ValueError(f"replay_add: done_col {done_col} outside [-1, {len(columns)})")
        if done_col >= 0 and storage.col_rings[done_col].dtype != torch.float32:
            raise TypeError(f"replay_add: the done column ring must be float32, got {storage.col_rings[done_col].dtype}")
        if (done_col >= 0 or final_obs is not None) and done is None:
            raise ValueError("replay_add: final_obs and a done column need done")
        flat = [(f"column {c}", x, storage.col_rings[c].dtype) for c, x in enumerate(columns) if c != done_col]
        if done is not None:
            if not torch.is_tensor(done) or done.element_size() != 1:
                raise TypeError(f"replay_add: done must have a 1-byte dtype, got {getattr(done, 'dtype', type(done))}")
            flat.append(("done", done, done.dtype))
        for name, x, dt in flat:
            if not torch.is_tensor(x) or x.shape != (T, self.n) or not x.is_contiguous():
                raise ValueError(f"replay_add: {name} must be a contiguous [{T}, {self.n}] tensor, got {tuple(getattr(x, 'shape', ()))}")
            if x.dtype != dt:
                raise TypeError(f"replay_add: {name} is {x.dtype}, its ring holds {dt}")
        for name, x in views + [(n_, x) for n_, x, _ in flat]:
            if x.device != self.device:
                raise ValueError(f"replay_add: {name} lives on {x.device}, the engine on {self.device}")
        k = len(columns)
        src = (C.c_void_p * max(k, 1))(*[None if c == done_col else x.data_ptr() for c, x in enumerate(columns)])
        with torch.cuda.device(self.device):
            self._chk(self._L.ptg_replay_add(self._h, C.byref(d), C.c_void_p(prev_obs.data_ptr()), C.c_void_p(obs.data_ptr()),
                                             obs.stride(0), obs.stride(1), obs.stride(2),
                                             C.c_void_p(final_obs.data_ptr()) if final_obs is not None else None,
                                             C.c_void_p(done.data_ptr()) if done is not None else None, done_col, k, src, T, self._stream()))

    def replay_sample(self, storage, batch_size=None, idx=None, seed=0, want_obs=True, want_next=True, want_cols=None, norm_col=-1,
                      want_idx=False, out=None):
        """Enqueue, on the current stream, SB3's ReplayBuffer.sample / _get_samples (include/ptg_env.h: ptg_replay_sample): a gather
        at the flat indices idx (int64 [B], i = slot * N + env) or, with idx None, at batch_size indices drawn on the device from
        (seed, cursor[1], row).  Returns (obs [B, F] | None, next_obs [B, F] | None, [column outputs [B] | None], idx_out [B] | None);
        want_cols: a bool per column ring (None: all); norm_col: the reward column, normalised as vn_normalize(training=False)
        would; out: the same 4-tuple of preallocated outputs (for a captured call).  No synchronisation; an index out of range, or a
        draw from an empty buffer, leaves its row untouched and makes the next sync() raise PtgError with code PTG_E_INDEX."""
        torch = self._torch
        d = self._replay_desc(storage, "replay_sample")
        k = len(storage.col_rings)
        F = storage.obs_ring.shape[2]
        if idx is not None:
            if not torch.is_tensor(idx) or idx.dtype != torch.int64:
                raise TypeError(f"replay_sample: idx must be an int64 tensor, got {getattr(idx, 'dtype', type(idx))}")
            if idx.dim() != 1 or not idx.is_contiguous() or idx.device != self.device:
                raise ValueError(f"replay_sample: idx must be 1-D and contiguous on {self.device}, got shape {tuple(idx.shape)} on {idx.device}")
            if batch_size is not None and int(batch_size) != idx.shape[0]:
                raise ValueError(f"replay_sample: batch_size {batch_size} but {idx.shape[0]} indices")
            B = idx.shape[0]
        else:
            if batch_size is None:
                raise ValueError("replay_sample: neither idx nor batch_size given")
            B = int(batch_size)
        if B < 1:
            raise ValueError(f"replay_sample: an empty batch ({B} rows)")
        if not -1 <= norm_col < k:
            raise ValueError(f"replay_sample: norm_col {norm_col} outside [-1, {k})")
        want_cols = [True] * k if want_cols is None else [bool(w) for w in want_cols]
        if len(want_cols) != k:
            raise ValueError(f"replay_sample: {k} column rings but {len(want_cols)} entries in want_cols")
        with torch.cuda.device(self.device):
            if out is None:
                mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
                out = (mk((B, F), storage.obs_ring.dtype) if want_obs else None, mk((B, F), storage.obs_ring.dtype) if want_next else None,
                       [mk((B,), x.dtype) if w else None for x, w in zip(storage.col_rings, want_cols)], mk((B,), torch.int64) if want_idx else None)
            o0, o1, outs, io = out
            outs = list(outs)
            if len(outs) != k:
                raise ValueError(f"replay_sample: {k} column rings but {len(outs)} column outputs")
            exp = [("obs output", o0, (B, F), storage.obs_ring.dtype), ("next_obs output", o1, (B, F), storage.obs_ring.dtype), ("idx output", io, (B,), torch.int64)]
            exp += [(f"output of column {c}", o, (B,), x.dtype) for c, (o, x) in enumerate(zip(outs, storage.col_rings))]
            for name, x, shape, dt in exp:
                if x is not None and (not torch.is_tensor(x) or x.shape != shape or x.dtype != dt or not x.is_contiguous() or x.device != self.device):
                    raise ValueError(f"replay_sample: {name} must be a contiguous {list(shape)} tensor of {dt} on {self.device}, got "
                                     f"{tuple(getattr(x, 'shape', ()))} of {getattr(x, 'dtype', type(x))}")
            if all(x is None for _, x, _, _ in exp):
                raise ValueError("replay_sample: no output asked for")
            if norm_col >= 0 and outs[norm_col] is None:
                raise ValueError("replay_sample: norm_col names a column without an output")
            if norm_col >= 0 and storage.col_rings[norm_col].dtype != self.out_dtype:
                raise TypeError(f"replay_sample: the reward column is {storage.col_rings[norm_col].dtype}, the engine normalises {self.out_dtype}")
            dst = (C.c_void_p * max(k, 1))(*[None if o is None else o.data_ptr() for o in outs])
            ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
            self._chk(self._L.ptg_replay_sample(self._h, C.byref(d), ptr(idx), B, int(seed) & (2 ** 64 - 1), ptr(o0), ptr(o1), dst,
                                                norm_col, ptr(io), self._stream()))
        return o0, o1, outs, io

    # ------------------------------------------------------------------ the action head while collecting
    def new_draw_counter(self):
        """The zeroed device counter of the action heads' draws: uint64 [1], held as an int64 tensor.  A stochastic act_* call advances
        it by one on the device, so a replayed graph draws afresh; checkpoint it with int(counter)."""
        return self._torch.zeros(1, dtype=self._torch.int64, device=self.device)

    def _act_counter(self, who, counter, deterministic):
        torch = self._torch
        if counter is None:
            if not deterministic:
                raise ValueError(f"{who}: a stochastic head needs a draw counter (new_draw_counter())")
            return None
        if not torch.is_tensor(counter) or counter.dtype != torch.int64 or counter.shape != (1,):
            raise TypeError(f"{who}: counter must be an int64 tensor of 1 element (new_draw_counter()), got "
                            f"{getattr(counter, 'dtype', type(counter))} {tuple(getattr(counter, 'shape', ()))}")
        if counter.device != self.device:
            raise ValueError(f"{who}: counter lives on {counter.device}, the engine on {self.device}")
        return counter

    def _act_outputs(self, who, kind, out, specs):
        """the output tensors of a head: out's (checked) or fresh ones; specs = [(field, wanted, dtype)] in the namedtuple's order"""
        torch = self._torch
        if out is not None and (not isinstance(out, tuple) or len(out) != len(specs)):
            raise ValueError(f"{who}: out must be the {kind.__name__} of an earlier call")
        res = []
        for k, (name, wanted, dt) in enumerate(specs):
            x = None if out is None else out[k]
            if out is None and wanted:
                with torch.cuda.device(self.device):
                    x = torch.empty(self.n, dtype=dt, device=self.device)
            if x is not None:
                if not wanted:
                    raise ValueError(f"{who}: out.{name} given, but the head has no such output or it was not asked for")
                if not torch.is_tensor(x) or x.shape != (self.n,) or x.dtype != dt or not x.is_contiguous() or x.device != self.device:
                    raise ValueError(f"{who}: out.{name} must be a contiguous [{self.n}] tensor of {dt} on {self.device}, got "
                                     f"{tuple(getattr(x, 'shape', ()))} of {getattr(x, 'dtype', type(x))}")
            elif name == "actions":
                raise ValueError(f"{who}: out.actions is missing")
            res.append(x)
        return kind(*res)

    def _act_input(self, who, x, name, discrete):
        """logits / Q-values [N, A] with unit column stride and a row stride >= A (a slice of a wider output), or means [N] / [N, 1]"""
        torch = self._torch
        if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{who}: {name} must be a float32 or float64 tensor, got {getattr(x, 'dtype', type(x))}")
        if x.device != self.device:
            raise ValueError(f"{who}: {name} lives on {x.device}, the engine on {self.device}")
        if discrete:
            if x.dim() != 2 or x.shape[0] != self.n or not 2 <= x.shape[1] <= 32:
                raise ValueError(f"{who}: {name} must be [{self.n}, A] with 2 <= A <= 32, got shape {tuple(x.shape)}")
            if x.stride(1) != 1 or (self.n > 1 and x.stride(0) < x.shape[1]):
                raise ValueError(f"{who}: {name} needs unit column stride and a row stride >= A, got strides {tuple(x.stride())}")
            return x.shape[1], max(x.stride(0), x.shape[1])
        if x.dim() == 2 and x.shape[1] == 1:
            x = x[:, 0]
        if x.shape != (self.n,):
            raise ValueError(f"{who}: {name} must be [{self.n}] (or [{self.n}, 1]: the env's Box has one dimension), got shape {tuple(x.shape)}")
        if self.n > 1 and x.stride(0) < 1:
            raise ValueError(f"{who}: {name} has stride {x.stride(0)}")
        return 1, max(x.stride(0), 1)

    def _act_dtype(self, who, act_dtype, out):
        """the discrete heads' action dtype: the caller's, else that of out.actions, else int32"""
        torch = self._torch
        if act_dtype is None and isinstance(out, tuple) and out and torch.is_tensor(out[0]):
            act_dtype = out[0].dtype
        act_dtype = torch.int32 if act_dtype is None else act_dtype
        if act_dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{who}: act_dtype must be torch.int32 or torch.int64, got {act_dtype}")
        return act_dtype

    def _act_launch(self, head, x, counter, seed, res):
        torch = self._torch
        ptr = lambda t: None if t is None else t.data_ptr()
        head.in_dtype = _lib.OUT_F64 if x.dtype == torch.float64 else _lib.OUT_F32
        head.in_dev, head.seed, head.counter_dev = x.data_ptr(), int(seed) & (2 ** 64 - 1), ptr(counter)
        head.act_dev, head.logp_dev, head.ent_dev = ptr(res.actions), ptr(getattr(res, "log_prob", None)), ptr(getattr(res, "entropy", None))
        head.raw_dev = ptr(getattr(res, "raw", None))
        head.act_kind = self._action_kind(res.actions)
        with torch.cuda.device(self.device):
            self._chk(self._L.ptg_act(self._h, C.byref(head), self._stream()))
        return res

    def act_categorical(self, logits, counter, seed=0, deterministic=False, out=None, want_logp=True, want_entropy=True, act_dtype=None):
        """Enqueue, on the current stream, SB3's CategoricalDistribution.sample (deterministic: mode), log_prob and entropy of the
        logits [N, A] (float32 / float64, 2 <= A <= 32, a column slice of a wider tensor is fine) in ONE launch (include/ptg_env.h:
        ptg_act, which states the arithmetic).  act_dtype None: the dtype of out.actions when out is given, else torch.int32 (torch is
        imported lazily here, so the default is spelled None).  counter: new_draw_counter(); row e of the c-th call draws from (seed, c, global env
        offset + e).  Returns CategoricalAct(actions [N] of act_dtype (torch.int32, the default, or int64: what step() takes), log_prob
        [N], entropy [N] in the logits' dtype, or None when not wanted); out: an earlier call's result, reused (a captured call).
        No synchronisation; a row with a NaN or +Inf logit, or -Inf in every column, gets action 0 and NaN outputs and makes the next
        sync() raise PtgError with code PTG_E_NONFINITE."""
        who = "act_categorical"
        A, s_n = self._act_input(who, logits, "logits", True)
        counter = self._act_counter(who, counter, deterministic)
        res = self._act_outputs(who, CategoricalAct, out, [("actions", True, self._act_dtype(who, act_dtype, out)), ("log_prob", want_logp, logits.dtype),
                                                           ("entropy", want_entropy, logits.dtype)])
        head = _lib.PtgHead(kind=_lib.HEAD_CATEGORICAL, flags=_lib.HEAD_DETERMINISTIC if deterministic else 0, n_actions=A, in_s_n=s_n)
        return self._act_launch(head, logits, counter, seed, res)

    def act_eps_greedy(self, q, eps, counter, seed=0, deterministic=False, out=None, act_dtype=None):
        """DQN's collecting policy in one launch: with probability eps a uniform random action, else the first maximal Q-value of
        q [N, A]; deterministic: always the latter (eps is not read).  eps: a float64 device tensor of 1 element, read when the kernel
        runs (anneal it in place between replays), or a Python float, written to a fresh device scalar by a fill kernel ahead of the head
        on the same stream -- a captured call then keeps that value on every replay.
        Returns EpsGreedyAct(actions).  A row with a NaN or +Inf value, and every row when eps is NaN or outside [0, 1], gets action 0
        and makes the next sync() raise PtgError with code PTG_E_NONFINITE."""
        torch = self._torch
        who = "act_eps_greedy"
        A, s_n = self._act_input(who, q, "q", True)
        counter = self._act_counter(who, counter, deterministic)
        if torch.is_tensor(eps):
            if eps.dtype != torch.float64 or eps.numel() != 1 or not eps.is_contiguous():
                raise TypeError(f"{who}: a tensor eps must be float64 with 1 element, got {eps.dtype} {tuple(eps.shape)}")
            if eps.device != self.device:
                raise ValueError(f"{who}: eps lives on {eps.device}, the engine on {self.device}")
        elif eps is None:
            if not deterministic:
                raise ValueError(f"{who}: a stochastic call needs eps")
        else:
            eps = float(eps)                                  # written to the device below, once every check has passed
        res = self._act_outputs(who, EpsGreedyAct, out, [("actions", True, self._act_dtype(who, act_dtype, out))])
        if isinstance(eps, float):                            # a fill kernel on the current stream, not a host copy: it can be captured, and
            with torch.cuda.device(self.device):              # a replay then writes the same value into the graph's own memory
                eps = torch.full((1,), eps, dtype=torch.float64, device=self.device)
        head = _lib.PtgHead(kind=_lib.HEAD_EPS_GREEDY, flags=_lib.HEAD_DETERMINISTIC if deterministic else 0, n_actions=A, in_s_n=s_n,
                            param_dev=None if eps is None else eps.data_ptr())
        return self._act_launch(head, q, counter, seed, res)

    def act_gaussian(self, mean, log_std, counter, clip=(-1.0, 1.0), squash=False, seed=0, deterministic=False, out=None, want_raw=True,
                     want_logp=True, want_entropy=None):
        """The Gaussian heads in one launch: g = mean + exp(log_std) * z, z a Box-Muller normal (deterministic: z = 0).  Plain
        (TD3 with log_std = log(sigma_exp); continuous A2C / PPO): actions = clip(g), log_prob and entropy of N(mean, sigma);
        squash=True (SAC / TQC): actions = clip(tanh(g)), log_prob with SB3's tanh correction, no entropy.  mean [N] (or [N, 1]),
        log_std of mean's dtype: 1 element (state-independent) or [N]; both may be rewritten between replays.  Returns
        GaussianAct(actions float32 [N] for step(), raw = g unclipped and unsquashed (what an on-policy buffer stores), log_prob,
        entropy).  A non-finite mean or a NaN / +Inf log_std gives action 0, NaN outputs and PTG_E_NONFINITE at the next sync()."""
        torch = self._torch
        who = "act_gaussian"
        self._act_input(who, mean, "mean", False)
        m1 = mean[:, 0] if mean.dim() == 2 else mean
        if not torch.is_tensor(log_std) or log_std.dtype != mean.dtype:
            raise TypeError(f"{who}: log_std must be a tensor of mean's dtype {mean.dtype}, got {getattr(log_std, 'dtype', type(log_std))}")
        if log_std.device != self.device:
            raise ValueError(f"{who}: log_std lives on {log_std.device}, the engine on {self.device}")
        if log_std.numel() == 1:
            p_s = 0
        elif log_std.numel() == self.n and log_std.is_contiguous() and log_std.dim() <= 2:
            p_s = 1
        else:
            raise ValueError(f"{who}: log_std must have 1 element or be a contiguous [{self.n}] tensor, got shape {tuple(log_std.shape)}")
        lo, hi = float(clip[0]), float(clip[1])
        if not lo <= hi:
            raise ValueError(f"{who}: clip {clip} is not an interval")
        if want_entropy is None:
            want_entropy = not squash
        if squash and want_entropy:
            raise ValueError(f"{who}: a squashed Gaussian has no closed-form entropy")
        counter = self._act_counter(who, counter, deterministic)
        res = self._act_outputs(who, GaussianAct, out, [("actions", True, torch.float32), ("raw", want_raw, mean.dtype), ("log_prob", want_logp, mean.dtype),
                                                        ("entropy", want_entropy, mean.dtype)])
        flags = (_lib.HEAD_DETERMINISTIC if deterministic else 0) | (_lib.HEAD_SQUASH if squash else 0)
        head = _lib.PtgHead(kind=_lib.HEAD_GAUSSIAN, flags=flags, in_s_n=max(m1.stride(0), 1), param_dev=log_std.data_ptr(), param_s_n=p_s, clip_lo=lo, clip_hi=hi)
        return self._act_launch(head, m1, counter, seed, res)

    # ------------------------------------------------------------------ the loss of a minibatch and its gradients
    def policy_loss_workspace(self, batch):
        """the device scratch of policy_loss for a batch of this size (a uint8 tensor; reuse it across calls of up to that size)"""
        nbytes = self._L.ptg_policy_loss_workspace(int(batch))
        if nbytes < 0:
            raise ValueError(f"policy_loss_workspace: batch must be >= 1, got {batch}")
        with self._torch.cuda.device(self.device):
            return self._torch.empty(nbytes, dtype=self._torch.uint8, device=self.device)

    def policy_loss(self, kind, head_input, values, actions, old_log_prob, advantages, returns, *, clip_range=None, clip_range_vf=None,
                    ent_coef=0.0, vf_coef=0.5, normalize_advantage=None, old_values=None, log_std=None, out=None, workspace=None):
        """Enqueue, on the current stream, SB3's evaluate_actions and the loss lines of PPO.train (kind "ppo") or A2C.train ("a2c") on
        one minibatch together with their gradients (include/ptg_env.h: ptg_policy_loss, which states the arithmetic).
        head_input: logits [B, A] (2 <= A <= 32, unit column stride, row stride >= A: a column slice of an [B, A + 1] actor-critic
        output is fine) with int32 / int64 actions [B] -- or, with log_std (a 1-element tensor), the Gaussian head's means [B] /
        [B, 1] with the stored raw samples [B] as actions.  values [B] (any stride >= 1); old_log_prob (PPO; None for A2C),
        advantages, returns and old_values (required iff clip_range_vf is given) contiguous [B]; every float tensor of ONE dtype,
        float32 or float64.  clip_range is required for PPO.  normalize_advantage None: SB3's default, True for PPO, False for A2C.
        Returns PolicyLoss(stats float64 [8] = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv mean, adv
        std; grad_input = d loss / d head_input, shaped like it; grad_values [B]; grad_log_std [1] or None).  out: an earlier result
        (or any such tuple: grad_input and grad_values may be views of one [B, A + 1] tensor), reused by a captured call; workspace:
        policy_loss_workspace(B) or larger, allocated when missing.  Fresh gradients are torch.empty: a row refused for its action
        keeps what was there.  No synchronisation; a bad row makes the next sync() raise PtgError (PTG_E_INDEX / PTG_E_NONFINITE)."""
        torch = self._torch
        who = "policy_loss"
        if kind not in ("ppo", "a2c"):
            raise ValueError(f"{who}: kind must be 'ppo' or 'a2c', got {kind!r}")
        ppo = kind == "ppo"
        x = head_input
        if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{who}: head_input must be a float32 or float64 tensor, got {getattr(x, 'dtype', type(x))}")
        gauss = log_std is not None
        dt = x.dtype
        if gauss:
            if x.dim() == 2 and x.shape[1] == 1:
                x = x[:, 0]
            if x.dim() != 1 or x.shape[0] < 1:
                raise ValueError(f"{who}: with log_std, head_input must be the means [B] or [B, 1], got shape {tuple(head_input.shape)}")
            B, A = x.shape[0], 0
            if B > 1 and x.stride(0) < 1:
                raise ValueError(f"{who}: head_input has stride {x.stride(0)}")
            s_n = max(x.stride(0), 1)
            if not torch.is_tensor(log_std) or log_std.dtype != dt or log_std.numel() != 1:
                raise TypeError(f"{who}: log_std must be a 1-element tensor of {dt}, got {getattr(log_std, 'dtype', type(log_std))} "
                                f"{tuple(getattr(log_std, 'shape', ()))}")
        else:
            if x.dim() != 2 or x.shape[0] < 1 or not 2 <= x.shape[1] <= 32:
                raise ValueError(f"{who}: head_input must be logits [B, A] with 2 <= A <= 32 (or means [B] with log_std), got shape {tuple(x.shape)}")
            B, A = x.shape
            if x.stride(1) != 1 or (B > 1 and x.stride(0) < A):
                raise ValueError(f"{who}: logits need unit column stride and a row stride >= A, got strides {tuple(x.stride())}")
            s_n = max(x.stride(0), A)
        if not torch.is_tensor(actions) or actions.dtype not in ((dt,) if gauss else (torch.int32, torch.int64)):
            raise TypeError(f"{who}: actions must be {'the raw samples in ' + str(dt) if gauss else 'int32 or int64'}, got {getattr(actions, 'dtype', type(actions))}")
        if not torch.is_tensor(values) or values.dtype != dt:
            raise TypeError(f"{who}: values must be a tensor of {dt}, got {getattr(values, 'dtype', type(values))}")
        if values.dim() == 2 and values.shape[1] == 1:
            values = values[:, 0]
        if values.shape != (B,) or (B > 1 and values.stride(0) < 1):
            raise ValueError(f"{who}: values must be [{B}] with a stride >= 1, got shape {tuple(values.shape)}, strides {tuple(values.stride())}")
        if clip_range_vf is not None and old_values is None:
            raise ValueError(f"{who}: clip_range_vf needs old_values")
        if ppo and old_log_prob is None:
            raise ValueError(f"{who}: PPO needs old_log_prob")
        cols = [("actions", actions), ("advantages", advantages), ("returns", returns)]
        cols += [("old_log_prob", old_log_prob)] if ppo else []
        cols += [("old_values", old_values)] if clip_range_vf is not None else []
        for name, c in cols:
            if not torch.is_tensor(c) or (name != "actions" and c.dtype != dt):
                raise TypeError(f"{who}: {name} must be a tensor of {dt}, got {getattr(c, 'dtype', type(c))}")
            if c.shape != (B,) or not c.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous [{B}] tensor, got shape {tuple(c.shape)}, strides {tuple(c.stride())}")
        for name, c in [("head_input", x), ("values", values)] + cols + ([("log_std", log_std)] if gauss else []):
            if c.device != self.device:
                raise ValueError(f"{who}: {name} lives on {c.device}, the engine on {self.device}")
        if ppo:
            if clip_range is None or not float(clip_range) >= 0.0:
                raise ValueError(f"{who}: PPO needs a clip_range >= 0, got {clip_range}")
        if clip_range_vf is not None and not float(clip_range_vf) >= 0.0:
            raise ValueError(f"{who}: clip_range_vf must be >= 0 (or None), got {clip_range_vf}")
        if normalize_advantage is None:
            normalize_advantage = ppo
        if out is not None:
            if not isinstance(out, tuple) or len(out) != 4:
                raise ValueError(f"{who}: out must be the PolicyLoss of an earlier call")
            stats, g_in, g_val, g_ls = out
        else:
            with torch.cuda.device(self.device):
                stats = torch.empty(8, dtype=torch.float64, device=self.device)
                g_in = torch.empty((B,) if gauss else (B, A), dtype=dt, device=self.device)
                g_val = torch.empty(B, dtype=dt, device=self.device)
                g_ls = torch.empty(1, dtype=dt, device=self.device) if gauss else None
        if gauss and torch.is_tensor(g_in) and g_in.dim() == 2 and g_in.shape[1] == 1:
            g_in = g_in[:, 0]
        for name, t, shape, tdt in (("stats", stats, (8,), torch.float64), ("grad_input", g_in, (B,) if gauss else (B, A), dt), ("grad_values", g_val, (B,), dt)) + \
                ((("grad_log_std", g_ls, (1,), dt),) if gauss else ()):
            if not torch.is_tensor(t) or t.shape != shape or t.dtype != tdt or t.device != self.device:
                raise ValueError(f"{who}: out.{name} must be a {list(shape)} tensor of {tdt} on {self.device}, got "
                                 f"{tuple(getattr(t, 'shape', ()))} of {getattr(t, 'dtype', type(t))}")
        if not gauss and g_ls is not None:
            raise ValueError(f"{who}: out.grad_log_std given, but the categorical head has no log_std")
        if not stats.is_contiguous() or (not gauss and g_in.stride(1) != 1) or (B > 1 and (g_in.stride(0) < max(A, 1) or g_val.stride(0) < 1)):
            raise ValueError(f"{who}: out.stats must be contiguous, out.grad_input needs unit column stride and a row stride >= A, out.grad_values a "
                             f"stride >= 1; got strides {tuple(stats.stride())}, {tuple(g_in.stride())}, {tuple(g_val.stride())}")
        if workspace is not None:
            if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != self.device:
                raise ValueError(f"{who}: workspace must be a contiguous uint8 tensor on {self.device} (policy_loss_workspace({B}))")
            if workspace.numel() < self._L.ptg_policy_loss_workspace(B):
                raise ValueError(f"{who}: workspace has {workspace.numel()} bytes, a batch of {B} needs {self._L.ptg_policy_loss_workspace(B)}")
        else:
            workspace = self.policy_loss_workspace(B)
        d = _lib.PtgLoss(kind=_lib.LOSS_PPO if ppo else _lib.LOSS_A2C, head=_lib.HEAD_GAUSSIAN if gauss else _lib.HEAD_CATEGORICAL,
                         flags=(_lib.LOSS_NORM_ADV if normalize_advantage else 0) | (_lib.LOSS_CLIP_VF if clip_range_vf is not None else 0),
                         n_actions=A, in_dtype=_lib.OUT_F64 if dt == torch.float64 else _lib.OUT_F32,
                         act_kind=_lib.ACT_I64 if actions.dtype == torch.int64 else _lib.ACT_I32, batch=B,
                         in_dev=x.data_ptr(), in_s_n=s_n, val_dev=values.data_ptr(), val_s_n=max(values.stride(0), 1), act_dev=actions.data_ptr(),
                         old_logp_dev=old_log_prob.data_ptr() if ppo else None, adv_dev=advantages.data_ptr(), ret_dev=returns.data_ptr(),
                         old_val_dev=old_values.data_ptr() if clip_range_vf is not None else None, log_std_dev=log_std.data_ptr() if gauss else None,
                         clip_range=float(clip_range) if ppo else 0.0, clip_range_vf=float(clip_range_vf) if clip_range_vf is not None else 0.0,
                         ent_coef=float(ent_coef), vf_coef=float(vf_coef), stats_dev=stats.data_ptr(), grad_in_dev=g_in.data_ptr(),
                         g_s_n=max(g_in.stride(0), A, 1), grad_val_dev=g_val.data_ptr(), gv_s_n=max(g_val.stride(0), 1),
                         grad_log_std_dev=g_ls.data_ptr() if gauss else None, ws_dev=workspace.data_ptr())
        with torch.cuda.device(self.device):
            self._chk(self._L.ptg_policy_loss(self._h, C.byref(d), self._stream()))
        return PolicyLoss(stats, g_in, g_val, g_ls)

    def market_feature_series(self):
        """The pre-normalised float32 feature series the kernels read, each [n_sets, length]: dict(featA, featB (hourly), gas_n, eua_n
        (daily)).  Columns 14 / 15 of a "split" observation row index the flattened arrays."""
        out = {}
        for which, name in enumerate(("featA", "featB", "gas_n", "eua_n")):
            cnt = C.c_int(0)
            self._chk(self._L.ptg_market_feature_series(self._h, which, None, 0, C.byref(cnt)))
            a = np.zeros(cnt.value, np.float32)
            self._chk(self._L.ptg_market_feature_series(self._h, which, a.ctypes.data_as(C.POINTER(C.c_float)), cnt.value, C.byref(cnt)))
            out[name] = a.reshape(self.n_sets, -1)
        return out

    def debug_get_index_lut(self):
        nT = C.c_int(0)
        self._chk(self._L.ptg_debug_get_index_lut(self._h, None, None, C.byref(nT)))
        T = np.zeros(nT.value)
        lut = np.zeros((6, nT.value), np.int32)
        self._chk(self._L.ptg_debug_get_index_lut(self._h, _dp(T), lut.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nT)))
        return T, lut

    def debug_table_plan(self):
        """What the tables made of this handle: dict(has_lut16, lds_lut, nT, key_init, i_reset, key_cold_max, key_hot_min, key_standby_max)."""
        out = np.zeros(8, np.int32)
        self._chk(self._L.ptg_debug_table_plan(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        keys = ("has_lut16", "lds_lut", "nT", "key_init", "i_reset", "key_cold_max", "key_hot_min", "key_standby_max")
        return {k: int(v) for k, v in zip(keys, out)}

    def debug_window_record(self, table_id, start_row):
        out = np.zeros(7)
        self._chk(self._L.ptg_debug_window_record(self._h, int(table_id), int(start_row), _dp(out)))
        return out
