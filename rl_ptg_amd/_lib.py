"""ctypes binding of libptg_env.so (include/ptg_env.h).  There is no CPU fallback: if the HIP library is
missing or fails to load, importing code gets a loud error."""
import ctypes as C
import os
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "ptg_env.hip")                # the environment: N_PARTS translation units of the parallel build
SRC_TRAIN = os.path.join(CSRC, "ptg_train.hip")        # the training ops: one translation unit
SRC_MLP = os.path.join(CSRC, "ptg_mlp.hip")            # the MLP forward and backward: one translation unit
HDR = os.path.join(ROOT, "include", "ptg_env.h")
LIB_PATH = os.environ.get("PTG_LIB_PATH") or os.path.join(PKG, "lib", "libptg_env.so")      # PTG_LIB_PATH: an experiment build of the same source
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall"]
N_PARTS = 9          # translation units of ptg_env.hip in the parallel build: -DPTG_PART=0..8 (ptg_env.hip, "PTG_PART")

N_TABLES, N_INFO = 17, 24
ACT_I32, ACT_F32, ACT_I64 = 0, 1, 2
OUT_F32, OUT_F64 = 0, 1
E_INVALID, E_HIP, E_ACTION, E_RANGE, E_INDEX, E_NONFINITE = -1, -2, -3, -4, -5, -6
MB_MAX_COLS = 8
MB_PERM_ROUNDS = 6                       # PTG_MB_PERM_ROUNDS
MB_DRAWN_MAX_ROWS = 1 << 48              # PTG_MB_DRAWN_MAX_ROWS
OBS_ROW_MAJOR, OBS_FEATURE_MAJOR, OBS_SB3_FLAT, OBS_SPLIT = 0, 1, 2, 3
HEAD_CATEGORICAL, HEAD_EPS_GREEDY, HEAD_GAUSSIAN = 0, 1, 2
HEAD_DETERMINISTIC, HEAD_SQUASH = 1, 2
LOSS_PPO, LOSS_A2C = 0, 1
LOSS_NORM_ADV, LOSS_CLIP_VF = 1, 2
OPTIM_ADAM, OPTIM_RMSPROP, OPTIM_POLYAK = 0, 1, 2
OPTIM_CLIP, OPTIM_TARGETS, OPTIM_ZERO_GRAD = 1, 2, 4
TD_DQN, TD_CRITICS = 0, 1                                 # the quantile critics (TQC) have their own entry point: ptg_quantile_loss
TD_ENTROPY, TD_LOG_ALPHA = 1, 2
TD_MAX_CRITICS = 4
QL_LOG_ALPHA = 1
QL_MAX_QUANTILES = 64
RS_SQUASH, RS_SMOOTH = 0, 1
RS_DETERMINISTIC = 1
SDE_RS_DETERMINISTIC, SDE_RS_SHARED_E = 1, 2
AL_MIN, AL_MEAN, AL_ALPHA_ONLY = 0, 1, 2
AL_ENTROPY, AL_LOG_ALPHA, AL_ENT_COEF = 1, 2, 4
MLP_MAX_LAYERS, MLP_MAX_WIDTH = 10, 1024
MLP_RELU, MLP_TANH, MLP_NONE = 0, 1, 2
MLP_KEEP_HIDDEN, MLP_NARROW, MLP_WIDE = 1, 2, 4
MLP_SPLIT_INPUT = 16                                      # ptg_mlp.flags: x holds split observation rows
MLP_ACCUMULATE = 8
MLP_GROUP_MAX = 8
TRAIN_GROUP_MAX = 8                                       # PTG_TRAIN_GROUP_MAX

_D1 = ["noise"]
_I1 = ["eps_len_d", "sim_step", "time_step_op", "price_ahead"]
_D2 = ["convert_mol_to_Nm3", "H_u_CH4", "H_u_H2", "dt_water", "cp_water", "rho_water", "Molar_mass_CO2",
       "Molar_mass_H2O", "h_H2O_evap", "eeg_el_price", "heat_price", "o2_price", "water_price",
       "min_load_electrolyzer", "max_h2_volumeflow", "eta_CHP",
       "t_cat_standby", "t_cat_startup_cold", "t_cat_startup_hot"]
_I2 = ["time1_start_p_f", "time2_start_f_p", "time_p_f", "time_f_p", "time1_p_f_p", "time2_p_f_p",
       "time23_p_f_p", "time3_p_f_p", "time34_p_f_p", "time4_p_f_p", "time45_p_f_p", "time5_p_f_p",
       "time1_f_p_f", "time2_f_p_f", "time23_f_p_f", "time3_f_p_f", "time34_f_p_f", "time4_f_p_f",
       "time45_f_p_f", "time5_f_p_f", "i_fully_developed", "j_fully_developed"]
_D3 = ["el_l_b", "el_u_b", "gas_l_b", "gas_u_b", "eua_l_b", "eua_u_b", "T_l_b", "T_u_b", "h2_l_b", "h2_u_b",
       "ch4_l_b", "ch4_u_b", "h2_res_l_b", "h2_res_u_b", "h2o_l_b", "h2o_u_b", "heat_l_b", "heat_u_b"]
_I3 = ["raw_modified", "action_type", "train_or_eval", "eps_sim_steps"]
_D4 = ["state_change_penalty", "t_cat_initial"]
_I4 = ["out_dtype", "obs_layout"]
CONFIG_KEYS = _D1 + _I1 + _D2 + _I2 + _D3 + _I3 + _D4 + _I4


class PtgConfig(C.Structure):
    _fields_ = ([(k, C.c_double) for k in _D1] + [(k, C.c_int32) for k in _I1] + [(k, C.c_double) for k in _D2] +
                [(k, C.c_int32) for k in _I2] + [(k, C.c_double) for k in _D3] + [(k, C.c_int32) for k in _I3] +
                [(k, C.c_double) for k in _D4] + [(k, C.c_int32) for k in _I4])


class PtgTables(C.Structure):
    _fields_ = [("data_host", C.POINTER(C.c_double) * N_TABLES), ("rows", C.c_int32 * N_TABLES)]


class PtgMarket(C.Structure):
    _fields_ = [("n_hours", C.c_int32), ("el_host", C.POINTER(C.c_double)), ("pot_rew_host", C.POINTER(C.c_double)),
                ("part_full_host", C.POINTER(C.c_double)), ("n_days", C.c_int32), ("gas_host", C.POINTER(C.c_double)),
                ("eua_host", C.POINTER(C.c_double)), ("scenario", C.c_int32), ("reserved", C.c_int32),
                ("rew_l_b", C.c_double), ("rew_u_b", C.c_double), ("r_0", C.c_double)]


class PtgReplay(C.Structure):                               # ptg_replay: caller-owned replay buffer storage
    _fields_ = [("capacity", C.c_int64), ("obs_dim", C.c_int32), ("obs_bytes", C.c_int32), ("obs_ring", C.c_void_p),
                ("next_ring", C.c_void_p), ("n_cols", C.c_int32), ("col_bytes", C.c_int32 * MB_MAX_COLS),
                ("col_ring", C.c_void_p * MB_MAX_COLS), ("cursor_dev", C.c_void_p)]


class PtgRolloutBuffer(C.Structure):                        # ptg_rollout_buffer: caller-owned on-policy collect storage
    _fields_ = [("n_steps", C.c_int64), ("obs_dim", C.c_int32), ("obs_bytes", C.c_int32), ("obs_rows", C.c_void_p), ("n_cols", C.c_int32),
                ("col_bytes", C.c_int32 * MB_MAX_COLS), ("col_rows", C.c_void_p * MB_MAX_COLS), ("cursor_dev", C.c_void_p)]


class PtgHead(C.Structure):                                 # ptg_head: one call of the action head
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("n_actions", C.c_int32), ("in_dtype", C.c_int32), ("in_dev", C.c_void_p),
                ("in_s_n", C.c_int64), ("param_dev", C.c_void_p), ("param_s_n", C.c_int32), ("act_kind", C.c_int32),
                ("clip_lo", C.c_double), ("clip_hi", C.c_double), ("seed", C.c_uint64), ("counter_dev", C.c_void_p),
                ("act_dev", C.c_void_p), ("raw_dev", C.c_void_p), ("logp_dev", C.c_void_p), ("ent_dev", C.c_void_p)]


class PtgLoss(C.Structure):                                 # ptg_loss: one call of the policy loss
    _fields_ = [("kind", C.c_int32), ("head", C.c_int32), ("flags", C.c_int32), ("n_actions", C.c_int32), ("in_dtype", C.c_int32),
                ("act_kind", C.c_int32), ("batch", C.c_int64), ("in_dev", C.c_void_p), ("in_s_n", C.c_int64), ("val_dev", C.c_void_p),
                ("val_s_n", C.c_int64), ("act_dev", C.c_void_p), ("old_logp_dev", C.c_void_p), ("adv_dev", C.c_void_p), ("ret_dev", C.c_void_p),
                ("old_val_dev", C.c_void_p), ("log_std_dev", C.c_void_p), ("clip_range", C.c_double), ("clip_range_vf", C.c_double),
                ("ent_coef", C.c_double), ("vf_coef", C.c_double), ("stats_dev", C.c_void_p), ("grad_in_dev", C.c_void_p), ("g_s_n", C.c_int64),
                ("grad_val_dev", C.c_void_p), ("gv_s_n", C.c_int64), ("grad_log_std_dev", C.c_void_p), ("ws_dev", C.c_void_p)]


class PtgSdeNoise(C.Structure):                             # ptg_sde_noise: one refill of gSDE's exploration matrix
    _fields_ = [("in_dtype", C.c_int32), ("latent_dim", C.c_int32), ("log_std_dev", C.c_void_p), ("seed", C.c_uint64), ("counter_dev", C.c_void_p),
                ("e_dev", C.c_void_p), ("e_s_n", C.c_int64)]


class PtgSdeHead(C.Structure):                              # ptg_sde_head: one call of gSDE's collecting head
    _fields_ = [("flags", C.c_int32), ("in_dtype", C.c_int32), ("latent_dim", C.c_int32), ("act_kind", C.c_int32), ("mean_dev", C.c_void_p),
                ("mean_s_n", C.c_int64), ("latent_dev", C.c_void_p), ("latent_s_n", C.c_int64), ("e_dev", C.c_void_p), ("e_s_n", C.c_int64),
                ("log_std_dev", C.c_void_p), ("clip_lo", C.c_double), ("clip_hi", C.c_double), ("act_dev", C.c_void_p), ("raw_dev", C.c_void_p),
                ("logp_dev", C.c_void_p), ("ent_dev", C.c_void_p)]


class PtgSdeLoss(C.Structure):                              # ptg_sde_loss: one call of the policy loss on gSDE's head
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("in_dtype", C.c_int32), ("latent_dim", C.c_int32), ("batch", C.c_int64),
                ("mean_dev", C.c_void_p), ("mean_s_n", C.c_int64), ("val_dev", C.c_void_p), ("val_s_n", C.c_int64), ("latent_dev", C.c_void_p),
                ("latent_s_n", C.c_int64), ("log_std_dev", C.c_void_p), ("act_dev", C.c_void_p), ("old_logp_dev", C.c_void_p), ("adv_dev", C.c_void_p),
                ("ret_dev", C.c_void_p), ("old_val_dev", C.c_void_p), ("clip_range", C.c_double), ("clip_range_vf", C.c_double),
                ("ent_coef", C.c_double), ("vf_coef", C.c_double), ("stats_dev", C.c_void_p), ("grad_in_dev", C.c_void_p), ("g_s_n", C.c_int64),
                ("grad_val_dev", C.c_void_p), ("gv_s_n", C.c_int64), ("grad_log_std_dev", C.c_void_p), ("grad_latent_dev", C.c_void_p),
                ("gl_s_n", C.c_int64), ("ws_dev", C.c_void_p)]


class PtgSdeRs(C.Structure):                                # ptg_sde_rs: one call of gSDE's squashed head for SAC / TQC, forward or backward
    _fields_ = [("flags", C.c_int32), ("in_dtype", C.c_int32), ("latent_dim", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int64),
                ("mean_dev", C.c_void_p), ("mean_s_n", C.c_int64), ("latent_dev", C.c_void_p), ("latent_s_n", C.c_int64), ("e_dev", C.c_void_p),
                ("e_s_n", C.c_int64), ("log_std_dev", C.c_void_p), ("clip_mean", C.c_double), ("act_dev", C.c_void_p), ("step_act_dev", C.c_void_p),
                ("logp_dev", C.c_void_p), ("saved_dev", C.c_void_p), ("grad_act_dev", C.c_void_p), ("grad_logp_dev", C.c_void_p),
                ("grad_mean_dev", C.c_void_p), ("gm_s_n", C.c_int64), ("grad_latent_dev", C.c_void_p), ("gl_s_n", C.c_int64),
                ("grad_log_std_dev", C.c_void_p), ("ws_dev", C.c_void_p)]


class PtgOptimTensor(C.Structure):                          # ptg_optim_tensor: one record of the optimiser's tensor table
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state1", C.c_void_p), ("state2", C.c_void_p), ("target", C.c_void_p),
                ("numel", C.c_int64)]


class PtgOptimSpan(C.Structure):                            # ptg_optim_span: one record of the optimiser's chunk table
    _fields_ = [("tensor", C.c_int64), ("offset", C.c_int64)]


class PtgOptim(C.Structure):                                # ptg_optim: one call of the optimiser step
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32), ("n_tensors", C.c_int64),
                ("n_chunks", C.c_int64), ("tensors_dev", C.c_void_p), ("chunks_dev", C.c_void_p), ("state_dev", C.c_void_p),
                ("lr_dev", C.c_void_p), ("norm_dev", C.c_void_p), ("ws_dev", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("alpha", C.c_double), ("tau", C.c_double), ("max_norm", C.c_double)]


class PtgTd(C.Structure):                                   # ptg_td: one call of the TD loss
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("n_actions", C.c_int32), ("n_critics", C.c_int32), ("q_dtype", C.c_int32),
                ("act_kind", C.c_int32), ("rew_dtype", C.c_int32), ("done_dtype", C.c_int32), ("batch", C.c_int64),
                ("q_dev", C.c_void_p * TD_MAX_CRITICS), ("q_s_n", C.c_int64 * TD_MAX_CRITICS), ("next_q_dev", C.c_void_p * TD_MAX_CRITICS),
                ("next_s_n", C.c_int64 * TD_MAX_CRITICS), ("act_dev", C.c_void_p), ("rew_dev", C.c_void_p), ("done_dev", C.c_void_p),
                ("next_logp_dev", C.c_void_p), ("alpha_dev", C.c_void_p), ("gamma", C.c_double), ("alpha", C.c_double), ("scale", C.c_double),
                ("stats_dev", C.c_void_p), ("grad_q_dev", C.c_void_p * TD_MAX_CRITICS), ("g_s_n", C.c_int64 * TD_MAX_CRITICS),
                ("y_dev", C.c_void_p), ("ws_dev", C.c_void_p)]


class PtgQl(C.Structure):                                   # ptg_ql: one call of the quantile-Huber loss
    _fields_ = [("flags", C.c_int32), ("n_critics", C.c_int32), ("n_quantiles", C.c_int32), ("n_drop", C.c_int32), ("q_dtype", C.c_int32),
                ("rew_dtype", C.c_int32), ("done_dtype", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int64),
                ("cur_dev", C.c_void_p * TD_MAX_CRITICS), ("cur_s_n", C.c_int64 * TD_MAX_CRITICS), ("next_dev", C.c_void_p * TD_MAX_CRITICS),
                ("next_s_n", C.c_int64 * TD_MAX_CRITICS), ("grad_dev", C.c_void_p * TD_MAX_CRITICS), ("g_s_n", C.c_int64 * TD_MAX_CRITICS),
                ("rew_dev", C.c_void_p), ("done_dev", C.c_void_p), ("next_logp_dev", C.c_void_p), ("alpha_dev", C.c_void_p),
                ("gamma", C.c_double), ("alpha", C.c_double), ("stats_dev", C.c_void_p), ("y_dev", C.c_void_p), ("ws_dev", C.c_void_p)]


class PtgRs(C.Structure):                                   # ptg_rs: one call of the training-time actor head, forward or backward
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("q_dtype", C.c_int32), ("reserved", C.c_int32), ("batch", C.c_int64),
                ("mean_dev", C.c_void_p), ("mean_s_n", C.c_int64), ("log_std_dev", C.c_void_p), ("log_std_s_n", C.c_int64),
                ("seed", C.c_uint64), ("counter_dev", C.c_void_p), ("noise_std", C.c_double), ("noise_clip", C.c_double),
                ("clip_lo", C.c_double), ("clip_hi", C.c_double), ("act_dev", C.c_void_p), ("logp_dev", C.c_void_p), ("noise_dev", C.c_void_p),
                ("grad_act_dev", C.c_void_p), ("grad_logp_dev", C.c_void_p), ("grad_mean_dev", C.c_void_p), ("gm_s_n", C.c_int64),
                ("grad_log_std_dev", C.c_void_p), ("gl_s_n", C.c_int64)]


class PtgAl(C.Structure):                                   # ptg_al: one call of the actor / entropy-coefficient loss
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("n_critics", C.c_int32), ("n_quantiles", C.c_int32), ("q_dtype", C.c_int32),
                ("reserved", C.c_int32), ("batch", C.c_int64), ("q_dev", C.c_void_p * TD_MAX_CRITICS), ("q_s_n", C.c_int64 * TD_MAX_CRITICS),
                ("logp_dev", C.c_void_p), ("alpha_dev", C.c_void_p), ("alpha", C.c_double), ("target_entropy", C.c_double),
                ("stats_dev", C.c_void_p), ("grad_q_dev", C.c_void_p * TD_MAX_CRITICS), ("g_s_n", C.c_int64 * TD_MAX_CRITICS),
                ("grad_logp_dev", C.c_void_p), ("grad_log_alpha_dev", C.c_void_p), ("ws_dev", C.c_void_p)]


class PtgMlp(C.Structure):                                  # ptg_mlp: one call of the MLP forward
    _fields_ = [("batch", C.c_int64), ("n_layers", C.c_int32), ("flags", C.c_int32), ("hidden_act", C.c_int32), ("out_act", C.c_int32),
                ("f1", C.c_int32), ("f2", C.c_int32), ("x_dev", C.c_void_p), ("x_s_n", C.c_int64), ("x2_dev", C.c_void_p), ("x2_s_n", C.c_int64),
                ("w_dev", C.c_void_p * MLP_MAX_LAYERS), ("w_s_n", C.c_int64 * MLP_MAX_LAYERS), ("b_dev", C.c_void_p * MLP_MAX_LAYERS),
                ("width", C.c_int32 * MLP_MAX_LAYERS), ("out_dev", C.c_void_p), ("out_s_n", C.c_int64), ("ws_dev", C.c_void_p), ("ws_bytes", C.c_int64)]


class PtgMlpBwd(C.Structure):                               # ptg_mlp_bwd: one call of the MLP backward
    _fields_ = [("fwd", PtgMlp), ("gout_dev", C.c_void_p), ("gout_s_n", C.c_int64), ("dw_dev", C.c_void_p * MLP_MAX_LAYERS),
                ("dw_s_n", C.c_int64 * MLP_MAX_LAYERS), ("db_dev", C.c_void_p * MLP_MAX_LAYERS), ("dx_dev", C.c_void_p), ("dx_s_n", C.c_int64),
                ("dx2_dev", C.c_void_p), ("dx2_s_n", C.c_int64), ("bws_dev", C.c_void_p), ("bws_bytes", C.c_int64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


# state fields of ptg_get_state / ptg_set_state
STATE_FIELDS = {"meth_state": 0, "i": 1, "j": 2, "k": 3, "hot_cold": 4, "standby_tid": 5, "startup_tid": 6,
                "partial_tid": 7, "full_tid": 8, "current_action": 9, "act_ep_d": 10, "ep_ptr": 11,
                "noise_count": 12, "n_state_changes": 13, "market_set": 14, "T_cat": 32, "cum_rew": 33}

EXPORTS = ["ptg_abi_version", "ptg_create", "ptg_destroy", "ptg_num_envs", "ptg_obs_dim", "ptg_last_error",
           "ptg_set_market_assignment", "ptg_set_episode_plan", "ptg_set_noise_tape", "ptg_set_noise_rng", "ptg_set_global_env_offset", "ptg_set_feature_pitch", "ptg_fill_noise_tape",
           "ptg_get_noise_tape", "ptg_reset", "ptg_step", "ptg_rollout", "ptg_rollout_info", "ptg_rollout_launches", "ptg_step_host", "ptg_host_layout", "ptg_host_layout_ex", "ptg_step_host_begin", "ptg_step_host_tail", "ptg_step_host_end", "ptg_step_host_finish", "ptg_host_buffers_changed", "ptg_profile", "ptg_profile_read", "ptg_profile_read_ex", "ptg_finished_dropped", "ptg_steps_to_episode_end", "ptg_note_replays", "ptg_set_replay_proof", "ptg_sync", "ptg_get_state", "ptg_set_state",
           "ptg_finished_episodes", "ptg_finished_episodes_dev", "ptg_episode_stats_dev", "ptg_vn_init", "ptg_vn_batch_moments", "ptg_vn_apply", "ptg_vn_clear_done", "ptg_vn_get", "ptg_vn_set", "ptg_gae", "ptg_minibatch", "ptg_minibatch_drawn", "ptg_minibatch_end_epoch", "ptg_replay_add", "ptg_replay_sample", "ptg_rollout_buffer_begin", "ptg_rollout_buffer_add", "ptg_act", "ptg_policy_loss_workspace", "ptg_policy_loss",
           "ptg_sde_resample", "ptg_sde_act", "ptg_sde_policy_loss_workspace", "ptg_sde_policy_loss",
           "ptg_sde_resample_rows", "ptg_sde_rsample", "ptg_sde_rsample_backward_workspace", "ptg_sde_rsample_backward",
           "ptg_optim_chunk", "ptg_optim_workspace", "ptg_optim_step", "ptg_td_loss_workspace", "ptg_td_loss", "ptg_quantile_loss_workspace", "ptg_quantile_loss",
           "ptg_rsample", "ptg_rsample_backward", "ptg_actor_loss_workspace", "ptg_actor_loss", "ptg_mlp_workspace", "ptg_mlp_forward", "ptg_mlp_backward_workspace", "ptg_mlp_backward",
           "ptg_mlp_group_forward", "ptg_mlp_group_backward", "ptg_policy_loss_group", "ptg_optim_step_group",
           "ptg_td_loss_group", "ptg_actor_loss_group", "ptg_rsample_group", "ptg_rsample_backward_group",
           "ptg_market_feature_series", "ptg_debug_get_index_lut", "ptg_debug_window_record", "ptg_debug_table_plan"]


def build(force=False, verbose=False):
    """hipcc cross-compiles the extension for gfx950 in-tree (no GPU needed to build)."""
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    newest = max([os.path.getmtime(HDR)] + [os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)])
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest:
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = int(os.environ.get("PTG_BUILD_JOBS", "0")) or min(N_PARTS + 2, os.cpu_count() or 1)
    if jobs <= 1:                                             # the three files whole (no PTG_PART) in one hipcc call
        cmd = [hipcc] + HIPCC_FLAGS + ["-shared", "-o", LIB_PATH, SRC, SRC_TRAIN, SRC_MLP]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return LIB_PATH
    # ptg_env.hip compiled N_PARTS times, each time with a different share of the hot-kernel instantiations, ptg_train.hip and
    # ptg_mlp.hip once each, `jobs` at a time
    obj_dir = os.path.join(os.path.dirname(LIB_PATH), "obj")
    os.makedirs(obj_dir, exist_ok=True)
    objs = [os.path.join(obj_dir, f"ptg_env_part{k}.o") for k in range(N_PARTS)] + [os.path.join(obj_dir, "ptg_train.o"), os.path.join(obj_dir, "ptg_mlp.o")]
    cmds = [[hipcc] + HIPCC_FLAGS + ["-Wno-unused-function", f"-DPTG_PART={k}", "-c", "-o", objs[k], SRC] for k in range(N_PARTS)]
    cmds.append([hipcc] + HIPCC_FLAGS + ["-c", "-o", objs[N_PARTS], SRC_TRAIN])
    cmds.append([hipcc] + HIPCC_FLAGS + ["-c", "-o", objs[N_PARTS + 1], SRC_MLP])
    running, todo, failed = [], list(enumerate(cmds)), []
    while todo or running:
        while todo and len(running) < jobs:
            k, cmd = todo.pop(0)
            if verbose:
                print(" ".join(cmd))
            running.append((k, subprocess.Popen(cmd)))
        k, proc = running.pop(0)
        if proc.wait() != 0:
            failed.append(k)
    if failed:
        raise RuntimeError(f"hipcc failed on {[os.path.basename(objs[k]) for k in failed]} ({SRC}, {SRC_TRAIN}, {SRC_MLP})")
    link = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(rl_ptg_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.ptg_abi_version.restype = C.c_int
    import re
    want = int(re.search(r"#define PTG_ABI_VERSION (\d+)", open(HDR).read()).group(1))
    if L.ptg_abi_version() != want:      # e.g. a stale experiment build behind PTG_LIB_PATH
        raise RuntimeError(f"{LIB_PATH} has ABI version {L.ptg_abi_version()}, include/ptg_env.h declares {want}: rebuild it "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    vp, dp, u8p, i32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    L.ptg_abi_version.restype = C.c_int
    L.ptg_create.argtypes = [C.POINTER(PtgConfig), C.POINTER(PtgTables), C.POINTER(PtgMarket), C.c_int, C.c_int, C.c_int,
                             C.POINTER(vp)]
    L.ptg_destroy.argtypes = [vp]
    L.ptg_destroy.restype = None
    L.ptg_num_envs.argtypes = [vp]
    L.ptg_obs_dim.argtypes = [vp]
    L.ptg_last_error.argtypes = [vp]
    L.ptg_last_error.restype = C.c_char_p
    L.ptg_set_market_assignment.argtypes = [vp, u8p]
    L.ptg_set_episode_plan.argtypes = [vp, dp, C.c_int, C.c_int64, C.c_int64]
    L.ptg_set_noise_tape.argtypes = [vp, dp, C.c_int]
    L.ptg_fill_noise_tape.argtypes = [vp, C.c_uint64, C.c_int, vp]
    L.ptg_set_noise_rng.argtypes = [vp, C.c_uint64]
    L.ptg_set_global_env_offset.argtypes = [vp, C.c_int64]
    L.ptg_set_feature_pitch.argtypes = [vp, C.c_int64]
    L.ptg_get_noise_tape.argtypes = [vp, dp]
    L.ptg_reset.argtypes = [vp, u8p, vp, vp]
    L.ptg_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ptg_rollout.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.ptg_rollout_info.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.ptg_rollout_launches.argtypes = [vp, C.c_int]
    L.ptg_step_host.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int), vp]
    L.ptg_host_layout.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ptg_host_layout_ex.argtypes = [vp] + [C.POINTER(C.c_size_t)] * 4
    L.ptg_step_host_begin.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.ptg_step_host_tail.argtypes = [vp, C.POINTER(C.c_int)]
    L.ptg_step_host_end.argtypes = [vp]
    L.ptg_step_host_finish.argtypes = [vp, C.POINTER(C.c_int)]
    L.ptg_host_buffers_changed.argtypes = [vp]
    L.ptg_profile.argtypes = [vp, C.c_int]
    L.ptg_profile_read.argtypes = [vp, dp, C.c_int, C.POINTER(C.c_int)]
    L.ptg_profile_read_ex.argtypes = [vp, dp, dp, dp, C.c_int, C.POINTER(C.c_int)]
    L.ptg_finished_dropped.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ptg_steps_to_episode_end.argtypes = [vp, C.POINTER(C.c_int)]
    L.ptg_note_replays.argtypes = [vp, C.c_int]
    L.ptg_set_replay_proof.argtypes = [vp, C.c_int]
    L.ptg_sync.argtypes = [vp, vp]
    L.ptg_get_state.argtypes = [vp, C.c_int, vp]
    L.ptg_set_state.argtypes = [vp, C.c_int, vp]
    L.ptg_finished_episodes.argtypes = [vp, dp, i32p, i32p, C.c_int, C.POINTER(C.c_int)]
    L.ptg_finished_episodes_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int, vp]
    L.ptg_episode_stats_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp]
    L.ptg_vn_init.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.ptg_vn_batch_moments.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.ptg_vn_apply.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp]
    L.ptg_vn_clear_done.argtypes = [vp, vp, C.c_int, vp]
    L.ptg_vn_get.argtypes = [vp, dp, dp]
    L.ptg_vn_set.argtypes = [vp, dp, dp]
    L.ptg_gae.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp]
    L.ptg_minibatch.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, vp,
                                C.c_int, C.POINTER(vp), i32p, C.POINTER(vp), vp]
    L.ptg_minibatch_drawn.argtypes = [vp, vp, C.c_uint64, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, vp,
                                      C.c_int, C.POINTER(vp), i32p, C.POINTER(vp), vp]
    L.ptg_minibatch_end_epoch.argtypes = [vp, vp, vp]
    L.ptg_replay_add.argtypes = [vp, C.POINTER(PtgReplay), vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, C.c_int, C.c_int, C.POINTER(vp), C.c_int64, vp]
    L.ptg_replay_sample.argtypes = [vp, C.POINTER(PtgReplay), vp, C.c_int64, C.c_uint64, vp, vp, C.POINTER(vp), C.c_int, vp, vp]
    L.ptg_rollout_buffer_begin.argtypes = [vp, C.POINTER(PtgRolloutBuffer), vp, C.c_int64, C.c_int64, C.c_int64, vp]
    L.ptg_rollout_buffer_add.argtypes = [vp, C.POINTER(PtgRolloutBuffer), vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), vp]
    L.ptg_act.argtypes = [vp, C.POINTER(PtgHead), vp]
    L.ptg_policy_loss_workspace.argtypes = [C.c_int64]
    L.ptg_policy_loss_workspace.restype = C.c_int64
    L.ptg_policy_loss.argtypes = [vp, C.POINTER(PtgLoss), vp]
    L.ptg_sde_resample.argtypes = [vp, C.POINTER(PtgSdeNoise), vp]
    L.ptg_sde_act.argtypes = [vp, C.POINTER(PtgSdeHead), vp]
    L.ptg_sde_policy_loss_workspace.argtypes = [C.c_int64, C.c_int32]
    L.ptg_sde_policy_loss_workspace.restype = C.c_int64
    L.ptg_sde_policy_loss.argtypes = [vp, C.POINTER(PtgSdeLoss), vp]
    L.ptg_sde_resample_rows.argtypes = [vp, C.POINTER(PtgSdeNoise), C.c_int64, vp]
    L.ptg_sde_rsample.argtypes = [vp, C.POINTER(PtgSdeRs), vp]
    L.ptg_sde_rsample_backward_workspace.argtypes = [C.c_int64, C.c_int32]
    L.ptg_sde_rsample_backward_workspace.restype = C.c_int64
    L.ptg_sde_rsample_backward.argtypes = [vp, C.POINTER(PtgSdeRs), vp]
    L.ptg_optim_chunk.argtypes = []
    L.ptg_optim_workspace.argtypes = [C.c_int64]
    L.ptg_optim_workspace.restype = C.c_int64
    L.ptg_optim_step.argtypes = [vp, C.POINTER(PtgOptim), vp]
    L.ptg_td_loss_workspace.argtypes = [C.c_int64]
    L.ptg_td_loss_workspace.restype = C.c_int64
    L.ptg_td_loss.argtypes = [vp, C.POINTER(PtgTd), vp]
    L.ptg_quantile_loss_workspace.argtypes = [C.c_int64]
    L.ptg_quantile_loss_workspace.restype = C.c_int64
    L.ptg_quantile_loss.argtypes = [vp, C.POINTER(PtgQl), vp]
    L.ptg_rsample.argtypes = [vp, C.POINTER(PtgRs), vp]
    L.ptg_rsample_backward.argtypes = [vp, C.POINTER(PtgRs), vp]
    L.ptg_actor_loss_workspace.argtypes = [C.c_int64]
    L.ptg_actor_loss_workspace.restype = C.c_int64
    L.ptg_actor_loss.argtypes = [vp, C.POINTER(PtgAl), vp]
    L.ptg_mlp_workspace.argtypes = [C.c_int64, C.c_int32, i32p, C.c_int32]
    L.ptg_mlp_workspace.restype = C.c_int64
    L.ptg_mlp_forward.argtypes = [vp, C.POINTER(PtgMlp), vp]
    L.ptg_mlp_backward_workspace.argtypes = [C.c_int64, C.c_int32, i32p, C.c_int32]
    L.ptg_mlp_backward_workspace.restype = C.c_int64
    L.ptg_mlp_backward.argtypes = [vp, C.POINTER(PtgMlpBwd), vp]
    L.ptg_mlp_group_forward.argtypes = [vp, C.POINTER(PtgMlp), C.c_int32, vp]
    L.ptg_mlp_group_backward.argtypes = [vp, C.POINTER(PtgMlpBwd), C.c_int32, vp]
    L.ptg_policy_loss_group.argtypes = [vp, C.POINTER(PtgLoss), C.c_int32, vp]
    L.ptg_optim_step_group.argtypes = [vp, C.POINTER(PtgOptim), C.c_int32, vp]
    L.ptg_td_loss_group.argtypes = [vp, C.POINTER(PtgTd), C.c_int32, vp]
    L.ptg_actor_loss_group.argtypes = [vp, C.POINTER(PtgAl), C.c_int32, vp]
    L.ptg_rsample_group.argtypes = [vp, C.POINTER(PtgRs), C.c_int32, vp]
    L.ptg_rsample_backward_group.argtypes = [vp, C.POINTER(PtgRs), C.c_int32, vp]
    L.ptg_market_feature_series.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.ptg_debug_get_index_lut.argtypes = [vp, dp, i32p, C.POINTER(C.c_int)]
    L.ptg_debug_window_record.argtypes = [vp, C.c_int, C.c_int, dp]
    L.ptg_debug_table_plan.argtypes = [vp, i32p]
    for name in EXPORTS:
        getattr(L, name)
    _lib = L
    return L
