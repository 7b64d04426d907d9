/*
 * ptg_env.h -- C ABI of the MI355X-native batched Power-to-Gas environment (libptg_env.so).
 *
 * Drop-in boundary for the reference's hot path: N independent copies of
 *     PTGEnv.step / PTGEnv.reset            /root/reference/env/ptg_gym_env.py:336-481, :483-506
 * as the reference vectorises them with SB3's DummyVecEnv (src/rl_utils.py:448-453, :484): envs are stepped
 * in env order and a finished env is reset at once.  The Python side (rl_ptg_amd/vec_env.py) binds these
 * entry points with ctypes and presents the VecEnv / gym.Env surface; INTEGRATION.md shows the reference-side
 * binding.  Plain C types only: no torch / numpy types cross this boundary.
 *
 * Pointer conventions
 *   *_host : host memory, read (or written) synchronously during the call.
 *   *_dev  : device memory on the handle's GPU (e.g. torch.Tensor.data_ptr() of a ROCm tensor), accessed
 *            asynchronously on the hipStream_t passed as `stream` (NULL = the default stream).
 * Ownership: the caller owns every buffer it passes; the library owns its device-resident state, tables and
 * price series (copies made in ptg_create) until ptg_destroy.
 * Errors: every function returns 0 on success or a negative PTG_E_* code; ptg_last_error() gives the text.
 * No C++ exception crosses the boundary.  A handle is not thread-safe; work is stream-ordered.
 */
#ifndef PTG_ENV_H
#define PTG_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTG_ABI_VERSION 13  /* 2: + ptg_rollout_launches, ptg_rollout_info, ptg_vn_*, PTG_OBS_SB3_FLAT;  3: + ptg_profile*, ptg_step_host, ptg_host_layout, PTG_OBS_SPLIT, ptg_market_feature_series;
                             * 4: + ptg_profile_read_ex, ptg_finished_dropped, ptg_host_buffers_changed, ptg_steps_to_episode_end,
                             *    ptg_host_layout_ex (status section), ptg_step_host_begin / _tail / _end / _finish, ptg_set_feature_pitch;
                             * 5: + ptg_note_replays, ptg_set_replay_proof (the hot kernels read the step count from the device state: captured launches can be replayed);
                             * 6: + ptg_vn_clear_done (frozen reward normalisation clears the returns of finished envs on the device);
                             * 7: + ptg_debug_table_plan;
                             * 8: + ptg_finished_episodes_dev, ptg_episode_stats_dev (the finished-episode list handed over on the device);
                             * 9: + ptg_gae (advantages and returns of a rollout on the device);
                             * 10: + ptg_minibatch, PTG_E_INDEX (shuffled minibatches gathered from the rollout buffers on the device);
                             * 11: + ptg_replay, ptg_replay_add, ptg_replay_sample (the off-policy algorithms' replay buffer on the device);
                             * 12: + ptg_head, ptg_act, PTG_E_NONFINITE (policy outputs to actions, log-probs and entropy in one launch);
                             * 13: + ptg_loss, ptg_policy_loss, ptg_policy_loss_workspace (the PPO / A2C loss and its gradients in one pass);
                             *     additive, version unchanged: + ptg_optim, ptg_optim_step, ptg_optim_workspace, ptg_optim_chunk (the optimiser step behind
                             *     the loss: grad-norm clip, Adam / RMSprop, Polyak, zero_grad); + ptg_td, ptg_td_loss, ptg_td_loss_workspace (DQN's
                             *     and the TD3 / SAC critics' loss with its gradients); + ptg_ql, ptg_quantile_loss, ptg_quantile_loss_workspace (TQC's
                             *     quantile-Huber critic loss with its gradients); + ptg_rs, ptg_rsample, ptg_rsample_backward (the training-time
                             *     actor head of SAC / TQC forward and backward, TD3's smoothed target action); + ptg_al, ptg_actor_loss,
                             *     ptg_actor_loss_workspace (the SAC / TQC / TD3 actor loss and the entropy-coefficient loss with their
                             *     gradients); + ptg_mlp, ptg_mlp_forward, ptg_mlp_workspace (the inference forward of the policy and target MLPs,
                             *     one fused f32 MFMA launch per layer); + ptg_mlp_bwd, ptg_mlp_backward, ptg_mlp_backward_workspace (the backward pass
                             *     of those MLPs, two f32 MFMA launches per layer); + PTG_MLP_GROUP_MAX, ptg_mlp_group_forward, ptg_mlp_group_backward
                             *     (up to eight MLPs of equal depth in the launches of one); + ptg_rollout_buffer, ptg_rollout_buffer_begin, ptg_rollout_buffer_add
                             *     (the on-policy algorithms' collect storage with its cursor on the device); + ptg_sde_noise, ptg_sde_head, ptg_sde_loss, ptg_sde_resample,
                             *     ptg_sde_act, ptg_sde_policy_loss, ptg_sde_policy_loss_workspace (gSDE: the state-dependent exploration head while
                             *     collecting and its PPO / A2C loss); + ptg_sde_rs, ptg_sde_resample_rows, ptg_sde_rsample,
                             *     ptg_sde_rsample_backward, ptg_sde_rsample_backward_workspace (gSDE for SAC / TQC: the squashed head, its reparametrised sample and the
                             *     backward); + ptg_minibatch_drawn, ptg_minibatch_end_epoch (ptg_minibatch with its indices drawn on the device from an
                             *     epoch cursor, so a PPO / A2C gradient step replays); + PTG_TRAIN_GROUP_MAX, ptg_policy_loss_group, ptg_optim_step_group (the loss
                             *     and the optimiser step of up to eight independent PPO / A2C agents in the launches of one); no earlier declaration changed */
#define PTG_N_TABLES 17
#define PTG_N_COLS 7
#define PTG_N_INFO 24
#define PTG_MAX_MARKET_SETS 4

enum {
    PTG_OK = 0,
    PTG_E_INVALID = -1,        /* bad argument / call order */
    PTG_E_HIP = -2,            /* a HIP runtime call failed (no device, out of memory, ...) */
    PTG_E_ACTION = -3,         /* a discrete action outside [-5, 4] reached a kernel (reference: IndexError, :347) */
    PTG_E_RANGE = -4,          /* a price index left the series (reference: IndexError, :446-447) */
    PTG_E_INDEX = -5,          /* ptg_minibatch / ptg_replay_sample met a sample index out of range (NumPy: IndexError); ptg_policy_loss / ptg_td_loss an action outside [0, A); ptg_rollout_buffer_add a full buffer */
    PTG_E_NONFINITE = -6       /* ptg_act met a row it cannot act on: NaN / +Inf input, all -Inf logits, NaN parameter, epsilon outside [0, 1];
                                * ptg_policy_loss / ptg_td_loss / ptg_quantile_loss / ptg_actor_loss a row it has no finite loss for;
                                * ptg_rsample / ptg_rsample_backward a non-finite mean, log_std, noise or incoming gradient */
};

/* table ids: order of op_data_files, src/rl_utils.py:108-113 */
enum {
    PTG_T_STARTUP_COLD = 0, PTG_T_STARTUP_HOT, PTG_T_COOLDOWN, PTG_T_STANDBY_DOWN, PTG_T_STANDBY_UP,
    PTG_T_OP1_START_P, PTG_T_OP2_START_F, PTG_T_OP3_P_F, PTG_T_OP4_P_F_P_5, PTG_T_OP5_P_F_P_10,
    PTG_T_OP6_P_F_P_15, PTG_T_OP7_P_F_P_22, PTG_T_OP8_F_P, PTG_T_OP9_F_P_F_5, PTG_T_OP10_F_P_F_10,
    PTG_T_OP11_F_P_F_15, PTG_T_OP12_F_P_F_20
};

enum { PTG_ACT_I32 = 0, PTG_ACT_F32 = 1, PTG_ACT_I64 = 2 };   /* element type of the action buffer */
enum { PTG_OUT_F32 = 0, PTG_OUT_F64 = 1 };                    /* element type of obs / reward buffers */
/* Observation matrix layout.  ROW_MAJOR [N][F] is what DummyVecEnv hands to SB3 (one row per env).  FEATURE_MAJOR [F][N]
 * is the struct-of-arrays form the kernels write with fully coalesced stores (a wave writes 64 consecutive envs of one
 * feature); its transpose view is the same [N][F] matrix, e.g. torch: obs.t(). Rollouts: [T][N][F] resp. [T][F][N].
 * SB3_FLAT [N][F + 5] is the row SB3's CombinedExtractor builds from the Dict observation (the reference's policies are
 * "MultiInputPolicy"): sub-spaces concatenated in sorted key order, the Discrete(6) METH_STATUS one-hot encoded -- 40
 * columns for 'mod', 31 for 'raw' at price_ahead 13; ptg_obs_dim() reports the width.  Replaces: obs_as_tensor +
 * preprocess_obs + CombinedExtractor.forward on the caller's side.
 * SPLIT [N][16] (float32): the part of the SB3_FLAT row that depends on the env's own state, plus WHERE its market features are:
 *   columns 0-5 METH_STATUS one-hot, 6 T_CAT, 7 H2_in, 8 CH4_syn, 9 H2_res, 10 H2O_DE, 11 Elec_Heating, 12 sin, 13 cos,
 *   14 hour index, 15 day index -- the start of the env's 13-hour (2-day) windows in the normalised feature series of
 *   ptg_market_feature_series (index = market_set * series_length + hour or day; exact in float32 up to 2^24).  That series is
 *   float32 whatever out_dtype is: a float64 handle's SPLIT rows hold float64 env columns, but the market columns a consumer rebuilds
 *   from the indices carry one float32 rounding of the float64 feature (tests/test_split_oracle.py compares them at that tolerance).
 * The 26 ('raw': 17) market features of a row are a function of that index alone, so a policy's first layer can be evaluated as
 *   W_env . row[0:14] + G[hour index] (+ G_day[day index]),  G = the market columns of W applied to every window of the series
 * (rl_ptg_amd/policy_split.py): 73 instead of 169 bytes per env-step leave the env kernel, and the first layer multiplies 14
 * instead of 40 inputs.  The project's own networks take the rows as they are: ptg_mlp_forward / ptg_mlp_backward and the group calls
 * with PTG_MLP_SPLIT_INPUT rebuild the flat row inside the first layer's operand fetch, with the bits of the flat call and no table
 * (below, and DESIGN.md section 21).  Replaces: the market sub-spaces of the Dict observation going through CombinedExtractor into the first
 * Linear of the reference's MultiInputPolicy (src/rl_config_agent.py:126-149). */
enum { PTG_OBS_ROW_MAJOR = 0, PTG_OBS_FEATURE_MAJOR = 1, PTG_OBS_SB3_FLAT = 2, PTG_OBS_SPLIT = 3 };

/* Constants of the env: the flat kwargs of Preprocessing.dict_env_kwargs (src/rl_utils.py:345-365), same names.
 * Replaces: the attribute set PTGEnv.__init__ copies from dict_input (env/ptg_gym_env.py:40). */
typedef struct ptg_config {
    double noise;                       /* config_env.yaml:28; informational for host tapes, sigma of ptg_fill_noise_tape */
    int32_t eps_len_d, sim_step, time_step_op, price_ahead;
    double convert_mol_to_Nm3, H_u_CH4, H_u_H2, dt_water, cp_water, rho_water, Molar_mass_CO2,
           Molar_mass_H2O, h_H2O_evap, eeg_el_price, heat_price, o2_price, water_price,
           min_load_electrolyzer, max_h2_volumeflow, eta_CHP;
    double t_cat_standby, t_cat_startup_cold, t_cat_startup_hot;
    int32_t time1_start_p_f, time2_start_f_p, time_p_f, time_f_p, time1_p_f_p, time2_p_f_p, time23_p_f_p,
            time3_p_f_p, time34_p_f_p, time4_p_f_p, time45_p_f_p, time5_p_f_p, time1_f_p_f, time2_f_p_f,
            time23_f_p_f, time3_f_p_f, time34_f_p_f, time4_f_p_f, time45_f_p_f, time5_f_p_f,
            i_fully_developed, j_fully_developed;
    double el_l_b, el_u_b, gas_l_b, gas_u_b, eua_l_b, eua_u_b, T_l_b, T_u_b, h2_l_b, h2_u_b, ch4_l_b,
           ch4_u_b, h2_res_l_b, h2_res_u_b, h2o_l_b, h2o_u_b, heat_l_b, heat_u_b;
    int32_t raw_modified;               /* 0 = "raw" (26 features), 1 = "mod" (35 features); :165,185 */
    int32_t action_type;                /* 0 = "discrete", 1 = "continuous"; :144-158 */
    int32_t train_or_eval;              /* 0 = "train", 1 = "eval" (info rows available); :471-474 */
    int32_t eps_sim_steps;              /* :508-511 */
    double state_change_penalty;        /* :332 */
    double t_cat_initial;               /* 16 in the reference (:117) */
    int32_t out_dtype;                  /* PTG_OUT_F32 | PTG_OUT_F64 */
    int32_t obs_layout;                 /* PTG_OBS_ROW_MAJOR | PTG_OBS_FEATURE_MAJOR | PTG_OBS_SB3_FLAT | PTG_OBS_SPLIT */
} ptg_config;

/* The 17 process tables (src/rl_utils.py:46-67): row-major [rows][7] = t, T_cat, n_h2, n_ch4, n_h2_res, m_h2o, P_el */
typedef struct ptg_tables {
    const double* data_host[PTG_N_TABLES];
    int32_t rows[PTG_N_TABLES];
} ptg_tables;

/* One business scenario's market view as 1-D series.  Replaces the materialised tensors
 *   e_r_b[c, i, t] == series_c[t + i]  (src/rl_utils.py:250-263)   g_e[c, i, d] == series_c[d + i]  (:266-281)
 * plus the scenario-dependent scalars (b_s3 env/ptg_gym_env.py:76-77; rew_l_b/u_b src/rl_utils.py:378-379;
 * r_0 = reward_level[0] env/ptg_gym_env.py:125).  All sets of one handle share n_hours / n_days. */
typedef struct ptg_market {
    int32_t n_hours;                    /* >= last hour index used + price_ahead */
    const double* el_host;              /* ct/kWh */
    const double* pot_rew_host;         /* ct/h   (calculate_optimum, src/rl_opt.py:26-152, column 20) */
    const double* part_full_host;       /* -1/0/1 (column 23) */
    int32_t n_days;
    const double* gas_host;             /* ct/kWh, scenario override applied (src/rl_utils.py:119-126) */
    const double* eua_host;             /* Euro/t */
    int32_t scenario;                   /* 1, 2 or 3 */
    int32_t reserved;
    double rew_l_b, rew_u_b, r_0;
} ptg_market;

typedef struct ptg_env ptg_env;

/* ---- life cycle ---------------------------------------------------------------------------------------- */
/* Builds the device-resident tables for step_size = sim_step / time_step_op:
 *   window records (row 12 of SURVEY §8a: T of the last row + NumPy-pairwise means of the 5 flow columns for every
 *   possible window start, incl. the table-end / startup->partial splice cases of _perform_sim_step :525-557) and
 *   the _get_index lookup (:514-523) for every distinct catalyst temperature x 6 destination tables.
 * Replaces PTGEnv.__init__ (:28-79) for n_envs envs.  Envs must be reset before the first step. */
int ptg_create(const ptg_config* cfg, const ptg_tables* tables, const ptg_market* sets, int n_sets,
               int n_envs, int device_id, ptg_env** out);
void ptg_destroy(ptg_env* env);
int ptg_abi_version(void);
int ptg_num_envs(const ptg_env* env);
int ptg_obs_dim(const ptg_env* env);                 /* 35 ('mod') / 26 ('raw') for price_ahead = 13 */
const char* ptg_last_error(const ptg_env* env);      /* env may be NULL: error of the last failed ptg_create */

/* ---- configuration of the batch ------------------------------------------------------------------------ */
/* market set (business scenario) of every env; default 0 */
int ptg_set_market_assignment(ptg_env* env, const uint8_t* set_of_env_host);
/* Training episodes (env/ptg_gym_env.py:59-62, :490-493): eps_ind as the reference holds it.  Env e takes
 * eps_ind[(first_ptr + e + m*stride) mod n] at its m-th reset from now on: with first_ptr = N_total + shard_offset and
 * stride = N_total this is the order in which N_total reference envs sharing the module-global ep_index reset under
 * DummyVecEnv when they terminate together (exclusive prefix sum over done flags).  n = 0: validation/test env. */
int ptg_set_episode_plan(ptg_env* env, const double* eps_ind_host, int n, int64_t first_ptr, int64_t stride);
/* Normal draws consumed at state changes (:584-585,598-599,620-621): the c-th draw of env e is tape[e*len + c mod len].
 * Host tape (e.g. numpy Generator.normal(0, noise) per env for bit parity with the reference), env-major [n_envs][per_env_len] as
 * written here; the library keeps it draw-major on the device (ptg_set / get_noise_tape transpose, a temporary device buffer of the
 * tape's size while they run) ... */
int ptg_set_noise_tape(ptg_env* env, const double* tape_host, int per_env_len);
/* ... or the device's counter-based generator: the c-th draw of the env with GLOBAL index g is
 *   noise(seed, g, c) = cfg.noise * BoxMuller(u1, u2),  (u1, u2) from three rounds of the 32-bit integer finaliser "lowbias32"
 *   keyed by (seed, g, c); Box-Muller in float32 with the hardware log2 / sqrt / cos instructions.
 * ptg_set_noise_rng draws it inside the step kernels (no tape, unbounded); ptg_fill_noise_tape writes the first per_env_len
 * draws of the same streams to the tape (so both modes give identical trajectories while the tape does not wrap).
 * Both reset the per-env draw counters.  Statistically equivalent to, not bit-equal with, NumPy's Generator.normal. */
int ptg_set_noise_rng(ptg_env* env, uint64_t seed);
int ptg_fill_noise_tape(ptg_env* env, uint64_t seed, int per_env_len, void* stream);
/* FEATURE_MAJOR outputs only: elements between two feature planes of the caller's observation buffers (obs_dev, final_obs_dev, the
 * observation section of a host block; rollouts: [T][F][pitch]), n_envs <= pitch <= n_envs + 2^20; default n_envs (planes back to back).
 * Element (t, q, e) lives at ((t * F + q) * pitch + e).  Why: with float64 outputs and a power-of-two batch the planes are 2^19 bytes
 * apart and the 35 stores of a wave differ only above bit 19 -- measured 0.59 of the HBM peak; a pitch of n_envs + 128 elements
 * (1 KiB) brings 0.70 (profiles/r03_fm_pitch.txt: pads of 256 B .. 130 KiB; 4 KiB and 64 KiB multiples do not help) for a consumer
 * that can read a pitched matrix (torch: storage [F, pitch], view [:, :n_envs]).  float32 planes (2^18 bytes apart) do not need it.
 * No reference counterpart (the reference has no batch dimension). */
int ptg_set_feature_pitch(ptg_env* env, int64_t pitch_elems);
/* global index of this handle's env 0 (multi-GPU shards): keys the RNG streams; default 0 */
int ptg_set_global_env_offset(ptg_env* env, int64_t offset);
int ptg_get_noise_tape(ptg_env* env, double* tape_host);          /* [n_envs][per_env_len] */

/* ---- the hot path --------------------------------------------------------------------------------------- */
/* reset (:483-506) of all envs (mask_host NULL) or of those with mask != 0; obs rows of reset envs are written. */
int ptg_reset(ptg_env* env, const uint8_t* mask_host, void* obs_dev, void* stream);
/* One vector step (:336-481) + DummyVecEnv auto-reset.
 *   actions_dev  [N]     int32 / float32 / int64 per action_kind (PTG_ACT_*)
 *   obs_dev      [N][F]  out_dtype ([F][N] when cfg.obs_layout is FEATURE_MAJOR; final_obs_dev alike);
 *                        row of a finished env = observation after its reset
 *   rew_dev      [N]     out_dtype
 *   done_dev     [N]     uint8
 *   final_obs_dev[N][F]  (nullable) rows of finished envs = terminal observation
 *   info_dev     [N][24] (nullable, float64) _get_info (:251-278) in key order, Meth_Action as its index */
int ptg_step(ptg_env* env, const void* actions_dev, int action_kind, void* obs_dev, void* rew_dev,
             uint8_t* done_dev, void* final_obs_dev, double* info_dev, void* stream);
/* T vector steps fused, state held in registers: actions [T][N] -> obs [T][N][F], rew [T][N], done [T][N].
 * Same results as T calls of ptg_step.  One kernel launch covers up to 65 536 envs and as many steps as fit its LDS action
 * stage (a few hundred); wider batches / longer rollouts are issued as consecutive launches on `stream`. */
int ptg_rollout(ptg_env* env, const void* actions_dev, int action_kind, int n_steps, void* obs_dev, void* rew_dev,
                uint8_t* done_dev, void* stream);
/* ptg_rollout that also records the 24 _get_info fields of every step: info_dev [T][N][24] float64 (key order of
 * env/ptg_gym_env.py:251-278, Meth_Action as its index).  Replaces: the per-step info dicts Postprocessing.test_performance
 * collects into its stats array (src/rl_utils.py:528-565).  float64 outputs: the fused rollout kernel writes the rows (it evaluates
 * the reference-order reward terms anyway); float32 outputs: the generic step kernel, T launches. */
int ptg_rollout_info(ptg_env* env, const void* actions_dev, int action_kind, int n_steps, void* obs_dev, void* rew_dev,
                     uint8_t* done_dev, double* info_dev, void* stream);
/* One vector step with HOST buffers in and out -- the call behind VecEnv.step_wait.  Replaces DummyVecEnv.step_wait's loop
 * `for env_idx: obs, rew, terminated, truncated, info = envs[env_idx].step(actions[env_idx])` + `_save_obs` (SB3 dummy_vec_env.py,
 * as the reference builds it in src/rl_utils.py:448-453).
 *   actions_host  [N] of action_kind
 *   out_host      one block: observations [N][F] (layout per cfg.obs_layout) at offset 0, rewards [N] at off_rew, done flags
 *                 [N] uint8 at off_done (ptg_host_layout gives the offsets and the total size; all 16-byte aligned)
 *   final_obs_host [N][F] (nullable): rows of the envs whose episode ended = terminal observation; written only when *n_done > 0
 *   info_host     [N][24] float64 (nullable; needs cfg.train_or_eval = 1)
 *   n_done        number of envs whose episode ended on this step
 * Synchronises `stream` before it returns and reports kernel-flagged errors (PTG_E_ACTION / PTG_E_RANGE) like ptg_sync.
 * When the blocks are pinned, device-mapped host memory (hipHostMalloc, torch pin_memory) and small (<= 256 KiB in all) the
 * kernels read and write them in place -- no copies; otherwise the library stages through device buffers with one copy each way. */
int ptg_host_layout(const ptg_env* env, size_t* off_rew, size_t* off_done, size_t* total);
int ptg_step_host(ptg_env* env, const void* actions_host, int action_kind, void* out_host, void* final_obs_host, double* info_host,
                  int* n_done, void* stream);
/* The out_host block has a fourth section since ABI 4 (ptg_host_layout's `total` includes it): "status" [N] uint8 at off_status = the
 * METH_STATUS of every env's returned observation row, contiguous -- what a NumPy caller turns into the int64 METH_STATUS vector of
 * the Dict observation (:219-249) without gathering one column out of N rows. */
int ptg_host_layout_ex(const ptg_env* env, size_t* off_rew, size_t* off_done, size_t* off_status, size_t* total);
/* ptg_step_host in three phases, for a caller with work of its own to overlap (VecEnv.step_async / step_wait):
 *   ptg_step_host_begin  enqueues everything on `stream` and returns: actions in, the step kernel(s), the outputs back -- as two copies
 *                        for staged batches, [rewards | done flags | status] (+ info rows) first, the observations behind them;
 *   ptg_step_host_tail   waits until rewards, done flags, status (and info rows) are in out_host and counts the finished envs -- the
 *                        observations of a large batch are still crossing PCIe while the caller works on the small part;
 *   ptg_step_host_end    waits for the observations, reports kernel-flagged errors (PTG_E_ACTION / PTG_E_RANGE), and fetches the terminal
 *                        observations when episodes ended.  One host step at a time per handle; ptg_step_host == begin + tail + end. */
int ptg_step_host_begin(ptg_env* env, const void* actions_host, int action_kind, void* out_host, void* final_obs_host, double* info_host,
                        void* stream);
int ptg_step_host_tail(ptg_env* env, int* n_done);
int ptg_step_host_end(ptg_env* env);
int ptg_step_host_finish(ptg_env* env, int* n_done);      /* tail + end in one call */
/* ptg_step_host remembers, per buffer ADDRESS (the last 8), whether the buffer is device-mapped pinned memory.  A buffer must stay
 * allocated / registered for as long as it is passed to ptg_step_host; a caller that frees one and later passes memory of another
 * kind at the same address calls this first (forgets the classifications). */
int ptg_host_buffers_changed(ptg_env* env);
/* hipGraph capture.  ptg_step / ptg_rollout enqueue kernels only (no synchronisation, no host round trip), so they can be captured on
 * `stream` -- e.g. together with the policy's forward pass, whose ~10 launches per step otherwise bound a device-resident collect loop
 * (profiles/r03_policy_loop.txt) -- and the captured launches can be REPLAYED: the hot kernels read the common step count from the device
 * state.
 *   * A captured ptg_step, by default, is the hot kernel alone: replay it at most ptg_steps_to_episode_end() - 1 times and make the
 *     episode's terminating step an eager call (a replay that reaches that step raises PTG_E_INVALID at the next synchronising call).
 *     After ptg_set_replay_proof(env, 1) a captured ptg_step is enqueued as the hot kernel, which does nothing when it finds the batch on
 *     the terminating step, plus the generic kernel behind it, which does nothing otherwise -- a replay takes the right one by itself,
 *     across episode ends, auto-reset (episode plan) and finished-episode list included, for the price of one empty launch per step
 *     (+1.5-2 us).  final_obs_dev of the captured call receives the terminal observations.
 *   * A captured ptg_rollout must not be replayed across an episode end (a fused launch cannot terminate; eager calls are cut there by
 *     the host): ptg_steps_to_episode_end() says how far it may go; a replay that runs over raises PTG_E_INVALID at the next
 *     synchronising call.
 *   * ptg_note_replays(env, n): after replaying captured launches that together advanced the batch by n vector steps BEYOND the first
 *     replay (the capture call counts as executed once, like an eager call), so that eager calls, ptg_steps_to_episode_end,
 *     ptg_rollout_launches and ptg_finished_episodes stay in step; the count wraps at the episode length.  On a de-synchronised batch
 *     there is no common count: the call only tells ptg_finished_episodes that replays may have finished episodes.
 *   * De-synchronising the batch (a partial ptg_reset, or ptg_set_state of unequal step counts) invalidates the hot launches captured
 *     before it: their kernels take the step count from one env.  The library keeps a device word in stream order with the batch's
 *     synchronisation (ptg_create, ptg_reset, ptg_set_state of the step count), and a replayed hot kernel that finds it set takes no
 *     step: a default captured ptg_step or a captured ptg_rollout leaves the state and its outputs untouched and raises PTG_E_INVALID at
 *     the next synchronising call; a replay-proof ptg_step hands every step to its generic kernel, which steps each env by its own
 *     count (correct, at the generic kernel's speed).  A full ptg_reset (or ptg_set_state of equal step counts) re-arms the captured
 *     launches.  A ptg_step captured while the batch is de-synchronised is the generic kernel and replays correctly either way.
 * Buffers are the graph's (fixed addresses); kernel-flagged errors surface at the next ptg_sync / ptg_step_host / ptg_finished_episodes.
 * No reference counterpart. */
int ptg_note_replays(ptg_env* env, int n_steps);
int ptg_set_replay_proof(ptg_env* env, int enable);
/* Number of kernel launches ptg_rollout(env, ..., n_steps, ...) would issue from the envs' current position (for
 * per-launch timing); negative PTG_E_* on a bad argument. */
int ptg_rollout_launches(ptg_env* env, int n_steps);
/* Per-launch device time of the hot kernels (bench.py's roofline figure; no reference counterpart -- the reference times
 * env.step with time.perf_counter at best).  ptg_profile(env, 1) starts a collection: every k_step_hot / k_rollout_pc launch
 * from then on carries a (start, stop) HIP event pair stamped at the kernel's own begin and end (hipExtLaunchKernelGGL), i.e.
 * what `rocprofv3 --kernel-trace` reports for the dispatch, without host launch latency in the interval.  ptg_profile(env, 0)
 * stops it.  ptg_profile_read waits for the recorded launches, returns their durations in microseconds in launch order
 * (count = min(launches, cap)) and clears the collection.  Launches being captured into a hipGraph must not be profiled. */
int ptg_profile(ptg_env* env, int enable);
int ptg_profile_read(ptg_env* env, double* us_host, int cap, int* count);
/* ptg_profile_read with the launches' helper kernel accounted for.  A rollout launch may run a table refresher beside it (k_refresh on
 * a stream forked from the caller's: the rolling passes of a long launch right after a synchronised reset; the pass at the head of a
 * launch is part of the rollout kernel itself).  Per recorded launch: us_host = the kernel's own duration, helper_us_host (nullable)
 * = its helper's duration or 0, span_us_host (nullable) = the length of the UNION of the two intervals, first start to last end --
 * the figure bench.py's roofline uses. */
int ptg_profile_read_ex(ptg_env* env, double* us_host, double* helper_us_host, double* span_us_host, int cap, int* count);
/* hipStreamSynchronize(stream) + report an error a kernel flagged (PTG_E_ACTION / PTG_E_RANGE / PTG_E_INDEX / PTG_E_NONFINITE). */
int ptg_sync(ptg_env* env, void* stream);

/* ---- state access (parity tests, checkpointing) -------------------------------------------------------- */
enum {
    PTG_F_METH_STATE = 0, PTG_F_I, PTG_F_J, PTG_F_K, PTG_F_HOT_COLD, PTG_F_STANDBY_TID, PTG_F_STARTUP_TID,
    PTG_F_PARTIAL_TID, PTG_F_FULL_TID, PTG_F_CURRENT_ACTION, PTG_F_ACT_EP_D, PTG_F_EP_PTR, PTG_F_NOISE_COUNT,
    PTG_F_N_STATE_CHANGES, PTG_F_MARKET_SET,       /* int32[N] */
    PTG_F_T_CAT = 32, PTG_F_CUM_REW                /* float64[N] */
};
int ptg_get_state(ptg_env* env, int field, void* out_host);
int ptg_set_state(ptg_env* env, int field, const void* in_host);

/* Episodes finished since the last call (Monitor's info["episode"]: r = sum of returned rewards, l = steps),
 * compacted on the device with a wave ballot prefix.  Returns up to cap entries and clears the list.  The list is a ring
 * of max(2 * n_envs, 1024) entries: when more episodes finish between two calls the oldest are dropped.  Synchronises the
 * device only if a launch that can finish episodes (a generic / terminating step) ran since the last call. */
int ptg_finished_episodes(ptg_env* env, double* returns_host, int32_t* lengths_host, int32_t* env_ids_host,
                          int cap, int* count);
/* When can the next episode end?  A batch whose envs share one step count (reset together, stepped together -- every batch until a
 * partial reset or ptg_set_state de-synchronises it) ends its episodes on ONE known vector step (:508-511): *steps = the number of
 * vector steps from now up to and including that one (>= 1).  *steps = 0: not known to the host (an episode may end on any step).
 * A sharded job uses it to issue the episodic-return all-gather only in windows that contain an episode boundary. */
int ptg_steps_to_episode_end(ptg_env* env, int* steps);
/* Finished episodes that were never handed out since ptg_create: overwritten in the ring before a query came, or cut off by a
 * query's `cap`.  0 for every caller that queries at least once per 2 * n_envs finished episodes with cap >= that.  Counts the host
 * query (ptg_finished_episodes) only: a device drain reports its own drops in count_dev[1]. */
int ptg_finished_dropped(ptg_env* env, uint64_t* dropped_total);
/* Stream-ordered hand-over of the finished-episode list, device to device.  Enqueues kernels only: no host
 * synchronisation, no host copy, so it may be captured into a hipGraph behind a (replay-proof) ptg_step.
 *   ret_dev  [cap] float64   len_dev [cap] int32   env_dev [cap] int32 (GLOBAL env index = offset + e)   -- each nullable
 *   count_dev uint32[2]: [0] entries in the caller's list, [1] entries dropped
 *   append = 0: the list starts at 0 (count_dev is overwritten);  append = 1: entries go behind count_dev[0], drops add to [1]
 * Takes the live entries of the ring oldest first (the order ptg_finished_episodes hands out), at most cap - count_dev[0]
 * of them; what does not fit, and what the ring had already overwritten, is counted in count_dev[1]; the ring is empty
 * afterwards either way.  Must be ordered (same stream, or events) behind the launches whose episodes it collects.
 * PTG_E_INVALID (nothing enqueued): count_dev NULL, cap < 1, or all three arrays NULL.  The host query's bookkeeping is not
 * touched: a ptg_finished_episodes after a drain still synchronises and finds an empty ring.
 * Replaces: reading Monitor's info["episode"] out of the step infos on the host (SB3 monitor.py, as the reference wraps its
 * envs in src/rl_utils.py:448-453) for a collect loop that never leaves the device. */
int ptg_finished_episodes_dev(ptg_env* env, double* ret_dev, int32_t* len_dev, int32_t* env_dev, int cap,
                              uint32_t* count_dev, int append, void* stream);
/* Monitor's statistic of a device list: stats_dev float64[6] = {count, sum r, sum r^2, sum len, min r, max r} over the first
 * count_dev[0] entries (accumulate = 1: merged into what stats_dev holds; min / max of an empty list are +inf / -inf).
 * len_dev may be NULL (sum len = 0).  Deterministic: a fixed reduction order, no floating-point atomics -- the same list gives
 * the same bits on every call.  ep_rew_mean = stats[1] / stats[0]. */
int ptg_episode_stats_dev(ptg_env* env, const double* ret_dev, const int32_t* len_dev, const uint32_t* count_dev,
                          double* stats_dev, int accumulate, void* stream);

/* ---- VecNormalize(env, norm_obs=False) reward normalisation on the device ------------------------------------------
 * Replaces: stable_baselines3.common.vec_env.VecNormalize.step_wait / _update_reward / normalize_reward and
 * RunningMeanStd.update (SB3 2.0.0a13, the reference's pin; wrapped around the env in src/rl_utils.py:453), over a
 * [T][N] reward matrix as ptg_rollout (T >= 1) or ptg_step (T = 1) writes it:
 *   returns = returns * gamma + reward;  running moments of `returns` updated with the step's batch mean / variance;
 *   reward_out = clip(reward / sqrt(var + epsilon), +-clip_reward);  returns[done] = 0.
 * Two phases so that a job sharded over GPUs normalises with the moments of ALL envs: ptg_vn_batch_moments advances this
 * handle's returns and yields per-step (count, mean, M2) of its envs; the caller merges the shards' moments (Chan's formula,
 * rl_ptg_amd.dist.merge_moments -- one all-gather per rollout) and hands the merged [T][3] array to ptg_vn_apply, which
 * updates the running statistics step by step and writes the normalised rewards.  moments_dev NULL = single-GPU: the
 * handle's own moments are used.  A NaN reward propagates as in np.clip (NaN statistics, NaN outputs from then on).
 * Frozen statistics (SB3 training = False): skip ptg_vn_batch_moments, call ptg_vn_apply with training = 0 (returns not
 * advanced, statistics unchanged) and ptg_vn_clear_done with the window's [T][N] done flags, which does returns[done] = 0:
 * an env's return is zeroed iff any of its T flags is set. */
int ptg_vn_init(ptg_env* env, double gamma, double epsilon, double clip_reward);      /* SB3 defaults: 0.99, 1e-8, 10.0 */
int ptg_vn_batch_moments(ptg_env* env, const void* rew_dev, const uint8_t* done_dev, int n_steps, double* moments_dev, void* stream);
int ptg_vn_apply(ptg_env* env, const void* rew_dev, int n_steps, const double* moments_dev, void* rew_out_dev, int training,
                 void* stream);
int ptg_vn_clear_done(ptg_env* env, const uint8_t* done_dev, int n_steps, void* stream);
/* running statistics {mean, var, count} and the per-env discounted returns (either pointer may be NULL) */
int ptg_vn_get(ptg_env* env, double* stats3_host, double* returns_host);
int ptg_vn_set(ptg_env* env, const double* stats3_host, const double* returns_host);

/* ---- generalised advantage estimation of a rollout on the device ----------------------------------------------------
 * Replaces: stable_baselines3.common.buffers.RolloutBuffer.compute_returns_and_advantage (SB3 2.0.0a13), which the
 * reference's A2C and PPO run after every collect (gamma / gae_lambda / n_steps of config/config_agent.yaml) -- a Python loop
 * backwards over the n_steps rows of the buffer -- over the [T][N] matrices a rollout leaves on the device:
 *   rew_dev  [T][N]  rewards (as ptg_rollout or ptg_vn_apply wrote them)
 *   val_dev  [T][N]  V of the observation the action of step t was chosen from
 *   done_dev [T][N]  uint8, ptg_rollout's convention: done[t][e] != 0 = env e's episode ended ON step t.  SB3's
 *                    episode_starts[t + 1] is done[t] and its final `dones` argument is done[T - 1], so the non-terminal
 *                    factor of step t is 1 - done[t] for every t, the last one included
 *   last_val_dev [N] V of the observation after step T - 1
 *   adv_dev  [T][N]  advantages;  ret_dev [T][N] (nullable) returns = advantages + values
 * dtype (PTG_OUT_F32 | PTG_OUT_F64) is the element type of all five float arrays, whatever the handle's out_dtype is (a
 * critic is float32 on a float64 engine too).  Arithmetic: SB3's, in that type, in SB3's operand order, every operation
 * rounded once (no fused multiply-add), backwards over t with last = 0 before t = T - 1:
 *   nnt = 1 - done[t];   nv = t == T - 1 ? last_val : val[t + 1];   g = (dtype)gamma;   gl = (dtype)(gamma * gae_lambda)
 *   delta = (rew[t] + (g * nv) * nnt) - val[t];   last = delta + ((gl * nnt) * last);   adv[t] = last;   ret[t] = last + val[t]
 * -- bit for bit what NumPy computes on arrays of that type.  nnt multiplies, it does not select: a NaN or Inf next value at a
 * finished step poisons that step's result as it does in NumPy.
 * Aliasing: adv_dev may be rew_dev and ret_dev may be val_dev (a lane reads its column's element before it writes it);
 * no other overlap between inputs and outputs.
 * The reference never truncates an episode (env/ptg_gym_env.py:478-481: truncated is always False), so there is no
 * time-limit bootstrap to add to the rewards and none is needed.
 * Enqueues one kernel on `stream`: no host synchronisation, no allocation, so it may be captured into a hipGraph.  Reads
 * nothing of the handle but its n_envs and device and writes nothing of it but, on a refusal, the ptg_last_error text:
 * env state, the finished-episode ring and the ptg_vn_* statistics are untouched.  PTG_E_INVALID (nothing enqueued): NULL handle, NULL rew / val / done / last_val / adv,
 * n_steps < 1, a dtype other than the two, a non-finite gamma or gae_lambda. */
int ptg_gae(ptg_env* env, const void* rew_dev, const void* val_dev, const uint8_t* done_dev, const void* last_val_dev,
            int n_steps, int dtype, double gamma, double gae_lambda, void* adv_dev, void* ret_dev, void* stream);

/* ---- one shuffled minibatch gathered from the buffers of a rollout on the device -----------------------------------
 * Replaces: stable_baselines3.common.buffers.RolloutBuffer.get / _get_samples (SB3 2.0.0a13), through which the reference's
 * PPO (config/config_agent.yaml: batch_size 203, n_steps 21 * batch_size) and A2C (get(None): one batch of everything) read
 * every training batch: swap_and_flatten turns each [T][N][...] buffer into [N * T][...], a permutation of T * N is drawn,
 * and each batch is the rows indices[start : start + batch_size] of every buffer.  Here nothing is transposed or copied
 * beforehand: one launch gathers one batch straight from the [T][N] layout the rollout, ptg_vn_apply and ptg_gae leave.
 *   idx_dev [B]        int32 (idx_bytes 4) or int64 (idx_bytes 8) sample indices in swap_and_flatten's order:
 *                      i = e * n_steps + t, 0 <= i < n_steps * n_envs, names step t of env e.  The caller draws the
 *                      permutation (any device RNG) and passes consecutive slices; repeats are legal (a gather).
 *   obs_dev            (nullable, with obs_out_dev) the rollout's observations, addressed by strides in ELEMENTS: feature
 *                      f of step t, env e is element t * obs_s_t + e * obs_s_n + f * obs_s_f; obs_dim features of
 *                      obs_bytes (4 | 8) bytes.  [T][N][F] row-major, SB3_FLAT and SPLIT buffers: (N * F, F, 1);
 *                      [T][F][N] feature-major with plane pitch p (ptg_set_feature_pitch; p = N without): (F * p, 1, p).
 *   obs_out_dev        [B][obs_dim] row-major contiguous
 *   cols_host [n_cols] device pointers of up to 8 contiguous [T][N] arrays of col_bytes_host[c] (1 | 2 | 4 | 8) bytes per
 *                      element, copied as raw bytes: actions, values, log-probs, advantages, returns, done flags ...
 *   cols_out_host      device pointers of their outputs, [B] contiguous each
 * The three host arrays are read during the call; the kernel receives the pointers by value, so a captured call
 * holds no host memory.  Output row b is the source row (t, e) = (idx[b] % n_steps, idx[b] / n_steps), byte for byte
 * (no arithmetic touches the payload: NaN payloads, signed zeros and subnormals arrive as they are).
 * An index outside [0, n_steps * n_envs) is rejected before any address is formed from it: its output row and
 * column entries are left untouched, the other rows are gathered as usual, and the next ptg_sync (or any call that reports
 * kernel-flagged errors) returns PTG_E_INDEX once.  Outputs must not overlap inputs or each other: this is not checked.
 * Enqueues one kernel on `stream`: no host synchronisation, no allocation, so it may be captured into a hipGraph
 * and replayed with other contents in idx_dev.  Reads nothing of the handle but its n_envs and device: env state, the
 * finished-episode ring and the ptg_vn_* statistics are untouched.  Observations are optional (columns only is valid), and
 * so are columns.  PTG_E_INVALID (nothing enqueued): NULL handle, NULL idx_dev, idx_bytes other than 4 | 8, batch < 1,
 * n_steps < 1, obs_dev without obs_out_dev or the reverse, obs_dim < 1, obs_bytes other than 4 | 8 or a negative stride
 * with observations, n_cols outside [0, 8], a NULL column or column output (or NULL arrays with n_cols > 0), a column
 * element size other than 1 | 2 | 4 | 8, neither observations nor a column. */
#define PTG_MB_MAX_COLS 8
int ptg_minibatch(ptg_env* env, const void* idx_dev, int idx_bytes, int64_t batch, int n_steps,
                  const void* obs_dev, int64_t obs_s_t, int64_t obs_s_n, int64_t obs_s_f, int obs_dim, int obs_bytes, void* obs_out_dev,
                  int n_cols, const void* const* cols_host, const int* col_bytes_host, void* const* cols_out_host, void* stream);

/* ---- the same gather with its indices drawn on the device: a PPO / A2C gradient step that replays -------------------
 * ptg_minibatch needs a permutation in memory and a different slice of it per batch, so a captured gather replays only after the
 * host has rewritten its idx buffer.  ptg_minibatch_drawn takes no indices: row l of batch j of epoch c is
 *   idx[l] = perm_c(j * batch + l),      (c, j) = cursor_dev[0], cursor_dev[1] read on the device (the launch may be a replay),
 * where perm_c is a keyed bijection of [0, TN), TN = n_steps * n_envs, computed per row; no permutation exists in memory.  The value
 * is SB3's swap_and_flatten index i = e * n_steps + t, exactly as ptg_minibatch reads it, and from the index on the two calls are
 * one kernel: same strides, columns, byte-for-byte copy.  A trailing one-thread kernel advances the cursor in stream order, so one
 * captured graph of gather -> networks -> loss -> backward -> optimiser replays through every minibatch of every epoch.
 *
 * perm_c, in integer arithmetic only (tests/minibatch_drawn_restatement.py restates these lines in Python integers), with
 * h = lowbias32 and (w0, w1) the two words of ptg_replay_sample's keying above:
 *   n = max(2, bit_length(TN - 1));  a = n / 2 (the low half's bits);  b = n - a (the high half's);  mask_a = 2^a - 1, mask_b = 2^b - 1
 *   k_r = w0 of (seed, c, r) -- the chain above with the epoch c in the batch counter's place and the round r in the row's --
 *         for r = 0 .. R - 1, R = PTG_MB_PERM_ROUNDS = 6
 *   F(x): lo = x & mask_a; hi = (x >> a) & mask_b;
 *         for r = 0 .. R - 1:  r even: hi ^= h(lo ^ k_r) & mask_b;   r odd: lo ^= h(hi ^ k_r) & mask_a;
 *         F(x) = hi << a | lo                       (a Feistel network: every round is its own inverse, F a bijection of [0, 2^n))
 *   perm_c(i) = the first of F(i), F(F(i)), ... that is below TN        (cycle-walking: i itself lies on that cycle, so the walk
 *         ends and perm_c is a bijection of [0, TN); 2^n < 2 TN for TN > 2, so a walk is two applications on average; the longest
 *         seen on the host was 17, at TN = 4097 over 40 epochs.  Only a wave's 16 index lanes walk.)
 * R: the position-octile x value-octile counts over 400 epochs (a chi-square of 49 degrees of freedom, 99.9 % quantile 85.4;
 * tests/test_minibatch_drawn_host.py) read, in the mean of 16 seeds at TN = 1218, 2796 for R = 2, 50.4 for R = 4 (every one below
 * the bound), 43.0 for R = 6 and 43.4 for NumPy's own permutations: R = 4 passes the bound and is still told from uniform by this
 * statistic, R = 6 is not, so 6 it is: four more hashes on 16 lanes of a wave.
 * NOT a uniform draw from the TN! orders: 6 x 32 key bits per (seed, epoch) reach at most 2^192 of them, and at TN <= 6 whole
 * classes of orders are over- or under-represented whatever R is.  What is claimed, and tested, is a bijection whose
 * position-to-value statistics are indistinguishable from uniform at training sizes (TN = 203 and up).  SB3's NumPy stream is not
 * reproduced, as it was not by ptg_minibatch, which takes any permutation.
 *
 *   cursor_dev         uint64[2] on the device, zero at creation: {epochs finished, batches drawn in this epoch}.  Behind the gather:
 *                      j += 1; if (j >= TN / batch) { j = 0; epochs += 1; }.  Checkpoint and restore it as two integers.
 *   seed               with the epoch, the permutation's key
 *   idx_out_dev        (nullable) int64 [batch]: the indices used
 *   everything else    as in ptg_minibatch
 * A drawn index is below TN by construction.  A POSITION j * batch + l at or past TN -- a cursor restored past its epoch, or a
 * batch size changed in the middle of one -- is never walked (no cycle through it is known to return below TN): its row, column
 * entries and idx_out entry are left untouched and the next ptg_sync returns PTG_E_INDEX once; the cursor kernel then starts the
 * next epoch.
 * ptg_minibatch_end_epoch ends an epoch that was cut short (SB3's PPO leaves its epoch loop on target_kl): if (j != 0) { j = 0;
 * epochs += 1; } -- a fresh epoch is left alone -- as one one-thread kernel.
 * Both enqueue kernels only -- ptg_minibatch_drawn two, ptg_minibatch_end_epoch one: no host synchronisation, no allocation, no
 * host memory in the launch; env state, the finished-episode ring and the ptg_vn_* statistics are untouched.
 * PTG_E_INVALID (nothing enqueued): everything ptg_minibatch refuses but its indices; a NULL cursor_dev; n_steps * n_envs not a
 * multiple of batch (a ragged last batch cannot feed a graph of fixed shape and stays with ptg_minibatch; the reference's PPO has
 * n_steps = 21 * batch_size and A2C's batch is everything); n_steps * n_envs above PTG_MB_DRAWN_MAX_ROWS = 2^48, the bound up to
 * which the restatement and the kernel are checked (the arithmetic itself holds for any n <= 64). */
#define PTG_MB_PERM_ROUNDS 6
#define PTG_MB_DRAWN_MAX_ROWS ((uint64_t)1 << 48)
int ptg_minibatch_drawn(ptg_env* env, uint64_t* cursor_dev, uint64_t seed, int64_t* idx_out_dev, int64_t batch, int n_steps,
                        const void* obs_dev, int64_t obs_s_t, int64_t obs_s_n, int64_t obs_s_f, int obs_dim, int obs_bytes, void* obs_out_dev,
                        int n_cols, const void* const* cols_host, const int* col_bytes_host, void* const* cols_out_host, void* stream);
int ptg_minibatch_end_epoch(ptg_env* env, uint64_t* cursor_dev, void* stream);

/* ---- the replay buffer of the off-policy algorithms on the device ---------------------------------------------------
 * Replaces: stable_baselines3.common.buffers.ReplayBuffer / DictReplayBuffer .add, .sample and ._get_samples (SB3 2.0.0a13,
 * optimize_memory_usage off), from which the reference's DQN, TD3, SAC and TQC train (src/rl_config_agent.py:80-222; buffers of
 * 1 M - 20 M transitions, train_freq 1 - 9): every env step is followed by an add and, shortly after, by a sample.  With these two
 * calls collect -> store -> sample stays on the GPU and can be captured in a hipGraph behind ptg_step / ptg_rollout.
 * Storage is the caller's (the library allocates nothing) and is described by a ptg_replay, read during the call:
 *   capacity           S = max(buffer_size / n_envs, 1) rows of n_envs transitions (SB3's rule)
 *   obs_ring, next_ring  [S][N][obs_dim] row-major contiguous, obs_bytes (4 | 8) per element: observations, next observations
 *   col_ring[c]        n_cols <= PTG_MB_MAX_COLS contiguous [S][N] arrays of col_bytes[c] (1 | 2 | 4 | 8) bytes per element:
 *                      actions, rewards, dones ...
 *   cursor_dev         uint64[2] on the device, zero at creation: {vector steps added since creation, batches drawn on the device
 *                      so far}.  It lives on the device so that captured launches can be replayed, as the hot kernels take the
 *                      step count from device state.  pos = cursor[0] % S, full = cursor[0] >= S, size = min(cursor[0], S).
 * Transition (slot s, env e) has the flat index i = s * N + e, 0 <= i < size * N: it is the row number in every ring.
 *
 * ptg_replay_add stores a window of T = n_steps vector steps as ptg_step (T = 1) or ptg_rollout left them.  With a = cursor[0]
 * read on the device, step t goes to slot (a + t) % S (a window may wrap; n_steps <= S, so its slots are distinct):
 *   obs_ring slot      t == 0 ? prev_obs[e] : obs[t - 1][e]; prev_obs_dev [N][obs_dim] is the observation the first action was
 *                      chosen from, addressed with obs_s_n, obs_s_f
 *   next_ring slot     obs[t][e], or final_obs[t][e] where done[t][e] != 0 and final_obs_dev (nullable; the strides of obs_dev) is
 *                      given: OffPolicyAlgorithm._store_transition's infos[e]["terminal_observation"].  Without final_obs_dev a
 *                      finished row keeps the post-reset observation; no SB3 off-policy target reads it there: every target
 *                      multiplies the next value by (1 - done), and the reference never truncates (env/ptg_gym_env.py:478-481),
 *                      so `timeouts` is identically 0 and is not stored.
 *   col_ring[c] slot   cols_host[c][t][e] (contiguous [T][N] device arrays), byte for byte; column done_col (-1: none) is instead
 *                      written as float32 0.0f / 1.0f from done_dev (uint8 [T][N]): SB3's dtype, so sampling is a pure copy.
 *                      cols_host[done_col] is not read.
 * Observations are addressed through element strides exactly as in ptg_minibatch: row-major / SB3_FLAT / SPLIT (N * F, F, 1),
 * feature-major with pitch p (F * p, 1, p).  A trailing one-thread kernel does cursor[0] += T in stream order.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, ring, cursor, prev_obs_dev, obs_dev or column; capacity < 1;
 * n_steps < 1 or > capacity; obs_dim outside [1, 2^20]; obs_bytes other than 4 | 8; a negative stride; n_cols other than the
 * descriptor's or outside [0, 8]; a column element size other than 1 | 2 | 4 | 8; done_col outside [-1, n_cols) or naming a
 * column that is not 4 bytes; done_dev NULL with final_obs_dev or a done column.
 *
 * ptg_replay_sample gathers `batch` transitions: [batch][obs_dim] rows of obs_ring into obs_out_dev and of next_ring into
 * next_obs_out_dev, [batch] entries of column c into cols_out_host[c] (raw bytes), the indices used into idx_out_dev (int64
 * [batch]).  Every output is nullable (cols_out_host itself too), but at least one is required.
 *   idx_dev            int64 [batch] flat indices supplied by the caller (repeats are legal), or NULL: the kernel draws them.
 *                      Row b of the c-th drawn batch (c = cursor[1]) takes, with h = lowbias32 (x ^= x >> 16; x *= 0x7feb352d;
 *                      x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16) and lo / hi the 32-bit halves, all arithmetic modulo 2^32:
 *                        k = h(lo(seed) ^ 0x9E3779B9); k = h(k + hi(seed)); k = h(k ^ lo(c)); k = h(k + hi(c));
 *                        k = h(k ^ lo(b)); k = h(k + hi(b)); w0 = h(k ^ 0x85EBCA6B); w1 = h(k ^ 0xC2B2AE35);
 *                        i = floor(((w0 << 32) | w1) * (size * N) / 2^64)        (__umul64hi; bias at most size * N / 2^64)
 *                      and a trailing one-thread kernel does cursor[1] += 1, so a replayed graph draws a fresh batch.
 *   norm_col           >= 0: the reward column; its output is what ptg_vn_apply(training = 0) writes for the same raw values with the
 *                      statistics the handle holds when the kernel runs -- (OUT)clip((double)r / sqrt(var + epsilon)), the same
 *                      expression, operand types and rounding: SB3's _normalize_reward (rewards are stored raw and normalised at
 *                      sample time with the current variance).  Its element size must match the handle's out_dtype, ptg_vn_init must
 *                      have been called and the column must have an output.  -1: raw bytes.
 * size = min(cursor[0], S) is read on the device.  An explicit index outside [0, size * N) (a negative one included), or any draw
 * from an empty buffer, never becomes an address: the row, its column entries and its idx_out entry are left untouched, the other
 * rows are gathered as usual, and the next ptg_sync returns PTG_E_INDEX once.  Outputs must not overlap the rings or each other.
 * Both calls enqueue kernels only (no host synchronisation, no allocation), so both may be captured into a hipGraph and replayed;
 * neither touches env state, the finished-episode ring or the ptg_vn_* statistics.
 * PTG_E_INVALID (nothing enqueued): the descriptor's faults above; batch < 1; no output at all; norm_col outside [-1, n_cols),
 * before ptg_vn_init, on a column of another element size than out_dtype, or without an output. */
typedef struct ptg_replay {
    int64_t capacity;
    int32_t obs_dim, obs_bytes;
    void* obs_ring;
    void* next_ring;
    int32_t n_cols;
    int32_t col_bytes[PTG_MB_MAX_COLS];
    void* col_ring[PTG_MB_MAX_COLS];
    uint64_t* cursor_dev;
} ptg_replay;
int ptg_replay_add(ptg_env* env, const ptg_replay* rb, const void* prev_obs_dev, const void* obs_dev, int64_t obs_s_t, int64_t obs_s_n,
                   int64_t obs_s_f, const void* final_obs_dev, const uint8_t* done_dev, int done_col, int n_cols, const void* const* cols_host,
                   int64_t n_steps, void* stream);
int ptg_replay_sample(ptg_env* env, const ptg_replay* rb, const int64_t* idx_dev, int64_t batch, uint64_t seed, void* obs_out_dev,
                      void* next_obs_out_dev, void* const* cols_out_host, int norm_col, int64_t* idx_out_dev, void* stream);

/* ---- the rollout buffer of the on-policy algorithms on the device ----------------------------------------------------
 * Replaces: stable_baselines3.common.buffers.RolloutBuffer.reset / add (SB3 2.0.0a13), into which the reference's PPO (its default,
 * rl_alg : PPO) and A2C collect: every action is chosen from the observation before it, so the collect step is network -> ptg_act ->
 * ptg_step, captured into a hipGraph once and replayed.  A replayed graph has fixed addresses; with these two calls the step's results
 * go to the next row all the same, because the row number lives on the device.  ptg_gae and ptg_minibatch read what they leave.
 * Storage is the caller's (the library allocates nothing) and is described by a ptg_rollout_buffer, read during the call:
 *   n_steps            T >= 1 steps per window
 *   obs_rows           T + 1 observation blocks of obs_dim features, obs_bytes (4 | 8) per element, each laid out exactly like the
 *                      block ptg_step writes (below), row r starting r * row_pitch elements behind row 0
 *   col_rows[c]        n_cols <= PTG_MB_MAX_COLS contiguous [T][N] arrays of col_bytes[c] (1 | 2 | 4 | 8) bytes per element: rewards,
 *                      done flags (uint8, ptg_step's own array, which ptg_gae takes), actions, values, log-probs ...  No column has a
 *                      meaning to the kernel.
 *   cursor_dev         uint64[2] on the device: {rows added in this window, completion ticket}.  The second word is reserved: begin zeroes it,
 *                      add leaves it (a one-launch measurement build counts its workgroups in it).
 * Row layout.  Row 0 holds the observation the window's first action is chosen from.  After the window obs_rows[0 .. T) are SB3's
 * `observations` (what ptg_minibatch gathers from) and obs_rows[T] is `new_obs` (what last_values is computed from and what the next
 * window begins with); SB3's episode_starts[t + 1] is the done column's row t.  No copy of the previous observation is kept anywhere.
 *   ptg_rollout_buffer_begin(env, rb, obs_dev, obs_s_n, obs_s_f, row_pitch, stream)
 *                      copies the block obs_dev into row 0 and sets both cursor words to 0 (RolloutBuffer.reset).
 *   ptg_rollout_buffer_add(env, rb, obs_dev, obs_s_n, obs_s_f, row_pitch, n_cols, cols_host, col_stride_host, stream)
 *                      with t = cursor[0] read on the device: obs_dev, the block ptg_step just wrote, goes to row t + 1; entry e of
 *                      column source c goes to col_rows[c][t][e], byte for byte, read at cols_host[c] + e * col_stride_host[c]
 *                      elements (stride >= 1: the value column out[:, A] of a joint network output is read in place); then
 *                      cursor[0] = t + 1.  cols_host / col_stride_host [n_cols] are host arrays of device pointers / element strides.
 * No transposing.  Feature f of env e is element e * obs_s_n + f * obs_s_f of the source block AND of the buffer row: a row has the
 * source's layout.  Row-major, SB3_FLAT and SPLIT blocks, (obs_s_n, obs_s_f) = (F, 1), and feature-major blocks without a pitch,
 * (1, N), are one contiguous run of N * F elements, row_pitch = N * F; a feature-major block with plane pitch p (ptg_set_feature_pitch),
 * (1, p), is F runs of N elements, row_pitch = F * p, and the p - N pad elements of a plane are neither read nor written.
 * ptg_minibatch reads both forms with obs_s_t = row_pitch.  Elements move as 16-byte pieces when the block is one contiguous run of a
 * whole number of them and obs_dev, obs_rows and row_pitch * obs_bytes are multiples of 16, else one by one.
 * Full buffer.  ptg_rollout_buffer_add with t >= n_steps never forms an address: nothing is written, the cursor stays, and the next
 * ptg_sync (or any call that reports kernel-flagged errors) returns PTG_E_INDEX once (SB3 raises IndexError in the same place).
 * Cursor.  Every workgroup of add's copy kernel reads cursor[0] before anything else; a trailing one-thread kernel advances it in
 * stream order (or flags the full buffer), as ptg_replay_add does.  A one-launch form -- the workgroup that draws the last of one
 * ticket per workgroup on cursor[1] advances the cursor -- was measured beside it inside a captured collect step and is not in the
 * library.  There is no spin-wait, no cooperative launch and no atomic; the stored bytes do not depend on the grid.
 * Both calls enqueue kernels only (begin one, add two): no host synchronisation, no allocation, pointers by value in the launch, so a captured add holds
 * no host memory and every replay stores at the next row.  Neither touches env state, the finished-episode ring or the ptg_vn_*
 * statistics.  Overlap of the sources with the buffer, of buffer rows with each other (a row_pitch below a block's extent) and of the
 * columns is NOT checked.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, obs_rows, cursor, obs_dev or column (of the descriptor or of cols_host,
 * or NULL arrays with n_cols > 0); n_steps < 1; obs_dim outside [1, 2^20]; obs_bytes other than 4 | 8; a negative stride or pitch;
 * n_cols other than the descriptor's or outside [0, 8]; a column element size other than 1 | 2 | 4 | 8; a column stride < 1. */
typedef struct ptg_rollout_buffer {
    int64_t n_steps;
    int32_t obs_dim, obs_bytes;
    void* obs_rows;
    int32_t n_cols;
    int32_t col_bytes[PTG_MB_MAX_COLS];
    void* col_rows[PTG_MB_MAX_COLS];
    uint64_t* cursor_dev;
} ptg_rollout_buffer;
int ptg_rollout_buffer_begin(ptg_env* env, const ptg_rollout_buffer* rb, const void* obs_dev, int64_t obs_s_n, int64_t obs_s_f,
                             int64_t row_pitch, void* stream);
int ptg_rollout_buffer_add(ptg_env* env, const ptg_rollout_buffer* rb, const void* obs_dev, int64_t obs_s_n, int64_t obs_s_f, int64_t row_pitch,
                           int n_cols, const void* const* cols_host, const int64_t* col_stride_host, void* stream);

/* ---- the action head: policy outputs to actions, log-probs and entropy in one launch --------------------------------
 * Replaces what the reference's algorithms (src/rl_config_agent.py:80-222) run between the network's output and env.step while
 * collecting (SB3 2.0.0a13 common/distributions.py, dqn/policies.py, common/off_policy_algorithm.py):
 *   PTG_HEAD_CATEGORICAL  A2C / PPO, action_type "discrete": CategoricalDistribution.sample / log_prob / entropy of the logits
 *   PTG_HEAD_EPS_GREEDY   DQN: a uniform random action with probability epsilon (_sample_action), else argmax of the Q-values
 *   PTG_HEAD_GAUSSIAN     TD3 clip(mu + N(0, sigma_exp), -1, 1); SAC / TQC tanh(mu + sigma z) (PTG_HEAD_SQUASH); A2C / PPO with
 *                         action_type "continuous": DiagGaussianDistribution, clipped to the Box for the env and stored unclipped
 * -- six to ten element-wise launches in torch.  The env's Box is one-dimensional, so the Gaussian head has D = 1: one mean and one
 * action per env.  Out of scope: the networks (evaluate_actions at training time is ptg_policy_loss, below).  gSDE (use_sde) has ops of its own: ptg_sde_resample / ptg_sde_act, behind ptg_policy_loss.
 * The head is described by a ptg_head, read during the call:
 *   kind          PTG_HEAD_CATEGORICAL | PTG_HEAD_EPS_GREEDY | PTG_HEAD_GAUSSIAN
 *   flags         PTG_HEAD_DETERMINISTIC: the mode; nothing is drawn, counter_dev is neither read nor advanced (and may be NULL).
 *                 PTG_HEAD_SQUASH (Gaussian only): tanh
 *   in_dtype      PTG_OUT_F32 | PTG_OUT_F64: the element type of in_dev, of the Gaussian param_dev and of raw / logp / ent
 *   in_dev        discrete kinds: [N][A] logits or Q-values, element (e, j) at e * in_s_n + j, in_s_n >= A = n_actions, 2 <= A <= 32
 *                 (a stride above A reads a slice of a wider [N, A + 1] actor-critic output).  Gaussian: the means [N], element
 *                 e at e * in_s_n, in_s_n >= 1 (n_actions is not read)
 *   param_dev     on the device, so that a replayed graph sees an update.  EPS_GREEDY: epsilon, float64 [1] (not read and
 *                 nullable when deterministic).  GAUSSIAN: log_std in in_dtype, element e at e * param_s_n with param_s_n 0 (one
 *                 value: SB3's state-independent parameter, or log(sigma_exp) for TD3) or 1 (per env: SAC's actor).
 *   clip_lo, clip_hi   Gaussian: bounds of the env action (host doubles)
 *   seed, counter_dev  the draw: counter_dev is the caller's uint64 [1] on the device.  Row e of the c-th call (c = *counter_dev
 *                 read on the device) takes the words (w0, w1) of ptg_replay_sample's chain above with the key
 *                 (seed, c, global env offset + e) in place of (seed, c, b): a shard draws what its slice of one big batch would
 *                 draw (ptg_set_global_env_offset).  A trailing one-thread kernel does *counter_dev += 1 in stream order, unless
 *                 the call is deterministic: a replayed graph draws afresh.
 *   act_dev       [N] of act_kind: PTG_ACT_I32 | PTG_ACT_I64 for the discrete kinds, PTG_ACT_F32 for Gaussian -- what ptg_step takes
 *   raw_dev       [N] in_dtype, nullable, Gaussian only: the unclipped, unsquashed sample (what an on-policy buffer stores)
 *   logp_dev, ent_dev  [N] in_dtype, nullable: log-probability of the action taken, entropy of the row's distribution
 * Arithmetic: all of it in float64 whatever in_dtype is, every operation rounded once (no fused multiply-add), results rounded
 * once on the store.  l_j = (double)in[e][j]; exp, log, sqrt, cos, tanh are the double-precision library functions.
 *   categorical   m = max_j l_j;  e_j = exp(l_j - m);  s = e_0 + e_1 + ... in index order;  logp_j = (l_j - m) - log(s)
 *                 entropy = -(t_0 + t_1 + ...), t_j = (e_j / s) * logp_j in index order, terms with e_j == 0 left out
 *                 draw: u = ((w0 << 21) | (w1 >> 11)) * 2^-53;  action = the first j with u * s < e_0 + ... + e_j (the partial
 *                 sums of s), or A - 1 if there is none;  mode: the first j with l_j == m.  logp = logp_action
 *   eps-greedy    integers only: t = (uint64)(eps * 2^32);  explore iff w0 < t (eps = 1: always; eps = 0: never);
 *                 exploring: action = (w1 * A) >> 32 (64-bit product), else the first j with l_j == m.  Deterministic: the latter
 *   Gaussian      u1 = (w0 + 1) * 2^-32;  u2 = w1 * 2^-32;  z = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2), so |z| <=
 *                 sqrt(64 ln 2) = 6.66;  deterministic: z = 0.   g = mu + exp(log_std) * z;  raw = g
 *                 plain: action = clip(g, lo, hi);  logp = ((-(z * z) / 2) - log_std) - 0.9189385332046727 (= 1/2 log 2 pi);
 *                 entropy = 1.4189385332046727 + log_std
 *                 squashed: a = tanh(g);  action = clip(a, lo, hi);  logp = plain logp - log((1 - a * a) + 1e-6) (SB3's epsilon);
 *                 no entropy.   clip(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x), then rounded to float32
 * Bad rows: a discrete row whose maximum is not finite (a NaN or +Inf entry, or every entry -Inf), a Gaussian row whose mean is
 * not finite or whose log_std is NaN or +Inf, and every row of a stochastic eps-greedy call whose epsilon is NaN or outside [0, 1]
 * get action 0 and NaN in raw / logp / ent; the other rows are computed as usual, and the next ptg_sync (or any call that
 * reports kernel-flagged errors) returns PTG_E_NONFINITE once.  A -Inf logit beside a finite one is legal: probability 0.
 * Enqueues kernels only (one, plus the counter kernel): no host synchronisation, no allocation, so it may be captured into a
 * hipGraph and replayed.  Reads nothing of the handle but its n_envs, device and global env offset: env state, the
 * finished-episode ring, the ptg_vn_* statistics and every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, head, in_dev or act_dev; NULL counter_dev unless deterministic; an unknown kind
 * or flag; PTG_HEAD_SQUASH on a discrete kind; n_actions outside [2, 32] or in_s_n < n_actions (discrete), in_s_n < 1
 * (Gaussian); an in_dtype other than the two; an act_kind that is not the kind's; a missing param_dev; param_s_n other than
 * 0 | 1 (Gaussian); clip_lo > clip_hi or a NaN bound (Gaussian); raw_dev on a discrete kind; logp_dev or ent_dev on eps-greedy;
 * ent_dev on a squashed head. */
enum { PTG_HEAD_CATEGORICAL = 0, PTG_HEAD_EPS_GREEDY = 1, PTG_HEAD_GAUSSIAN = 2 };
enum { PTG_HEAD_DETERMINISTIC = 1, PTG_HEAD_SQUASH = 2 };
typedef struct ptg_head {
    int32_t kind, flags;
    int32_t n_actions, in_dtype;
    const void* in_dev;
    int64_t in_s_n;
    const void* param_dev;
    int32_t param_s_n, act_kind;
    double clip_lo, clip_hi;
    uint64_t seed;
    uint64_t* counter_dev;
    void* act_dev;
    void* raw_dev;
    void* logp_dev;
    void* ent_dev;
} ptg_head;
int ptg_act(ptg_env* env, const ptg_head* head, void* stream);

/* ---- the policy loss: PPO / A2C loss, SB3's logged statistics and the gradients w.r.t. the network's outputs in one pass ------
 * Replaces what the reference's A2C and PPO (src/rl_config_agent.py:80-222) run on every minibatch between the network's output
 * and the gradient that goes back into the network (SB3 2.0.0a13): ActorCriticPolicy.evaluate_actions' Categorical / DiagGaussian
 * log_prob and entropy, the loss lines of PPO.train (ppo/ppo.py) / A2C.train (a2c/a2c.py) -- advantage normalisation; ratio,
 * clamp and min; value clipping and MSE; the entropy term; approx_kl and clip_fraction -- and autograd's walk back over the same
 * graph: some forty element-wise launches forward and as many backward.  Every gradient of these losses with respect to the
 * network's outputs is a closed form of quantities the forward pass holds, so one pass emits the loss, the statistics SB3 logs,
 * d loss / d logits (or means), d loss / d values and d loss / d log_std; the caller's backward starts from those
 * (rl_ptg_amd/loss.py wraps the call in a torch.autograd.Function).  Out of scope: the networks, target_kl's early stop (the
 * caller reads stats[4]), the squashed and off-policy losses, a per-env log_std.  The gSDE head's loss is ptg_sde_policy_loss, below.  The optimiser and max_grad_norm follow the
 * backward pass as ptg_optim_step, below.
 * The call is described by a ptg_loss, read during the call (B = batch, A = n_actions):
 *   kind          PTG_LOSS_PPO | PTG_LOSS_A2C
 *   head          PTG_HEAD_CATEGORICAL | PTG_HEAD_GAUSSIAN (unsquashed, D = 1, as in ptg_act)
 *   flags         PTG_LOSS_NORM_ADV: normalise the advantages over the batch.  PTG_LOSS_CLIP_VF: clip the value step
 *   batch         B >= 1, a 64-bit count that is not tied to the handle's n_envs (A2C's one batch is all T * N rows)
 *   in_dtype      PTG_OUT_F32 | PTG_OUT_F64: the element type of EVERY float input and of every gradient
 *   in_dev        categorical: logits [B][A], element (i, j) at i * in_s_n + j, in_s_n >= A, 2 <= A <= 32.  Gaussian: the means [B],
 *                 element i at i * in_s_n, in_s_n >= 1 (n_actions is not read)
 *   val_dev       values [B], element i at i * val_s_n, val_s_n >= 1: a column of an [B][A + 1] actor-critic output is read in place
 *   act_dev       [B] contiguous.  Categorical: the chosen actions, act_kind PTG_ACT_I32 | PTG_ACT_I64.  Gaussian: the stored raw
 *                 (unclipped) samples in in_dtype; act_kind is not read
 *   old_logp_dev, adv_dev, ret_dev   [B] contiguous in in_dtype, what ptg_minibatch gathers (old_logp_dev: PPO only; A2C neither
 *                 needs nor reads it)
 *   old_val_dev   [B] contiguous, required iff PTG_LOSS_CLIP_VF
 *   log_std_dev   Gaussian only: one value in in_dtype on the device (SB3's state-independent log_std), so that a replayed graph
 *                 sees the optimiser's update
 *   clip_range, clip_range_vf, ent_coef, vf_coef   host doubles eps, eps_v, c_e, c_v; a captured call keeps them.  clip_range is
 *                 read by PPO only, clip_range_vf with PTG_LOSS_CLIP_VF only
 *   stats_dev     float64 [8] = {loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv mean, adv std}; the last
 *                 two are the moments actually used, 0 and 1 when the advantages are not normalised
 *   grad_in_dev   d loss / d in_dev in in_dtype with the shape rules of in_dev and the row stride g_s_n
 *   grad_val_dev  d loss / d values, element i at i * gv_s_n.  With g_s_n = gv_s_n = A + 1 the two fill one [B][A + 1] tensor
 *   grad_log_std_dev   [1] in in_dtype, Gaussian only, nullable
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_policy_loss_workspace(batch) bytes; its contents
 *                 mean nothing before or after the call
 * Arithmetic: all of it in float64 whatever in_dtype is, every operation rounded once (no fused multiply-add), gradients rounded
 * once on the store; exp, log, sqrt are the double-precision library functions.  Row i, l_j = (double)in[i][j], a = its action:
 *   categorical   m, e_j, s, logp_j and the entropy H exactly as ptg_act states them;  p_j = e_j / s;  lp = logp_a
 *   Gaussian      sigma = exp(ls);  z = (a - mu) / sigma;  lp = ((-(z * z) / 2) - ls) - 0.9189385332046727;  H = 1.4189385332046727 + ls
 *   advantages    PTG_LOSS_NORM_ADV and B > 1: Ah = (adv - mean) / (std + 1e-8), std = sqrt(M2 / (B - 1)) (torch.std's unbiased one),
 *                 (count, mean, M2) merged over the batch with Chan's formula;  otherwise (SB3 skips a batch of one) Ah = adv.
 *                 Advantages are data: nothing is differentiated through them or their moments
 *   PPO           d = lp - old;  r = exp(d);  c = r < 1 - eps ? 1 - eps : (r > 1 + eps ? 1 + eps : r);  t1 = Ah * r;  t2 = Ah * c;
 *                 surrogate = t2 < t1 ? t2 : t1;  g = t1 if t1 < t2 or 1 - eps <= r <= 1 + eps, else 0 (torch.minimum's and
 *                 clamp's tie rules: on a tie each branch carries half, and an unclipped ratio is always a tie);
 *                 kl = (r - 1) - d;  cf = |r - 1| > eps ? 1 : 0
 *   A2C           surrogate = Ah * lp;  g = Ah;  kl = cf = 0
 *   value         without PTG_LOSS_CLIP_VF vh = v and pass = 1; with it dv = v - old_v, vh = old_v + clamp(dv, -eps_v, eps_v),
 *                 pass = -eps_v <= dv <= eps_v;   dq = ret - vh;  q = dq * dq;  h = pass ? 2 * (vh - ret) : 0
 *   means         policy_loss = -(sum surrogate / B);  value_loss = sum q / B;  entropy_loss = -(sum H / B);  approx_kl = sum kl / B;
 *                 clip_fraction = sum cf / B;  loss = (policy_loss + c_e * entropy_loss) + c_v * value_loss
 *   gradients     d loss / d l_j = ((-g) * ([j == a] - p_j) + c_e * (p_j * (logp_j + H))) / B, the c_e term left out where e_j == 0 (as
 *                 H leaves that column out): a column of probability 0 that was not chosen gets 0
 *                 d loss / d v = (c_v * h) / B;   Gaussian: d loss / d mu = ((-g) * (z / sigma)) / B,
 *                 d loss / d log_std = (-(sum g * ((z * z) - 1)) / B) - c_e
 * Sums run in a fixed order that depends on B alone (per wave a shuffle tree, the waves of a 256-row block in order, the blocks'
 * partials in ws_dev, a last pass over the partials; no floating-point atomics): the same inputs give the same bits on every run.
 * Known difference from SB3: it normalises float32 advantages in float32; here the moments and Ah are float64.
 * Bad rows.  No index ever becomes an address: a categorical action outside [0, A) leaves the row's gradients untouched and the
 * next ptg_sync (or any call that reports kernel-flagged errors) returns PTG_E_INDEX once.  A row whose logit maximum is not finite
 * (a NaN or +Inf entry, or every entry -Inf), a non-finite value, advantage, return, old log-prob (PPO), old value (with
 * PTG_LOSS_CLIP_VF) or mean, a NaN or +Inf log_std, an action whose log-probability is not finite (a -Inf logit, a zero sigma, a
 * non-finite sample), and a PPO row whose ratio r = exp(lp - old) is not finite (it overflows: Ah * r would be Inf, or NaN where Ah
 * is 0) gets NaN gradients and the next ptg_sync returns PTG_E_NONFINITE once.  Either kind of row makes stats[0..5]
 * (and the log_std gradient) NaN; the other rows' gradients are computed as usual -- except that a non-finite advantage under
 * PTG_LOSS_NORM_ADV makes the moments, and with them every row, NaN, as the arithmetic says.  A -Inf logit on a column that was
 * not chosen is legal: probability 0.
 * Enqueues kernels only -- one for B <= 256 (PPO's minibatch of 203); else rows + final merge, and two more in front for the
 * moments under PTG_LOSS_NORM_ADV -- with no host synchronisation and no allocation, so it may be captured into a hipGraph and
 * replayed.  Reads nothing of the handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and every
 * replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, in_dev, val_dev, act_dev, adv_dev, ret_dev, stats_dev, grad_in_dev,
 * grad_val_dev or ws_dev (or a ws_dev that is not 8-byte aligned); NULL old_logp_dev for PPO; an unknown kind, head or flag; batch < 1
 * (or above 2^31: the row kernel's grid stays at half of the 2^32 threads one launch may have; the largest batch run is 20 x 65 536); n_actions outside [2, 32] (categorical); in_s_n or g_s_n below n_actions (Gaussian: below 1), val_s_n or gv_s_n
 * below 1; an in_dtype other than the two; an act_kind other than PTG_ACT_I32 | PTG_ACT_I64 (categorical); PTG_LOSS_CLIP_VF without
 * old_val_dev; the Gaussian head without log_std_dev; grad_log_std_dev on the categorical head; a NaN or negative clip_range (PPO)
 * or clip_range_vf (with PTG_LOSS_CLIP_VF).
 * ptg_policy_loss_workspace(batch): bytes of scratch a batch of that size needs (88 per 256 rows + 32); negative for batch < 1 or above 2^31. */
enum { PTG_LOSS_PPO = 0, PTG_LOSS_A2C = 1 };
enum { PTG_LOSS_NORM_ADV = 1, PTG_LOSS_CLIP_VF = 2 };
typedef struct ptg_loss {
    int32_t kind, head;
    int32_t flags, n_actions;
    int32_t in_dtype, act_kind;
    int64_t batch;
    const void* in_dev;
    int64_t in_s_n;
    const void* val_dev;
    int64_t val_s_n;
    const void* act_dev;
    const void* old_logp_dev;
    const void* adv_dev;
    const void* ret_dev;
    const void* old_val_dev;
    const void* log_std_dev;
    double clip_range, clip_range_vf, ent_coef, vf_coef;
    double* stats_dev;
    void* grad_in_dev;
    int64_t g_s_n;
    void* grad_val_dev;
    int64_t gv_s_n;
    void* grad_log_std_dev;
    void* ws_dev;
} ptg_loss;
int64_t ptg_policy_loss_workspace(int64_t batch);
int ptg_policy_loss(ptg_env* env, const ptg_loss* d, void* stream);

/* ---- gSDE: the state-dependent exploration head while collecting, and its PPO / A2C loss ------------------------------------
 * Replaces what SB3 2.0.0a13 runs for the reference's agent switch `gSDE : True` (config/config_agent.yaml; src/rl_config_agent.py
 * passes it as use_sde) in A2C and PPO: common/distributions.py::StateDependentNoiseDistribution with its on-policy defaults
 * full_std=True, use_expln=False, squash_output=False, learn_features=False, epsilon = 1e-6 -- sample_weights, proba_distribution,
 * sample, log_prob, entropy, mode -- and evaluate_actions plus the loss lines of PPO.train / A2C.train on that distribution: about a
 * dozen element-wise launches, an mm and a bmm per collect step in torch.  The env's Box is one-dimensional, so D = 1: log_std is
 * [L, 1], an exploration matrix is one [L] row per env.  L = latent_dim is the width of the policy's last hidden layer,
 * 1 <= L <= PTG_MLP_MAX_WIDTH (1024); the latent rows are what a PTG_MLP_KEEP_HIDDEN forward leaves in its workspace, whose rows are
 * padded to 16 bytes, so every [.][L] array here has a row stride >= L.
 * Out of scope: use_expln; full_std=False; D > 1; fusing the head into the network's last layer.  sde_sample_freq is the caller's
 * schedule of ptg_sde_resample.  SAC / TQC with gSDE (squashing, clip_mean, learn_features=True, reset_noise per gradient step) has
 * ops of its own: ptg_sde_resample_rows / ptg_sde_rsample / ptg_sde_rsample_backward, behind ptg_sde_policy_loss.
 * Arithmetic, all three ops: float64 whatever in_dtype is, every operation rounded once (no fused multiply-add), results rounded once
 * on the store; exp, log, sqrt, cos are the double-precision library functions.  s_k = exp((double)log_std[k]); h_k a latent entry.
 * Sums over k run in an order given by L alone: unit k belongs to lane k mod 64, a lane adds its terms ascending in k from 0.0, the 64
 * lane sums meet in ptg_policy_loss's shuffle tree (offsets 32, 16, ..., 1).
 *
 * ptg_sde_resample (sample_weights) fills the exploration matrix E_dev [N][L] in in_dtype, element (e, k) at e * e_s_n + k, N the
 * handle's n_envs.  With c = *counter_dev (uint64 [1], read on the device), element (e, k) takes the words (w0, w1) of
 * ptg_replay_sample's chain with the key (seed, c, (global env offset + e) * 1024 + k) -- the key depends neither on L nor on the
 * shard -- z is ptg_act's Gaussian draw from (w0, w1), and E[e][k] = s_k * z.  log_std_dev is [L] contiguous in in_dtype, read when
 * the kernel runs.  A trailing one-thread kernel does *counter_dev += 1, so a replayed graph draws afresh.  A NaN or +Inf log_std[k]
 * makes column k NaN and the next ptg_sync returns PTG_E_NONFINITE once.  Two launches.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, log_std_dev, counter_dev or e_dev; an in_dtype other than the two;
 * latent_dim outside [1, 1024]; e_s_n < latent_dim. */
typedef struct ptg_sde_noise {
    int32_t in_dtype, latent_dim;
    const void* log_std_dev;
    uint64_t seed;
    uint64_t* counter_dev;
    void* e_dev;
    int64_t e_s_n;
} ptg_sde_noise;
int ptg_sde_resample(ptg_env* env, const ptg_sde_noise* d, void* stream);

/* ptg_sde_act (proba_distribution, sample / mode, log_prob, entropy) is the collecting head, one launch:
 *   flags         PTG_HEAD_DETERMINISTIC: the mode; noise = 0, e_dev is neither read nor required
 *   mean_dev      [N] in in_dtype, element e at e * mean_s_n, mean_s_n >= 1
 *   latent_dev    [N][L], element (e, k) at e * latent_s_n + k, latent_s_n >= L;  e_dev likewise with e_s_n;  log_std_dev [L] contiguous
 *   act_dev       [N] float32 (act_kind PTG_ACT_F32): what ptg_step takes;  raw_dev, logp_dev, ent_dev [N] in in_dtype, nullable
 * Per env:  noise = sum_k h_k * E_k;  V = (sum_k (h_k * h_k) * (s_k * s_k)) + 1e-6;  sd = sqrt(V);  lsd = log(sd);  g = mu + noise;
 * raw = g;  action = clip(g, clip_lo, clip_hi) rounded to float32 (ptg_act's clip);  logp = ((-(noise * noise)) / (2 * V)) - lsd -
 * 0.9189385332046727;  entropy = 1.4189385332046727 + lsd.
 * Bad rows: a row whose mean or any latent entry is not finite, and every row when any log_std is NaN or +Inf, gets action 0 and NaN
 * in raw / logp / ent; the other rows are computed as usual and the next ptg_sync returns PTG_E_NONFINITE once.
 * Reads nothing of the handle but its n_envs and device.  Enqueues one kernel: no host synchronisation, no allocation.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, mean_dev, latent_dev, log_std_dev or act_dev; NULL e_dev unless
 * deterministic; an unknown flag; an in_dtype other than the two; latent_dim outside [1, 1024]; an act_kind other than PTG_ACT_F32;
 * mean_s_n < 1; latent_s_n < latent_dim; e_s_n < latent_dim (unless deterministic); clip_lo > clip_hi or a NaN bound. */
typedef struct ptg_sde_head {
    int32_t flags, in_dtype;
    int32_t latent_dim, act_kind;
    const void* mean_dev;
    int64_t mean_s_n;
    const void* latent_dev;
    int64_t latent_s_n;
    const void* e_dev;
    int64_t e_s_n;
    const void* log_std_dev;
    double clip_lo, clip_hi;
    void* act_dev;
    void* raw_dev;
    void* logp_dev;
    void* ent_dev;
} ptg_sde_head;
int ptg_sde_act(ptg_env* env, const ptg_sde_head* d, void* stream);

/* ptg_sde_policy_loss is ptg_policy_loss for this head.  kind, flags, batch, in_dtype, val_dev / val_s_n, old_logp_dev, adv_dev,
 * ret_dev, old_val_dev, the four host doubles, stats_dev [8], grad_in_dev / g_s_n (d loss / d means), grad_val_dev / gv_s_n mean
 * exactly what they mean in ptg_loss, and the advantage, PPO / A2C, value and "means" lines are ptg_policy_loss's (one device text
 * serves both).  mean_dev / mean_s_n are ptg_loss's Gaussian in_dev / in_s_n.  New:
 *   latent_dev    [B][L], element (i, k) at i * latent_s_n + k, latent_s_n >= L
 *   log_std_dev   [L] contiguous in in_dtype, read when the kernels run
 *   act_dev       [B] contiguous in in_dtype: the stored raw samples
 *   grad_log_std_dev   [L] contiguous in in_dtype, required
 *   grad_latent_dev    [B][L] with row stride gl_s_n >= L, nullable (SB3's on-policy learn_features=False: NULL)
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_sde_policy_loss_workspace(batch, latent_dim) bytes
 * Row i:  V, sd, lsd as in ptg_sde_act;  d = a - mu;  lp = ((-(d * d)) / (2 * V)) - lsd - 0.9189385332046727;  H = 1.4189385332046727 + lsd.
 * Gradients, g the surrogate's derivative of ptg_policy_loss:
 *   d loss / d mu = ((-g) * (d / V)) / B
 *   c_i = (((-g) * (((d * d) / V) - 1)) - c_e) / (2 * V)               (B times the loss's derivative with respect to V_i)
 *   d loss / d log_std[k] = ((2 * (s_k * s_k)) * sum_i c_i * (h_ik * h_ik)) / B
 *   d loss / d h_ik = ((c_i * (2 * h_ik)) * (s_k * s_k)) / B
 * Batch sums run in an order given by (B, L) alone, with no floating-point atomics -- the same inputs give the same bits on every
 * run.  With R = ceil(B / 4096) rows per wave, block b of 4 waves owns rows [4 R b, 4 R (b + 1)); wave w walks rows 4 R b + w,
 * 4 R b + w + 4, ... ascending; sum_i c_i * h_ik^2 is added per wave in that order from 0.0, then the block's waves in wave order,
 * then the blocks ascending.  The five means: per wave in the same row order, then ptg_policy_loss's steps 2 and 3 over these blocks.
 * Bad rows follow ptg_policy_loss's rules (NaN gradients, NaN stats[0..5], PTG_E_NONFINITE at the next ptg_sync); besides, a
 * non-finite latent entry or a non-finite V makes its row bad, and a NaN or +Inf log_std makes every row bad.  A bad row makes
 * every entry of grad_log_std NaN.
 * Enqueues kernels only -- s_k^2 into the workspace, the rows, the means, the log_std gradient, and two more in front for the moments
 * under PTG_LOSS_NORM_ADV -- no host synchronisation, no allocation.  Reads nothing of the handle but its device.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, mean_dev, val_dev, latent_dev, log_std_dev, act_dev, adv_dev, ret_dev,
 * stats_dev, grad_in_dev, grad_val_dev, grad_log_std_dev or ws_dev (or a ws_dev that is not 8-byte aligned); NULL old_logp_dev for
 * PPO; an unknown kind or flag; batch outside [1, 2^31]; an in_dtype other than the two; latent_dim outside [1, 1024]; mean_s_n,
 * g_s_n, val_s_n or gv_s_n below 1; latent_s_n, or gl_s_n with grad_latent_dev, below latent_dim; PTG_LOSS_CLIP_VF without
 * old_val_dev; a NaN or negative clip_range (PPO) or clip_range_vf (with PTG_LOSS_CLIP_VF).
 * ptg_sde_policy_loss_workspace(batch, latent_dim): bytes of scratch; with m = ceil(B / 256) and n = ceil(B / (4 R)) blocks it is
 * 8 * (4 + 3 m + L + n * (8 + L)); negative for a batch outside [1, 2^31] or a latent_dim outside [1, 1024]. */
typedef struct ptg_sde_loss {
    int32_t kind, flags;
    int32_t in_dtype, latent_dim;
    int64_t batch;
    const void* mean_dev;
    int64_t mean_s_n;
    const void* val_dev;
    int64_t val_s_n;
    const void* latent_dev;
    int64_t latent_s_n;
    const void* log_std_dev;
    const void* act_dev;
    const void* old_logp_dev;
    const void* adv_dev;
    const void* ret_dev;
    const void* old_val_dev;
    double clip_range, clip_range_vf, ent_coef, vf_coef;
    double* stats_dev;
    void* grad_in_dev;
    int64_t g_s_n;
    void* grad_val_dev;
    int64_t gv_s_n;
    void* grad_log_std_dev;
    void* grad_latent_dev;
    int64_t gl_s_n;
    void* ws_dev;
} ptg_sde_loss;
int64_t ptg_sde_policy_loss_workspace(int64_t batch, int32_t latent_dim);
int ptg_sde_policy_loss(ptg_env* env, const ptg_sde_loss* d, void* stream);

/* ---- gSDE for SAC and TQC: the squashed head, its reparametrised sample and the backward --------------------------------------
 * Replaces what SB3 2.0.0a13 runs for `gSDE : True` under SAC and TQC: sac/policies.py::Actor with use_sde builds
 * StateDependentNoiseDistribution(1, full_std=True, use_expln=False, learn_features=True, squash_output=True); log_std is [L, 1],
 * initialised at -3 and NOT clamped; mu = Sequential(Linear(L, 1), Hardtanh(-clip_mean, clip_mean)), clip_mean = 2.0; the latent is
 * the trunk's output, behind its activation.  Actor.action_log_prob (proba_distribution, sample, tanh, log_prob with the
 * log(1 - a^2 + 1e-6) correction) runs two or three times on every gradient step, and autograd walks back over it into the mean,
 * into the latent (through the variance and through the noise) and into log_std (through the variance and through the resampled
 * matrix itself, which is weights_dist.rsample()).  SAC.train / TQC.train call actor.reset_noise() (batch_size = 1) once per gradient
 * step: ONE [L] row serves the whole batch, the actor's pass over the observations and the target's pass over the next
 * observations alike.  While collecting, reset_noise(n_envs) gives one row per env; no log-prob, no gradient.
 * D = 1, 1 <= L <= 1024, strides and the arithmetic rules (float64, one rounding per operation, the order of the sums over k) as
 * stated above for the on-policy ops; tanh is the double-precision library function.  s_k = exp((double)log_std[k]), h_ik a latent entry.
 * Out of scope: use_expln; full_std=False; D > 1; sde_sample_freq as anything but the caller's schedule of the resample calls.
 *
 * ptg_sde_resample_rows is the training matrix: `rows` >= 1 rows of [L] at e_dev with the row stride e_s_n, E[r][k] = s_k * z, z
 * ptg_act's Gaussian draw from the words of ptg_replay_sample's chain keyed (seed, c, r * 1024 + k), c = *counter_dev -- NO global
 * env offset and no reading of n_envs: a row is a batch row, as in ptg_rsample.  Everything else (the descriptor, the trailing
 * one-thread kernel that does *counter_dev += 1, a NaN or +Inf log_std[k] making column k NaN and PTG_E_NONFINITE at the next
 * ptg_sync, two launches) is ptg_sde_resample's.  At global env offset 0 the first n_envs rows' keys are ptg_sde_resample's, so a
 * caller that holds both matrices keeps the streams apart: rl_ptg_amd.SquashedSdeNoise gives the training row a counter of its own
 * and the seed (seed XOR 0x9E3779B97F4A7C15).
 * PTG_E_INVALID (nothing enqueued): ptg_sde_resample's list, and rows outside [1, 2^31].
 *
 * ptg_sde_rsample is the forward, one launch; ptg_sde_rsample_backward the backward.  Both read a ptg_sde_rs, B = batch:
 *   flags         PTG_SDE_RS_DETERMINISTIC: noise = 0, e_dev is neither read nor required.  PTG_SDE_RS_SHARED_E: e_dev is ONE [L]
 *                 row for all B rows (training; e_s_n is not read); without it e_dev is [B][L], element (i, k) at i * e_s_n + k
 *                 (collecting: B is the matrix's row count)
 *   in_dtype      PTG_OUT_F32 | PTG_OUT_F64: of mean, latent, E, log_std, act, logp and of every gradient tensor
 *   batch         B >= 1, a 64-bit count that is not tied to the handle's n_envs; at most 2^31
 *   mean_dev      [B], element i at i * mean_s_n >= 1: the UNCLIPPED output of Linear(L, 1)
 *   latent_dev    [B][L], element (i, k) at i * latent_s_n + k, latent_s_n >= L;   log_std_dev [L] contiguous
 *   clip_mean     c, a host double: > 0 applies the Hardtanh, +Inf switches it off; <= 0 or NaN is refused
 *   act_dev       [B] contiguous in in_dtype: a = tanh(g)
 *   step_act_dev  float32 [B] contiguous, nullable: a rounded to float32, what ptg_step takes when in_dtype is float64 (0 on a bad row)
 *   logp_dev      [B] contiguous in in_dtype, nullable
 *   saved_dev     float64 [B][2] contiguous, 8-byte aligned: (noise, V) of row i at 2 i and 2 i + 1; nullable in the forward, which
 *                 writes it; the backward reads and requires it
 *   grad_act_dev, grad_logp_dev   backward inputs, [B] contiguous in in_dtype: d loss / d act and d loss / d logp; each nullable (= 0), not both
 *   grad_mean_dev [B], element i at i * gm_s_n >= 1, required: the gradient with respect to the unclipped mean
 *   grad_latent_dev   [B][L] with the row stride gl_s_n >= L, nullable
 *   grad_log_std_dev  [L] contiguous in in_dtype, nullable; refused without PTG_SDE_RS_SHARED_E (a collecting matrix has no backward)
 *   ws_dev        backward only: caller-owned device scratch, 8-byte aligned, at least ptg_sde_rsample_backward_workspace(batch,
 *                 latent_dim) bytes
 * Forward, row i, mu = mean[i], E_k the shared row's or row i's entry:
 *   m = mu < -c ? -c : (mu > c ? c : mu)
 *   V = (sum_k (h_ik * h_ik) * (s_k * s_k)) + 1e-6;   noise = sum_k h_ik * E_k  (deterministic: 0);   sd = sqrt(V);   lsd = log(sd)
 *   g = m + noise;   a = tanh(g);   act = a
 *   logp = ((((-(noise * noise)) / (2 * V)) - lsd) - 0.9189385332046727) - log((1 - a * a) + 1e-6)
 * With PTG_SDE_RS_SHARED_E the forward gives the bits of the per-row call on B copies of the row.
 * Backward, row i: ga = grad_act[i], gl = grad_logp[i] (0 when NULL); (noise, V) = saved[i]; m, g, a recomputed as above;
 *   d = 1 - a * a;   q = ((2 * a) * d) / (d + 1e-6);   t = ga * d + gl * q
 *   grad_mean = (-c < mu && mu < c) ? t : 0                 (torch's Hardtanh backward: exclusive at both ends)
 *   n = t - gl * (noise / V);   cV = (gl * (((noise * noise) / V) - 1)) / (2 * V)
 *   grad_latent[i][k] = (n * E_k) + ((cV * (2 * h_ik)) * (s_k * s_k))          (deterministic: E_k = 0)
 *   grad_log_std[k] = sum_i h_ik * grad_latent[i][k]        (the variance path 2 s_k^2 sum_i cV h_ik^2 and the matrix path
 *                     E_k sum_i n h_ik in one sum; computed whether or not grad_latent_dev is stored)
 * The batch sum runs in ptg_sde_policy_loss's order, given by (B, L) alone, with no floating-point atomics: R = ceil(B / 4096) rows
 * per wave, block b of 4 waves owns rows [4 R b, 4 R (b + 1)); wave w adds rows 4 R b + w, 4 R b + w + 4, ... ascending from 0.0, then
 * the block's waves in wave order, then the blocks ascending.
 * Known differences from SB3.  (1) SB3's log_prob(actions) recovers g as atanh(clamp(tanh(g), +-(1 - eps))), eps float32's; this op
 * uses g itself -- identical in exact arithmetic while the clamp is inactive; where the clamp saturates, SB3's gradient through the
 * action is zero and this one is not.  (2) Everything is float64, where SB3 computes in float32 and draws with torch's generator
 * (ptg_rsample's note).
 * Bad rows: a row whose mean, any latent entry, V or noise (backward: a saved value or an incoming gradient) is not finite, and every
 * row when any log_std is NaN or +Inf.  A bad row gets NaN in act, logp, grad_mean and its grad_latent row, 0 in step_act, and makes
 * every entry of grad_log_std NaN; the other rows keep their bits; the next ptg_sync returns PTG_E_NONFINITE once.  An exactly
 * saturated row (a = +-1, d = 0) is legal: q = 0 and logp is finite.
 * Enqueues kernels only -- the forward one (a wave per row, s_k * s_k once per workgroup in LDS), the backward s_k * s_k into the
 * workspace, the rows, and with grad_log_std_dev the sum over the blocks' column partials -- no host synchronisation, no allocation;
 * capturable.  Reads nothing of the handle but its device.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, mean_dev, latent_dev or log_std_dev; NULL e_dev unless deterministic; an
 * unknown flag; an in_dtype other than the two; latent_dim outside [1, 1024]; batch outside [1, 2^31]; mean_s_n < 1; latent_s_n <
 * latent_dim; e_s_n < latent_dim (stochastic, without PTG_SDE_RS_SHARED_E); a clip_mean that is <= 0 or NaN; a saved_dev that is not
 * 8-byte aligned; forward: NULL act_dev; backward: NULL saved_dev, grad_mean_dev or ws_dev (or a ws_dev that is not 8-byte aligned),
 * both incoming gradients NULL, gm_s_n < 1, gl_s_n < latent_dim with grad_latent_dev, grad_log_std_dev without PTG_SDE_RS_SHARED_E.
 * ptg_sde_rsample_backward_workspace(batch, latent_dim): bytes of scratch; with n = ceil(B / (4 R)) blocks it is 8 * L * (1 + n);
 * negative for a batch outside [1, 2^31] or a latent_dim outside [1, 1024]. */
enum { PTG_SDE_RS_DETERMINISTIC = 1, PTG_SDE_RS_SHARED_E = 2 };
typedef struct ptg_sde_rs {
    int32_t flags, in_dtype;
    int32_t latent_dim, reserved;
    int64_t batch;
    const void* mean_dev;
    int64_t mean_s_n;
    const void* latent_dev;
    int64_t latent_s_n;
    const void* e_dev;
    int64_t e_s_n;
    const void* log_std_dev;
    double clip_mean;
    void* act_dev;
    float* step_act_dev;
    void* logp_dev;
    double* saved_dev;
    const void* grad_act_dev;
    const void* grad_logp_dev;
    void* grad_mean_dev;
    int64_t gm_s_n;
    void* grad_latent_dev;
    int64_t gl_s_n;
    void* grad_log_std_dev;
    void* ws_dev;
} ptg_sde_rs;
int ptg_sde_resample_rows(ptg_env* env, const ptg_sde_noise* d, int64_t rows, void* stream);
int ptg_sde_rsample(ptg_env* env, const ptg_sde_rs* d, void* stream);
int64_t ptg_sde_rsample_backward_workspace(int64_t batch, int32_t latent_dim);
int ptg_sde_rsample_backward(ptg_env* env, const ptg_sde_rs* d, void* stream);

/* ---- the optimiser step: grad-norm clip, Adam / RMSprop, Polyak and zero_grad for all tensors of an optimiser --------------------
 * Replaces what the reference's agents (src/rl_config_agent.py; SB3 2.0.0a13 on torch) run behind loss.backward() on every minibatch:
 * torch.nn.utils.clip_grad_norm_(params, max_grad_norm), optimizer.step() of torch.optim.Adam (PPO, DQN, TD3, SAC, TQC) or RMSprop
 * (A2C), optimizer.zero_grad(), and -- TD3 / SAC / TQC after every gradient step, DQN every target_update_interval -- SB3's
 * polyak_update(params, targets, tau).  ALL parameter tensors of one optimiser take the step in a chain of at most three launches,
 * whatever their number: the tensor list does not travel in the launch arguments but in two caller-owned device tables.
 *   ptg_optim_tensor [n_tensors]   one record per tensor: device pointers to the parameter, its gradient, state 1 (Adam: exp_avg;
 *                 RMSprop: square_avg), state 2 (Adam: exp_avg_sq; else unused), its target (with PTG_OPTIM_TARGETS / PTG_OPTIM_POLYAK;
 *                 else unused) -- each `numel` contiguous elements of the descriptor's dtype; unused pointers are NULL
 *   ptg_optim_span [n_chunks]      one record per chunk: the index of its tensor and the element offset of the chunk in it.  A chunk is
 *                 C = 1024 consecutive elements of one tensor (the value ptg_optim_chunk returns); a tensor of numel elements has
 *                 ceil(numel / C) chunks at offsets 0, C, 2 C ..., the last one ragged.  One workgroup of 256 threads owns one chunk,
 *                 thread t its elements 4 t .. 4 t + 3.  C = 1024: PPO's 0.3 M parameters make some 300 chunks, more than the 256 CUs
 * The library cannot check what the tables point at: that every pointer covers numel elements, that the spans tile the tensors exactly
 * once -- every offset a multiple of C, every multiple of C below numel present -- and that no two tensors overlap is the caller's
 * contract (rl_ptg_amd/train_ops.py builds the tables from checked tensors).  A span whose tensor index is outside [0, n_tensors) or
 * whose offset is negative or no multiple of C (the 16-byte accesses rest on that) never becomes an address: it is skipped and the
 * next ptg_sync returns PTG_E_INDEX once.  Elements move as 16-byte pieces where every base a chunk uses is 16-byte aligned, else one by one: a
 * parameter may be a view at an odd element offset of a flat buffer.  Addressing is size_t throughout.
 * The call is described by a ptg_optim, read during the call:
 *   kind          PTG_OPTIM_ADAM | PTG_OPTIM_RMSPROP | PTG_OPTIM_POLYAK (targets only: no gradient, no state, one launch)
 *   flags         PTG_OPTIM_CLIP: clip by the total norm (max_norm).  PTG_OPTIM_TARGETS: also move the targets (tau).
 *                 PTG_OPTIM_ZERO_GRAD: write 0 to every gradient element after reading it (zero_grad(set_to_none=False): the
 *                 gradient pointers stay valid for the next replay).  PTG_OPTIM_POLYAK takes neither CLIP nor ZERO_GRAD
 *   dtype         PTG_OUT_F32 | PTG_OUT_F64: the ONE element type of every parameter, gradient, state and target tensor
 *   n_tensors, n_chunks, tensors_dev, chunks_dev   the two tables, 8-byte aligned
 *   state_dev     float64 [4] on the device = {t, beta1^t, beta2^t, spare}: the step count and the running products, {0, 1, 1, 0}
 *                 before the first step.  They advance on the device, by one multiplication per call, so a replayed graph takes step
 *                 t + 1.  RMSprop advances t only
 *   lr_dev        float64 [1] on the device, read when the kernel runs (anneal it in place between replays); NULL: the host double lr
 *   norm_dev      float64 [1] on the device: receives the total norm, the value clip_grad_norm_ returns.  Required with PTG_OPTIM_CLIP,
 *                 not written without it
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_optim_workspace(n_chunks) bytes; its contents mean
 *                 nothing before or after the call.  PTG_OPTIM_POLYAK does not use it
 *   lr, beta1, beta2, eps, alpha, tau, max_norm   host doubles; a captured call keeps them
 * Arithmetic.  Every element is loaded, converted to float64, computed in float64 with every operation rounded once (no fused
 * multiply-add; sqrt and the division are the correctly rounded ones) and rounded once to dtype on the store; the operand order is
 * torch's (CPU kernels).  g = (double)grad[i], and likewise m, v, s, p, q for exp_avg, exp_avg_sq, square_avg, parameter, target:
 *   total norm    with PTG_OPTIM_CLIP, clip_grad_norm_'s L2 norm with error_if_nonfinite=False: total = sqrt(sum g * g) over every element
 *                 of every gradient, in float64 in a fixed order -- thread t of a chunk adds its four squares in element order
 *                 (to 0.0), a shuffle tree over the wave's 64 lanes (xor 32, 16, 8, 4, 2, 1), the chunk's four waves in wave order, one
 *                 partial per chunk in ws_dev; then one workgroup in which thread u adds the partials of chunks u, u + 256, ... in that
 *                 order, the same tree, the four waves in wave order.  No floating-point atomics: the same inputs give the same bits
 *                 on every run, and the order depends on the tables alone.  A partial sum passes through at most
 *                 d = 22 + ceil(n_chunks / 256) roundings (1 square + 3, 6, 3 additions in the chunk; ceil(n_chunks / 256), 6, 3 after)
 *                 coef = min(max_norm / (total + 1e-6), 1.0) (torch.clamp: a NaN stays);  g' = g * coef.  Without PTG_OPTIM_CLIP there is
 *                 no norm pass and coef = 1.0 (g' = g exactly).  Known difference: the gradient tensors are NOT rewritten with
 *                 g'; no caller reads them after the step, and g' is not rounded to dtype on its way into the update
 *   Adam          torch.optim.Adam's single-tensor lines, no amsgrad, weight decay or maximize:
 *                 t += 1;  P1 = P1 * beta1;  P2 = P2 * beta2  (the running products in state_dev; torch evaluates beta ** t -- known
 *                 difference, a few ulp);  step_size = lr / (1 - P1);  bc2 = sqrt(1 - P2)
 *                 m = beta1 * m + (1 - beta1) * g'  (torch's lerp form m + (g' - m) * (1 - beta1) differs by an ulp: known difference)
 *                 v = beta2 * v + ((1 - beta2) * g') * g'
 *                 p = p + ((-step_size) * m) / (sqrt(v) / bc2 + eps)          with the unrounded m and v of this step
 *   RMSprop       torch.optim.RMSprop without momentum, not centered, no weight decay:
 *                 s = alpha * s + ((1 - alpha) * g') * g';   p = p + ((-lr) * g') / (sqrt(s) + eps)
 *   Polyak        SB3's polyak_update: q = (1 - tau) * q + tau * p, with p the parameter AS STORED by this call (rounded to dtype), so
 *                 the fused call equals the step followed by a PTG_OPTIM_POLYAK call, bit for bit.  tau = 1 copies a finite parameter
 *                 onto a finite target (DQN's hard update), as SB3's lines do: -0.0 arrives as +0.0 over a positive target, and a
 *                 non-finite target stays poisoned (0 * Inf)
 * Non-finite gradients propagate as the arithmetic says, as they do in torch.  A non-finite total norm, or without a norm pass a
 * non-finite gradient element, makes the next ptg_sync return PTG_E_NONFINITE once (its text names the calls that share that word).
 * Enqueues kernels only: the norm pass (with PTG_OPTIM_CLIP), a one-workgroup head kernel that merges the partials, advances
 * state_dev and writes the scalars of the update, and the update -- three launches, two without clipping, one for PTG_OPTIM_POLYAK --
 * with no host synchronisation and no allocation, so the call may be captured into a hipGraph and replayed.  Reads nothing of the
 * handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle or descriptor; an unknown kind, flag or dtype; PTG_OPTIM_POLYAK with PTG_OPTIM_CLIP
 * or PTG_OPTIM_ZERO_GRAD; n_tensors < 1; n_chunks outside [1, 2^31); a NULL or misaligned table; tau outside [0, 1] or NaN (with
 * targets); and for the two optimisers a NULL state_dev, a NULL or misaligned ws_dev, a negative or non-finite lr (with lr_dev NULL)
 * or eps, a beta outside [0, 1) (Adam), a negative or non-finite alpha (RMSprop), PTG_OPTIM_CLIP without norm_dev or with a negative
 * or NaN max_norm.
 * ptg_optim_workspace(n_chunks): bytes of scratch (8 per chunk + 32); negative for n_chunks outside [1, 2^31).
 * ptg_optim_chunk(): C, so that callers and tests find the chunk edges without hard-coding it. */
enum { PTG_OPTIM_ADAM = 0, PTG_OPTIM_RMSPROP = 1, PTG_OPTIM_POLYAK = 2 };
enum { PTG_OPTIM_CLIP = 1, PTG_OPTIM_TARGETS = 2, PTG_OPTIM_ZERO_GRAD = 4 };
typedef struct ptg_optim_tensor {
    void* param;
    void* grad;
    void* state1;
    void* state2;
    void* target;
    int64_t numel;
} ptg_optim_tensor;
typedef struct ptg_optim_span {
    int64_t tensor;
    int64_t offset;
} ptg_optim_span;
typedef struct ptg_optim {
    int32_t kind, flags;
    int32_t dtype, reserved;
    int64_t n_tensors, n_chunks;
    const void* tensors_dev;
    const void* chunks_dev;
    double* state_dev;
    const double* lr_dev;
    double* norm_dev;
    void* ws_dev;
    double lr, beta1, beta2, eps, alpha, tau, max_norm;
} ptg_optim;
int ptg_optim_chunk(void);
int64_t ptg_optim_workspace(int64_t n_chunks);
int ptg_optim_step(ptg_env* env, const ptg_optim* d, void* stream);

/* ---- the TD losses of the off-policy algorithms: DQN's and the TD3 / SAC critics', with their gradients, in one pass ----------------
 * Replaces what the reference's DQN, TD3 and SAC (src/rl_config_agent.py:80-222; SB3 2.0.0a13 DQN.train, TD3.train, SAC.train) run on
 * every gradient step between ptg_replay_sample's batch and the gradient that goes back into the Q network(s): the TD target
 * (th.max / th.min over the target network's outputs, the (1 - dones) * gamma product, SAC's entropy term), the gather of the chosen
 * Q-value, smooth_l1_loss or the sum of mse_loss, and autograd's walk back over the same graph.  Every gradient with respect to the
 * current Q-values is a closed form of what the forward pass holds, so one pass emits the loss, five statistics, d loss / d Q and
 * (optionally) the target; the caller's backward starts from those (rl_ptg_amd/loss.py: dqn_loss, td3_critic_loss, sac_critic_loss).
 * Out of scope: TQC's quantile-Huber critic loss (it has its own entry point, ptg_quantile_loss below; kind 2 stays refused here), the
 * actor and entropy-coefficient losses (ptg_actor_loss), TD3's target-action noise (it precedes the target networks: ptg_rsample,
 * PTG_RS_SMOOTH), double DQN, prioritised replay, the networks.
 * The call is described by a ptg_td, read during the call (B = batch, A = n_actions, K = n_critics):
 *   kind          PTG_TD_DQN | PTG_TD_CRITICS
 *   flags         PTG_TD_ENTROPY (critics only): SAC's term, the minimum loses alpha * next_log_prob.  PTG_TD_LOG_ALPHA (with
 *                 PTG_TD_ENTROPY and alpha_dev): the device scalar holds log alpha (SAC's learned log_ent_coef), alpha = exp of it
 *   batch         B >= 1, a 64-bit count that is not tied to the handle's n_envs; at most 2^31
 *   q_dtype       PTG_OUT_F32 | PTG_OUT_F64: the element type of every Q tensor, of next_logp_dev, of every gradient and of y_dev
 *   rew_dtype, done_dtype   PTG_OUT_F32 | PTG_OUT_F64, each on its own: the replay buffer's done column is float32, its reward column
 *                 has the engine's out_dtype
 *   DQN           q_dev[0] = Q(s, .) [B][A] and next_q_dev[0] = Q_target(s', .) [B][A], element (i, j) at i * s_n + j with the row strides
 *                 q_s_n[0], next_s_n[0] >= A, 2 <= A <= 32; act_dev the chosen actions [B] contiguous, act_kind PTG_ACT_I32 | PTG_ACT_I64;
 *                 grad_q_dev[0] [B][A] with the row stride g_s_n[0] >= A.  The other array entries and n_critics are not read
 *   critics       q_dev[k], next_q_dev[k], grad_q_dev[k] for k < K, 1 <= K <= PTG_TD_MAX_CRITICS: [B] each, element i at i * stride with its
 *                 own stride >= 1 -- SB3's tuple of [B, 1] tensors and the columns of one [B, K] tensor both fit.  The pointers and
 *                 strides travel by value in the launch.  n_actions, act_dev and act_kind are not read
 *   rew_dev, done_dev   [B] contiguous.  done is a number, not a flag: it need not be 0 or 1
 *   next_logp_dev [B] contiguous in q_dtype: log pi(a' | s') of the next action; required iff PTG_TD_ENTROPY
 *   alpha_dev     float64 [1] on the device, read when the kernel runs (the optimiser moves it between replays); NULL: the host double alpha
 *   gamma, alpha, scale   host doubles; a captured call keeps them.  scale = c: 1 for TD3, 0.5 for SAC; not read by DQN
 *   stats_dev     float64 [8] = {loss, mean current Q (DQN: the chosen one; critics: over k and rows), mean y, mean |delta|, share of the
 *                 delta with |delta| >= 1 (critics: over k and rows), alpha as used (0 without PTG_TD_ENTROPY), 0, 0}
 *   y_dev         nullable: receives the target y [B] contiguous in q_dtype
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_td_loss_workspace(batch) bytes; its contents mean nothing
 *                 before or after the call
 * Arithmetic: all of it in float64 whatever the dtypes are, every operation rounded once (no fused multiply-add), outputs rounded once
 * on the store; exp (PTG_TD_LOG_ALPHA only) is the double-precision library function.  Row i, r = rew[i], d = done[i]:
 *   DQN           m = next_q[i][0];  for j = 1 .. A - 1: l = next_q[i][j], m = l if l > m or l != l  (torch.max's NaN rule: a NaN in any
 *                 column makes m NaN -- fmax would drop it)
 *                 y = r + ((1 - d) * gamma) * m;   delta = q[i][a] - y
 *                 term = |delta| < 1 ? 0.5 * (delta * delta) : |delta| - 0.5        (smooth_l1_loss, beta = 1)
 *                 loss = (sum term) / B;   d loss / d q[i][j] = [j == a] * clamp(delta, -1, 1) / B: the whole row is written, zeros off
 *                 the chosen column
 *   critics       m = next_q_0[i];  for k = 1 .. K - 1: l = next_q_k[i], m = l if l < m or l != l  (th.min, the same NaN rule)
 *                 with PTG_TD_ENTROPY: m = m - alpha * next_logp[i]
 *                 y = r + ((1 - d) * gamma) * m;   delta_k = q_k[i] - y
 *                 term = ((0 + delta_0 * delta_0) + delta_1 * delta_1) + ...  in k order
 *                 loss = (c * (sum term)) / B;   d loss / d q_k[i] = ((c * 2) * delta_k) / B
 *   statistics    stats[1] = (sum of the current Q) / n, stats[2] = (sum y) / B, stats[3] = (sum |delta|) / n, stats[4] = (number of
 *                 |delta| >= 1) / n, with n = B (DQN) or B * K (critics; a row adds its K values in k order before it enters the sum)
 * Sums run in ptg_policy_loss's fixed order (per wave a shuffle tree, the four waves of a 256-row block in order, one partial per block
 * in ws_dev, a last pass over the partials; no floating-point atomics): the same inputs give the same bits on every run.
 * Known differences from SB3: it computes these lines in float32 where the networks are float32; here they are float64 and rounded
 * once.  SB3 adds K per-critic means, sum_k mean_i delta_k^2; here the rows' sums of K terms are added and divided once.
 * Bad rows.  No index ever becomes an address: a DQN action outside [0, A) leaves the row's gradient row and its y untouched and the
 * next ptg_sync (or any call that reports kernel-flagged errors) returns PTG_E_INDEX once.  A row is non-finite when its y or its
 * chosen (critics: any current) Q is not finite -- a non-finite reward, done, next-Q extremum, log-prob or alpha, a NaN anywhere in the
 * next-Q row, or 0 * Inf where (1 - d) * gamma is 0: it gets NaN gradients (DQN: the whole row), its y as computed, and the next
 * ptg_sync returns PTG_E_NONFINITE once.  Either kind of row makes stats[0..4] NaN; the other rows are computed as usual.  A -Inf
 * next-Q beside a larger one is legal for DQN's max (a +Inf beside a smaller one for the critics' min), and so is a non-finite current
 * Q on a column that was not chosen: it is not read.
 * Enqueues kernels only -- one for B <= 256, else the rows and a one-workgroup merge of the block partials (the reference's batches,
 * DQN's 544, TD3's 257 and SAC's 470, take these two) -- with no host synchronisation and no allocation, so the call may be captured into a
 * hipGraph and replayed.  Reads nothing of the handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and
 * every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, stats_dev, rew_dev, done_dev or ws_dev (or a ws_dev that is not 8-byte
 * aligned); a NULL q_dev, next_q_dev or grad_q_dev entry in use; NULL act_dev (DQN); an unknown kind, flag or dtype code; batch < 1 or
 * above 2^31; n_actions outside [2, 32] or an act_kind other than PTG_ACT_I32 | PTG_ACT_I64 (DQN); n_critics outside [1, 4] (critics);
 * a row stride below A (DQN) or a stride below 1 (critics); PTG_TD_ENTROPY on DQN, or without next_logp_dev; PTG_TD_LOG_ALPHA without
 * PTG_TD_ENTROPY or without alpha_dev.
 * ptg_td_loss_workspace(batch): bytes of scratch a batch of that size needs (64 per 256 rows); negative for batch < 1 or above 2^31. */
#define PTG_TD_MAX_CRITICS 4
enum { PTG_TD_DQN = 0, PTG_TD_CRITICS = 1 };      /* the quantile critics (TQC) have their own entry point: ptg_quantile_loss */
enum { PTG_TD_ENTROPY = 1, PTG_TD_LOG_ALPHA = 2 };
typedef struct ptg_td {
    int32_t kind, flags;
    int32_t n_actions, n_critics;
    int32_t q_dtype, act_kind;
    int32_t rew_dtype, done_dtype;
    int64_t batch;
    const void* q_dev[PTG_TD_MAX_CRITICS];
    int64_t q_s_n[PTG_TD_MAX_CRITICS];
    const void* next_q_dev[PTG_TD_MAX_CRITICS];
    int64_t next_s_n[PTG_TD_MAX_CRITICS];
    const void* act_dev;
    const void* rew_dev;
    const void* done_dev;
    const void* next_logp_dev;
    const double* alpha_dev;
    double gamma, alpha, scale;
    double* stats_dev;
    void* grad_q_dev[PTG_TD_MAX_CRITICS];
    int64_t g_s_n[PTG_TD_MAX_CRITICS];
    void* y_dev;
    void* ws_dev;
} ptg_td;
int64_t ptg_td_loss_workspace(int64_t batch);
int ptg_td_loss(ptg_env* env, const ptg_td* d, void* stream);

/* ---- the quantile-Huber loss of TQC's critics, with its gradients, in one pass -------------------------------------------------------
 * Replaces what the reference's TQC (src/rl_config_agent.py:80-222; sb3_contrib's TQC.train, critic part, and
 * quantile_huber_loss(current_quantiles, target_quantiles, sum_over_quantiles=False)) runs on every gradient step between
 * ptg_replay_sample's batch and the gradient that goes back into the quantile critics: th.sort over the target critics' K * Q quantiles,
 * the slice that drops the top d * K of them, the entropy term, the (1 - dones) * gamma product, the [B, K, Q, M] tensor of pairwise
 * differences, abs / where / comparison / mean over it, and autograd's walk back.  The kernel never stores a pair: one pass emits the
 * loss, four statistics, d loss / d current quantile and (optionally) the targets; the caller's backward starts from those
 * (rl_ptg_amd/loss.py: tqc_critic_loss).
 * Out of scope: the actor and entropy-coefficient losses (ptg_actor_loss below), the networks.
 * The call is described by a ptg_ql, read during the call.  Sizes: B = batch rows, K = n_critics, Q = n_quantiles per critic,
 * d = n_drop (top_quantiles_to_drop_per_net), M = K * (Q - d) kept target quantiles.  The reference: B = 290, K = 2, Q = 30, d = 2,
 * M = 56, gamma = 0.9639, alpha = 0.00047; SB3's defaults: Q = 25, d = 2.
 *   flags         PTG_QL_LOG_ALPHA (with alpha_dev): the device scalar holds log alpha (the learned log_ent_coef), alpha = exp of it
 *   n_critics     1 <= K <= PTG_TD_MAX_CRITICS;   n_quantiles  1 <= Q <= PTG_QL_MAX_QUANTILES;   n_drop  0 <= d < Q
 *   batch         B >= 1, a 64-bit count that is not tied to the handle's n_envs; at most 2^31
 *   q_dtype       PTG_OUT_F32 | PTG_OUT_F64: the element type of every quantile tensor, of next_logp_dev, of every gradient and of y_dev
 *   rew_dtype, done_dtype   PTG_OUT_F32 | PTG_OUT_F64, each on its own
 *   cur_dev[k], next_dev[k], grad_dev[k]   for k < K: [B][Q] each, element (b, i) at b * stride + i with its own row stride cur_s_n[k],
 *                 next_s_n[k], g_s_n[k] >= Q.  SB3's stacked [B, K, Q] tensor fits (pointer offset k * Q, stride K * Q) and so does a
 *                 tuple of K [B, Q] tensors.  The pointers and strides travel by value in the launch
 *   rew_dev, done_dev   [B] contiguous.  done is a number, not a flag
 *   next_logp_dev [B] contiguous in q_dtype: log pi(a' | s') of the next action.  The entropy term is always present
 *   alpha_dev     float64 [1] on the device, read when the kernel runs; NULL: the host double alpha
 *   gamma, alpha  host doubles; a captured call keeps them
 *   stats_dev     float64 [8] = {loss, mean current quantile (over B * K * Q), mean y (over B * M), mean |delta| (over n), share of the
 *                 pairs with |delta| > 1 (over n: the linear branch; strictly greater, where ptg_td_loss counts >=), alpha as used, 0, 0}
 *   y_dev         nullable: receives the targets y [B][M] contiguous in q_dtype
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_quantile_loss_workspace(batch) bytes; its contents mean
 *                 nothing before or after the call
 * Arithmetic: all of it in float64 whatever the dtypes are, every operation rounded once (no fused multiply-add), outputs rounded once
 * on the store; exp (PTG_QL_LOG_ALPHA only) is the double-precision library function.  Row b, r = rew[b], dn = done[b], lp = next_logp[b]:
 *   sort          s = the K * Q next quantiles of the row, all critics together, ascending in torch.sort's order: element p (flat index
 *                 k * Q + i, value v_p) comes before element e iff v_p < v_e, or v_e is a NaN and v_p is not; otherwise the smaller
 *                 flat index comes first.  A NaN ranks above +Inf.  s_0 .. s_(M-1) are kept
 *   target        t_j = s_j - alpha * lp;   y_j = r + ((1 - dn) * gamma) * t_j
 *   pairs         for every current quantile theta = cur_k[b][i], tau_i = (i + 0.5) / Q:  acc = 0, ls = 0, then for j = 0 .. M - 1 in
 *                 this order:  delta = y_j - theta;  a = |delta|;  w = |tau_i - (delta < 0 ? 1 : 0)|;
 *                 h = a > 1 ? a - 0.5 : 0.5 * (delta * delta);  c = clamp(delta, -1, 1);  acc = acc + w * c;  ls = ls + w * h
 *   gradient      n = ((B * K) * Q) * M as a double;   d loss / d cur_k[b][i] = (-acc) / n
 *   loss          (sum of ls over all rows, critics and quantiles) / n
 *   statistics    stats[1] = (sum theta) / ((B * K) * Q), stats[2] = (sum y) / (B * M), stats[3] = (sum a) / n, stats[4] = (number of
 *                 pairs with a > 1) / n
 * Sums run in a fixed order (a lane adds its pairs in flat-index order, per wave a shuffle tree, the four waves = rows of a block in
 * order, one partial per block in ws_dev, a last pass over the partials; no floating-point atomics): the same inputs give the same bits
 * on every run.
 * Known differences from SB3: it keeps cum_prob and, with float32 networks, every one of these lines in float32; here everything is
 * float64 and rounded once.  SB3's .mean() sums in torch's order; here the order is the fixed one above.
 * Bad rows.  There is no index, so PTG_E_INDEX never arises.  A row is non-finite when any kept y_j or any of its current quantiles is
 * not finite: all of its K * Q gradients become NaN, its y is written as computed, stats[0..4] become NaN and the next ptg_sync returns
 * PTG_E_NONFINITE once; the other rows are computed as usual.  A NaN or +Inf among the dropped top d * K values is legal, as a -Inf
 * beside a larger value is for DQN's max; with d = 0 nothing is dropped, so a NaN or +Inf anywhere among the next quantiles makes the
 * row non-finite.
 * Enqueues kernels only -- one wave per row, four rows per 256-thread workgroup; one launch for B <= 4, else the rows and a
 * one-workgroup merge of the block partials -- with no host synchronisation and no allocation, so the call may be captured into a
 * hipGraph and replayed.  Reads nothing of the handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and
 * every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, stats_dev, rew_dev, done_dev, next_logp_dev or ws_dev (or a ws_dev that is
 * not 8-byte aligned); a NULL cur_dev, next_dev or grad_dev entry in use; an unknown flag or dtype code; batch < 1 or above 2^31;
 * n_critics outside [1, 4]; n_quantiles outside [1, 64]; n_drop outside [0, n_quantiles); a row stride below Q; PTG_QL_LOG_ALPHA
 * without alpha_dev.
 * ptg_quantile_loss_workspace(batch): bytes of scratch a batch of that size needs (64 per 4 rows); negative for batch < 1 or above 2^31. */
#define PTG_QL_MAX_QUANTILES 64
enum { PTG_QL_LOG_ALPHA = 1 };
typedef struct ptg_ql {
    int32_t flags, n_critics;
    int32_t n_quantiles, n_drop;
    int32_t q_dtype, rew_dtype;
    int32_t done_dtype, reserved;
    int64_t batch;
    const void* cur_dev[PTG_TD_MAX_CRITICS];
    int64_t cur_s_n[PTG_TD_MAX_CRITICS];
    const void* next_dev[PTG_TD_MAX_CRITICS];
    int64_t next_s_n[PTG_TD_MAX_CRITICS];
    void* grad_dev[PTG_TD_MAX_CRITICS];
    int64_t g_s_n[PTG_TD_MAX_CRITICS];
    const void* rew_dev;
    const void* done_dev;
    const void* next_logp_dev;
    const double* alpha_dev;
    double gamma, alpha;
    double* stats_dev;
    void* y_dev;
    void* ws_dev;
} ptg_ql;
int64_t ptg_quantile_loss_workspace(int64_t batch);
int ptg_quantile_loss(ptg_env* env, const ptg_ql* d, void* stream);

/* ---- the training-time actor head: reparametrised sample, log-prob and their backward; TD3's smoothed target action -----------------
 * Replaces what the reference's SAC and TQC (src/rl_config_agent.py:80-222; SB3 2.0.0a13 sac/policies.py Actor.action_log_prob with
 * SquashedDiagGaussianDistribution) run on every gradient step between the actor network's (mean, log_std) and the critics: the
 * log_std clamp to [-20, 2], exp, rsample, tanh, the Gaussian log-density, the log(1 - a^2 + 1e-6) correction -- and autograd's walk
 * back over all of it -- and TD3.train's target-policy smoothing (normal_(0, target_policy_noise).clamp(-c, c), added, clamped again).
 * ptg_act's squashed Gaussian serves while collecting: it is sized by n_envs, has no clamp and no gradient.  D = 1 as everywhere.
 * The call is described by a ptg_rs, read during the call; ptg_rsample is the forward, ptg_rsample_backward the backward:
 *   kind          PTG_RS_SQUASH (SAC / TQC) | PTG_RS_SMOOTH (TD3's target action: forward only, no log-prob)
 *   flags         PTG_RS_DETERMINISTIC: z = 0; counter_dev is neither read nor advanced (and may be NULL)
 *   q_dtype       PTG_OUT_F32 | PTG_OUT_F64: the element type of mean, log_std, act, logp and of the four gradient tensors
 *   batch         B >= 1, a 64-bit count that is not tied to the handle's n_envs; at most 2^31
 *   mean_dev      [B], element b at b * mean_s_n, mean_s_n >= 1
 *   log_std_dev   [B], element b at b * log_std_s_n >= 1: the network's UNCLAMPED output.  Not read by PTG_RS_SMOOTH
 *   seed, counter_dev   the draw: row b of the c-th call (c = *counter_dev, uint64 [1], read on the device) takes the words (w0, w1) of
 *                 ptg_replay_sample's chain keyed (seed, c, b) -- NO global env offset: a row is a batch row, not an env.  A trailing
 *                 one-thread kernel does *counter_dev += 1 in stream order unless the call is deterministic, as ptg_act does
 *   noise_std, noise_clip, clip_lo, clip_hi   PTG_RS_SMOOTH only, host doubles: sigma_t >= 0 and finite, c >= 0, lo <= hi
 *   act_dev       [B] contiguous in q_dtype: the action, unclipped (tanh keeps it inside [-1, 1])
 *   logp_dev      [B] contiguous in q_dtype, nullable; refused for PTG_RS_SMOOTH
 *   noise_dev     float64 [B] contiguous, nullable in the forward, where it receives z; the backward reads it (so it does not depend on
 *                 the counter) and requires it
 *   grad_act_dev, grad_logp_dev   backward inputs, [B] contiguous in q_dtype: d L / d act and d L / d logp; each nullable (= 0), not both
 *   grad_mean_dev, grad_log_std_dev   backward outputs, element b at b * gm_s_n and b * gl_s_n (>= 1), both required
 * Arithmetic: all of it in float64 whatever q_dtype is, every operation rounded once (no fused multiply-add), outputs rounded once on
 * the store; exp, log, sqrt, cos, tanh are the double-precision library functions.  Row b, mu = mean[b], l = log_std[b]:
 *   clamp         ls = l < -20 ? -20 : (l > 2 ? 2 : l)  (a NaN stays NaN);   pass = (-20 <= l && l <= 2);   sigma = exp(ls)
 *   draw          u1 = (w0 + 1) * 2^-32;  u2 = w1 * 2^-32;  z = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2): ptg_act's Gaussian
 *                 lines;  deterministic: z = 0
 *   squash        g = mu + sigma * z;   a = tanh(g);   act = a
 *                 logp = (((-(z * z)) / 2 - ls) - 0.9189385332046727) - log((1 - a * a) + 1e-6)
 *   smooth        act = clip(mu + clip(sigma_t * z, -c, c), lo, hi),  clip(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x)  (ptg_act's)
 *   backward      ls, pass, sigma, g, a recomputed as above with z = noise[b];  ga = grad_act[b], gl = grad_logp[b] (0 when NULL)
 *                 d = 1 - a * a;   sz = sigma * z;   q = ((2 * a) * d) / (d + 1e-6)
 *                 grad_mean = ga * d + gl * q
 *                 grad_log_std = pass ? (ga * (d * sz) + gl * (q * sz - 1)) : 0      (torch's clamp gradient, inclusive at both ends)
 * With log_std inside the clamp the forward gives the bits of ptg_act's squashed head at the same (seed, counter) on a handle with
 * n_envs = B and no global env offset.
 * Known difference from SB3: it computes these lines in float32 where the networks are float32, and draws with torch's generator.
 * Bad rows: a non-finite mean or a NaN log_std (an infinite log_std clamps and is legal); in the backward also a non-finite incoming
 * gradient or noise value.  A bad row gets NaN in act and logp (backward: in both gradients; its noise is written as drawn), the other
 * rows are computed as usual, and the next ptg_sync (or any call that reports kernel-flagged errors) returns PTG_E_NONFINITE once.
 * Enqueues kernels only -- one lane per row, 256-thread workgroups, one launch plus the counter kernel -- with no host synchronisation
 * and no allocation, so a call may be captured into a hipGraph and replayed (a replay draws afresh).  Reads nothing of the handle but
 * its device: env state, the finished-episode ring, the ptg_vn_* statistics and every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor or mean_dev; an unknown kind, flag or dtype code; batch < 1 or above 2^31;
 * a stride below 1; PTG_RS_SQUASH without log_std_dev; forward: NULL act_dev, NULL counter_dev unless deterministic, a noise_dev
 * that is not 8-byte aligned, PTG_RS_SMOOTH with logp_dev, with a negative, NaN or infinite noise_std, a negative or NaN noise_clip,
 * clip_lo > clip_hi or a NaN bound; backward: PTG_RS_SMOOTH, NULL (or misaligned) noise_dev, both incoming gradients NULL, a NULL
 * gradient output. */
enum { PTG_RS_SQUASH = 0, PTG_RS_SMOOTH = 1 };
enum { PTG_RS_DETERMINISTIC = 1 };
typedef struct ptg_rs {
    int32_t kind, flags;
    int32_t q_dtype, reserved;
    int64_t batch;
    const void* mean_dev;
    int64_t mean_s_n;
    const void* log_std_dev;
    int64_t log_std_s_n;
    uint64_t seed;
    uint64_t* counter_dev;
    double noise_std, noise_clip, clip_lo, clip_hi;
    void* act_dev;
    void* logp_dev;
    double* noise_dev;
    const void* grad_act_dev;
    const void* grad_logp_dev;
    void* grad_mean_dev;
    int64_t gm_s_n;
    void* grad_log_std_dev;
    int64_t gl_s_n;
} ptg_rs;
int ptg_rsample(ptg_env* env, const ptg_rs* d, void* stream);
int ptg_rsample_backward(ptg_env* env, const ptg_rs* d, void* stream);

/* ---- the actor and entropy-coefficient losses of SAC / TQC / TD3, with their gradients, in one pass ---------------------------------
 * Replaces the actor half of a gradient step of the reference's TD3, SAC and TQC (src/rl_config_agent.py:80-222; SB3 2.0.0a13 SAC.train,
 * TD3.train, sb3_contrib's TQC.train):
 *   ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
 *   SAC  actor_loss = (ent_coef * log_prob - th.min(q_values_pi, dim=1)).mean()
 *   TQC  actor_loss = (ent_coef * log_prob - critic(obs, a_pi).mean(2).mean(1)).mean()
 *   TD3  actor_loss = -critic.q1_forward(obs, actor(obs)).mean()
 * and autograd's walk back to the critics' outputs, the log-prob and log_ent_coef: closed forms of what the forward pass holds.
 * The call is described by a ptg_al, read during the call (B = batch, K = n_critics, Q = n_quantiles):
 *   kind          PTG_AL_MIN (SAC): q_dev[k] is [B], element b at b * q_s_n[k], stride >= 1, 1 <= K <= PTG_TD_MAX_CRITICS; n_quantiles
 *                 is not read.  PTG_AL_MEAN (TQC; TD3 is K = Q = 1 without PTG_AL_ENTROPY): q_dev[k] is [B][Q], element (b, i) at
 *                 b * q_s_n[k] + i with a row stride >= Q, 1 <= Q <= PTG_QL_MAX_QUANTILES: the stacked [B, K, Q] tensor (pointer offset
 *                 k * Q, stride K * Q) and a list both fit.  PTG_AL_ALPHA_ONLY: only the entropy-coefficient loss; no q is read,
 *                 n_critics and n_quantiles are not read, the flags must be PTG_AL_LOG_ALPHA | PTG_AL_ENT_COEF
 *   flags         PTG_AL_ENTROPY: the alpha * lp term; needs logp_dev.  PTG_AL_LOG_ALPHA (with alpha_dev): the device scalar holds
 *                 log alpha, alpha = exp of it; needs PTG_AL_ENTROPY or PTG_AL_ENT_COEF.  PTG_AL_ENT_COEF: also emit the
 *                 entropy-coefficient loss; needs PTG_AL_LOG_ALPHA, logp_dev and a finite target_entropy
 *   q_dtype       PTG_OUT_F32 | PTG_OUT_F64: the element type of every q tensor, of logp_dev and of the gradients but grad_log_alpha_dev
 *   logp_dev      [B] contiguous in q_dtype: log pi(a_pi | s)
 *   alpha_dev     float64 [1] on the device, read when the kernel runs; NULL: the host double alpha.  The three forms of alpha are
 *                 ptg_td_loss's: a host double, a device scalar, a device log alpha.  Without PTG_AL_ENTROPY and PTG_AL_ENT_COEF alpha
 *                 is 0 and nothing is read
 *   target_entropy   H_t, a host double (SB3: -dim(action space) = -1)
 *   stats_dev     float64 [8] = {actor_loss, ent_coef_loss, mean lp, mean m, alpha as used, d ent_coef_loss / d log alpha, 0, 0}, with 0
 *                 where a part is not asked for (actor_loss and mean m for PTG_AL_ALPHA_ONLY; ent_coef_loss and its gradient without
 *                 PTG_AL_ENT_COEF; mean lp when no flag reads it).  &stats_dev[4] is a float64 device scalar that ptg_td_loss,
 *                 ptg_quantile_loss and a later ptg_actor_loss accept as alpha_dev (not a log: without their LOG_ALPHA flag)
 *   grad_q_dev[k] shaped and strided (g_s_n[k]) like q_dev[k], required for k < K
 *   grad_logp_dev [B] contiguous in q_dtype, nullable; goes with PTG_AL_ENTROPY
 *   grad_log_alpha_dev   float64 [1], nullable; goes with PTG_AL_ENT_COEF
 *   ws_dev        caller-owned device scratch, 8-byte aligned, at least ptg_actor_loss_workspace(batch) bytes
 * Arithmetic: all of it in float64 whatever q_dtype is, every operation rounded once, outputs rounded once on the store; exp
 * (PTG_AL_LOG_ALPHA only) is the double-precision library function.  Row b, lp = logp[b]:
 *   MIN           m = q_0[b], k* = 0;  for k = 1 .. K - 1: l = q_k[b], and m = l, k* = k if l < m or l != l  (th.min's NaN rule; of
 *                 equal values the first index wins);   d loss / d q_k[b] = [k == k*] * ((-1) / B), every k written
 *   MEAN          m = (sum_k ((sum_i theta_ki) / Q)) / K, both sums from 0 in index order;   d loss / d theta = (-1) / ((B * K) * Q)
 *   both          term = alpha * lp - m with PTG_AL_ENTROPY, else -m;   d loss / d lp[b] = alpha / B
 *   batch         actor_loss = (sum term) / B;   mean lp = (sum lp) / B;   mean m = (sum m) / B
 *                 with PTG_AL_ENT_COEF: S = sum (lp + H_t);  ent_coef_loss = -(log alpha * (S / B));  d / d log alpha = -(S / B)
 * Sums run in ptg_policy_loss's fixed order (per wave a shuffle tree, the four waves of a 256-row block in order, one partial per block
 * in ws_dev, a last pass over the partials; no floating-point atomics): the same inputs give the same bits on every run.
 * Known differences from SB3: it computes these lines in float32 where the networks are float32, and sums in torch's order; here
 * everything is float64, rounded once, in the fixed order above.
 * Call order: SB3 computes ent_coef_loss BEFORE the critic update and the actor loss AFTER it, both with the alpha from before the
 * alpha optimiser's step.  PTG_AL_ALPHA_ONLY exists so that the order can be reproduced: its stats_dev[4] keeps that alpha on the
 * device for the critic loss and the later actor loss while the optimiser moves log alpha.
 * Bad rows.  There is no index.  A row whose m or lp (when read) is not finite -- a NaN critic, a -Inf minimum, any non-finite
 * quantile -- and every row when alpha (or, with alpha_dev, the scalar it is made from) is not finite gets NaN gradients; stats[0..3]
 * and stats[5] (and grad_log_alpha_dev) become NaN and the next ptg_sync returns PTG_E_NONFINITE once; the other rows are computed as
 * usual.  A +Inf critic beside a smaller one is legal for the minimum.
 * Enqueues kernels only -- one lane per row; one launch for B <= 256, else the rows and a one-workgroup merge of the block partials --
 * with no host synchronisation and no allocation, so the call may be captured into a hipGraph and replayed.  Reads nothing of the
 * handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and every replay cursor are untouched.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, stats_dev or ws_dev (or a ws_dev that is not 8-byte aligned); an unknown
 * kind, flag or dtype code; batch < 1 or above 2^31; n_critics outside [1, 4]; n_quantiles outside [1, 64] (MEAN); a NULL q_dev or
 * grad_q_dev entry in use; a stride below 1 (MIN) or below Q (MEAN); PTG_AL_ALPHA_ONLY with PTG_AL_ENTROPY or without PTG_AL_ENT_COEF;
 * PTG_AL_ENT_COEF without PTG_AL_LOG_ALPHA or with a target_entropy that is not finite; PTG_AL_LOG_ALPHA without alpha_dev or without
 * a flag that uses alpha; a flag that reads logp_dev without it; grad_logp_dev without PTG_AL_ENTROPY; grad_log_alpha_dev without
 * PTG_AL_ENT_COEF or not 8-byte aligned.
 * ptg_actor_loss_workspace(batch): bytes of scratch a batch of that size needs (64 per 256 rows); negative for batch < 1 or above 2^31. */
enum { PTG_AL_MIN = 0, PTG_AL_MEAN = 1, PTG_AL_ALPHA_ONLY = 2 };
enum { PTG_AL_ENTROPY = 1, PTG_AL_LOG_ALPHA = 2, PTG_AL_ENT_COEF = 4 };
typedef struct ptg_al {
    int32_t kind, flags;
    int32_t n_critics, n_quantiles;
    int32_t q_dtype, reserved;
    int64_t batch;
    const void* q_dev[PTG_TD_MAX_CRITICS];
    int64_t q_s_n[PTG_TD_MAX_CRITICS];
    const void* logp_dev;
    const double* alpha_dev;
    double alpha, target_entropy;
    double* stats_dev;
    void* grad_q_dev[PTG_TD_MAX_CRITICS];
    int64_t g_s_n[PTG_TD_MAX_CRITICS];
    void* grad_logp_dev;
    double* grad_log_alpha_dev;
    void* ws_dev;
} ptg_al;
int64_t ptg_actor_loss_workspace(int64_t batch);
int ptg_actor_loss(ptg_env* env, const ptg_al* d, void* stream);

/* ---- the inference forward of an MLP: one fused launch per layer, Linear + bias + activation on the f32 matrix cores -------------------
 * Replaces th.no_grad() calls of the nets that SB3's create_mlp builds for the reference (config/config_agent.yaml: 2 - 7 hidden layers
 * of 233 - 808 units, ReLU or Tanh): the policy while collecting and evaluating, the target actor / critics / q_net of a gradient step.
 * The backward pass is ptg_mlp_backward (below), which reads what a PTG_MLP_KEEP_HIDDEN call of this one leaves; together they are the
 * training forward and backward.
 * The call is described by a ptg_mlp, read during the call and holding no host memory (B = batch, n = n_layers):
 *   batch         B, 1 <= B <= 2^31
 *   n_layers      n, 1 <= n <= PTG_MLP_MAX_LAYERS (the reference's deepest net is DQN's: 7 hidden layers and the output layer)
 *   flags         PTG_MLP_KEEP_HIDDEN: every post-activation hidden layer stays in ws_dev (below).  PTG_MLP_NARROW / PTG_MLP_WIDE, for
 *                 tests and measurements: every layer takes that tile route instead of the host's choice; both at once are refused.
 *                 PTG_MLP_SPLIT_INPUT: x_dev holds PTG_OBS_SPLIT rows (below)
 *   hidden_act    PTG_MLP_RELU | PTG_MLP_TANH, applied after every layer but the last
 *   out_act       PTG_MLP_NONE | PTG_MLP_RELU | PTG_MLP_TANH, applied after the last (TD3's actor ends in tanh; a trunk called on its own
 *                 ends in its hidden activation)
 *   x_dev, x2_dev the input as one or two pieces [B][f1] and [B][f2], float32, element (b, k) at b * x_s_n + k (b * x2_s_n + k), row
 *                 strides >= f1 (f2): a critic's th.cat([obs, action], 1) without the cat.  x2_dev NULL: one piece, f2 must be 0.
 *                 f1 + f2 is the first layer's fan-in, 1 <= f1, 0 <= f2, f1 + f2 <= PTG_MLP_MAX_WIDTH
 *   w_dev[l]      float32 [width[l]][in_l] in torch's Linear.weight layout, element (j, k) at j * w_s_n[l] + k, w_s_n[l] >= in_l, where
 *                 in_0 = f1 + f2 and in_l = width[l - 1];  b_dev[l] float32 [width[l]] contiguous;  1 <= width[l] <= PTG_MLP_MAX_WIDTH
 *   out_dev       float32 [B][O], O = width[n - 1], element (b, j) at b * out_s_n + j, out_s_n >= O, 4-byte aligned
 *   ws_dev        caller-owned device scratch, 4-byte aligned, ws_bytes >= ptg_mlp_workspace(batch, n_layers, width, flags).  The
 *                 activations travel through it between the launches.  With P(w) = w rounded up to a multiple of 4 (rows 16 bytes
 *                 apart or a multiple of that, counted from ws_dev): without PTG_MLP_KEEP_HIDDEN two alternating buffers of
 *                 B * P(widest hidden layer) floats, hidden layer l in buffer l & 1 at byte offset (l & 1) * 4 * B * P(widest); with
 *                 it hidden layer l (l = 0 .. n - 2, post-activation) is [B][width[l]] float32 with row stride P(width[l]) at byte
 *                 offset 4 * B * (P(width[0]) + ... + P(width[l - 1])) -- the tensors a backward pass would read.  16 bytes for n = 1
 * Arithmetic, which is the definition (tests/mlp_restatement.py restates it).  Row b, unit j of a layer with fan-in K, input x, in float32:
 *   acc = bias[j]
 *   for k = 0 .. K - 1 in ascending order:  acc = fmaf(x[b][k], W[j][k], acc)        one rounding per step, subnormals kept
 *   y[b][j] = act(acc):  NONE acc;  RELU acc > 0 ? acc : (acc != acc ? acc : 0) (a NaN stays a NaN, -0 gives +0);  TANH the
 *             double-precision library tanh of the float32 acc, rounded once to float32
 * v_mfma_f32_16x16x4_f32 (four ascending k per instruction) and v_mfma_f32_32x32x2_f32 (two) both realise this chain with the bias as
 * the initial accumulator, so an element's bits do not depend on B, on the row's place in the batch, on the tile route or on the grid;
 * there is no split-K and no atomic.  Padding is exact: in a padded k position both operands are 0 and fmaf(0, 0, acc) = acc, with one
 * exception, fmaf(0, 0, -0) = +0: a result of -0 may come out as +0 (compare with +0 == -0).  The lanes of padded rows, padded units
 * and padded k get 0 (such a lane re-reads an element inside the tensor and discards it: nothing outside a tensor is read) and are never stored.
 * Non-finite values propagate as IEEE 754 dictates, inside their own row only; the op has no error word of its own (ptg_act, which
 * consumes the logits, reports such a row).  float64 networks are out of scope.
 * Enqueues n kernels, k_mlp_layer, with no host synchronisation and no allocation, so the call may be captured into a hipGraph and
 * replayed; the weights are read when the kernels run, so a replay sees an optimiser step or a Polyak update made in place.  Reads
 * nothing of the handle but its device: env state, the finished-episode ring, the ptg_vn_* statistics and every replay cursor are
 * untouched.  Overlap between any two of the buffers is NOT checked; out_dev and ws_dev must not overlap anything the call reads.
 * PTG_E_INVALID (nothing enqueued): NULL handle, descriptor, x_dev, w_dev[l] or b_dev[l] (l < n), out_dev or ws_dev; batch outside
 * [1, 2^31]; n_layers outside [1, PTG_MLP_MAX_LAYERS]; f1 < 1, f2 < 0, f1 + f2 or a width outside [1, PTG_MLP_MAX_WIDTH]; x2_dev with
 * f2 = 0 or f2 > 0 without it; a row stride below its width; an unknown activation code (NONE as hidden_act too); an unknown flag or both
 * route flags; ws_bytes below what ptg_mlp_workspace returns; an out_dev or ws_dev that is not 4-byte aligned.
 * ptg_mlp_workspace(batch, n_layers, widths, flags): bytes of scratch such a call needs, widths = the n_layers layer widths; negative for
 * a NULL widths or a count, width or flag the call would refuse.  PTG_MLP_SPLIT_INPUT is accepted and changes no size.
 * PTG_MLP_SPLIT_INPUT: x_dev is [B][16] float32 PTG_OBS_SPLIT rows, x_s_n >= 16, and the first layer reads the
 * SB3_FLAT row they stand for.  f1 must be that row's width on this handle, 2 P + 14 for 'mod' and P + 18 for 'raw' (P = price_ahead); the
 * fan-in stays f1 + f2 and x2_dev works as before.  Column k < f1 of row b is x[b][c] for one of the 14 env columns c, or
 * series[(int) x[b][14] + q] (a daily series of 'raw': x[b][15]) for column q of a market sub-space, in the column map of ptg_create's
 * SB3_FLAT rows (rl_ptg_amd/policy_split.py restates it: flat_columns, env_columns) over the float32 series of ptg_market_feature_series.
 * Those are the words an SB3_FLAT row holds, read in the same ascending k: THE RESULT OF A SPLIT CALL HAS THE BITS OF THE SAME CALL ON THE
 * REBUILT FLAT ROWS, on either route, single or grouped, forward and backward.  The flag works on any handle, whatever its own obs_layout:
 * the map depends on raw_modified, price_ahead and the series only.  Beyond the device the call reads the handle's series and its error
 * words.  An index is device data and never becomes an address unchecked: the hour index is valid when it is an integer in
 * [0, C_h - P], the day index ('raw' only; 'mod' never reads it) when it is an integer in [0, C_d - 2], C_h and C_d the counts
 * ptg_market_feature_series reports; negative, past the end, fractional, NaN and Inf are invalid.  For an invalid index the load is
 * clamped into the series, the row's market columns read as NaN -- so the row's outputs are NaN; every other row keeps its bits -- and the
 * next ptg_sync (or any call that reports kernel-flagged errors) returns PTG_E_INDEX once.  Further PTG_E_INVALID: f1 not the handle's
 * flat width; x_s_n < 16; market series shorter than one window or longer than 2^24 (indices would not be exact in float32). */
#define PTG_MLP_MAX_LAYERS 10
#define PTG_MLP_MAX_WIDTH 1024
enum { PTG_MLP_RELU = 0, PTG_MLP_TANH = 1, PTG_MLP_NONE = 2 };
enum { PTG_MLP_KEEP_HIDDEN = 1, PTG_MLP_NARROW = 2, PTG_MLP_WIDE = 4 };
enum { PTG_MLP_SPLIT_INPUT = 16 };      /* 8 is PTG_MLP_ACCUMULATE, of ptg_mlp_bwd.flags */
typedef struct ptg_mlp {
    int64_t batch;
    int32_t n_layers, flags;
    int32_t hidden_act, out_act;
    int32_t f1, f2;
    const float* x_dev;
    int64_t x_s_n;
    const float* x2_dev;
    int64_t x2_s_n;
    const float* w_dev[PTG_MLP_MAX_LAYERS];
    int64_t w_s_n[PTG_MLP_MAX_LAYERS];
    const float* b_dev[PTG_MLP_MAX_LAYERS];
    int32_t width[PTG_MLP_MAX_LAYERS];
    float* out_dev;
    int64_t out_s_n;
    void* ws_dev;
    int64_t ws_bytes;
} ptg_mlp;
int64_t ptg_mlp_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags);
int ptg_mlp_forward(ptg_env* env, const ptg_mlp* d, void* stream);

/* ---- the backward pass of an MLP: per layer one launch for the input gradient and one for the weight and bias gradients ----------------
 * Runs after a ptg_mlp_forward call with PTG_MLP_KEEP_HIDDEN and reads what that call left: the hidden layers in its ws_dev, the output
 * in its out_dev.  With it a gradient step is sample -> forward -> loss -> backward -> optimiser on project kernels, with defined bits,
 * no allocation, capturable into a hipGraph.  The call is described by a ptg_mlp_bwd, read during the call and holding no host memory:
 *   fwd           the forward call's ptg_mlp, unchanged (same pointers, strides, widths, batch); it must carry PTG_MLP_KEEP_HIDDEN.  Its
 *                 x_dev / x2_dev, w_dev[l], ws_dev and out_dev are read; b_dev[l] must be non-NULL but is not read
 *   gout_dev      float32 [B][O], O = width[n - 1]: the gradient with respect to the output, element (b, j) at b * gout_s_n + j,
 *                 gout_s_n >= O
 *   dw_dev[l]     float32 [width[l]][in_l], element (j, k) at j * dw_s_n[l] + k, dw_s_n[l] >= in_l: the gradient of w_dev[l];
 *   db_dev[l]     float32 [width[l]] contiguous: the gradient of b_dev[l].  dw_dev[l] and db_dev[l] are both set or both NULL; a NULL pair
 *                 freezes that layer (no k_mlp_dw launch for it); all NULL: no parameter gradients (a critic inside an actor loss)
 *   dx_dev        float32 [B][f1], row stride dx_s_n >= f1, or NULL;  dx2_dev float32 [B][f2], row stride dx2_s_n >= f2, or NULL (it needs
 *                 f2 > 0): the gradient with respect to the input's pieces, each optional (SAC / TD3 / TQC's actor loss wants the
 *                 critic's action piece alone).  Both NULL: the first layer's input-gradient launch is left out
 *   bws_dev       caller-owned device scratch, 4-byte aligned, bws_bytes >= ptg_mlp_backward_workspace(batch, n_layers, width, flags):
 *                 two alternating buffers of B * P(widest of ALL n widths) floats, P as in the forward.  dz of layer l (the gradient at
 *                 its pre-activation) is [B][width[l]] with row stride P(width[l]) at byte offset (l & 1) * 4 * B * P(widest); layer l
 *                 overwrites layer l + 2, so after the call dz of layers 0 and 1 (n >= 2) are what is left.  The last
 *                 layer's dz is stored only when out_act != NONE; with NONE gout_dev is read in place
 *   flags         PTG_MLP_ACCUMULATE: dw_dev / db_dev are added to, not overwritten (below)
 * Arithmetic, which is the definition (tests/mlp_backward_restatement.py restates it).  All float32, one rounding per step, subnormals
 * kept.  Layer l with fan-in K, width O, input x (hidden layer l - 1, or the call's one- or two-piece input), post-activation output h
 * (hidden layer l, or out_dev); g[b][j] the gradient with respect to h[b][j] (gout for the last layer, else dx of the layer above):
 *   dz[b][j]:  NONE g;  RELU h > 0 ? g : (h != h ? g : 0) -- a select, not a product: a NaN g under a dead unit gives 0, a NaN unit
 *              passes g (torch's threshold_backward on the saved output);  TANH t = h * h; u = 1 - t; dz = g * u, three roundings
 *   dx[b][k]:  acc = 0;     for j = 0 .. O - 1 ascending: acc = fmaf(dz[b][j], W[j][k], acc);   dx[b][k] = acc
 *   dW[j][k]:  acc = init;  for b = 0 .. B - 1 ascending: acc = fmaf(dz[b][j], x[b][k], acc);   dW[j][k] = acc
 *   db[j]:     acc = init;  for b ascending: acc = acc + dz[b][j] (= fmaf(dz[b][j], 1, acc): it rides in the dW tile as a column of ones)
 *   init = 0, or with PTG_MLP_ACCUMULATE the value already in dW / db: a call on rows [0, B1) followed by an accumulating call on rows
 *   [B1, B) leaves the bits of one call on [0, B) -- micro-batched gradient accumulation is exact.
 * v_mfma_f32_16x16x4_f32 realises these chains with the accumulator as C (four ascending reduction steps per instruction).  A row's dx
 * depends on nothing outside its own row of dz, so its bits do not depend on B, on the row's place in the batch or on the grid; dW and db
 * depend on B's rows in their order and on nothing else.  No split-K, no atomics.  Padded reduction positions contribute fmaf(0, 0, acc),
 * exact except -0 -> +0 (the forward's rule).  Non-finite values propagate as IEEE 754 dictates: a non-finite dz row reaches every
 * dW[j][.] and db[j] it touches and no other row's dx.
 * Enqueues, serially on the one stream: k_mlp_dz_out when out_act != NONE; then for l = n - 1 .. 0 k_mlp_dw (when dw_dev[l] is set) and
 * k_mlp_dx (for l = 0 only when dx_dev or dx2_dev is set) -- at most 2 n + 1 launches.  No host synchronisation and no allocation; reads
 * nothing of the handle but its device.  Overlap between any two buffers is NOT checked: the outputs and bws_dev must not overlap each
 * other or anything the call reads.
 * PTG_E_INVALID (nothing enqueued): NULL handle or descriptor; anything ptg_mlp_forward refuses in fwd; fwd without
 * PTG_MLP_KEEP_HIDDEN; NULL gout_dev or gout_s_n below the output width; dw_dev[l] without db_dev[l] or the reverse (l < n); dw_s_n[l]
 * below the fan-in; dx_s_n below f1; dx2_dev with f2 = 0 or dx2_s_n below f2; an unknown flag; NULL or misaligned bws_dev; bws_bytes
 * below what ptg_mlp_backward_workspace returns.
 * ptg_mlp_backward_workspace(batch, n_layers, widths, flags): 8 * batch * P(widest width) bytes; negative for a NULL widths or a count,
 * width or flag the call would refuse (flags: the backward's own, so PTG_MLP_SPLIT_INPUT, a flag of fwd, is refused here).
 * With PTG_MLP_SPLIT_INPUT in fwd.flags the weight and bias gradients of the first layer read the rebuilt flat row as the forward does
 * (an invalid index: NaN in that row's products, PTG_E_INDEX); dx_dev must be NULL -- an observation has no gradient -- and a non-NULL
 * one is PTG_E_INVALID; dx2_dev works as before.  The backward's own flags know no PTG_MLP_SPLIT_INPUT. */
enum { PTG_MLP_ACCUMULATE = 8 };
typedef struct ptg_mlp_bwd {
    ptg_mlp fwd;
    const float* gout_dev;
    int64_t gout_s_n;
    float* dw_dev[PTG_MLP_MAX_LAYERS];
    int64_t dw_s_n[PTG_MLP_MAX_LAYERS];
    float* db_dev[PTG_MLP_MAX_LAYERS];
    float* dx_dev;
    int64_t dx_s_n;
    float* dx2_dev;
    int64_t dx2_s_n;
    void* bws_dev;
    int64_t bws_bytes;
    int32_t flags, reserved;
} ptg_mlp_bwd;
int64_t ptg_mlp_backward_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags);
int ptg_mlp_backward(ptg_env* env, const ptg_mlp_bwd* d, void* stream);

/* ---- a group of MLPs of equal depth in the launches of one: twin critics, critics and their targets, a policy and a value net ----------
 * ptg_mlp_group_forward and ptg_mlp_group_backward run n_nets networks, 1 <= n_nets <= PTG_MLP_GROUP_MAX, in exactly the launches that
 * ONE network's ptg_mlp_forward / ptg_mlp_backward enqueues: n in the forward; in the backward k_mlp_dz_out when out_act != NONE, then
 * per layer one weight-gradient and one input-gradient launch (kernels k_mlp_layer_group, k_mlp_dz_out_group, k_mlp_dw_group,
 * k_mlp_dx_group: the third grid dimension is the network, the first two are the largest tile counts of the group).  A weight-gradient
 * launch of layer l is enqueued when ANY network sets dw_dev[l], the first layer's input-gradient launch when ANY network sets dx_dev
 * or dx2_dev; the workgroups of a network that freezes the layer, or wants no dx, return at once and write nothing.
 *   nets          an array of n_nets of the single calls' descriptors, read during the call and holding no host memory afterwards.  Each
 *                 network has its own x_dev / x2_dev (f1 and f2 may differ), width[], w_dev / b_dev, out_dev, ws_dev, and in the backward
 *                 its own gout_dev, dw_dev / db_dev (frozen layers per network), dx_dev / dx2_dev (each optional per network), bws_dev.
 *                 Workspace sizes are ptg_mlp_workspace and ptg_mlp_backward_workspace, per network.
 *   sharing       networks may share what is only read: x_dev, x2_dev, even weights.  Every out_dev, ws_dev, gradient and bws_dev of
 *                 every network must be distinct from every other and from anything the call reads; overlap is NOT checked.
 *   must agree    batch, n_layers, hidden_act, out_act and flags (PTG_MLP_SPLIT_INPUT among them) of all networks; in the backward its own flags (PTG_MLP_ACCUMULATE) too.
 *   routes        a group always runs the 16 x 16 route: PTG_MLP_WIDE in any descriptor is refused, PTG_MLP_NARROW is accepted and means
 *                 nothing.  A single network at a large batch (B >= 4 096 with layers wider than 512) belongs to ptg_mlp_forward and its
 *                 128 x 128 route.
 * Arithmetic: none of its own.  EVERY ELEMENT A GROUPED CALL WRITES IS DEFINED AS WHAT THE SINGLE CALL ON THAT NETWORK'S DESCRIPTOR WRITES
 * -- out, the kept hidden layers, dx, dW, db and the dz left in bws_dev -- bit for bit: an element of the single ops does not depend on
 * the grid, and the grouped kernels run the single kernels' tile code.  A shared input's gradient is NOT summed: each network writes its
 * own dx.
 * No host synchronisation and no allocation; capturable into a hipGraph; the weights are read when the kernels run.
 * PTG_E_INVALID (nothing enqueued; every check runs before the first launch): NULL handle or array; n_nets outside
 * [1, PTG_MLP_GROUP_MAX]; anything the single call refuses in a descriptor, its text behind "net <i>: "; PTG_MLP_WIDE; a disagreement
 * in one of the fields above, which names the two networks and the field. */
#define PTG_MLP_GROUP_MAX 8
int ptg_mlp_group_forward(ptg_env* env, const ptg_mlp* nets, int32_t n_nets, void* stream);
int ptg_mlp_group_backward(ptg_env* env, const ptg_mlp_bwd* nets, int32_t n_nets, void* stream);

/* ---- the PPO / A2C loss and the optimiser step of up to eight independent agents in the launches of one: seeds, sweeps ------------------
 * ptg_policy_loss_group and ptg_optim_step_group run n_members descriptors, 1 <= n_members <= PTG_TRAIN_GROUP_MAX, of the single calls
 * (ptg_loss, ptg_optim, unchanged) in exactly the launches that ONE ptg_policy_loss / ptg_optim_step enqueues.  The descriptors are read
 * during the call and travel by value in the launch arguments -- eight ptg_loss members take 8 x 208 = 1 664 bytes, eight ptg_optim
 * members 8 x 136 = 1 088 bytes of the 4 096 bytes of kernel arguments a launch may have -- so a captured call holds no host memory.
 * ptg_policy_loss_group:
 *   must agree    kind, head, flags, n_actions, in_dtype, act_kind and batch of all members.
 *   its own       every pointer and stride; clip_range, clip_range_vf, ent_coef, vf_coef; stats_dev, ws_dev (ptg_policy_loss_workspace(batch)
 *                 bytes each), the gradient outputs and log_std_dev.
 *   launches      those of the single call for that batch and those flags: one for batch <= 256 (k_pl_rows); beyond that the rows and
 *                 the final merge (k_pl_rows, k_loss_final), with two more in front for the advantage moments under PTG_LOSS_NORM_ADV
 *                 (k_pl_moments, k_pl_merge_group) -- the single call's kernels instantiated over the group's arguments.  The member is
 *                 a grid dimension.
 *   arithmetic    none of its own: a grouped kernel is the single kernel's text on the member its block index names, every member's sums run in the single
 *                 call's order, which depends on batch alone, and nothing is reduced across members.  MEMBER i's stats, grad_in, grad_val
 *                 AND grad_log_std ARE DEFINED AS WHAT ptg_policy_loss(&members[i]) WRITES, bit for bit.
 * ptg_optim_step_group:
 *   must agree    kind, flags and dtype of all members.
 *   its own       the two tables, n_tensors, n_chunks; state_dev, lr_dev (NULL or not, per member), norm_dev, ws_dev
 *                 (ptg_optim_workspace(n_chunks) bytes of that member); lr, beta1, beta2, eps, alpha, tau, max_norm.
 *   launches      three (k_optim_norm, k_optim_head, k_optim_update, instantiated over the group's arguments), two without
 *                 PTG_OPTIM_CLIP, one for PTG_OPTIM_POLYAK, whatever n_members is.  The norm pass and the update run on a grid of (the largest n_chunks of the
 *                 group) x n_members workgroups: a workgroup owns one chunk of one member, and the surplus workgroups of a member with
 *                 fewer chunks leave at once.  The head kernel runs one workgroup per member.
 *   arithmetic    none of its own.  Each member keeps its own total norm and clip coefficient, its own step count and running products and
 *                 its own partials in its own ws_dev, added in the order of its own tables: MEMBER i's PARAMETERS, STATES, TARGETS,
 *                 GRADIENTS (PTG_OPTIM_ZERO_GRAD), state_dev AND norm_dev AFTER THE CALL ARE DEFINED AS THOSE AFTER
 *                 ptg_optim_step(&members[i]), bit for bit.
 * Members may share what is only read (an observation batch's columns, lr_dev).  Every output and scratch buffer of every member must be
 * distinct from every other member's and from anything the call reads; two members with EQUAL stats_dev, ws_dev, grad_in_dev or
 * grad_val_dev (the loss), state_dev, norm_dev or ws_dev (the optimiser) are refused, overlap beyond equal base pointers is NOT checked.
 * The two error words of the handle are shared: a bad row or span in member i, or a non-finite norm in member i, raises the word as the
 * single call does (the next ptg_sync returns PTG_E_INDEX or PTG_E_NONFINITE once) and changes nothing in any other member's outputs.
 * No host synchronisation and no allocation; capturable into a hipGraph.
 * PTG_E_INVALID (nothing enqueued, every output untouched; every check runs before the first launch): NULL handle or members;
 * n_members outside [1, PTG_TRAIN_GROUP_MAX]; anything the single call refuses in a descriptor, the single call's text behind
 * "member <i>: " (one checker serves both entries); a disagreement in one of the fields above, which names the field and the two
 * members; two members that share one of the output or scratch pointers above.
 * Not grouped: the gSDE and quantile losses; the minibatch gathers; members of different batch.  The TD and actor
 * losses and the training-time actor head have grouped entries of their own, below. */
#define PTG_TRAIN_GROUP_MAX 8
int ptg_policy_loss_group(ptg_env* env, const ptg_loss* members, int32_t n_members, void* stream);
int ptg_optim_step_group(ptg_env* env, const ptg_optim* members, int32_t n_members, void* stream);

/* ---- the off-policy losses and the actor head of up to eight independent agents in the launches of one ---------
 * ptg_td_loss_group, ptg_actor_loss_group, ptg_rsample_group and ptg_rsample_backward_group run n_members descriptors, 1 <= n_members <=
 * PTG_TRAIN_GROUP_MAX, of the single calls (ptg_td, ptg_al, ptg_rs, unchanged) in exactly the launches that ONE single call enqueues,
 * whatever n_members is.  The descriptors are read during the call and travel by value in the launch arguments -- eight members take
 * 8 x 328 = 2 624 (td), 8 x 232 = 1 856 (actor loss) and 8 x 176 = 1 408 bytes (rsample) of the 4 096 a launch may have -- so a captured
 * call holds no host memory.  The member is a grid dimension; a grouped kernel is the single kernel's text on the member its block index
 * names, every member's sums run in the single call's order, which depends on batch alone, and nothing is reduced across members:
 * WHAT MEMBER i's OUTPUTS HOLD AFTER A GROUPED CALL IS DEFINED AS WHAT THE SINGLE CALL ON &members[i] WRITES, bit for bit.
 * ptg_td_loss_group:
 *   must agree    kind, flags, n_actions, n_critics, q_dtype, rew_dtype, done_dtype, act_kind and batch.
 *   its own       every pointer and stride; gamma, alpha, alpha_dev (NULL or not, where the flags allow either), scale; y_dev (NULL or not).
 *   distinct      stats_dev, ws_dev, y_dev, and every grad_q_dev entry against every entry of every other member.
 *   launches      one for batch <= 256 (k_td_rows), else the rows and the final merge (k_td_rows, k_loss_final: one workgroup a member).
 * ptg_actor_loss_group:
 *   must agree    kind, flags, n_critics, n_quantiles, q_dtype and batch.
 *   its own       every pointer and stride; alpha, alpha_dev, target_entropy; grad_logp_dev and grad_log_alpha_dev (NULL or not).
 *   distinct      stats_dev, ws_dev, every grad_q_dev entry, grad_logp_dev, grad_log_alpha_dev.
 *   launches      one for batch <= 256 (k_al_rows), else the rows and the final merge.
 * ptg_rsample_group / ptg_rsample_backward_group:
 *   must agree    kind, flags, q_dtype and batch.
 *   its own       every pointer and stride; seed and counter_dev; noise_std, noise_clip, clip_lo, clip_hi.
 *   distinct      forward: act_dev, logp_dev, noise_dev and -- unless deterministic -- counter_dev: the grouped forward reads every
 *                 counter before any of them is advanced, which n_members calls in turn on one counter would not; backward: the two
 *                 gradient outputs.
 *   launches      forward: k_rs_fwd and one launch that advances every member's counter by one (one thread a member), or k_rs_fwd alone
 *                 when deterministic; backward: one.
 * Members may share what is only read.  Two members with EQUAL base pointers in one of the `distinct` fields are refused; overlap beyond
 * equal base pointers is NOT checked.  The error words of the handle are shared: a bad row in member i raises the word as the single
 * call does (the next ptg_sync returns PTG_E_INDEX or PTG_E_NONFINITE once) and changes nothing in any other member's outputs.
 * No host synchronisation and no allocation; capturable into a hipGraph.
 * PTG_E_INVALID (nothing enqueued, every output untouched; every check runs before the first launch): NULL handle or members;
 * n_members outside [1, PTG_TRAIN_GROUP_MAX]; anything the single call refuses in a descriptor, the single call's text behind
 * "member <i>: " (one checker serves both entries); a disagreement in one of the fields above, which names the field and the two
 * members; two members that share one of the pointers above.
 * Not grouped: ptg_quantile_loss, the gSDE ops, the replay buffer's add and sample, members of different batch. */
int ptg_td_loss_group(ptg_env* env, const ptg_td* members, int32_t n_members, void* stream);
int ptg_actor_loss_group(ptg_env* env, const ptg_al* members, int32_t n_members, void* stream);
int ptg_rsample_group(ptg_env* env, const ptg_rs* members, int32_t n_members, void* stream);
int ptg_rsample_backward_group(ptg_env* env, const ptg_rs* members, int32_t n_members, void* stream);

/* The pre-normalised float32 market feature series the kernels read, as [n_sets][series length]: which = 0 Pot_Reward ('raw':
 * Elec_Price) hourly, 1 Part_Full hourly ('mod' only), 2 Gas_Price daily, 3 EUA_Price daily.  out_host NULL: only *count.
 * For the SPLIT layout's consumer (column 14 / 15 of a row index these arrays). */
int ptg_market_feature_series(ptg_env* env, int which, float* out_host, int cap, int* count);

/* diagnostics for tests: the device-built lookup products */
int ptg_debug_get_index_lut(ptg_env* env, double* T_values_host, int32_t* lut_host /*[6][nT]*/, int* n_T);
int ptg_debug_window_record(ptg_env* env, int table_id, int start_row, double* out7_host /*T_last, 5 means, key*/);
/* what the tables made of the handle (read-only): {16-bit lookup copy exists, the fused rollout keeps it in LDS, nT, key of the initial
 * temperature, reset row of cooldown, key_cold_max, key_hot_min, key_standby_max} */
int ptg_debug_table_plan(ptg_env* env, int32_t* out8_host);

#ifdef __cplusplus
}
#endif
#endif /* PTG_ENV_H */
