// ptg_handle.h -- internal to libptg_env.so: what ptg_env.hip (the environment) and ptg_train.hip (the training ops) both use.
// The device data that a handle embeds, the handle itself, and the host helpers of an entry point.  Included by those two files and
// nothing else.  The types live in an anonymous namespace, so every translation unit has its own copy, as the parts of the parallel
// build always had.
#ifndef PTG_HANDLE_H
#define PTG_HANDLE_H

#include "../../include/ptg_env.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------------ device data
struct alignas(64) Rec {      // one window start: 64 B = half an L2 line, never straddles a line
    double T;                 // catalyst temperature of the window's last row (:452)
    double m[5];              // np.average of n_h2, n_ch4, n_h2_res, m_h2o, P_el over the window (:454-458)
    int tkey;                 // index of T in the sorted distinct-temperature list
    int pad;
    double spare;
};
static_assert(sizeof(Rec) == 64, "Rec must be 64 bytes");

// Strength-reduced record of the float32 fast path.  The reward (:280-334) is linear in the three prices once the
// window is fixed: rew = base + ch4*(b_s3*k_chp + k_eua*eua) + c_gas*gas - c_el*el, and the electrolyzer efficiency
// polynomial (:311-317) depends on the window only -- so k_build_fast evaluates it once per window start.
struct alignas(64) RecFast {
    double base, ch4, c_gas, c_el;   // all pre-multiplied by sim_step/3600 except ch4 (raw mean methane flow)
    float feat[6];                   // normalised T_cat, H2, CH4, H2_res, H2O, el_heating (:212-217)
    int tkey;
    int pad;
};
static_assert(sizeof(RecFast) == 64, "RecFast must be 64 bytes");

// Per-env state, three arrays of naturally aligned structs (16-B / 16-B / 8-B lanes -> dwordx4 / dwordx2 accesses)
struct alignas(16) StA { int i, j, k; unsigned flags; };   // flags: [0:3) meth_state [3] hot_cold [4] standby=up [5] startup=hot
                                                            // [6:9) part_op [9:12) full_op [12:15) current_action [15:17) market set [17:32) T key
struct alignas(16) StB { double cum; int act_d; int nctr; };   // cum_rew (:330), act_ep_d (:61,492), noise draws consumed so far
struct alignas(8) StC { int nchg; int epp; };                  // state changes this episode (tracked when the penalty is on), pointer into
                                                               // eps_ind -- touched on penalised state changes / resets only

struct Regs {
    StA a; StB b; StC c;
    bool c_loaded, c_dirty;
};

struct DevParams {
    int fm_pitch;                // feature-major outputs: elements between two feature planes (>= N; ptg_set_feature_pitch)
    int N, S, sim_step, eps_sim_steps, PA, F, mod, eps_len_d;
    int E, ep_stride;                      // eps_ind length (0 = eval env), pointer stride (mod E)
    int noise_inline, track_changes;       // draw noise from the counter RNG in the kernel; maintain StC.nchg (penalty != 0)
    unsigned long long noise_seed;
    long long env_offset;                  // global index of env 0 of this shard (keys the RNG streams)
    double noise_sigma;
    int key_cold_max, key_hot_min, key_standby_max, key_init, i_reset, nT, tape_len;
    int n_hours, n_days, hstride, dstride;
    int t1_start_p_f, t2_start_f_p, t_p_f, t_f_p, t1_p_f_p, t2_p_f_p, t3_p_f_p, t34_p_f_p, t4_p_f_p, t45_p_f_p,
        t5_p_f_p, t1_f_p_f, t2_f_p_f, t23_f_p_f, t3_f_p_f, t34_f_p_f, t4_f_p_f, t45_f_p_f, t5_f_p_f, i_full, j_full;
    // reward / normalisation constants (:280-334, :206-217)
    double c_mol, Hu_ch4, Hu_h2, dt_cp_evap, heat_price, o2_price, eeg, eta_chp, one_m_eta_chp, M_co2, M_h2o,
           rho, water_price, min_load, max_h2, c_m2, c_m3, sim_step_d;
    double T_lo, T_rng, h2_lo, h2_rng, ch4_lo, ch4_rng, h2r_lo, h2r_rng, h2o_lo, h2o_rng, heat_lo, heat_rng;
    double reset_flow[5], T_init;
    double k_chp, k_eua;                   // fast path: per-unit-CH4 CHP revenue and EUA revenue factors (x sim_step/3600)
    // tables
    const Rec* rec;
    const RecFast* recf;
    const int2* tabmeta;                   // [17] {rows, record base}
    const int* argidx;                     // [6][nT]
    const double* Tvals;                   // [nT]
    const double* tape;                    // [tape_len][N] (draw-major, see k_fill_noise)
    const int* eps_ind;                    // [E]
    const double2* sincos;                 // [eps_sim_steps + 1]
    const float2* sincos32;
    // market, [set][...] with strides hstride / dstride
    const double *el, *featA, *featB, *gas, *eua, *gas_n, *eua_n;
    const float *featA32, *featB32, *gas_n32, *eua_n32;
    const double *pot_raw, *pf_raw;        // un-normalised pot_rew / part_full for info rows
    const double2* setc;                   // [sets] {b_s3, r_0 * state_change_penalty}
    // state
    StA* st_a; StB* st_b; StC* st_c;
    // finished-episode list
    double* fin_ret; int* fin_len; int* fin_env; int* fin_count; int fin_cap;
    const int* cmap; int q_stat;          // SB3_FLAT layout: canonical column -> flat column; canonical index of METH_STATUS (else cmap = null)
    int split;                            // SPLIT layout (16 columns: status one-hot, 8 env features, hour / day series index; q_stat set too)
    int* err;                             // [6] in pinned HOST memory: {invalid action seen, price index out of range, hot kernel on the
                                          // terminating step, replay on a de-synchronised batch, minibatch / replay sample index out of range,
                                          // action head met a non-finite row} (check_error_flags); kernels store 1 (plain
                                          // stores of a constant need no atomic), the host reads it after a stream synchronise -- no copy
    int* term_flag;                       // device word: "the hot step kernel of this (captured) step found the batch on the terminating step
                                          // and skipped it" -- written by k_step_hot, read by the k_step enqueued behind it
};

// the 32-bit integer finaliser that the counter-based device RNGs chain (noise_draw in ptg_env.hip, rb_draw_word in ptg_train.hip)
__device__ __forceinline__ unsigned lowbias32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

}  // namespace

struct ptg_env {
    ptg_config cfg;
    int n = 0, device = 0, n_sets = 0, F = 0, S = 0;
    bool reset_done = false;
    DevParams P;
    std::vector<void*> allocs;
    std::vector<double> Tvals;
    std::vector<int> tab_rows, rec_base;
    size_t rec_total = 0;
    bool fast = false, fm = false, flat = false, split = false;
    double* d_tape = nullptr;
    unsigned short* d_lut16 = nullptr;
    unsigned short* d_rkey = nullptr;   // temperature keys of all window records (k_rollout_pc producers)
    float* d_pool32 = nullptr; double* d_pool64 = nullptr;
    unsigned off_featB = 0, off_gasn = 0, off_euan = 0, off_gas = 0, off_eua = 0, off_sc = 0;
    unsigned o64_featA = 0, o64_featB = 0, o64_gasn = 0, o64_euan = 0, o64_sc = 0;
    std::vector<float> pool32_host;
    std::vector<double> pool64_host;
    int* d_ladder = nullptr;
    int sync_k = -1;             // common step count k of all envs when the batch is known to be synchronised, else -1
    int step_skip_term = 0;      // argument of the next k_step_hot launch: 1 while ptg_step is being captured (see ptg_step)
    int replay_proof = 0;        // ptg_set_replay_proof: a captured ptg_step is enqueued as hot kernel + predicated generic kernel
    // VecNormalize reward normalisation (ptg_vn_*): per-env discounted returns, running (mean, var, count), scratch
    double *vn_returns = nullptr, *vn_stats = nullptr, *vn_partials = nullptr, *vn_den = nullptr, *vn_moments = nullptr;
    size_t vn_partials_cap = 0; int vn_T_cap = 0;
    double vn_gamma = 0.99, vn_eps = 1e-8, vn_clip = 10.0;
    bool fin_maybe = false;      // a generic step ran since the last ptg_finished_episodes: only those can finish episodes
    void* fin_stage = nullptr; size_t fin_stage_bytes = 0;      // pinned staging of ptg_finished_episodes
    unsigned long long fin_dropped = 0;      // finished episodes never handed out: ring overflow, or a query whose cap was too small
    int tape_len = 0;
    double *d_pot_raw = nullptr, *d_pf_raw = nullptr;
    int* d_eps_ind = nullptr;
    // experiment knobs, read from the environment ONCE in ptg_create (PTG_NO_HOT_KERNELS, PTG_NO_LDS_LUT, PTG_NO_REFRESH, PTG_REFRESH_ALWAYS, PTG_PC_CHUNK, PTG_BLOCK)
    bool knob_no_hot = false, knob_no_lds_lut = false, knob_no_refresh = false, knob_refresh_always = false;
    int front_horizon = 0;       // steps after a synchronised reset during which the table refresher keeps rolling (k_refresh)
    hipStream_t ref_stream = nullptr;
    hipEvent_t ev_fork = nullptr;        // the refresher's stream is forked from the caller's
    double unrefreshed_bytes = 1e18;      // written by this handle's kernels since the tables were last re-read (first launch: refresh)
    int n_cu = 256;
    std::vector<const void*> attr_done;   // kernels whose dynamic-LDS limit has been raised on this handle's device
    int* err_host = nullptr;     // DevParams::err as the host sees it
    int* d_desync = nullptr;     // HotParams::desync: sync_k < 0 as the device sees it (set_desync)
    // ptg_step_host: device staging for batches too large for zero-copy, and the classification of the caller's buffers
    void *hs_act = nullptr, *hs_out = nullptr, *hs_final = nullptr; double* hs_info = nullptr;
    struct HostStep {            // a ptg_step_host call between its phases (begin .. tail .. end)
        bool active = false, zc = false, tail_done = false;
        void* out_host = nullptr; void* final_host = nullptr; double* info_host = nullptr;
        hipStream_t st = nullptr;
        int n_done = 0;
    } hs;
    int status_col_flat = 5;           // SB3_FLAT rows: first of the six one-hot METH_STATUS columns (ptg_create, from the column map)
    hipEvent_t ev_tail = nullptr;      // recorded behind the copy of [rewards | done flags | status] (+ info rows): the part the caller needs first
    struct HostPtr { const void* host = nullptr; void* dev = nullptr; };      // dev == nullptr: not device-mapped (pageable, or not host memory)
    HostPtr hs_map[8]; int hs_next = 0;      // classification of the caller's buffers by address: a small round-robin cache (a VecEnv rotates 4 blocks)
    int knob_chunk = 65536, knob_block = 0;
    // per-launch timing (ptg_profile): kernel-attached start / stop events of the launches since profiling was switched on
    double* rollout_info = nullptr;   // set by ptg_rollout_info around its hot launches: the [T][N][24] info matrix (float64 kernels only)
    bool profiling = false;
    struct ProfRec { hipEvent_t e0 = nullptr, e1 = nullptr, h0 = nullptr, h1 = nullptr; };      // the launch's events; its helper's (k_refresh), if any
    std::vector<ProfRec> prof_used;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_free;
    std::string err;
};

// The error text of a call: into the handle, or (null handle) into the thread's slot that ptg_last_error(NULL) reads.  One
// definition, in part 0 of ptg_env.hip; hidden like the launchers of ptg_hot.
__attribute__((visibility("hidden"))) int set_err(ptg_env* h, int code, const char* fmt, ...);

namespace {

#define HIP_TRY(h, call)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return set_err(h, PTG_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int dev_alloc(ptg_env* h, T** p, size_t count)
{
    void* q = nullptr;
    HIP_TRY(h, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    h->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

inline int grid_for(long long n, int block) { return (int)((n + block - 1) / block); }

int launch_check(ptg_env* h, const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(h, PTG_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

hipStream_t as_stream(void* s) { return (hipStream_t)s; }

}  // namespace

#endif
