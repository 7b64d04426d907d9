// ptg_train.hip -- the training-side operations of include/ptg_env.h (rl_ptg_amd/train_ops.py): HIP kernels + C ABI.  They read
// and write the caller's rollout buffers and step no environment; of a handle they use n, device, cfg.out_dtype, P.err, P.env_offset
// and the vn_* members (ptg_handle.h).  One translation unit of its own beside the parts of ptg_env.hip.
//
// What replaces what:
//   k_vn_*            VecNormalize(norm_obs=False) reward normalisation over the [T][N] rewards.
//   k_gae             SB3's RolloutBuffer.compute_returns_and_advantage (GAE) over the [T][N] rewards, values and done flags.
//   k_minibatch       SB3's RolloutBuffer.get / _get_samples: one shuffled minibatch gathered from the [T][N] buffers of a rollout.
//   k_rb_*            SB3's ReplayBuffer.add / sample over caller-owned rings on the device (the off-policy algorithms).
//   k_act             the action head while collecting: SB3's Categorical sample / log_prob / entropy, DQN's epsilon-greedy, the Gaussian heads.
//   k_pl_*            the PPO / A2C loss of a minibatch, SB3's logged statistics and the gradients w.r.t. the network's outputs in one pass.
//   k_sde_*           gSDE (SB3's StateDependentNoiseDistribution): the exploration matrix, the collecting head, the PPO / A2C loss; k_sde_rs_*: SAC / TQC's squashed head and its backward.
//   k_optim_*         clip_grad_norm_, torch.optim.Adam / RMSprop, SB3's polyak_update and zero_grad over all tensors of an optimiser.
//   k_td_*            the TD loss of DQN / the TD3 and SAC critics on a replay batch, its statistics and the gradients w.r.t. the Q-values.
//   k_ql_*            TQC's quantile-Huber critic loss on a replay batch, its statistics and the gradients w.r.t. the current quantiles.
//   k_rs_*            SB3's Actor.action_log_prob on a replay batch (SAC / TQC), forward and backward, and TD3's target-policy smoothing.
//   k_al_*            the SAC / TQC / TD3 actor loss and the entropy-coefficient loss with their gradients.
// Built with -ffp-contract=off: the float64 expressions keep the reference's operand order.
#include "ptg_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <type_traits>

namespace {

// ================================================================================== VecNormalize reward normalisation
// stable-baselines3 2.0.0a13 (the reference's pin, requirements.txt:5; un-vendored), vec_env/vec_normalize.py + running_mean_std.py,
// as the reference uses it: VecNormalize(env, norm_obs=False) (src/rl_utils.py:453).  Per vector step:
//   returns = returns * gamma + reward;  ret_rms.update(returns)   [batch mean / population variance over the envs, merged into
//   the running moments];  reward_out = clip(reward / sqrt(ret_rms.var + epsilon), +-clip_reward);  returns[done] = 0.
// Over a [T][N] reward matrix that is: a per-env recurrence with per-step moments over the envs (k_vn_moments, k_vn_merge), a
// T-step scalar scan of the running moments (k_vn_scan) and an elementwise pass (k_vn_norm).  Moments travel as
// (count, mean, M2) and are merged with Chan's formula -- across waves here, across GPUs in rl_ptg_amd/dist.py.
__device__ __forceinline__ void chan_merge(double& ca, double& ma, double& Ma, double cb, double mb, double Mb)
{
    if (cb == 0.0) return;
    if (ca == 0.0) { ca = cb; ma = mb; Ma = Mb; return; }
    const double tot = ca + cb, delta = mb - ma;
    ma = ma + delta * cb / tot;
    Ma = Ma + Mb + delta * delta * ca * cb / tot;
    ca = tot;
}

// Per-env recurrence + per-step moments of every wave (one wave per workgroup).  Cross-lane reductions per step would
// dominate (a float64 butterfly is 12 dependent ds_bpermute or DPP stages: measured 0.33-0.46 us per step at one wave per SIMD),
// so the work is transposed instead: for 64 steps at a time lane e runs the recurrence of ITS env and parks the 64 returns in
// an LDS tile [step][env]; then lane t sums row t -- the moments of step t over the wave's envs -- in a private loop (two
// passes: mean, then squared deviations) and writes that step's partial.  No cross-lane instruction at all.
template <typename OUT>
__global__ void __launch_bounds__(64)
k_vn_moments(const OUT* __restrict__ rew, const uint8_t* __restrict__ done, int N, int T, double gamma, double* __restrict__ returns,
             double* __restrict__ partials, int nW)
{
    constexpr int TS = 64, PITCH = 65;                      // 65: row t starts 2 banks after row t-1
    __shared__ double tile[TS * PITCH];
    const int lane = threadIdx.x, w = blockIdx.x;           // w = wave index = workgroup index
    const int e_raw = w * 64 + lane;
    const bool live = e_raw < N;
    const int e = live ? e_raw : N - 1;
    const int n_live = min(64, N - w * 64);
    double ret = live ? returns[e] : 0.0;
    for (int t0 = 0; t0 < T; t0 += TS) {
        const int nt = min(TS, T - t0);
        for (int tb = 0; tb < nt; tb += 8) {                // recurrence, loads batched eight steps at a time
            OUT r[8]; uint8_t d[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const size_t g = (size_t)(t0 + min(tb + j, nt - 1)) * N + e;
                r[j] = rew[g]; d[j] = done[g];
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (tb + j < nt) {
                    ret = ret * gamma + (double)r[j];       // _update_reward
                    tile[(tb + j) * PITCH + lane] = ret;
                    ret = d[j] ? 0.0 : ret;                 // self.returns[dones] = 0
                }
            }
        }
        __syncthreads();
        if (lane < nt) {                                    // lane t: moments of step t0 + t over this wave's envs
            const double* row = tile + lane * PITCH;
            double s = 0.0;
            for (int q = 0; q < n_live; q++) s += row[q];
            const double mean = s / (double)n_live;         // np.mean
            double m2 = 0.0;
            for (int q = 0; q < n_live; q++) { const double dv = row[q] - mean; m2 += dv * dv; }
            double* p = partials + ((size_t)(t0 + lane) * nW + w) * 3;
            p[0] = (double)n_live; p[1] = mean; p[2] = m2;
        }
        __syncthreads();
    }
    if (live) returns[e] = ret;
}

// one wave merges the nW partials of step t into moments[3 t ..]: k_vn_merge's body, and k_pl_merge_group's per member (t = 0)
__device__ __forceinline__ void vn_merge_step(const double* __restrict__ partials, int nW, double* __restrict__ moments, int t)
{
    const int lane = threadIdx.x;
    double c = 0.0, m = 0.0, M = 0.0;
    for (int w = lane; w < nW; w += 64) {
        const double* p = partials + ((size_t)t * nW + w) * 3;
        chan_merge(c, m, M, p[0], p[1], p[2]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double cb = __shfl_xor(c, off, 64), mb = __shfl_xor(m, off, 64), Mb = __shfl_xor(M, off, 64);
        // both partners must end with the same value: merge in a fixed (lower lane first) order
        double ca = c, ma = m, Ma = M;
        if (lane & off) { double tc = cb, tm = mb, tM = Mb; chan_merge(tc, tm, tM, ca, ma, Ma); c = tc; m = tm; M = tM; }
        else { chan_merge(ca, ma, Ma, cb, mb, Mb); c = ca; m = ma; M = Ma; }
    }
    if (lane == 0) { moments[t * 3 + 0] = c; moments[t * 3 + 1] = m; moments[t * 3 + 2] = M; }
}

__global__ void __launch_bounds__(64)
k_vn_merge(const double* __restrict__ partials, int nW, double* __restrict__ moments)
{
    vn_merge_step(partials, nW, moments, blockIdx.x);
}

// RunningMeanStd.update_from_moments over the T steps of a launch; den[t] = sqrt(var + epsilon) AFTER the update of step t
// (step_wait updates before it normalises).  update_from_moments IS Chan's merge of (count, mean, var * count), which is
// associative: one wave runs it as a prefix scan (per-lane chunks of the steps, a 6-stage scan of the lane totals, then the
// chunks again) -- a chain of ~2 T / 64 + 6 merges instead of T, each a float64 division.  training == 0: frozen statistics.
__global__ void __launch_bounds__(64)
k_vn_scan(const double* __restrict__ moments, int T, int training, double epsilon, double* __restrict__ stats, double* __restrict__ den)
{
    const int lane = threadIdx.x;
    const double mean0 = stats[0], var0 = stats[1], count0 = stats[2];
    const int chunk = (T + 63) / 64, t_lo = min(T, lane * chunk), t_hi = min(T, t_lo + chunk);
    if (!training) {
        for (int t = t_lo; t < t_hi; t++) den[t] = sqrt(var0 + epsilon);
        return;
    }
    double c = 0.0, m = 0.0, M = 0.0;                       // this lane's chunk, merged
    for (int t = t_lo; t < t_hi; t++) chan_merge(c, m, M, moments[t * 3 + 0], moments[t * 3 + 1], moments[t * 3 + 2]);
    double ic = c, im = m, iM = M;                          // inclusive scan over the lanes (earlier steps first)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double pc = __shfl_up(ic, off, 64), pm = __shfl_up(im, off, 64), pM = __shfl_up(iM, off, 64);
        if (lane >= off) { chan_merge(pc, pm, pM, ic, im, iM); ic = pc; im = pm; iM = pM; }
    }
    double rc = __shfl_up(ic, 1, 64), rm = __shfl_up(im, 1, 64), rM = __shfl_up(iM, 1, 64);      // exclusive prefix
    if (lane == 0) { rc = 0.0; rm = 0.0; rM = 0.0; }
    double qc = count0, qm = mean0, qM = var0 * count0;     // running moments before this lane's first step
    chan_merge(qc, qm, qM, rc, rm, rM);
    for (int t = t_lo; t < t_hi; t++) {
        chan_merge(qc, qm, qM, moments[t * 3 + 0], moments[t * 3 + 1], moments[t * 3 + 2]);
        den[t] = sqrt(qM / qc + epsilon);
    }
    if (lane == 63) { stats[0] = qm; stats[1] = qM / qc; stats[2] = qc; }      // lane 63's prefix + chunk = all T steps
}

template <typename OUT>
__global__ void __launch_bounds__(256)
k_vn_norm(const OUT* __restrict__ rew, OUT* __restrict__ out, const double* __restrict__ den, int N, size_t total, double clip)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const double v = (double)rew[g] / den[g / (size_t)N];
    const double lo = v < -clip ? -clip : v;                // np.clip: compare-selects that fall through to v, so a NaN stays
    out[g] = (OUT)(lo > clip ? clip : lo);                  // NaN (fmax(NaN, x) would be x)
}

// Frozen statistics (training == 0): the returns are not advanced, only returns[done] = 0 after every step -- so over a T-step
// window an env's return is zeroed iff any of its T done flags is set.
__global__ void __launch_bounds__(256)
k_vn_clear_done(const uint8_t* __restrict__ done, int N, int T, double* __restrict__ returns)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    bool any = false;
    for (int t = 0; t < T; t++) any |= done[(size_t)t * N + e] != 0;
    if (any) returns[e] = 0.0;
}

// ================================================================================== generalised advantage estimation
// stable-baselines3 2.0.0a13, common/buffers.py RolloutBuffer.compute_returns_and_advantage, as the reference's A2C and PPO run it
// after every collect (config/config_agent.yaml: gamma / gae_lambda / n_steps).  With done[t] = episode_starts[t + 1] (and the
// method's `dones` argument = done[T - 1]) the loop over `step` backwards is, in the arrays' own precision F:
//   nnt = 1 - done[t];  nv = t == T - 1 ? last_val : val[t + 1]
//   delta = rew[t] + gamma * nv * nnt - val[t];  last = delta + gamma * gae_lambda * nnt * last;  adv[t] = last;  ret[t] = last + val[t]
// evaluated left to right as Python does: (g * nv) * nnt and (gl * nnt) * last, g = F(gamma), gl = F(gamma * gae_lambda), every
// operation rounded once (no contraction into an FMA: bit equality with NumPy depends on it).  nnt multiplies, it does not
// select: a NaN / Inf next value at a finished step poisons the result as it does in NumPy.
// The same shape as k_vn_moments' recurrence: one lane per env, serial in t, every load and store coalesced over the envs, the
// loads of a batch of steps issued ahead of the dependent arithmetic.  The next value is carried in a register, and a batch's
// loads are all issued before its first store, so a lane reads every element of its column before it writes it: adv may be
// rew's buffer and ret may be val's (hence no __restrict__ on those four).
__device__ __forceinline__ float rn_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float rn_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float rn_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double rn_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double rn_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double rn_sub(double a, double b) { return __dsub_rn(a, b); }

template <typename F, int U>
__global__ void __launch_bounds__(64)
k_gae(const F* rew, const F* val, const uint8_t* __restrict__ done, const F* __restrict__ last_val, int N, int T, F g, F gl,
      F* adv, F* ret)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * 64 + threadIdx.x;            // one wave per workgroup: a mid-size batch spreads over the CUs
    if (e >= N) return;
    F nv = last_val[e], last = (F)0;
    for (int tb = T - 1; tb >= 0; tb -= U) {                // steps tb, tb - 1, ... tb - U + 1
        F r[U], v[U]; uint8_t d[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const size_t i = (size_t)max(tb - j, 0) * N + e;
            r[j] = rew[i]; v[j] = val[i]; d[j] = done[i];
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            if (tb - j >= 0) {
                const size_t i = (size_t)(tb - j) * N + e;
                const F nnt = d[j] ? (F)0 : (F)1;           // 1 - done, exactly
                const F delta = rn_sub(rn_add(r[j], rn_mul(rn_mul(g, nv), nnt)), v[j]);
                last = rn_add(delta, rn_mul(rn_mul(gl, nnt), last));
                adv[i] = last;
                if (ret) ret[i] = rn_add(last, v[j]);
                nv = v[j];
            }
        }
    }
}

// ================================================================================== shuffled minibatches of a rollout
// stable-baselines3 2.0.0a13, common/buffers.py RolloutBuffer.get / _get_samples: swap_and_flatten every [T][N][...] buffer to
// [N * T][...] (flat index i = e * T + t), draw a permutation, yield the rows indices[start : start + batch_size] of every buffer.
// k_minibatch gathers ONE such batch straight from the [T][N] layout: output row b = source row (idx[b] % T, idx[b] / T), the
// observations through strides (row-major [T][N][F] and feature-major [T][F][pitch] alike), up to PTG_MB_MAX_COLS [T][N] columns
// of 1 / 2 / 4 / 8-byte elements as raw bytes.  A byte copy: no arithmetic touches the payload.
// One wave owns MB_ROWS consecutive output rows.  Lane l < MB_ROWS loads idx[b0 + l], checks it, does the row's ONE division by T
// and keeps the source row's byte offset; it also copies the row's column entries (consecutive lanes, consecutive output elements).
// Then all 64 lanes run over the consecutive units (16-byte pieces when row length and every row base allow it, else elements) of
// the wave's MB_ROWS x F output block -- every store instruction is one contiguous segment, every load a run of whole rows -- and
// fetch each unit's row offset from the owning lane (two ds_bpermute, no LDS allocation).  (row, unit-in-row) advance by the
// wave-uniform (64 / P, 64 % P) per step, so there is no division per unit.  MB_U units per lane are loaded before the first is
// stored.  An index outside [0, T * N) never becomes an address: its row is skipped and err[4] is set (PTG_E_INDEX).
constexpr int MB_ROWS = 16;              // rows per wave: a 203-row PPO batch spreads over 13 waves, 65 536 rows over 16 waves per CU
constexpr int MB_WAVES = 4;              // waves per workgroup
constexpr int MB_U = 4;                  // units in flight per lane
constexpr unsigned MB_BAD = 0xFFFFFFFFu; // high word of the row offset of a rejected index (a real offset stays far below 2^63)

struct MbCols {                          // by value in the launch: a captured call holds no host memory
    const void* src[PTG_MB_MAX_COLS];
    void* dst[PTG_MB_MAX_COLS];
    int bytes[PTG_MB_MAX_COLS];
    int n;
};

template <typename V>
__device__ __forceinline__ void mb_copy_col(const void* src, void* dst, size_t from, size_t to)
{
    ((V*)dst)[to] = ((const V*)src)[from];
}

__device__ __forceinline__ void mb_copy_entry(int bytes, const void* src, void* dst, size_t from, size_t to)
{
    switch (bytes) {
        case 1: mb_copy_col<uint8_t>(src, dst, from, to); break;
        case 2: mb_copy_col<uint16_t>(src, dst, from, to); break;
        case 4: mb_copy_col<uint32_t>(src, dst, from, to); break;
        default: mb_copy_col<uint64_t>(src, dst, from, to); break;
    }
}

// The second half of a gathering wave (k_minibatch, k_rb_sample): lane l < rows holds `off`, the byte offset of its source row in
// `src` (high word MB_BAD: a rejected row); all 64 lanes stream the rows x P units of the wave's contiguous output block `out`.
template <typename V>
__device__ __forceinline__ void mb_stream_rows(const char* __restrict__ src, size_t unit_stride, unsigned P, size_t off, unsigned rows,
                                               unsigned lane, char* __restrict__ out_block)
{
    const unsigned off_lo = (unsigned)off, off_hi = (unsigned)(off >> 32);
    const unsigned dr = 64u / P, dp = 64u - dr * P;          // one step of 64 units, in (rows, units of a row)
    unsigned r = lane / P, p = lane - r * P;
    V* const out = (V*)out_block;                            // the wave's block of rows x P units, unit q = r * P + p at out[q]
    const unsigned units = rows * P;                         // host: P <= 2^20
    for (unsigned q = lane; q - lane < units; q += 64u * MB_U) {            // wave-uniform trip count: every lane stays for the cross-lane reads
        V v[MB_U];
        bool ok[MB_U];
#pragma unroll
        for (int j = 0; j < MB_U; j++) {
            const unsigned rr = min(r, (unsigned)MB_ROWS - 1);              // a lane in range for the cross-lane read
            const unsigned lo = __shfl(off_lo, (int)rr), hi = __shfl(off_hi, (int)rr);
            ok[j] = r < rows && hi != MB_BAD;
            v[j] = V();
            if (ok[j]) v[j] = *(const V*)(src + (((size_t)hi << 32) | lo) + (size_t)p * unit_stride);
            r += dr; p += dp;
            if (p >= P) { p -= P; r++; }
        }
#pragma unroll
        for (int j = 0; j < MB_U; j++)
            if (ok[j]) out[q + 64u * j] = v[j];
    }
}

// The two 32-bit words of row b of the c-th device-drawn batch under `seed` (include/ptg_env.h states the same lines; the tests
// restate them in integer arithmetic): a chain of lowbias32 over the six 32-bit halves of (seed, c, b), then two finalisers.
__device__ __forceinline__ unsigned long long rb_draw_word(unsigned long long seed, unsigned long long c, unsigned long long b)
{
    unsigned k = lowbias32((unsigned)seed ^ 0x9E3779B9u);
    k = lowbias32(k + (unsigned)(seed >> 32));
    k = lowbias32(k ^ (unsigned)c);
    k = lowbias32(k + (unsigned)(c >> 32));
    k = lowbias32(k ^ (unsigned)b);
    k = lowbias32(k + (unsigned)(b >> 32));
    const unsigned w0 = lowbias32(k ^ 0x85EBCA6Bu), w1 = lowbias32(k ^ 0xC2B2AE35u);
    return ((unsigned long long)w0 << 32) | w1;
}

// The index source "drawn" of k_minibatch (include/ptg_env.h, ptg_minibatch_drawn, states the same lines; tests/
// minibatch_drawn_restatement.py restates them in Python integers): no permutation exists in memory, row b of batch j of epoch c
// is perm_c(j * B + b), a keyed bijection of [0, TN) -- PTG_MB_PERM_ROUNDS Feistel rounds over the a low and b high bits of the
// position, applied until the result is below TN.  2^(a + b) < 2 TN for TN > 2, so a walk is two applications on average.
struct MbDraw {                          // by value in the launch
    const unsigned long long* cursor;    // {epochs finished, batches drawn in this epoch}, read here: the launch may be a replay
    unsigned long long seed;
    long long* idx_out;                  // nullable: the indices used, [B]
    unsigned a, b;                       // bits of the low and of the high half
};
struct MbDrawn {};                       // k_minibatch's index type I for that source: idx is not read

__device__ __forceinline__ unsigned long long mb_perm_rounds(unsigned long long x, const unsigned (&key)[PTG_MB_PERM_ROUNDS], unsigned a,
                                                             unsigned mask_a, unsigned mask_b)
{
    unsigned lo = (unsigned)x & mask_a, hi = (unsigned)(x >> a) & mask_b;
#pragma unroll
    for (int r = 0; r < PTG_MB_PERM_ROUNDS; r += 2) {
        hi ^= lowbias32(lo ^ key[r]) & mask_b;
        lo ^= lowbias32(hi ^ key[r + 1]) & mask_a;
    }
    return ((unsigned long long)hi << a) | lo;
}

template <typename V, typename I>
__global__ void __launch_bounds__(64 * MB_WAVES)
k_minibatch(const I* __restrict__ idx, MbDraw draw, size_t B, unsigned T, size_t N, size_t TN, const char* __restrict__ obs, size_t s_t,
            size_t s_n, size_t unit_stride, unsigned P, char* __restrict__ obs_out, MbCols cols, int* err)
{
    constexpr bool DRAWN = std::is_same<I, MbDrawn>::value;
    const unsigned lane = threadIdx.x & 63u;
    const size_t b0 = ((size_t)blockIdx.x * MB_WAVES + (threadIdx.x >> 6)) * MB_ROWS;
    if (b0 >= B) return;                                     // wave-uniform
    const unsigned rows = (unsigned)min((size_t)MB_ROWS, B - b0);
    size_t off = (size_t)MB_BAD << 32;                       // byte offset of this lane's source row in the observation buffer
    [[maybe_unused]] unsigned key[PTG_MB_PERM_ROUNDS];
    if constexpr (DRAWN) {                                   // lane r makes round key r; every lane of the wave is still here
        const unsigned mine = (unsigned)(rb_draw_word(draw.seed, draw.cursor[0], lane % PTG_MB_PERM_ROUNDS) >> 32);
#pragma unroll
        for (int r = 0; r < PTG_MB_PERM_ROUNDS; r++) key[r] = __shfl(mine, r);
    }
    if (lane < rows) {
        long long v;
        if constexpr (DRAWN) {
            // the position in the epoch's order; one at or past TN (a cursor set past its epoch, or a batch size changed within one)
            // lies on no cycle that is known to return below TN, so it is never walked: rejected like an index out of range
            const unsigned long long pos = draw.cursor[1] * B + b0 + lane;
            const unsigned mask_a = (1u << draw.a) - 1u, mask_b = (1u << draw.b) - 1u;              // host: a <= b <= 24
            unsigned long long x = pos;
            if (pos < TN)
                do x = mb_perm_rounds(x, key, draw.a, mask_a, mask_b); while (x >= TN);     // ends: pos itself lies on x's cycle
            v = (long long)x;
            if (draw.idx_out && pos < TN) draw.idx_out[b0 + lane] = v;
        } else {
            v = (long long)idx[b0 + lane];
        }
        if ((unsigned long long)v < (unsigned long long)TN) {
            size_t e, t;
            if (TN <= 0xFFFFFFFFull) { const unsigned u = (unsigned)v; e = u / T; t = u - (unsigned)e * T; }   // the common case: 32-bit division
            else { e = (size_t)v / T; t = (size_t)v - e * T; }
            off = t * s_t + e * s_n;
            const size_t from = t * N + e, to = b0 + lane;
            for (int c = 0; c < cols.n; c++)                 // wave-uniform trip count and switch
                mb_copy_entry(cols.bytes[c], cols.src[c], cols.dst[c], from, to);
        } else {
            err[4] = 1;
        }
    }
    if (obs) mb_stream_rows<V>(obs, unit_stride, P, off, rows, lane, obs_out + b0 * P * sizeof(V));
}

// One thread, in stream order behind a drawn gather (as k_rb_bump is behind k_rb_sample): the next batch, and behind the epoch's last
// one -- `batches` = TN / B -- the next epoch.  finish: ptg_minibatch_end_epoch, an epoch cut short ends; a fresh one is left alone.
__global__ void k_mb_cursor(unsigned long long* cursor, unsigned long long batches, int finish)
{
    unsigned long long j = cursor[1];
    if (finish) {
        if (j == 0) return;
    } else if (++j < batches) {
        cursor[1] = j;
        return;
    }
    cursor[0] += 1;
    cursor[1] = 0;
}

// ================================================================================== replay buffer of the off-policy algorithms
// stable-baselines3 2.0.0a13, common/buffers.py ReplayBuffer.add / sample / _get_samples (optimize_memory_usage off), which the
// reference's DQN, TD3, SAC and TQC train from.  The caller owns the rings (ptg_replay, include/ptg_env.h): observations and next
// observations [S][N][F] row-major, up to PTG_MB_MAX_COLS columns [S][N], and a device cursor {steps added, batches drawn}.
// k_rb_add / k_rb_add_tr store a window of T vector steps at slots (cursor[0] + t) % S; k_rb_sample gathers a batch at flat indices
// i = slot * N + e -- the caller's, or drawn on the device -- which in these rings ARE the row numbers: no division per row.
// k_rb_bump advances a cursor word in stream order behind them, so a captured add / sample can be replayed.
struct RbAdd {                           // by value in the launch
    const char *prev, *obs, *fin;        // prev [N][F]; obs, fin (nullable) [T][N][F], all through the byte strides s_t, s_n (and s_f)
    const uint8_t* done;                 // [T][N], nullable when neither fin nor a done column needs it
    size_t s_t, s_n, s_f;                // bytes
    char *ring0, *ring1;                 // observations, next observations
    const unsigned long long* cursor;
    size_t S, N;
    unsigned T, F;
    MbCols cols;                         // src: the window's [T][N] columns, dst: their rings [S][N]
    int done_col;                        // the column written as float32 0 / 1 from `done`, or -1
};

__device__ __forceinline__ void rb_add_cols(const RbAdd& a, size_t from, size_t to)
{
    for (int c = 0; c < a.cols.n; c++) {
        if (c == a.done_col) ((float*)a.cols.dst[c])[to] = a.done[from] ? 1.0f : 0.0f;
        else mb_copy_entry(a.cols.bytes[c], a.cols.src[c], a.cols.dst[c], from, to);
    }
}

// Rows that are contiguous in the source (s_f = one element): a slot [N][F] of either ring is then ONE contiguous run of N * P units
// (V = a 16-byte piece when row length and every base allow it, else an element), unit u of the slot = (env u / P, unit u % P of
// its row); consecutive lanes take consecutive units, so every store is a contiguous segment and every load a run of whole rows
// (a single run for a [T][N][F] contiguous source).  A finished env's next observation comes from `fin`: a per-row select of the
// source pointer.  The lane on a row's first unit also moves the row's column entries.  blockIdx.y strides over the steps.
template <typename V>
__global__ void __launch_bounds__(256)
k_rb_add(RbAdd a, unsigned P, size_t NP)
{
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= NP) return;
    size_t e; unsigned p;
    if (NP <= 0xFFFFFFFFull) { const unsigned q = (unsigned)u / P; e = q; p = (unsigned)u - q * P; }
    else { e = u / P; p = (unsigned)(u - e * P); }
    const size_t a0 = (size_t)(a.cursor[0] % a.S);
    const size_t in_row = e * a.s_n + (size_t)p * sizeof(V);
    for (unsigned t = blockIdx.y; t < a.T; t += gridDim.y) {
        size_t slot = a0 + t;                                // T <= S: at most one wrap
        if (slot >= a.S) slot -= a.S;
        const size_t from = (size_t)t * a.N + e, to = slot * a.N + e;
        const char* s0 = (t == 0 ? a.prev : a.obs + (size_t)(t - 1) * a.s_t) + in_row;
        const char* s1 = (a.fin && a.done[from] ? a.fin : a.obs) + (size_t)t * a.s_t + in_row;
        const V v0 = *(const V*)s0, v1 = *(const V*)s1;
        const size_t o = (slot * NP + u) * sizeof(V);
        *(V*)(a.ring0 + o) = v0;
        *(V*)(a.ring1 + o) = v1;
        if (p == 0) rb_add_cols(a, from, to);
    }
}

// Any other source (feature-major [T][F][pitch]: s_n = one element): a 64-env x 32-feature tile of each ring goes through LDS, read
// with the lanes along the envs (coalesced in a feature plane), written with the lanes along the features (128- / 256-byte
// segments of the ring's rows).  The 33-element pitch keeps both phases off one bank.
constexpr int RB_TE = 64, RB_TF = 32;
template <typename E>
__global__ void __launch_bounds__(256)
k_rb_add_tr(RbAdd a)
{
    __shared__ E tile[2][RB_TE][RB_TF + 1];
    const unsigned tid = threadIdx.x;
    const size_t e0 = (size_t)blockIdx.x * RB_TE;
    const unsigned el = tid & 63u, fr = tid >> 6, fl = tid & 31u, er = tid >> 5;
    const size_t a0 = (size_t)(a.cursor[0] % a.S);
    for (unsigned t = blockIdx.y; t < a.T; t += gridDim.y) {
        size_t slot = a0 + t;
        if (slot >= a.S) slot -= a.S;
        const size_t e = e0 + el;
        const bool live = e < a.N;
        const char *s0 = nullptr, *s1 = nullptr;
        if (live) {
            s0 = (t == 0 ? a.prev : a.obs + (size_t)(t - 1) * a.s_t) + e * a.s_n;
            s1 = (a.fin && a.done[(size_t)t * a.N + e] ? a.fin : a.obs) + (size_t)t * a.s_t + e * a.s_n;
        }
        for (unsigned f0 = 0; f0 < a.F; f0 += RB_TF) {
            if (live)
                for (unsigned f = fr; f < RB_TF && f0 + f < a.F; f += 4) {
                    tile[0][el][f] = *(const E*)(s0 + (size_t)(f0 + f) * a.s_f);
                    tile[1][el][f] = *(const E*)(s1 + (size_t)(f0 + f) * a.s_f);
                }
            __syncthreads();
            if (f0 + fl < a.F)
                for (unsigned r = er; r < RB_TE && e0 + r < a.N; r += 8) {
                    const size_t o = ((slot * a.N + e0 + r) * a.F + f0 + fl) * sizeof(E);
                    *(E*)(a.ring0 + o) = tile[0][r][fl];
                    *(E*)(a.ring1 + o) = tile[1][r][fl];
                }
            __syncthreads();
        }
        if (tid < 64 && live) rb_add_cols(a, (size_t)t * a.N + e, slot * a.N + e);
    }
}

__global__ void k_rb_bump(unsigned long long* word, unsigned long long by) { *word += by; }

// the Gaussian draw of a word pair (include/ptg_env.h, ptg_act): Box-Muller's cosine branch on u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ double rb_draw_normal(unsigned long long w)
{
    const unsigned w0 = (unsigned)(w >> 32), w1 = (unsigned)w;
    const double u1 = ((double)w0 + 1.0) * 2.3283064365386963e-10, u2 = (double)w1 * 2.3283064365386963e-10;      // 2^-32
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

struct RbNorm {                          // SB3's _normalize_reward at sample time: column `col` through k_vn_norm's expression
    int col;                             // -1: none
    const double* stats;                 // the handle's {mean, var, count}
    double eps, clip;
};

template <typename OUT>
__device__ __forceinline__ void rb_norm_entry(const void* src, void* dst, size_t from, size_t to, double den, double clip)
{
    const double v = (double)((const OUT*)src)[from] / den;                 // k_vn_norm's lines
    const double lo = v < -clip ? -clip : v;
    ((OUT*)dst)[to] = (OUT)(lo > clip ? clip : lo);
}

// k_minibatch's scheme with two row sources sharing one offset: a wave owns MB_ROWS output rows; lane l < rows takes or draws
// the index of row b0 + l, checks it against size * N (size = min(cursor[0], S), read here: the launch may be a replay) and moves
// the row's column entries; then all 64 lanes stream the rows x F block of each ring.  An index out of range, or any draw from an
// empty buffer, never becomes an address: the row is left as it was and err[4] is set (PTG_E_INDEX).
template <typename V>
__global__ void __launch_bounds__(64 * MB_WAVES)
k_rb_sample(const long long* __restrict__ idx, size_t B, unsigned long long seed, const unsigned long long* __restrict__ cursor, size_t S,
            size_t N, size_t row_bytes, unsigned P, const char* __restrict__ ring0, const char* __restrict__ ring1, char* __restrict__ out0,
            char* __restrict__ out1, MbCols cols, RbNorm norm, long long* __restrict__ idx_out, int* err)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t b0 = ((size_t)blockIdx.x * MB_WAVES + (threadIdx.x >> 6)) * MB_ROWS;
    if (b0 >= B) return;                                     // wave-uniform
    const unsigned rows = (unsigned)min((size_t)MB_ROWS, B - b0);
    size_t off = (size_t)MB_BAD << 32;
    if (lane < rows) {
        const unsigned long long added = cursor[0];
        const unsigned long long total = (added < S ? added : S) * N;
        const size_t to = b0 + lane;
        unsigned long long i;
        if (idx) i = (unsigned long long)idx[to];            // a negative index is a huge one
        else i = total ? __umul64hi(rb_draw_word(seed, cursor[1], to), total) : ~0ull;
        if (i < total) {
            off = (size_t)i * row_bytes;
            if (idx_out) idx_out[to] = (long long)i;
            for (int c = 0; c < cols.n; c++) {
                if (!cols.dst[c]) continue;
                if (c == norm.col) {
                    const double den = sqrt(norm.stats[1] + norm.eps);      // k_vn_scan's frozen denominator
                    if (cols.bytes[c] == 8) rb_norm_entry<double>(cols.src[c], cols.dst[c], (size_t)i, to, den, norm.clip);
                    else rb_norm_entry<float>(cols.src[c], cols.dst[c], (size_t)i, to, den, norm.clip);
                } else {
                    mb_copy_entry(cols.bytes[c], cols.src[c], cols.dst[c], (size_t)i, to);
                }
            }
        } else {
            err[4] = 1;
        }
    }
    if (out0) mb_stream_rows<V>(ring0, sizeof(V), P, off, rows, lane, out0 + b0 * row_bytes);
    if (out1) mb_stream_rows<V>(ring1, sizeof(V), P, off, rows, lane, out1 + b0 * row_bytes);
}

// ================================================================================== rollout buffer of the on-policy algorithms
// stable-baselines3 2.0.0a13, common/buffers.py RolloutBuffer.reset / add, which the reference's PPO and A2C collect into.  The
// caller owns the storage (ptg_rollout_buffer, include/ptg_env.h): T + 1 observation blocks in the engine's own layout, up to
// PTG_MB_MAX_COLS columns [T][N] and a device cursor {rows added in this window, completion ticket}.  k_ro_add copies the block
// ptg_step just wrote to row cursor[0] + 1 and one entry per env and column to row cursor[0] of the columns; every workgroup reads
// cursor[0] before anything else, and k_ro_bump advances it in stream order behind the copy, as k_rb_bump does for the replay buffer.
// A full buffer (cursor[0] >= T) forms no address: k_ro_bump raises err[4] (PTG_E_INDEX) and leaves the cursor.  The same kernel with
// begin = 1 copies into row 0 and zeroes both cursor words.
// Two one-launch forms were measured beside it and lost; they compile only into a measurement build,
// -DPTG_RO_FORM=1 | 2 (tools/rollout_buffer_cost.py), never into the library that ships: the workgroup that draws the last ticket (one
// atomicAdd per workgroup on cursor[1]) zeroes the ticket and advances the cursor, behind a __threadfence (1) or without one (2).
// A block keeps the source's layout (no transpose): unit u of a block lies at the same byte offset in the source and in the row.
// One contiguous run (row-major, sb3_flat, split, feature-major without a pitch): unit u at u * sizeof(V), V a 16-byte piece when the
// run is a whole number of them and every base is aligned, else an element.  Strided (feature-major with a pitch): element
// u = o * inner + i at o * s_outer + i * s_inner, the lanes along the unit-stride axis; pad columns are neither read nor written.
// A workgroup takes 256 * RO_U consecutive units, lane l the units l, l + 256, ...: every load and store instruction of a wave is one
// contiguous segment, and RO_U loads are in flight before the first store.  Lane e < N of the launch moves env e's column entries
// (consecutive lanes, consecutive entries of every column ring).  The data path holds no atomic.
constexpr int RO_U = 4;                  // units in flight per lane: 640 workgroups, not 2 560, at 65 536 envs x 40 float32
#ifndef PTG_RO_FORM
#define PTG_RO_FORM 0                    // 0: k_ro_bump behind the copy (ships); 1, 2: the ticket forms of a measurement build
#endif

struct RoAdd {                           // by value in the launch: a captured call holds no host memory
    const char* obs;                     // the source block
    char* rows;                          // buffer row 0
    unsigned long long* cursor;          // {rows added, ticket (counted in by a measurement build only; else 0)}
    int* err;
    size_t row_bytes;                    // between buffer rows
    size_t T, N, units, inner;           // inner == units: one contiguous run
    size_t s_outer, s_inner;             // bytes
    const char* col_src[PTG_MB_MAX_COLS];
    char* col_dst[PTG_MB_MAX_COLS];
    size_t col_stride[PTG_MB_MAX_COLS];  // of the source, bytes
    int col_bytes[PTG_MB_MAX_COLS];
    int n_cols;
};

template <typename V>
__global__ void __launch_bounds__(256)
k_ro_add(RoAdd a, int begin)
{
    const unsigned long long t = begin ? 0ull : a.cursor[0];
    const bool full = !begin && t >= a.T;
    if (!full) {
        char* const dst = a.rows + (size_t)(begin ? 0ull : t + 1) * a.row_bytes;
        const size_t u0 = (size_t)blockIdx.x * (256 * RO_U) + threadIdx.x;
        V v[RO_U];
        size_t off[RO_U];
        bool ok[RO_U];
#pragma unroll
        for (int j = 0; j < RO_U; j++) {
            const size_t u = u0 + (size_t)j * 256;
            ok[j] = u < a.units;
            off[j] = u * sizeof(V);
            if (a.inner != a.units) {                        // launch-uniform
                if (a.units <= 0xFFFFFFFFull) { const unsigned o = (unsigned)u / (unsigned)a.inner; off[j] = o * a.s_outer + ((unsigned)u - o * (unsigned)a.inner) * a.s_inner; }
                else { const size_t o = u / a.inner; off[j] = o * a.s_outer + (u - o * a.inner) * a.s_inner; }
            }
            v[j] = V();
            if (ok[j]) v[j] = *(const V*)(a.obs + off[j]);
        }
#pragma unroll
        for (int j = 0; j < RO_U; j++)
            if (ok[j]) *(V*)(dst + off[j]) = v[j];
        const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (!begin && e < a.N)
            for (int c = 0; c < a.n_cols; c++) {             // wave-uniform trip count and switch
                const char* s = a.col_src[c] + e * a.col_stride[c];
                char* d = a.col_dst[c] + ((size_t)t * a.N + e) * (size_t)a.col_bytes[c];
                switch (a.col_bytes[c]) {
                    case 1: *(uint8_t*)d = *(const uint8_t*)s; break;
                    case 2: *(uint16_t*)d = *(const uint16_t*)s; break;
                    case 4: *(uint32_t*)d = *(const uint32_t*)s; break;
                    default: *(uint64_t*)d = *(const uint64_t*)s; break;
                }
            }
    }
    if (begin) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.cursor[0] = 0; a.cursor[1] = 0; }
        return;
    }
#if PTG_RO_FORM != 0
    // Measurement build.  The cursor must not move before every workgroup has read it.  It cannot: a workgroup's loads of cursor[0]
    // have returned before its stores are issued (their addresses, and the branch on `full`, depend on t), the stores stand before
    // the barrier in program order, and the draw stands behind it -- so every draw follows its workgroup's read, and the one write
    // of cursor[0] follows the draw that returned gridDim.x - 1, i.e. all draws.  The draw is a relaxed atomic and the two stores
    // behind it are plain: nothing in this launch reads what they publish, and the end of the kernel publishes them to the next.
    // Form 1 adds the agent-scope release the first design asked for; it orders nothing that anyone waits for.
#if PTG_RO_FORM == 1
    __threadfence();
#endif
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(&a.cursor[1], 1ull) == (unsigned long long)gridDim.x - 1) {
        a.cursor[1] = 0;
        if (full) a.err[4] = 1;
        else a.cursor[0] = t + 1;
    }
#endif
}

#if PTG_RO_FORM == 0
// DeviceReplayBuffer's form: the copy kernel, then this one in stream order.
__global__ void k_ro_bump(unsigned long long* cursor, unsigned long long T, int* err)
{
    if (cursor[0] >= T) err[4] = 1;
    else cursor[0] += 1;
}
#endif

// ================================================================================== the action head
// What runs between the network's output and env.step while collecting (include/ptg_env.h, ptg_act, states the lines; the tests
// restate them in NumPy): SB3's CategoricalDistribution sample / log_prob / entropy, DQN's epsilon-greedy, the Gaussian heads of
// TD3 / SAC / TQC / continuous A2C and PPO.  One lane per env on consecutive envs, no cross-lane traffic; float64 arithmetic
// whatever the input type, rounded once on the store.  A discrete row is read three times (maximum; sum; partial sums, entropy and
// the chosen log-prob) straight from global memory: a wave's 64 x A block is 64 * A * sizeof(IN) contiguous bytes (1 280 at float32,
// A = 5), every pass after the first finds its lines in the L1 / L2, and the launch is bound by its own latency at every batch
// the project runs -- an LDS-staged tile was measured beside it and bought nothing, so it is not in the tree.
// Nothing per lane is indexed dynamically, so nothing spills to scratch for A up to 32.
struct ActArgs {                         // by value in the launch
    const void* in; size_t s_n;          // elements
    const void* param; size_t param_s;   // EPS_GREEDY: const double* epsilon; GAUSSIAN: log_std in IN, stride 0 | 1
    void *act, *raw, *logp, *ent;
    const unsigned long long* counter;   // null when deterministic
    unsigned long long seed;
    long long env_offset;
    double lo, hi;
    size_t N;
    int A, kind, flags, act_kind;
    int* err;
};

__device__ __forceinline__ void act_store_action(const ActArgs& a, size_t e, long long v)
{
    if (a.act_kind == PTG_ACT_I64) ((long long*)a.act)[e] = v; else ((int*)a.act)[e] = (int)v;
}

constexpr int ACT_BLOCK = 256;
template <typename IN>
__global__ void __launch_bounds__(ACT_BLOCK)
k_act(ActArgs a)
{
    const size_t e = (size_t)blockIdx.x * ACT_BLOCK + threadIdx.x;
    if (e >= a.N) return;                                    // the ragged last wave
    const bool det = (a.flags & PTG_HEAD_DETERMINISTIC) != 0;
    unsigned w0 = 0, w1 = 0;
    if (!det) {
        const unsigned long long w = rb_draw_word(a.seed, a.counter[0], (unsigned long long)(a.env_offset + (long long)e));
        w0 = (unsigned)(w >> 32); w1 = (unsigned)w;
    }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    IN* const logp_o = (IN*)a.logp; IN* const ent_o = (IN*)a.ent; IN* const raw_o = (IN*)a.raw;
    if (a.kind == PTG_HEAD_GAUSSIAN) {
        const double mu = (double)((const IN*)a.in)[e * a.s_n];
        const double ls = (double)((const IN*)a.param)[e * a.param_s];
        if (!(fabs(mu) <= 1.7976931348623157e308) || !(ls <= 1.7976931348623157e308)) {       // NaN or Inf mean; NaN or +Inf log_std
            ((float*)a.act)[e] = 0.0f;
            if (raw_o) raw_o[e] = (IN)nan;
            if (logp_o) logp_o[e] = (IN)nan;
            if (ent_o) ent_o[e] = (IN)nan;
            a.err[5] = 1;
            return;
        }
        const double z = det ? 0.0 : rb_draw_normal(((unsigned long long)w0 << 32) | w1);
        const double g = mu + exp(ls) * z;
        double lp = ((-(z * z) / 2.0) - ls) - 0.9189385332046727;
        double x = g;
        if (a.flags & PTG_HEAD_SQUASH) {
            x = tanh(g);
            lp = lp - log((1.0 - x * x) + 1e-6);
        }
        x = x < a.lo ? a.lo : (x > a.hi ? a.hi : x);
        ((float*)a.act)[e] = (float)x;
        if (raw_o) raw_o[e] = (IN)g;
        if (logp_o) logp_o[e] = (IN)lp;
        if (ent_o) ent_o[e] = (IN)(1.4189385332046727 + ls);
        return;
    }
    // discrete kinds: maximum and its first index
    const IN* __restrict__ row = (const IN*)a.in + e * a.s_n;
    const int A = a.A;
    double m = (double)row[0];
    int jm = 0;
    bool bad = m != m;
    for (int j = 1; j < A; j++) {
        const double l = (double)row[j];
        bad = bad || l != l;
        if (l > m) { m = l; jm = j; }
    }
    bad = bad || !(fabs(m) <= 1.7976931348623157e308);       // +Inf somewhere, or -Inf everywhere
    if (a.kind == PTG_HEAD_EPS_GREEDY) {
        long long action = jm;
        if (!det) {
            const double eps = ((const double*)a.param)[0];
            if (!(eps >= 0.0 && eps <= 1.0)) bad = true;
            else if ((unsigned long long)w0 < (unsigned long long)(eps * 4294967296.0))
                action = (long long)(((unsigned long long)w1 * (unsigned long long)A) >> 32);
        }
        if (bad) { action = 0; a.err[5] = 1; }
        act_store_action(a, e, action);
        return;
    }
    if (bad) {
        act_store_action(a, e, 0);
        if (logp_o) logp_o[e] = (IN)nan;
        if (ent_o) ent_o[e] = (IN)nan;
        a.err[5] = 1;
        return;
    }
    double s = 0.0;
    for (int j = 0; j < A; j++) s += exp((double)row[j] - m);
    const double log_s = log(s);
    const double us = det ? 0.0 : (double)(((unsigned long long)w0 << 21) | (unsigned long long)(w1 >> 11)) * 1.1102230246251565e-16 * s;      // 2^-53
    double c = 0.0, ent = 0.0, lp = 0.0;
    int action = det ? jm : -1;
    for (int j = 0; j < A; j++) {
        const double d = (double)row[j] - m;
        const double ej = exp(d);
        const double lpj = d - log_s;
        c += ej;
        if (ej != 0.0) ent += (ej / s) * lpj;
        const bool take = det ? j == jm : (action < 0 && (us < c || j == A - 1));
        if (take) { action = j; lp = lpj; }
    }
    act_store_action(a, e, action);
    if (logp_o) logp_o[e] = (IN)lp;
    if (ent_o) ent_o[e] = (IN)(-ent);
}

// ================================================================================== the policy loss
// What runs between the network's output on a minibatch and the gradient that goes back into it (include/ptg_env.h, ptg_policy_loss,
// states the lines; tests/policy_loss_restatement.py restates them in NumPy): SB3's evaluate_actions (Categorical / DiagGaussian
// log_prob and entropy) and the loss lines of PPO.train / A2C.train, with d loss / d logits (or means), d loss / d values and
// d loss / d log_std in closed form -- every one is a function of quantities the forward pass holds, so no graph is walked back.
// One lane per row on consecutive rows, float64 arithmetic whatever the input type, gradients rounded once on the store.  A
// categorical row is read as k_act reads it (maximum; sum; entropy and the chosen log-prob) plus a fourth pass that writes the
// gradients, which need the row's complete entropy; exp is evaluated again instead of kept, so nothing per lane is indexed dynamically.
// Batch-wide quantities (the advantage moments, six sums, the log_std gradient) are reduced in a fixed order, the same for every
// loss of this file (loss_tail and k_loss_final are its only text):
//   1. a shuffle tree per wave (pl_wave_sum: offsets 32, 16, ..., 1)
//   2. the block's four waves in wave order (pl_block_sum)
//   3. a batch of one block ends there; else every block stores its PL_TERMS sums at partials + block * PL_PITCH in the caller's
//      workspace and one more block follows, whose thread t adds the partials of blocks t, t + PL_BLOCK, t + 2 PL_BLOCK, ... in that
//      order from 0.0, then steps 1 and 2 again
// The order is given by the block count alone and there are no floating-point atomics: the same inputs give the same bits.  Moments
// travel as (count, mean, M2) and meet in chan_merge, as the reward normalisation's do.
struct LossArgs {                        // by value in the launch
    const void* in; size_t s_n;          // elements
    const void* val; size_t v_s;
    const void *act, *old_lp, *adv, *ret, *old_val, *log_std;
    void* g_in; size_t g_s;
    void* g_val; size_t gv_s;
    void* g_ls;
    double* stats;
    double* ws;                          // [0..2] merged advantage moments; [4 ..) moment partials [nblk][3]; then row partials [nblk][8]
    double eps, eps_v, ent_coef, vf_coef;
    size_t B;
    int A, kind, head, flags, act_kind, nblk;
    int* err;
};
struct PlRow { double surr, q, H, kl, cf, gls; };     // a row's terms of the five means and of the log_std gradient's sum

constexpr int PL_BLOCK = 256, PL_WAVES = PL_BLOCK / 64, PL_TERMS = 6, PL_PITCH = 8;
constexpr double PL_DBL_MAX = 1.7976931348623157e308;

__device__ __forceinline__ double pl_wave_sum(double v)      // a + b == b + a: every lane ends with the same bits
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ bool pl_finite(double x) { return fabs(x) <= PL_DBL_MAX; }

// (count, mean, M2) of the block's advantages: two shuffle trees per wave (sum -> mean, then squared deviations from it: a sum of
// squares would cancel), the block's waves merged in wave order.  Every thread of the block calls it; `sh` holds PL_WAVES * 3 doubles.
template <typename IN>
__device__ __forceinline__ void pl_block_moments(const LossArgs& a, size_t i, bool live, double* sh, double& c, double& m, double& M)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double x = live ? (double)((const IN*)a.adv)[i] : 0.0;
    const double n = pl_wave_sum(live ? 1.0 : 0.0);
    const double s = pl_wave_sum(x);
    const double mean = n > 0.0 ? s / n : 0.0;
    const double dv = live ? x - mean : 0.0;
    const double m2 = pl_wave_sum(dv * dv);
    if (lane == 0) { sh[w * 3 + 0] = n; sh[w * 3 + 1] = mean; sh[w * 3 + 2] = m2; }
    __syncthreads();
    c = 0.0; m = 0.0; M = 0.0;
    for (int k = 0; k < PL_WAVES; k++) chan_merge(c, m, M, sh[k * 3 + 0], sh[k * 3 + 1], sh[k * 3 + 2]);
}

// What a row of either policy loss (this one and the gSDE one below) reads besides its head's own input, and the header's lines that
// do not depend on the head: they stand here once.
struct PlIn { double v, adv, ret, old, ov; };        // value, advantage, return, old log-prob (PPO), old value (PTG_LOSS_CLIP_VF)

template <typename IN>
__device__ __forceinline__ bool pl_load(const LossArgs& a, size_t i, PlIn& x)      // true: one of the five is not finite
{
    x.v = (double)((const IN*)a.val)[i * a.v_s];
    x.adv = (double)((const IN*)a.adv)[i]; x.ret = (double)((const IN*)a.ret)[i];
    x.old = a.kind == PTG_LOSS_PPO ? (double)((const IN*)a.old_lp)[i] : 0.0;
    x.ov = (a.flags & PTG_LOSS_CLIP_VF) ? (double)((const IN*)a.old_val)[i] : 0.0;
    return !pl_finite(x.v) || !pl_finite(x.adv) || !pl_finite(x.ret) || !pl_finite(x.old) || !pl_finite(x.ov);
}

// PPO's log-ratio and ratio of a row with log-probability lp (A2C: 0 and 1); true: the ratio overflows (Ah * r would be Inf, or NaN where Ah is 0)
__device__ __forceinline__ bool pl_ratio(const LossArgs& a, const PlIn& x, double lp, double& d, double& r)
{
    d = 0.0; r = 1.0;
    if (a.kind != PTG_LOSS_PPO) return false;
    d = lp - x.old;
    r = exp(d);
    return !pl_finite(r);
}

// the advantage, PPO / A2C and value lines of a good row: fills surr, q, kl and cf of t, returns the surrogate's derivative g and
// through gv d loss / d value
__device__ __forceinline__ double pl_lines(const LossArgs& a, const PlIn& x, double lp, double d, double r, bool norm, double mean, double den,
                                           PlRow& t, double& gv)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double ah = norm ? (x.adv - mean) / den : x.adv;
    double g;
    if (a.kind == PTG_LOSS_PPO) {
        const double lo = 1.0 - a.eps, hi = 1.0 + a.eps;
        const double c = r < lo ? lo : (r > hi ? hi : r);
        const double t1 = ah * r, t2 = ah * c;
        t.surr = (t1 != t1 || t2 != t2) ? nan : (t2 < t1 ? t2 : t1);
        g = (t1 < t2 || (r >= lo && r <= hi)) ? t1 : 0.0;
        t.kl = (r - 1.0) - d;
        t.cf = fabs(r - 1.0) > a.eps ? 1.0 : 0.0;
    } else {
        t.surr = ah * lp;
        g = ah;
    }
    double vh = x.v;
    bool pass = true;
    if (a.flags & PTG_LOSS_CLIP_VF) {
        const double dv = x.v - x.ov;
        const double cl = dv < -a.eps_v ? -a.eps_v : (dv > a.eps_v ? a.eps_v : dv);
        vh = x.ov + cl;
        pass = dv >= -a.eps_v && dv <= a.eps_v;
    }
    const double dq = x.ret - vh;
    t.q = dq * dq;
    const double h = pass ? 2.0 * (vh - x.ret) : 0.0;
    gv = (a.vf_coef * h) / (double)a.B;
    return g;
}

// One row: its gradients are stored, its terms returned.  mean / den: the advantage moments in use (den = std + 1e-8).
template <typename IN>
__device__ __forceinline__ PlRow pl_row(const LossArgs& a, size_t i, bool norm, double mean, double den)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const PlRow poison{nan, nan, nan, nan, nan, nan};
    const double Bd = (double)a.B;
    const bool cat = a.head == PTG_HEAD_CATEGORICAL;
    const int A = a.A;
    long long act = 0;
    if (cat) {
        act = a.act_kind == PTG_ACT_I64 ? ((const long long*)a.act)[i] : (long long)((const int*)a.act)[i];
        if (act < 0 || act >= (long long)A) { a.err[4] = 1; return poison; }      // never an address; the row's gradients stay as they were
    }
    PlIn x;
    bool bad = pl_load<IN>(a, i, x);
    IN* const g_row = (IN*)a.g_in + i * a.g_s;
    const IN* __restrict__ row = (const IN*)a.in + i * a.s_n;
    double lp = 0.0, H = 0.0, m = 0.0, s = 1.0, log_s = 0.0, z = 0.0, sigma = 1.0;
    if (cat) {
        m = (double)row[0];
        bad = bad || m != m;
        for (int j = 1; j < A; j++) {
            const double l = (double)row[j];
            bad = bad || l != l;
            if (l > m) m = l;
        }
        bad = bad || !pl_finite(m);                          // +Inf somewhere, or -Inf everywhere
        if (!bad) {
            s = 0.0;
            for (int j = 0; j < A; j++) s += exp((double)row[j] - m);
            log_s = log(s);
            double ent = 0.0;
            for (int j = 0; j < A; j++) {
                const double d = (double)row[j] - m;
                const double ej = exp(d);
                const double lpj = d - log_s;
                if (ej != 0.0) ent += (ej / s) * lpj;
                if (j == (int)act) lp = lpj;
            }
            H = -ent;
        }
    } else {
        const double mu = (double)row[0], ls = (double)((const IN*)a.log_std)[0], smp = (double)((const IN*)a.act)[i];
        bad = bad || !pl_finite(mu) || !(ls <= PL_DBL_MAX);   // NaN or Inf mean; NaN or +Inf log_std
        sigma = exp(ls);
        z = (smp - mu) / sigma;
        lp = ((-(z * z) / 2.0) - ls) - 0.9189385332046727;
        H = 1.4189385332046727 + ls;
    }
    bad = bad || !pl_finite(lp);                             // an action of probability 0 (a -Inf logit, a zero sigma), a non-finite sample
    double d, r;
    bad = pl_ratio(a, x, lp, d, r) || bad;
    IN* const g_v = (IN*)a.g_val + i * a.gv_s;
    if (bad) {
        if (cat) { for (int j = 0; j < A; j++) g_row[j] = (IN)nan; } else g_row[0] = (IN)nan;
        g_v[0] = (IN)nan;
        a.err[5] = 1;
        return poison;
    }
    PlRow t{0.0, 0.0, H, 0.0, 0.0, 0.0};
    double gv;
    const double g = pl_lines(a, x, lp, d, r, norm, mean, den, t, gv);
    g_v[0] = (IN)gv;
    if (cat) {
        for (int j = 0; j < A; j++) {
            const double d = (double)row[j] - m;
            const double ej = exp(d);
            const double p = ej / s;
            double gr = (-g) * ((j == (int)act ? 1.0 : 0.0) - p);
            if (ej != 0.0) gr = gr + a.ent_coef * (p * ((d - log_s) + H));      // the entropy term of a probability-0 column is left out, as in H
            g_row[j] = (IN)(gr / Bd);
        }
    } else {
        g_row[0] = (IN)(((-g) * (z / sigma)) / Bd);
        t.gls = g * ((z * z) - 1.0);
    }
    return t;
}

// the sums of a whole batch -> the eight statistics and the log_std gradient; one thread
template <typename IN>
__device__ __forceinline__ void pl_finish(const LossArgs& a, const double* sum, double mean, double sd)
{
    const double Bd = (double)a.B;
    const double pl = -(sum[0] / Bd), vl = sum[1] / Bd, el = -(sum[2] / Bd);
    a.stats[0] = (pl + a.ent_coef * el) + a.vf_coef * vl;
    a.stats[1] = pl; a.stats[2] = vl; a.stats[3] = el;
    a.stats[4] = sum[3] / Bd; a.stats[5] = sum[4] / Bd;
    a.stats[6] = mean; a.stats[7] = sd;
    if (a.g_ls) ((IN*)a.g_ls)[0] = (IN)((-(sum[5]) / Bd) - a.ent_coef);
}

// the block's sums of PL_TERMS values: a shuffle tree per wave, then the waves in wave order (thread 0 holds the result)
__device__ __forceinline__ void pl_block_sum(double* v, double* sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PL_TERMS; k++) {
        v[k] = pl_wave_sum(v[k]);
        if (lane == 0) sh[w * PL_PITCH + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < PL_TERMS; k++) {
            double s = sh[k];
            for (int q = 1; q < PL_WAVES; q++) s += sh[q * PL_PITCH + k];
            v[k] = s;
        }
    }
}

// how every row kernel of a loss ends: the block's sums, then on thread 0 either the statistics (ONE: the block is the whole batch;
// fin(v) is the loss's *_finish) or the block's partial for k_loss_final.  Every thread of the block calls it.
template <bool ONE, typename FIN>
__device__ __forceinline__ void loss_tail(double* v, double* sh, double* part, FIN fin)
{
    pl_block_sum(v, sh);
    if (threadIdx.x == 0) {
        if (ONE) fin(v);
        else {
            double* p = part + (size_t)blockIdx.x * PL_PITCH;
#pragma unroll
            for (int k = 0; k < PL_TERMS; k++) p[k] = v[k];
        }
    }
}

// the last launch of a loss of more than one block, one block: step 3 of the order above, then FIN()(a, v) -- the loss's *_finish --
// on thread 0.  A: the loss's launch arguments (their nblk is read), part: where the row kernel left its partials.
// ---- grouped launches (include/ptg_env.h, ptg_policy_loss_group and ptg_optim_step_group) ----------------------
// Up to PTG_TRAIN_GROUP_MAX calls in the launches of one: the single kernels' by-value arguments side by side in the kernel arguments
// (eight LossArgs: 1 664 bytes, eight OptArgs: 1 088 bytes, of the 4 096 a launch takes), the member a grid dimension.  A kernel
// that serves both is ONE text with the argument type as its last template parameter, ARGS: the call's own arguments (the default:
// the single call's instantiation, whose code is what it was before the parameter existed, profiles/train_group_resources.txt) or a
// TrainGroup of them, of which train_member picks the block's.  m[i] is read out of the kernel-argument segment at a computed offset,
// no private copy.  Nothing is reduced across members and a member's sums run in the order its own call gives them: a member's bits
// are those of its own call.
template <typename T>
struct TrainGroup {
    T m[PTG_TRAIN_GROUP_MAX];
};
template <typename A>
__device__ __forceinline__ const A& train_member(const A& a, unsigned) { return a; }
template <typename A>
__device__ __forceinline__ const A& train_member(const TrainGroup<A>& g, unsigned i) { return g.m[i]; }

// ARGS = TrainGroup<A>: one block per member, and the partials are where FIN::partials(a) says (`part` is not read)
template <typename A, typename FIN, typename ARGS = A>
__global__ void __launch_bounds__(PL_BLOCK)
k_loss_final(ARGS args, const double* part)
{
    const A& a = train_member(args, blockIdx.x);
    if constexpr (!std::is_same<ARGS, A>::value) part = FIN::partials(a);
    __shared__ double sh[PL_WAVES * PL_PITCH];
    double v[PL_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < a.nblk; b += PL_BLOCK) {
#pragma unroll
        for (int k = 0; k < PL_TERMS; k++) v[k] += part[(size_t)b * PL_PITCH + k];
    }
    pl_block_sum(v, sh);
    if (threadIdx.x == 0) FIN()(a, v);
}

// where the policy loss keeps its row partials: behind the merged moments and the moment partials
__host__ __device__ __forceinline__ double* pl_partials(const LossArgs& a) { return a.ws + 4 + (size_t)a.nblk * 3; }

// blockIdx.x is the block within the batch, blockIdx.y (grouped) the member; the members agree in batch, so no block is surplus
template <typename IN, typename ARGS = LossArgs>
__global__ void __launch_bounds__(PL_BLOCK)
k_pl_moments(ARGS args)
{
    const LossArgs& a = train_member(args, blockIdx.y);
    __shared__ double sh[PL_WAVES * 3];
    const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    double c, m, M;
    pl_block_moments<IN>(a, i, i < a.B, sh, c, m, M);
    if (threadIdx.x == 0) {
        double* p = a.ws + 4 + (size_t)blockIdx.x * 3;
        p[0] = c; p[1] = m; p[2] = M;
    }
}

// ONE: the whole batch is this block (B <= PL_BLOCK): moments, rows and statistics in one launch.  Otherwise the moments come
// merged from the workspace and the block leaves its partial sums there for k_loss_final.
template <typename IN, bool ONE, typename ARGS = LossArgs>
__global__ void __launch_bounds__(PL_BLOCK)
k_pl_rows(ARGS args)
{
    const LossArgs& a = train_member(args, blockIdx.y);
    __shared__ double sh[PL_WAVES * PL_PITCH];
    const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    const bool live = i < a.B;                               // the ragged last wave: no row, zero terms, but it takes part in the trees
    const bool norm = (a.flags & PTG_LOSS_NORM_ADV) != 0 && a.B > 1;
    double mean = 0.0, sd = 1.0;
    if (norm) {
        double c, m, M;
        if (ONE) { pl_block_moments<IN>(a, i, live, sh, c, m, M); __syncthreads(); }
        else { c = a.ws[0]; m = a.ws[1]; M = a.ws[2]; }
        mean = m;
        sd = sqrt(M / ((double)a.B - 1.0));                  // torch.std: the unbiased one
    }
    PlRow t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) t = pl_row<IN>(a, i, norm, mean, sd + 1e-8);
    double v[PL_TERMS] = {t.surr, t.q, t.H, t.kl, t.cf, t.gls};
    loss_tail<ONE>(v, sh, pl_partials(a), [&](const double* s) { pl_finish<IN>(a, s, mean, sd); });
}

template <typename IN>
struct PlFinal {                         // mean and sd once more from the merged moments, as k_pl_rows<IN, false> has them
    __device__ static const double* partials(const LossArgs& a) { return pl_partials(a); }
    __device__ void operator()(const LossArgs& a, const double* v) const
    {
        const bool norm = (a.flags & PTG_LOSS_NORM_ADV) != 0 && a.B > 1;
        pl_finish<IN>(a, v, norm ? a.ws[1] : 0.0, norm ? sqrt(a.ws[2] / ((double)a.B - 1.0)) : 1.0);
    }
};

static_assert(sizeof(TrainGroup<LossArgs>) == 8 * 208 && sizeof(TrainGroup<LossArgs>) + sizeof(const double*) <= 4096, "the launch takes 4 096 bytes of kernel arguments");

// k_vn_merge's merge with the member as the block index: one wave per member merges its moment partials into its ws[0..2]
__global__ void __launch_bounds__(64)
k_pl_merge_group(const TrainGroup<LossArgs> g)
{
    const LossArgs& a = g.m[blockIdx.x];
    vn_merge_step(a.ws + 4, a.nblk, a.ws, 0);
}

// ================================================================================== gSDE: the state-dependent exploration head and its loss
// SB3's StateDependentNoiseDistribution with its on-policy defaults (include/ptg_env.h, ptg_sde_*, states the lines;
// tests/sde_restatement.py restates them in NumPy).  The work is per (row, latent unit), so a row is a WAVE here, not a lane: lane l
// owns the units k = l, l + 64, ... < L <= 1024, at most SDE_MAX_J = 16 of them, which it keeps in registers between the row's
// reductions and its gradient pass -- the loops over j are unrolled to NJ = 4 | 8 | 16 (the kernels' template axis), so no register
// array is indexed dynamically.  A row's loads are 64 consecutive elements per j.  Row sums: the lane's own terms ascending in j from
// 0.0, then pl_wave_sum.  s_k * s_k never costs an exp per (row, k): the head's workgroup computes it once into LDS and walks its
// rows, the loss reads it as float64 [L] from the workspace, where a leading kernel left it.
constexpr int SDE_MAX_J = PTG_MLP_MAX_WIDTH / 64, SDE_WAVES = 4, SDE_BLOCK = 64 * SDE_WAVES;
constexpr int SDE_MAX_BLOCKS = 1024;     // of the head and of the loss's row kernel: beyond that a wave walks more rows

// rows a wave of the row kernels walks: 1 up to 4 096 rows, so that a small batch spreads over the CUs
__host__ __device__ __forceinline__ size_t sde_rows_per_wave(size_t rows) { return (rows - 1) / ((size_t)SDE_WAVES * SDE_MAX_BLOCKS) + 1; }

struct SdeNoiseArgs {                    // by value in the launch
    const void* log_std;
    void* E; size_t e_s;                 // elements
    const unsigned long long* counter;
    unsigned long long seed;
    long long env_offset;
    size_t N, rows_per_block;
    int L;
    int* err;
};

// E[e][k] = exp(log_std[k]) * z(seed, c, (global env) * 1024 + k): one wave per 64 columns and run of rows, so that a lane takes
// its column's exp once and its stores are 64 consecutive elements
template <typename IN>
__global__ void __launch_bounds__(64)
k_sde_resample(SdeNoiseArgs a)
{
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (k >= a.L) return;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double ls = (double)((const IN*)a.log_std)[k];
    const bool bad = !(ls <= PL_DBL_MAX);                    // NaN or +Inf
    if (bad) a.err[5] = 1;
    const double s = exp(ls);
    const unsigned long long c = a.counter[0];
    const size_t e0 = (size_t)blockIdx.y * a.rows_per_block;
    const size_t e1 = e0 + a.rows_per_block < a.N ? e0 + a.rows_per_block : a.N;
    IN* const E = (IN*)a.E;
    for (size_t e = e0; e < e1; e++) {
        const unsigned long long key = (unsigned long long)(a.env_offset + (long long)e) * (unsigned long long)PTG_MLP_MAX_WIDTH + (unsigned long long)k;
        const double z = rb_draw_normal(rb_draw_word(a.seed, c, key));
        E[e * a.e_s + (size_t)k] = (IN)(bad ? nan : s * z);
    }
}

struct SdeActArgs {                      // by value in the launch
    const void* mean; size_t m_s;        // elements
    const void* lat; size_t lat_s;
    const void* E; size_t e_s;           // null when deterministic
    const void* log_std;
    void *act, *raw, *logp, *ent;
    double lo, hi;
    size_t N, rows_per_wave;
    int L;
    int* err;
};

template <typename IN, int NJ>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_act(SdeActArgs a)
{
    __shared__ double sh_s2[PTG_MLP_MAX_WIDTH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int ls_bad = 0;
    for (int k = threadIdx.x; k < L; k += SDE_BLOCK) {
        const double ls = (double)((const IN*)a.log_std)[k];
        ls_bad |= !(ls <= PL_DBL_MAX);                       // NaN or +Inf: every row is bad
        const double s = exp(ls);
        sh_s2[k] = s * s;
    }
    ls_bad = __syncthreads_or(ls_bad);
    double s2[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) s2[j] = lane + 64 * j < L ? sh_s2[lane + 64 * j] : 0.0;
    const IN* const lat = (const IN*)a.lat; const IN* const E = (const IN*)a.E;
    IN* const raw_o = (IN*)a.raw; IN* const logp_o = (IN*)a.logp; IN* const ent_o = (IN*)a.ent;
    const size_t base = (size_t)blockIdx.x * (a.rows_per_wave * SDE_WAVES);
    for (size_t t = 0; t < a.rows_per_wave; t++) {
        const size_t e = base + t * SDE_WAVES + (size_t)w;
        if (e >= a.N) break;                                 // wave-uniform: the ragged end
        double vp = 0.0, np = 0.0;
        bool h_bad = false;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            if (k < L) {
                const double h = (double)lat[e * a.lat_s + (size_t)k];
                h_bad = h_bad || !pl_finite(h);
                vp += (h * h) * s2[j];
                if (E) np += h * (double)E[e * a.e_s + (size_t)k];
            }
        }
        const double V = pl_wave_sum(vp) + 1e-6;
        const double noise = E ? pl_wave_sum(np) : 0.0;
        const bool bad_lat = __ballot(h_bad) != 0ull;
        const double mu = (double)((const IN*)a.mean)[e * a.m_s];
        const bool bad = ls_bad || bad_lat || !pl_finite(mu);
        const double lsd = log(sqrt(V));
        const double g = mu + noise;
        const double x = g < a.lo ? a.lo : (g > a.hi ? a.hi : g);
        if (lane == 0) {                                     // the row's scalars are the same on every lane; one of them stores
            ((float*)a.act)[e] = bad ? 0.0f : (float)x;
            if (raw_o) raw_o[e] = (IN)(bad ? nan : g);
            if (logp_o) logp_o[e] = (IN)(bad ? nan : (((-(noise * noise)) / (2.0 * V)) - lsd) - 0.9189385332046727);
            if (ent_o) ent_o[e] = (IN)(bad ? nan : 1.4189385332046727 + lsd);
            if (bad) a.err[5] = 1;
        }
    }
}

// The loss.  The row kernel reads the latent once: a wave walks its rows ascending (rows base + w, base + w + 4, ...), adds c_i * h_ik^2
// to its columns' partials in registers, the block's four waves meet in LDS in wave order and the block leaves one [L] partial, which
// k_sde_cols adds over the blocks ascending.  The five means go the way of every loss here (loss_tail, k_loss_final): a wave's sums
// sit on its lane 0 with zeroes beside them, so pl_block_sum's tree returns them unchanged.  The block count is given by B alone.
struct SdeLossArgs {                     // by value in the launch
    LossArgs l;                          // mean as `in`, the stored samples as `act`, log_std [L]; head, A, act_kind are not read
    const void* lat; size_t lat_s;       // elements
    void* g_lat; size_t gl_s;            // null: no latent gradient
    const double* s2;                    // float64 [L] in the workspace
    double *row_part, *col_part;         // [nblk][PL_PITCH], [nblk][L]
    size_t rows_per_wave;
    int L, nblk;                         // blocks of the row kernel (l.nblk: of the moments)
};

// the workspace, in doubles: [0..2] merged moments, [4 ..) moment partials [l.nblk][3], s2 [L], row partials [nblk][PL_PITCH], column partials [nblk][L]
__host__ __device__ __forceinline__ double* sde_s2(const LossArgs& l) { return l.ws + 4 + (size_t)l.nblk * 3; }

// The column-partial tail of a row kernel (the loss's and the squashed head's backward): a lane holds its units' sums over the rows its
// wave walked; the block's waves meet in LDS in wave order and the block leaves one [L] partial.  sde_col_sum adds column k's
// partials over the blocks ascending.
template <int NJ>
__device__ __forceinline__ void sde_col_tail(const double (&acc)[NJ], double* sh_col, double* col_part, int L, int lane, int w)
{
    for (int q = 0; q < SDE_WAVES; q++) {
        if (w == q) {
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int k = lane + 64 * j;
                if (k < L) sh_col[k] = q == 0 ? acc[j] : sh_col[k] + acc[j];
            }
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < L; k += SDE_BLOCK) col_part[(size_t)blockIdx.x * (size_t)L + (size_t)k] = sh_col[k];
}

__device__ __forceinline__ double sde_col_sum(const double* col_part, int nblk, int L, int k)
{
    double s = col_part[k];
    for (int b = 1; b < nblk; b++) s += col_part[(size_t)b * (size_t)L + (size_t)k];
    return s;
}

template <typename IN>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_s2(const void* log_std, int L, double* s2)
{
    const int k = (int)blockIdx.x * SDE_BLOCK + (int)threadIdx.x;
    if (k >= L) return;
    const double ls = (double)((const IN*)log_std)[k];
    const double s = exp(ls);
    s2[k] = !(ls <= PL_DBL_MAX) ? __longlong_as_double(0x7FF8000000000000ll) : s * s;       // NaN or +Inf: V, and with it every row, is not finite
}

template <typename IN, int NJ>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_rows(SdeLossArgs a)
{
    __shared__ double sh[PL_WAVES * PL_PITCH];
    __shared__ double sh_col[PTG_MLP_MAX_WIDTH];
    static_assert(SDE_WAVES == PL_WAVES && SDE_BLOCK == PL_BLOCK, "loss_tail serves a block of PL_WAVES waves");
    const LossArgs& l = a.l;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double Bd = (double)l.B;
    const bool norm = (l.flags & PTG_LOSS_NORM_ADV) != 0 && l.B > 1;
    const double mean = norm ? l.ws[1] : 0.0, sd = norm ? sqrt(l.ws[2] / (Bd - 1.0)) : 1.0;
    double s2[NJ], acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) { s2[j] = lane + 64 * j < L ? a.s2[lane + 64 * j] : 0.0; acc[j] = 0.0; }
    const IN* const lat = (const IN*)a.lat;
    IN* const g_lat = (IN*)a.g_lat;
    PlRow sum{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t base = (size_t)blockIdx.x * (a.rows_per_wave * SDE_WAVES);
    for (size_t t = 0; t < a.rows_per_wave; t++) {
        const size_t i = base + t * SDE_WAVES + (size_t)w;
        if (i >= l.B) break;                                 // wave-uniform: the ragged end
        double h[NJ], hh[NJ], vp = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            h[j] = k < L ? (double)lat[i * a.lat_s + (size_t)k] : 0.0;
            hh[j] = h[j] * h[j];
            vp += hh[j] * s2[j];
        }
        const double V = pl_wave_sum(vp) + 1e-6;             // a non-finite latent entry or s2 makes it non-finite, whatever meets it
        // the row's scalars, the same on every lane
        PlIn x;
        bool bad = pl_load<IN>(l, i, x);
        const double mu = (double)((const IN*)l.in)[i * l.s_n], smp = (double)((const IN*)l.act)[i];
        bad = bad || !pl_finite(mu) || !pl_finite(V);
        const double lsd = log(sqrt(V));
        const double dm = smp - mu;
        const double lp = (((-(dm * dm)) / (2.0 * V)) - lsd) - 0.9189385332046727;
        bad = bad || !pl_finite(lp);                         // a non-finite sample
        double d, r;
        bad = pl_ratio(l, x, lp, d, r) || bad;
        PlRow tr{nan, nan, nan, nan, nan, 0.0};
        double g_mu = nan, gv = nan, ci = nan;
        if (!bad) {
            tr = PlRow{0.0, 0.0, 1.4189385332046727 + lsd, 0.0, 0.0, 0.0};
            const double g = pl_lines(l, x, lp, d, r, norm, mean, sd + 1e-8, tr, gv);
            g_mu = ((-g) * (dm / V)) / Bd;
            ci = (((-g) * (((dm * dm) / V) - 1.0)) - l.ent_coef) / (2.0 * V);
        }
        sum.surr += tr.surr; sum.q += tr.q; sum.H += tr.H; sum.kl += tr.kl; sum.cf += tr.cf;
        if (lane == 0) {
            ((IN*)l.g_in)[i * l.g_s] = (IN)g_mu;
            ((IN*)l.g_val)[i * l.gv_s] = (IN)gv;
            if (bad) l.err[5] = 1;
        }
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            acc[j] += ci * hh[j];
            if (g_lat && k < L) g_lat[i * a.gl_s + (size_t)k] = (IN)(((ci * (2.0 * h[j])) * s2[j]) / Bd);
        }
    }
    sde_col_tail<NJ>(acc, sh_col, a.col_part, L, lane, w);
    const bool first = lane == 0;
    double v[PL_TERMS] = {first ? sum.surr : 0.0, first ? sum.q : 0.0, first ? sum.H : 0.0, first ? sum.kl : 0.0, first ? sum.cf : 0.0, 0.0};
    loss_tail<false>(v, sh, a.row_part, [](const double*) {});
}

// d loss / d log_std[k] from the blocks' column partials, ascending
template <typename IN>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_cols(SdeLossArgs a, void* g_ls)
{
    const int k = (int)blockIdx.x * SDE_BLOCK + (int)threadIdx.x;
    if (k >= a.L) return;
    const double s = sde_col_sum(a.col_part, a.nblk, a.L, k);
    ((IN*)g_ls)[k] = (IN)(((2.0 * a.s2[k]) * s) / (double)a.l.B);
}

template <typename IN>
struct SdeFinal {                        // the eight statistics; the log_std gradient is k_sde_cols'
    __device__ void operator()(const SdeLossArgs& a, const double* v) const
    {
        LossArgs l = a.l;
        l.g_ls = nullptr;
        PlFinal<IN>()(l, v);
    }
};

// ---- gSDE for SAC / TQC: the squashed head's reparametrised sample and its backward (include/ptg_env.h, ptg_sde_rsample, states the
// lines; tests/sde_squash_restatement.py restates them).  The forward is k_sde_act's shape: a wave per row, s_k * s_k once per
// workgroup in LDS -- the target's pass and the collecting head have no workspace, and at a replay batch a leading launch would cost
// more than the workgroup's L exps.  With one shared row the lane keeps its E entries in registers across its rows.  The backward
// has a workspace for its column partials anyway, so k_sde_s2 leaves s_k * s_k there as it does for the loss, and the row kernel needs
// no reduction over k at all: (noise, V) come from the forward, every line of a row is a lane's own but the bad-latent ballot.
struct SdeRsArgs {                       // by value in the launch
    const void* mean; size_t m_s;        // elements
    const void* lat; size_t lat_s;
    const void* E; size_t e_s;           // null when deterministic
    const void* log_std;                 // forward
    const double* s2;                    // backward: float64 [L] in the workspace
    void *act, *logp;
    float* step_act;
    double* saved;                       // [B][2]: noise, V
    const void *g_act, *g_logp;
    void* g_mean; size_t gm_s;
    void* g_lat; size_t gl_s;
    double* col_part;                    // [nblk][L]; null: no log_std gradient
    double c;                            // clip_mean
    size_t B, rows_per_wave;
    int L, nblk, shared;
    int* err;
};

__device__ __forceinline__ double sde_hardtanh(double mu, double c) { return mu < -c ? -c : (mu > c ? c : mu); }      // a NaN falls through

template <typename IN, int NJ>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_rs_fwd(SdeRsArgs a)
{
    __shared__ double sh_s2[PTG_MLP_MAX_WIDTH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int ls_bad = 0;
    for (int k = threadIdx.x; k < L; k += SDE_BLOCK) {
        const double ls = (double)((const IN*)a.log_std)[k];
        ls_bad |= !(ls <= PL_DBL_MAX);                       // NaN or +Inf: every row is bad
        const double s = exp(ls);
        sh_s2[k] = s * s;
    }
    ls_bad = __syncthreads_or(ls_bad);
    const IN* const lat = (const IN*)a.lat; const IN* const E = (const IN*)a.E;
    const bool shared = a.shared != 0;
    double s2[NJ], es[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int k = lane + 64 * j;
        s2[j] = k < L ? sh_s2[k] : 0.0;
        es[j] = (shared && k < L) ? (double)E[k] : 0.0;
    }
    IN* const act_o = (IN*)a.act; IN* const logp_o = (IN*)a.logp;
    const size_t base = (size_t)blockIdx.x * (a.rows_per_wave * SDE_WAVES);
    for (size_t t = 0; t < a.rows_per_wave; t++) {
        const size_t i = base + t * SDE_WAVES + (size_t)w;
        if (i >= a.B) break;                                 // wave-uniform: the ragged end
        double vp = 0.0, np = 0.0;
        bool h_bad = false;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            if (k < L) {
                const double h = (double)lat[i * a.lat_s + (size_t)k];
                h_bad = h_bad || !pl_finite(h);
                vp += (h * h) * s2[j];
                if (E) np += h * (shared ? es[j] : (double)E[i * a.e_s + (size_t)k]);
            }
        }
        const double V = pl_wave_sum(vp) + 1e-6;
        const double noise = E ? pl_wave_sum(np) : 0.0;
        const bool bad_lat = __ballot(h_bad) != 0ull;
        const double mu = (double)((const IN*)a.mean)[i * a.m_s];
        const bool bad = ls_bad || bad_lat || !pl_finite(mu) || !pl_finite(V) || !pl_finite(noise);
        const double m = sde_hardtanh(mu, a.c);
        const double lsd = log(sqrt(V));
        const double g = m + noise;
        const double x = tanh(g);
        if (lane == 0) {                                     // the row's scalars are the same on every lane; one of them stores
            act_o[i] = (IN)(bad ? nan : x);
            if (a.step_act) a.step_act[i] = bad ? 0.0f : (float)x;
            if (logp_o) logp_o[i] = (IN)(bad ? nan : ((((-(noise * noise)) / (2.0 * V)) - lsd) - 0.9189385332046727) - log((1.0 - x * x) + 1e-6));
            if (a.saved) { a.saved[2 * i] = noise; a.saved[2 * i + 1] = V; }
            if (bad) a.err[5] = 1;
        }
    }
}

template <typename IN, int NJ>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_rs_bwd(SdeRsArgs a)
{
    __shared__ double sh_col[PTG_MLP_MAX_WIDTH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const IN* const lat = (const IN*)a.lat; const IN* const E = (const IN*)a.E;
    IN* const g_lat = (IN*)a.g_lat;
    const bool shared = a.shared != 0;
    double s2[NJ], es[NJ], acc[NJ];
    bool s_bad = false;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int k = lane + 64 * j;
        s2[j] = k < L ? a.s2[k] : 0.0;
        s_bad = s_bad || s2[j] != s2[j];                     // k_sde_s2's NaN: a NaN or +Inf log_std, every row is bad
        es[j] = (shared && k < L) ? (double)E[k] : 0.0;
        acc[j] = 0.0;
    }
    const bool ls_bad = __ballot(s_bad) != 0ull;
    const size_t base = (size_t)blockIdx.x * (a.rows_per_wave * SDE_WAVES);
    for (size_t t = 0; t < a.rows_per_wave; t++) {
        const size_t i = base + t * SDE_WAVES + (size_t)w;
        if (i >= a.B) break;                                 // wave-uniform: the ragged end
        // the row's scalars, the same on every lane
        const double mu = (double)((const IN*)a.mean)[i * a.m_s], noise = a.saved[2 * i], V = a.saved[2 * i + 1];
        const double ga = a.g_act ? (double)((const IN*)a.g_act)[i] : 0.0, gl = a.g_logp ? (double)((const IN*)a.g_logp)[i] : 0.0;
        double h[NJ];
        bool h_bad = false;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            h[j] = k < L ? (double)lat[i * a.lat_s + (size_t)k] : 0.0;
            h_bad = h_bad || !pl_finite(h[j]);
        }
        const bool bad = ls_bad || __ballot(h_bad) != 0ull || !pl_finite(mu) || !pl_finite(noise) || !pl_finite(V) || !pl_finite(ga) || !pl_finite(gl);
        const double x = tanh(sde_hardtanh(mu, a.c) + noise);
        const double d = 1.0 - x * x;
        const double q = ((2.0 * x) * d) / (d + 1e-6);
        const double tt = ga * d + gl * q;
        const double n = bad ? nan : tt - gl * (noise / V);
        const double cV = bad ? nan : (gl * (((noise * noise) / V) - 1.0)) / (2.0 * V);
        if (lane == 0) {
            ((IN*)a.g_mean)[i * a.gm_s] = (IN)(bad ? nan : ((-a.c < mu && mu < a.c) ? tt : 0.0));
            if (bad) a.err[5] = 1;
        }
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int k = lane + 64 * j;
            const double e = E ? (shared ? es[j] : (k < L ? (double)E[i * a.e_s + (size_t)k] : 0.0)) : 0.0;
            const double gh = (n * e) + ((cV * (2.0 * h[j])) * s2[j]);
            acc[j] += h[j] * gh;
            if (g_lat && k < L) g_lat[i * a.gl_s + (size_t)k] = (IN)gh;
        }
    }
    if (a.col_part) sde_col_tail<NJ>(acc, sh_col, a.col_part, L, lane, w);
}

// d loss / d log_std[k] of the squashed head from the blocks' column partials, ascending
template <typename IN>
__global__ void __launch_bounds__(SDE_BLOCK)
k_sde_rs_cols(const double* col_part, int nblk, int L, void* g_ls)
{
    const int k = (int)blockIdx.x * SDE_BLOCK + (int)threadIdx.x;
    if (k >= L) return;
    ((IN*)g_ls)[k] = (IN)sde_col_sum(col_part, nblk, L, k);
}

// ================================================================================== the optimiser step
// What runs behind loss.backward() (include/ptg_env.h, ptg_optim_step, states the lines; tests/optim_restatement.py restates them in
// NumPy): torch's clip_grad_norm_, the single-tensor lines of torch.optim.Adam / RMSprop, SB3's polyak_update and zero_grad, for ALL
// parameter tensors of an optimiser in a chain of launches whose length does not depend on the tensor count.  The tensor list lives in
// two caller-owned device tables: one ptg_optim_tensor per tensor, one ptg_optim_span per chunk of OPT_CHUNK consecutive elements of
// one tensor.  One workgroup owns one chunk; thread t owns its elements 4 t .. 4 t + 3 -- one 16-byte piece in float32, two in float64
// -- and moves them as such when every base of the chunk is 16-byte aligned, else element by element (a view at an odd offset of a flat
// buffer).  Arithmetic in float64 whatever the tensors' type, rounded once on the store.
//   k_optim_norm    sum of g * g per chunk: the lane's four terms in order, a shuffle tree, the four waves in wave order -> ws[4 + chunk]
//   k_optim_head    one block: the partials in an order given by the chunk count alone -> total norm, clip coefficient; advances the
//                   step count and the running beta products; writes the float64 scalars k_optim_update reads.  A kernel of its own,
//                   so that no block of the update can meet a half-advanced state
//   k_optim_update  clip, moments, parameter, target, zeroed gradient: every element read once and written once
// No floating-point atomics, no grid-wide wait: the same inputs give the same bits.
constexpr int OPT_BLOCK = 256, OPT_PER = 4, OPT_CHUNK = OPT_BLOCK * OPT_PER, OPT_WAVES = OPT_BLOCK / 64, OPT_WS_HEAD = 4;

struct OptArgs {                         // by value in the launch: a captured call holds no host memory
    const ptg_optim_tensor* tensors;
    const ptg_optim_span* chunks;
    double* ws;                          // [0] clip coefficient, [1] step size, [2] sqrt(1 - beta2^t), [3] spare; [4 ..) one partial per chunk
    double* state;                       // {t, beta1^t, beta2^t, spare}
    const double* lr_dev;
    double* norm;
    double lr, b1, b2, eps, alpha, tau, max_norm;
    long long n_tensors;
    unsigned n_chunks;
    int kind, flags;
    int* err;
};

// the chunk of this block: false when its record names no tensor of the table or an offset that is no multiple of OPT_CHUNK (never an
// address; err[4])
__device__ __forceinline__ bool opt_chunk(const OptArgs& a, ptg_optim_tensor& t, size_t& e0, int& n)
{
    const ptg_optim_span c = a.chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= a.n_tensors || c.offset < 0 || c.offset % OPT_CHUNK != 0) { a.err[4] = 1; return false; }
    t = a.tensors[c.tensor];
    const size_t off = (size_t)c.offset, numel = t.numel > 0 ? (size_t)t.numel : 0;
    e0 = off + (size_t)threadIdx.x * OPT_PER;
    n = e0 < numel ? (int)min((size_t)OPT_PER, numel - e0) : 0;            // this thread's live elements: 4, or fewer in a ragged last chunk
    return true;
}

__device__ __forceinline__ bool opt_al16(const void* base) { return ((uintptr_t)base & 15u) == 0; }      // a null (unused) base passes

template <typename T>
__device__ __forceinline__ void opt_load(const void* base, size_t e0, int n, bool wide, double* x)
{
    const T* p = (const T*)base + e0;
    if (wide && n == OPT_PER) {
        if (sizeof(T) == 4) {
            const float4 q = *(const float4*)p;
            x[0] = (double)q.x; x[1] = (double)q.y; x[2] = (double)q.z; x[3] = (double)q.w;
        } else {
            const double2 q0 = ((const double2*)p)[0], q1 = ((const double2*)p)[1];
            x[0] = q0.x; x[1] = q0.y; x[2] = q1.x; x[3] = q1.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < OPT_PER; j++) x[j] = j < n ? (double)p[j] : 0.0;
    }
}

template <typename T>
__device__ __forceinline__ void opt_store(void* base, size_t e0, int n, bool wide, const double* x)
{
    T* p = (T*)base + e0;
    if (wide && n == OPT_PER) {
        if (sizeof(T) == 4) {
            *(float4*)p = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
        } else {
            ((double2*)p)[0] = make_double2(x[0], x[1]);
            ((double2*)p)[1] = make_double2(x[2], x[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < OPT_PER; j++)
            if (j < n) p[j] = (T)x[j];
    }
}

// the block's sum: a shuffle tree per wave, then the waves in wave order (thread 0 holds the result)
__device__ __forceinline__ double opt_block_sum(double v, double* sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = pl_wave_sum(v);
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        s = sh[0];
        for (int q = 1; q < OPT_WAVES; q++) s += sh[q];
    }
    return s;
}

static_assert(sizeof(TrainGroup<OptArgs>) == 8 * 136 && sizeof(TrainGroup<OptArgs>) <= 4096, "the launch takes 4 096 bytes of kernel arguments");

// Grouped (ARGS = TrainGroup<OptArgs>, above k_loss_final): the norm pass and the update run on a grid of (the largest chunk count of
// the group, members); a workgroup owns chunk blockIdx.x of member blockIdx.y, and where that member has fewer chunks it returns
// before any load and before the first barrier -- a test uniform over the workgroup.  The head kernel runs one workgroup per member.
template <typename T, typename ARGS = OptArgs>
__global__ void __launch_bounds__(OPT_BLOCK)
k_optim_norm(ARGS args)
{
    const OptArgs& a = train_member(args, blockIdx.y);
    if (!std::is_same<ARGS, OptArgs>::value && blockIdx.x >= a.n_chunks) return;
    __shared__ double sh[OPT_WAVES];
    ptg_optim_tensor t; size_t e0; int n;
    const bool ok = opt_chunk(a, t, e0, n);                  // block-uniform
    double s = 0.0;
    if (ok && n > 0) {
        double g[OPT_PER];
        opt_load<T>(t.grad, e0, n, opt_al16(t.grad), g);
#pragma unroll
        for (int j = 0; j < OPT_PER; j++) s += g[j] * g[j];  // a dead element adds +0.0
    }
    s = opt_block_sum(s, sh);
    if (threadIdx.x == 0) a.ws[OPT_WS_HEAD + blockIdx.x] = s;
}

template <typename ARGS = OptArgs>
__global__ void __launch_bounds__(OPT_BLOCK)
k_optim_head(ARGS args)
{
    const OptArgs& a = train_member(args, blockIdx.x);
    __shared__ double sh[OPT_WAVES];
    const bool clip = (a.flags & PTG_OPTIM_CLIP) != 0;
    double s = 0.0;
    if (clip)
        for (unsigned c = threadIdx.x; c < a.n_chunks; c += OPT_BLOCK) s += a.ws[OPT_WS_HEAD + c];
    s = opt_block_sum(s, sh);
    if (threadIdx.x != 0) return;
    double coef = 1.0;
    if (clip) {
        const double total = sqrt(s);
        a.norm[0] = total;
        const double c = a.max_norm / (total + 1e-6);
        coef = c > 1.0 ? 1.0 : c;                            // torch.clamp(max=1.0): a NaN stays
        if (!pl_finite(total)) a.err[5] = 1;
    }
    const double lr = a.lr_dev ? a.lr_dev[0] : a.lr;
    a.ws[0] = coef;
    if (a.kind == PTG_OPTIM_ADAM) {
        const double t = a.state[0] + 1.0, p1 = a.state[1] * a.b1, p2 = a.state[2] * a.b2;
        a.state[0] = t; a.state[1] = p1; a.state[2] = p2;
        a.ws[1] = lr / (1.0 - p1);                           // step_size = lr / bias_correction1
        a.ws[2] = sqrt(1.0 - p2);                            // bias_correction2_sqrt
    } else {
        a.state[0] = a.state[0] + 1.0;
        a.ws[1] = lr;
        a.ws[2] = 1.0;
    }
}

template <typename T, typename ARGS = OptArgs>
__global__ void __launch_bounds__(OPT_BLOCK)
k_optim_update(ARGS args)
{
    const OptArgs& a = train_member(args, blockIdx.y);
    if (!std::is_same<ARGS, OptArgs>::value && blockIdx.x >= a.n_chunks) return;
    ptg_optim_tensor t; size_t e0; int n;
    if (!opt_chunk(a, t, e0, n) || n == 0) return;
    const bool polyak = a.kind == PTG_OPTIM_POLYAK, adam = a.kind == PTG_OPTIM_ADAM;
    const bool targets = polyak || (a.flags & PTG_OPTIM_TARGETS) != 0;
    const void* s2 = adam ? t.state2 : nullptr;
    const void* tg = targets ? t.target : nullptr;
    // a chunk starts a multiple of OPT_CHUNK elements into its tensor (opt_chunk refuses any other offset) and a thread a multiple of
    // four elements into the chunk, so the tensors' bases decide the alignment of every 16-byte piece
    const bool wide = opt_al16(t.param) && opt_al16(polyak ? nullptr : t.grad) && opt_al16(polyak ? nullptr : t.state1) && opt_al16(s2) && opt_al16(tg);
    double p[OPT_PER];
    opt_load<T>(t.param, e0, n, wide, p);
    if (!polyak) {
        const double coef = a.ws[0], ss = a.ws[1], bc2 = a.ws[2];
        double g[OPT_PER], m[OPT_PER], v[OPT_PER];
        opt_load<T>(t.grad, e0, n, wide, g);
        opt_load<T>(t.state1, e0, n, wide, m);
        if (adam) opt_load<T>(t.state2, e0, n, wide, v);
        bool bad = false;
#pragma unroll
        for (int j = 0; j < OPT_PER; j++) {
            bad = bad || !pl_finite(g[j]);
            const double gp = g[j] * coef;                   // coef == 1.0 without clipping: the gradient itself
            if (adam) {
                m[j] = a.b1 * m[j] + (1.0 - a.b1) * gp;
                v[j] = a.b2 * v[j] + ((1.0 - a.b2) * gp) * gp;
                const double denom = sqrt(v[j]) / bc2 + a.eps;
                p[j] = p[j] + ((-ss) * m[j]) / denom;
            } else {                                         // RMSprop: state1 is square_avg
                m[j] = a.alpha * m[j] + ((1.0 - a.alpha) * gp) * gp;
                const double avg = sqrt(m[j]) + a.eps;
                p[j] = p[j] + ((-ss) * gp) / avg;
            }
            g[j] = 0.0;
        }
        if (bad && !(a.flags & PTG_OPTIM_CLIP)) a.err[5] = 1;      // with a norm pass the head kernel reports it: total is not finite
        opt_store<T>(t.param, e0, n, wide, p);
        opt_store<T>(t.state1, e0, n, wide, m);
        if (adam) opt_store<T>(t.state2, e0, n, wide, v);
        if (a.flags & PTG_OPTIM_ZERO_GRAD) opt_store<T>(t.grad, e0, n, wide, g);
    }
    if (targets) {
        double q[OPT_PER];
        opt_load<T>(t.target, e0, n, wide, q);
#pragma unroll
        for (int j = 0; j < OPT_PER; j++) q[j] = (1.0 - a.tau) * q[j] + a.tau * (double)(T)p[j];      // the parameter as it was just stored
        opt_store<T>(t.target, e0, n, wide, q);
    }
}

// ================================================================================== the TD losses of the off-policy algorithms
// What runs between ptg_replay_sample's batch and the gradient that goes back into the Q network(s) (include/ptg_env.h, ptg_td_loss,
// states the lines; tests/td_loss_restatement.py restates them in NumPy): the TD target, the chosen Q-value, smooth_l1_loss (DQN.train)
// or the sum of the critics' squared errors (TD3.train, SAC.train) and d loss / d Q in closed form.  One lane per row on consecutive
// rows, float64 arithmetic whatever the input types, outputs rounded once on the store.  A DQN row of next-Q values is read once,
// straight from memory as k_act and pl_row read theirs; the critics' K pointers and strides sit in the launch arguments and every loop
// over them is unrolled over PTG_TD_MAX_CRITICS with a k < K guard, so nothing per lane (and no launch argument) is indexed
// dynamically.  The reward and done columns have dtypes of their own, read behind a wave-uniform branch.  The five sums go through
// the fixed-order scheme stated above LossArgs (loss_tail, k_loss_final).
constexpr int TD_K = PTG_TD_MAX_CRITICS;

struct TdArgs {                          // by value in the launch: a captured call holds no host memory
    const void* q[TD_K]; size_t q_s[TD_K];       // elements
    const void* nq[TD_K]; size_t nq_s[TD_K];
    void* g[TD_K]; size_t g_s[TD_K];
    const void *act, *rew, *done, *lp;
    const double* alpha_dev;
    void* y;
    double* stats;
    double* ws;                          // one partial [PL_PITCH] per block
    double gamma, alpha, scale;
    size_t B;
    int A, K, kind, flags, act_kind, rew_f64, done_f64, nblk;
    int* err;
};
struct TdRow { double term, q, y, ad, ge; };      // a row's terms of the five means

__device__ __forceinline__ double td_rd(const void* p, int f64, size_t i)
{
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

// alpha as this call uses it: 0 without the entropy term; else the host double, the device scalar, or exp of it
__device__ __forceinline__ double td_alpha(const TdArgs& a)
{
    if (!(a.flags & PTG_TD_ENTROPY)) return 0.0;
    if (!a.alpha_dev) return a.alpha;
    const double s = a.alpha_dev[0];
    return (a.flags & PTG_TD_LOG_ALPHA) ? exp(s) : s;
}

template <typename IN>
__device__ __forceinline__ TdRow td_row_dqn(const TdArgs& a, size_t i)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const TdRow poison{nan, nan, nan, nan, nan};
    const int A = a.A;
    const long long act = a.act_kind == PTG_ACT_I64 ? ((const long long*)a.act)[i] : (long long)((const int*)a.act)[i];
    if (act < 0 || act >= (long long)A) { a.err[4] = 1; return poison; }      // never an address; the row's gradients and y stay as they were
    const IN* __restrict__ nrow = (const IN*)a.nq[0] + i * a.nq_s[0];
    double m = (double)nrow[0];
    for (int j = 1; j < A; j++) {
        const double l = (double)nrow[j];
        if (l > m || l != l) m = l;                          // torch.max: a NaN wins and then stays (NaN > x and x > NaN are false)
    }
    const double r = td_rd(a.rew, a.rew_f64, i), d = td_rd(a.done, a.done_f64, i);
    const double y = r + ((1.0 - d) * a.gamma) * m;
    const double qa = (double)((const IN*)a.q[0])[i * a.q_s[0] + (size_t)act];
    if (a.y) ((IN*)a.y)[i] = (IN)y;
    IN* const g_row = (IN*)a.g[0] + i * a.g_s[0];
    if (!pl_finite(y) || !pl_finite(qa)) {
        for (int j = 0; j < A; j++) g_row[j] = (IN)nan;
        a.err[5] = 1;
        return poison;
    }
    const double dl = qa - y, ad = fabs(dl);
    const double gc = (dl < -1.0 ? -1.0 : (dl > 1.0 ? 1.0 : dl)) / (double)a.B;
    for (int j = 0; j < A; j++) g_row[j] = (IN)(j == (int)act ? gc : 0.0);
    return TdRow{ad < 1.0 ? 0.5 * (dl * dl) : ad - 0.5, qa, y, ad, ad >= 1.0 ? 1.0 : 0.0};
}

template <typename IN>
__device__ __forceinline__ TdRow td_row_critics(const TdArgs& a, size_t i, double alpha)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const int K = a.K;
    double m = (double)((const IN*)a.nq[0])[i * a.nq_s[0]];
#pragma unroll
    for (int k = 1; k < TD_K; k++) {
        if (k < K) {
            const double l = (double)((const IN*)a.nq[k])[i * a.nq_s[k]];
            if (l < m || l != l) m = l;                      // th.min, the same NaN rule
        }
    }
    if (a.flags & PTG_TD_ENTROPY) m = m - alpha * (double)((const IN*)a.lp)[i];
    const double r = td_rd(a.rew, a.rew_f64, i), d = td_rd(a.done, a.done_f64, i);
    const double y = r + ((1.0 - d) * a.gamma) * m;
    double qk[TD_K];
    bool bad = !pl_finite(y);
#pragma unroll
    for (int k = 0; k < TD_K; k++) {
        qk[k] = 0.0;
        if (k < K) {
            qk[k] = (double)((const IN*)a.q[k])[i * a.q_s[k]];
            bad = bad || !pl_finite(qk[k]);
        }
    }
    if (a.y) ((IN*)a.y)[i] = (IN)y;
    if (bad) {
#pragma unroll
        for (int k = 0; k < TD_K; k++)
            if (k < K) ((IN*)a.g[k])[i * a.g_s[k]] = (IN)nan;
        a.err[5] = 1;
        return TdRow{nan, nan, nan, nan, nan};
    }
    const double c2 = a.scale * 2.0, Bd = (double)a.B;
    TdRow t{0.0, 0.0, y, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < TD_K; k++) {
        if (k < K) {
            const double dl = qk[k] - y, ad = fabs(dl);
            ((IN*)a.g[k])[i * a.g_s[k]] = (IN)((c2 * dl) / Bd);
            t.term = t.term + dl * dl;
            t.q = t.q + qk[k];
            t.ad = t.ad + ad;
            t.ge = t.ge + (ad >= 1.0 ? 1.0 : 0.0);
        }
    }
    return t;
}

// the sums of a whole batch -> the eight statistics; one thread
__device__ __forceinline__ void td_finish(const TdArgs& a, const double* sum, double alpha)
{
    const bool dqn = a.kind == PTG_TD_DQN;
    const double Bd = (double)a.B, n = dqn ? Bd : Bd * (double)a.K;
    a.stats[0] = dqn ? sum[0] / Bd : (a.scale * sum[0]) / Bd;
    a.stats[1] = sum[1] / n; a.stats[2] = sum[2] / Bd; a.stats[3] = sum[3] / n; a.stats[4] = sum[4] / n;
    a.stats[5] = alpha; a.stats[6] = 0.0; a.stats[7] = 0.0;
}

// ONE: the whole batch is this block (B <= PL_BLOCK): rows and statistics in one launch.  Otherwise the block leaves its partial sums
// in the workspace for k_loss_final.
// blockIdx.x is the block within the batch, blockIdx.y (ARGS = TrainGroup<TdArgs>, ptg_td_loss_group) the member
template <typename IN, bool DQN, bool ONE, typename ARGS = TdArgs>
__global__ void __launch_bounds__(PL_BLOCK)
k_td_rows(ARGS args)
{
    const TdArgs& a = train_member(args, blockIdx.y);
    __shared__ double sh[PL_WAVES * PL_PITCH];
    const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    const bool live = i < a.B;                               // the ragged last wave: no row, zero terms, but it takes part in the trees
    const double alpha = td_alpha(a);
    TdRow t{0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) t = DQN ? td_row_dqn<IN>(a, i) : td_row_critics<IN>(a, i, alpha);
    double v[PL_TERMS] = {t.term, t.q, t.y, t.ad, t.ge, 0.0};
    loss_tail<ONE>(v, sh, a.ws, [&](const double* s) { td_finish(a, s, alpha); });
}

struct TdFinal {
    __device__ static const double* partials(const TdArgs& a) { return a.ws; }
    __device__ void operator()(const TdArgs& a, const double* v) const { td_finish(a, v, td_alpha(a)); }
};

static_assert(sizeof(TrainGroup<TdArgs>) == 8 * 328 && sizeof(TrainGroup<TdArgs>) + sizeof(const double*) <= 4096, "the launch takes 4 096 bytes of kernel arguments");

// ================================================================================== the quantile-Huber loss of TQC's critics
// sb3_contrib's TQC.train critic lines and quantile_huber_loss(sum_over_quantiles=False) (include/ptg_env.h, ptg_quantile_loss, states
// the lines; tests/quantile_loss_restatement.py restates them): per row the K * Q next quantiles of all critics are sorted, the lowest
// M = K * (Q - d) become targets, and every current quantile meets every target in a Huber pair -- K * Q * M pairs a row, none of which
// is ever stored.  The one loss whose kernel is not "one lane per row": one WAVE per row, four rows per 256-thread block.  A wave's
// slice of LDS (QL_MAX doubles) holds the staged next quantiles, then -- in place -- the kept ones in ascending order, then the targets
// y.  The sort is a rank count: every element counts the elements that precede it under a strict total order (value, NaN last, flat
// index), so the ranks are a permutation and the kept values depend on no race.  The lanes then stride over the K * Q (k, i) pairs and
// run the j loop over the targets out of LDS (every lane reads the same address: a broadcast) in the header's order.  The K pointers
// travel by value and are picked behind an unrolled k == kk guard, as td_row_critics picks its.  A wave without a row takes every
// barrier and every tree with zero terms.  Sums: the scheme stated above LossArgs, the block's four waves being its four rows.
constexpr int QL_MAX = PTG_TD_MAX_CRITICS * PTG_QL_MAX_QUANTILES, QL_PER = QL_MAX / 64;      // 256 values a row, at most 4 a lane

struct QlArgs {                          // by value in the launch: a captured call holds no host memory
    const void* cur[TD_K]; size_t cur_s[TD_K];   // elements
    const void* nq[TD_K]; size_t nq_s[TD_K];
    void* g[TD_K]; size_t g_s[TD_K];
    const void *rew, *done, *lp;
    const double* alpha_dev;
    void* y;
    double* stats;
    double* ws;                          // one partial [PL_PITCH] per block
    double gamma, alpha;
    size_t B;
    int K, Q, M, KQ, flags, rew_f64, done_f64, nblk;
    int* err;
};

__device__ __forceinline__ double ql_alpha(const QlArgs& a)
{
    if (!a.alpha_dev) return a.alpha;
    const double s = a.alpha_dev[0];
    return (a.flags & PTG_QL_LOG_ALPHA) ? exp(s) : s;
}

// element (row, i) of critic k: the pointer is chosen behind an unrolled guard, never indexed by k
template <typename IN>
__device__ __forceinline__ double ql_pick(const void* const (&ptr)[TD_K], const size_t (&st)[TD_K], int k, size_t row, int i)
{
    double v = 0.0;
#pragma unroll
    for (int kk = 0; kk < TD_K; kk++)
        if (kk == k) v = (double)((const IN*)ptr[kk])[row * st[kk] + (size_t)i];
    return v;
}

// the sums of a whole batch -> the eight statistics; one thread
__device__ __forceinline__ void ql_finish(const QlArgs& a, const double* sum, double alpha)
{
    const double BK = (double)a.B * (double)a.K, BKQ = BK * (double)a.Q, n = BKQ * (double)a.M;
    a.stats[0] = sum[0] / n; a.stats[1] = sum[1] / BKQ; a.stats[2] = sum[2] / ((double)a.B * (double)a.M);
    a.stats[3] = sum[3] / n; a.stats[4] = sum[4] / n;
    a.stats[5] = alpha; a.stats[6] = 0.0; a.stats[7] = 0.0;
}

// ONE: the whole batch is this block (B <= 4 rows): rows and statistics in one launch
template <typename IN, bool ONE>
__global__ void __launch_bounds__(PL_BLOCK)
k_ql_rows(QlArgs a)
{
    __shared__ double slab[PL_WAVES * QL_MAX];               // 8 KiB: a wave's next quantiles -> the kept ones, sorted -> the targets
    __shared__ double sh[PL_WAVES * PL_PITCH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * PL_WAVES + (size_t)w;
    const bool live = row < a.B;                             // the ragged last block: no row, zero terms, every barrier and tree
    const int KQ = a.KQ, Q = a.Q, M = a.M;
    double* const s = slab + w * QL_MAX;
    const double alpha = ql_alpha(a);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    // 1. stage: the lanes stride over the flat index p = k * Q + i
    double v[QL_PER];
#pragma unroll
    for (int t = 0; t < QL_PER; t++) {
        const int p = lane + 64 * t;
        v[t] = 0.0;
        if (live && p < KQ) {
            v[t] = ql_pick<IN>(a.nq, a.nq_s, p / Q, row, p % Q);
            s[p] = v[t];
        }
    }
    __syncthreads();
    // 2. rank: e precedes p iff v_e < v_p, or v_p is a NaN and v_e is not, or neither precedes by value and e < p (torch.sort's order)
    int rank[QL_PER];
#pragma unroll
    for (int t = 0; t < QL_PER; t++) {
        const int p = lane + 64 * t;
        rank[t] = QL_MAX;
        if (live && p < KQ) {
            const double x = v[t];
            const bool xn = x != x;
            int c = 0;
#pragma unroll 4
            for (int e = 0; e < KQ; e++) {
                const double z = s[e];
                const bool zn = z != z;
                const bool e_first = z < x || (xn && !zn), p_first = x < z || (zn && !xn);
                c += (e_first || (!p_first && e < p)) ? 1 : 0;
            }
            rank[t] = c;
        }
    }
    __syncthreads();                                         // every read of the staged values is over: the slice is rewritten in place
#pragma unroll
    for (int t = 0; t < QL_PER; t++)
        if (rank[t] < M) s[rank[t]] = v[t];                  // a permutation of 0 .. KQ - 1: one writer per slot
    __syncthreads();
    // 3. targets, in place; the current quantiles of this lane's pairs
    bool bad = false;
    double sum_y = 0.0;
    if (live) {
        const double r = td_rd(a.rew, a.rew_f64, row), dn = td_rd(a.done, a.done_f64, row);
        const double al = alpha * (double)((const IN*)a.lp)[row], c = (1.0 - dn) * a.gamma;
        for (int j = lane; j < M; j += 64) {
            const double y = r + c * (s[j] - al);
            s[j] = y;
            if (a.y) ((IN*)a.y)[row * (size_t)M + (size_t)j] = (IN)y;
            bad = bad || !pl_finite(y);
            sum_y = sum_y + y;
        }
    }
    double th[QL_PER];
#pragma unroll
    for (int t = 0; t < QL_PER; t++) {
        const int p = lane + 64 * t;
        th[t] = 0.0;
        if (live && p < KQ) {
            th[t] = ql_pick<IN>(a.cur, a.cur_s, p / Q, row, p % Q);
            bad = bad || !pl_finite(th[t]);
        }
    }
    __syncthreads();
    bad = __any(bad ? 1 : 0) != 0;                           // the wave's row: any kept target or any current quantile not finite
    // 4. pairs: the j loop in order, all of it out of LDS
    const double n = (((double)a.B * (double)a.K) * (double)Q) * (double)M;
    double sum_ls = 0.0, sum_q = 0.0, sum_ad = 0.0, sum_gt = 0.0;
#pragma unroll
    for (int t = 0; t < QL_PER; t++) {
        const int p = lane + 64 * t;
        if (live && p < KQ) {
            const int k = p / Q, i = p % Q;
            double g = nan;
            if (!bad) {
                const double theta = th[t], tau = ((double)i + 0.5) / (double)Q;
                double acc = 0.0, ls = 0.0, ad = 0.0;
                int gt = 0;
#pragma unroll 4
                for (int j = 0; j < M; j++) {                // unrolled for the LDS reads only: each accumulator still adds in j order
                    const double dl = s[j] - theta, ab = fabs(dl);
                    const double wt = fabs(tau - (dl < 0.0 ? 1.0 : 0.0));
                    const double hb = ab > 1.0 ? ab - 0.5 : 0.5 * (dl * dl);
                    const double cl = dl < -1.0 ? -1.0 : (dl > 1.0 ? 1.0 : dl);
                    acc = acc + wt * cl;
                    ls = ls + wt * hb;
                    ad = ad + ab;
                    gt += ab > 1.0 ? 1 : 0;
                }
                g = (-acc) / n;
                sum_ls = sum_ls + ls; sum_q = sum_q + theta; sum_ad = sum_ad + ad; sum_gt = sum_gt + (double)gt;
            }
#pragma unroll
            for (int kk = 0; kk < TD_K; kk++)
                if (kk == k) ((IN*)a.g[kk])[row * a.g_s[kk] + (size_t)i] = (IN)g;
        }
    }
    if (live && bad) {
        sum_ls = sum_q = sum_y = sum_ad = sum_gt = nan;
        if (lane == 0) a.err[5] = 1;
    }
    // 5. the row's terms -> the block's partial
    double sums[PL_TERMS] = {sum_ls, sum_q, sum_y, sum_ad, sum_gt, 0.0};
    loss_tail<ONE>(sums, sh, a.ws, [&](const double* s) { ql_finish(a, s, alpha); });
}

struct QlFinal {
    __device__ void operator()(const QlArgs& a, const double* v) const { ql_finish(a, v, ql_alpha(a)); }
};

// ================================================================================== the training-time actor head
// SB3's Actor.action_log_prob as SAC and TQC run it on a replay batch (include/ptg_env.h, ptg_rsample, states the lines;
// tests/actor_restatement.py restates them): the log_std clamp, exp, the reparametrised sample, tanh, the Gaussian log-density and the
// tanh correction -- and, in k_rs_bwd, autograd's walk back over all of it in closed form from the stored noise.  TD3's smoothed
// target action is the third kind.  k_act's shape: one lane per row on consecutive rows, no cross-lane traffic, float64 arithmetic
// whatever the dtype, rounded once on the store.  The draw is k_act's, keyed (seed, *counter, row) with no env offset.
struct RsArgs {                          // by value in the launch: a captured call holds no host memory
    const void* mean; size_t m_s;        // elements
    const void* ls; size_t ls_s;
    void *act, *logp;
    double* noise;
    const void *g_act, *g_logp;
    void* g_mean; size_t gm_s;
    void* g_ls; size_t gl_s;
    const unsigned long long* counter;   // null when deterministic
    unsigned long long seed;
    double sigma_t, c, lo, hi;           // PTG_RS_SMOOTH
    size_t B;
    int kind;
    int* err;
};

__device__ __forceinline__ double rs_clamp_log_std(double l) { return l < -20.0 ? -20.0 : (l > 2.0 ? 2.0 : l); }      // a NaN falls through

static_assert(sizeof(TrainGroup<RsArgs>) == 8 * 176 && sizeof(TrainGroup<RsArgs>) <= 4096, "the launch takes 4 096 bytes of kernel arguments");

// blockIdx.x is the block within the batch, blockIdx.y (ARGS = TrainGroup<RsArgs>, ptg_rsample_group) the member
template <typename IN, typename ARGS = RsArgs>
__global__ void __launch_bounds__(ACT_BLOCK)
k_rs_fwd(ARGS args)
{
    const RsArgs& a = train_member(args, blockIdx.y);
    const size_t b = (size_t)blockIdx.x * ACT_BLOCK + threadIdx.x;
    if (b >= a.B) return;                                    // the ragged last wave
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double z = 0.0;
    if (a.counter) {
        z = rb_draw_normal(rb_draw_word(a.seed, a.counter[0], (unsigned long long)b));
    }
    if (a.noise) a.noise[b] = z;
    const double mu = (double)((const IN*)a.mean)[b * a.m_s];
    IN* const act_o = (IN*)a.act; IN* const logp_o = (IN*)a.logp;
    if (a.kind == PTG_RS_SMOOTH) {
        if (!pl_finite(mu)) { act_o[b] = (IN)nan; a.err[5] = 1; return; }
        const double n = a.sigma_t * z;
        const double nc = n < -a.c ? -a.c : (n > a.c ? a.c : n);
        const double x = mu + nc;
        act_o[b] = (IN)(x < a.lo ? a.lo : (x > a.hi ? a.hi : x));
        return;
    }
    const double l = (double)((const IN*)a.ls)[b * a.ls_s];
    if (!pl_finite(mu) || l != l) {                          // NaN or Inf mean; NaN log_std (an infinite one clamps)
        act_o[b] = (IN)nan;
        if (logp_o) logp_o[b] = (IN)nan;
        a.err[5] = 1;
        return;
    }
    const double ls = rs_clamp_log_std(l);
    const double g = mu + exp(ls) * z;
    const double x = tanh(g);
    act_o[b] = (IN)x;
    if (logp_o) logp_o[b] = (IN)((((-(z * z) / 2.0) - ls) - 0.9189385332046727) - log((1.0 - x * x) + 1e-6));
}

// k_rb_bump's step for the grouped forward: one thread per member (the block index), each on its own counter word -- the members'
// counters are distinct and, the flags agreeing, none is null when this is launched
__global__ void k_rs_bump_group(const TrainGroup<RsArgs> g)
{
    unsigned long long* const word = const_cast<unsigned long long*>(g.m[blockIdx.x].counter);
    *word += 1ull;
}

template <typename IN, typename ARGS = RsArgs>
__global__ void __launch_bounds__(ACT_BLOCK)
k_rs_bwd(ARGS args)
{
    const RsArgs& a = train_member(args, blockIdx.y);
    const size_t b = (size_t)blockIdx.x * ACT_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double mu = (double)((const IN*)a.mean)[b * a.m_s], l = (double)((const IN*)a.ls)[b * a.ls_s], z = a.noise[b];
    const double ga = a.g_act ? (double)((const IN*)a.g_act)[b] : 0.0, gl = a.g_logp ? (double)((const IN*)a.g_logp)[b] : 0.0;
    IN* const gm_o = (IN*)a.g_mean + b * a.gm_s; IN* const gls_o = (IN*)a.g_ls + b * a.gl_s;
    if (!pl_finite(mu) || l != l || !pl_finite(z) || !pl_finite(ga) || !pl_finite(gl)) {
        gm_o[0] = (IN)nan; gls_o[0] = (IN)nan;
        a.err[5] = 1;
        return;
    }
    const double ls = rs_clamp_log_std(l);
    const bool pass = -20.0 <= l && l <= 2.0;                // torch's clamp gradient: inclusive at both ends
    const double sigma = exp(ls);
    const double x = tanh(mu + sigma * z);
    const double d = 1.0 - x * x, sz = sigma * z;
    const double q = ((2.0 * x) * d) / (d + 1e-6);
    gm_o[0] = (IN)(ga * d + gl * q);
    gls_o[0] = (IN)(pass ? ga * (d * sz) + gl * (q * sz - 1.0) : 0.0);
}

// ================================================================================== the actor and entropy-coefficient losses
// SB3's SAC.train / TD3.train and sb3_contrib's TQC.train actor lines and the entropy-coefficient loss (include/ptg_env.h,
// ptg_actor_loss, states the lines; tests/actor_restatement.py restates them) with d loss / d Q (or quantile), d loss / d log_prob and
// d loss / d log alpha in closed form.  k_td_rows' shape: one lane per row, the critics' pointers and strides by value, every loop over
// them unrolled over PTG_TD_MAX_CRITICS behind a k < K guard; a TQC lane walks its K * Q quantiles in index order (two strided reads
// and one store each).  Four sums and a poison word go through the fixed-order scheme stated above LossArgs.
struct AlArgs {                          // by value in the launch
    const void* q[TD_K]; size_t q_s[TD_K];       // elements
    void* g[TD_K]; size_t g_s[TD_K];
    const void* lp;
    const double* alpha_dev;
    void* g_lp;
    double* g_la;
    double* stats;
    double* ws;                          // one partial [PL_PITCH] per block
    double alpha, H_t;
    size_t B;
    int K, Q, kind, flags, nblk;
    int* err;
};

// alpha as this call uses it (0 when neither the entropy term nor the entropy-coefficient loss is asked for) and whether it is usable
__device__ __forceinline__ double al_alpha(const AlArgs& a, bool& ok)
{
    ok = true;
    if (!(a.flags & (PTG_AL_ENTROPY | PTG_AL_ENT_COEF))) return 0.0;
    double al = a.alpha;
    if (a.alpha_dev) {
        const double s = a.alpha_dev[0];
        al = (a.flags & PTG_AL_LOG_ALPHA) ? exp(s) : s;
        ok = pl_finite(s);
    }
    ok = ok && pl_finite(al);
    return al;
}

// the sums of a whole batch -> the eight statistics and d loss / d log alpha; one thread
__device__ __forceinline__ void al_finish(const AlArgs& a, const double* sum, double alpha)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double Bd = (double)a.B;
    const bool bad = sum[4] != sum[4], ec = (a.flags & PTG_AL_ENT_COEF) != 0;
    const bool reads_lp = (a.flags & (PTG_AL_ENTROPY | PTG_AL_ENT_COEF)) != 0;
    double el = 0.0, gla = 0.0;
    if (ec) {
        const double sb = sum[3] / Bd;
        el = -(a.alpha_dev[0] * sb);
        gla = -sb;
    }
    a.stats[0] = bad ? nan : (a.kind == PTG_AL_ALPHA_ONLY ? 0.0 : sum[0] / Bd);
    a.stats[1] = bad ? nan : el;
    a.stats[2] = bad ? nan : (reads_lp ? sum[1] / Bd : 0.0);
    a.stats[3] = bad ? nan : (a.kind == PTG_AL_ALPHA_ONLY ? 0.0 : sum[2] / Bd);
    a.stats[4] = alpha;
    a.stats[5] = bad ? nan : gla;
    a.stats[6] = 0.0; a.stats[7] = 0.0;
    if (ec && a.g_la) a.g_la[0] = bad ? nan : gla;
}

// ONE: the whole batch is this block (B <= PL_BLOCK): rows and statistics in one launch.  Otherwise the block leaves its partial sums
// in the workspace for k_loss_final.
// blockIdx.x is the block within the batch, blockIdx.y (ARGS = TrainGroup<AlArgs>, ptg_actor_loss_group) the member
template <typename IN, bool ONE, typename ARGS = AlArgs>
__global__ void __launch_bounds__(PL_BLOCK)
k_al_rows(ARGS args)
{
    const AlArgs& a = train_member(args, blockIdx.y);
    __shared__ double sh[PL_WAVES * PL_PITCH];
    const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    const bool live = i < a.B;                               // the ragged last wave: no row, zero terms, but it takes part in the trees
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    bool alpha_ok;
    const double alpha = al_alpha(a, alpha_ok);
    double v[PL_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // term, lp, m, lp + H_t, poison (NaN once a row is bad), unused
    if (live) {
        const int K = a.K, Q = a.Q;
        const double Bd = (double)a.B;
        const bool ent = (a.flags & PTG_AL_ENTROPY) != 0, reads_lp = (a.flags & (PTG_AL_ENTROPY | PTG_AL_ENT_COEF)) != 0;
        const double lp = reads_lp ? (double)((const IN*)a.lp)[i] : 0.0;
        double m = 0.0;
        int ks = 0;
        if (a.kind == PTG_AL_MIN) {
            m = (double)((const IN*)a.q[0])[i * a.q_s[0]];
#pragma unroll
            for (int k = 1; k < TD_K; k++) {
                if (k < K) {
                    const double l = (double)((const IN*)a.q[k])[i * a.q_s[k]];
                    if (l < m || l != l) { m = l; ks = k; }  // th.min: a NaN wins and then stays; of equal values the first
                }
            }
        } else if (a.kind == PTG_AL_MEAN) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < TD_K; k++) {
                if (k < K) {
                    const IN* __restrict__ row = (const IN*)a.q[k] + i * a.q_s[k];
                    double t = 0.0;
                    for (int j = 0; j < Q; j++) t += (double)row[j];
                    s += t / (double)Q;
                }
            }
            m = s / (double)K;
        }
        const bool bad = !alpha_ok || !pl_finite(m) || !pl_finite(lp);
        if (a.kind == PTG_AL_MIN) {
            const double gq = (-1.0) / Bd;
#pragma unroll
            for (int k = 0; k < TD_K; k++)
                if (k < K) ((IN*)a.g[k])[i * a.g_s[k]] = (IN)(bad ? nan : (k == ks ? gq : 0.0));
        } else if (a.kind == PTG_AL_MEAN) {
            const double gq = bad ? nan : (-1.0) / ((Bd * (double)K) * (double)Q);
#pragma unroll
            for (int k = 0; k < TD_K; k++) {
                if (k < K) {
                    IN* __restrict__ row = (IN*)a.g[k] + i * a.g_s[k];
                    for (int j = 0; j < Q; j++) row[j] = (IN)gq;
                }
            }
        }
        if (a.g_lp) ((IN*)a.g_lp)[i] = (IN)(bad ? nan : alpha / Bd);
        if (bad) {
            a.err[5] = 1;
            v[0] = nan; v[1] = nan; v[2] = nan; v[3] = nan; v[4] = nan;
        } else {
            v[0] = ent ? alpha * lp - m : -m;
            v[1] = lp; v[2] = m; v[3] = lp + a.H_t;
        }
    }
    loss_tail<ONE>(v, sh, a.ws, [&](const double* s) { al_finish(a, s, alpha); });
}

struct AlFinal {
    __device__ static const double* partials(const AlArgs& a) { return a.ws; }
    __device__ void operator()(const AlArgs& a, const double* v) const
    {
        bool ok;
        const double alpha = al_alpha(a, ok);
        al_finish(a, v, alpha);
    }
};

static_assert(sizeof(TrainGroup<AlArgs>) == 8 * 232 && sizeof(TrainGroup<AlArgs>) + sizeof(const double*) <= 4096, "the launch takes 4 096 bytes of kernel arguments");

// ================================================================================================= host side
// the gathers' launch: the unit type V (16-byte piece or element) and the index source -- the caller's int32 / int64 indices, or with
// idx null the drawn ones -- are the kernel's two template axes
template <typename V>
void launch_minibatch(hipStream_t st, const void* idx, int idx_bytes, const MbDraw& draw, size_t B, unsigned T, size_t N, const char* obs,
                             size_t s_t, size_t s_n, size_t unit_stride, unsigned P, char* obs_out, const MbCols& cols, int* err)
{
    const dim3 grid((unsigned)((B + MB_ROWS * MB_WAVES - 1) / (MB_ROWS * MB_WAVES))), block(64 * MB_WAVES);
    if (!idx)
        hipLaunchKernelGGL((k_minibatch<V, MbDrawn>), grid, block, 0, st, (const MbDrawn*)nullptr, draw, B, T, N, N * T, obs, s_t, s_n, unit_stride, P, obs_out, cols, err);
    else if (idx_bytes == 8)
        hipLaunchKernelGGL((k_minibatch<V, long long>), grid, block, 0, st, (const long long*)idx, draw, B, T, N, N * T, obs, s_t, s_n, unit_stride, P, obs_out, cols, err);
    else
        hipLaunchKernelGGL((k_minibatch<V, int>), grid, block, 0, st, (const int*)idx, draw, B, T, N, N * T, obs, s_t, s_n, unit_stride, P, obs_out, cols, err);
}

// the blocks of a loss's batch at `per` rows a block (PL_BLOCK; the quantile loss: PL_WAVES), and the bytes of that many partials
static int64_t loss_blocks(int64_t batch, int per) { return (batch - 1) / per + 1; }
static int64_t loss_partials_bytes(int64_t nblk) { return nblk * PL_PITCH * (int64_t)sizeof(double); }

// the workspace of a loss that keeps nothing but its partials there; the limit is ptg_policy_loss's: 2^23 blocks of 256 threads (the
// quantile loss: 2^29 blocks of four rows)
static int64_t loss_workspace(int64_t batch, int per)
{
    if (batch < 1 || batch > (int64_t)1 << 31) return PTG_E_INVALID;
    return loss_partials_bytes(loss_blocks(batch, per));
}

// the launches of a loss: a batch of one block has rows and statistics in one launch (`one`, the row kernel's ONE instantiation);
// else the rows (`many`), then k_loss_final over the partials at `part`
template <typename FIN, typename A>
void launch_loss(hipStream_t st, const A& a, const double* part, void (*one)(A), void (*many)(A))
{
    const dim3 grid((unsigned)a.nblk), block(PL_BLOCK);
    if (a.nblk == 1) {
        hipLaunchKernelGGL(one, grid, block, 0, st, a);
        return;
    }
    hipLaunchKernelGGL(many, grid, block, 0, st, a);
    hipLaunchKernelGGL((k_loss_final<A, FIN>), dim3(1), block, 0, st, a, part);
}

// the grouped launches of a loss whose row kernel keeps nothing but its partials in the workspace: launch_loss's, the member as the
// grid's y (rows) or x (the final merge, which finds each member's partials through FIN::partials)
template <typename FIN, typename A>
void launch_loss_group(hipStream_t st, const TrainGroup<A>& g, int n_members, void (*one)(TrainGroup<A>), void (*many)(TrainGroup<A>))
{
    const dim3 rows((unsigned)g.m[0].nblk, (unsigned)n_members), block(PL_BLOCK);
    if (g.m[0].nblk == 1) {
        hipLaunchKernelGGL(one, rows, block, 0, st, g);
        return;
    }
    hipLaunchKernelGGL(many, rows, block, 0, st, g);
    hipLaunchKernelGGL((k_loss_final<A, FIN, TrainGroup<A>>), dim3((unsigned)n_members), block, 0, st, g, (const double*)nullptr);
}

// the gSDE row kernels' NJ: the smallest of 4 | 8 | 16 that holds a lane's ceil(L / 64) units
static int sde_nj(int L) { const int nj = (L + 63) / 64; return nj <= 4 ? 4 : (nj <= 8 ? 8 : SDE_MAX_J); }
static int64_t sde_loss_blocks(int64_t batch) { return loss_blocks(batch, (int)sde_rows_per_wave((size_t)batch) * SDE_WAVES); }

template <typename IN>
void launch_sde_act(hipStream_t st, dim3 grid, const SdeActArgs& a)
{
    const dim3 block(SDE_BLOCK);
    switch (sde_nj(a.L)) {
    case 4: hipLaunchKernelGGL((k_sde_act<IN, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((k_sde_act<IN, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_sde_act<IN, SDE_MAX_J>), grid, block, 0, st, a);
    }
}

// the rows, then the five means over the blocks' partials and the log_std gradient over their column partials
template <typename IN>
void launch_sde_loss(hipStream_t st, const SdeLossArgs& a, void* g_ls)
{
    const dim3 grid((unsigned)a.nblk), block(SDE_BLOCK);
    switch (sde_nj(a.L)) {
    case 4: hipLaunchKernelGGL((k_sde_rows<IN, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((k_sde_rows<IN, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_sde_rows<IN, SDE_MAX_J>), grid, block, 0, st, a);
    }
    hipLaunchKernelGGL((k_loss_final<SdeLossArgs, SdeFinal<IN>>), dim3(1), dim3(PL_BLOCK), 0, st, a, (const double*)a.row_part);
    hipLaunchKernelGGL(k_sde_cols<IN>, dim3((unsigned)((a.L - 1) / SDE_BLOCK + 1)), block, 0, st, a, g_ls);
}

template <typename IN>
void launch_sde_rs(hipStream_t st, const SdeRsArgs& a, bool backward)
{
    const dim3 grid((unsigned)a.nblk), block(SDE_BLOCK);
    if (!backward) {
        switch (sde_nj(a.L)) {
        case 4: hipLaunchKernelGGL((k_sde_rs_fwd<IN, 4>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_sde_rs_fwd<IN, 8>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((k_sde_rs_fwd<IN, SDE_MAX_J>), grid, block, 0, st, a);
        }
        return;
    }
    switch (sde_nj(a.L)) {
    case 4: hipLaunchKernelGGL((k_sde_rs_bwd<IN, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((k_sde_rs_bwd<IN, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_sde_rs_bwd<IN, SDE_MAX_J>), grid, block, 0, st, a);
    }
}

// what ptg_rsample and ptg_rsample_backward refuse alike; the text of the first fault, or null
const char* rs_desc_error(const ptg_rs* d, bool backward)
{
    if (d->kind != PTG_RS_SQUASH && d->kind != PTG_RS_SMOOTH) return "unknown kind";
    if (d->flags & ~PTG_RS_DETERMINISTIC) return "unknown flag";
    if (d->q_dtype != PTG_OUT_F32 && d->q_dtype != PTG_OUT_F64) return "q_dtype must be PTG_OUT_F32 or PTG_OUT_F64";
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return "batch outside [1, 2^31]";
    if (!d->mean_dev || d->mean_s_n < 1) return "null mean_dev or mean_s_n < 1";
    if (d->kind == PTG_RS_SQUASH && (!d->log_std_dev || d->log_std_s_n < 1)) return "null log_std_dev or log_std_s_n < 1";
    if (backward) {
        if (d->kind != PTG_RS_SQUASH) return "PTG_RS_SMOOTH has no backward";
        if (!d->noise_dev || (uintptr_t)d->noise_dev % sizeof(double) != 0) return "noise_dev is null or not aligned to 8 bytes";
        if (!d->grad_act_dev && !d->grad_logp_dev) return "grad_act_dev and grad_logp_dev are both null";
        if (!d->grad_mean_dev || !d->grad_log_std_dev) return "null grad_mean_dev or grad_log_std_dev";
        if (d->gm_s_n < 1 || d->gl_s_n < 1) return "gm_s_n or gl_s_n < 1";
        return nullptr;
    }
    if (!d->act_dev) return "null act_dev";
    if (!(d->flags & PTG_RS_DETERMINISTIC) && !d->counter_dev) return "a stochastic call needs counter_dev";
    if (d->noise_dev && (uintptr_t)d->noise_dev % sizeof(double) != 0) return "noise_dev is not aligned to 8 bytes";
    if (d->kind == PTG_RS_SMOOTH) {
        if (d->logp_dev) return "PTG_RS_SMOOTH has no log-prob";
        if (!(d->noise_std >= 0.0) || !std::isfinite(d->noise_std)) return "noise_std is negative or not finite";
        if (!(d->noise_clip >= 0.0)) return "noise_clip is negative or NaN";
        if (!(d->clip_lo <= d->clip_hi)) return "clip_lo > clip_hi (or a NaN bound)";
    }
    return nullptr;
}

// ---- what ptg_policy_loss / ptg_optim_step and their grouped entries share: one descriptor check, one set of launch arguments ------
// a fault's text into `why`; true, so that a checker can `return train_fault(...)`
__attribute__((format(printf, 3, 4))) bool train_fault(char* why, size_t cap, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why, cap, fmt, ap);
    va_end(ap);
    return true;
}

// what a ptg_loss is refused for, in the single call's order; true with the text in `why`
bool loss_desc_fault(const ptg_loss* d, char* why, size_t cap)
{
    if (d->kind != PTG_LOSS_PPO && d->kind != PTG_LOSS_A2C) return train_fault(why, cap, "unknown kind %d", d->kind);
    if (d->head != PTG_HEAD_CATEGORICAL && d->head != PTG_HEAD_GAUSSIAN) return train_fault(why, cap, "head %d is neither categorical nor Gaussian", d->head);
    if (d->flags & ~(PTG_LOSS_NORM_ADV | PTG_LOSS_CLIP_VF)) return train_fault(why, cap, "unknown flag in %d", d->flags);
    const bool ppo = d->kind == PTG_LOSS_PPO, gauss = d->head == PTG_HEAD_GAUSSIAN, clipv = (d->flags & PTG_LOSS_CLIP_VF) != 0;
    if (ptg_policy_loss_workspace(d->batch) < 0) return train_fault(why, cap, "batch %lld outside [1, 2^31]", (long long)d->batch);
    if (d->in_dtype != PTG_OUT_F32 && d->in_dtype != PTG_OUT_F64) return train_fault(why, cap, "in_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!d->in_dev || !d->val_dev || !d->act_dev || !d->adv_dev || !d->ret_dev) return train_fault(why, cap, "null input, values, actions, advantages or returns");
    if (ppo && !d->old_logp_dev) return train_fault(why, cap, "PPO needs old_logp_dev");
    if (!d->stats_dev || !d->grad_in_dev || !d->grad_val_dev) return train_fault(why, cap, "null stats_dev, grad_in_dev or grad_val_dev");
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return train_fault(why, cap, "ws_dev is null or not aligned to 8 bytes");
    if (clipv && !d->old_val_dev) return train_fault(why, cap, "PTG_LOSS_CLIP_VF needs old_val_dev");
    if (d->val_s_n < 1 || d->gv_s_n < 1) return train_fault(why, cap, "val_s_n or gv_s_n < 1");
    if (gauss) {
        if (d->in_s_n < 1 || d->g_s_n < 1) return train_fault(why, cap, "in_s_n or g_s_n < 1");
        if (!d->log_std_dev) return train_fault(why, cap, "the Gaussian head needs log_std_dev");
    } else {
        if (d->n_actions < 2 || d->n_actions > 32) return train_fault(why, cap, "n_actions outside [2, 32]");
        if (d->in_s_n < d->n_actions || d->g_s_n < d->n_actions) return train_fault(why, cap, "in_s_n or g_s_n < n_actions");
        if (d->act_kind != PTG_ACT_I32 && d->act_kind != PTG_ACT_I64) return train_fault(why, cap, "the categorical head takes PTG_ACT_I32 or PTG_ACT_I64 actions");
        if (d->grad_log_std_dev) return train_fault(why, cap, "grad_log_std_dev is the Gaussian head's");
    }
    if (ppo && !(d->clip_range >= 0.0)) return train_fault(why, cap, "clip_range is negative or NaN");
    if (clipv && !(d->clip_range_vf >= 0.0)) return train_fault(why, cap, "clip_range_vf is negative or NaN");
    return false;
}

LossArgs loss_args(ptg_env* h, const ptg_loss* d)
{
    LossArgs a{};
    a.in = d->in_dev; a.s_n = (size_t)d->in_s_n; a.val = d->val_dev; a.v_s = (size_t)d->val_s_n;
    a.act = d->act_dev; a.old_lp = d->old_logp_dev; a.adv = d->adv_dev; a.ret = d->ret_dev; a.old_val = d->old_val_dev; a.log_std = d->log_std_dev;
    a.g_in = d->grad_in_dev; a.g_s = (size_t)d->g_s_n; a.g_val = d->grad_val_dev; a.gv_s = (size_t)d->gv_s_n; a.g_ls = d->grad_log_std_dev;
    a.stats = d->stats_dev; a.ws = (double*)d->ws_dev;
    a.eps = d->clip_range; a.eps_v = d->clip_range_vf; a.ent_coef = d->ent_coef; a.vf_coef = d->vf_coef;
    a.B = (size_t)d->batch; a.A = d->n_actions; a.kind = d->kind; a.head = d->head; a.flags = d->flags; a.act_kind = d->act_kind;
    a.nblk = (int)loss_blocks(d->batch, PL_BLOCK);
    a.err = h->P.err;
    return a;
}

// what a ptg_optim is refused for, in the single call's order; true with the text in `why`
bool optim_desc_fault(const ptg_optim* d, char* why, size_t cap)
{
    const int kind = d->kind, flags = d->flags;
    if (kind != PTG_OPTIM_ADAM && kind != PTG_OPTIM_RMSPROP && kind != PTG_OPTIM_POLYAK) return train_fault(why, cap, "unknown kind %d", kind);
    if (flags & ~(PTG_OPTIM_CLIP | PTG_OPTIM_TARGETS | PTG_OPTIM_ZERO_GRAD)) return train_fault(why, cap, "unknown flag in %d", flags);
    const bool polyak = kind == PTG_OPTIM_POLYAK, clip = (flags & PTG_OPTIM_CLIP) != 0, targets = polyak || (flags & PTG_OPTIM_TARGETS) != 0;
    if (polyak && (flags & (PTG_OPTIM_CLIP | PTG_OPTIM_ZERO_GRAD))) return train_fault(why, cap, "PTG_OPTIM_POLYAK reads no gradient: no PTG_OPTIM_CLIP, no PTG_OPTIM_ZERO_GRAD");
    if (d->dtype != PTG_OUT_F32 && d->dtype != PTG_OUT_F64) return train_fault(why, cap, "dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (d->n_tensors < 1) return train_fault(why, cap, "n_tensors < 1");
    if (ptg_optim_workspace(d->n_chunks) < 0) return train_fault(why, cap, "n_chunks %lld outside [1, 2^31)", (long long)d->n_chunks);
    if (!d->tensors_dev || !d->chunks_dev) return train_fault(why, cap, "null tensor or chunk table");
    if ((uintptr_t)d->tensors_dev % 8 != 0 || (uintptr_t)d->chunks_dev % 8 != 0) return train_fault(why, cap, "a table is not aligned to 8 bytes");
    if (targets && !(d->tau >= 0.0 && d->tau <= 1.0)) return train_fault(why, cap, "tau outside [0, 1] (or NaN)");
    if (!polyak) {
        if (!d->state_dev) return train_fault(why, cap, "null state_dev");
        if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return train_fault(why, cap, "ws_dev is null or not aligned to 8 bytes");
        if (!d->lr_dev && !(d->lr >= 0.0 && std::isfinite(d->lr))) return train_fault(why, cap, "lr is negative or not finite (and lr_dev is null)");
        if (!(d->eps >= 0.0) || !std::isfinite(d->eps)) return train_fault(why, cap, "eps is negative or not finite");
        if (kind == PTG_OPTIM_ADAM && (!(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0)))
            return train_fault(why, cap, "a beta outside [0, 1)");
        if (kind == PTG_OPTIM_RMSPROP && !(d->alpha >= 0.0 && std::isfinite(d->alpha))) return train_fault(why, cap, "alpha is negative or not finite");
        if (clip && !d->norm_dev) return train_fault(why, cap, "PTG_OPTIM_CLIP needs norm_dev");
        if (clip && !(d->max_norm >= 0.0)) return train_fault(why, cap, "max_norm is negative or NaN");
    }
    return false;
}

OptArgs optim_args(ptg_env* h, const ptg_optim* d)
{
    OptArgs a{};
    a.tensors = (const ptg_optim_tensor*)d->tensors_dev; a.chunks = (const ptg_optim_span*)d->chunks_dev;
    a.ws = (double*)d->ws_dev; a.state = d->state_dev; a.lr_dev = d->lr_dev; a.norm = d->norm_dev;
    a.lr = d->lr; a.b1 = d->beta1; a.b2 = d->beta2; a.eps = d->eps; a.alpha = d->alpha; a.tau = d->tau; a.max_norm = d->max_norm;
    a.n_tensors = (long long)d->n_tensors; a.n_chunks = (unsigned)d->n_chunks; a.kind = d->kind; a.flags = d->flags; a.err = h->P.err;
    return a;
}

// What a single and a grouped entry refuse before the first launch, in one order: the array, the count, each descriptor's own fault
// (grouped: behind "member i: "), then, grouped, `agree` -- a disagreement with member 0, or an output that two members share.  0, or
// the error set in h
template <typename D, typename Fault, typename Agree>
int train_refuse(ptg_env* h, const char* who, const D* members, int n_members, bool grouped, Fault fault, Agree agree)
{
    if (!members) return set_err(h, PTG_E_INVALID, "%s: null descriptor%s", who, grouped ? " array" : "");
    if (n_members < 1 || n_members > PTG_TRAIN_GROUP_MAX) return set_err(h, PTG_E_INVALID, "%s: n_members %d outside [1, %d]", who, n_members, PTG_TRAIN_GROUP_MAX);
    char why[240];
    for (int i = 0; i < n_members; i++) {
        if (!fault(&members[i], why, sizeof why)) continue;
        return grouped ? set_err(h, PTG_E_INVALID, "%s: member %d: %s", who, i, why) : set_err(h, PTG_E_INVALID, "%s: %s", who, why);
    }
    if (grouped && agree(why, sizeof why)) return set_err(h, PTG_E_INVALID, "%s: %s", who, why);
    return 0;
}

// two members that name one output or scratch buffer: the half of "outputs must not overlap" that the host can see
bool train_shared(const void* p, const void* q, const char* field, int i, int j, char* why, size_t cap)
{
    return p && p == q ? train_fault(why, cap, "members %d and %d share %s", i, j, field) : false;
}

#define TRAIN_AGREE(field, fmt, cast)                                                                                                                    \
    if (b.field != a.field) return train_fault(why, cap, "members 0 and %d disagree in " #field ": " fmt " and " fmt, i, (cast)a.field, (cast)b.field)
#define TRAIN_DISTINCT(field)                                                                                                                            \
    if (train_shared(m[i].field, m[j].field, #field, j, i, why, cap)) return true

bool loss_group_fault(const ptg_loss* m, int n, char* why, size_t cap)
{
    const ptg_loss& a = m[0];
    for (int i = 1; i < n; i++) {
        const ptg_loss& b = m[i];
        TRAIN_AGREE(kind, "%d", int); TRAIN_AGREE(head, "%d", int); TRAIN_AGREE(flags, "%d", int); TRAIN_AGREE(n_actions, "%d", int);
        TRAIN_AGREE(in_dtype, "%d", int); TRAIN_AGREE(act_kind, "%d", int); TRAIN_AGREE(batch, "%lld", long long);
    }
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++) {
            TRAIN_DISTINCT(stats_dev); TRAIN_DISTINCT(ws_dev); TRAIN_DISTINCT(grad_in_dev); TRAIN_DISTINCT(grad_val_dev);
        }
    return false;
}

bool optim_group_fault(const ptg_optim* m, int n, char* why, size_t cap)
{
    const ptg_optim& a = m[0];
    for (int i = 1; i < n; i++) {
        const ptg_optim& b = m[i];
        TRAIN_AGREE(kind, "%d", int); TRAIN_AGREE(flags, "%d", int); TRAIN_AGREE(dtype, "%d", int);
    }
    if (a.kind == PTG_OPTIM_POLYAK) return false;             // it reads no state, norm or scratch
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++) {
            TRAIN_DISTINCT(state_dev); TRAIN_DISTINCT(norm_dev); TRAIN_DISTINCT(ws_dev);
        }
    return false;
}

// ---- what ptg_td_loss / ptg_actor_loss / ptg_rsample(_backward) and their grouped entries share -------------
// what a ptg_td is refused for, in the single call's order; true with the text in `why`
bool td_desc_fault(const ptg_td* d, char* why, size_t cap)
{
    if (d->kind != PTG_TD_DQN && d->kind != PTG_TD_CRITICS) return train_fault(why, cap, "unknown kind %d", d->kind);
    if (d->flags & ~(PTG_TD_ENTROPY | PTG_TD_LOG_ALPHA)) return train_fault(why, cap, "unknown flag in %d", d->flags);
    const bool dqn = d->kind == PTG_TD_DQN, ent = (d->flags & PTG_TD_ENTROPY) != 0, log_alpha = (d->flags & PTG_TD_LOG_ALPHA) != 0;
    const auto dtype_ok = [](int c) { return c == PTG_OUT_F32 || c == PTG_OUT_F64; };
    if (ptg_td_loss_workspace(d->batch) < 0) return train_fault(why, cap, "batch %lld outside [1, 2^31]", (long long)d->batch);
    if (!dtype_ok(d->q_dtype) || !dtype_ok(d->rew_dtype) || !dtype_ok(d->done_dtype))
        return train_fault(why, cap, "q_dtype, rew_dtype and done_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!d->rew_dev || !d->done_dev || !d->stats_dev) return train_fault(why, cap, "null rew_dev, done_dev or stats_dev");
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return train_fault(why, cap, "ws_dev is null or not aligned to 8 bytes");
    if (dqn && ent) return train_fault(why, cap, "PTG_TD_ENTROPY applies to the critics only");
    if (log_alpha && !ent) return train_fault(why, cap, "PTG_TD_LOG_ALPHA needs PTG_TD_ENTROPY");
    if (ent && !d->next_logp_dev) return train_fault(why, cap, "PTG_TD_ENTROPY needs next_logp_dev");
    if (log_alpha && !d->alpha_dev) return train_fault(why, cap, "PTG_TD_LOG_ALPHA needs alpha_dev");
    int K = 1;
    int64_t min_stride = 1;
    if (dqn) {
        if (d->n_actions < 2 || d->n_actions > 32) return train_fault(why, cap, "n_actions outside [2, 32]");
        if (d->act_kind != PTG_ACT_I32 && d->act_kind != PTG_ACT_I64) return train_fault(why, cap, "DQN takes PTG_ACT_I32 or PTG_ACT_I64 actions");
        if (!d->act_dev) return train_fault(why, cap, "DQN needs act_dev");
        min_stride = d->n_actions;
    } else {
        if (d->n_critics < 1 || d->n_critics > PTG_TD_MAX_CRITICS) return train_fault(why, cap, "n_critics outside [1, %d]", PTG_TD_MAX_CRITICS);
        K = d->n_critics;
    }
    for (int k = 0; k < K; k++) {
        if (!d->q_dev[k] || !d->next_q_dev[k] || !d->grad_q_dev[k]) return train_fault(why, cap, "null q_dev, next_q_dev or grad_q_dev [%d]", k);
        if (d->q_s_n[k] < min_stride || d->next_s_n[k] < min_stride || d->g_s_n[k] < min_stride)
            return train_fault(why, cap, "q_s_n, next_s_n or g_s_n [%d] below %lld", k, (long long)min_stride);
    }
    return false;
}

// the critics a checked ptg_td / ptg_al names: DQN's one Q network, none for the entropy-coefficient loss alone
int td_critics(const ptg_td* d) { return d->kind == PTG_TD_DQN ? 1 : d->n_critics; }
int al_critics(const ptg_al* d) { return d->kind == PTG_AL_ALPHA_ONLY ? 0 : d->n_critics; }

TdArgs td_args(ptg_env* h, const ptg_td* d)
{
    const bool ent = (d->flags & PTG_TD_ENTROPY) != 0;
    const int K = td_critics(d);
    TdArgs a{};
    for (int k = 0; k < K; k++) {
        a.q[k] = d->q_dev[k]; a.q_s[k] = (size_t)d->q_s_n[k];
        a.nq[k] = d->next_q_dev[k]; a.nq_s[k] = (size_t)d->next_s_n[k];
        a.g[k] = d->grad_q_dev[k]; a.g_s[k] = (size_t)d->g_s_n[k];
    }
    a.act = d->act_dev; a.rew = d->rew_dev; a.done = d->done_dev; a.lp = ent ? d->next_logp_dev : nullptr;
    a.alpha_dev = ent ? d->alpha_dev : nullptr;
    a.y = d->y_dev; a.stats = d->stats_dev; a.ws = (double*)d->ws_dev;
    a.gamma = d->gamma; a.alpha = d->alpha; a.scale = d->scale;
    a.B = (size_t)d->batch; a.A = d->n_actions; a.K = K; a.kind = d->kind; a.flags = d->flags; a.act_kind = d->act_kind;
    a.rew_f64 = d->rew_dtype == PTG_OUT_F64; a.done_f64 = d->done_dtype == PTG_OUT_F64;
    a.nblk = (int)loss_blocks(d->batch, PL_BLOCK);
    a.err = h->P.err;
    return a;
}

// what a ptg_al is refused for, in the single call's order; true with the text in `why`
bool al_desc_fault(const ptg_al* d, char* why, size_t cap)
{
    if (d->kind != PTG_AL_MIN && d->kind != PTG_AL_MEAN && d->kind != PTG_AL_ALPHA_ONLY) return train_fault(why, cap, "unknown kind %d", d->kind);
    if (d->flags & ~(PTG_AL_ENTROPY | PTG_AL_LOG_ALPHA | PTG_AL_ENT_COEF)) return train_fault(why, cap, "unknown flag in %d", d->flags);
    const bool only = d->kind == PTG_AL_ALPHA_ONLY, ent = (d->flags & PTG_AL_ENTROPY) != 0, log_alpha = (d->flags & PTG_AL_LOG_ALPHA) != 0,
               ec = (d->flags & PTG_AL_ENT_COEF) != 0;
    if (ptg_actor_loss_workspace(d->batch) < 0) return train_fault(why, cap, "batch %lld outside [1, 2^31]", (long long)d->batch);
    if (d->q_dtype != PTG_OUT_F32 && d->q_dtype != PTG_OUT_F64) return train_fault(why, cap, "q_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!d->stats_dev) return train_fault(why, cap, "null stats_dev");
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return train_fault(why, cap, "ws_dev is null or not aligned to 8 bytes");
    if (only && (ent || !ec)) return train_fault(why, cap, "PTG_AL_ALPHA_ONLY takes PTG_AL_ENT_COEF and no PTG_AL_ENTROPY");
    if (ec && !log_alpha) return train_fault(why, cap, "PTG_AL_ENT_COEF needs PTG_AL_LOG_ALPHA");
    if (log_alpha && !ent && !ec) return train_fault(why, cap, "PTG_AL_LOG_ALPHA needs PTG_AL_ENTROPY or PTG_AL_ENT_COEF");
    if (log_alpha && !d->alpha_dev) return train_fault(why, cap, "PTG_AL_LOG_ALPHA needs alpha_dev");
    if ((ent || ec) && !d->logp_dev) return train_fault(why, cap, "PTG_AL_ENTROPY and PTG_AL_ENT_COEF need logp_dev");
    if (ec && !std::isfinite(d->target_entropy)) return train_fault(why, cap, "PTG_AL_ENT_COEF needs a finite target_entropy");
    if (d->grad_logp_dev && !ent) return train_fault(why, cap, "grad_logp_dev goes with PTG_AL_ENTROPY");
    if (d->grad_log_alpha_dev && (!ec || (uintptr_t)d->grad_log_alpha_dev % sizeof(double) != 0))
        return train_fault(why, cap, "grad_log_alpha_dev goes with PTG_AL_ENT_COEF and is aligned to 8 bytes");
    if (!only) {
        if (d->n_critics < 1 || d->n_critics > PTG_TD_MAX_CRITICS) return train_fault(why, cap, "n_critics outside [1, %d]", PTG_TD_MAX_CRITICS);
        int Q = 1;
        if (d->kind == PTG_AL_MEAN) {
            if (d->n_quantiles < 1 || d->n_quantiles > PTG_QL_MAX_QUANTILES) return train_fault(why, cap, "n_quantiles outside [1, %d]", PTG_QL_MAX_QUANTILES);
            Q = d->n_quantiles;
        }
        for (int k = 0; k < d->n_critics; k++) {
            if (!d->q_dev[k] || !d->grad_q_dev[k]) return train_fault(why, cap, "null q_dev or grad_q_dev [%d]", k);
            if (d->q_s_n[k] < Q || d->g_s_n[k] < Q) return train_fault(why, cap, "q_s_n or g_s_n [%d] below %d", k, Q);
        }
    }
    return false;
}

AlArgs al_args(ptg_env* h, const ptg_al* d)
{
    const bool ent = (d->flags & PTG_AL_ENTROPY) != 0, ec = (d->flags & PTG_AL_ENT_COEF) != 0;
    const int K = al_critics(d);
    AlArgs a{};
    for (int k = 0; k < K; k++) {
        a.q[k] = d->q_dev[k]; a.q_s[k] = (size_t)d->q_s_n[k];
        a.g[k] = d->grad_q_dev[k]; a.g_s[k] = (size_t)d->g_s_n[k];
    }
    a.lp = (ent || ec) ? d->logp_dev : nullptr; a.alpha_dev = (ent || ec) ? d->alpha_dev : nullptr;
    a.g_lp = d->grad_logp_dev; a.g_la = d->grad_log_alpha_dev; a.stats = d->stats_dev; a.ws = (double*)d->ws_dev;
    a.alpha = d->alpha; a.H_t = ec ? d->target_entropy : 0.0;
    a.B = (size_t)d->batch; a.K = K; a.Q = d->kind == PTG_AL_MEAN ? d->n_quantiles : 1; a.kind = d->kind; a.flags = d->flags;
    a.nblk = (int)loss_blocks(d->batch, PL_BLOCK);
    a.err = h->P.err;
    return a;
}

// any grad_q_dev of member i against any of member j: the K gradient outputs of a member are K buffers
template <typename D>
bool train_shared_grads(const D* m, int K, int i, int j, char* why, size_t cap)
{
    for (int k = 0; k < K; k++)
        for (int l = 0; l < K; l++)
            if (train_shared(m[i].grad_q_dev[k], m[j].grad_q_dev[l], "grad_q_dev", j, i, why, cap)) return true;
    return false;
}

bool td_group_fault(const ptg_td* m, int n, char* why, size_t cap)
{
    const ptg_td& a = m[0];
    for (int i = 1; i < n; i++) {
        const ptg_td& b = m[i];
        TRAIN_AGREE(kind, "%d", int); TRAIN_AGREE(flags, "%d", int); TRAIN_AGREE(n_actions, "%d", int); TRAIN_AGREE(n_critics, "%d", int);
        TRAIN_AGREE(q_dtype, "%d", int); TRAIN_AGREE(rew_dtype, "%d", int); TRAIN_AGREE(done_dtype, "%d", int); TRAIN_AGREE(act_kind, "%d", int);
        TRAIN_AGREE(batch, "%lld", long long);
    }
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++) {
            TRAIN_DISTINCT(stats_dev); TRAIN_DISTINCT(ws_dev); TRAIN_DISTINCT(y_dev);
            if (train_shared_grads(m, td_critics(&a), i, j, why, cap)) return true;
        }
    return false;
}

bool al_group_fault(const ptg_al* m, int n, char* why, size_t cap)
{
    const ptg_al& a = m[0];
    for (int i = 1; i < n; i++) {
        const ptg_al& b = m[i];
        TRAIN_AGREE(kind, "%d", int); TRAIN_AGREE(flags, "%d", int); TRAIN_AGREE(n_critics, "%d", int); TRAIN_AGREE(n_quantiles, "%d", int);
        TRAIN_AGREE(q_dtype, "%d", int); TRAIN_AGREE(batch, "%lld", long long);
    }
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++) {
            TRAIN_DISTINCT(stats_dev); TRAIN_DISTINCT(ws_dev);
            if (train_shared_grads(m, al_critics(&a), i, j, why, cap)) return true;
            TRAIN_DISTINCT(grad_logp_dev); TRAIN_DISTINCT(grad_log_alpha_dev);
        }
    return false;
}

// a shared counter_dev is refused too: the grouped forward reads every counter before any bump, G calls in turn would not
bool rs_group_fault(const ptg_rs* m, int n, bool backward, char* why, size_t cap)
{
    const ptg_rs& a = m[0];
    for (int i = 1; i < n; i++) {
        const ptg_rs& b = m[i];
        TRAIN_AGREE(kind, "%d", int); TRAIN_AGREE(flags, "%d", int); TRAIN_AGREE(q_dtype, "%d", int); TRAIN_AGREE(batch, "%lld", long long);
    }
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++) {
            if (backward) {
                TRAIN_DISTINCT(grad_mean_dev); TRAIN_DISTINCT(grad_log_std_dev);
                if (train_shared(m[i].grad_mean_dev, m[j].grad_log_std_dev, "grad_mean_dev and grad_log_std_dev", j, i, why, cap)) return true;
                if (train_shared(m[i].grad_log_std_dev, m[j].grad_mean_dev, "grad_mean_dev and grad_log_std_dev", j, i, why, cap)) return true;
            } else {
                TRAIN_DISTINCT(act_dev); TRAIN_DISTINCT(logp_dev); TRAIN_DISTINCT(noise_dev);
                if (!(a.flags & PTG_RS_DETERMINISTIC)) TRAIN_DISTINCT(counter_dev);
            }
        }
    return false;
}
#undef TRAIN_AGREE
#undef TRAIN_DISTINCT

}  // namespace

extern "C" {

// ---- VecNormalize(norm_obs=False) on the device ---------------------------------------------------------------------
int ptg_vn_init(ptg_env* h, double gamma, double epsilon, double clip_reward)
{
    if (!h) return PTG_E_INVALID;
    if (!(gamma >= 0.0) || !(epsilon >= 0.0) || !(clip_reward > 0.0)) return set_err(h, PTG_E_INVALID, "ptg_vn_init: bad gamma / epsilon / clip_reward");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (!h->vn_returns) {
        if ((rc = dev_alloc(h, &h->vn_returns, (size_t)h->n)) || (rc = dev_alloc(h, &h->vn_stats, 3))) return rc;
    }
    h->vn_gamma = gamma; h->vn_eps = epsilon; h->vn_clip = clip_reward;
    const double st[3] = {0.0, 1.0, 1e-4};                  // RunningMeanStd(epsilon=1e-4): mean 0, var 1, count 1e-4
    HIP_TRY(h, hipMemset(h->vn_returns, 0, sizeof(double) * h->n));
    HIP_TRY(h, hipMemcpy(h->vn_stats, st, sizeof st, hipMemcpyHostToDevice));
    return 0;
}

static int vn_scratch(ptg_env* h, int T)
{
    const int nW = (h->n + 63) / 64;
    const size_t need = (size_t)T * nW * 3;
    if (need > h->vn_partials_cap) {
        if (h->vn_partials) (void)hipFree(h->vn_partials);
        h->vn_partials = nullptr; h->vn_partials_cap = 0;
        if (hipMalloc((void**)&h->vn_partials, need * sizeof(double)) != hipSuccess) return set_err(h, PTG_E_HIP, "hipMalloc of %zu bytes failed", need * sizeof(double));
        h->vn_partials_cap = need;
    }
    if (T > h->vn_T_cap) {
        if (h->vn_den) (void)hipFree(h->vn_den);
        if (h->vn_moments) (void)hipFree(h->vn_moments);
        h->vn_den = h->vn_moments = nullptr; h->vn_T_cap = 0;
        if (hipMalloc((void**)&h->vn_den, sizeof(double) * T) != hipSuccess || hipMalloc((void**)&h->vn_moments, sizeof(double) * 3 * T) != hipSuccess)
            return set_err(h, PTG_E_HIP, "hipMalloc failed");
        h->vn_T_cap = T;
    }
    return 0;
}

int ptg_vn_batch_moments(ptg_env* h, const void* rew_dev, const uint8_t* done_dev, int n_steps, double* moments_dev, void* stream)
{
    if (!h || !rew_dev || !done_dev || n_steps < 1) return set_err(h, PTG_E_INVALID, "ptg_vn_batch_moments: bad argument");
    if (!h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_vn_batch_moments: call ptg_vn_init first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if ((rc = vn_scratch(h, n_steps))) return rc;
    hipStream_t st = as_stream(stream);
    const int nW = (h->n + 63) / 64;
    const dim3 grid(nW), block(64);
    if (h->cfg.out_dtype == PTG_OUT_F64)
        hipLaunchKernelGGL(k_vn_moments<double>, grid, block, 0, st, (const double*)rew_dev, done_dev, h->n, n_steps, h->vn_gamma, h->vn_returns, h->vn_partials, nW);
    else
        hipLaunchKernelGGL(k_vn_moments<float>, grid, block, 0, st, (const float*)rew_dev, done_dev, h->n, n_steps, h->vn_gamma, h->vn_returns, h->vn_partials, nW);
    hipLaunchKernelGGL(k_vn_merge, dim3(n_steps), dim3(64), 0, st, h->vn_partials, nW, moments_dev ? moments_dev : h->vn_moments);
    return launch_check(h, "k_vn_moments");
}

int ptg_vn_apply(ptg_env* h, const void* rew_dev, int n_steps, const double* moments_dev, void* rew_out_dev, int training, void* stream)
{
    if (!h || !rew_dev || !rew_out_dev || n_steps < 1) return set_err(h, PTG_E_INVALID, "ptg_vn_apply: bad argument");
    if (!h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_vn_apply: call ptg_vn_init first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if ((rc = vn_scratch(h, n_steps))) return rc;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_vn_scan, dim3(1), dim3(64), 0, st, moments_dev ? moments_dev : h->vn_moments, n_steps, training, h->vn_eps, h->vn_stats, h->vn_den);
    const size_t total = (size_t)n_steps * h->n;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (h->cfg.out_dtype == PTG_OUT_F64)
        hipLaunchKernelGGL(k_vn_norm<double>, grid, block, 0, st, (const double*)rew_dev, (double*)rew_out_dev, h->vn_den, h->n, total, h->vn_clip);
    else
        hipLaunchKernelGGL(k_vn_norm<float>, grid, block, 0, st, (const float*)rew_dev, (float*)rew_out_dev, h->vn_den, h->n, total, h->vn_clip);
    return launch_check(h, "k_vn_norm");
}

int ptg_vn_clear_done(ptg_env* h, const uint8_t* done_dev, int n_steps, void* stream)
{
    if (!h || !done_dev || n_steps < 1) return set_err(h, PTG_E_INVALID, "ptg_vn_clear_done: bad argument");
    if (!h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_vn_clear_done: call ptg_vn_init first");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_vn_clear_done, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, as_stream(stream), done_dev, h->n, n_steps, h->vn_returns);
    return launch_check(h, "k_vn_clear_done");
}

int ptg_vn_get(ptg_env* h, double* stats3_host, double* returns_host)
{
    if (!h || !h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_vn_get: not initialised");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (stats3_host) HIP_TRY(h, hipMemcpy(stats3_host, h->vn_stats, sizeof(double) * 3, hipMemcpyDeviceToHost));
    if (returns_host) HIP_TRY(h, hipMemcpy(returns_host, h->vn_returns, sizeof(double) * h->n, hipMemcpyDeviceToHost));
    return 0;
}

int ptg_vn_set(ptg_env* h, const double* stats3_host, const double* returns_host)
{
    if (!h || !h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_vn_set: not initialised");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (stats3_host) HIP_TRY(h, hipMemcpy(h->vn_stats, stats3_host, sizeof(double) * 3, hipMemcpyHostToDevice));
    if (returns_host) HIP_TRY(h, hipMemcpy(h->vn_returns, returns_host, sizeof(double) * h->n, hipMemcpyHostToDevice));
    return 0;
}

// ---- RolloutBuffer.compute_returns_and_advantage on the device ------------------------------------------------------
int ptg_gae(ptg_env* h, const void* rew_dev, const void* val_dev, const uint8_t* done_dev, const void* last_val_dev, int n_steps,
            int dtype, double gamma, double gae_lambda, void* adv_dev, void* ret_dev, void* stream)
{
    if (!h || !rew_dev || !val_dev || !done_dev || !last_val_dev || !adv_dev || n_steps < 1) return set_err(h, PTG_E_INVALID, "ptg_gae: bad argument");
    if (dtype != PTG_OUT_F32 && dtype != PTG_OUT_F64) return set_err(h, PTG_E_INVALID, "ptg_gae: bad dtype");
    if (!std::isfinite(gamma) || !std::isfinite(gae_lambda)) return set_err(h, PTG_E_INVALID, "ptg_gae: gamma / gae_lambda must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    const double gl = gamma * gae_lambda;                   // Python's float product, before it meets the array's dtype
    const dim3 grid((unsigned)((h->n + 63) / 64)), block(64);
    // 32 (float64: 16) steps of loads in flight per lane: 18 KiB per wave, 72 KiB per CU at the 4 waves per CU of 65 536 envs
    if (dtype == PTG_OUT_F64)
        hipLaunchKernelGGL((k_gae<double, 16>), grid, block, 0, as_stream(stream), (const double*)rew_dev, (const double*)val_dev, done_dev,
                           (const double*)last_val_dev, h->n, n_steps, gamma, gl, (double*)adv_dev, (double*)ret_dev);
    else
        hipLaunchKernelGGL((k_gae<float, 32>), grid, block, 0, as_stream(stream), (const float*)rew_dev, (const float*)val_dev, done_dev,
                           (const float*)last_val_dev, h->n, n_steps, (float)gamma, (float)gl, (float*)adv_dev, (float*)ret_dev);
    return launch_check(h, "k_gae");
}

// ---- RolloutBuffer.get's _get_samples on the device: one minibatch per launch ---------------------------------------
// ptg_minibatch (the caller's indices) and ptg_minibatch_drawn (`drawn`, idx_dev null: the indices drawn on the device, the cursor
// advanced behind the gather) share every check and the launch; `who` names the entry point in the refusal
static int minibatch_gather(ptg_env* h, const char* who, bool drawn, const void* idx_dev, int idx_bytes, uint64_t* cursor_dev, uint64_t seed,
                            int64_t* idx_out_dev, int64_t batch, int n_steps, const void* obs_dev, int64_t obs_s_t, int64_t obs_s_n, int64_t obs_s_f, int obs_dim, int obs_bytes,
                            void* obs_out_dev, int n_cols, const void* const* cols_host, const int* col_bytes_host, void* const* cols_out_host, void* stream)
{
    if (!h || (!drawn && !idx_dev) || batch < 1 || n_steps < 1) return set_err(h, PTG_E_INVALID, "%s: bad argument", who);
    if (!drawn && idx_bytes != 4 && idx_bytes != 8) return set_err(h, PTG_E_INVALID, "%s: indices must be int32 or int64", who);
    if (batch > (int64_t)0x7FFFFFFF * (MB_ROWS * MB_WAVES)) return set_err(h, PTG_E_INVALID, "%s: batch too large for one launch", who);
    if ((obs_dev == nullptr) != (obs_out_dev == nullptr)) return set_err(h, PTG_E_INVALID, "%s: observations and their output go together", who);
    if (obs_dev && (obs_dim < 1 || obs_dim > (1 << 20) || (obs_bytes != 4 && obs_bytes != 8) || obs_s_t < 0 || obs_s_n < 0 || obs_s_f < 0))
        return set_err(h, PTG_E_INVALID, "%s: bad observation shape (obs_dim in [1, 2^20], 4- or 8-byte elements, strides >= 0)", who);
    if (n_cols < 0 || n_cols > PTG_MB_MAX_COLS) return set_err(h, PTG_E_INVALID, "%s: at most %d columns", who, PTG_MB_MAX_COLS);
    if (n_cols > 0 && (!cols_host || !col_bytes_host || !cols_out_host)) return set_err(h, PTG_E_INVALID, "%s: null column arrays", who);
    if (!obs_dev && n_cols == 0) return set_err(h, PTG_E_INVALID, "%s: nothing to gather", who);
    MbCols cols{};
    cols.n = n_cols;
    for (int c = 0; c < n_cols; c++) {
        const int s = col_bytes_host[c];
        if (!cols_host[c] || !cols_out_host[c]) return set_err(h, PTG_E_INVALID, "%s: column %d or its output is null", who, c);
        if (s != 1 && s != 2 && s != 4 && s != 8) return set_err(h, PTG_E_INVALID, "%s: column %d has %d-byte elements (1, 2, 4 or 8)", who, c, s);
        cols.src[c] = cols_host[c]; cols.dst[c] = cols_out_host[c]; cols.bytes[c] = s;
    }
    const size_t B = (size_t)batch, N = (size_t)h->n, sz = (size_t)obs_bytes;
    const unsigned T = (unsigned)n_steps;
    MbDraw draw{};
    if (drawn) {
        const uint64_t TN = (uint64_t)N * T;
        if (!cursor_dev) return set_err(h, PTG_E_INVALID, "%s: null cursor", who);
        if (TN % B != 0) return set_err(h, PTG_E_INVALID, "%s: a batch of %lld rows does not divide the %llu rows of the rollout", who, (long long)batch, (unsigned long long)TN);
        if (TN > PTG_MB_DRAWN_MAX_ROWS) return set_err(h, PTG_E_INVALID, "%s: more than 2^48 rows", who);
        unsigned n = 2;                                      // max(2, bit_length(TN - 1))
        while (n < 64 && ((TN - 1) >> n) != 0) n++;
        draw = MbDraw{(const unsigned long long*)cursor_dev, (unsigned long long)seed, (long long*)idx_out_dev, n / 2, n - n / 2};
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const char* obs = (const char*)obs_dev;
    char* out = (char*)obs_out_dev;
    const size_t row_bytes = obs_dev ? (size_t)obs_dim * sz : 0, s_t = (size_t)obs_s_t * sz, s_n = (size_t)obs_s_n * sz;
    // 16-byte pieces when a row is contiguous, a whole number of them, and every row starts on one -- in the buffer and in the output
    const bool wide = obs_dev && obs_s_f == 1 && row_bytes % 16 == 0 && s_t % 16 == 0 && s_n % 16 == 0 &&
                      (uintptr_t)obs % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (wide) launch_minibatch<uint4>(st, idx_dev, idx_bytes, draw, B, T, N, obs, s_t, s_n, 16, (unsigned)(row_bytes / 16), out, cols, h->P.err);
    else if (obs_bytes == 8) launch_minibatch<uint64_t>(st, idx_dev, idx_bytes, draw, B, T, N, obs, s_t, s_n, (size_t)obs_s_f * 8, (unsigned)obs_dim, out, cols, h->P.err);
    else launch_minibatch<uint32_t>(st, idx_dev, idx_bytes, draw, B, T, N, obs, s_t, s_n, (size_t)obs_s_f * 4, obs_dev ? (unsigned)obs_dim : 1u, out, cols, h->P.err);
    if (drawn) hipLaunchKernelGGL(k_mb_cursor, dim3(1), dim3(1), 0, st, (unsigned long long*)cursor_dev, (unsigned long long)((uint64_t)N * T / B), 0);
    return launch_check(h, "k_minibatch");
}

int ptg_minibatch(ptg_env* h, const void* idx_dev, int idx_bytes, int64_t batch, int n_steps, const void* obs_dev, int64_t obs_s_t,
                  int64_t obs_s_n, int64_t obs_s_f, int obs_dim, int obs_bytes, void* obs_out_dev, int n_cols, const void* const* cols_host,
                  const int* col_bytes_host, void* const* cols_out_host, void* stream)
{
    return minibatch_gather(h, "ptg_minibatch", false, idx_dev, idx_bytes, nullptr, 0, nullptr, batch, n_steps, obs_dev, obs_s_t, obs_s_n, obs_s_f, obs_dim,
                            obs_bytes, obs_out_dev, n_cols, cols_host, col_bytes_host, cols_out_host, stream);
}

int ptg_minibatch_drawn(ptg_env* h, uint64_t* cursor_dev, uint64_t seed, int64_t* idx_out_dev, int64_t batch, int n_steps, const void* obs_dev,
                        int64_t obs_s_t, int64_t obs_s_n, int64_t obs_s_f, int obs_dim, int obs_bytes, void* obs_out_dev, int n_cols,
                        const void* const* cols_host, const int* col_bytes_host, void* const* cols_out_host, void* stream)
{
    return minibatch_gather(h, "ptg_minibatch_drawn", true, nullptr, 0, cursor_dev, seed, idx_out_dev, batch, n_steps, obs_dev, obs_s_t, obs_s_n, obs_s_f,
                            obs_dim, obs_bytes, obs_out_dev, n_cols, cols_host, col_bytes_host, cols_out_host, stream);
}

int ptg_minibatch_end_epoch(ptg_env* h, uint64_t* cursor_dev, void* stream)
{
    if (!h || !cursor_dev) return set_err(h, PTG_E_INVALID, "ptg_minibatch_end_epoch: null handle or cursor");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_mb_cursor, dim3(1), dim3(1), 0, as_stream(stream), (unsigned long long*)cursor_dev, 0ull, 1);
    return launch_check(h, "k_mb_cursor");
}

// ---- ReplayBuffer.add / sample on the device, over the caller's rings ------------------------------------------------
static const char* replay_desc_error(const ptg_replay* rb)
{
    if (!rb) return "null descriptor";
    if (!rb->obs_ring || !rb->next_ring || !rb->cursor_dev) return "null ring or cursor in the descriptor";
    if (rb->capacity < 1) return "capacity < 1";
    if (rb->obs_dim < 1 || rb->obs_dim > (1 << 20) || (rb->obs_bytes != 4 && rb->obs_bytes != 8)) return "obs_dim outside [1, 2^20] or obs_bytes other than 4 | 8";
    if (rb->n_cols < 0 || rb->n_cols > PTG_MB_MAX_COLS) return "n_cols outside [0, 8]";
    for (int c = 0; c < rb->n_cols; c++) {
        const int s = rb->col_bytes[c];
        if (!rb->col_ring[c]) return "null column ring";
        if (s != 1 && s != 2 && s != 4 && s != 8) return "a column element size other than 1 | 2 | 4 | 8";
    }
    return nullptr;
}

int ptg_replay_add(ptg_env* h, const ptg_replay* rb, const void* prev_obs_dev, const void* obs_dev, int64_t obs_s_t, int64_t obs_s_n,
                   int64_t obs_s_f, const void* final_obs_dev, const uint8_t* done_dev, int done_col, int n_cols, const void* const* cols_host,
                   int64_t n_steps, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (const char* why = replay_desc_error(rb)) return set_err(h, PTG_E_INVALID, "ptg_replay_add: %s", why);
    if (!prev_obs_dev || !obs_dev) return set_err(h, PTG_E_INVALID, "ptg_replay_add: null observations");
    if (n_steps < 1 || n_steps > rb->capacity || n_steps > 0x7FFFFFFF) return set_err(h, PTG_E_INVALID, "ptg_replay_add: n_steps outside [1, capacity]");
    if (obs_s_t < 0 || obs_s_n < 0 || obs_s_f < 0) return set_err(h, PTG_E_INVALID, "ptg_replay_add: negative stride");
    if (n_cols != rb->n_cols || (n_cols > 0 && !cols_host)) return set_err(h, PTG_E_INVALID, "ptg_replay_add: n_cols differs from the descriptor's, or null column array");
    if (done_col < -1 || done_col >= n_cols) return set_err(h, PTG_E_INVALID, "ptg_replay_add: done_col outside [-1, n_cols)");
    if (done_col >= 0 && rb->col_bytes[done_col] != 4) return set_err(h, PTG_E_INVALID, "ptg_replay_add: the done column must have 4-byte (float32) elements");
    if ((done_col >= 0 || final_obs_dev) && !done_dev) return set_err(h, PTG_E_INVALID, "ptg_replay_add: done_dev is needed by final_obs_dev and by the done column");
    RbAdd a{};
    for (int c = 0; c < n_cols; c++) {
        if (c != done_col && !cols_host[c]) return set_err(h, PTG_E_INVALID, "ptg_replay_add: column %d is null", c);
        a.cols.src[c] = cols_host[c]; a.cols.dst[c] = rb->col_ring[c]; a.cols.bytes[c] = rb->col_bytes[c];
    }
    a.cols.n = n_cols;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const size_t sz = (size_t)rb->obs_bytes, N = (size_t)h->n, row_bytes = (size_t)rb->obs_dim * sz;
    a.prev = (const char*)prev_obs_dev; a.obs = (const char*)obs_dev; a.fin = (const char*)final_obs_dev; a.done = done_dev;
    a.s_t = (size_t)obs_s_t * sz; a.s_n = (size_t)obs_s_n * sz; a.s_f = (size_t)obs_s_f * sz;
    a.ring0 = (char*)rb->obs_ring; a.ring1 = (char*)rb->next_ring; a.cursor = (const unsigned long long*)rb->cursor_dev;
    a.S = (size_t)rb->capacity; a.N = N; a.T = (unsigned)n_steps; a.F = (unsigned)rb->obs_dim; a.done_col = done_col;
    const unsigned gy = (unsigned)std::min<int64_t>(n_steps, 65535);
    if (obs_s_f == 1) {
        // 16-byte pieces when a row is a whole number of them and every row starts on one, in the sources and in the rings
        const auto al = [](const void* q) { return (uintptr_t)q % 16 == 0; };
        const bool wide = row_bytes % 16 == 0 && a.s_t % 16 == 0 && a.s_n % 16 == 0 && al(a.prev) && al(a.obs) && al(a.fin) && al(a.ring0) && al(a.ring1);
        const unsigned P = wide ? (unsigned)(row_bytes / 16) : (unsigned)rb->obs_dim;
        const size_t NP = N * P;
        const dim3 grid((unsigned)((NP + 255) / 256), gy), block(256);
        if (wide) hipLaunchKernelGGL(k_rb_add<uint4>, grid, block, 0, st, a, P, NP);
        else if (sz == 8) hipLaunchKernelGGL(k_rb_add<uint64_t>, grid, block, 0, st, a, P, NP);
        else hipLaunchKernelGGL(k_rb_add<uint32_t>, grid, block, 0, st, a, P, NP);
    } else {
        const dim3 grid((unsigned)((N + RB_TE - 1) / RB_TE), gy), block(256);
        if (sz == 8) hipLaunchKernelGGL(k_rb_add_tr<uint64_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_rb_add_tr<uint32_t>, grid, block, 0, st, a);
    }
    hipLaunchKernelGGL(k_rb_bump, dim3(1), dim3(1), 0, st, (unsigned long long*)rb->cursor_dev, (unsigned long long)n_steps);
    return launch_check(h, "k_rb_add");
}

int ptg_replay_sample(ptg_env* h, const ptg_replay* rb, const int64_t* idx_dev, int64_t batch, uint64_t seed, void* obs_out_dev,
                      void* next_obs_out_dev, void* const* cols_out_host, int norm_col, int64_t* idx_out_dev, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (const char* why = replay_desc_error(rb)) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: %s", why);
    if (batch < 1 || batch > (int64_t)0x7FFFFFFF * (MB_ROWS * MB_WAVES)) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: batch < 1 or too large for one launch");
    if (norm_col < -1 || norm_col >= rb->n_cols) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: norm_col outside [-1, n_cols)");
    MbCols cols{};
    cols.n = rb->n_cols;
    bool any = obs_out_dev || next_obs_out_dev || idx_out_dev;
    for (int c = 0; c < rb->n_cols; c++) {
        cols.src[c] = rb->col_ring[c]; cols.dst[c] = cols_out_host ? cols_out_host[c] : nullptr; cols.bytes[c] = rb->col_bytes[c];
        any = any || cols.dst[c];
    }
    if (!any) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: no output");
    RbNorm norm{-1, nullptr, 0.0, 0.0};
    if (norm_col >= 0) {
        if (!h->vn_returns) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: norm_col needs ptg_vn_init first");
        if (rb->col_bytes[norm_col] != (h->cfg.out_dtype == PTG_OUT_F64 ? 8 : 4))
            return set_err(h, PTG_E_INVALID, "ptg_replay_sample: the reward column's element size differs from the handle's out_dtype");
        if (!cols.dst[norm_col]) return set_err(h, PTG_E_INVALID, "ptg_replay_sample: norm_col names a column without an output");
        norm = RbNorm{norm_col, h->vn_stats, h->vn_eps, h->vn_clip};
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const size_t B = (size_t)batch, N = (size_t)h->n, row_bytes = (size_t)rb->obs_dim * (size_t)rb->obs_bytes;
    const char *r0 = (const char*)rb->obs_ring, *r1 = (const char*)rb->next_ring;
    char *o0 = (char*)obs_out_dev, *o1 = (char*)next_obs_out_dev;
    const unsigned long long* cur = (const unsigned long long*)rb->cursor_dev;
    const auto al = [](const void* q) { return (uintptr_t)q % 16 == 0; };
    const bool wide = row_bytes % 16 == 0 && al(r0) && al(r1) && al(o0) && al(o1);
    const dim3 grid((unsigned)((B + MB_ROWS * MB_WAVES - 1) / (MB_ROWS * MB_WAVES))), block(64 * MB_WAVES);
    const long long* idx = (const long long*)idx_dev;
    long long* idx_out = (long long*)idx_out_dev;
    const size_t S = (size_t)rb->capacity;
    if (wide) hipLaunchKernelGGL(k_rb_sample<uint4>, grid, block, 0, st, idx, B, (unsigned long long)seed, cur, S, N, row_bytes, (unsigned)(row_bytes / 16), r0, r1, o0, o1, cols, norm, idx_out, h->P.err);
    else if (rb->obs_bytes == 8) hipLaunchKernelGGL(k_rb_sample<uint64_t>, grid, block, 0, st, idx, B, (unsigned long long)seed, cur, S, N, row_bytes, (unsigned)rb->obs_dim, r0, r1, o0, o1, cols, norm, idx_out, h->P.err);
    else hipLaunchKernelGGL(k_rb_sample<uint32_t>, grid, block, 0, st, idx, B, (unsigned long long)seed, cur, S, N, row_bytes, (unsigned)rb->obs_dim, r0, r1, o0, o1, cols, norm, idx_out, h->P.err);
    if (!idx_dev) hipLaunchKernelGGL(k_rb_bump, dim3(1), dim3(1), 0, st, (unsigned long long*)rb->cursor_dev + 1, 1ull);
    return launch_check(h, "k_rb_sample");
}

// ---- RolloutBuffer.reset / add on the device, over the caller's rows --------------------------------------------------
// begin (cols_host unused) and add share every check and the launch; `who` names the entry point in the refusal
static int rollout_buffer_store(ptg_env* h, const char* who, bool begin, const ptg_rollout_buffer* rb, const void* obs_dev, int64_t obs_s_n,
                                int64_t obs_s_f, int64_t row_pitch, int n_cols, const void* const* cols_host, const int64_t* col_stride_host, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!rb) return set_err(h, PTG_E_INVALID, "%s: null descriptor", who);
    if (!rb->obs_rows || !rb->cursor_dev) return set_err(h, PTG_E_INVALID, "%s: null obs_rows or cursor in the descriptor", who);
    if (rb->n_steps < 1) return set_err(h, PTG_E_INVALID, "%s: n_steps < 1", who);
    if (rb->obs_dim < 1 || rb->obs_dim > (1 << 20) || (rb->obs_bytes != 4 && rb->obs_bytes != 8))
        return set_err(h, PTG_E_INVALID, "%s: obs_dim outside [1, 2^20] or obs_bytes other than 4 | 8", who);
    if (rb->n_cols < 0 || rb->n_cols > PTG_MB_MAX_COLS) return set_err(h, PTG_E_INVALID, "%s: n_cols outside [0, 8]", who);
    for (int c = 0; c < rb->n_cols; c++) {
        const int s = rb->col_bytes[c];
        if (!rb->col_rows[c]) return set_err(h, PTG_E_INVALID, "%s: column %d of the descriptor is null", who, c);
        if (s != 1 && s != 2 && s != 4 && s != 8) return set_err(h, PTG_E_INVALID, "%s: column %d has %d-byte elements (1, 2, 4 or 8)", who, c, s);
    }
    if (!obs_dev) return set_err(h, PTG_E_INVALID, "%s: null observations", who);
    if (obs_s_n < 0 || obs_s_f < 0 || row_pitch < 0) return set_err(h, PTG_E_INVALID, "%s: negative stride or pitch", who);
    RoAdd a{};
    if (!begin) {
        if (n_cols != rb->n_cols || (n_cols > 0 && (!cols_host || !col_stride_host)))
            return set_err(h, PTG_E_INVALID, "%s: n_cols differs from the descriptor's, or null column arrays", who);
        for (int c = 0; c < n_cols; c++) {
            if (!cols_host[c]) return set_err(h, PTG_E_INVALID, "%s: column %d is null", who, c);
            if (col_stride_host[c] < 1) return set_err(h, PTG_E_INVALID, "%s: column %d has stride %lld (>= 1)", who, c, (long long)col_stride_host[c]);
            a.col_src[c] = (const char*)cols_host[c]; a.col_dst[c] = (char*)rb->col_rows[c]; a.col_bytes[c] = rb->col_bytes[c];
            a.col_stride[c] = (size_t)col_stride_host[c] * (size_t)rb->col_bytes[c];
        }
        a.n_cols = n_cols;
    }
    const size_t sz = (size_t)rb->obs_bytes, N = (size_t)h->n, F = (size_t)rb->obs_dim, s_n = (size_t)obs_s_n, s_f = (size_t)obs_s_f;
    a.obs = (const char*)obs_dev; a.rows = (char*)rb->obs_rows; a.cursor = (unsigned long long*)rb->cursor_dev; a.err = h->P.err;
    a.row_bytes = (size_t)row_pitch * sz; a.T = (size_t)rb->n_steps; a.N = N;
    // one contiguous run of N * F elements: [N][F] rows back to back, or [F][N] planes back to back
    const bool run = ((F == 1 || s_f == 1) && (N == 1 || s_n == F)) || ((N == 1 || s_n == 1) && (F == 1 || s_f == N));
    bool wide = false;
    if (run) {
        const auto al = [](const void* q) { return (uintptr_t)q % 16 == 0; };
        wide = (N * F * sz) % 16 == 0 && a.row_bytes % 16 == 0 && al(a.obs) && al(a.rows);
        a.units = a.inner = wide ? N * F * sz / 16 : N * F;
    } else {
        a.units = N * F;
        if (s_n == 1) { a.inner = N; a.s_inner = sz; a.s_outer = s_f * sz; }          // planes at a pitch: the lanes along the envs
        else { a.inner = F; a.s_inner = s_f * sz; a.s_outer = s_n * sz; }
    }
    const size_t per = 256 * RO_U, blocks = std::max((a.units + per - 1) / per, begin ? (size_t)1 : (N + 255) / 256);
    if (blocks > 0x7FFFFFFFull) return set_err(h, PTG_E_INVALID, "%s: the block is too large for one launch", who);
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)blocks), block(256);
    if (wide) hipLaunchKernelGGL(k_ro_add<uint4>, grid, block, 0, st, a, (int)begin);
    else if (sz == 8) hipLaunchKernelGGL(k_ro_add<uint64_t>, grid, block, 0, st, a, (int)begin);
    else hipLaunchKernelGGL(k_ro_add<uint32_t>, grid, block, 0, st, a, (int)begin);
#if PTG_RO_FORM == 0
    if (!begin) hipLaunchKernelGGL(k_ro_bump, dim3(1), dim3(1), 0, st, a.cursor, (unsigned long long)a.T, a.err);
#endif
    return launch_check(h, "k_ro_add");
}

int ptg_rollout_buffer_begin(ptg_env* h, const ptg_rollout_buffer* rb, const void* obs_dev, int64_t obs_s_n, int64_t obs_s_f, int64_t row_pitch,
                             void* stream)
{
    return rollout_buffer_store(h, "ptg_rollout_buffer_begin", true, rb, obs_dev, obs_s_n, obs_s_f, row_pitch, 0, nullptr, nullptr, stream);
}

int ptg_rollout_buffer_add(ptg_env* h, const ptg_rollout_buffer* rb, const void* obs_dev, int64_t obs_s_n, int64_t obs_s_f, int64_t row_pitch,
                           int n_cols, const void* const* cols_host, const int64_t* col_stride_host, void* stream)
{
    return rollout_buffer_store(h, "ptg_rollout_buffer_add", false, rb, obs_dev, obs_s_n, obs_s_f, row_pitch, n_cols, cols_host, col_stride_host, stream);
}

// ---- the action head: policy outputs -> actions, log-probs, entropy ----------------------------------------------------
int ptg_act(ptg_env* h, const ptg_head* hd, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!hd) return set_err(h, PTG_E_INVALID, "ptg_act: null head");
    const int kind = hd->kind, flags = hd->flags;
    if (kind != PTG_HEAD_CATEGORICAL && kind != PTG_HEAD_EPS_GREEDY && kind != PTG_HEAD_GAUSSIAN) return set_err(h, PTG_E_INVALID, "ptg_act: unknown kind %d", kind);
    if (flags & ~(PTG_HEAD_DETERMINISTIC | PTG_HEAD_SQUASH)) return set_err(h, PTG_E_INVALID, "ptg_act: unknown flag in %d", flags);
    const bool gauss = kind == PTG_HEAD_GAUSSIAN, det = (flags & PTG_HEAD_DETERMINISTIC) != 0, squash = (flags & PTG_HEAD_SQUASH) != 0;
    if (squash && !gauss) return set_err(h, PTG_E_INVALID, "ptg_act: PTG_HEAD_SQUASH applies to the Gaussian head only");
    if (!hd->in_dev || !hd->act_dev) return set_err(h, PTG_E_INVALID, "ptg_act: null input or action output");
    if (!det && !hd->counter_dev) return set_err(h, PTG_E_INVALID, "ptg_act: a stochastic head needs counter_dev");
    if (hd->in_dtype != PTG_OUT_F32 && hd->in_dtype != PTG_OUT_F64) return set_err(h, PTG_E_INVALID, "ptg_act: in_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (gauss) {
        if (hd->in_s_n < 1) return set_err(h, PTG_E_INVALID, "ptg_act: in_s_n < 1");
        if (hd->act_kind != PTG_ACT_F32) return set_err(h, PTG_E_INVALID, "ptg_act: the Gaussian head writes PTG_ACT_F32 actions");
        if (!hd->param_dev) return set_err(h, PTG_E_INVALID, "ptg_act: the Gaussian head needs log_std in param_dev");
        if (hd->param_s_n != 0 && hd->param_s_n != 1) return set_err(h, PTG_E_INVALID, "ptg_act: param_s_n must be 0 or 1");
        if (!(hd->clip_lo <= hd->clip_hi)) return set_err(h, PTG_E_INVALID, "ptg_act: clip_lo > clip_hi (or a NaN bound)");
        if (squash && hd->ent_dev) return set_err(h, PTG_E_INVALID, "ptg_act: a squashed Gaussian has no closed-form entropy");
    } else {
        if (hd->n_actions < 2 || hd->n_actions > 32) return set_err(h, PTG_E_INVALID, "ptg_act: n_actions outside [2, 32]");
        if (hd->in_s_n < hd->n_actions) return set_err(h, PTG_E_INVALID, "ptg_act: in_s_n < n_actions");
        if (hd->act_kind != PTG_ACT_I32 && hd->act_kind != PTG_ACT_I64) return set_err(h, PTG_E_INVALID, "ptg_act: a discrete head writes PTG_ACT_I32 or PTG_ACT_I64 actions");
        if (hd->raw_dev) return set_err(h, PTG_E_INVALID, "ptg_act: raw_dev is the Gaussian head's");
        if (kind == PTG_HEAD_EPS_GREEDY) {
            if (hd->logp_dev || hd->ent_dev) return set_err(h, PTG_E_INVALID, "ptg_act: epsilon-greedy has no log-prob or entropy");
            if (!det && !hd->param_dev) return set_err(h, PTG_E_INVALID, "ptg_act: epsilon-greedy needs epsilon in param_dev");
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    ActArgs a{};
    a.in = hd->in_dev; a.s_n = (size_t)hd->in_s_n; a.param = hd->param_dev; a.param_s = gauss ? (size_t)hd->param_s_n : 0;
    a.act = hd->act_dev; a.raw = hd->raw_dev; a.logp = hd->logp_dev; a.ent = hd->ent_dev;
    a.counter = det ? nullptr : (const unsigned long long*)hd->counter_dev; a.seed = (unsigned long long)hd->seed; a.env_offset = h->P.env_offset;
    a.lo = hd->clip_lo; a.hi = hd->clip_hi; a.N = (size_t)h->n; a.A = hd->n_actions; a.kind = kind; a.flags = flags; a.act_kind = hd->act_kind;
    a.err = h->P.err;
    const dim3 grid((unsigned)((a.N + ACT_BLOCK - 1) / ACT_BLOCK)), block(ACT_BLOCK);
    if (hd->in_dtype == PTG_OUT_F64) hipLaunchKernelGGL(k_act<double>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_act<float>, grid, block, 0, st, a);
    if (!det) hipLaunchKernelGGL(k_rb_bump, dim3(1), dim3(1), 0, st, (unsigned long long*)hd->counter_dev, 1ull);
    return launch_check(h, "k_act");
}

// ---- the policy loss: PPO / A2C loss, SB3's logged statistics and the gradients w.r.t. the network's outputs --------------
int64_t ptg_policy_loss_workspace(int64_t batch)
{
    if (batch < 1) return PTG_E_INVALID;
    if (batch > (int64_t)1 << 31) return PTG_E_INVALID;     // 2^23 blocks of 256 threads: half of the 2^32 threads one launch may have
    const int64_t nblk = loss_blocks(batch, PL_BLOCK);
    return (4 + nblk * 3) * (int64_t)sizeof(double) + loss_partials_bytes(nblk);
}

// THE policy loss: ptg_policy_loss is this walk over one descriptor with the single kernels, ptg_policy_loss_group the same walk with
// the grouped ones.  `grouped` is the entry that was called, not n_members > 1: a group of one launches the grouped kernels
static int policy_loss_walk(ptg_env* h, const char* who, const ptg_loss* members, int n_members, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = train_refuse(h, who, members, n_members, grouped, loss_desc_fault,
                              [&](char* why, size_t cap) { return loss_group_fault(members, n_members, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_loss* d = &members[0];     // batch, dtype and flags: the group's
    TrainGroup<LossArgs> g{};
    for (int i = 0; i < n_members; i++) g.m[i] = loss_args(h, &members[i]);
    const LossArgs& a = g.m[0];
    const bool f64 = d->in_dtype == PTG_OUT_F64, norm = (d->flags & PTG_LOSS_NORM_ADV) != 0 && d->batch > 1;
    const dim3 block(PL_BLOCK), rows((unsigned)a.nblk, (unsigned)n_members), per_member((unsigned)n_members);
    if (!grouped) {
        if (a.nblk > 1 && norm) {                            // PPO's minibatch is one block, which takes its moments itself
            const dim3 grid((unsigned)a.nblk);
            if (f64) hipLaunchKernelGGL(k_pl_moments<double>, grid, block, 0, st, a);
            else hipLaunchKernelGGL(k_pl_moments<float>, grid, block, 0, st, a);
            hipLaunchKernelGGL(k_vn_merge, dim3(1), dim3(64), 0, st, (const double*)(a.ws + 4), a.nblk, a.ws);
        }
        if (f64) launch_loss<PlFinal<double>>(st, a, pl_partials(a), k_pl_rows<double, true>, k_pl_rows<double, false>);
        else launch_loss<PlFinal<float>>(st, a, pl_partials(a), k_pl_rows<float, true>, k_pl_rows<float, false>);
        return launch_check(h, "k_pl_rows");
    }
    if (a.nblk > 1 && norm) {
        if (f64) hipLaunchKernelGGL((k_pl_moments<double, TrainGroup<LossArgs>>), rows, block, 0, st, g);
        else hipLaunchKernelGGL((k_pl_moments<float, TrainGroup<LossArgs>>), rows, block, 0, st, g);
        hipLaunchKernelGGL(k_pl_merge_group, per_member, dim3(64), 0, st, g);
    }
    if (a.nblk == 1) {
        if (f64) hipLaunchKernelGGL((k_pl_rows<double, true, TrainGroup<LossArgs>>), rows, block, 0, st, g);
        else hipLaunchKernelGGL((k_pl_rows<float, true, TrainGroup<LossArgs>>), rows, block, 0, st, g);
    } else {
        if (f64) hipLaunchKernelGGL((k_pl_rows<double, false, TrainGroup<LossArgs>>), rows, block, 0, st, g);
        else hipLaunchKernelGGL((k_pl_rows<float, false, TrainGroup<LossArgs>>), rows, block, 0, st, g);
        if (f64) hipLaunchKernelGGL((k_loss_final<LossArgs, PlFinal<double>, TrainGroup<LossArgs>>), per_member, block, 0, st, g, (const double*)nullptr);
        else hipLaunchKernelGGL((k_loss_final<LossArgs, PlFinal<float>, TrainGroup<LossArgs>>), per_member, block, 0, st, g, (const double*)nullptr);
    }
    return launch_check(h, "k_pl_rows (grouped)");
}

int ptg_policy_loss(ptg_env* h, const ptg_loss* d, void* stream) { return policy_loss_walk(h, "ptg_policy_loss", d, 1, false, stream); }

int ptg_policy_loss_group(ptg_env* h, const ptg_loss* members, int32_t n_members, void* stream)
{
    return policy_loss_walk(h, "ptg_policy_loss_group", members, n_members, true, stream);
}

// ---- gSDE: the exploration matrix, the collecting head, the PPO / A2C loss ----------------------------------------------
static bool sde_dtype_ok(int dt) { return dt == PTG_OUT_F32 || dt == PTG_OUT_F64; }
static bool sde_width_ok(int L) { return L >= 1 && L <= PTG_MLP_MAX_WIDTH; }

// ptg_sde_resample and ptg_sde_resample_rows: `rows` rows whose keys start at the global row `offset`
static int sde_resample(ptg_env* h, const char* who, const ptg_sde_noise* d, long long offset, int64_t rows, void* stream)
{
    if (!d) return set_err(h, PTG_E_INVALID, "%s: null descriptor", who);
    if (!sde_dtype_ok(d->in_dtype)) return set_err(h, PTG_E_INVALID, "%s: in_dtype must be PTG_OUT_F32 or PTG_OUT_F64", who);
    if (!sde_width_ok(d->latent_dim)) return set_err(h, PTG_E_INVALID, "%s: latent_dim %d outside [1, %d]", who, d->latent_dim, PTG_MLP_MAX_WIDTH);
    if (!d->log_std_dev || !d->counter_dev || !d->e_dev) return set_err(h, PTG_E_INVALID, "%s: null log_std_dev, counter_dev or e_dev", who);
    if (d->e_s_n < d->latent_dim) return set_err(h, PTG_E_INVALID, "%s: e_s_n < latent_dim", who);
    if (rows < 1 || rows > (int64_t)1 << 31) return set_err(h, PTG_E_INVALID, "%s: rows %lld outside [1, 2^31]", who, (long long)rows);
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    SdeNoiseArgs a{};
    a.log_std = d->log_std_dev; a.E = d->e_dev; a.e_s = (size_t)d->e_s_n; a.counter = (const unsigned long long*)d->counter_dev;
    a.seed = (unsigned long long)d->seed; a.env_offset = offset; a.N = (size_t)rows; a.L = d->latent_dim; a.err = h->P.err;
    a.rows_per_block = (a.N - 1) / SDE_MAX_BLOCKS + 1;
    const dim3 grid((unsigned)((a.L + 63) / 64), (unsigned)((a.N - 1) / a.rows_per_block + 1)), block(64);
    if (d->in_dtype == PTG_OUT_F64) hipLaunchKernelGGL(k_sde_resample<double>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_sde_resample<float>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_rb_bump, dim3(1), dim3(1), 0, st, (unsigned long long*)d->counter_dev, 1ull);
    return launch_check(h, "k_sde_resample");
}

int ptg_sde_resample(ptg_env* h, const ptg_sde_noise* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    return sde_resample(h, "ptg_sde_resample", d, h->P.env_offset, h->n, stream);        // a row is an env
}

int ptg_sde_act(ptg_env* h, const ptg_sde_head* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!d) return set_err(h, PTG_E_INVALID, "ptg_sde_act: null descriptor");
    if (d->flags & ~PTG_HEAD_DETERMINISTIC) return set_err(h, PTG_E_INVALID, "ptg_sde_act: unknown flag in %d", d->flags);
    const bool det = (d->flags & PTG_HEAD_DETERMINISTIC) != 0;
    if (!sde_dtype_ok(d->in_dtype)) return set_err(h, PTG_E_INVALID, "ptg_sde_act: in_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!sde_width_ok(d->latent_dim)) return set_err(h, PTG_E_INVALID, "ptg_sde_act: latent_dim %d outside [1, %d]", d->latent_dim, PTG_MLP_MAX_WIDTH);
    if (d->act_kind != PTG_ACT_F32) return set_err(h, PTG_E_INVALID, "ptg_sde_act: the head writes PTG_ACT_F32 actions");
    if (!d->mean_dev || !d->latent_dev || !d->log_std_dev || !d->act_dev) return set_err(h, PTG_E_INVALID, "ptg_sde_act: null mean_dev, latent_dev, log_std_dev or act_dev");
    if (!det && !d->e_dev) return set_err(h, PTG_E_INVALID, "ptg_sde_act: a stochastic head needs e_dev");
    if (d->mean_s_n < 1) return set_err(h, PTG_E_INVALID, "ptg_sde_act: mean_s_n < 1");
    if (d->latent_s_n < d->latent_dim) return set_err(h, PTG_E_INVALID, "ptg_sde_act: latent_s_n < latent_dim");
    if (!det && d->e_s_n < d->latent_dim) return set_err(h, PTG_E_INVALID, "ptg_sde_act: e_s_n < latent_dim");
    if (!(d->clip_lo <= d->clip_hi)) return set_err(h, PTG_E_INVALID, "ptg_sde_act: clip_lo > clip_hi (or a NaN bound)");
    HIP_TRY(h, hipSetDevice(h->device));
    SdeActArgs a{};
    a.mean = d->mean_dev; a.m_s = (size_t)d->mean_s_n; a.lat = d->latent_dev; a.lat_s = (size_t)d->latent_s_n;
    a.E = det ? nullptr : d->e_dev; a.e_s = det ? 0 : (size_t)d->e_s_n; a.log_std = d->log_std_dev;
    a.act = d->act_dev; a.raw = d->raw_dev; a.logp = d->logp_dev; a.ent = d->ent_dev;
    a.lo = d->clip_lo; a.hi = d->clip_hi; a.N = (size_t)h->n; a.L = d->latent_dim; a.err = h->P.err;
    a.rows_per_wave = sde_rows_per_wave(a.N);
    const dim3 grid((unsigned)((a.N - 1) / (a.rows_per_wave * SDE_WAVES) + 1));
    if (d->in_dtype == PTG_OUT_F64) launch_sde_act<double>(as_stream(stream), grid, a);
    else launch_sde_act<float>(as_stream(stream), grid, a);
    return launch_check(h, "k_sde_act");
}

int64_t ptg_sde_policy_loss_workspace(int64_t batch, int32_t latent_dim)
{
    if (batch < 1 || batch > (int64_t)1 << 31 || !sde_width_ok(latent_dim)) return PTG_E_INVALID;
    const int64_t nmb = loss_blocks(batch, PL_BLOCK), nblk = sde_loss_blocks(batch);
    return (4 + nmb * 3 + latent_dim + nblk * latent_dim) * (int64_t)sizeof(double) + loss_partials_bytes(nblk);
}

int ptg_sde_policy_loss(ptg_env* h, const ptg_sde_loss* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!d) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: null descriptor");
    if (d->kind != PTG_LOSS_PPO && d->kind != PTG_LOSS_A2C) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: unknown kind %d", d->kind);
    if (d->flags & ~(PTG_LOSS_NORM_ADV | PTG_LOSS_CLIP_VF)) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: unknown flag in %d", d->flags);
    const bool ppo = d->kind == PTG_LOSS_PPO, clipv = (d->flags & PTG_LOSS_CLIP_VF) != 0;
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: batch %lld outside [1, 2^31]", (long long)d->batch);
    if (!sde_dtype_ok(d->in_dtype)) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: in_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!sde_width_ok(d->latent_dim)) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: latent_dim %d outside [1, %d]", d->latent_dim, PTG_MLP_MAX_WIDTH);
    if (!d->mean_dev || !d->val_dev || !d->latent_dev || !d->log_std_dev || !d->act_dev || !d->adv_dev || !d->ret_dev)
        return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: null means, values, latent, log_std, actions, advantages or returns");
    if (ppo && !d->old_logp_dev) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: PPO needs old_logp_dev");
    if (!d->stats_dev || !d->grad_in_dev || !d->grad_val_dev || !d->grad_log_std_dev) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: null stats_dev, grad_in_dev, grad_val_dev or grad_log_std_dev");
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: ws_dev is null or not aligned to 8 bytes");
    if (clipv && !d->old_val_dev) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: PTG_LOSS_CLIP_VF needs old_val_dev");
    if (d->mean_s_n < 1 || d->g_s_n < 1 || d->val_s_n < 1 || d->gv_s_n < 1) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: mean_s_n, g_s_n, val_s_n or gv_s_n < 1");
    if (d->latent_s_n < d->latent_dim) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: latent_s_n < latent_dim");
    if (d->grad_latent_dev && d->gl_s_n < d->latent_dim) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: gl_s_n < latent_dim");
    if (ppo && !(d->clip_range >= 0.0)) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: clip_range is negative or NaN");
    if (clipv && !(d->clip_range_vf >= 0.0)) return set_err(h, PTG_E_INVALID, "ptg_sde_policy_loss: clip_range_vf is negative or NaN");
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    SdeLossArgs a{};
    LossArgs& l = a.l;
    l.in = d->mean_dev; l.s_n = (size_t)d->mean_s_n; l.val = d->val_dev; l.v_s = (size_t)d->val_s_n;
    l.act = d->act_dev; l.old_lp = d->old_logp_dev; l.adv = d->adv_dev; l.ret = d->ret_dev; l.old_val = d->old_val_dev; l.log_std = d->log_std_dev;
    l.g_in = d->grad_in_dev; l.g_s = (size_t)d->g_s_n; l.g_val = d->grad_val_dev; l.gv_s = (size_t)d->gv_s_n; l.g_ls = d->grad_log_std_dev;
    l.stats = d->stats_dev; l.ws = (double*)d->ws_dev;
    l.eps = d->clip_range; l.eps_v = d->clip_range_vf; l.ent_coef = d->ent_coef; l.vf_coef = d->vf_coef;
    l.B = (size_t)d->batch; l.kind = d->kind; l.head = PTG_HEAD_GAUSSIAN; l.flags = d->flags;
    l.nblk = (int)loss_blocks(d->batch, PL_BLOCK);
    l.err = h->P.err;
    a.lat = d->latent_dev; a.lat_s = (size_t)d->latent_s_n; a.g_lat = d->grad_latent_dev; a.gl_s = (size_t)d->gl_s_n;
    a.L = d->latent_dim; a.nblk = (int)sde_loss_blocks(d->batch); a.rows_per_wave = sde_rows_per_wave(l.B);
    double* const s2 = sde_s2(l);
    a.s2 = s2; a.row_part = s2 + a.L; a.col_part = a.row_part + (size_t)a.nblk * PL_PITCH;
    const bool f64 = d->in_dtype == PTG_OUT_F64, norm = (d->flags & PTG_LOSS_NORM_ADV) != 0 && d->batch > 1;
    const dim3 block(SDE_BLOCK), cols((unsigned)((a.L - 1) / SDE_BLOCK + 1));
    if (f64) hipLaunchKernelGGL(k_sde_s2<double>, cols, block, 0, st, d->log_std_dev, a.L, s2);
    else hipLaunchKernelGGL(k_sde_s2<float>, cols, block, 0, st, d->log_std_dev, a.L, s2);
    if (norm) {
        const dim3 grid((unsigned)l.nblk);
        if (f64) hipLaunchKernelGGL(k_pl_moments<double>, grid, dim3(PL_BLOCK), 0, st, l);
        else hipLaunchKernelGGL(k_pl_moments<float>, grid, dim3(PL_BLOCK), 0, st, l);
        hipLaunchKernelGGL(k_vn_merge, dim3(1), dim3(64), 0, st, (const double*)(l.ws + 4), l.nblk, l.ws);
    }
    if (f64) launch_sde_loss<double>(st, a, d->grad_log_std_dev);
    else launch_sde_loss<float>(st, a, d->grad_log_std_dev);
    return launch_check(h, "k_sde_rows");
}

// ---- gSDE for SAC / TQC: the training matrix, the squashed head's reparametrised sample, its backward ------------------------------
int ptg_sde_resample_rows(ptg_env* h, const ptg_sde_noise* d, int64_t rows, void* stream)
{
    if (!h) return PTG_E_INVALID;
    return sde_resample(h, "ptg_sde_resample_rows", d, 0, rows, stream);                 // a row is a batch row: no env offset
}

// what ptg_sde_rsample and ptg_sde_rsample_backward refuse alike, then each its own; the text of the first fault, or null
static const char* sde_rs_error(const ptg_sde_rs* d, bool backward)
{
    if (!d) return "null descriptor";
    if (d->flags & ~(PTG_SDE_RS_DETERMINISTIC | PTG_SDE_RS_SHARED_E)) return "unknown flag";
    const bool det = (d->flags & PTG_SDE_RS_DETERMINISTIC) != 0, shared = (d->flags & PTG_SDE_RS_SHARED_E) != 0;
    if (!sde_dtype_ok(d->in_dtype)) return "in_dtype must be PTG_OUT_F32 or PTG_OUT_F64";
    if (!sde_width_ok(d->latent_dim)) return "latent_dim outside [1, 1024]";
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return "batch outside [1, 2^31]";
    if (!d->mean_dev || !d->latent_dev || !d->log_std_dev) return "null mean_dev, latent_dev or log_std_dev";
    if (!det && !d->e_dev) return "a stochastic call needs e_dev";
    if (d->mean_s_n < 1) return "mean_s_n < 1";
    if (d->latent_s_n < d->latent_dim) return "latent_s_n < latent_dim";
    if (!det && !shared && d->e_s_n < d->latent_dim) return "e_s_n < latent_dim";
    if (!(d->clip_mean > 0.0)) return "clip_mean is <= 0 or NaN";
    if ((uintptr_t)d->saved_dev % sizeof(double) != 0) return "saved_dev is not aligned to 8 bytes";
    if (!backward) return d->act_dev ? nullptr : "null act_dev";
    if (!d->saved_dev || !d->grad_mean_dev) return "null saved_dev or grad_mean_dev";
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return "ws_dev is null or not aligned to 8 bytes";
    if (!d->grad_act_dev && !d->grad_logp_dev) return "grad_act_dev and grad_logp_dev are both null";
    if (d->gm_s_n < 1) return "gm_s_n < 1";
    if (d->grad_latent_dev && d->gl_s_n < d->latent_dim) return "gl_s_n < latent_dim";
    if (d->grad_log_std_dev && !shared) return "grad_log_std_dev without PTG_SDE_RS_SHARED_E";
    return nullptr;
}

static void sde_rs_args(ptg_env* h, const ptg_sde_rs* d, SdeRsArgs& a)
{
    const bool det = (d->flags & PTG_SDE_RS_DETERMINISTIC) != 0;
    a.mean = d->mean_dev; a.m_s = (size_t)d->mean_s_n; a.lat = d->latent_dev; a.lat_s = (size_t)d->latent_s_n;
    a.E = det ? nullptr : d->e_dev; a.shared = !det && (d->flags & PTG_SDE_RS_SHARED_E) != 0; a.e_s = (det || a.shared) ? 0 : (size_t)d->e_s_n;
    a.log_std = d->log_std_dev; a.act = d->act_dev; a.logp = d->logp_dev; a.step_act = d->step_act_dev; a.saved = d->saved_dev;
    a.g_act = d->grad_act_dev; a.g_logp = d->grad_logp_dev; a.g_mean = d->grad_mean_dev; a.gm_s = (size_t)d->gm_s_n;
    a.g_lat = d->grad_latent_dev; a.gl_s = (size_t)d->gl_s_n;
    a.c = d->clip_mean; a.B = (size_t)d->batch; a.rows_per_wave = sde_rows_per_wave(a.B); a.L = d->latent_dim;
    a.nblk = (int)sde_loss_blocks(d->batch); a.err = h->P.err;
}

int ptg_sde_rsample(ptg_env* h, const ptg_sde_rs* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (const char* why = sde_rs_error(d, false)) return set_err(h, PTG_E_INVALID, "ptg_sde_rsample: %s", why);
    HIP_TRY(h, hipSetDevice(h->device));
    SdeRsArgs a{};
    sde_rs_args(h, d, a);
    if (d->in_dtype == PTG_OUT_F64) launch_sde_rs<double>(as_stream(stream), a, false);
    else launch_sde_rs<float>(as_stream(stream), a, false);
    return launch_check(h, "k_sde_rs_fwd");
}

int64_t ptg_sde_rsample_backward_workspace(int64_t batch, int32_t latent_dim)
{
    if (batch < 1 || batch > (int64_t)1 << 31 || !sde_width_ok(latent_dim)) return PTG_E_INVALID;
    return (int64_t)latent_dim * (1 + sde_loss_blocks(batch)) * (int64_t)sizeof(double);
}

int ptg_sde_rsample_backward(ptg_env* h, const ptg_sde_rs* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (const char* why = sde_rs_error(d, true)) return set_err(h, PTG_E_INVALID, "ptg_sde_rsample_backward: %s", why);
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    SdeRsArgs a{};
    sde_rs_args(h, d, a);
    double* const s2 = (double*)d->ws_dev;
    a.s2 = s2; a.col_part = d->grad_log_std_dev ? s2 + a.L : nullptr;
    const bool f64 = d->in_dtype == PTG_OUT_F64;
    const dim3 block(SDE_BLOCK), cols((unsigned)((a.L - 1) / SDE_BLOCK + 1));
    if (f64) hipLaunchKernelGGL(k_sde_s2<double>, cols, block, 0, st, d->log_std_dev, a.L, s2);
    else hipLaunchKernelGGL(k_sde_s2<float>, cols, block, 0, st, d->log_std_dev, a.L, s2);
    if (f64) launch_sde_rs<double>(st, a, true);
    else launch_sde_rs<float>(st, a, true);
    if (a.col_part) {
        if (f64) hipLaunchKernelGGL(k_sde_rs_cols<double>, cols, block, 0, st, (const double*)a.col_part, a.nblk, a.L, d->grad_log_std_dev);
        else hipLaunchKernelGGL(k_sde_rs_cols<float>, cols, block, 0, st, (const double*)a.col_part, a.nblk, a.L, d->grad_log_std_dev);
    }
    return launch_check(h, "k_sde_rs_bwd");
}

// ---- the optimiser step: grad-norm clip, Adam / RMSprop, Polyak and zero_grad for all tensors of an optimiser -----------
int ptg_optim_chunk(void) { return OPT_CHUNK; }

int64_t ptg_optim_workspace(int64_t n_chunks)
{
    if (n_chunks < 1 || n_chunks > 0x7FFFFFFF) return PTG_E_INVALID;      // one workgroup per chunk: the grid's x dimension
    return (OPT_WS_HEAD + n_chunks) * (int64_t)sizeof(double);
}

// THE optimiser step: ptg_optim_step is this walk over one descriptor with the single kernels, ptg_optim_step_group the same walk with
// the grouped ones on a grid of (the largest chunk count, members)
static int optim_step_walk(ptg_env* h, const char* who, const ptg_optim* members, int n_members, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = train_refuse(h, who, members, n_members, grouped, optim_desc_fault,
                              [&](char* why, size_t cap) { return optim_group_fault(members, n_members, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_optim* d = &members[0];    // kind, flags and dtype: the group's
    const bool polyak = d->kind == PTG_OPTIM_POLYAK, clip = (d->flags & PTG_OPTIM_CLIP) != 0, f64 = d->dtype == PTG_OUT_F64;
    TrainGroup<OptArgs> g{};
    unsigned most = 1;
    for (int i = 0; i < n_members; i++) {
        g.m[i] = optim_args(h, &members[i]);
        most = std::max(most, g.m[i].n_chunks);
    }
    const OptArgs& a = g.m[0];
    const dim3 block(OPT_BLOCK);
    if (!grouped) {
        const dim3 grid(a.n_chunks);
        if (!polyak) {
            if (clip) {
                if (f64) hipLaunchKernelGGL(k_optim_norm<double>, grid, block, 0, st, a);
                else hipLaunchKernelGGL(k_optim_norm<float>, grid, block, 0, st, a);
            }
            hipLaunchKernelGGL(k_optim_head<>, dim3(1), block, 0, st, a);
        }
        if (f64) hipLaunchKernelGGL(k_optim_update<double>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_optim_update<float>, grid, block, 0, st, a);
        return launch_check(h, "k_optim_update");
    }
    const dim3 grid(most, (unsigned)n_members);
    if (!polyak) {
        if (clip) {
            if (f64) hipLaunchKernelGGL((k_optim_norm<double, TrainGroup<OptArgs>>), grid, block, 0, st, g);
            else hipLaunchKernelGGL((k_optim_norm<float, TrainGroup<OptArgs>>), grid, block, 0, st, g);
        }
        hipLaunchKernelGGL(k_optim_head<TrainGroup<OptArgs>>, dim3((unsigned)n_members), block, 0, st, g);
    }
    if (f64) hipLaunchKernelGGL((k_optim_update<double, TrainGroup<OptArgs>>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_optim_update<float, TrainGroup<OptArgs>>), grid, block, 0, st, g);
    return launch_check(h, "k_optim_update (grouped)");
}

int ptg_optim_step(ptg_env* h, const ptg_optim* d, void* stream) { return optim_step_walk(h, "ptg_optim_step", d, 1, false, stream); }

int ptg_optim_step_group(ptg_env* h, const ptg_optim* members, int32_t n_members, void* stream)
{
    return optim_step_walk(h, "ptg_optim_step_group", members, n_members, true, stream);
}

// ---- the TD losses: DQN's and the TD3 / SAC critics', the statistics and the gradients w.r.t. the current Q-values ---------
int64_t ptg_td_loss_workspace(int64_t batch) { return loss_workspace(batch, PL_BLOCK); }

// THE TD loss: ptg_td_loss is this walk over one descriptor with the single kernels, ptg_td_loss_group the same walk with the grouped
// ones.  `grouped` is the entry that was called, not n_members > 1: a group of one launches the grouped kernels
static int td_loss_walk(ptg_env* h, const char* who, const ptg_td* members, int n_members, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = train_refuse(h, who, members, n_members, grouped, td_desc_fault,
                              [&](char* why, size_t cap) { return td_group_fault(members, n_members, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_td* d = &members[0];       // kind, dtype and batch: the group's
    TrainGroup<TdArgs> g{};
    for (int i = 0; i < n_members; i++) g.m[i] = td_args(h, &members[i]);
    const TdArgs& a = g.m[0];
    const bool f64 = d->q_dtype == PTG_OUT_F64, dqn = d->kind == PTG_TD_DQN;      // the Q dtype and the kind are the row kernel's template axes
    if (!grouped) {
        if (f64 && dqn) launch_loss<TdFinal>(st, a, a.ws, k_td_rows<double, true, true>, k_td_rows<double, true, false>);
        else if (f64) launch_loss<TdFinal>(st, a, a.ws, k_td_rows<double, false, true>, k_td_rows<double, false, false>);
        else if (dqn) launch_loss<TdFinal>(st, a, a.ws, k_td_rows<float, true, true>, k_td_rows<float, true, false>);
        else launch_loss<TdFinal>(st, a, a.ws, k_td_rows<float, false, true>, k_td_rows<float, false, false>);
        return launch_check(h, "k_td_rows");
    }
    using G = TrainGroup<TdArgs>;
    if (f64 && dqn) launch_loss_group<TdFinal>(st, g, n_members, k_td_rows<double, true, true, G>, k_td_rows<double, true, false, G>);
    else if (f64) launch_loss_group<TdFinal>(st, g, n_members, k_td_rows<double, false, true, G>, k_td_rows<double, false, false, G>);
    else if (dqn) launch_loss_group<TdFinal>(st, g, n_members, k_td_rows<float, true, true, G>, k_td_rows<float, true, false, G>);
    else launch_loss_group<TdFinal>(st, g, n_members, k_td_rows<float, false, true, G>, k_td_rows<float, false, false, G>);
    return launch_check(h, "k_td_rows (grouped)");
}

int ptg_td_loss(ptg_env* h, const ptg_td* d, void* stream) { return td_loss_walk(h, "ptg_td_loss", d, 1, false, stream); }

int ptg_td_loss_group(ptg_env* h, const ptg_td* members, int32_t n_members, void* stream)
{
    return td_loss_walk(h, "ptg_td_loss_group", members, n_members, true, stream);
}

// ---- the quantile-Huber loss of TQC's critics, the statistics and the gradients w.r.t. the current quantiles -------------------------
int64_t ptg_quantile_loss_workspace(int64_t batch) { return loss_workspace(batch, PL_WAVES); }

int ptg_quantile_loss(ptg_env* h, const ptg_ql* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!d) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: null descriptor");
    if (d->flags & ~PTG_QL_LOG_ALPHA) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: unknown flag in %d", d->flags);
    const auto dtype_ok = [](int c) { return c == PTG_OUT_F32 || c == PTG_OUT_F64; };
    if (ptg_quantile_loss_workspace(d->batch) < 0) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: batch %lld outside [1, 2^31]", (long long)d->batch);
    if (!dtype_ok(d->q_dtype) || !dtype_ok(d->rew_dtype) || !dtype_ok(d->done_dtype))
        return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: q_dtype, rew_dtype and done_dtype must be PTG_OUT_F32 or PTG_OUT_F64");
    if (!d->rew_dev || !d->done_dev || !d->next_logp_dev || !d->stats_dev)
        return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: null rew_dev, done_dev, next_logp_dev or stats_dev");
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(double) != 0) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: ws_dev is null or not aligned to 8 bytes");
    if ((d->flags & PTG_QL_LOG_ALPHA) && !d->alpha_dev) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: PTG_QL_LOG_ALPHA needs alpha_dev");
    if (d->n_critics < 1 || d->n_critics > PTG_TD_MAX_CRITICS) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: n_critics outside [1, %d]", PTG_TD_MAX_CRITICS);
    if (d->n_quantiles < 1 || d->n_quantiles > PTG_QL_MAX_QUANTILES)
        return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: n_quantiles outside [1, %d]", PTG_QL_MAX_QUANTILES);
    if (d->n_drop < 0 || d->n_drop >= d->n_quantiles) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: n_drop outside [0, n_quantiles)");
    const int K = d->n_critics, Q = d->n_quantiles;
    for (int k = 0; k < K; k++) {
        if (!d->cur_dev[k] || !d->next_dev[k] || !d->grad_dev[k]) return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: null cur_dev, next_dev or grad_dev [%d]", k);
        if (d->cur_s_n[k] < Q || d->next_s_n[k] < Q || d->g_s_n[k] < Q)
            return set_err(h, PTG_E_INVALID, "ptg_quantile_loss: cur_s_n, next_s_n or g_s_n [%d] below %d", k, Q);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    QlArgs a{};
    for (int k = 0; k < K; k++) {
        a.cur[k] = d->cur_dev[k]; a.cur_s[k] = (size_t)d->cur_s_n[k];
        a.nq[k] = d->next_dev[k]; a.nq_s[k] = (size_t)d->next_s_n[k];
        a.g[k] = d->grad_dev[k]; a.g_s[k] = (size_t)d->g_s_n[k];
    }
    a.rew = d->rew_dev; a.done = d->done_dev; a.lp = d->next_logp_dev; a.alpha_dev = d->alpha_dev;
    a.y = d->y_dev; a.stats = d->stats_dev; a.ws = (double*)d->ws_dev;
    a.gamma = d->gamma; a.alpha = d->alpha;
    a.B = (size_t)d->batch; a.K = K; a.Q = Q; a.M = K * (Q - d->n_drop); a.KQ = K * Q; a.flags = d->flags;
    a.rew_f64 = d->rew_dtype == PTG_OUT_F64; a.done_f64 = d->done_dtype == PTG_OUT_F64;
    a.nblk = (int)loss_blocks(d->batch, PL_WAVES);
    a.err = h->P.err;
    if (d->q_dtype == PTG_OUT_F64) launch_loss<QlFinal>(st, a, a.ws, k_ql_rows<double, true>, k_ql_rows<double, false>);
    else launch_loss<QlFinal>(st, a, a.ws, k_ql_rows<float, true>, k_ql_rows<float, false>);
    return launch_check(h, "k_ql_rows");
}

// ---- the training-time actor head: reparametrised squashed-Gaussian sample with its log-prob, its backward, TD3's smoothed target action ----
static RsArgs rs_args(ptg_env* h, const ptg_rs* d)
{
    RsArgs a{};
    a.mean = d->mean_dev; a.m_s = (size_t)d->mean_s_n; a.ls = d->log_std_dev; a.ls_s = (size_t)d->log_std_s_n;
    a.act = d->act_dev; a.logp = d->logp_dev; a.noise = d->noise_dev;
    a.g_act = d->grad_act_dev; a.g_logp = d->grad_logp_dev;
    a.g_mean = d->grad_mean_dev; a.gm_s = (size_t)d->gm_s_n; a.g_ls = d->grad_log_std_dev; a.gl_s = (size_t)d->gl_s_n;
    a.counter = (d->flags & PTG_RS_DETERMINISTIC) ? nullptr : (const unsigned long long*)d->counter_dev; a.seed = (unsigned long long)d->seed;
    a.sigma_t = d->noise_std; a.c = d->noise_clip; a.lo = d->clip_lo; a.hi = d->clip_hi;
    a.B = (size_t)d->batch; a.kind = d->kind; a.err = h->P.err;
    return a;
}

// THE actor head: ptg_rsample and ptg_rsample_backward are this walk over one descriptor with the single kernels, their grouped entries
// the same walk with the grouped ones on a grid of (blocks of the batch, members).  `grouped` is the entry that was called
static int rsample_walk(ptg_env* h, const char* who, const ptg_rs* members, int n_members, bool grouped, bool backward, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = train_refuse(h, who, members, n_members, grouped,
                              [&](const ptg_rs* d, char* why, size_t cap) { const char* e = rs_desc_error(d, backward); return e ? train_fault(why, cap, "%s", e) : false; },
                              [&](char* why, size_t cap) { return rs_group_fault(members, n_members, backward, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_rs* d = &members[0];       // dtype, flags and batch: the group's
    TrainGroup<RsArgs> g{};
    for (int i = 0; i < n_members; i++) g.m[i] = rs_args(h, &members[i]);
    const RsArgs& a = g.m[0];
    const bool f64 = d->q_dtype == PTG_OUT_F64;
    const unsigned nblk = (unsigned)((a.B + ACT_BLOCK - 1) / ACT_BLOCK);
    const dim3 block(ACT_BLOCK);
    if (!grouped) {
        const dim3 grid(nblk);
        if (backward) {
            if (f64) hipLaunchKernelGGL(k_rs_bwd<double>, grid, block, 0, st, a);
            else hipLaunchKernelGGL(k_rs_bwd<float>, grid, block, 0, st, a);
            return launch_check(h, "k_rs_bwd");
        }
        if (f64) hipLaunchKernelGGL(k_rs_fwd<double>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_rs_fwd<float>, grid, block, 0, st, a);
        if (a.counter) hipLaunchKernelGGL(k_rb_bump, dim3(1), dim3(1), 0, st, (unsigned long long*)d->counter_dev, 1ull);
        return launch_check(h, "k_rs_fwd");
    }
    const dim3 grid(nblk, (unsigned)n_members);
    if (backward) {
        if (f64) hipLaunchKernelGGL((k_rs_bwd<double, TrainGroup<RsArgs>>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((k_rs_bwd<float, TrainGroup<RsArgs>>), grid, block, 0, st, g);
        return launch_check(h, "k_rs_bwd (grouped)");
    }
    if (f64) hipLaunchKernelGGL((k_rs_fwd<double, TrainGroup<RsArgs>>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_rs_fwd<float, TrainGroup<RsArgs>>), grid, block, 0, st, g);
    if (a.counter) hipLaunchKernelGGL(k_rs_bump_group, dim3((unsigned)n_members), dim3(1), 0, st, g);      // the flags agree: every member has its counter
    return launch_check(h, "k_rs_fwd (grouped)");
}

int ptg_rsample(ptg_env* h, const ptg_rs* d, void* stream) { return rsample_walk(h, "ptg_rsample", d, 1, false, false, stream); }

int ptg_rsample_backward(ptg_env* h, const ptg_rs* d, void* stream) { return rsample_walk(h, "ptg_rsample_backward", d, 1, false, true, stream); }

int ptg_rsample_group(ptg_env* h, const ptg_rs* members, int32_t n_members, void* stream)
{
    return rsample_walk(h, "ptg_rsample_group", members, n_members, true, false, stream);
}

int ptg_rsample_backward_group(ptg_env* h, const ptg_rs* members, int32_t n_members, void* stream)
{
    return rsample_walk(h, "ptg_rsample_backward_group", members, n_members, true, true, stream);
}

// ---- the actor and entropy-coefficient losses of SAC / TQC / TD3, the statistics and the gradients -----------------------------------
int64_t ptg_actor_loss_workspace(int64_t batch) { return loss_workspace(batch, PL_BLOCK); }

// THE actor loss: ptg_actor_loss is this walk over one descriptor with the single kernels, ptg_actor_loss_group the same walk with the
// grouped ones.  `grouped` is the entry that was called
static int actor_loss_walk(ptg_env* h, const char* who, const ptg_al* members, int n_members, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = train_refuse(h, who, members, n_members, grouped, al_desc_fault,
                              [&](char* why, size_t cap) { return al_group_fault(members, n_members, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    TrainGroup<AlArgs> g{};
    for (int i = 0; i < n_members; i++) g.m[i] = al_args(h, &members[i]);
    const AlArgs& a = g.m[0];
    const bool f64 = members[0].q_dtype == PTG_OUT_F64;      // the group's
    if (!grouped) {
        if (f64) launch_loss<AlFinal>(st, a, a.ws, k_al_rows<double, true>, k_al_rows<double, false>);
        else launch_loss<AlFinal>(st, a, a.ws, k_al_rows<float, true>, k_al_rows<float, false>);
        return launch_check(h, "k_al_rows");
    }
    using G = TrainGroup<AlArgs>;
    if (f64) launch_loss_group<AlFinal>(st, g, n_members, k_al_rows<double, true, G>, k_al_rows<double, false, G>);
    else launch_loss_group<AlFinal>(st, g, n_members, k_al_rows<float, true, G>, k_al_rows<float, false, G>);
    return launch_check(h, "k_al_rows (grouped)");
}

int ptg_actor_loss(ptg_env* h, const ptg_al* d, void* stream) { return actor_loss_walk(h, "ptg_actor_loss", d, 1, false, stream); }

int ptg_actor_loss_group(ptg_env* h, const ptg_al* members, int32_t n_members, void* stream)
{
    return actor_loss_walk(h, "ptg_actor_loss_group", members, n_members, true, stream);
}

}  // extern "C"
