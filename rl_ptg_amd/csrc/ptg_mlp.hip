// ptg_mlp.hip -- the inference forward of an MLP (include/ptg_env.h, ptg_mlp_forward, states the arithmetic; tests/mlp_restatement.py
// restates it).  One launch per layer: Linear + bias + activation fused, on gfx950's exact-float32 MFMA (v_mfma_f32_16x16x4_f32 and
// v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product).  The translation unit shares ptg_handle.h with ptg_env.hip
// and ptg_train.hip and reads nothing of the handle but its device.
//
// D = A * B + C with A = the rows of the input (A[i][k] = x[row0 + i][k]), B = the weights transposed (B[k][j] = W[col0 + j][k]) and
// C = the bias broadcast down its column.  Lane maps (one f32 VGPR per operand per lane):
//   16x16x4   lane l: A[l & 15][l >> 4], B[l >> 4][l & 15];   C/D register g: row 4 * (l >> 4) + g, column l & 15
//   32x32x2   lane l: A[l & 31][l >> 5], B[l >> 5][l & 31];   C/D register g: row (g & 3) + 8 * (g >> 2) + 4 * (l >> 5), column l & 31
// The output column is on the lane in both, so the bias of a lane's unit initialises all of its accumulator registers, and for a fixed
// register 16 (32) neighbouring lanes store neighbouring units of one row.
//
// Two routes, the same bits by construction (the order rule forbids split-K, so a small batch can only be spread over the units):
//   NARROW   one wave per workgroup, a 16-row x 16-unit tile on 16x16x4, K in chunks of 32 staged in LDS; ceil(B / 16) * ceil(O / 16)
//            workgroups, so a 808 x 808 weight matrix is read by 51 workgroups already at B = 6
//   WIDE     four waves per workgroup, a 128 x 128 tile on 32x32x2, each wave 2 x 2 tiles of 32 x 32 (four independent accumulators),
//            K in chunks of 32 staged in LDS
// Both keep a ring of chunks in flight in registers (four NARROW, two WIDE) while the matrix cores work on the current one: at the
// reference's batch sizes a layer is a dependent chain of K / 4 MFMAs.  Loads are single dwords: odd widths (743, 233) leave weight
// rows off 16-byte alignment and the two-piece input splits a row anywhere; a load instruction of a wave still reads 32 neighbouring
// floats of each of two rows.
#include "ptg_handle.h"

#include <cmath>
#include <cstdint>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MLP_NARROW = 0, MLP_WIDE = 1;
constexpr int NR_TILE = 16, NR_KC = 32, NR_PITCH = NR_KC + 4;       // LDS word of (row r, k): 36 r + k; 36 r (mod 64) are 16 multiples of 4, + k & 3: the 64 lanes of a read hit 64 banks
constexpr int WD_TILE = 128, WD_KC = 32, WD_PITCH = WD_KC + 1;      // 33 r + k: the 32 rows of a fragment read fall on distinct banks
constexpr int NR_DEPTH = 4, WD_DEPTH = 2;                           // chunks in flight per workgroup: 4 x 16 and 2 x 32 prefetch registers per lane
// the host's switch: a layer takes WIDE for B >= 16 384 and O > 256, and already for B >= 4 096 when O > 512
constexpr int64_t MLP_WIDE_MIN_ROWS = 16384, MLP_WIDE_MIN_ROWS_BROAD = 4096;
constexpr int MLP_WIDE_MIN_UNITS = 256, MLP_BROAD_UNITS = 512;

struct MlpLayer {                        // by value in the launch: a captured call holds no host memory
    const float* x; size_t x_s;          // the input's first piece [B][F1]
    const float* x2; size_t x2_s;        // its second piece [B][K - F1]; with one piece F1 = K and x2 = x, never selected
    const float* w; size_t w_s;          // [O][K]
    const float* bias;                   // [O]
    float* y; size_t y_s;                // [B][O]
    size_t B;
    int F1, K, O;
};

// Branch-free loads: the index of a lane beyond an edge is clamped into the tensor, the element is read and discarded for 0.  A
// predicated load is a branch per element here, and at the reference's batch sizes those branches, not the MFMA chain, were the time.
__device__ __forceinline__ float mlp_x(const MlpLayer& a, size_t row, int k, bool inside)
{
    const size_t rc = min(row, a.B - 1);
    const int kc = min(k, a.K - 1);
    const float* p = kc < a.F1 ? a.x + (rc * a.x_s + (size_t)kc) : a.x2 + (rc * a.x2_s + (size_t)(kc - a.F1));
    const float v = *p;
    return inside ? v : 0.0f;
}

__device__ __forceinline__ float mlp_w(const MlpLayer& a, int u, int k, bool inside)
{
    const float v = a.w[(size_t)min(u, a.O - 1) * a.w_s + (size_t)min(k, a.K - 1)];
    return inside ? v : 0.0f;
}

template <int ACT>
__device__ __forceinline__ float mlp_act(float v)
{
    if constexpr (ACT == PTG_MLP_RELU) return v > 0.0f ? v : (v != v ? v : 0.0f);
    else if constexpr (ACT == PTG_MLP_TANH) return (float)tanh((double)v);
    else return v;
}

template <int ACT, int ROUTE>
__global__ __launch_bounds__(ROUTE == MLP_NARROW ? 64 : 256) void k_mlp_layer(const MlpLayer a)
{
    if constexpr (ROUTE == MLP_NARROW) {
        __shared__ float xs[NR_TILE * NR_PITCH], ws[NR_TILE * NR_PITCH];
        const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
        const size_t row0 = (size_t)blockIdx.x * NR_TILE;
        const int col0 = blockIdx.y * NR_TILE;
        const float bj = col0 + r < a.O ? a.bias[col0 + r] : 0.0f;
        f32x4 acc = {bj, bj, bj, bj};
        constexpr int PER = NR_TILE * NR_KC / 64;            // 8 rows and 8 units per lane and chunk
        float xr[NR_DEPTH][PER], wr[NR_DEPTH][PER];          // a ring of NR_DEPTH chunks in flight: the slot index is static once unrolled
        const int kx = lane & 31, r2 = lane >> 5;
        auto fetch = [&](int d, int k0) {                    // lane: k = k0 + kx of every second row and unit; 0 beyond an edge
            const int k = k0 + kx;
            const bool kin = k < a.K;
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int rr = r2 + 2 * i;
                const size_t row = row0 + rr;
                const int u = col0 + rr;
                xr[d][i] = mlp_x(a, row, k, kin && row < a.B);
                wr[d][i] = mlp_w(a, u, k, kin && u < a.O);
            }
        };
#pragma unroll
        for (int d = 0; d < NR_DEPTH; d++)
            if (d * NR_KC < a.K) fetch(d, d * NR_KC);
        for (int k0 = 0; k0 < a.K; k0 += NR_DEPTH * NR_KC) {
#pragma unroll
            for (int d = 0; d < NR_DEPTH; d++) {
                const int kc = k0 + d * NR_KC;
                if (kc >= a.K) break;                        // uniform over the workgroup
#pragma unroll
                for (int i = 0; i < PER; i++) {
                    xs[(r2 + 2 * i) * NR_PITCH + kx] = xr[d][i];
                    ws[(r2 + 2 * i) * NR_PITCH + kx] = wr[d][i];
                }
                __syncthreads();
                if (kc + NR_DEPTH * NR_KC < a.K) fetch(d, kc + NR_DEPTH * NR_KC);
                float av[NR_KC / 4], bv[NR_KC / 4];          // all operands of the chunk out of LDS first, then the MFMAs back to back: the
#pragma unroll                                               // chain is the layer's latency at small B.  A ragged last chunk runs its padded
                for (int s = 0; s < NR_KC / 4; s++) {        // steps too: both operands are 0 there, which is exact
                    av[s] = xs[r * NR_PITCH + 4 * s + q];
                    bv[s] = ws[r * NR_PITCH + 4 * s + q];
                }
#pragma unroll
                for (int s = 0; s < NR_KC / 4; s++)          // four ascending k per instruction
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
                __syncthreads();
            }
        }
        const int u = col0 + r;
        if (u < a.O) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const size_t row = row0 + 4 * q + g;
                if (row < a.B) a.y[row * a.y_s + (size_t)u] = mlp_act<ACT>(acc[g]);
            }
        }
    } else {
        __shared__ float xs[WD_TILE * WD_PITCH], ws[WD_TILE * WD_PITCH];
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr_ = wave >> 1, wc = wave & 1, c = lane & 31, hf = lane >> 5;
        const size_t row0 = (size_t)blockIdx.x * WD_TILE;
        const int col0 = blockIdx.y * WD_TILE;
        const bool live = row0 + (size_t)(wr_ * 64) < a.B && col0 + wc * 64 < a.O;      // wave-uniform: a quadrant wholly outside computes nothing
        f32x16 acc[2][2];
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int u = col0 + wc * 64 + n * 32 + c;
            const float bj = u < a.O ? a.bias[u] : 0.0f;
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int g = 0; g < 16; g++) acc[m][n][g] = bj;
        }
        constexpr int PER = WD_TILE * WD_KC / 256;           // 16 rows and 16 units per thread and chunk
        float xr[WD_DEPTH][PER], wr[WD_DEPTH][PER];
        const int kx = t & 31, r8 = t >> 5;
        auto fetch = [&](int d, int k0) {
            const int k = k0 + kx;
            const bool kin = k < a.K;
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int rr = r8 + 8 * i;
                const size_t row = row0 + rr;
                const int u = col0 + rr;
                xr[d][i] = mlp_x(a, row, k, kin && row < a.B);
                wr[d][i] = mlp_w(a, u, k, kin && u < a.O);
            }
        };
#pragma unroll
        for (int d = 0; d < WD_DEPTH; d++)
            if (d * WD_KC < a.K) fetch(d, d * WD_KC);
        for (int k0 = 0; k0 < a.K; k0 += WD_DEPTH * WD_KC) {
#pragma unroll
          for (int d = 0; d < WD_DEPTH; d++) {
            const int kc = k0 + d * WD_KC;
            if (kc >= a.K) break;                            // uniform over the workgroup
#pragma unroll
            for (int i = 0; i < PER; i++) {
                xs[(r8 + 8 * i) * WD_PITCH + kx] = xr[d][i];
                ws[(r8 + 8 * i) * WD_PITCH + kx] = wr[d][i];
            }
            __syncthreads();
            if (kc + WD_DEPTH * WD_KC < a.K) fetch(d, kc + WD_DEPTH * WD_KC);
            if (live) {
#pragma unroll
                for (int s = 0; s < WD_KC / 2; s++) {        // two ascending k per instruction; unrolled, so the LDS reads run ahead of the MFMAs
                    const float a0 = xs[(wr_ * 64 + c) * WD_PITCH + 2 * s + hf], a1 = xs[(wr_ * 64 + 32 + c) * WD_PITCH + 2 * s + hf];
                    const float b0 = ws[(wc * 64 + c) * WD_PITCH + 2 * s + hf], b1 = ws[(wc * 64 + 32 + c) * WD_PITCH + 2 * s + hf];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                }
            }
            __syncthreads();
          }
        }
        if (live) {
#pragma unroll
            for (int n = 0; n < 2; n++) {
                const int u = col0 + wc * 64 + n * 32 + c;
                if (u >= a.O) continue;
#pragma unroll
                for (int m = 0; m < 2; m++)
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        const size_t row = row0 + (size_t)(wr_ * 64 + m * 32 + (g & 3) + 8 * (g >> 2) + 4 * hf);
                        if (row < a.B) a.y[row * a.y_s + (size_t)u] = mlp_act<ACT>(acc[m][n][g]);
                    }
            }
        }
    }
}

template <int ROUTE>
void launch_mlp_layer(hipStream_t st, const MlpLayer& a, int act)
{
    const int tile = ROUTE == MLP_NARROW ? NR_TILE : WD_TILE;
    const dim3 grid((unsigned)((a.B - 1) / tile + 1), (unsigned)((a.O - 1) / tile + 1)), block(ROUTE == MLP_NARROW ? 64 : 256);      // x: up to 2^27 row tiles
    if (act == PTG_MLP_RELU) k_mlp_layer<PTG_MLP_RELU, ROUTE><<<grid, block, 0, st>>>(a);
    else if (act == PTG_MLP_TANH) k_mlp_layer<PTG_MLP_TANH, ROUTE><<<grid, block, 0, st>>>(a);
    else k_mlp_layer<PTG_MLP_NONE, ROUTE><<<grid, block, 0, st>>>(a);
}

inline int64_t mlp_pitch(int w) { return ((int64_t)w + 3) / 4 * 4; }

}  // namespace

extern "C" {

int64_t ptg_mlp_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags)
{
    if (batch < 1 || batch > (int64_t)1 << 31 || n_layers < 1 || n_layers > PTG_MLP_MAX_LAYERS || !widths) return PTG_E_INVALID;
    if (flags & ~(PTG_MLP_KEEP_HIDDEN | PTG_MLP_NARROW | PTG_MLP_WIDE)) return PTG_E_INVALID;
    if ((flags & PTG_MLP_NARROW) && (flags & PTG_MLP_WIDE)) return PTG_E_INVALID;
    int64_t sum = 0, widest = 0;
    for (int l = 0; l < n_layers; l++) {
        if (widths[l] < 1 || widths[l] > PTG_MLP_MAX_WIDTH) return PTG_E_INVALID;
        if (l < n_layers - 1) {
            sum += mlp_pitch(widths[l]);
            widest = std::max(widest, mlp_pitch(widths[l]));
        }
    }
    const int64_t floats = (flags & PTG_MLP_KEEP_HIDDEN) ? batch * sum : 2 * batch * widest;
    return std::max<int64_t>(16, floats * (int64_t)sizeof(float));
}

int ptg_mlp_forward(ptg_env* h, const ptg_mlp* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!d) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: null descriptor");
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: batch %lld outside [1, 2^31]", (long long)d->batch);
    if (d->n_layers < 1 || d->n_layers > PTG_MLP_MAX_LAYERS) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: n_layers %d outside [1, %d]", d->n_layers, PTG_MLP_MAX_LAYERS);
    if (d->flags & ~(PTG_MLP_KEEP_HIDDEN | PTG_MLP_NARROW | PTG_MLP_WIDE)) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: unknown flag in %d", d->flags);
    if ((d->flags & PTG_MLP_NARROW) && (d->flags & PTG_MLP_WIDE)) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: PTG_MLP_NARROW and PTG_MLP_WIDE exclude each other");
    if (d->hidden_act != PTG_MLP_RELU && d->hidden_act != PTG_MLP_TANH) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: hidden_act must be PTG_MLP_RELU or PTG_MLP_TANH");
    if (d->out_act != PTG_MLP_NONE && d->out_act != PTG_MLP_RELU && d->out_act != PTG_MLP_TANH) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: unknown out_act %d", d->out_act);
    if (d->f1 < 1 || d->f2 < 0 || (int64_t)d->f1 + d->f2 > PTG_MLP_MAX_WIDTH)
        return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: f1 = %d, f2 = %d: need f1 >= 1, f2 >= 0, f1 + f2 <= %d", d->f1, d->f2, PTG_MLP_MAX_WIDTH);
    if (!d->x_dev || d->x_s_n < d->f1) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: x_dev is null or x_s_n below f1 = %d", d->f1);
    if ((d->x2_dev != nullptr) != (d->f2 > 0)) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: x2_dev and f2 > 0 go together");
    if (d->x2_dev && d->x2_s_n < d->f2) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: x2_s_n below f2 = %d", d->f2);
    const int n = d->n_layers;
    int fan_in = d->f1 + d->f2;
    for (int l = 0; l < n; l++) {
        if (d->width[l] < 1 || d->width[l] > PTG_MLP_MAX_WIDTH) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: width[%d] = %d outside [1, %d]", l, d->width[l], PTG_MLP_MAX_WIDTH);
        if (!d->w_dev[l] || !d->b_dev[l]) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: null w_dev or b_dev [%d]", l);
        if (d->w_s_n[l] < fan_in) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: w_s_n[%d] below the fan-in %d", l, fan_in);
        fan_in = d->width[l];
    }
    if (!d->out_dev || (uintptr_t)d->out_dev % sizeof(float) != 0) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: out_dev is null or not aligned to 4 bytes");
    if (d->out_s_n < d->width[n - 1]) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: out_s_n below the output width %d", d->width[n - 1]);
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(float) != 0) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: ws_dev is null or not aligned to 4 bytes");
    const int64_t need = ptg_mlp_workspace(d->batch, n, d->width, d->flags);
    if (d->ws_bytes < need) return set_err(h, PTG_E_INVALID, "ptg_mlp_forward: ws_bytes = %lld, the call needs %lld", (long long)d->ws_bytes, (long long)need);
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const bool keep = (d->flags & PTG_MLP_KEEP_HIDDEN) != 0;
    const size_t B = (size_t)d->batch;
    size_t widest = 0;
    for (int l = 0; l < n - 1; l++) widest = std::max(widest, (size_t)mlp_pitch(d->width[l]));
    MlpLayer a{};
    a.B = B;
    a.x = d->x_dev; a.x_s = (size_t)d->x_s_n; a.x2 = d->x2_dev ? d->x2_dev : d->x_dev; a.x2_s = (size_t)d->x2_s_n;
    a.F1 = d->f1; a.K = d->f1 + d->f2;
    size_t kept = 0;                                         // floats of ws_dev before hidden layer l (KEEP_HIDDEN)
    for (int l = 0; l < n; l++) {
        const bool last = l == n - 1;
        a.w = d->w_dev[l]; a.w_s = (size_t)d->w_s_n[l]; a.bias = d->b_dev[l]; a.O = d->width[l];
        if (last) {
            a.y = d->out_dev; a.y_s = (size_t)d->out_s_n;
        } else {
            a.y = (float*)d->ws_dev + (keep ? kept : (size_t)(l & 1) * B * widest);
            a.y_s = (size_t)mlp_pitch(d->width[l]);
        }
        const int act = last ? d->out_act : d->hidden_act;
        const bool wide = (d->flags & PTG_MLP_WIDE) || (!(d->flags & PTG_MLP_NARROW) && ((d->batch >= MLP_WIDE_MIN_ROWS && a.O > MLP_WIDE_MIN_UNITS) || (d->batch >= MLP_WIDE_MIN_ROWS_BROAD && a.O > MLP_BROAD_UNITS)));
        if (wide) launch_mlp_layer<MLP_WIDE>(st, a, act);
        else launch_mlp_layer<MLP_NARROW>(st, a, act);
        if (int rc = launch_check(h, "k_mlp_layer")) return rc;
        kept += B * a.y_s;
        a.x = a.x2 = a.y; a.x_s = a.y_s; a.x2_s = 0; a.F1 = a.K = a.O;      // this layer's output is the next one's input
    }
    return 0;
}

}  // extern "C"
