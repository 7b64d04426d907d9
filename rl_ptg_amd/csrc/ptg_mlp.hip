// ptg_mlp.hip -- the forward of an MLP (include/ptg_env.h, ptg_mlp_forward, states the arithmetic; tests/mlp_restatement.py
// restates it) and, in the second half of the file, its backward pass (ptg_mlp_backward; tests/mlp_backward_restatement.py).
// The forward: one launch per layer: Linear + bias + activation fused, on gfx950's exact-float32 MFMA (v_mfma_f32_16x16x4_f32 and
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

// ---- the backward pass (include/ptg_env.h, ptg_mlp_backward, states the arithmetic) ---------------------------------
// Two kernels per layer on v_mfma_f32_16x16x4_f32, one wave per workgroup, a 16 x 16 tile, the reduction in chunks of 32 through LDS with
// the forward's ring of chunks in flight (four in k_mlp_dx, two in k_mlp_dw).  The lane maps are the forward's; what changes is which tensor
// index rides on which:
//   k_mlp_dx   D[b][k] = sum_j dz[b][j] W[j][k]:  A[l & 15][l >> 4] = dz[row0 + (l & 15)][j0 + (l >> 4)] (staged [row][j], pitch 36, as the
//              forward's input), B[l >> 4][l & 15] = W[j0 + (l >> 4)][col0 + (l & 15)] (staged [j][k], pitch 16: the word of a read is
//              16 (4 s + q) + r, 64 lanes on 64 banks; W's rows are read along k, 16 neighbouring floats of each of four rows per load)
//   k_mlp_dw   D[j][k] = sum_b dz[b][j] x[b][k]:  A[l & 15][l >> 4] = dz[b0 + (l >> 4)][j0 + (l & 15)], B[l >> 4][l & 15] = x[b0 + (l >> 4)][k0 + (l & 15)]:
//              both staged [b][.] with pitch 16, A read transposed out of LDS.  x has one column more than the fan-in, all ones: the
//              tile column K is the bias gradient.  The accumulator starts at 0 or at the gradient already there
// C/D register g of lane l is row 4 (l >> 4) + g, column l & 15 in both, so 16 neighbouring lanes store 16 neighbouring floats of a row.
namespace {

#ifndef PTG_MLP_DW_DEPTH
#define PTG_MLP_DW_DEPTH 2               // an experiment build may set 4: 224 registers instead of 118, two waves per SIMD instead of four
#endif
constexpr int BW_TILE = 16, BW_RC = 32, BW_DEPTH = 4, BW_PITCH_T = 16;      // tile, reduction chunk, chunks in flight in k_mlp_dx, pitch of a [reduction][16] stage
constexpr int DW_DEPTH = PTG_MLP_DW_DEPTH;                                  // chunks in flight in k_mlp_dw

struct MlpDx {                           // by value in the launch
    const float* dz; size_t dz_s;        // [B][O], the gradient at this layer's pre-activation
    const float* w; size_t w_s;          // [O][K]
    const float* h; size_t h_s;          // [B][K] the kept output of the layer below (ACT_BELOW != NONE)
    float* y; size_t y_s;                // ACT_BELOW != NONE: dz of the layer below [B][K];  NONE: dx's first piece [B][F1] or NULL
    float* y2; size_t y2_s;              // NONE: dx's second piece [B][K - F1] or NULL
    size_t B;
    int F1, K, O;
};

struct MlpDw {
    const float* dz; size_t dz_s;        // [B][O]
    const float* x; size_t x_s;          // the layer's input, first piece [B][F1]
    const float* x2; size_t x2_s;        // second piece [B][K - F1]; one piece: F1 = K, x2 = x
    float* dw; size_t dw_s;              // [O][K]
    float* db;                           // [O]
    size_t B;
    int F1, K, O, accumulate;
};

struct MlpDzOut {
    const float* g; size_t g_s;          // grad_out [B][O]
    const float* h; size_t h_s;          // out [B][O]
    float* dz; size_t dz_s;
    size_t B;
    int O;
};

// the activation derivative on the kept output h: RELU a select, TANH three roundings (t = h h, u = 1 - t, g u)
template <int ACT>
__device__ __forceinline__ float mlp_dact(float h, float g)
{
    if constexpr (ACT == PTG_MLP_RELU) return h > 0.0f ? g : (h != h ? g : 0.0f);
    else if constexpr (ACT == PTG_MLP_TANH) return __fmul_rn(g, __fsub_rn(1.0f, __fmul_rn(h, h)));
    else return g;
}

template <int ACT_BELOW>
__global__ __launch_bounds__(64) void k_mlp_dx(const MlpDx a)
{
    __shared__ float zs[BW_TILE * NR_PITCH], wt[BW_RC * BW_PITCH_T];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * BW_TILE;
    const int col0 = blockIdx.y * BW_TILE;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int PER = BW_TILE * BW_RC / 64;                // 8 elements of dz and 8 of W per lane and chunk
    float zr[BW_DEPTH][PER], wr[BW_DEPTH][PER];
    const int jx = lane & 31, r2 = lane >> 5;
    const int kw = col0 + r, kwc = min(kw, a.K - 1);
    auto fetch = [&](int d, int j0) {                        // dz: j = j0 + jx of every second row;  W: column kw of every fourth row j
        const int j = j0 + jx, jc = min(j, a.O - 1);
        const bool jin = j < a.O;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const size_t row = row0 + r2 + 2 * i;
            const float z = a.dz[min(row, a.B - 1) * a.dz_s + (size_t)jc];
            zr[d][i] = jin && row < a.B ? z : 0.0f;
            const int jw = j0 + q + 4 * i;
            const float w = a.w[(size_t)min(jw, a.O - 1) * a.w_s + (size_t)kwc];
            wr[d][i] = jw < a.O && kw < a.K ? w : 0.0f;
        }
    };
#pragma unroll
    for (int d = 0; d < BW_DEPTH; d++)
        if (d * BW_RC < a.O) fetch(d, d * BW_RC);
    for (int j0 = 0; j0 < a.O; j0 += BW_DEPTH * BW_RC) {
#pragma unroll
        for (int d = 0; d < BW_DEPTH; d++) {
            const int jc = j0 + d * BW_RC;
            if (jc >= a.O) break;                            // uniform over the workgroup
#pragma unroll
            for (int i = 0; i < PER; i++) {
                zs[(r2 + 2 * i) * NR_PITCH + jx] = zr[d][i];
                wt[(q + 4 * i) * BW_PITCH_T + r] = wr[d][i];
            }
            __syncthreads();
            if (jc + BW_DEPTH * BW_RC < a.O) fetch(d, jc + BW_DEPTH * BW_RC);
            float av[BW_RC / 4], bv[BW_RC / 4];
#pragma unroll
            for (int s = 0; s < BW_RC / 4; s++) {
                av[s] = zs[r * NR_PITCH + 4 * s + q];
                bv[s] = wt[(4 * s + q) * BW_PITCH_T + r];
            }
#pragma unroll
            for (int s = 0; s < BW_RC / 4; s++)              // four ascending j per instruction
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
            __syncthreads();
        }
    }
    if (kw < a.K) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const size_t row = row0 + 4 * q + g;
            if (row >= a.B) continue;
            if constexpr (ACT_BELOW == PTG_MLP_NONE) {       // the first layer: dx to the caller's pieces, each optional
                if (kw < a.F1) {
                    if (a.y) a.y[row * a.y_s + (size_t)kw] = acc[g];
                } else if (a.y2) a.y2[row * a.y2_s + (size_t)(kw - a.F1)] = acc[g];
            } else {
                a.y[row * a.y_s + (size_t)kw] = mlp_dact<ACT_BELOW>(a.h[row * a.h_s + (size_t)kw], acc[g]);
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_mlp_dw(const MlpDw a)
{
    __shared__ float zs[BW_RC * BW_PITCH_T], xs[BW_RC * BW_PITCH_T];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int j0 = blockIdx.x * BW_TILE, k0 = blockIdx.y * BW_TILE;      // k runs to K inclusive: column K is the bias gradient
    const int ko = k0 + r;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.accumulate && ko <= a.K) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int j = j0 + 4 * q + g;
            if (j < a.O) acc[g] = ko < a.K ? a.dw[(size_t)j * a.dw_s + (size_t)ko] : a.db[j];
        }
    }
    constexpr int PER = BW_TILE * BW_RC / 64;                // 8 rows per lane and chunk
    float zr[DW_DEPTH][PER], xr[DW_DEPTH][PER];
    const int jz = j0 + r, jzc = min(jz, a.O - 1), kc = min(ko, a.K - 1);
    const bool one = ko == a.K;
    const float* xp = kc < a.F1 ? a.x + (size_t)kc : a.x2 + (size_t)(kc - a.F1);
    const size_t xps = kc < a.F1 ? a.x_s : a.x2_s;
    auto fetch = [&](int d, size_t b0) {                     // lane: unit jz and column ko of every fourth row
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const size_t row = b0 + q + 4 * i, rc = min(row, a.B - 1);
            const bool rin = row < a.B;
            const float z = a.dz[rc * a.dz_s + (size_t)jzc];
            zr[d][i] = rin && jz < a.O ? z : 0.0f;
            const float x = xp[rc * xps];
            xr[d][i] = rin && ko <= a.K ? (one ? 1.0f : x) : 0.0f;
        }
    };
#pragma unroll
    for (int d = 0; d < DW_DEPTH; d++)
        if ((size_t)(d * BW_RC) < a.B) fetch(d, (size_t)(d * BW_RC));
    for (size_t b0 = 0; b0 < a.B; b0 += DW_DEPTH * BW_RC) {
#pragma unroll
        for (int d = 0; d < DW_DEPTH; d++) {
            const size_t bc = b0 + d * BW_RC;
            if (bc >= a.B) break;                            // uniform over the workgroup
#pragma unroll
            for (int i = 0; i < PER; i++) {
                zs[(q + 4 * i) * BW_PITCH_T + r] = zr[d][i];
                xs[(q + 4 * i) * BW_PITCH_T + r] = xr[d][i];
            }
            __syncthreads();
            if (bc + DW_DEPTH * BW_RC < a.B) fetch(d, bc + DW_DEPTH * BW_RC);
            float av[BW_RC / 4], bv[BW_RC / 4];
#pragma unroll
            for (int s = 0; s < BW_RC / 4; s++) {            // A transposed out of LDS: row of the stage = reduction index
                av[s] = zs[(4 * s + q) * BW_PITCH_T + r];
                bv[s] = xs[(4 * s + q) * BW_PITCH_T + r];
            }
#pragma unroll
            for (int s = 0; s < BW_RC / 4; s++)              // four ascending b per instruction
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
            __syncthreads();
        }
    }
    if (ko <= a.K) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int j = j0 + 4 * q + g;
            if (j >= a.O) continue;
            if (ko < a.K) a.dw[(size_t)j * a.dw_s + (size_t)ko] = acc[g];
            else a.db[j] = acc[g];
        }
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void k_mlp_dz_out(const MlpDzOut a)
{
    const size_t total = a.B * (size_t)a.O, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const size_t b = i / (size_t)a.O, j = i % (size_t)a.O;
        a.dz[b * a.dz_s + j] = mlp_dact<ACT>(a.h[b * a.h_s + j], a.g[b * a.g_s + j]);
    }
}

// what ptg_mlp_forward refuses in a descriptor, restated for the embedded one: NULL when it is well-formed
const char* mlp_desc_fault(const ptg_mlp* d)
{
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return "batch outside [1, 2^31]";
    if (d->n_layers < 1 || d->n_layers > PTG_MLP_MAX_LAYERS) return "n_layers outside [1, PTG_MLP_MAX_LAYERS]";
    if (d->flags & ~(PTG_MLP_KEEP_HIDDEN | PTG_MLP_NARROW | PTG_MLP_WIDE)) return "unknown flag in the forward's flags";
    if ((d->flags & PTG_MLP_NARROW) && (d->flags & PTG_MLP_WIDE)) return "PTG_MLP_NARROW and PTG_MLP_WIDE exclude each other";
    if (d->hidden_act != PTG_MLP_RELU && d->hidden_act != PTG_MLP_TANH) return "hidden_act must be PTG_MLP_RELU or PTG_MLP_TANH";
    if (d->out_act != PTG_MLP_NONE && d->out_act != PTG_MLP_RELU && d->out_act != PTG_MLP_TANH) return "unknown out_act";
    if (d->f1 < 1 || d->f2 < 0 || (int64_t)d->f1 + d->f2 > PTG_MLP_MAX_WIDTH) return "need f1 >= 1, f2 >= 0, f1 + f2 <= PTG_MLP_MAX_WIDTH";
    if (!d->x_dev || d->x_s_n < d->f1) return "x_dev is null or x_s_n below f1";
    if ((d->x2_dev != nullptr) != (d->f2 > 0)) return "x2_dev and f2 > 0 go together";
    if (d->x2_dev && d->x2_s_n < d->f2) return "x2_s_n below f2";
    int fan_in = d->f1 + d->f2;
    for (int l = 0; l < d->n_layers; l++) {
        if (d->width[l] < 1 || d->width[l] > PTG_MLP_MAX_WIDTH) return "a width outside [1, PTG_MLP_MAX_WIDTH]";
        if (!d->w_dev[l] || !d->b_dev[l]) return "a null w_dev or b_dev";
        if (d->w_s_n[l] < fan_in) return "a w_s_n below the fan-in";
        fan_in = d->width[l];
    }
    if (!d->out_dev || (uintptr_t)d->out_dev % sizeof(float) != 0) return "out_dev is null or not aligned to 4 bytes";
    if (d->out_s_n < d->width[d->n_layers - 1]) return "out_s_n below the output width";
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(float) != 0) return "ws_dev is null or not aligned to 4 bytes";
    if (d->ws_bytes < ptg_mlp_workspace(d->batch, d->n_layers, d->width, d->flags)) return "ws_bytes below what ptg_mlp_workspace returns";
    return nullptr;
}

}  // namespace

extern "C" {

int64_t ptg_mlp_backward_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags)
{
    if (batch < 1 || batch > (int64_t)1 << 31 || n_layers < 1 || n_layers > PTG_MLP_MAX_LAYERS || !widths) return PTG_E_INVALID;
    if (flags & ~PTG_MLP_ACCUMULATE) return PTG_E_INVALID;
    int64_t widest = 0;
    for (int l = 0; l < n_layers; l++) {
        if (widths[l] < 1 || widths[l] > PTG_MLP_MAX_WIDTH) return PTG_E_INVALID;
        widest = std::max(widest, mlp_pitch(widths[l]));
    }
    return 2 * batch * widest * (int64_t)sizeof(float);
}

int ptg_mlp_backward(ptg_env* h, const ptg_mlp_bwd* d, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (!d) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: null descriptor");
    const ptg_mlp* f = &d->fwd;
    if (const char* why = mlp_desc_fault(f)) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: the forward's descriptor: %s", why);
    if (!(f->flags & PTG_MLP_KEEP_HIDDEN)) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: the forward's descriptor must carry PTG_MLP_KEEP_HIDDEN");
    if (d->flags & ~PTG_MLP_ACCUMULATE) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: unknown flag in %d", d->flags);
    const int n = f->n_layers;
    if (!d->gout_dev || d->gout_s_n < f->width[n - 1]) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: gout_dev is null or gout_s_n below the output width %d", f->width[n - 1]);
    int fan_in = f->f1 + f->f2;
    for (int l = 0; l < n; l++) {
        if ((d->dw_dev[l] != nullptr) != (d->db_dev[l] != nullptr)) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: dw_dev[%d] and db_dev[%d] go together", l, l);
        if (d->dw_dev[l] && d->dw_s_n[l] < fan_in) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: dw_s_n[%d] below the fan-in %d", l, fan_in);
        fan_in = f->width[l];
    }
    if (d->dx_dev && d->dx_s_n < f->f1) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: dx_s_n below f1 = %d", f->f1);
    if (d->dx2_dev && f->f2 == 0) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: dx2_dev without a second input piece");
    if (d->dx2_dev && d->dx2_s_n < f->f2) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: dx2_s_n below f2 = %d", f->f2);
    if (!d->bws_dev || (uintptr_t)d->bws_dev % sizeof(float) != 0) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: bws_dev is null or not aligned to 4 bytes");
    const int64_t need = ptg_mlp_backward_workspace(f->batch, n, f->width, d->flags);
    if (d->bws_bytes < need) return set_err(h, PTG_E_INVALID, "ptg_mlp_backward: bws_bytes = %lld, the call needs %lld", (long long)d->bws_bytes, (long long)need);
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const size_t B = (size_t)f->batch;
    size_t widest = 0, kept[PTG_MLP_MAX_LAYERS + 1] = {0};   // kept[l]: floats of ws_dev before hidden layer l
    for (int l = 0; l < n; l++) {
        widest = std::max(widest, (size_t)mlp_pitch(f->width[l]));
        kept[l + 1] = kept[l] + B * (size_t)mlp_pitch(f->width[l]);
    }
    auto buf = [&](int l) { return (float*)d->bws_dev + (size_t)(l & 1) * B * widest; };      // dz of layer l, row stride P(width[l])
    const float* dz = d->gout_dev;
    size_t dz_s = (size_t)d->gout_s_n;
    if (f->out_act != PTG_MLP_NONE) {
        MlpDzOut e{d->gout_dev, (size_t)d->gout_s_n, f->out_dev, (size_t)f->out_s_n, buf(n - 1), (size_t)mlp_pitch(f->width[n - 1]), B, f->width[n - 1]};
        const size_t total = B * (size_t)e.O;
        const unsigned blocks = (unsigned)std::min<size_t>((total - 1) / 256 + 1, 65536);
        if (f->out_act == PTG_MLP_RELU) k_mlp_dz_out<PTG_MLP_RELU><<<blocks, 256, 0, st>>>(e);
        else k_mlp_dz_out<PTG_MLP_TANH><<<blocks, 256, 0, st>>>(e);
        if (int rc = launch_check(h, "k_mlp_dz_out")) return rc;
        dz = e.dz; dz_s = e.dz_s;
    }
    for (int l = n - 1; l >= 0; l--) {
        const int O = f->width[l], K = l ? f->width[l - 1] : f->f1 + f->f2;
        const float* x = l ? (const float*)f->ws_dev + kept[l - 1] : f->x_dev;      // the layer's input: hidden layer l - 1, or the call's
        const size_t x_s = l ? (size_t)mlp_pitch(K) : (size_t)f->x_s_n;
        if (d->dw_dev[l]) {
            MlpDw a{};
            a.dz = dz; a.dz_s = dz_s; a.x = x; a.x_s = x_s; a.B = B; a.K = K; a.O = O;
            a.x2 = !l && f->x2_dev ? f->x2_dev : x; a.x2_s = !l && f->x2_dev ? (size_t)f->x2_s_n : x_s; a.F1 = l ? K : f->f1;
            a.dw = d->dw_dev[l]; a.dw_s = (size_t)d->dw_s_n[l]; a.db = d->db_dev[l]; a.accumulate = (d->flags & PTG_MLP_ACCUMULATE) != 0;
            k_mlp_dw<<<dim3((unsigned)((O - 1) / BW_TILE + 1), (unsigned)(K / BW_TILE + 1)), 64, 0, st>>>(a);
            if (int rc = launch_check(h, "k_mlp_dw")) return rc;
        }
        if (!l && !d->dx_dev && !d->dx2_dev) break;
        MlpDx a{};
        a.dz = dz; a.dz_s = dz_s; a.w = f->w_dev[l]; a.w_s = (size_t)f->w_s_n[l]; a.B = B; a.K = K; a.O = O;
        const dim3 grid((unsigned)((B - 1) / BW_TILE + 1), (unsigned)((K - 1) / BW_TILE + 1));
        if (l) {
            a.h = x; a.h_s = x_s; a.y = buf(l - 1); a.y_s = x_s; a.F1 = K;
            if (f->hidden_act == PTG_MLP_RELU) k_mlp_dx<PTG_MLP_RELU><<<grid, 64, 0, st>>>(a);
            else k_mlp_dx<PTG_MLP_TANH><<<grid, 64, 0, st>>>(a);
            dz = a.y; dz_s = a.y_s;
        } else {
            a.y = d->dx_dev; a.y_s = (size_t)d->dx_s_n; a.y2 = d->dx2_dev; a.y2_s = (size_t)d->dx2_s_n; a.F1 = f->f1;
            k_mlp_dx<PTG_MLP_NONE><<<grid, 64, 0, st>>>(a);
        }
        if (int rc = launch_check(h, "k_mlp_dx")) return rc;
    }
    return 0;
}

}  // extern "C"
