// ptg_mlp.hip -- the forward of an MLP (include/ptg_env.h, ptg_mlp_forward, states the arithmetic; tests/mlp_restatement.py
// restates it) and, in the second half of the file, its backward pass (ptg_mlp_backward; tests/mlp_backward_restatement.py).
// The forward: one launch per layer: Linear + bias + activation fused, on gfx950's exact-float32 MFMA (v_mfma_f32_16x16x4_f32 and
// v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product).  The translation unit shares ptg_handle.h with ptg_env.hip
// and ptg_train.hip and reads nothing of the handle but its device -- and, for a PTG_MLP_SPLIT_INPUT call, its
// config's raw_modified and price_ahead, its float32 market series and P.err.
//
// D = A * B + C with A = the rows of the input (A[i][k] = x[row0 + i][k]), B = the weights transposed (B[k][j] = W[col0 + j][k]) and
// C = the bias broadcast down its column.  Lane maps (one f32 VGPR per operand per lane):
//   16x16x4   lane l: A[l & 15][l >> 4], B[l >> 4][l & 15];   C/D register g: row 4 * (l >> 4) + g, column l & 15
//   32x32x2   lane l: A[l & 31][l >> 5], B[l >> 5][l & 31];   C/D register g: row (g & 3) + 8 * (g >> 2) + 4 * (l >> 5), column l & 31
// The output column is on the lane in both, so the bias of a lane's unit initialises all of its accumulator registers, and for a fixed
// register 16 (32) neighbouring lanes store neighbouring units of one row.
//
// Two routes, the same bits by construction (the order rule forbids split-K, so a small batch can only be spread over the units):
//   NARROW   one wave per workgroup, a 16-row x 16-unit tile on 16x16x4; ceil(B / 16) * ceil(O / 16) workgroups, so a 808 x 808 weight
//            matrix is read by 51 workgroups already at B = 6
//   WIDE     four waves per workgroup, a 128 x 128 tile on 32x32x2, each wave 2 x 2 tiles of 32 x 32 (four independent accumulators)
// Every MFMA kernel of the file runs its reduction through ONE pipeline, mlp_ring: chunks of 32 staged in LDS, a ring of chunks in flight
// in registers (four NARROW, two WIDE) while the matrix cores work on the current one: at the reference's batch sizes a layer is a
// dependent chain of K / 4 MFMAs.  A kernel plugs in its fetch (which tensor index rides on which lane), its LDS layout and its MFMAs, and
// keeps its epilogue.  Loads are single dwords: odd widths (743, 233) leave weight rows off 16-byte alignment and the two-piece input
// splits a row anywhere; a load instruction of a wave still reads 32 neighbouring floats of each of two rows.
// Groups (ptg_mlp_group_forward, ptg_mlp_group_backward): the 16 x 16 tile bodies of the forward and of the backward
// are device functions with two entry points each, the single kernel and a grouped one that runs the tiles of up to PTG_MLP_GROUP_MAX
// networks of equal depth in one launch; a network's bits are those of its own single call.  On the host the walk over the layers is ONE
// per direction (mlp_forward_walk, mlp_backward_walk) behind one refusal prologue (mlp_refuse): a single entry is the walk at n = 1 with
// the single kernels, a grouped entry the same walk with the grouped ones, and every grid comes from one function per kernel (mlp_grid).
#include "ptg_handle.h"

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>

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

// ---- split observation rows as the first layer's input (include/ptg_env.h, PTG_MLP_SPLIT_INPUT) --------------------
// The first piece is [B][16] split rows, and layer 0 reads the SB3_FLAT row they stand for: column k < F1 is one of the row's 14 env
// columns, or series[(int) row[14 | 15] + q] of a market sub-space.  A lane's column is fixed over its rows, so the source is resolved
// once per lane and chunk (mlp_split_col) and a row costs one load of the row's column and one of the series (mlp_split_x).  Both are
// branch-free, as mlp_x is: the index is clamped into the series before it becomes an address, whatever the row holds; a lane on an env
// column or on the second piece reads series word 0 and discards it.  An index that is no integer in [0, last] makes the row's market
// columns NaN and raises err[4] (PTG_E_INDEX at the next ptg_sync): one store per lane behind the reduction.
// Only the split instantiations carry an MlpSplit; the flat ones are given the empty MlpFlat and compile to what they were.
struct MlpFlat {};
struct MlpSplit {                        // by value in the launch: a captured call holds no host memory
    const float* pool;                   // the handle's float32 series, one allocation (ptg_handle.h: d_pool32)
    int off[3];                          // market sub-space m of the flat row: column k0 + q = pool[off[m] + index + q], 0 <= q < len
    unsigned seg[3];                     // k0 | len << 16 | daily << 31 (len 0: unused); daily: the index is column 15 of a split row, the day, not column 14
    int last_hour, last_day;             // the last valid indices
    int* err;                            // DevParams::err
};
template <typename S>
constexpr bool mlp_is_split = std::is_same<S, MlpSplit>::value;

// The 14 env columns keep one order in every flat row, whatever raw_modified and price_ahead insert between them (the keys sort the same):
// nibble e is the split column of the e-th flat column that is no market column (mlp_split_args checks it against the sorted map)
constexpr unsigned long long MLP_SPLIT_ENV_ORDER = 0xCD654321097AB8ull;

struct MlpSplitCol {                     // where a lane's column comes from
    const float* p; size_t ps;           // row b's word: p[b * ps]: the env column, the index column or the second piece's column
    const float* sp; int last;           // market: the series moved on by q, and the last valid index
    unsigned nan;                        // market: the bits of a quiet NaN, else 0
};

// k inside [0, K); A: MlpLayer or MlpDw.  The sub-spaces are visited by template argument, not by a loop counter
template <typename A, int... M>
__device__ __forceinline__ MlpSplitCol mlp_split_col(const A& a, const MlpSplit& s, int k, std::integer_sequence<int, M...>)
{
    int e = k, c = 0, last = s.last_hour;                    // e: k less the market columns below it
    const float* sp = s.pool;
    bool market = false;
    auto sub = [&](int off, unsigned seg) {
        const int k0 = seg & 0xffff, len = (seg >> 16) & 0x7fff;
        const bool daily = seg >> 31, in = k >= k0 && k < k0 + len;
        sp = in ? s.pool + (off + k - k0) : sp;
        last = in ? (daily ? s.last_day : s.last_hour) : last;
        c = in ? (daily ? 15 : 14) : c;
        market = market || in;
        e -= k >= k0 + len ? len : 0;
    };
    (sub(s.off[M], s.seg[M]), ...);
    c = market ? c : (int)(MLP_SPLIT_ENV_ORDER >> (4 * min(max(e, 0), 13))) & 15;
    // The pieces are read BEFORE the choice between them.  Read inside its arms, the choice becomes a choice between two addresses
    // inside the fetch's closure, and the closure, the MlpSplit with it, then stays in scratch (544 bytes in k_mlp_layer_split)
    const float *const x = a.x, *const x2 = a.x2;
    const size_t x_s = a.x_s, x2_s = a.x2_s;
    const int F1 = a.F1;                 // the market sub-spaces end below it
    const bool second = k >= F1;
    return MlpSplitCol{second ? x2 + (size_t)(k - F1) : x + (size_t)c, second ? x2_s : x_s, sp, last, market ? 0x7fc00000u : 0u};
}

template <typename A>
__device__ __forceinline__ MlpSplitCol mlp_split_col(const A& a, const MlpSplit& s, int k)
{
    return mlp_split_col(a, s, k, std::make_integer_sequence<int, 3>{});
}

// row inside [0, B).  i is an address only after the clamp; (float) i == f holds for an integer in [0, last] and for nothing else
// (NaN, Inf, a fraction, a negative value, one past the end), last < 2^24 (mlp_desc_fault).  The verdict is kept as bits to OR into
// the series word -- any word with them is a NaN, a word without them itself -- and not as a lane mask: a mask per row in flight, beside
// the edge masks, is what the 128 x 128 route has no scalar registers for (63 spilled)
__device__ __forceinline__ float mlp_split_x(const MlpSplitCol& c, size_t row, unsigned& bad)
{
    const float f = c.p[row * c.ps];
    const int i = min((int)(f >= 0.0f ? fminf(f, 2.0e9f) : 0.0f), c.last);
    const unsigned poison = (float)i == f ? 0u : c.nan;
    bad |= poison;
    const float v = c.sp[i];
    return c.nan ? __uint_as_float(__float_as_uint(v) | poison) : f;
}

template <int ACT>
__device__ __forceinline__ float mlp_act(float v)
{
    if constexpr (ACT == PTG_MLP_RELU) return v > 0.0f ? v : (v != v ? v : 0.0f);
    else if constexpr (ACT == PTG_MLP_TANH) return (float)tanh((double)v);
    else return v;
}

// The pipeline over a reduction of length n (int K or O, size_t B) in chunks of RC: fetch(d, r0) loads the chunk at r0 into slot d of the
// kernel's register ring, stage(d) writes slot d to LDS, mma() consumes the staged chunk.  DEPTH chunks are in flight; a slot is
// refetched, DEPTH chunks ahead, as soon as it is staged.  d is static once unrolled; the break is uniform over the workgroup.  The
// lambdas capture what they only read by value and the ring and the accumulator by reference: these loops are optimised before they are
// inlined into the kernel, and behind reference captures the tile's invariants might alias the ring, so every prologue slot recomputed them
// (120 to 170 instructions per slot; k_mlp_dw, whose slots are short, is the exception and says why).
template <int DEPTH, int RC, typename N, typename Fetch, typename Stage, typename Mma>
__device__ __forceinline__ void mlp_ring(N n, Fetch fetch, Stage stage, Mma mma)
{
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if ((N)(d * RC) < n) fetch(d, (N)(d * RC));
    for (N r0 = 0; r0 < n; r0 += DEPTH * RC) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const N rc = r0 + d * RC;
            if (rc >= n) break;
            stage(d);
            __syncthreads();
            if (rc + DEPTH * RC < n) fetch(d, rc + DEPTH * RC);
            mma();
            __syncthreads();
        }
    }
}

// One chunk of 32 on 16x16x4, four ascending reduction indices per instruction: step s reads as[ia(s)] and bs[ib(s)].  All operands of
// the chunk come out of LDS first, then the MFMAs run back to back: the chain is the layer's latency at small B.  A ragged last chunk
// runs its padded steps too: both operands are 0 there, which is exact.
template <typename IA, typename IB>
__device__ __forceinline__ void mlp_chain16(const float* as, const float* bs, IA ia, IB ib, f32x4& acc)
{
    float av[NR_KC / 4], bv[NR_KC / 4];
#pragma unroll
    for (int s = 0; s < NR_KC / 4; s++) {
        av[s] = as[ia(s)];
        bv[s] = bs[ib(s)];
    }
#pragma unroll
    for (int s = 0; s < NR_KC / 4; s++)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
}

// The NARROW tile (bx, by) of a layer: the body of k_mlp_layer<ACT, MLP_NARROW> and of k_mlp_layer_group<ACT>, which picks `a` out of its group
template <int ACT, typename S>
__device__ __forceinline__ void mlp_layer_tile16(const MlpLayer a, const S s, unsigned bx, unsigned by)
{
    __shared__ float xs[NR_TILE * NR_PITCH], ws[NR_TILE * NR_PITCH];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const size_t row0 = (size_t)bx * NR_TILE;
    const int col0 = (int)by * NR_TILE;
    const float bj = col0 + r < a.O ? a.bias[col0 + r] : 0.0f;
    f32x4 acc = {bj, bj, bj, bj};
    constexpr int PER = NR_TILE * NR_KC / 64;            // 8 rows and 8 units per lane and chunk
    float xr[NR_DEPTH][PER], wr[NR_DEPTH][PER];
    const int kx = lane & 31, r2 = lane >> 5;
    auto fetch = [=, &xr, &wr](int d, int k0) {          // lane: k = k0 + kx of every second row and unit; 0 beyond an edge
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
    // the split fetch: the source of column k once per chunk
    [[maybe_unused]] unsigned bad = 0;                   // this lane met an invalid index
    [[maybe_unused]] auto fetch_split = [=, &xr, &wr, &bad](int d, int k0) {
        (void)xr, (void)wr, (void)bad;
        if constexpr (mlp_is_split<S>) {      // the flat instantiations give this body nothing to compile
            const int k = k0 + kx;
            const bool kin = k < a.K;
            const MlpSplitCol src = mlp_split_col(a, s, min(k, a.K - 1));
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int rr = r2 + 2 * i;
                const size_t row = row0 + rr;
                const int u = col0 + rr;
                const float v = mlp_split_x(src, min(row, a.B - 1), bad);
                xr[d][i] = kin ? v : 0.0f;                   // a row beyond B repeats row B - 1 and is never stored: no mask per row (mlp_split_x)
                wr[d][i] = mlp_w(a, u, k, kin);                 // nor per unit: a unit beyond O repeats unit O - 1 and is never stored
            }
        }
    };
    auto stage = [=, &xr, &wr](int d) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            xs[(r2 + 2 * i) * NR_PITCH + kx] = xr[d][i];
            ws[(r2 + 2 * i) * NR_PITCH + kx] = wr[d][i];
        }
    };
    auto at = [=](int s) { return r * NR_PITCH + 4 * s + q; };
    if constexpr (mlp_is_split<S>) {
        mlp_ring<NR_DEPTH, NR_KC>(a.K, fetch_split, stage, [=, &acc] { mlp_chain16(xs, ws, at, at, acc); });
        if (bad) s.err[4] = 1;
    } else {
        mlp_ring<NR_DEPTH, NR_KC>(a.K, fetch, stage, [=, &acc] { mlp_chain16(xs, ws, at, at, acc); });
    }
    const int u = col0 + r;
    if (u < a.O) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const size_t row = row0 + 4 * q + g;
            if (row < a.B) a.y[row * a.y_s + (size_t)u] = mlp_act<ACT>(acc[g]);
        }
    }
}

// The WIDE tile of a layer: the body of k_mlp_layer<ACT, MLP_WIDE> and of its split twin
template <int ACT, typename S>
__device__ __forceinline__ void mlp_layer_tile128(const MlpLayer a, const S s)
{
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
    auto fetch = [=, &xr, &wr](int d, int k0) {
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
    [[maybe_unused]] unsigned bad = 0;
    [[maybe_unused]] auto fetch_split = [=, &xr, &wr, &bad](int d, int k0) {
        (void)xr, (void)wr, (void)bad;
        if constexpr (mlp_is_split<S>) {      // the flat instantiations give this body nothing to compile
            const int k = k0 + kx;
            const bool kin = k < a.K;
            const MlpSplitCol src = mlp_split_col(a, s, min(k, a.K - 1));
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int rr = r8 + 8 * i;
                const size_t row = row0 + rr;
                const int u = col0 + rr;
                const float v = mlp_split_x(src, min(row, a.B - 1), bad);
                xr[d][i] = kin ? v : 0.0f;                   // a row beyond B repeats row B - 1 and is never stored: no mask per row (mlp_split_x)
                wr[d][i] = mlp_w(a, u, k, kin);                 // nor per unit: a unit beyond O repeats unit O - 1 and is never stored
            }
        }
    };
    auto stage = [=, &xr, &wr](int d) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            xs[(r8 + 8 * i) * WD_PITCH + kx] = xr[d][i];
            ws[(r8 + 8 * i) * WD_PITCH + kx] = wr[d][i];
        }
    };
    auto mma = [=, &acc] {
        if (!live) return;
#pragma unroll
        for (int p = 0; p < WD_KC / 2; p++) {            // two ascending k per instruction; unrolled, so the LDS reads run ahead of the MFMAs
            const float a0 = xs[(wr_ * 64 + c) * WD_PITCH + 2 * p + hf], a1 = xs[(wr_ * 64 + 32 + c) * WD_PITCH + 2 * p + hf];
            const float b0 = ws[(wc * 64 + c) * WD_PITCH + 2 * p + hf], b1 = ws[(wc * 64 + 32 + c) * WD_PITCH + 2 * p + hf];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    };
    if constexpr (mlp_is_split<S>) {
        mlp_ring<WD_DEPTH, WD_KC>(a.K, fetch_split, stage, mma);
        if (bad) s.err[4] = 1;
    } else {
        mlp_ring<WD_DEPTH, WD_KC>(a.K, fetch, stage, mma);
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

template <int ACT, int ROUTE>
__global__ __launch_bounds__(ROUTE == MLP_NARROW ? 64 : 256) void k_mlp_layer(const MlpLayer a)
{
    if constexpr (ROUTE == MLP_NARROW) mlp_layer_tile16<ACT>(a, MlpFlat{}, blockIdx.x, blockIdx.y);
    else mlp_layer_tile128<ACT>(a, MlpFlat{});
}

// layer 0 of a PTG_MLP_SPLIT_INPUT call
template <int ACT, int ROUTE>
__global__ __launch_bounds__(ROUTE == MLP_NARROW ? 64 : 256) void k_mlp_layer_split(const MlpLayer a, const MlpSplit s)
{
    if constexpr (ROUTE == MLP_NARROW) mlp_layer_tile16<ACT>(a, s, blockIdx.x, blockIdx.y);
    else mlp_layer_tile128<ACT>(a, s);
}

// a runtime activation as a template argument: f(std::integral_constant<int, ACT>)
template <typename F>
void mlp_with_act(int act, F f)
{
    if (act == PTG_MLP_RELU) f(std::integral_constant<int, PTG_MLP_RELU>{});
    else if (act == PTG_MLP_TANH) f(std::integral_constant<int, PTG_MLP_TANH>{});
    else f(std::integral_constant<int, PTG_MLP_NONE>{});
}

// ---- the grouped launches (include/ptg_env.h, ptg_mlp_group_forward) ------------------------------------------------
// Up to PTG_MLP_GROUP_MAX networks in one launch: the by-value structs of the single kernels side by side in the kernel arguments,
// blockIdx.z picks the network, gridDim.x / .y are the largest tile counts of the group.  The tile bodies are the single kernels': a
// network's bits are those of its own call.  A workgroup whose tile lies outside its network, or whose network takes no part in the
// launch, returns before any load and before the first barrier; every test for that is uniform over the workgroup.  net[blockIdx.z]
// is read out of the kernel-argument segment with scalar loads at a computed offset: no private copy (profiles/mlp_group_resources.txt).
template <typename T>
struct MlpGroup {
    T net[PTG_MLP_GROUP_MAX];
};

template <int ACT>
__global__ __launch_bounds__(64) void k_mlp_layer_group(const MlpGroup<MlpLayer> g)
{
    const MlpLayer& a = g.net[blockIdx.z];
    if ((size_t)blockIdx.x * NR_TILE >= a.B || (int)blockIdx.y * NR_TILE >= a.O) return;
    mlp_layer_tile16<ACT>(a, MlpFlat{}, blockIdx.x, blockIdx.y);
}

template <int ACT>
__global__ __launch_bounds__(64) void k_mlp_layer_group_split(const MlpGroup<MlpLayer> g, const MlpSplit s)      // one map: the networks share the handle
{
    const MlpLayer& a = g.net[blockIdx.z];
    if ((size_t)blockIdx.x * NR_TILE >= a.B || (int)blockIdx.y * NR_TILE >= a.O) return;
    mlp_layer_tile16<ACT>(a, s, blockIdx.x, blockIdx.y);
}

// The grid of a launch: the component-wise maximum over the networks that take part, blockIdx.z the network.  own(i) is the grid network i
// needs by itself (mlp_layer_grid, mlp_dw_grid, mlp_dx_grid, mlp_dz_out_blocks), or dim3() where it only rides along.  One network: its own grid.
template <typename Own>
dim3 mlp_grid(int n_nets, Own own)
{
    dim3 grid(1, 1, (unsigned)n_nets);
    for (int i = 0; i < n_nets; i++) {
        const dim3 e = own(i);
        grid.x = std::max(grid.x, e.x);
        grid.y = std::max(grid.y, e.y);
    }
    return grid;
}

dim3 mlp_layer_grid(const MlpLayer& a, int tile)
{
    return dim3((unsigned)((a.B - 1) / tile + 1), (unsigned)((a.O - 1) / tile + 1));      // x: up to 2^27 row tiles
}

// The layout of both workspaces (include/ptg_env.h): a hidden layer and a dz buffer are [batch][pitch(l)] floats
struct MlpLayout {
    int64_t batch;
    int n;
    const int32_t* width;
    bool in_range() const
    {
        if (batch < 1 || batch > (int64_t)1 << 31 || n < 1 || n > PTG_MLP_MAX_LAYERS || !width) return false;
        for (int l = 0; l < n; l++)
            if (width[l] < 1 || width[l] > PTG_MLP_MAX_WIDTH) return false;
        return true;
    }
    int64_t pitch(int l) const { return ((int64_t)width[l] + 3) / 4 * 4; }
    int64_t kept(int l) const            // floats of the forward's ws_dev before hidden layer l (KEEP_HIDDEN)
    {
        int64_t sum = 0;
        for (int i = 0; i < l; i++) sum += batch * pitch(i);
        return sum;
    }
    int64_t alt(int l, int layers) const // floats before layer l's of the two alternating buffers, each as wide as the widest of the first `layers`
    {
        int64_t widest = 0;
        for (int i = 0; i < layers; i++) widest = std::max(widest, pitch(i));
        return (l & 1) * batch * widest;
    }
    int64_t forward_bytes(int flags) const { return std::max<int64_t>(16, ((flags & PTG_MLP_KEEP_HIDDEN) ? kept(n - 1) : 2 * alt(1, n - 1)) * (int64_t)sizeof(float)); }
    int64_t backward_bytes() const { return 2 * alt(1, n) * (int64_t)sizeof(float); }
};

__attribute__((format(printf, 3, 4))) bool mlp_fault(char* why, size_t cap, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why, cap, fmt, ap);
    va_end(ap);
    return true;
}

constexpr int MLP_FWD_FLAGS = PTG_MLP_KEEP_HIDDEN | PTG_MLP_NARROW | PTG_MLP_WIDE | PTG_MLP_SPLIT_INPUT;

// The SB3_FLAT row of handle h as a split call rebuilds it: ptg_create's column map (sub-spaces by sorted key, METH_STATUS one-hot over
// six columns; rl_ptg_amd/policy_split.py restates it as flat_columns / env_columns) over the handle's float32 series.  Returns the row's
// width, 2 P + 14 for 'mod' and P + 18 for 'raw' (-1: the sorted map does not have the env columns in the kernels' order); s may be null
int mlp_split_args(const ptg_env* h, MlpSplit* s)
{
    struct Sub { const char* key; int width, split_col, which; };      // split_col: first column of a split row (env); which: the series (market)
    const int P = h->cfg.price_ahead;
    std::vector<Sub> subs;
    if (h->cfg.raw_modified) { subs.push_back({"Pot_Reward", P, -1, 0}); subs.push_back({"Part_Full", P, -1, 1}); }
    else { subs.push_back({"Elec_Price", P, -1, 0}); subs.push_back({"Gas_Price", 2, -1, 2}); subs.push_back({"EUA_Price", 2, -1, 3}); }
    const char* tail[9] = {"METH_STATUS", "T_CAT", "H2_in_MolarFlow", "CH4_syn_MolarFlow", "H2_res_MolarFlow", "H2O_DE_MassFlow", "Elec_Heating", "Temp_hour_enc_sin",
                           "Temp_hour_enc_cos"};
    for (int q = 0; q < 9; q++) subs.push_back({tail[q], q ? 1 : 6, q ? 5 + q : 0, -1});
    std::sort(subs.begin(), subs.end(), [](const Sub& a, const Sub& b) { return strcmp(a.key, b.key) < 0; });      // Python's sorted() of ASCII keys
    const float* series[4] = {h->P.featA32, h->P.featB32, h->P.gas_n32, h->P.eua_n32};      // all inside d_pool32, featA32 its first word
    int k = 0, m = 0, e = 0;
    bool ordered = true;                 // the env columns come in MLP_SPLIT_ENV_ORDER
    if (s) {
        *s = MlpSplit{};
        s->pool = h->d_pool32; s->last_hour = h->n_sets * h->P.n_hours - P; s->last_day = h->n_sets * h->P.n_days - 2; s->err = h->P.err;
    }
    for (const Sub& sb : subs) {
        if (sb.which >= 0) {
            if (s) { s->off[m] = (int)(series[sb.which] - h->d_pool32); s->seg[m] = (unsigned)k | (unsigned)sb.width << 16 | (sb.which >= 2 ? 1u << 31 : 0u); }
            m++;
        } else {
            for (int j = 0; j < sb.width; j++, e++) ordered = ordered && (int)((MLP_SPLIT_ENV_ORDER >> (4 * e)) & 15) == sb.split_col + j;
        }
        k += sb.width;
    }
    return ordered && e == 14 ? k : -1;
}

// what ptg_mlp_forward refuses in a descriptor, for it and for the backward's embedded one: false when d is well-formed, else the text in why
bool mlp_desc_fault(const ptg_env* h, const ptg_mlp* d, char* why, size_t cap)
{
    if (d->batch < 1 || d->batch > (int64_t)1 << 31) return mlp_fault(why, cap, "batch %lld outside [1, 2^31]", (long long)d->batch);
    if (d->n_layers < 1 || d->n_layers > PTG_MLP_MAX_LAYERS) return mlp_fault(why, cap, "n_layers %d outside [1, %d]", d->n_layers, PTG_MLP_MAX_LAYERS);
    if (d->flags & ~MLP_FWD_FLAGS) return mlp_fault(why, cap, "unknown flag in %d", d->flags);
    if ((d->flags & PTG_MLP_NARROW) && (d->flags & PTG_MLP_WIDE)) return mlp_fault(why, cap, "PTG_MLP_NARROW and PTG_MLP_WIDE exclude each other");
    if (d->hidden_act != PTG_MLP_RELU && d->hidden_act != PTG_MLP_TANH) return mlp_fault(why, cap, "hidden_act must be PTG_MLP_RELU or PTG_MLP_TANH");
    if (d->out_act != PTG_MLP_NONE && d->out_act != PTG_MLP_RELU && d->out_act != PTG_MLP_TANH) return mlp_fault(why, cap, "unknown out_act %d", d->out_act);
    if (d->f1 < 1 || d->f2 < 0 || (int64_t)d->f1 + d->f2 > PTG_MLP_MAX_WIDTH)
        return mlp_fault(why, cap, "f1 = %d, f2 = %d: need f1 >= 1, f2 >= 0, f1 + f2 <= %d", d->f1, d->f2, PTG_MLP_MAX_WIDTH);
    if (d->flags & PTG_MLP_SPLIT_INPUT) {
        const int flat = mlp_split_args(h, nullptr);
        if (d->f1 != flat) return mlp_fault(why, cap, "PTG_MLP_SPLIT_INPUT: f1 = %d, the handle's flat row has %d columns", d->f1, flat);
        if (!d->x_dev) return mlp_fault(why, cap, "x_dev is null");
        if (d->x_s_n < 16) return mlp_fault(why, cap, "PTG_MLP_SPLIT_INPUT: x_s_n = %lld below the 16 columns of a split row", (long long)d->x_s_n);
        const int64_t hours = (int64_t)h->n_sets * h->P.n_hours, days = (int64_t)h->n_sets * h->P.n_days;
        if (hours < h->cfg.price_ahead || days < 2 || hours > (int64_t)1 << 24 || days > (int64_t)1 << 24)
            return mlp_fault(why, cap, "PTG_MLP_SPLIT_INPUT: %lld hours and %lld days of market series: shorter than one window, or indices not exact in float32", (long long)hours, (long long)days);
    } else if (!d->x_dev || d->x_s_n < d->f1) return mlp_fault(why, cap, "x_dev is null or x_s_n below f1 = %d", d->f1);
    if ((d->x2_dev != nullptr) != (d->f2 > 0)) return mlp_fault(why, cap, "x2_dev and f2 > 0 go together");
    if (d->x2_dev && d->x2_s_n < d->f2) return mlp_fault(why, cap, "x2_s_n below f2 = %d", d->f2);
    const int n = d->n_layers;
    int fan_in = d->f1 + d->f2;
    for (int l = 0; l < n; l++) {
        if (d->width[l] < 1 || d->width[l] > PTG_MLP_MAX_WIDTH) return mlp_fault(why, cap, "width[%d] = %d outside [1, %d]", l, d->width[l], PTG_MLP_MAX_WIDTH);
        if (!d->w_dev[l] || !d->b_dev[l]) return mlp_fault(why, cap, "null w_dev or b_dev [%d]", l);
        if (d->w_s_n[l] < fan_in) return mlp_fault(why, cap, "w_s_n[%d] below the fan-in %d", l, fan_in);
        fan_in = d->width[l];
    }
    if (!d->out_dev || (uintptr_t)d->out_dev % sizeof(float) != 0) return mlp_fault(why, cap, "out_dev is null or not aligned to 4 bytes");
    if (d->out_s_n < d->width[n - 1]) return mlp_fault(why, cap, "out_s_n below the output width %d", d->width[n - 1]);
    if (!d->ws_dev || (uintptr_t)d->ws_dev % sizeof(float) != 0) return mlp_fault(why, cap, "ws_dev is null or not aligned to 4 bytes");
    const int64_t need = MlpLayout{d->batch, n, d->width}.forward_bytes(d->flags);
    if (d->ws_bytes < need) return mlp_fault(why, cap, "ws_bytes = %lld, the call needs %lld", (long long)d->ws_bytes, (long long)need);
    return false;
}

// The launch arguments of a forward call, layer by layer: the call's input, then layer l's parameters and output, then that output as
// the next layer's input
MlpLayer mlp_first_input(const ptg_mlp* d)
{
    MlpLayer a{};
    a.B = (size_t)d->batch;
    a.x = d->x_dev; a.x_s = (size_t)d->x_s_n; a.x2 = d->x2_dev ? d->x2_dev : d->x_dev; a.x2_s = (size_t)d->x2_s_n;
    a.F1 = d->f1; a.K = d->f1 + d->f2;
    return a;
}

void mlp_set_layer(MlpLayer& a, const ptg_mlp* d, int l)
{
    const int n = d->n_layers;
    const MlpLayout lay{d->batch, n, d->width};
    a.w = d->w_dev[l]; a.w_s = (size_t)d->w_s_n[l]; a.bias = d->b_dev[l]; a.O = d->width[l];
    if (l == n - 1) {
        a.y = d->out_dev; a.y_s = (size_t)d->out_s_n;
    } else {
        a.y = (float*)d->ws_dev + ((d->flags & PTG_MLP_KEEP_HIDDEN) ? lay.kept(l) : lay.alt(l, n - 1));
        a.y_s = (size_t)lay.pitch(l);
    }
}

void mlp_next_input(MlpLayer& a)
{
    a.x = a.x2 = a.y; a.x_s = a.y_s; a.x2_s = 0; a.F1 = a.K = a.O;      // this layer's output is the next one's input
}

// what a group refuses beyond its descriptors' own faults: a route that is not the 16 x 16 one, and a disagreement with net 0 in a field
// that the launches share.  nets: ptg_mlp, or ptg_mlp_bwd (which begins with one), `stride` bytes apart
bool mlp_group_fault(const void* nets, size_t stride, int n_nets, char* why, size_t cap)
{
    auto net = [&](int i) { return (const ptg_mlp*)((const char*)nets + (size_t)i * stride); };
    const ptg_mlp* a = net(0);
    for (int i = 0; i < n_nets; i++) {
        const ptg_mlp* b = net(i);
        if (b->flags & PTG_MLP_WIDE) return mlp_fault(why, cap, "net %d: PTG_MLP_WIDE: a group runs the 16 x 16 route", i);
        if (b->batch != a->batch) return mlp_fault(why, cap, "nets 0 and %d disagree in batch: %lld and %lld", i, (long long)a->batch, (long long)b->batch);
        if (b->n_layers != a->n_layers) return mlp_fault(why, cap, "nets 0 and %d disagree in n_layers: %d and %d", i, a->n_layers, b->n_layers);
        if (b->hidden_act != a->hidden_act) return mlp_fault(why, cap, "nets 0 and %d disagree in hidden_act: %d and %d", i, a->hidden_act, b->hidden_act);
        if (b->out_act != a->out_act) return mlp_fault(why, cap, "nets 0 and %d disagree in out_act: %d and %d", i, a->out_act, b->out_act);
        if (b->flags != a->flags) return mlp_fault(why, cap, "nets 0 and %d disagree in flags: %d and %d", i, a->flags, b->flags);
    }
    return false;
}

// What all four entries refuse before their first launch, in one order: the array, the count, each descriptor's own fault (`fault`:
// mlp_desc_fault or mlp_bwd_fault; grouped: behind "net i: "), then, grouped, what the networks must agree in.  0, or the error set in h
template <typename D, typename Fault>
int mlp_refuse(ptg_env* h, const char* who, const D* nets, int n_nets, bool grouped, Fault fault)
{
    if (!nets) return set_err(h, PTG_E_INVALID, "%s: null descriptor%s", who, grouped ? " array" : "");
    if (n_nets < 1 || n_nets > PTG_MLP_GROUP_MAX) return set_err(h, PTG_E_INVALID, "%s: n_nets %d outside [1, %d]", who, n_nets, PTG_MLP_GROUP_MAX);
    char why[240];
    for (int i = 0; i < n_nets; i++) {
        if (!fault(&nets[i], why, sizeof why)) continue;
        return grouped ? set_err(h, PTG_E_INVALID, "%s: net %d: %s", who, i, why) : set_err(h, PTG_E_INVALID, "%s: %s", who, why);
    }
    if (!grouped) return 0;
    if (mlp_group_fault(nets, sizeof(D), n_nets, why, sizeof why)) return set_err(h, PTG_E_INVALID, "%s: %s", who, why);
    if constexpr (std::is_same<D, ptg_mlp_bwd>::value)
        for (int i = 1; i < n_nets; i++)
            if (nets[i].flags != nets[0].flags)
                return set_err(h, PTG_E_INVALID, "%s: nets 0 and %d disagree in the backward's flags: %d and %d", who, i, nets[0].flags, nets[i].flags);
    return 0;
}

// THE forward: ptg_mlp_forward is this walk over one network with the single kernel (and its NARROW / WIDE choice), ptg_mlp_group_forward
// the same walk with the grouped kernel.  `grouped` is the entry that was called, not n_nets > 1: a group of one launches the grouped kernel
int mlp_forward_walk(ptg_env* h, const char* who, const ptg_mlp* nets, int n_nets, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = mlp_refuse(h, who, nets, n_nets, grouped, [h](const ptg_mlp* d, char* why, size_t cap) { return mlp_desc_fault(h, d, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_mlp* d = &nets[0];         // depth, activations, batch and flags: the group's
    const int n = d->n_layers;
    MlpSplit s{};                        // PTG_MLP_SPLIT_INPUT: layer 0 of every network rebuilds its flat row
    if (d->flags & PTG_MLP_SPLIT_INPUT) mlp_split_args(h, &s);
    MlpGroup<MlpLayer> g{};
    for (int i = 0; i < n_nets; i++) g.net[i] = mlp_first_input(&nets[i]);
    for (int l = 0; l < n; l++) {
        for (int i = 0; i < n_nets; i++) mlp_set_layer(g.net[i], &nets[i], l);
        const MlpLayer& a = g.net[0];
        const bool wide = !grouped && ((d->flags & PTG_MLP_WIDE) || (!(d->flags & PTG_MLP_NARROW) && ((d->batch >= MLP_WIDE_MIN_ROWS && a.O > MLP_WIDE_MIN_UNITS) || (d->batch >= MLP_WIDE_MIN_ROWS_BROAD && a.O > MLP_BROAD_UNITS))));
        const dim3 grid = mlp_grid(n_nets, [&](int i) { return mlp_layer_grid(g.net[i], wide ? WD_TILE : NR_TILE); });
        mlp_with_act(l == n - 1 ? d->out_act : d->hidden_act, [&](auto A) {
            constexpr int ACT = decltype(A)::value;
            if (l == 0 && (d->flags & PTG_MLP_SPLIT_INPUT)) {
                if (grouped) k_mlp_layer_group_split<ACT><<<grid, 64, 0, st>>>(g, s);
                else if (wide) k_mlp_layer_split<ACT, MLP_WIDE><<<grid, 256, 0, st>>>(a, s);
                else k_mlp_layer_split<ACT, MLP_NARROW><<<grid, 64, 0, st>>>(a, s);
            } else if (grouped) k_mlp_layer_group<ACT><<<grid, 64, 0, st>>>(g);
            else if (wide) k_mlp_layer<ACT, MLP_WIDE><<<grid, 256, 0, st>>>(a);
            else k_mlp_layer<ACT, MLP_NARROW><<<grid, 64, 0, st>>>(a);
        });
        if (int rc = launch_check(h, grouped ? "k_mlp_layer_group" : "k_mlp_layer")) return rc;
        for (int i = 0; i < n_nets; i++) mlp_next_input(g.net[i]);
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t ptg_mlp_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags)
{
    const MlpLayout lay{batch, n_layers, widths};
    if (!lay.in_range() || (flags & ~MLP_FWD_FLAGS) || ((flags & PTG_MLP_NARROW) && (flags & PTG_MLP_WIDE))) return PTG_E_INVALID;      // PTG_MLP_SPLIT_INPUT changes no size
    return lay.forward_bytes(flags);
}

int ptg_mlp_forward(ptg_env* h, const ptg_mlp* d, void* stream)
{
    return mlp_forward_walk(h, "ptg_mlp_forward", d, 1, false, stream);
}

int ptg_mlp_group_forward(ptg_env* h, const ptg_mlp* nets, int32_t n_nets, void* stream)
{
    return mlp_forward_walk(h, "ptg_mlp_group_forward", nets, n_nets, true, stream);
}

}  // extern "C"

// ---- the backward pass (include/ptg_env.h, ptg_mlp_backward, states the arithmetic) ---------------------------------
// Two kernels per layer on v_mfma_f32_16x16x4_f32, one wave per workgroup, a 16 x 16 tile, the reduction through mlp_ring and mlp_chain16
// as in the NARROW route (four chunks in flight in k_mlp_dx, two in k_mlp_dw).  The lane maps are the forward's; what a kernel plugs in is
// which tensor index rides on which:
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
static_assert(BW_RC == NR_KC, "mlp_chain16 consumes chunks of NR_KC");

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

// The tile bodies: each is its single kernel's whole text and the grouped kernel's, which picks `a` out of its group (forward half of the file)
template <int ACT_BELOW>
__device__ __forceinline__ void mlp_dx_tile(const MlpDx a, unsigned bx, unsigned by)
{
    __shared__ float zs[BW_TILE * NR_PITCH], wt[BW_RC * BW_PITCH_T];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const size_t row0 = (size_t)bx * BW_TILE;
    const int col0 = (int)by * BW_TILE;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int PER = BW_TILE * BW_RC / 64;                // 8 elements of dz and 8 of W per lane and chunk
    float zr[BW_DEPTH][PER], wr[BW_DEPTH][PER];
    const int jx = lane & 31, r2 = lane >> 5;
    const int kw = col0 + r, kwc = min(kw, a.K - 1);
    auto fetch = [=, &zr, &wr](int d, int j0) {              // dz: j = j0 + jx of every second row;  W: column kw of every fourth row j
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
    auto stage = [=, &zr, &wr](int d) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            zs[(r2 + 2 * i) * NR_PITCH + jx] = zr[d][i];
            wt[(q + 4 * i) * BW_PITCH_T + r] = wr[d][i];
        }
    };
    mlp_ring<BW_DEPTH, BW_RC>(a.O, fetch, stage, [=, &acc] {
        mlp_chain16(zs, wt, [=](int s) { return r * NR_PITCH + 4 * s + q; }, [=](int s) { return (4 * s + q) * BW_PITCH_T + r; }, acc);
    });
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

template <int ACT_BELOW>
__global__ __launch_bounds__(64) void k_mlp_dx(const MlpDx a)
{
    mlp_dx_tile<ACT_BELOW>(a, blockIdx.x, blockIdx.y);
}

template <int ACT_BELOW>
__global__ __launch_bounds__(64) void k_mlp_dx_group(const MlpGroup<MlpDx> g)
{
    const MlpDx& a = g.net[blockIdx.z];
    if (ACT_BELOW == PTG_MLP_NONE && !a.y && !a.y2) return;      // this network wants no first-layer dx
    if ((size_t)blockIdx.x * BW_TILE >= a.B || (int)blockIdx.y * BW_TILE >= a.K) return;
    mlp_dx_tile<ACT_BELOW>(a, blockIdx.x, blockIdx.y);
}

template <typename S>
__device__ __forceinline__ void mlp_dw_tile(const MlpDw a, const S s, unsigned bx, unsigned by)
{
    __shared__ float zs[BW_RC * BW_PITCH_T], xs[BW_RC * BW_PITCH_T];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int j0 = (int)bx * BW_TILE, k0 = (int)by * BW_TILE;      // k runs to K inclusive: column K is the bias gradient
    const int ko = k0 + r;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.accumulate && ko <= a.K) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int j = j0 + 4 * q + g;
            if (j < a.O) acc[g] = ko < a.K ? a.dw[(size_t)j * a.dw_s + (size_t)ko] : a.db[j];
        }
    }
    constexpr int DEPTH = PTG_MLP_DW_DEPTH, PER = BW_TILE * BW_RC / 64;      // chunks in flight; 8 rows per lane and chunk
    float zr[DEPTH][PER], xr[DEPTH][PER];
    const int jz = j0 + r, jzc = min(jz, a.O - 1), kc = min(ko, a.K - 1);
    const bool one = ko == a.K;
    const float* xp = kc < a.F1 ? a.x + (size_t)kc : a.x2 + (size_t)(kc - a.F1);
    const size_t xps = kc < a.F1 ? a.x_s : a.x2_s;
    [[maybe_unused]] MlpSplitCol src{};                      // split: the lane's column is one over all its rows
    [[maybe_unused]] unsigned bad = 0;
    if constexpr (mlp_is_split<S>) src = mlp_split_col(a, s, kc);
    // captures by reference, against mlp_ring's rule: by value the compiler moves the address products into the loop (72 registers
    // instead of 120, 3 - 4 % more time at B = 257 .. 658, profiles/mlp_ring_ab.txt); its prologue is short either way
    auto fetch = [&](int d, size_t b0) {                     // lane: unit jz and column ko of every fourth row
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const size_t row = b0 + q + 4 * i, rc = min(row, a.B - 1);
            const bool rin = row < a.B;
            const float z = a.dz[rc * a.dz_s + (size_t)jzc];
            zr[d][i] = rin && jz < a.O ? z : 0.0f;
            float x;
            if constexpr (mlp_is_split<S>) x = mlp_split_x(src, rc, bad);
            else x = xp[rc * xps];
            xr[d][i] = rin && ko <= a.K ? (one ? 1.0f : x) : 0.0f;
        }
    };
    auto stage = [&](int d) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            zs[(q + 4 * i) * BW_PITCH_T + r] = zr[d][i];
            xs[(q + 4 * i) * BW_PITCH_T + r] = xr[d][i];
        }
    };
    auto at = [&](int s) { return (4 * s + q) * BW_PITCH_T + r; };      // A transposed out of LDS: row of the stage = reduction index
    mlp_ring<DEPTH, BW_RC>(a.B, fetch, stage, [&] { mlp_chain16(zs, xs, at, at, acc); });
    if constexpr (mlp_is_split<S>)
        if (bad) s.err[4] = 1;
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

__global__ __launch_bounds__(64) void k_mlp_dw(const MlpDw a)
{
    mlp_dw_tile(a, MlpFlat{}, blockIdx.x, blockIdx.y);
}

// layer 0 of a PTG_MLP_SPLIT_INPUT call: x is the split rows, the operand the flat row they stand for
__global__ __launch_bounds__(64) void k_mlp_dw_split(const MlpDw a, const MlpSplit s)
{
    mlp_dw_tile(a, s, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(64) void k_mlp_dw_group(const MlpGroup<MlpDw> g)
{
    const MlpDw& a = g.net[blockIdx.z];
    if (!a.dw) return;                                       // this network freezes the layer
    if ((int)blockIdx.x * BW_TILE >= a.O || (int)blockIdx.y * BW_TILE > a.K) return;      // column K is the bias gradient
    mlp_dw_tile(a, MlpFlat{}, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(64) void k_mlp_dw_group_split(const MlpGroup<MlpDw> g, const MlpSplit s)
{
    const MlpDw& a = g.net[blockIdx.z];
    if (!a.dw) return;
    if ((int)blockIdx.x * BW_TILE >= a.O || (int)blockIdx.y * BW_TILE > a.K) return;
    mlp_dw_tile(a, s, blockIdx.x, blockIdx.y);
}

template <int ACT>
__device__ __forceinline__ void mlp_dz_out_rows(const MlpDzOut a)
{
    const size_t total = a.B * (size_t)a.O, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const size_t b = i / (size_t)a.O, j = i % (size_t)a.O;
        a.dz[b * a.dz_s + j] = mlp_dact<ACT>(a.h[b * a.h_s + j], a.g[b * a.g_s + j]);
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void k_mlp_dz_out(const MlpDzOut a)
{
    mlp_dz_out_rows<ACT>(a);
}

template <int ACT>
__global__ __launch_bounds__(256) void k_mlp_dz_out_group(const MlpGroup<MlpDzOut> g)      // gridDim.x: the blocks of the largest network; a block beyond a smaller one's elements loops zero times
{
    mlp_dz_out_rows<ACT>(g.net[blockIdx.z]);
}

// what ptg_mlp_backward refuses in a descriptor: false when d is well-formed, else the text in why
bool mlp_bwd_fault(const ptg_env* h, const ptg_mlp_bwd* d, char* why, size_t cap)
{
    const ptg_mlp* f = &d->fwd;
    char fwd[200];
    if (mlp_desc_fault(h, f, fwd, sizeof fwd)) return mlp_fault(why, cap, "the forward's descriptor: %s", fwd);
    if (!(f->flags & PTG_MLP_KEEP_HIDDEN)) return mlp_fault(why, cap, "the forward's descriptor must carry PTG_MLP_KEEP_HIDDEN");
    if (d->flags & ~PTG_MLP_ACCUMULATE) return mlp_fault(why, cap, "unknown flag in %d", d->flags);
    const int n = f->n_layers;
    if (!d->gout_dev || d->gout_s_n < f->width[n - 1]) return mlp_fault(why, cap, "gout_dev is null or gout_s_n below the output width %d", f->width[n - 1]);
    int fan_in = f->f1 + f->f2;
    for (int l = 0; l < n; l++) {
        if ((d->dw_dev[l] != nullptr) != (d->db_dev[l] != nullptr)) return mlp_fault(why, cap, "dw_dev[%d] and db_dev[%d] go together", l, l);
        if (d->dw_dev[l] && d->dw_s_n[l] < fan_in) return mlp_fault(why, cap, "dw_s_n[%d] below the fan-in %d", l, fan_in);
        fan_in = f->width[l];
    }
    if (d->dx_dev && (f->flags & PTG_MLP_SPLIT_INPUT)) return mlp_fault(why, cap, "dx_dev with PTG_MLP_SPLIT_INPUT: an observation has no gradient");
    if (d->dx_dev && d->dx_s_n < f->f1) return mlp_fault(why, cap, "dx_s_n below f1 = %d", f->f1);
    if (d->dx2_dev && f->f2 == 0) return mlp_fault(why, cap, "dx2_dev without a second input piece");
    if (d->dx2_dev && d->dx2_s_n < f->f2) return mlp_fault(why, cap, "dx2_s_n below f2 = %d", f->f2);
    if (!d->bws_dev || (uintptr_t)d->bws_dev % sizeof(float) != 0) return mlp_fault(why, cap, "bws_dev is null or not aligned to 4 bytes");
    const int64_t need = MlpLayout{f->batch, n, f->width}.backward_bytes();
    if (d->bws_bytes < need) return mlp_fault(why, cap, "bws_bytes = %lld, the call needs %lld", (long long)d->bws_bytes, (long long)need);
    return false;
}

// The launch arguments of a backward call, walked from the last layer down: dz_out() (when out_act != NONE), then per layer dw(l) before
// dx(l); dx(l) moves the walk's dz to the layer below
struct MlpBwdWalk {
    const ptg_mlp_bwd* d;
    const float* dz;                     // the gradient at the current layer's pre-activation: grad_out, or a buffer of bws_dev
    size_t dz_s;
    MlpBwdWalk() : d(nullptr), dz(nullptr), dz_s(0) {}
    explicit MlpBwdWalk(const ptg_mlp_bwd* desc) : d(desc), dz(desc->gout_dev), dz_s((size_t)desc->gout_s_n) {}
    MlpLayout lay() const { return MlpLayout{d->fwd.batch, d->fwd.n_layers, d->fwd.width}; }
    float* buf(int l) const { return (float*)d->bws_dev + lay().alt(l, d->fwd.n_layers); }      // dz of layer l, row stride pitch(l)
    int fan_in(int l) const { return l ? d->fwd.width[l - 1] : d->fwd.f1 + d->fwd.f2; }
    const float* input(int l) const { return l ? (const float*)d->fwd.ws_dev + lay().kept(l - 1) : d->fwd.x_dev; }      // the layer's input: hidden layer l - 1, or the call's
    size_t input_s(int l) const { return l ? (size_t)lay().pitch(l - 1) : (size_t)d->fwd.x_s_n; }
    MlpDzOut dz_out()
    {
        const ptg_mlp* f = &d->fwd;
        const int n = f->n_layers;
        const MlpDzOut e{d->gout_dev, (size_t)d->gout_s_n, f->out_dev, (size_t)f->out_s_n, buf(n - 1), (size_t)lay().pitch(n - 1), (size_t)f->batch, f->width[n - 1]};
        dz = e.dz; dz_s = e.dz_s;
        return e;
    }
    MlpDw dw(int l) const                // dw == NULL where the layer is frozen
    {
        const ptg_mlp* f = &d->fwd;
        const float* x = input(l);
        const size_t x_s = input_s(l);
        MlpDw a{};
        a.dz = dz; a.dz_s = dz_s; a.x = x; a.x_s = x_s; a.B = (size_t)f->batch; a.K = fan_in(l); a.O = f->width[l];
        a.x2 = !l && f->x2_dev ? f->x2_dev : x; a.x2_s = !l && f->x2_dev ? (size_t)f->x2_s_n : x_s; a.F1 = l ? a.K : f->f1;
        a.dw = d->dw_dev[l]; a.dw_s = (size_t)d->dw_s_n[l]; a.db = d->db_dev[l]; a.accumulate = (d->flags & PTG_MLP_ACCUMULATE) != 0;
        return a;
    }
    MlpDx dx(int l)
    {
        const ptg_mlp* f = &d->fwd;
        MlpDx a{};
        a.dz = dz; a.dz_s = dz_s; a.w = f->w_dev[l]; a.w_s = (size_t)f->w_s_n[l]; a.B = (size_t)f->batch; a.K = fan_in(l); a.O = f->width[l];
        if (l) {                         // dz of the layer below, through the derivative of the hidden activation on its kept output
            a.h = input(l); a.h_s = input_s(l); a.y = buf(l - 1); a.y_s = a.h_s; a.F1 = a.K;
            dz = a.y; dz_s = a.y_s;
        } else {
            a.y = d->dx_dev; a.y_s = (size_t)d->dx_s_n; a.y2 = d->dx2_dev; a.y2_s = (size_t)d->dx2_s_n; a.F1 = f->f1;
        }
        return a;
    }
};

unsigned mlp_dz_out_blocks(const MlpDzOut& e)
{
    return (unsigned)std::min<size_t>((e.B * (size_t)e.O - 1) / 256 + 1, 65536);
}

dim3 mlp_dw_grid(const MlpDw& a)
{
    return dim3((unsigned)((a.O - 1) / BW_TILE + 1), (unsigned)(a.K / BW_TILE + 1));      // K / 16 + 1, not (K - 1) / 16 + 1: column K is the bias gradient
}

dim3 mlp_dx_grid(const MlpDx& a)
{
    return dim3((unsigned)((a.B - 1) / BW_TILE + 1), (unsigned)((a.K - 1) / BW_TILE + 1));
}

// THE backward, as mlp_forward_walk is the forward: ptg_mlp_backward walks one network with the single kernels, ptg_mlp_group_backward
// up to PTG_MLP_GROUP_MAX with the grouped ones.  One skip rule: dw(l) is launched when any network wants it, dx(0) when any wants dx or dx2
int mlp_backward_walk(ptg_env* h, const char* who, const ptg_mlp_bwd* nets, int n_nets, bool grouped, void* stream)
{
    if (!h) return PTG_E_INVALID;
    if (int rc = mlp_refuse(h, who, nets, n_nets, grouped, [h](const ptg_mlp_bwd* d, char* why, size_t cap) { return mlp_bwd_fault(h, d, why, cap); })) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = as_stream(stream);
    const ptg_mlp* f = &nets[0].fwd;     // depth and activations: the group's
    const int n = f->n_layers;
    MlpSplit s{};
    if (f->flags & PTG_MLP_SPLIT_INPUT) mlp_split_args(h, &s);
    MlpBwdWalk w[PTG_MLP_GROUP_MAX];
    for (int i = 0; i < n_nets; i++) w[i] = MlpBwdWalk{&nets[i]};
    if (f->out_act != PTG_MLP_NONE) {
        MlpGroup<MlpDzOut> g{};
        for (int i = 0; i < n_nets; i++) g.net[i] = w[i].dz_out();
        const dim3 grid = mlp_grid(n_nets, [&](int i) { return dim3(mlp_dz_out_blocks(g.net[i])); });
        mlp_with_act(f->out_act, [&](auto A) {
            constexpr int ACT = decltype(A)::value;
            if (grouped) k_mlp_dz_out_group<ACT><<<grid, 256, 0, st>>>(g);
            else k_mlp_dz_out<ACT><<<grid, 256, 0, st>>>(g.net[0]);
        });
        if (int rc = launch_check(h, grouped ? "k_mlp_dz_out_group" : "k_mlp_dz_out")) return rc;
    }
    for (int l = n - 1; l >= 0; l--) {
        bool any_dw = false, any_dx = l > 0;
        for (int i = 0; i < n_nets; i++) {
            any_dw = any_dw || nets[i].dw_dev[l];
            any_dx = any_dx || nets[i].dx_dev || nets[i].dx2_dev;
        }
        if (any_dw) {                    // a network that freezes the layer rides along with dw == NULL: its workgroups return at once
            MlpGroup<MlpDw> g{};
            for (int i = 0; i < n_nets; i++) g.net[i] = w[i].dw(l);
            const dim3 grid = mlp_grid(n_nets, [&](int i) { return g.net[i].dw ? mlp_dw_grid(g.net[i]) : dim3(); });
            if (l == 0 && (f->flags & PTG_MLP_SPLIT_INPUT)) {
                if (grouped) k_mlp_dw_group_split<<<grid, 64, 0, st>>>(g, s);
                else k_mlp_dw_split<<<grid, 64, 0, st>>>(g.net[0], s);
            } else if (grouped) k_mlp_dw_group<<<grid, 64, 0, st>>>(g);
            else k_mlp_dw<<<grid, 64, 0, st>>>(g.net[0]);
            if (int rc = launch_check(h, grouped ? "k_mlp_dw_group" : "k_mlp_dw")) return rc;
        }
        if (!any_dx) break;
        MlpGroup<MlpDx> g{};             // l = 0: a network without dx_dev and dx2_dev rides along with both NULL
        for (int i = 0; i < n_nets; i++) g.net[i] = w[i].dx(l);
        const dim3 grid = mlp_grid(n_nets, [&](int i) { return l || g.net[i].y || g.net[i].y2 ? mlp_dx_grid(g.net[i]) : dim3(); });
        mlp_with_act(l ? f->hidden_act : PTG_MLP_NONE, [&](auto A) {
            constexpr int ACT_BELOW = decltype(A)::value;
            if (grouped) k_mlp_dx_group<ACT_BELOW><<<grid, 64, 0, st>>>(g);
            else k_mlp_dx<ACT_BELOW><<<grid, 64, 0, st>>>(g.net[0]);
        });
        if (int rc = launch_check(h, grouped ? "k_mlp_dx_group" : "k_mlp_dx")) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t ptg_mlp_backward_workspace(int64_t batch, int32_t n_layers, const int32_t* widths, int32_t flags)
{
    const MlpLayout lay{batch, n_layers, widths};
    return !lay.in_range() || (flags & ~PTG_MLP_ACCUMULATE) ? PTG_E_INVALID : lay.backward_bytes();
}

int ptg_mlp_backward(ptg_env* h, const ptg_mlp_bwd* d, void* stream)
{
    return mlp_backward_walk(h, "ptg_mlp_backward", d, 1, false, stream);
}

int ptg_mlp_group_backward(ptg_env* h, const ptg_mlp_bwd* nets, int32_t n_nets, void* stream)
{
    return mlp_backward_walk(h, "ptg_mlp_group_backward", nets, n_nets, true, stream);
}

}  // extern "C"
