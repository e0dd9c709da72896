// gruw.hip - every weight / bias gradient of the 64-cell fp32 BiGRU in ONE split-K launch (+ one small reduce launch):
//   dW_ih[g][i] = sum_bt dgi[bt][g] input[bt][i],  db_ih[g] = sum_bt dgi[bt][g]
//   dW_hh[g][j] = sum_bt dgh[bt][g] hprev[bt][j],  db_hh[g] = sum_bt dgh[bt][g]
// for both layers and both directions.  gemm.hip's k_gemm_batched served these as four launches per step (two per layer:
// 4 problems x split-K 16, then a reduce); they were the slowest kernels of the step against their bound (0.11 of the fp32
// MFMA rate) and sat in front of the block-1 conv wgrad on the helper stream.  What this kernel does not do:
//   - no second read of dgh's r and z thirds.  k_gru4_bwd (gru4.hip) writes each step's (dr, dz) to BOTH dgi and dgh from the
//     same two registers (v1 / v2 of rows kq = 0, 1: one template, with and without the fused heads phase), so only the n third
//     of dgh differs from dgi.  The tiles {R, Z, N} x input -> dW_ih and {R, Z, Nh} x hprev -> dW_hh take R and Z from dgi.
//   - no LDS operand tiles, no barrier in the K loop.  Every operand is K-major (row = bt, m or n contiguous), which IS the
//     v_mfma_f32_32x32x2_f32 operand layout: lane (n = lane & 31, kh = lane >> 5) needs A[k0 + kh][m0 + n] and
//     B[k0 + kh][n0 + n], coalesced 128-byte runs per load instruction.  A wave owns a 64 x 32 half of a 64 x 64 tile (two
//     32 x 32 accumulators) over its K slice: three dword loads feed two MFMAs, through a register ring one 64-row tile deep.
//   - no per-layer launches: grid = tiles x 4 x 2, 30 tiles at the headline shape (6 per direction for layer 0, 9 for layer 1).
// THE SUMS KEEP k_gemm_batched's ORDER, so the gradients are bit-equal to what its split-K 16 launches gave (and give, for the
// shapes that stay with it): K = B T' is cut into the same SED_GRU_SPLITK = 16 slices of whole 64-row tiles; a slice is one
// sequential chain of MFMAs per accumulator (k pairs in ascending order, rows past the end as zeros); the partials are added as
// k_gemm_reduce adds them, s_j = ((0 + P_j) + P_j+4) + P_j+8) + P_j+12 and then (s_0 + s_1) + (s_2 + s_3).  Workgroup j of a
// tile half holds the four slices j, j + 4, j + 8, j + 12 in its four waves and forms s_j through LDS in wave order;
// k_gru_wgrad_reduce adds the four s_j.  The bias gradients (row sums of A) follow the same rule: per slice and row, the four
// quarter sums over k % 64 / 16 of k_gemm_batched's VALU row sum, combined as (q_0 + q_1) + (q_2 + q_3).
// Every sum therefore has a fixed order that depends on the shapes alone, never on arrival order, stream or position in the step.
// The reduce as a launch of its own and the place at the end of the helper stream were chosen by measurement in the step:
// profiles/gru_wgrad_fused.md.
// Rows past the end of a slice are SELECTED to zero (their address is clamped into the buffer): a poisoned neighbour is NaN.
#include "common.h"
#include "kernels.h"

#define GW_WAVES 4
#define GW_RING 32                    // k-steps (of 2 rows) in flight per wave = one 64-row tile: 96 dword loads per lane
#define GW_TILE_FLOATS (64 * 64 + 64) // one partial: the tile in accumulator order [acc 4][reg / 4][lane 64][4] + 64 row sums of A
static_assert(SED_GRU_SPLITK == 4 * GW_WAVES, "k_gru_wgrad keeps the summation order of k_gemm_batched's split-K 16 + k_gemm_reduce");

__global__ __launch_bounds__(64 * GW_WAVES) void k_gru_wgrad(GruWgradArgs a) {
    __shared__ __attribute__((aligned(16))) float gw_sm[GW_WAVES * 32 * 64 + GW_WAVES * 64];
    f32x4* sm4 = (f32x4*)gw_sm;                        // [src wave][acc 2][reg / 4][lane 64] float4
    float* smb = gw_sm + GW_WAVES * 32 * 64;           // [src wave][64] row sums
    // blockIdx.x = tile * 8 + j * 2 + half: workgroup number % 8 - the XCD - is (j, half), and the tiles that share an operand
    // slice (each A block feeds 2 - 3 tiles, each B block 3) find it in ONE L2
    const int tile = blockIdx.x >> 3, j = (blockIdx.x >> 1) & 3, half = blockIdx.x & 1;
    const GruWgradTile& t = a.t[tile];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 31, kh = lane >> 5;
    // slice j + 4 wv of 16, cut as k_gemm_batched cuts K: whole 64-row tiles
    const int chunk = ((a.BT + SED_GRU_SPLITK - 1) / SED_GRU_SPLITK + 63) / 64 * 64;
    const int kbeg = (int)min((int64_t)a.BT, (int64_t)(j + 4 * wv) * chunk), kend = min(a.BT, kbeg + chunk), last = a.BT - 1;
    const bool do_bias = half == 0 && t.bias != nullptr;       // the first column half also sums the rows of A
    const float* A = t.A + n;
    const float* B = t.B + 32 * half + n;
    const size_t lda = t.lda, ldb = t.ldb;

    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    float rq[4] = {0.f, 0.f, 0.f, 0.f};                // row lane of A: the sums over k % 64 / 16 = 0 .. 3
    float ra0[GW_RING], ra1[GW_RING], rb[GW_RING];
    // raw loads only: the select to zero happens where the value is consumed, so that no load is waited for here.  The empty
    // asm pins each load where it is written: without it the compiler sinks the ring's loads to their uses, one trip later,
    // and the loop becomes load - wait - MFMA with nothing in flight (seen in the ISA: s_waitcnt vmcnt(0) per k-step)
    auto load = [&](int i, int krow) {
        const size_t k = (size_t)min(krow + kh, last);
        ra0[i] = A[k * lda]; ra1[i] = A[k * lda + 32];
        rb[i] = B[k * ldb];
        asm volatile("" ::: "memory");
    };
    if (kbeg < kend) {
#pragma unroll
        for (int i = 0; i < GW_RING; ++i) load(i, kbeg + 2 * i);
    }
    for (int k0 = kbeg; k0 < kend; k0 += 64) {
#pragma unroll
        for (int i = 0; i < GW_RING; ++i) {
            const bool ok = k0 + 2 * i + kh < kend;
            const float a0 = ok ? ra0[i] : 0.f, a1 = ok ? ra1[i] : 0.f, b = ok ? rb[i] : 0.f;
            acc[0] = mfma32(a0, b, acc[0]);
            acc[1] = mfma32(a1, b, acc[1]);
            if (do_bias) {
                // lane (n, kh) holds rows n and 32 + n of A at k0 + 2 i + kh; row `lane` needs both k, the even one first
                const float p0 = __shfl_xor(a0, 32), p1 = __shfl_xor(a1, 32);
                rq[i >> 3] += kh ? p1 : a0;
                rq[i >> 3] += kh ? a1 : p0;
            }
            load(i, k0 + 64 + 2 * i);
        }
    }
    // ---- s_j: the four waves' slices, added in wave order; the 8 float4 groups (accumulator q, registers 4 r4 ..) of a lane are
    // dealt to the waves, GW_GROUPS consecutive ones each
    constexpr int GW_GROUPS = 8 / GW_WAVES;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 v = {acc[q][4 * r4], acc[q][4 * r4 + 1], acc[q][4 * r4 + 2], acc[q][4 * r4 + 3]};
            sm4[(wv * 8 + q * 4 + r4) * 64 + lane] = v;
        }
    smb[wv * 64 + lane] = (rq[0] + rq[1]) + (rq[2] + rq[3]);
    __syncthreads();
    float* part = a.part + ((size_t)tile * 4 + j) * GW_TILE_FLOATS;
#pragma unroll
    for (int jj = 0; jj < GW_GROUPS; ++jj) {
        const int g = wv * GW_GROUPS + jj;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < GW_WAVES; ++w) v += sm4[(w * 8 + g) * 64 + lane];
        ((f32x4*)part)[((2 * (g >> 2) + half) * 4 + (g & 3)) * 64 + lane] = v;      // accumulator 2 (row half) + column half
    }
    if (wv == 0 && do_bias) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < GW_WAVES; ++w) v += smb[w * 64 + lane];
        part[64 * 64 + lane] = v;
    }
}

// C = (s_0 + s_1) + (s_2 + s_3) of a tile's four partials; grid = tiles x 4 (one accumulator each), 256 threads
__global__ __launch_bounds__(256) void k_gru_wgrad_reduce(GruWgradArgs a) {
    const int tile = blockIdx.x >> 2, q = blockIdx.x & 3;
    const GruWgradTile& t = a.t[tile];
    const int lane = threadIdx.x & 63, r4 = threadIdx.x >> 6;
    const float* part = a.part + (size_t)tile * 4 * GW_TILE_FLOATS;
    const f32x4* p4 = (const f32x4*)part + (q * 4 + r4) * 64 + lane;
    constexpr int S = GW_TILE_FLOATS / 4;
    f32x4 v = (p4[0] + p4[S]) + (p4[2 * S] + p4[3 * S]);
    v += 0.f;                                          // (k_gemm_reduce's absent bias: -0 becomes +0)
    const int col = 32 * (q & 1) + (lane & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) t.C[(size_t)(32 * (q >> 1) + mfma32_row(4 * r4 + e, lane)) * t.ldc + col] = v[e];
    if (q == 0 && threadIdx.x < 64 && t.bias != nullptr) {
        const float* pb = part + 64 * 64 + threadIdx.x;
        t.bias[threadIdx.x] = (pb[0] + pb[GW_TILE_FLOATS]) + (pb[2 * GW_TILE_FLOATS] + pb[3 * GW_TILE_FLOATS]);
    }
}

size_t gru_wgrad_part_floats(int n_tiles) { return (size_t)n_tiles * 4 * GW_TILE_FLOATS; }

int launch_gru_wgrad(const GruWgradLayer* layers, int n_layers, int BT, float* part, size_t part_floats, hipStream_t st) {
    SED_CHECK_ARG(layers && n_layers >= 1 && n_layers <= 2 && BT >= 1 && part, "gru_wgrad: bad argument");
    GruWgradArgs a;
    a.BT = BT; a.part = part; a.n_tiles = 0;
    for (int l = 0; l < n_layers; ++l) {
        const GruWgradLayer& L = layers[l];
        SED_CHECK_ARG(L.nin == 64 || L.nin == 128, "gru_wgrad: the layer input has 64 or 128 columns");
        const int nb = L.nin / 64;
        for (int dir = 0; dir < 2; ++dir) {
            const float* dgi = L.dgi + dir * 192;
            for (int ab = 0; ab < 3; ++ab)           // {R, Z, N} x input blocks -> dW_ih; the first column block carries db_ih
                for (int cb = 0; cb < nb; ++cb)
                    a.t[a.n_tiles++] = GruWgradTile{dgi + 64 * ab, L.input + 64 * cb, L.w_ih[dir] + (size_t)64 * ab * L.nin + 64 * cb,
                                                    cb == 0 ? L.b_ih[dir] + 64 * ab : nullptr, 384, L.nin, L.nin};
            for (int ab = 0; ab < 3; ++ab)           // {R, Z, Nh} x hprev -> dW_hh, db_hh
                a.t[a.n_tiles++] = GruWgradTile{ab < 2 ? dgi + 64 * ab : L.dgh + dir * 192 + 128, L.hprev + dir * 64,
                                                L.w_hh[dir] + (size_t)64 * ab * 64, L.b_hh[dir] + 64 * ab, 384, 128, 64};
        }
    }
    if (gru_wgrad_part_floats(a.n_tiles) > part_floats) {
        sed_set_error("gru_wgrad: partial buffer holds %zu floats, %d tiles need %zu", part_floats, a.n_tiles, gru_wgrad_part_floats(a.n_tiles));
        return SED_ERR_WORKSPACE;
    }
    k_gru_wgrad<<<a.n_tiles * 8, 64 * GW_WAVES, 0, st>>>(a);
    SED_CHECK_LAUNCH();
    k_gru_wgrad_reduce<<<a.n_tiles * 4, 256, 0, st>>>(a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
