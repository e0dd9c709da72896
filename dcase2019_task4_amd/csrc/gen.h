// gen.h - building blocks shared by the GENERIC kernel set (gconv.hip, gglu.hip, bconv.hip, bglu.hip, blk0.hip, grec.hip,
// ggemm.hip, gcrnn.hip): any conv width C in {64, 128}, any GRU width H that is a multiple of 64 up to 256.  The C = 64 / H = 64
// / fp32 configuration of baseline/config.py:53-58 keeps its own specialised kernels (conv.hip, bnglu.hip, gru4.hip).
//
// Two things live here:
//   - the storage helpers every member of the set uses: fp32 / bf16 / fp16 loads and stores of the conv-block activations
//     (ld1 / ld4 / st1, Stor<>, H16<>), the dropout keep bits (gen_keep16) and the pooled-pixel index (gen_rb_pixel);
//   - stream_gemm, the fp32 GEMM loop of gconv.hip (forward / dgrad) and gglu.hip: exact-fp32 products on
//     v_mfma_f32_32x32x2_f32.  The bf16-operand kernels (bconv.hip, bglu.hip, grec.hip) have loops of their own.
//
// Shape of the fp32 GEMM: C[m][n] += sum_k A[m][k] B[n][k] with BOTH operands k-contiguous - what channels-last activations
// and [out][in] weights give for free.  A lives in an LDS tile owned by the workgroup (a halo tile of the image, a row block of
// pixels); B (weights, packed once per forward by k_gen_pack) streams from L2 through a double-buffered LDS chunk.
#pragma once
#include "common.h"
#include "philox.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// ---- storage of the conv-block activations / gradients in HBM: fp32, or bf16 in SED_DTYPE_BF16 mode ----------------------
// (p0, y1, p1, y2 in ctx; dz1, dz2, dp0, dp1 in the backward workspace.  p2 - the GRU input - and dp2 stay fp32.)
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 ld4(const __bf16* p) {
    const bf16x4 v = *(const bf16x4*)p;
    return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const __bf16* p) { return (float)*p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(__bf16* p, float v) { *p = (__bf16)v; }
template <int BF> struct Stor { using T = float; };
template <> struct Stor<1> { using T = __bf16; };

// ---- SED_DTYPE_F16: the forward chain's 16-bit flavour.  H16<0> = bf16 (the bf16 mode), H16<1> = fp16. ----------------------
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
__device__ __forceinline__ f32x4 ld4(const _Float16* p) {
    const f16x4 v = *(const f16x4*)p;
    return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ float ld1(const _Float16* p) { return (float)*p; }
// fp16 stores SATURATE at +-65504: a value beyond fp16's range (none of the forward tensors of this model comes near it - they sit
// behind BatchNorms or are convolutions of O(1) inputs - but nothing in the arithmetic forbids conv weights from drifting there
// over a long run) becomes the largest finite fp16, which the BatchNorm behind it absorbs, instead of an Inf that turns the step
// into NaNs
__device__ __forceinline__ _Float16 f16_sat(float v) { return (_Float16)__builtin_fminf(__builtin_fmaxf(v, -65504.0f), 65504.0f); }
__device__ __forceinline__ void st1(_Float16* p, float v) { *p = f16_sat(v); }
template <int F16> struct H16 {
    using T = __bf16;
    using V8 = bf16x8;
    static __device__ __forceinline__ f32x16 mma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct H16<1> {
    using T = _Float16;
    using V8 = f16x8;
    static __device__ __forceinline__ f32x16 mma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// ---- the fp32 GEMM loop: B operand streamed through LDS ------------------------------------------------------------------
// LDS rows of fp32 MFMA operands are padded by one word: an odd stride, so that lane = row reads hit 32 distinct banks
constexpr int GEN_PAD = 1;
constexpr int GEN_KC = 32;              // default k-chunk of the streamed B operand
// four consecutive floats into such a row (odd word stride: no wider store is aligned)
__device__ __forceinline__ void gen_st4(float* p, f32x4 v) { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }

// acc[nb][.] += sum_{k < K} A(row of this lane, k) * Bg[(nb0 + nb) * 32 + (lane & 31)][k],  nb < NBW
//   Bg     global, row-major [32 * NBT][ldb] (k contiguous), 16-byte aligned rows; ALL 32 * NBT rows are staged (the waves of
//          a workgroup may each take a different slice nb0 .. nb0 + NBW of them)
//   a_row  per-lane LDS pointer to the first k of this lane's A row; the A elements of chunk ch start at a_row + aoff(ch)
//          (a functor: the 3x3 convolution moves to another halo pixel every C / KC chunks)
//   wbuf   LDS, 2 x [32 * NBT][KC + GEN_PAD] floats; every thread of the 256-thread workgroup must call (staging + barriers:
//          one barrier before the first MFMA - so LDS tiles written before the call are visible to all waves - and one
//          after the last, so they may be overwritten right after the call)
template <int NBT, int NBW, int KC, class AOff>
__device__ __forceinline__ void stream_gemm(const float* a_row, AOff aoff, const float* __restrict__ Bg, int ldb, int K, float* wbuf,
                                            f32x16 (&acc)[NBW], int nb0, int tid) {
    constexpr int N = 32 * NBT, WS = KC + GEN_PAD;
    constexpr int VPR = KC / 4;                              // 16-byte vectors per row
    constexpr int NV = N * VPR / 256;                        // vectors per thread per chunk
    static_assert(N * VPR % 256 == 0 && NV >= 1, "chunk must divide over 256 threads");
    const int lane = tid & 63, kh = lane >> 5, n = lane & 31;
    const int nch = K / KC;
    f32x4 st[NV];
    auto load = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int u = tid + 256 * i, row = u / VPR, cv = u % VPR;
            // (16-byte vector cv of the row, addressed in bytes: `+ 4 * cv` floats is the same address, but the kernels come
            // out in a different instruction order)
            st[i] = *(const f32x4*)((const char*)(Bg + (size_t)row * ldb + (size_t)ch * KC) + 16 * cv);
        }
    };
    auto store = [&](int buf) {
        float* wb = wbuf + buf * N * WS;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int u = tid + 256 * i, row = u / VPR, cv = u % VPR;
            gen_st4(wb + row * WS + cv * 4, st[i]);
        }
    };
    load(0);
    store(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        if (ch + 1 < nch) load(ch + 1);
        const float* ap = a_row + aoff(ch) + kh;            // 32x32x2: lane (n, kh) supplies k = 2 ks + kh
        const float* bp = wbuf + (ch & 1) * N * WS + (nb0 * 32 + n) * WS + kh;
#pragma unroll
        for (int ks = 0; ks < KC / 2; ++ks) {
            const float a = ap[2 * ks];
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) acc[nb] = mfma32(a, bp[nb * 32 * WS + 2 * ks], acc[nb]);
        }
        if (ch + 1 < nch) store((ch + 1) & 1);
        __syncthreads();
    }
}

// ---- dropout keep bits of one (row block, 32-channel slice) unit, generic in C ---------------------------------------
// unit u = rb * (C / 32) + nb.  p == 0.5: ONE Philox draw (index (u >> 3) * 64 + lane, stream 32 + block) carries the
// 16-bit fields of 8 consecutive units - for C = 64 this is exactly the stream of the specialised kernels (philox.h).
// Other rates: the 8-bit stream, one draw per (row block, channel, dt) as in philox.h.  Mirrored by oracle/philox.py.
__device__ __forceinline__ uint32_t gen_keep16(int rb, int nb, int C, int lane, int block, uint64_t seed, uint32_t thr) {
    if (thr == 128u) {
        const uint32_t u = (uint32_t)rb * (uint32_t)(C >> 5) + (uint32_t)nb;
        const u32x4 o = philox_stream((u >> 3) * 64u + (uint32_t)lane, PHILOX_STREAM_1BIT + (uint32_t)block, seed);
        return philox_field16(o, (int)(u & 7u));
    }
    const int c = 32 * nb + (lane & 31);
    return philox_keep16(philox_stream((uint32_t)(rb * C + c), (uint32_t)(2 * block + (lane >> 5)), seed), thr);
}

// pixel index (into [B][H][W]) of pooled pixel q at (dt, df); Ho = H / 2, Wo = W / 4
__device__ __forceinline__ int gen_rb_pixel(int q, int dt, int df, int H, int W, int Ho, int Wo) {
    const int wo = q % Wo, t = q / Wo;
    const int ho = t % Ho, b = t / Ho;
    return (b * H + 2 * ho + dt) * W + 4 * wo + df;
}
