// augment.hip - train-time batch augmentation on the device: mixup of features and targets, a circular time shift of
// features and strong targets, and SpecAugment-style time / frequency masks (sed_batch_augment; the definitions are in
// include/dcase_sed.h and are the project's own - the reference has no such code).
//
// k_batch_augment: one launch for the features, the teacher's noisy copy and the targets.  blockIdx.z selects the tensor,
// blockIdx.y the clip, blockIdx.x a tile of rows (time steps) of that clip.  Everything that depends on the clip alone -
// its table row, the partner's shift, both shifts reduced to [0, n), the clipped mask intervals - depends only on the block
// index, so the compiler keeps it in SGPRs; a thread owns one row and walks its columns, so the time roll costs one
// compare-and-add per row and no integer division per element.  Rows along m stay contiguous under the roll: 16-byte
// loads / stores when the row width is a multiple of 4 and the bases are 16-byte aligned, one float per lane otherwise.
// Pure element-wise traffic: no LDS, no atomics, no allocation; every product, sum and 1 - lambda is an individually
// rounded fp32 operation (no FMA contraction), so a numpy float32 statement agrees bit for bit.
#pragma clang fp contract(off)       // file-wide: it also covers common.h's inline helpers and anything added to this file later
#include "common.h"

// The individually rounded operations are plain operators compiled HERE, under the pragma above.  HIP's __fmul_rn /
// __fadd_rn / __fsub_rn are no help: their bodies live in the runtime header the compiler driver includes in front of this
// file's first line, so they are compiled under the default contraction mode, and once inlined the back end fused
// lambda * a + (1 - lambda) * p into v_pk_fma_f32 (seen in this kernel's ISA).
__device__ __forceinline__ float aug_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float aug_add(float a, float b) { return a + b; }
__device__ __forceinline__ float aug_sub(float a, float b) { return a - b; }

#define AUG_THREADS 256

struct AugTensor {
    const float* in;
    float* out;
    int n, w;          // rows (time steps) per clip, floats per row
    int lgx;           // log2 of the lanes that share one row
    int vec;           // 1: float4 columns (w % 4 == 0, bases 16-byte aligned)
    int feat;          // 1: features (shift_x, masks); 0: targets (shift_y, never masked)
};
struct AugArgs {
    AugTensor t[3];
    const int32_t* table;     // [B][8]: partner, lambda bits, shift_x, shift_y, f0, fw, t0, tw
    int B;
};

// ((s mod n) + n) mod n for any int32 s, n >= 1
__device__ __forceinline__ int aug_wrap(int s, int n) {
    const int m = s % n;
    return m < 0 ? m + n : m;
}
// [lo, lo + width) clipped to [0, n); width <= 0: empty
__device__ __forceinline__ void aug_interval(int lo, int width, int n, int& a, int& b) {
    const long long hi = (long long)lo + (width > 0 ? width : 0);
    a = lo < 0 ? 0 : (lo > n ? n : lo);
    b = hi < a ? a : (hi > n ? n : (int)hi);
}

template <bool VEC>
__device__ __forceinline__ void aug_row(const AugTensor& q, const float* __restrict__ own, const float* __restrict__ other,
                                        float* __restrict__ dst, bool mixing, float lam, float om, bool zero_row, int flo, int fhi,
                                        int lx) {
    const int step = 1 << q.lgx;
    if (VEC) {
        const int wv = q.w >> 2;
        for (int c = lx; c < wv; c += step) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!zero_row) {
                v = *(const f32x4*)(own + 4 * c);
                if (mixing) {
                    const f32x4 p = *(const f32x4*)(other + 4 * c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = aug_add(aug_mul(lam, v[j]), aug_mul(om, p[j]));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c + j >= flo && 4 * c + j < fhi) v[j] = 0.0f;
            }
            *(f32x4*)(dst + 4 * c) = v;
        }
    } else {
        for (int c = lx; c < q.w; c += step) {
            float v = 0.0f;
            if (!zero_row && !(c >= flo && c < fhi)) {
                v = own[c];
                if (mixing) v = aug_add(aug_mul(lam, v), aug_mul(om, other[c]));
            }
            dst[c] = v;
        }
    }
}

__global__ __launch_bounds__(AUG_THREADS) void k_batch_augment(AugArgs a) {
    const AugTensor q = a.t[blockIdx.z];
    const int b = blockIdx.y;
    const int lx = threadIdx.x & ((1 << q.lgx) - 1);
    const int row = blockIdx.x * (AUG_THREADS >> q.lgx) + (threadIdx.x >> q.lgx);
    if (row >= q.n) return;
    // ---- per-clip scalars ---------------------------------------------------------------------------------------------------
    const int32_t* pr = a.table + (size_t)b * 8;
    const int p = min(max(pr[0], 0), a.B - 1);              // no table content can address outside the batch
    const float lam = __int_as_float(pr[1]);
    const bool mixing = p != b && lam != 1.0f;               // otherwise the partner is not read at all
    const float om = aug_sub(1.0f, lam);
    const int col = q.feat ? 2 : 3;
    const int s_own = aug_wrap(pr[col], q.n);
    const int s_oth = aug_wrap(a.table[(size_t)p * 8 + col], q.n);
    int flo = 0, fhi = 0, tlo = 0, thi = 0;
    if (q.feat) {
        aug_interval(pr[4], pr[5], q.w, flo, fhi);
        aug_interval(pr[6], pr[7], q.n, tlo, thi);
    }
    // ---- this thread's row ---------------------------------------------------------------------------------------------------
    int ra = row - s_own, rb = row - s_oth;                   // r(t - s, n): both shifts are in [0, n)
    if (ra < 0) ra += q.n;
    if (rb < 0) rb += q.n;
    const size_t clip = (size_t)q.n * q.w;
    const float* own = q.in + (size_t)b * clip + (size_t)ra * q.w;
    const float* other = q.in + (size_t)p * clip + (size_t)rb * q.w;
    float* dst = q.out + (size_t)b * clip + (size_t)row * q.w;
    const bool zero_row = row >= tlo && row < thi;
    if (q.vec) aug_row<true>(q, own, other, dst, mixing, lam, om, zero_row, flo, fhi, lx);
    else aug_row<false>(q, own, other, dst, mixing, lam, om, zero_row, flo, fhi, lx);
}

static bool aug_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

extern "C" int sed_batch_augment(const float* x, const float* x_ema, const float* target, const int32_t* table, int B, int T,
                                 int M, int T3, int NC, float* out_x, float* out_x_ema, float* out_target, void* stream) {
    SED_CHECK_ARG(x && out_x && table, "sed_batch_augment: null argument");
    SED_CHECK_ARG((x_ema == nullptr) == (out_x_ema == nullptr), "sed_batch_augment: x_ema and out_x_ema go together");
    SED_CHECK_ARG((target == nullptr) == (out_target == nullptr), "sed_batch_augment: target and out_target go together");
    SED_CHECK_ARG(B >= 1 && B <= 65535 && T >= 1 && M >= 1, "sed_batch_augment: need 1 <= B <= 65535, T >= 1 and M >= 1");
    SED_CHECK_ARG((long long)T * M < (1ll << 31), "sed_batch_augment: a clip of T x M floats must stay below 2^31");
    if (target) {
        SED_CHECK_ARG(T3 >= 1 && NC >= 1, "sed_batch_augment: need T3 >= 1 and NC >= 1 with targets");
        SED_CHECK_ARG((long long)T3 * NC < (1ll << 31), "sed_batch_augment: a target of T3 x NC floats must stay below 2^31");
    }
    const size_t fb = (size_t)B * T * M * sizeof(float), gb = target ? (size_t)B * T3 * NC * sizeof(float) : 0;
    const size_t pb = (size_t)B * 8 * sizeof(int32_t);
    const void* ins[4] = {x, x_ema, target, table};
    const size_t in_bytes[4] = {fb, fb, gb, pb};
    const void* outs[3] = {out_x, out_x_ema, out_target};
    const size_t out_bytes[3] = {fb, fb, gb};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i)
            SED_CHECK_ARG(!aug_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "sed_batch_augment: an output overlaps an input");
        for (int o2 = o + 1; o2 < 3; ++o2)
            SED_CHECK_ARG(!aug_overlap(outs[o], out_bytes[o], outs[o2], out_bytes[o2]), "sed_batch_augment: two outputs overlap");
    }
    AugArgs a = {};
    a.table = table;
    a.B = B;
    int nt = 0, gx = 1;
    auto add = [&](const float* in, float* out, int n, int w, int feat) {
        AugTensor& q = a.t[nt++];
        q.in = in; q.out = out; q.n = n; q.w = w; q.feat = feat;
        q.vec = w % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0;
        const int cols = q.vec ? w / 4 : w;
        q.lgx = 0;
        while (q.lgx < 6 && (1 << q.lgx) < cols) ++q.lgx;          // up to one wave per row
        const int rows = AUG_THREADS >> q.lgx;
        gx = max(gx, (n + rows - 1) / rows);
    };
    add(x, out_x, T, M, 1);
    if (x_ema) add(x_ema, out_x_ema, T, M, 1);
    if (target) add(target, out_target, T3, NC, 0);
    // (tiles of the shorter tensor's z-slice that lie past its last row return at once)
    hipLaunchKernelGGL(k_batch_augment, dim3(gx, B, nt), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
