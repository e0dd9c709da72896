// bnglu.hip - BatchNorm-apply + GLU + dropout + AvgPool2d((2,4)) fused, forward and backward,
// for conv blocks 1 and 2.
//
// Reference ops (baseline/models/CNN.py:49-67, GLU CNN.py:11-16):
//   z = BatchNorm2d(y);  lin = Linear(64,64)(z over channels);  out = lin * sigmoid(z)
//   p = AvgPool2d((2,4))(Dropout(out))
//
// One wave owns a "row block" = 4 consecutive pooled pixels = 32 input pixels, ordered so that
// the 32x32x2 MFMA's D fragment leaves a whole 2x4 pooling window inside a lane pair: MFMA row
// m <-> pooled pixel j = m>>3, dt = (m>>2)&1, df = m&3; D register r of lane l holds
// (j = r>>2, dt = l>>5, df = r&3), so pooling is 3 adds in-lane plus one cross-half add.
// The GLU weight (64x64) lives in registers as MFMA B fragments for the whole kernel; the BN
// affine is applied while the y tile is staged into LDS (65-float pixel stride: conflict-free
// for lane = pixel A-fragment reads and for lane = channel epilogue reads).
//
// Backward recomputes z, lin and the dropout mask (Philox, no stored masks), then
//   dlin = g*sig(z);  dz = dlin @ Wglu + g*lin*sig'(z);  dWglu += dlin^T z   (all on the MFMA)
// and accumulates the BatchNorm-backward sums (sum dz, sum dz*y) so that the conv dgrad / wgrad
// kernels can form dy = ca*dz + cb*y + cc on the fly (conv.hip).
#include "common.h"
#include "philox.h"
#include "kernels.h"
#include <type_traits>

#define ZS 65   // pixel stride of LDS tiles (floats)

SED_TS_DEFINE(bnglu)

struct BnPrepArgs {
    const double* stat; double N;
    const float *gamma, *beta;
    float *run_mean, *run_var; int64_t* tracked;
    int train, update; float eps, momentum;
    float* bn;
};

// pixel index (into [B][H][W]) of MFMA row m of the row block starting at pooled pixel q0
__device__ __forceinline__ int rb_pixel(int q, int dt, int df, int H, int W, int Ho, int Wo) {
    const int wo = q % Wo, t = q / Wo;
    const int ho = t % Ho, b = t / Ho;
    return (b * H + 2 * ho + dt) * W + 4 * wo + df;
}

// A row block's conv output y (32 pixels x 64 channels) goes global -> registers -> LDS in two separately
// callable halves, so that the loads of row block k+1 are issued BEFORE the MFMAs of row block k: these kernels
// run one or two waves per SIMD, and a load consumed right after its issue exposes a full memory round trip
// (~2 us per row block in the first version; MFMA pipe busy 21 % in round 1's GLU backward).
struct YTile { float4 v[8]; };
__device__ __forceinline__ void tile_load(YTile& t, const float* __restrict__ y, int q0, int Q, int H, int W, int Ho,
                                          int Wo, int lane) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int m = (lane >> 4) + 4 * it, c4 = (lane & 15) * 4;
        // rows past the last pooled pixel read the last pixel's window instead of sitting under a branch (a branch per
        // load, each with a wait of its own); tile_store never uses what they hold
        const int q = min(q0 + (m >> 3), Q - 1);
        const int pix = rb_pixel(q, (m >> 2) & 1, m & 3, H, W, Ho, Wo);
        t.v[it] = *(const float4*)(y + (size_t)pix * 64 + c4);
    }
}
template <bool KEEP_Y>
__device__ __forceinline__ void tile_store(const YTile& t, const float4& sc, const float4& sh, float* zt, float* yt,
                                           int q0, int Q, int lane) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int m = (lane >> 4) + 4 * it, c4 = (lane & 15) * 4;
        float4 v = t.v[it];
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + (m >> 3) >= Q) v = make_float4(0.f, 0.f, 0.f, 0.f);
        else {
            z.x = fmaf(v.x, sc.x, sh.x); z.y = fmaf(v.y, sc.y, sh.y);
            z.z = fmaf(v.z, sc.z, sh.z); z.w = fmaf(v.w, sc.w, sh.w);
        }
        float* d = zt + m * ZS + c4;
        d[0] = z.x; d[1] = z.y; d[2] = z.z; d[3] = z.w;
        if (KEEP_Y) {
            float* e = yt + m * ZS + c4;
            e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        }
    }
}

// The BatchNorm statistics -> (mean, invstd, scale, shift) step of k_bn_prep runs in the prologue of every workgroup
// (64 threads, a few fp64 operations) instead of as a 1-workgroup kernel of its own in front: one launch and one
// dependency gap less on the forward chain per conv block.  Workgroup 0 also publishes bn[] for the backward and
// updates the running statistics.
// In two halves: bn_prep_load only REQUESTS the operands (every branch in it is uniform over the launch or the workgroup, and nothing
// in it waits), so that the caller can put its other prologue loads into the same round trip; bn_prep_body does the arithmetic.
struct BnPrepOperands { double s0, s1; float rm, rv, gamma, beta; };
__device__ __forceinline__ BnPrepOperands bn_prep_load(const BnPrepArgs& a, int c, bool publish) {
    BnPrepOperands o = {0.0, 0.0, 0.f, 0.f, a.gamma[c], a.beta[c]};
    if (a.train) { o.s0 = a.stat[c]; o.s1 = a.stat[64 + c]; }
    if (!a.train || (a.update && publish)) { o.rm = a.run_mean[c]; o.rv = a.run_var[c]; }
    return o;
}
__device__ __forceinline__ void bn_prep_body(const BnPrepArgs& a, const BnPrepOperands& o, int c, bool publish, float* bn_s /* LDS [256] */) {
    double mean, var;
    if (a.train) {
        mean = o.s0 / a.N;
        var = o.s1 / a.N - mean * mean;
        if (var < 0) var = 0;
        if (a.update && publish) {
            a.run_mean[c] = (float)((1.0 - a.momentum) * o.rm + a.momentum * mean);
            a.run_var[c] = (float)((1.0 - a.momentum) * o.rv + a.momentum * var * a.N / (a.N - 1.0));
            if (c == 0 && a.tracked) a.tracked[0] += 1;
        }
    } else {
        mean = o.rm;
        var = o.rv;
    }
    const double invstd = 1.0 / sqrt(var + (double)a.eps);
    const double scale = o.gamma * invstd;
    const float v0 = (float)mean, v1 = (float)invstd, v2 = (float)scale, v3 = (float)(o.beta - mean * scale);
    bn_s[c] = v0; bn_s[64 + c] = v1; bn_s[128 + c] = v2; bn_s[192 + c] = v3;
    if (publish) { a.bn[c] = v0; a.bn[64 + c] = v1; a.bn[128 + c] = v2; a.bn[192 + c] = v3; }
}

__global__ __launch_bounds__(256, 2) void k_glu_pool_fwd(const float* __restrict__ y, BnPrepArgs bnp,
                                                       const float* __restrict__ wglu, const float* __restrict__ bglu,
                                                       float* __restrict__ p, int H, int W, int Ho, int Wo, int Q,
                                                       int block_id, int use_drop, float p_drop,
                                                       const uint64_t* __restrict__ seed_ptr, uint16_t* __restrict__ mask_out) {
    __shared__ float zts[4][32 * ZS];
    __shared__ float WsT[64 * ZS];     // Wglu transposed [c][co], stride 65: coalesced global read, conflict-free both ways
    __shared__ __attribute__((aligned(16))) float bn_s[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = lane & 31, kh = lane >> 5;
    float* zt = zts[wv];
    // One round trip for the whole prologue: the BatchNorm operands (wave 0, requested first so that its fp64 arithmetic
    // starts while the rest is in flight), bglu, the seed, Wglu (four float4 per thread) and the first y tile are all
    // requested before anything waits.  (Before: the BN operands in four dependent groups with every other wave at the
    // barrier, Wglu dword by dword with a wait per trip, bglu and the y tile only behind the barrier - 15 drain points.)
    const int n_rb = (Q + 3) / 4;
    BnPrepOperands bno = {};
    if (tid < 64) bno = bn_prep_load(bnp, tid, blockIdx.x == 0);
    const float bg[2] = {bglu[n], bglu[32 + n]};
    const uint64_t seed = use_drop ? seed_ptr[0] : 0ull;
    float4 wq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wq[i] = ((const float4*)wglu)[tid + 256 * i];
    YTile yt_n;
    if (blockIdx.x * 4 + wv < n_rb) tile_load(yt_n, y, (blockIdx.x * 4 + wv) * 4, Q, H, W, Ho, Wo, lane);
    // (the empty asm keeps wave 0's arithmetic - and its wait - behind the requests above: the compiler had merged the two
    // `tid < 64` blocks in front of them)
    asm volatile("" : "+v"(bno.s0), "+v"(bno.s1), "+v"(bno.rm), "+v"(bno.rv), "+v"(bno.gamma), "+v"(bno.beta));
    if (tid < 64) bn_prep_body(bnp, bno, tid, blockIdx.x == 0, bn_s);
    const float* bn = bn_s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = 4 * (tid + 256 * i);                // Wglu[co = e >> 6][c = e & 63 .. + 3]
        float* d = &WsT[(e & 63) * ZS + (e >> 6)];
        d[0] = wq[i].x; d[ZS] = wq[i].y; d[2 * ZS] = wq[i].z; d[3 * ZS] = wq[i].w;
    }
    __syncthreads();
    float bw[32][2];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        bw[s][0] = WsT[(2 * s + kh) * ZS + n];            // B[k = c][j = co] = Wglu[co][c]
        bw[s][1] = WsT[(2 * s + kh) * ZS + 32 + n];
    }
    const uint32_t thr = drop_thresh8(p_drop);
    const bool one_bit = (thr == 128u);
    const float sc = 0.125f * (use_drop ? drop_scale8(p_drop) : 1.0f);
    const float4 bsc = *(const float4*)(bn + 128 + (lane & 15) * 4), bsh = *(const float4*)(bn + 192 + (lane & 15) * 4);
    for (int rb = blockIdx.x * 4 + wv; rb < n_rb; rb += gridDim.x * 4) {
        const int q0 = rb * 4;
        tile_store<false>(yt_n, bsc, bsh, zt, nullptr, q0, Q, lane);
        {
            const int rbn = rb + gridDim.x * 4;
            if (rbn < n_rb) tile_load(yt_n, y, rbn * 4, Q, H, W, Ho, Wo, lane);
        }
        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
        const float* A = zt + n * ZS + kh;
        // A operands two k-steps (four MFMAs) AHEAD, in rotating registers: written as `a = A[2 s]; mfma; mfma` the compiler
        // issued each ds_read right in front of the MFMAs that need it and the wave sat out one LDS latency per k-step pair
        // (ds_read2_b32 | s_waitcnt lgkmcnt(0) | 4 MFMAs, sixteen times per row block)
        float av[4];
        av[0] = A[0]; av[1] = A[2];
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            if (s + 2 < 32) av[(s + 2) & 3] = A[2 * (s + 2)];
            acc[0] = mfma32(av[s & 3], bw[s][0], acc[0]);
            acc[1] = mfma32(av[s & 3], bw[s][1], acc[1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        u32x4 o1 = {0u, 0u, 0u, 0u};
        if (use_drop && one_bit) o1 = philox_stream_1bit((uint32_t)rb, lane, block_id, seed);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = 32 * h + n;
            float pooled[4] = {0.f, 0.f, 0.f, 0.f};
            uint32_t m16 = 0xffffu;
            if (use_drop) {
                if (one_bit) {
                    m16 = philox_field16(o1, 2 * (rb & 3) + h);
                } else {
                    const u32x4 o = philox_stream((uint32_t)(rb * 64 + c), (uint32_t)(2 * block_id + kh), seed);
                    m16 = philox_keep16(o, thr);
                }
                if (mask_out) mask_out[((size_t)rb * 2 + h) * 64 + lane] = (uint16_t)m16;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float zr = zt[mfma32_row(r, lane) * ZS + c];
                const float v = (acc[h][r] + bg[h]) * sigmoidf_fast(zr);
                pooled[r >> 2] += ((m16 >> r) & 1u) ? v : 0.f;
            }
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) pooled[jx] += __shfl_xor(pooled[jx], 32);
            const int j0 = 2 * kh;
            if (q0 + j0 < Q) p[(size_t)(q0 + j0) * 64 + c] = (kh ? pooled[2] : pooled[0]) * sc;
            if (q0 + j0 + 1 < Q) p[(size_t)(q0 + j0 + 1) * 64 + c] = (kh ? pooled[3] : pooled[1]) * sc;
        }
    }
}

#define GLUACC_N SED_GLUACC_N     // layout: common.h

// (BnBwdPrepArgs, bn_bwd_coef, bn_bwd_prep_body: kernels.h - shared with the conv kernels that consume the result)

// ---- backward: two waves per SIMD share one row block, split by channel half ---------------------------------------
// Round 1's k_glu_pool_bwd (one wave per SIMD, 415 registers; removed) issued in order: whatever VALU / LDS /
// global work is not perfectly interleaved with its MFMAs leaves the MFMA pipe idle (phase timestamps: 9.5 us per row
// block for 5.7 us of MFMAs).  Here waves w and w+4 - same SIMD - work on the SAME row block: wave half h owns the 32
// channels [32h, 32h+32) everywhere a channel index is an OUTPUT (lin columns, dz columns, dW rows), so each wave has
// half the accumulators (<= 256 registers: two waves per SIMD) and, while one wave of the pair is in VALU / LDS /
// memory instructions, the other's MFMAs keep the pipe busy.  The tile (z, y, dlin) is shared through LDS; three
// LDS-only workgroup barriers per row block (tile staged | dlin complete | tile free).
__global__ __launch_bounds__(512, 1) void k_glu_pool_bwd8(const float* __restrict__ y, const float* __restrict__ bn,
                                                          const float* __restrict__ wglu, const float* __restrict__ bglu,
                                                          const float* __restrict__ dp, const float* __restrict__ dp_b,
                                                          float* __restrict__ dz, double* __restrict__ accg, int H, int W, int Ho,
                                                          int Wo, int Q, int use_drop, float p_drop,
                                                          const uint16_t* __restrict__ mask_in) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pr = wave & 3, hf = wave >> 2;                 // pair (row-block slot), channel half
    const int n = lane & 31, kh = lane >> 5;
    const int c_own = 32 * hf + n;                           // the channel this lane owns as an output column
    float* WsT = smem + 4 * (3 * 32 * ZS);                   // Wglu transposed [c][co], stride 65
    float* zt = smem + pr * (3 * 32 * ZS);
    float* yt = zt + 32 * ZS;
    float* dlt = yt + 32 * ZS;
    if (H & 1) {        // the floor-mode pool drops the last row of an odd-height image: its gradient is 0
        const int per_clip = W * 64, nb = Q / (Ho * Wo);
        for (int i = blockIdx.x * 512 + tid; i < nb * per_clip; i += gridDim.x * 512) {
            const int bb = i / per_clip, r = i % per_clip;
            dz[((size_t)bb * H + (H - 1)) * W * 64 + r] = 0.f;
        }
    }
    // Wglu is requested here (two float4 per thread) and goes to LDS only behind the first row block's prefetch below: one round
    // trip for the whole prologue (as `WsT[..] = wglu[e]` dword by dword in front of everything it was two of its own)
    float4 wq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) wq[i] = ((const float4*)wglu)[tid + 512 * i];
    const float bgl = bglu[c_own];
    const float sc = 0.125f * (use_drop ? drop_scale8(p_drop) : 1.0f);
    f32x16 dW[2];                                            // dW[co own half][c block b2]
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
        for (int r = 0; r < 16; ++r) dW[b2][r] = 0.f;
    float sdb = 0.f, sdz = 0.f, sdzy = 0.f;
    const int n_rb = (Q + 3) / 4;
    const float4 bsc = *(const float4*)(bn + 128 + (lane & 15) * 4), bsh = *(const float4*)(bn + 192 + (lane & 15) * 4);
    const float inv_wo = 1.0f / (float)Wo, inv_ho = 1.0f / (float)Ho;
    auto divmod = [](int a, int d, float inv, int& rem) {
        int qd = (int)((float)a * inv);
        int r = a - qd * d;
        if (r < 0) { r += d; --qd; }
        if (r >= d) { r -= d; ++qd; }
        rem = r;
        return qd;
    };
    auto pixel_offsets = [&](int q0, uint32_t (&po)[4]) {     // byte offsets of the 4 pooled pixels' image pixels (dt = df = 0)
        int wo, ho;
        const int t = divmod(q0, Wo, inv_wo, wo);
        int bb = divmod(t, Ho, inv_ho, ho);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            po[j] = (q0 + j < Q) ? (uint32_t)((bb * H + 2 * ho) * W + 4 * wo) * 256u : 0u;
            if (++wo == Wo) { wo = 0; if (++ho == Ho) { ho = 0; ++bb; } }
        }
    };
    const uint32_t ld_off = (uint32_t)((lane >> 4) * 64 + (lane & 15) * 4) * 4u;
    const uint32_t st_off = (uint32_t)(kh * W * 64 + c_own) * 4u;
    // this wave stages rows m = (lane >> 4) + 4 * it for it in [4 hf, 4 hf + 4) of the pair's tile
    f32x4 yv[4];
    float gq_n[4];
    uint32_t m_n = 0xffffu, po_n[4];
    int q_n = 0;
    auto prefetch_begin = [&](int rbn, bool valid) {
        q_n = valid ? rbn * 4 : 0;
        pixel_offsets(q_n, po_n);
    };
    const bool has_b = dp_b != nullptr;
    const float* dp_2 = has_b ? dp_b : dp;
    auto prefetch_slice = [&](int k) {                         // k in 0..3
        // rows it = 4 hf + k: pooled pixel 2 hf + (k >> 1) (selected without indexing po_n by a run-time value, which
        // would put the array in scratch), image row dt = k & 1
        const uint32_t pbase = (k >> 1) ? (hf ? po_n[3] : po_n[1]) : (hf ? po_n[2] : po_n[0]);
        yv[k] = *(const f32x4*)((const char*)y + (pbase + (uint32_t)((k & 1) * W) * 256u + ld_off));
        const int q = q_n + k;
        const uint32_t goff = (uint32_t)((q < Q ? q : 0) * 64 + c_own) * 4u;
        // both planes unconditionally (the second pointer is the first again when there is one plane) and a select: as
        // `if (dp_b) gq += load` this was a uniform branch whose load was followed at once by s_waitcnt vmcnt(0), which
        // also drained the yv and dp loads just issued - four times per prefetch, in front of phase 1's MFMAs.
        // (a select, not `+ 0.f`: that would turn a -0 gradient into +0)
        const float ga = *(const float*)((const char*)dp + goff), gb = *(const float*)((const char*)dp_2 + goff);
        gq_n[k] = has_b ? ga + gb : ga;
        if (q >= Q) gq_n[k] = 0.f;
        if (k == 0) m_n = use_drop ? (uint32_t)mask_in[((size_t)(q_n >> 2) * 2 + hf) * 64 + lane] : 0xffffu;
    };
    const int rb0 = blockIdx.x * 4 + pr;
    prefetch_begin(rb0, rb0 < n_rb);
#pragma unroll
    for (int k = 0; k < 4; ++k) prefetch_slice(k);
    // (the empty asm keeps slices 1 - 3 in front of the barrier: y and dp are read-only, so the compiler was free to sink their
    // loads behind it, and did - the gradient loads behind a wait of their own, the y loads behind a second one)
    asm volatile("" : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(gq_n[0]), "+v"(gq_n[1]), "+v"(gq_n[2]), "+v"(gq_n[3]));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = 4 * (tid + 512 * i);                   // Wglu[co = e >> 6][c = e & 63 .. + 3]
        float* d = &WsT[(e & 63) * ZS + (e >> 6)];
        d[0] = wq[i].x; d[ZS] = wq[i].y; d[2 * ZS] = wq[i].z; d[3 * ZS] = wq[i].w;
    }
    __syncthreads();
    float bw[32];                                            // phase 1: B[k = c][j = co own half] = Wglu[co][c]
#pragma unroll
    for (int s = 0; s < 32; ++s) bw[s] = WsT[(2 * s + kh) * ZS + c_own];
    const float* BT = WsT + c_own * ZS + kh;                 // phase 2: B[k = co][j = c own half] = WsT[c][co]
    // every pair runs the same number of trips (the barriers are workgroup-wide); pairs past the end idle through them
    const int trips = (n_rb - blockIdx.x * 4 + gridDim.x * 4 - 1) / (gridDim.x * 4);
    for (int trip = 0; trip < trips; ++trip) {
        const int rb = rb0 + trip * gridDim.x * 4;
        const bool live = rb < n_rb;
        const int q0 = rb * 4;
        if (live) {
            // ---- stage this wave's 4 of the 8 row groups: z = scale * y + shift, and y itself --------------------
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int it = 4 * hf + k, m = (lane >> 4) + 4 * it, c4 = (lane & 15) * 4;
                const f32x4 v = yv[k];
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                if (q0 + (m >> 3) < Q) { z.x = fmaf(v.x, bsc.x, bsh.x); z.y = fmaf(v.y, bsc.y, bsh.y); z.z = fmaf(v.z, bsc.z, bsh.z); z.w = fmaf(v.w, bsc.w, bsh.w); }
                float* d = zt + m * ZS + c4;
                d[0] = z.x; d[1] = z.y; d[2] = z.z; d[3] = z.w;
                float* e = yt + m * ZS + c4;
                e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
            }
        }
        float gq_c[4];
        uint32_t po[4];
        const uint32_t m_c = m_n;
#pragma unroll
        for (int j = 0; j < 4; ++j) { po[j] = po_n[j] + st_off; gq_c[j] = gq_n[j] * sc; }
        prefetch_begin(rb + gridDim.x * 4, rb + gridDim.x * 4 < n_rb);
        lds_barrier();                                        // A: the pair's tile is complete
        f32x16 lin, acc;
        float dzg[16];
        if (live) {
            // ---- phase 1: lin[:, own half] = z @ Wglu^T   ||   sigma(z), dlin = g * sigma -> LDS -------------------
#pragma unroll
            for (int r = 0; r < 16; ++r) lin[r] = 0.f;
            const float* A = zt + n * ZS + kh;
            float a_c[4], z_c[2];
#pragma unroll
            for (int u = 0; u < 4; ++u) a_c[u] = A[2 * u];
#pragma unroll
            for (int u = 0; u < 2; ++u) z_c[u] = zt[mfma32_row(u, lane) * ZS + c_own];
#pragma unroll
            for (int g4 = 0; g4 < 8; ++g4) {                  // 4 K-steps + 2 elements per group
                float a_n[4] = {0.f, 0.f, 0.f, 0.f}, z_n[2] = {0.f, 0.f};
                if (g4 + 1 < 8) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) a_n[u] = A[2 * (4 * (g4 + 1) + u)];
#pragma unroll
                    for (int u = 0; u < 2; ++u) z_n[u] = zt[mfma32_row(2 * (g4 + 1) + u, lane) * ZS + c_own];
                }
                if (g4 < 4) prefetch_slice(g4);
#pragma unroll
                for (int u = 0; u < 4; ++u) lin = mfma32(a_c[u], bw[4 * g4 + u], lin);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int r = 2 * g4 + u;
                    const float gg = ((m_c >> r) & 1u) ? gq_c[r >> 2] : 0.f;
                    const float sg = sigmoidf_fast(z_c[u]);
                    const float dl = gg * sg;
                    dlt[mfma32_row(r, lane) * ZS + c_own] = dl;
                    sdb += dl;
                    dzg[r] = dl * (1.0f - sg);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) a_c[u] = a_n[u];
                z_c[0] = z_n[0]; z_c[1] = z_n[1];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        lds_barrier();                                        // B: dlin of both halves is in LDS
        if (live) {
            // ---- phase 2: dz_lin[:, own half] = dlin @ Wglu   ||   gate path dzg = t * (lin + b) -------------------
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* A = dlt + n * ZS + kh;
            // operands two MFMAs ahead in rotating registers (a `_c = _n` copy per step made the wave wait for the prefetch
            // it had just issued: ds_read x2 | s_waitcnt lgkmcnt(0) | one MFMA, thirty-two times)
            float a_r[4], b_r[4];
            a_r[0] = A[0]; b_r[0] = BT[0]; a_r[1] = A[2]; b_r[1] = BT[2];
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                if (s + 2 < 32) { a_r[(s + 2) & 3] = A[2 * (s + 2)]; b_r[(s + 2) & 3] = BT[2 * (s + 2)]; }
                acc = mfma32(a_r[s & 3], b_r[s & 3], acc);
                if (s < 16) dzg[s] *= lin[s] + bgl;
                __builtin_amdgcn_sched_barrier(0);
            }
            // claim the prefetched registers while only loads are outstanding (vmcnt cannot tell loads from stores)
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(yv[k]), "+v"(gq_n[k]));
            asm volatile("" : "+v"(m_n));
            // ---- phase 3: dW[own co half][:] += dlin^T z   ||   dz = dz_lin + dzg -> global, BN-backward sums ------
            float a3[2], b3[2][2];
            a3[0] = dlt[kh * ZS + c_own]; b3[0][0] = zt[kh * ZS + n]; b3[0][1] = zt[kh * ZS + 32 + n];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if (s + 1 < 16) {          // the next step's three operands now, one pair of MFMAs ahead
                    const int mn = 2 * (s + 1) + kh;
                    a3[(s + 1) & 1] = dlt[mn * ZS + c_own];
                    b3[(s + 1) & 1][0] = zt[mn * ZS + n]; b3[(s + 1) & 1][1] = zt[mn * ZS + 32 + n];
                }
                dW[0] = mfma32(a3[s & 1], b3[s & 1][0], dW[0]);
                dW[1] = mfma32(a3[s & 1], b3[s & 1][1], dW[1]);
                const int r = s, i = mfma32_row(r, lane);
                const float v = acc[r] + dzg[r];
                if (q0 + (r >> 2) < Q) {
                    *(float*)((char*)dz + (po[r >> 2] + (uint32_t)((r & 3) * 64 * 4))) = v;
                    sdz += v;
                    sdzy += v * yt[i * ZS + c_own];
                }
            }
        }
        lds_barrier();                                        // C: the tile may be overwritten
    }
    // ---- reduce over the 4 pairs through LDS (each (co, c) lives in exactly one half), then fp64 atomics ---------------
    float* red = smem;   // [4 pairs][64][64]: 64 KB of the 100 KB of tiles
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[pr * 4096 + (32 * hf + mfma32_row(r, lane)) * 64 + 32 * b2 + n] = dW[b2][r];
    __syncthreads();
    for (int i = tid; i < 4096; i += 512)
        atomicAdd(&accg[i], (double)red[i] + (double)red[4096 + i] + (double)red[8192 + i] + (double)red[12288 + i]);
    __syncthreads();
    {
        const float v0 = sdb + __shfl_xor(sdb, 32), v1 = sdz + __shfl_xor(sdz, 32), v2 = sdzy + __shfl_xor(sdzy, 32);
        if (kh == 0) {
            red[(pr * 3 + 0) * 64 + c_own] = v0;
            red[(pr * 3 + 1) * 64 + c_own] = v1;
            red[(pr * 3 + 2) * 64 + c_own] = v2;
        }
    }
    __syncthreads();
    if (tid < 192) {
        const int which = tid >> 6, c = tid & 63;
        double v = 0;
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) v += (double)red[(w2 * 3 + which) * 64 + c];
        atomicAdd(&accg[4096 + which * 64 + c], v);
    }
}

// BatchNorm-backward coefficients + the block's parameter gradients: a kernel of its own again.  Folding it into the
// last workgroup of the GLU backward (ticket after a workgroup-scope release) was a RACE: about 1 step in 10 the last
// workgroup read the Sdz / Sdzy accumulators before every other workgroup's fp64 atomics had been performed
// (tools/determinism.py: bn1 / conv1 / block-0 gradients off by up to 7e-3); ordering those atomics device-wide needs
// __threadfence(), whose L2 write-back of the 31 MB of dz just produced costs more (17 us) than this launch (5 us).
__global__ __launch_bounds__(256) void k_bn_bwd_prep(BnBwdPrepArgs a) { bn_bwd_prep_body(a, threadIdx.x, 256); }

// ---- host launchers -------------------------------------------------------------------------------
int launch_glu_pool_fwd(const float* y, const double* stat, double N, const float* gamma, const float* beta, float* run_mean,
                        float* run_var, int64_t* tracked, int train, int update, float eps, float momentum, float* bn,
                        const float* wglu, const float* bglu, float* p, int B, int H, int W, int block_id, int use_drop,
                        float p_drop, const uint64_t* seed, uint16_t* mask_out, hipStream_t st) {
    BnPrepArgs a;
    a.stat = stat; a.N = N; a.gamma = gamma; a.beta = beta; a.run_mean = run_mean; a.run_var = run_var;
    a.tracked = tracked; a.train = train; a.update = update; a.eps = eps; a.momentum = momentum; a.bn = bn;
    SED_CHECK_ARG(((uintptr_t)wglu & 15) == 0, "glu weight must be 16-byte aligned (float4 staging loads)");
    const int Ho = H / 2, Wo = W / 4, Q = B * Ho * Wo;
    const int n_rb = (Q + 3) / 4;
    int grid = (n_rb + 3) / 4;
    if (grid > 512) grid = 512;
    k_glu_pool_fwd<<<grid, 256, 0, st>>>(y, a, wglu, bglu, p, H, W, Ho, Wo, Q, block_id, use_drop, p_drop, seed, mask_out);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

int launch_glu_pool_bwd(const float* y, const float* bn, const float* wglu, const float* bglu, const float* dp,
                        const float* dp_b, float* dz, double* acc, int zero_acc, int B, int H, int W, int use_drop, float p_drop,
                        const uint16_t* mask_in, const float* gamma, float* coef, float* g_gamma, float* g_beta, float* g_wglu,
                        float* g_bglu, float* g_convb, BnBwdPrepArgs* prep_out, hipStream_t st) {
    SED_CHECK_ARG(((uintptr_t)wglu & 15) == 0, "glu weight must be 16-byte aligned (float4 staging loads)");
    const int Ho = H / 2, Wo = W / 4, Q = B * Ho * Wo;
    const size_t lds = (size_t)(4 * 3 * 32 * ZS + 64 * ZS) * sizeof(float);
    static thread_local SedAttrOnce attr_done;
    if (attr_done.need()) {
        SED_CHECK_HIP(hipFuncSetAttribute((const void*)k_glu_pool_bwd8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (zero_acc) SED_CHECK_HIP(hipMemsetAsync(acc, 0, GLUACC_N * sizeof(double), st));
    BnBwdPrepArgs a;
    a.acc = acc; a.N = (double)B * H * W; a.gamma = gamma; a.bn = bn; a.coef = coef; a.g_gamma = g_gamma; a.g_beta = g_beta;
    a.g_wglu = g_wglu; a.g_bglu = g_bglu; a.g_convb = g_convb;
    const int n_rb = (Q + 3) / 4;
    int grid = (n_rb + 3) / 4;
    if (grid > 256) grid = 256;
    k_glu_pool_bwd8<<<grid, 512, lds, st>>>(y, bn, wglu, bglu, dp, dp_b, dz, acc, H, W, Ho, Wo, Q, use_drop, p_drop, mask_in);
    SED_CHECK_LAUNCH();
    if (prep_out) {             // the conv dgrad / wgrad kernels derive the coefficients themselves
        *prep_out = a;
        return SED_OK;
    }
    k_bn_bwd_prep<<<1, 256, 0, st>>>(a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

