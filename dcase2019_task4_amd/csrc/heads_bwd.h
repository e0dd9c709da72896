// heads_bwd.h - the body of the heads backward kernel, included by heads.hip once per form (no include guard):
//   HEADS_BWD_KERNEL      k_heads_bwd | k_heads_bwd_att
//   HEADS_BWD_ATT_PARAM   nothing | one more kernel parameter, `, const float* __restrict__ d_att` [B][T][NC] = dLoss/d(sof)
//   HEADS_BWD_ATT_TERM(i) nothing | `+ d_att[i]`: the gradient that reaches sof in front of the clamp's pass mask
// (sed_crnn_backward_att).  Text, not a template or an inlined function: k_heads_bwd sits at the 128-VGPR edge, and both of those
// forms moved its register allocation (HF = 512 spilled); with the macros empty the compiler sees the tokens it always saw.
template <int HF>
__global__ __launch_bounds__(HD_THREADS) void HEADS_BWD_KERNEL(const float* __restrict__ h, const float* __restrict__ wd,
                                                    const float* __restrict__ ws, const float* __restrict__ strong,
                                                    const float* __restrict__ weak, const float* __restrict__ logits_s,
                                                    const float* __restrict__ den, const float* __restrict__ d_strong,
                                                    const float* __restrict__ d_weak, float* __restrict__ dh,
                                                    float* __restrict__ part, int T, int NC, int use_drop, float p_drop,
                                                    const uint64_t* __restrict__ seed_ptr, double* __restrict__ zero, int n_zero,
                                                    HeadsLoss hl HEADS_BWD_ATT_PARAM) {
    HD_CONSTS(HF);
    constexpr int TPW = HF / 128;                      // dW tiles (16 outputs x 16 features) per wave: 2 x HF / 16 tiles, 16 waves
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    // the fp64 accumulators of the conv-block backward that follows (saves a memset node on the critical path)
    if (blockIdx.y == 0)
        for (int i = blockIdx.x * HD_THREADS + threadIdx.x; i < n_zero; i += gridDim.x * HD_THREADS) zero[i] = 0.0;
    float* xs = hsm;                                   // [HD_TC][HD_SB]
    float* wsm = xs + HD_TC * HD_SB;                   // [HD_MAXO][HD_SB]
    float* dl = wsm + HD_MAXO * HD_SB;                 // [HD_TC][HD_SD]
    float* dnum = dl + HD_TC * HD_SD;
    float* dden = dnum + 16;
    uint32_t* mk = (uint32_t*)(dden + 16);             // [HD_TC][HF / 16] keep bits of the staged chunk
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wv = tid >> 6;
    const int NY = gridDim.y, cy = blockIdx.y;         // this workgroup's share of the clip: chunks cy, cy + NY, ... (kernels.h heads_bwd_chunks)
    const int i16 = lane & 15, kq = lane >> 4;
    const uint64_t seed = use_drop ? seed_ptr[0] : 0ull;
    const uint32_t thr = drop_thresh8(p_drop);
    const float ks = use_drop ? drop_scale8(p_drop) : 1.0f;
    const int NO = 2 * NC;
    heads_stage_w<HF, HD_SB>(wd, ws, wsm, NC, tid);
    const bool fused = hl.strong_ema != nullptr;
    const int B = gridDim.x;
    float lacc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // weak_bce, strong_bce, mse_strong, mse_weak, weak_ema_bce, strong_ema_bce
    const float cw = fused ? hl.state->cons_weight : 0.f;
    const float inv_nS = 1.0f / (float)(B * T * NC), inv_nW = 1.0f / (float)(B * NC);
    const float inv_sb = (hl.shi > hl.slo) ? 1.0f / (float)((hl.shi - hl.slo) * T * NC) : 0.f;
    const float inv_wb = (hl.whi > hl.wlo) ? 1.0f / (float)((hl.whi - hl.wlo) * NC) : 0.f;
    const bool in_s = fused && b >= hl.slo && b < hl.shi, in_w = fused && b >= hl.wlo && b < hl.whi;
    float* tmaxs = dden + 16;                          // (aliases the mask words, which are first written inside the loop)
    if (in_w && wv < NC) {                             // target_weak = target.max(-2) (main.py:95): wave c takes class c
        float t = -3.0e38f;
        for (int tt = lane; tt < T; tt += 64) t = fmaxf(t, hl.target[((size_t)b * T + tt) * NC + wv]);
        t = wave_max(t);
        if (lane == 0) tmaxs[wv] = t;
    }
    if (fused) __syncthreads();
    if (tid < NC) {
        float dw;
        if (fused) {
            const float p = weak[b * NC + tid], pe = hl.weak_ema[b * NC + tid];
            const float diff = p - pe;
            const float once = cy == 0 ? 1.f : 0.f;          // the clip-level terms enter the sums through ONE of the clip's workgroups
            lacc[3] = once * diff * diff;
            dw = cw * 2.0f * diff * inv_nW;
            if (in_w) {
                const float t = tmaxs[tid];
                lacc[0] = once * bce_term(p, t);
                lacc[4] = once * bce_term(pe, t);
                dw += bce_grad(p, t) * inv_wb;
            }
            if (hl.d_weak_out) hl.d_weak_out[b * NC + tid] = dw;
        } else {
            dw = d_weak[b * NC + tid];
        }
        const float dn = den[b * NC + tid];
        dnum[tid] = dw / dn;
        dden[tid] = -dw * weak[b * NC + tid] / dn;
    }
    // dW[o][f] accumulates over chunks in the MFMA accumulator of the wave that owns the (o, f) tile
    f32x4 wacc[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) wacc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;    // thread o < NO
    for (int t0 = cy * HD_TC; t0 < T; t0 += NY * HD_TC) {
        __syncthreads();
        mk[tid] = heads_stage<HF, HD_SB>(h, xs, b, T, t0, use_drop, seed, thr, ks, tid);
        {   // softmax / sigmoid backward of the chunk's frames: 8 threads per frame, thread `sub` takes classes sub and sub + 8
            // (one thread per frame walking all classes left 7/8 of the workgroup idle for the longest serial stretch of
            // the kernel); the three per-frame reductions (max, sum of exponentials, dot) are DPP butterflies inside the
            // 8-lane group: quad_perm xor 1, xor 2, then row_half_mirror
            const int tl = tid >> 3, sub = tid & 7, t = t0 + tl;
            auto red8_sum = [](float v) {
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
                return v;
            };
            auto red8_max = [](float v) {
                v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
                v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
                v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
                return v;
            };
            float* dlr = dl + tl * HD_SD;
            if (tl >= HD_TC) {
                // (HF = 512: only the first HD_TC * 8 threads own a frame of the chunk)
            } else if (t < T) {
                const size_t e0 = (size_t)(b * T + t) * NC;
                const bool has[2] = {sub < NC, sub + 8 < NC};
                float lg[2], ex[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) lg[q] = has[q] ? logits_s[e0 + sub + 8 * q] : -3.0e38f;
                const float mx = red8_max(fmaxf(lg[0], lg[1]));
#pragma unroll
                for (int q = 0; q < 2; ++q) ex[q] = has[q] ? __expf(lg[q] - mx) : 0.f;
                const float inv = rcp_fast(red8_sum(ex[0] + ex[1]));
                float raw[2], ds[2], dsig[2], dpart = 0.f;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    raw[q] = 0.f; ds[q] = 0.f; dsig[q] = 0.f;
                    if (has[q]) {
                        const int c = sub + 8 * q;
                        const float sv = strong[e0 + c];
                        raw[q] = ex[q] * inv;
                        const float sof = fminf(fmaxf(raw[q], 1e-7f), 1.0f);
                        const float pass = (raw[q] >= 1e-7f && raw[q] <= 1.0f) ? 1.f : 0.f;
                        ds[q] = (dnum[c] * sv + dden[c] HEADS_BWD_ATT_TERM(e0 + c)) * pass;
                        dpart += raw[q] * ds[q];
                        float gin;
                        if (fused) {
                            const float pe = hl.strong_ema[e0 + c];
                            const float diff = sv - pe;
                            lacc[2] += diff * diff;
                            gin = cw * 2.0f * diff * inv_nS;
                            if (in_s) {
                                const float tg = hl.target[e0 + c];
                                lacc[1] += bce_term(sv, tg);
                                lacc[5] += bce_term(pe, tg);
                                gin += bce_grad(sv, tg) * inv_sb;
                            }
                            if (hl.d_strong_out) hl.d_strong_out[e0 + c] = gin;
                        } else {
                            gin = d_strong[e0 + c];
                        }
                        dsig[q] = (gin + dnum[c] * sof) * sv * (1.0f - sv);
                    }
                }
                const float dot = red8_sum(dpart);
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (has[q]) {
                        dlr[sub + 8 * q] = dsig[q];
                        dlr[NC + sub + 8 * q] = raw[q] * (ds[q] - dot);
                    }
                for (int o = NO + sub; o < HD_MAXO; o += 8) dlr[o] = 0.f;
            } else {
                for (int o = sub; o < HD_MAXO; o += 8) dlr[o] = 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TPW; ++q) {   // dW[o][f] += sum_t dl[t][o] x[t][f]: 2 x HF / 16 tiles, TPW per wave, K = HD_TC frames
            const int tile = wv * TPW + q, ot = tile / HD_GPF, ft = tile % HD_GPF;
            const float* A = dl + kq * HD_SD + 16 * ot + i16;          // A[i = o][k = t]
            const float* Bp = xs + kq * HD_SB + 16 * ft + i16;         // B[k = t][j = f]
#pragma unroll 8
            for (int s4 = 0; s4 < HD_TC / 4; ++s4) wacc[q] = mfma16(A[4 * s4 * HD_SD], Bp[4 * s4 * HD_SB], wacc[q]);
        }
        if (tid < NO) {
            float a = 0.f;
            for (int tl = 0; tl < HD_TC; ++tl) a += dl[tl * HD_SD + tid];
            bacc += a;
        }
        // dx[t][f] = (sum_o dl[t][o] W[o][f]) * mask: (HD_TC / 16) x (HF / 16) = 64 tiles, four per wave, K = 32
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int tile = wv * 4 + q, tt = tile / HD_GPF, ft = tile % HD_GPF;
            const float* A = dl + (16 * tt + i16) * HD_SD + kq;        // A[i = t][k = o]
            const float* Bp = wsm + kq * HD_SB + 16 * ft + i16;        // B[k = o][j = f]
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < 8; ++s4) acc = mfma16(A[4 * s4], Bp[4 * s4 * HD_SB], acc);
            const int f = 16 * ft + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tl = 16 * tt + 4 * kq + r, t = t0 + tl;
                if (t < T) {
                    const uint32_t keep = (mk[tl * HD_GPF + (f >> 4)] >> (f & 15)) & 1u;
                    dh[(size_t)(b * T + t) * HD_F + f] = keep ? acc[r] * ks : 0.f;
                }
            }
        }
    }
    float* pr = part + (size_t)(b * NY + cy) * (2 * (NC * HD_F + NC));
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int tile = wv * TPW + q, ot = tile / HD_GPF, ft = tile % HD_GPF, f = 16 * ft + i16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 16 * ot + 4 * kq + r;
            if (o < NC) pr[o * HD_F + f] = wacc[q][r];
            else if (o < NO) pr[NC * HD_F + NC + (o - NC) * HD_F + f] = wacc[q][r];
        }
    }
    if (tid < NC) pr[NC * HD_F + tid] = bacc;
    else if (tid < NO) pr[2 * NC * HD_F + NC + (tid - NC)] = bacc;
    if (!fused) return;
    // ---- the loss values: workgroup sums -> per-clip partials -> the last workgroup adds them in clip order ----
    __syncthreads();
    float* red = dl;                                    // [16 waves][8]
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = wave_sum(lacc[k]);
        if (lane == 0) red[wv * 8 + k] = v;
    }
    __syncthreads();
    const int NP = B * NY;                              // loss partials: one per workgroup, summed in (clip, chunk) order
    float* lpart = NY == 1 ? hl.losses + 8 : part + (size_t)NP * (2 * (NC * HD_F + NC));
    unsigned int* ticket = (unsigned int*)(hl.losses + 8 + 8 * B);
    __shared__ int is_last;
    if (tid < 6) {
        float s2 = 0.f;
        for (int w2 = 0; w2 < HD_THREADS / 64; ++w2) s2 += red[w2 * 8 + tid];
        lpart[8 * (b * NY + cy) + tid] = s2;
        __threadfence();
    }
    __syncthreads();
    if (tid == 0) is_last = (atomicAdd(ticket, 1u) == (unsigned int)(NP - 1));
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    {   // all per-clip partials in ONE round trip (a 6-thread loop over the clips paid one memory latency per clip), then
        // six threads add them up in clip order
        float* stage = dl + 128;                             // [8 * B] behind the wave partials (B <= 512; larger batches: loop)
        const bool staged = 8 * NP <= HD_TC * HD_SD - 128;
        if (staged)
            for (int e = tid; e < 8 * NP; e += HD_THREADS) stage[e] = __builtin_nontemporal_load(&lpart[e]);
        __syncthreads();
        if (tid < 6) {
            float s2 = 0.f;
            if (staged) for (int bb = 0; bb < NP; ++bb) s2 += stage[8 * bb + tid];
            else for (int bb = 0; bb < NP; ++bb) s2 += __builtin_nontemporal_load(&lpart[8 * bb + tid]);
            red[tid] = s2;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float wb = red[0] * inv_wb, sb = red[1] * inv_sb;
        const float cs = cw * red[2] * inv_nS, cwk = cw * red[3] * inv_nW;
        hl.losses[0] = wb + sb + cs + cwk;
        hl.losses[1] = wb; hl.losses[2] = sb; hl.losses[3] = cs; hl.losses[4] = cwk;
        hl.losses[5] = red[4] * inv_wb; hl.losses[6] = red[5] * inv_sb; hl.losses[7] = cw;
        *ticket = 0u;
        if (hl.advance) step_state_advance_early(hl.advance);   // every workgroup has read its fields of this step by now
    }
}
