// score.hip - validation scoring on the device: event-based, segment-based and clip-level (weak) counts, and the PSDS
// intersection counts (k_psds_counts, further down).
//
// Reference ops (baseline/main.py:328-352, evaluation_measures.py:19-102,124-182,234-246), host-side, once per epoch:
//   compute_strong_metrics(predictions, valid_df) -> sed_eval EventBasedMetrics(t_collar = 0.2, percentage_of_length = 0.2,
//       empty_system_output_handling = 'zero_score', event_matching_type = 'optimal') and SegmentBasedMetrics(1 s),
//       fed one file at a time with lists of dicts made from two pandas tables;
//   get_f_measure_by_class -> intermediate_at_measures per batch on the host.
// sed_eval is third-party and absent from this image and from the reference tree: the event / segment definitions below are
// restated from its published algorithm - PARITY WITH sed_eval ITSELF IS UNPINNED (as oracle/postprocess_np.py states for
// dcase_util).  Pinned: exact agreement with an independent numpy / scipy statement of the same definitions
// (tests/sed_eval_np.py, tests/test_gpu_metrics.py).
//
// k_event_counts: one workgroup per (operating point, clip), one wave per class column.  A wave decodes its column with the
// code k_postprocess runs (post.h) but keeps the events in LDS as fp64 seconds, then
//   event-based: lane r holds reference event r and a 64-bit mask of the estimated events compatible with it (the estimated
//     events are broadcast LDS reads).  Ntp = size of a maximum bipartite matching: one breadth-first augmenting-path search
//     per estimated event, every level of it one ballot - the frontier, the visited set and the matched set are wave-uniform
//     64-bit masks in SGPRs, so all variable-trip-count loops run on scalar control flow;
//   segment-based: lane s is segment s0 + s; an event covers segments max(0, floor(on / res)) .. ceil(off / res) - 1; the file's
//     segment count (for Ntn) is the maximum over the workgroup's columns, reduced through LDS.
// All counts are integers and the class totals are integer atomics, so results are bit-reproducible run to run.
#pragma clang fp contract(off)       // seconds are formed as (double)frame * num / den, exactly the host's two operations
#include "common.h"
#include "kernels.h"
#include "post.h"

#define SC_MAXEV 64                  // events per (clip, class) column and side: one lane / one mask bit each
#define SC_MAXSEG 65536              // segments per file
#define SC_MAXNC 16
#define SC_HEAD (SC_MAXNC * 4)       // bytes of the per-column segment counts in front of the decode buffers

struct EvArgs {
    const float* strong; int T, NC; const float* thr; const int32_t* win; double num, den;
    const int32_t* est_ptr; const double *est_on, *est_off;
    const int32_t* ref_ptr; const double *ref_on, *ref_off;
    double t_collar, pct, res;
    int32_t *ev_counts, *seg_counts; unsigned long long *ev_total, *seg_total; int32_t* err;
    int tpad;                        // bytes of one raw / flt buffer (0 when the events are given)
};

__device__ __forceinline__ int lane_read(int v, int src) {
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src));
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// segment index of a time, clamped to [0, SC_MAXSEG + 1] (NaN -> 0) so that the cast is defined
__device__ __forceinline__ int seg_index(double x) {
    return !(x > 0.0) ? 0 : (x > (double)SC_MAXSEG ? SC_MAXSEG + 1 : (int)x);
}

__global__ __launch_bounds__(1024) void k_event_counts(EvArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int NC = a.NC, n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = n * NC + c;
    double* e_on = (double*)smem + c * SC_MAXEV;                    // [NC][64] onsets, then [NC][64] offsets
    double* e_off = (double*)smem + (NC + c) * SC_MAXEV;
    int* s_nseg = (int*)(smem + (size_t)NC * SC_MAXEV * 16);        // [SC_MAXNC]
    int flags = 0;
    int n_est;
    if (a.strong) {
        uint8_t* raw = smem + (size_t)NC * SC_MAXEV * 16 + SC_HEAD + (size_t)c * 2 * a.tpad;
        const int window = a.win[k];
        if (window < 1 || window > 63) flags |= 8;
        const double num = a.num, den = a.den;
        n_est = pp_decode_column(a.strong + (size_t)n * a.T * NC + c, a.T, NC, a.thr[k], min(max(window, 1), 63), raw,
                                 raw + a.tpad, nullptr, [=](int i, int frame, bool is_offset) {
                                     if (i < SC_MAXEV) (is_offset ? e_off : e_on)[i] = (double)frame * num / den;
                                 });
    } else {
        const int e0 = a.est_ptr[col];
        n_est = a.est_ptr[col + 1] - e0;
        if (lane < n_est && n_est <= SC_MAXEV) {
            e_on[lane] = a.est_on[e0 + lane];
            e_off[lane] = a.est_off[e0 + lane];
        }
    }
    __syncthreads();
    const int r0 = a.ref_ptr[col], n_ref = a.ref_ptr[col + 1] - r0;
    if (n_ref > SC_MAXEV) flags |= 1;
    if (n_est > SC_MAXEV) flags |= 2;
    if (n_ref < 0 || n_est < 0) flags |= 16;
    const bool ok = flags == 0;                                            // wave-uniform
    const bool has_ref = ok && lane < n_ref, has_est = ok && lane < n_est;
    double r_on = 0.0, r_off = 0.0;
    if (has_ref) {
        r_on = a.ref_on[r0 + lane];
        r_off = a.ref_off[r0 + lane];
    }
    // ---- event-based: compatibility masks, then a maximum matching by augmenting paths ---------------------------------
    int ntp = 0;
    if (ok) {
        const double tol_off = fmax(a.t_collar, a.pct * (r_off - r_on));
        unsigned long long adj = 0;                                  // bit e: estimated event e is compatible with my reference
        for (int e = 0; e < n_est; ++e) {
            const double eo = e_on[e], ef = e_off[e];
            const bool hit = has_ref && fabs(r_on - eo) <= a.t_collar && fabs(r_off - ef) <= tol_off;
            adj |= (unsigned long long)hit << e;
        }
        int m_est = -1;                        // lane e: the reference matched to estimated event e
        int parent = 0;                        // lane r: the estimated event that reached reference r in this search
        unsigned long long matched_ref = 0;
        for (int root = 0; root < n_est; ++root) {
            unsigned long long frontier = 1ull << root, visited = 0;         // estimated events / reference events
            while (frontier) {
                const unsigned long long reach = adj & frontier;
                const bool fresh = reach != 0 && !((visited >> lane) & 1);
                const unsigned long long new_ref = __ballot(fresh);
                if (!new_ref) break;
                if (fresh) parent = __ffsll((long long)reach) - 1;
                const unsigned long long free_new = new_ref & ~matched_ref;
                if (free_new) {                // an unmatched reference: flip the path back to the root
                    int r = __ffsll((long long)free_new) - 1;
                    matched_ref |= 1ull << r;
                    for (int hop = 0; hop < SC_MAXEV; ++hop) {
                        const int e = lane_read(parent, r);
                        const int prev = lane_read(m_est, e);
                        if (lane == e) m_est = r;
                        if (prev < 0) break;
                        r = prev;
                    }
                    ++ntp;
                    break;
                }
                visited |= new_ref;
                frontier = __ballot(m_est >= 0 && ((new_ref >> (m_est & 63)) & 1));
            }
        }
    }
    // ---- segment-based ---------------------------------------------------------------------------------------------------
    int rlo = 0, rhi = 0, elo = 0, ehi = 0;
    if (has_ref) {
        rlo = seg_index(floor(r_on / a.res));
        rhi = seg_index(ceil(r_off / a.res));
    }
    if (has_est) {
        elo = seg_index(floor(e_on[lane] / a.res));
        ehi = seg_index(ceil(e_off[lane] / a.res));
    }
    const int col_seg = wave_imax(max(rhi, ehi));
    if (col_seg > SC_MAXSEG) flags |= 4;
    if (lane == 0) s_nseg[c] = col_seg;
    __syncthreads();
    const int file_seg = wave_imax(lane < NC ? s_nseg[lane] : 0);
    int tp = 0, fp = 0, fn = 0, tn = 0;
    if (ok && file_seg <= SC_MAXSEG) {
        for (int s0 = 0; s0 < col_seg; s0 += 64) {
            const int s = s0 + lane;
            bool ra = false, ea = false;
            for (int r = 0; r < n_ref; ++r) ra |= s >= lane_read(rlo, r) && s < lane_read(rhi, r);
            for (int e = 0; e < n_est; ++e) ea |= s >= lane_read(elo, e) && s < lane_read(ehi, e);
            tp += __popcll(__ballot(ra && ea));
            fp += __popcll(__ballot(ea && !ra));
            fn += __popcll(__ballot(ra && !ea));
        }
        tn = file_seg - tp - fp - fn;
    }
    if (lane == 0) {
        const size_t o = ((size_t)k * N + n) * NC + c, t = (size_t)k * NC + c;
        const int ev[3] = {ntp, n_ref, n_est}, sg[4] = {tp, fp, fn, tn};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (a.ev_counts) a.ev_counts[o * 3 + i] = ev[i];
            if (ev[i] > 0) atomicAdd(a.ev_total + t * 3 + i, (unsigned long long)ev[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (a.seg_counts) a.seg_counts[o * 4 + i] = sg[i];
            if (sg[i] > 0) atomicAdd(a.seg_total + t * 4 + i, (unsigned long long)sg[i]);
        }
        if (flags) atomicOr(a.err, flags);
    }
}

// ---- PSDS intersection counts (Bilen et al., ICASSP 2020) -------------------------------------------------------------------
// psds_eval is third-party and absent from this image and from the reference tree: the three criteria are restated from the
// paper (include/dcase_sed.h holds the definitions) - PARITY WITH psds_eval ITSELF IS UNPINNED.  Pinned: exact agreement
// with an independent numpy statement of the same definitions (tests/psds_np.py, tests/test_gpu_psds.py).
//
// k_psds_counts: the grid and the decode of k_event_counts, but the detections AND the references of all the file's classes
// are staged in LDS as fp64 (the cross-trigger test of class c reads the references of every other class).  No matching:
// every criterion is a sequential fp64 sum of interval intersections over the other side's events in stored order (broadcast
// LDS reads), a division and a comparison - lane e is detection e for DTC and CTTC, lane r is ground truth r for GTC, the
// relevance mask GTC reads is one ballot, every count a popcount.
struct PsArgs {
    const float* strong; int T, NC; const float* thr; const int32_t* win; double num, den;
    const int32_t* est_ptr; const double *est_on, *est_off;
    const int32_t* ref_ptr; const double *ref_on, *ref_off;
    double dtc, gtc, cttc;
    int32_t* columns; unsigned long long* totals; int32_t* err;
    int tpad;                        // bytes of one raw / flt buffer (0 when the events are given)
};

// max(0, min(d.off, g.off) - max(d.on, g.on))
__device__ __forceinline__ double ps_overlap(double a_on, double a_off, double b_on, double b_off) {
    return fmax(0.0, fmin(a_off, b_off) - fmax(a_on, b_on));
}
// sum / len >= threshold: the division first; an event of length <= 0 and a NaN ratio fail
__device__ __forceinline__ bool ps_passes(double sum, double len, double threshold) {
    return len > 0.0 && sum / len >= threshold;
}

__global__ __launch_bounds__(1024) void k_psds_counts(PsArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int NC = a.NC, n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = n * NC + c;
    double* ev = (double*)smem;                                     // [4][NC][64]: detection onsets, offsets, reference onsets, offsets
    double* d_on = ev + c * SC_MAXEV;
    double* d_off = ev + (NC + c) * SC_MAXEV;
    double* g_on = ev + 2 * NC * SC_MAXEV;                          // + class * SC_MAXEV
    double* g_off = ev + 3 * NC * SC_MAXEV;
    int* s_nref = (int*)(smem + (size_t)NC * SC_MAXEV * 32);        // [SC_MAXNC] references per column (0 for a column not scored)
    int flags = 0;
    int n_est;
    if (a.strong) {
        uint8_t* raw = smem + (size_t)NC * SC_MAXEV * 32 + SC_HEAD + (size_t)c * 2 * a.tpad;
        const int window = a.win[k];
        if (window < 1 || window > 63) flags |= 8;
        const double num = a.num, den = a.den;
        n_est = pp_decode_column(a.strong + (size_t)n * a.T * NC + c, a.T, NC, a.thr[k], min(max(window, 1), 63), raw,
                                 raw + a.tpad, nullptr, [=](int i, int frame, bool is_offset) {
                                     if (i < SC_MAXEV) (is_offset ? d_off : d_on)[i] = (double)frame * num / den;
                                 });
    } else {
        const int e0 = a.est_ptr[col];
        n_est = a.est_ptr[col + 1] - e0;
        if (lane < n_est && n_est <= SC_MAXEV) {
            d_on[lane] = a.est_on[e0 + lane];
            d_off[lane] = a.est_off[e0 + lane];
        }
    }
    const int r0 = a.ref_ptr[col];
    int n_ref = a.ref_ptr[col + 1] - r0;
    if (n_ref > SC_MAXEV) flags |= 1;
    if (n_est > SC_MAXEV) flags |= 2;
    if (n_ref < 0 || n_est < 0) flags |= 16;
    if (flags & (1 | 16)) n_ref = 0;
    if (lane < n_ref) {
        g_on[c * SC_MAXEV + lane] = a.ref_on[r0 + lane];
        g_off[c * SC_MAXEV + lane] = a.ref_off[r0 + lane];
    }
    if (lane == 0) s_nref[c] = n_ref;
    __syncthreads();
    const bool ok = flags == 0;                                            // wave-uniform
    const bool has_est = ok && lane < n_est, has_ref = ok && lane < n_ref;
    if (!ok) n_est = 0;
    double m_on = 0.0, m_off = 0.0;                    // lane e: detection e
    if (has_est) {
        m_on = d_on[lane];
        m_off = d_off[lane];
    }
    const double m_len = m_off - m_on;
    // ---- DTC: detection e is relevant iff its summed intersection with this class's ground truths covers dtc of it --------
    double sum = 0.0;
    for (int g = 0; g < n_ref; ++g) sum += ps_overlap(m_on, m_off, g_on[c * SC_MAXEV + g], g_off[c * SC_MAXEV + g]);
    const unsigned long long relevant = __ballot(has_est && ps_passes(sum, m_len, a.dtc));
    const bool cross = has_est && !((relevant >> lane) & 1);               // a false positive: a cross-trigger candidate
    const unsigned long long any_cross = __ballot(cross);
    int mine = 0;                                      // lane i: value i of this column's (TP, FP, CT[.][0 .. NC - 1])
    if (lane == 1) mine = __popcll(any_cross);
    // ---- GTC: ground truth r is found iff the relevant detections' summed intersection with it covers gtc of it -----------
    {
        double r_on = 0.0, r_off = 0.0;
        if (has_ref) {
            r_on = g_on[c * SC_MAXEV + lane];
            r_off = g_off[c * SC_MAXEV + lane];
        }
        sum = 0.0;
        for (int e = 0; e < n_est; ++e)
            if ((relevant >> e) & 1) sum += ps_overlap(d_on[e], d_off[e], r_on, r_off);
        const int tp = __popcll(__ballot(has_ref && ps_passes(sum, r_off - r_on, a.gtc)));
        if (lane == 0) mine = tp;
    }
    // ---- CTTC: a false positive of class c is a cross-trigger of class j when class j's ground truths cover cttc of it -----
    if (any_cross) {
        for (int j = 0; j < NC; ++j) {
            if (j == c) continue;
            const int nj = s_nref[j];
            sum = 0.0;
            for (int g = 0; g < nj; ++g) sum += ps_overlap(m_on, m_off, g_on[j * SC_MAXEV + g], g_off[j * SC_MAXEV + g]);
            const int ct = __popcll(__ballot(cross && ps_passes(sum, m_len, a.cttc)));
            if (lane == 2 + j) mine = ct;
        }
    }
    if (lane < 2 + NC) {
        const int W = 2 + NC;
        if (a.columns) a.columns[(((size_t)k * N + n) * NC + c) * W + lane] = mine;
        if (mine > 0) atomicAdd(a.totals + ((size_t)k * NC + c) * W + lane, (unsigned long long)mine);
    }
    if (lane == 0 && flags) atomicOr(a.err, flags);
}

// one wave per (threshold set, class): intermediate_at_measures (evaluation_measures.py:86-102) over all clips
__global__ __launch_bounds__(64) void k_weak_counts(const float* __restrict__ weak, const uint8_t* __restrict__ labels,
                                                    const float* __restrict__ thr, int N, int NC,
                                                    unsigned long long* __restrict__ out) {
    const int c = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const float t = thr[(size_t)k * NC + c];
    int tp = 0, fp = 0, fn = 0, tn = 0;
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane;
        const bool valid = n < N;
        const bool pred = valid && weak[(size_t)n * NC + c] > t;
        const bool lab = valid && labels[(size_t)n * NC + c] != 0;
        tp += __popcll(__ballot(pred && lab));
        fp += __popcll(__ballot(pred && !lab));
        fn += __popcll(__ballot(valid && !pred && lab));
        tn += __popcll(__ballot(valid && !pred && !lab));
    }
    if (lane == 0) {
        unsigned long long* o = out + ((size_t)k * NC + c) * 4;
        atomicAdd(o + 0, (unsigned long long)tp);
        atomicAdd(o + 1, (unsigned long long)fp);
        atomicAdd(o + 2, (unsigned long long)fn);
        atomicAdd(o + 3, (unsigned long long)tn);
    }
}

extern "C" int sed_event_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                                const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                                const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                                double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_counts,
                                int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* stream) {
    SED_CHECK_ARG(ref_ptr && ref_on && ref_off && ev_total && seg_total && err, "sed_event_counts: null argument");
    SED_CHECK_ARG(n_clips >= 1 && nclass >= 1 && nclass <= SC_MAXNC, "sed_event_counts: need n_clips >= 1 and 1 <= nclass <= 16");
    SED_CHECK_ARG(t_collar >= 0.0 && percentage_of_length >= 0.0 && time_resolution > 0.0,
                  "sed_event_counts: need t_collar >= 0, percentage_of_length >= 0, time_resolution > 0");
    if (strong) {
        SED_CHECK_ARG(thr && win && n_points >= 1 && n_points <= 65535, "sed_event_counts: need 1 <= n_points <= 65535 operating points");
        SED_CHECK_ARG(T >= 1 && T <= PP_MAXT, "sed_event_counts: need 1 <= T <= 2048 output frames");
        SED_CHECK_ARG(den > 0.0 && num > 0.0, "sed_event_counts: the frame -> second factor num / den must be positive");
    } else {
        SED_CHECK_ARG(est_ptr && est_on && est_off, "sed_event_counts: neither posteriors nor estimated events given");
        SED_CHECK_ARG(n_points == 1, "sed_event_counts: given events are one operating point (n_points = 1)");
    }
    EvArgs a;
    a.strong = strong; a.T = T; a.NC = nclass; a.thr = thr; a.win = win; a.num = num; a.den = den;
    a.est_ptr = est_ptr; a.est_on = est_on; a.est_off = est_off;
    a.ref_ptr = ref_ptr; a.ref_on = ref_on; a.ref_off = ref_off;
    a.t_collar = t_collar; a.pct = percentage_of_length; a.res = time_resolution;
    a.ev_counts = ev_counts; a.seg_counts = seg_counts;
    a.ev_total = (unsigned long long*)ev_total; a.seg_total = (unsigned long long*)seg_total; a.err = err;
    a.tpad = strong ? (T + 1 + 15) / 16 * 16 : 0;
    const size_t lds = (size_t)nclass * SC_MAXEV * 16 + SC_HEAD + (size_t)nclass * 2 * a.tpad;
    if (lds > 64 * 1024) {           // long clips with many classes only: 16 classes x 2048 frames need 82 KB of the CU's 160 KB
        static thread_local SedAttrOnce once;
        if (once.need())
            SED_CHECK_HIP(hipFuncSetAttribute((const void*)k_event_counts, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              SC_MAXNC * SC_MAXEV * 16 + SC_HEAD + SC_MAXNC * 2 * ((PP_MAXT + 16) / 16 * 16)));
    }
    k_event_counts<<<dim3(n_clips, n_points), nclass * 64, lds, (hipStream_t)stream>>>(a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_psds_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                               const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                               const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                               double dtc, double gtc, double cttc, int32_t* columns, int64_t* totals, int32_t* err,
                               void* stream) {
    SED_CHECK_ARG(ref_ptr && ref_on && ref_off && totals && err, "sed_psds_counts: null argument");
    SED_CHECK_ARG(n_clips >= 1 && nclass >= 1 && nclass <= SC_MAXNC, "sed_psds_counts: need n_clips >= 1 and 1 <= nclass <= 16");
    SED_CHECK_ARG(dtc >= 0.0 && dtc <= 1.0 && gtc >= 0.0 && gtc <= 1.0 && cttc >= 0.0 && cttc <= 1.0,
                  "sed_psds_counts: need dtc, gtc and cttc in [0, 1]");
    if (strong) {
        SED_CHECK_ARG(thr && win && n_points >= 1 && n_points <= 65535, "sed_psds_counts: need 1 <= n_points <= 65535 operating points");
        SED_CHECK_ARG(T >= 1 && T <= PP_MAXT, "sed_psds_counts: need 1 <= T <= 2048 output frames");
        SED_CHECK_ARG(den > 0.0 && num > 0.0, "sed_psds_counts: the frame -> second factor num / den must be positive");
    } else {
        SED_CHECK_ARG(est_ptr && est_on && est_off, "sed_psds_counts: neither posteriors nor estimated events given");
        SED_CHECK_ARG(n_points == 1, "sed_psds_counts: given events are one operating point (n_points = 1)");
    }
    PsArgs a;
    a.strong = strong; a.T = T; a.NC = nclass; a.thr = thr; a.win = win; a.num = num; a.den = den;
    a.est_ptr = est_ptr; a.est_on = est_on; a.est_off = est_off;
    a.ref_ptr = ref_ptr; a.ref_on = ref_on; a.ref_off = ref_off;
    a.dtc = dtc; a.gtc = gtc; a.cttc = cttc;
    a.columns = columns; a.totals = (unsigned long long*)totals; a.err = err;
    a.tpad = strong ? (T + 1 + 15) / 16 * 16 : 0;
    const size_t lds = (size_t)nclass * SC_MAXEV * 32 + SC_HEAD + (size_t)nclass * 2 * a.tpad;
    if (lds > 64 * 1024) {           // 16 classes x 2048 frames: 32 KB of events + 65 KB of decode buffers = 97 KB of the CU's 160 KB
        static thread_local SedAttrOnce once;
        if (once.need())
            SED_CHECK_HIP(hipFuncSetAttribute((const void*)k_psds_counts, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              SC_MAXNC * SC_MAXEV * 32 + SC_HEAD + SC_MAXNC * 2 * ((PP_MAXT + 16) / 16 * 16)));
    }
    k_psds_counts<<<dim3(n_clips, n_points), nclass * 64, lds, (hipStream_t)stream>>>(a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_weak_counts(const float* weak, const uint8_t* labels, int n_clips, int nclass, const float* thr,
                               int n_points, int64_t* counts, void* stream) {
    SED_CHECK_ARG(weak && labels && thr && counts, "sed_weak_counts: null argument");
    SED_CHECK_ARG(n_clips >= 1 && nclass >= 1 && nclass <= 65535 && n_points >= 1 && n_points <= 65535,
                  "sed_weak_counts: need n_clips >= 1, 1 <= nclass, n_points <= 65535");
    k_weak_counts<<<dim3(nclass, n_points), 64, 0, (hipStream_t)stream>>>(weak, labels, thr, n_clips, nclass,
                                                                          (unsigned long long*)counts);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
