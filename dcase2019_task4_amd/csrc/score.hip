// score.hip - validation scoring on the device: event-based, segment-based and clip-level (weak) counts, and the PSDS
// intersection counts (k_psds_counts, further down) and the counts of the overall error rate with substitutions
// (k_error_counts, after it).
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
//     events are broadcast LDS reads).  Ntp = size of a maximum bipartite matching: sc_max_matching (score.h, shared with
//     lscore.hip, as are the compatibility test, the limits and the error bits) - augmenting paths on wave-uniform masks;
//   segment-based: lane s is segment s0 + s; an event covers segments max(0, floor(on / res)) .. ceil(off / res) - 1; the file's
//     segment count (for Ntn) is the maximum over the workgroup's columns, reduced through LDS.
// All counts are integers and the class totals are integer atomics, so results are bit-reproducible run to run.
#pragma clang fp contract(off)       // seconds are formed as (double)frame * num / den, exactly the host's two operations
#include "common.h"
#include "kernels.h"
#include "post.h"
#include "score.h"

#define SC_HEAD (SC_MAXNC * 4)       // bytes of the per-column integers in front of the decode buffers

// what both clip kernels are given first: the estimated side (posteriors to decode, or CSR events) and the reference side
struct ScArgs {
    const float* strong; int T, NC; const float* thr; const int32_t* win; double num, den;
    const int32_t* est_ptr; const double *est_on, *est_off;
    const int32_t* ref_ptr; const double *ref_on, *ref_off;
};
// (err and tpad stay behind each kernel's own criteria and outputs: the kernels fetch their arguments in the pattern they
// always had, one wide scalar load over est_on .. the criteria)
struct EvArgs {
    ScArgs s;
    double t_collar, pct, res;
    int32_t *ev_counts, *seg_counts; unsigned long long *ev_total, *seg_total; int32_t* err;
    int tpad;                        // bytes of one raw / flt buffer (0 when the events are given)
};

struct ScColumn { int n_est, r0, n_ref, flags; };

__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// One wave's column (clip blockIdx.x, class threadIdx.x / 64) at operating point blockIdx.y: its estimated events, decoded
// with pp_decode_column or loaded from the CSR, go to e_on / e_off[0 .. min(n_est, 64)) as fp64 seconds.  `dec` is the
// workgroup's decode area, 2 * tpad bytes per wave.  Called by all 64 lanes of every wave of the workgroup (the decode
// contains workgroup barriers); the caller places the barrier that publishes e_on / e_off.  Returns the column's counts,
// the offset of its reference events and the error bits 1, 2, 8, 16 it raises.
__device__ __forceinline__ ScColumn sc_stage_column(const ScArgs& a, int tpad, uint8_t* dec, double* e_on, double* e_off) {
    const int n = blockIdx.x, k = blockIdx.y, c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = n * a.NC + c;
    ScColumn s;
    s.flags = 0;
    if (a.strong) {
        uint8_t* raw = dec + (size_t)c * 2 * tpad;
        const int window = a.win[k];
        if (window < 1 || window > 63) s.flags |= SC_ERR_WINDOW;
        const double num = a.num, den = a.den;
        s.n_est = pp_decode_column(a.strong + (size_t)n * a.T * a.NC + c, a.T, a.NC, a.thr[k], min(max(window, 1), 63), raw,
                                   raw + tpad, nullptr, [=](int i, int frame, bool is_offset) {
                                       if (i < SC_MAXEV) (is_offset ? e_off : e_on)[i] = (double)frame * num / den;
                                   });
    } else {
        const int e0 = a.est_ptr[col];
        s.n_est = a.est_ptr[col + 1] - e0;
        if (lane < s.n_est && s.n_est <= SC_MAXEV) {
            e_on[lane] = a.est_on[e0 + lane];
            e_off[lane] = a.est_off[e0 + lane];
        }
    }
    s.r0 = a.ref_ptr[col];
    s.n_ref = a.ref_ptr[col + 1] - s.r0;
    if (s.n_ref > SC_MAXEV) s.flags |= SC_ERR_MANY_REF;
    if (s.n_est > SC_MAXEV) s.flags |= SC_ERR_MANY_EST;
    if (s.n_ref < 0 || s.n_est < 0) s.flags |= SC_ERR_OFFSETS;
    return s;
}

__global__ __launch_bounds__(1024) void k_event_counts(EvArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int NC = a.s.NC, n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* e_on = (double*)smem + c * SC_MAXEV;                    // [NC][64] onsets, then [NC][64] offsets
    double* e_off = (double*)smem + (NC + c) * SC_MAXEV;
    int* s_nseg = (int*)(smem + (size_t)NC * SC_MAXEV * 16);        // [SC_MAXNC]
    const ScColumn col = sc_stage_column(a.s, a.tpad, smem + (size_t)NC * SC_MAXEV * 16 + SC_HEAD, e_on, e_off);
    __syncthreads();
    const int r0 = col.r0, n_ref = col.n_ref, n_est = col.n_est;
    int flags = col.flags;
    const bool ok = flags == 0;                                            // wave-uniform
    const bool has_ref = ok && lane < n_ref, has_est = ok && lane < n_est;
    double r_on = 0.0, r_off = 0.0;
    if (has_ref) {
        r_on = a.s.ref_on[r0 + lane];
        r_off = a.s.ref_off[r0 + lane];
    }
    // ---- event-based: compatibility masks, then a maximum matching by augmenting paths ---------------------------------
    int ntp = 0;
    if (ok) {
        const double tol_off = sc_offset_tolerance(r_on, r_off, a.t_collar, a.pct);
        unsigned long long adj = 0;                                  // bit e: estimated event e is compatible with my reference
        for (int e = 0; e < n_est; ++e) {
            const bool hit = has_ref && sc_compatible(r_on, r_off, tol_off, e_on, e_off, e, a.t_collar);
            adj |= (unsigned long long)hit << e;
        }
        ntp = sc_max_matching(adj, n_est, lane);
    }
    // ---- segment-based ---------------------------------------------------------------------------------------------------
    int rlo = 0, rhi = 0, elo = 0, ehi = 0;
    if (has_ref) {
        rlo = sc_seg_index(floor(r_on / a.res));
        rhi = sc_seg_index(ceil(r_off / a.res));
    }
    if (has_est) {
        elo = sc_seg_index(floor(e_on[lane] / a.res));
        ehi = sc_seg_index(ceil(e_off[lane] / a.res));
    }
    const int col_seg = wave_imax(max(rhi, ehi));
    if (col_seg > SC_MAXSEG) flags |= SC_ERR_SEGMENTS;
    if (lane == 0) s_nseg[c] = col_seg;
    __syncthreads();
    const int file_seg = wave_imax(lane < NC ? s_nseg[lane] : 0);
    int tp = 0, fp = 0, fn = 0, tn = 0;
    if (ok && file_seg <= SC_MAXSEG) {
        for (int s0 = 0; s0 < col_seg; s0 += 64) {
            const int s = s0 + lane;
            bool ra = false, ea = false;
            for (int r = 0; r < n_ref; ++r) ra |= s >= sc_lane_read(rlo, r) && s < sc_lane_read(rhi, r);
            for (int e = 0; e < n_est; ++e) ea |= s >= sc_lane_read(elo, e) && s < sc_lane_read(ehi, e);
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
    ScArgs s;
    double dtc, gtc, cttc;
    int32_t* columns; unsigned long long* totals; int32_t* err;
    int tpad;                        // bytes of one raw / flt buffer (0 when the events are given)
};

__global__ __launch_bounds__(1024) void k_psds_counts(PsArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int NC = a.s.NC, n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* ev = (double*)smem;                                     // [4][NC][64]: detection onsets, offsets, reference onsets, offsets
    double* d_on = ev + c * SC_MAXEV;
    double* d_off = ev + (NC + c) * SC_MAXEV;
    double* g_on = ev + 2 * NC * SC_MAXEV;                          // + class * SC_MAXEV
    double* g_off = ev + 3 * NC * SC_MAXEV;
    int* s_nref = (int*)(smem + (size_t)NC * SC_MAXEV * 32);        // [SC_MAXNC] references per column (0 for a column not scored)
    const ScColumn col = sc_stage_column(a.s, a.tpad, smem + (size_t)NC * SC_MAXEV * 32 + SC_HEAD, d_on, d_off);
    const int r0 = col.r0, flags = col.flags;
    int n_est = col.n_est, n_ref = col.n_ref;
    if (flags & (SC_ERR_MANY_REF | SC_ERR_OFFSETS)) n_ref = 0;
    if (lane < n_ref) {
        g_on[c * SC_MAXEV + lane] = a.s.ref_on[r0 + lane];
        g_off[c * SC_MAXEV + lane] = a.s.ref_off[r0 + lane];
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
    for (int g = 0; g < n_ref; ++g) sum += sc_overlap(m_on, m_off, g_on[c * SC_MAXEV + g], g_off[c * SC_MAXEV + g]);
    const unsigned long long relevant = __ballot(has_est && sc_passes(sum, m_len, a.dtc));
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
            if ((relevant >> e) & 1) sum += sc_overlap(d_on[e], d_off[e], r_on, r_off);
        const int tp = __popcll(__ballot(has_ref && sc_passes(sum, r_off - r_on, a.gtc)));
        if (lane == 0) mine = tp;
    }
    // ---- CTTC: a false positive of class c is a cross-trigger of class j when class j's ground truths cover cttc of it -----
    if (any_cross) {
        for (int j = 0; j < NC; ++j) {
            if (j == c) continue;
            const int nj = s_nref[j];
            sum = 0.0;
            for (int g = 0; g < nj; ++g) sum += sc_overlap(m_on, m_off, g_on[j * SC_MAXEV + g], g_off[j * SC_MAXEV + g]);
            const int ct = __popcll(__ballot(cross && sc_passes(sum, m_len, a.cttc)));
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

// ---- overall error rate with substitutions ----------------------------------------------------------------------------------
// (include/dcase_sed.h, "overall error rate", holds the definitions and the decision about sed_eval's greedy count.)
//
// k_error_counts: the grid and the decode of k_event_counts, both sides of all the clip's classes staged in LDS as in
// k_psds_counts.  Then the labels are dropped:
//   event-based: thread (class c, lane i) owns estimated event i and reference event i of class c and ranks each among ALL the
//     clip's events of its side by (onset, class, index) - a count over broadcast LDS reads, no assumption about the order
//     inside a column - and writes it to its rank in the merged lists (they take the place of the decode buffers).  Wave w
//     then owns the merged references 64 w .. 64 w + 63: sc_match_tile, the code k_ls_match runs on a long column.
//     Nany = the sum over the waves.  A merged cluster beyond 64 per side raises bit 1 / 2; the clip is then not scored.
//   segment-based: one thread per segment; the events' segment ranges (ints, in place of the staged seconds) give a 16-bit
//     mask of active classes per side, and sc_segment_sdi the segment's part of (S, D, I).
// The workgroup's sums are integer LDS atomics, the totals integer global atomics: bit-reproducible.
struct ErArgs {
    ScArgs s;
    double t_collar, pct, res;
    int32_t *ev_overall, *seg_overall; unsigned long long *ev_total, *seg_total; int32_t* err;
    int tpad;                        // bytes of one raw / flt buffer, at least ER_TPAD: two of them per class hold the merged lists
};
#define ER_HEAD 256                  // int32: [0, 16) n_est, [16, 32) n_ref per class, then file segments, flags, Nany, S, D, I
#define ER_TPAD (SC_MAXEV * 16)      // per class 64 events x (onset, offset) x 2 sides of fp64 = 2 * ER_TPAD bytes

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the number of events (c2, i2) of x[NC][64] (n[c2] of them in class c2) in front of event (c, i) with onset `on`, by
// (onset, class, index)
__device__ __forceinline__ int er_rank(const double* x, const int* n, int NC, double on, int c, int i) {
    int rank = 0;
    for (int c2 = 0; c2 < NC; ++c2) {
        const int n2 = n[c2];
        for (int i2 = 0; i2 < n2; ++i2) {
            const double o = x[c2 * SC_MAXEV + i2];
            rank += o < on || (o == on && (c2 < c || (c2 == c && i2 < i)));
        }
    }
    return rank;
}

__global__ __launch_bounds__(1024) void k_error_counts(ErArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int NC = a.s.NC, n = blockIdx.x, k = blockIdx.y, N = gridDim.x;
    const int tid = threadIdx.x, c = tid >> 6, lane = tid & 63;
    double* ev = (double*)smem;                                     // [4][NC][64]: estimated onsets, offsets, reference onsets, offsets
    int* hd = (int*)(smem + (size_t)NC * SC_MAXEV * 32);
    int *s_nest = hd, *s_nref = hd + SC_MAXNC, *s_acc = hd + 2 * SC_MAXNC;      // s_acc: file segments, flags, Nany, S, D, I
    uint8_t* dec = smem + (size_t)NC * SC_MAXEV * 32 + ER_HEAD;
    if (tid < 6) s_acc[tid] = 0;
    const ScColumn col = sc_stage_column(a.s, a.tpad, dec, ev + c * SC_MAXEV, ev + (NC + c) * SC_MAXEV);
    const int n_est = col.n_est, n_ref = col.n_ref;
    if (lane < n_ref && n_ref <= SC_MAXEV) {
        ev[(2 * NC + c) * SC_MAXEV + lane] = a.s.ref_on[col.r0 + lane];
        ev[(3 * NC + c) * SC_MAXEV + lane] = a.s.ref_off[col.r0 + lane];
    }
    if (lane == 0) {
        s_nest[c] = max(n_est, 0);
        s_nref[c] = max(n_ref, 0);
        if (col.flags) atomicOr(a.err, col.flags);
    }
    const bool bad_column = __syncthreads_or(col.flags != 0);       // (the barrier that publishes the staged events)
    int n_sys = 0, n_all_ref = 0;
    for (int c2 = 0; c2 < NC; ++c2) {
        n_sys += s_nest[c2];
        n_all_ref += s_nref[c2];
    }
    if (!bad_column) {                                              // every column holds 0 .. 64 events per side
        const bool has_est = lane < n_est, has_ref = lane < n_ref;
        double e_on = 0.0, e_off = 0.0, r_on = 0.0, r_off = 0.0;
        if (has_est) {
            e_on = ev[c * SC_MAXEV + lane];
            e_off = ev[(NC + c) * SC_MAXEV + lane];
        }
        if (has_ref) {
            r_on = ev[(2 * NC + c) * SC_MAXEV + lane];
            r_off = ev[(3 * NC + c) * SC_MAXEV + lane];
        }
        // ---- merge by onset: the decode buffers are dead, the merged lists take their place --------------------------------
        const int cap = NC * SC_MAXEV;
        double* m_ron = (double*)dec;                               // [cap] each
        double *m_roff = m_ron + cap, *m_eon = m_ron + 2 * cap, *m_eoff = m_ron + 3 * cap;
        if (has_est) {
            const int at = er_rank(ev, s_nest, NC, e_on, c, lane);
            m_eon[at] = e_on;
            m_eoff[at] = e_off;
        }
        if (has_ref) {
            const int at = er_rank(ev + 2 * NC * SC_MAXEV, s_nref, NC, r_on, c, lane);
            m_ron[at] = r_on;
            m_roff[at] = r_off;
        }
        int rlo = 0, rhi = 0, elo = 0, ehi = 0;
        if (has_ref) {
            rlo = sc_seg_index(floor(r_on / a.res));
            rhi = sc_seg_index(ceil(r_off / a.res));
        }
        if (has_est) {
            elo = sc_seg_index(floor(e_on / a.res));
            ehi = sc_seg_index(ceil(e_off / a.res));
        }
        const int col_seg = wave_imax(max(rhi, ehi));
        if (lane == 0 && col_seg > 0) atomicMax(&s_acc[0], col_seg);
        __syncthreads();                                            // the merged lists are complete, the staged seconds are dead
        int* sg = (int*)smem;                                       // [4][NC][64]: estimated first / end segment, reference first / end
        sg[c * SC_MAXEV + lane] = elo;
        sg[(NC + c) * SC_MAXEV + lane] = ehi;
        sg[(2 * NC + c) * SC_MAXEV + lane] = rlo;
        sg[(3 * NC + c) * SC_MAXEV + lane] = rhi;
        // ---- event-based: wave c owns the merged references 64 c .. 64 c + 63 ----------------------------------------------
        if (c * SC_MAXEV < n_all_ref) {                             // wave-uniform
            int flags = 0;
            const int got = sc_match_tile(m_ron, m_roff, n_all_ref, m_eon, m_eoff, n_sys, c * SC_MAXEV, a.t_collar, a.pct, lane,
                                          flags);
            if (lane == 0) {
                if (got > 0) atomicAdd(&s_acc[2], got);
                if (flags) atomicOr(&s_acc[1], flags);
            }
        }
        __syncthreads();
        // ---- segment-based: one thread per segment ---------------------------------------------------------------------------
        const int file_seg = s_acc[0];
        if (file_seg > SC_MAXSEG) {
            if (tid == 0) s_acc[1] |= SC_ERR_SEGMENTS;
        } else {
            int S = 0, D = 0, I = 0;
            for (int s = tid; s < file_seg; s += NC * 64) {
                unsigned ref_mask = 0, est_mask = 0;
                for (int c2 = 0; c2 < NC; ++c2) {
                    bool ea = false, ra = false;
                    for (int e = 0; e < s_nest[c2]; ++e) ea |= s >= sg[c2 * SC_MAXEV + e] && s < sg[(NC + c2) * SC_MAXEV + e];
                    for (int r = 0; r < s_nref[c2]; ++r)
                        ra |= s >= sg[(2 * NC + c2) * SC_MAXEV + r] && s < sg[(3 * NC + c2) * SC_MAXEV + r];
                    est_mask |= (unsigned)ea << c2;
                    ref_mask |= (unsigned)ra << c2;
                }
                sc_segment_sdi(ref_mask, est_mask, S, D, I);
            }
            S = wave_isum(S); D = wave_isum(D); I = wave_isum(I);
            if (lane == 0) {
                if (S) atomicAdd(&s_acc[3], S);
                if (D) atomicAdd(&s_acc[4], D);
                if (I) atomicAdd(&s_acc[5], I);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int flags = bad_column ? 0 : s_acc[1];                // (a column's own bits went to err above)
        const bool ok = !bad_column && flags == 0;
        const size_t o = (size_t)k * N + n;
        const int evo[3] = {n_all_ref, n_sys, ok ? s_acc[2] : 0};
        const int sgo[3] = {ok ? s_acc[3] : 0, ok ? s_acc[4] : 0, ok ? s_acc[5] : 0};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (a.ev_overall) a.ev_overall[o * 3 + i] = evo[i];
            if (evo[i] > 0) atomicAdd(a.ev_total + (size_t)k * 3 + i, (unsigned long long)evo[i]);
            if (a.seg_overall) a.seg_overall[o * 3 + i] = sgo[i];
            if (sgo[i] > 0) atomicAdd(a.seg_total + (size_t)k * 3 + i, (unsigned long long)sgo[i]);
        }
        if (flags) atomicOr(a.err, flags);
    }
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

// ---- host: the two clip entry points share the checks of the estimated and the reference side, and their launch --------------
#define SC_NEED(cond, msg)                                                     \
    do {                                                                       \
        if (!(cond)) {                                                         \
            sed_set_error("%s:%d: %s: " msg, __FILE__, __LINE__, what);        \
            return SED_ERR_BAD_ARG;                                            \
        }                                                                      \
    } while (0)

static int sc_fill(ScArgs& s, const char* what, const float* strong, int n_clips, int T, int nclass, int n_points,
                   const float* thr, const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                   const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off) {
    SC_NEED(ref_ptr && ref_on && ref_off, "null argument");
    SC_NEED(n_clips >= 1 && nclass >= 1 && nclass <= SC_MAXNC, "need n_clips >= 1 and 1 <= nclass <= 16");
    if (strong) {
        SC_NEED(thr && win && n_points >= 1 && n_points <= 65535, "need 1 <= n_points <= 65535 operating points");
        SC_NEED(T >= 1 && T <= PP_MAXT, "need 1 <= T <= 2048 output frames");
        SC_NEED(den > 0.0 && num > 0.0, "the frame -> second factor num / den must be positive");
    } else {
        SC_NEED(est_ptr && est_on && est_off, "neither posteriors nor estimated events given");
        SC_NEED(n_points == 1, "given events are one operating point (n_points = 1)");
    }
    s.strong = strong; s.T = T; s.NC = nclass; s.thr = thr; s.win = win; s.num = num; s.den = den;
    s.est_ptr = est_ptr; s.est_on = est_on; s.est_off = est_off;
    s.ref_ptr = ref_ptr; s.ref_on = ref_on; s.ref_off = ref_off;
    return SED_OK;
}
static int sc_tpad(const float* strong, int T) { return strong ? (T + 1 + 15) / 16 * 16 : 0; }

// One workgroup per (clip, operating point), one wave per class; SLOT = bytes of LDS per event slot in front of SC_HEAD and
// the decode buffers.  A template on the kernel: each kernel has its own once-flag for its own raised LDS limit.
template <class Args, void (*KERNEL)(Args), int SLOT, int HEAD = SC_HEAD>
static int sc_launch(const Args& a, int n_clips, int n_points, void* stream) {
    const int nclass = a.s.NC;
    const size_t lds = (size_t)nclass * SC_MAXEV * SLOT + HEAD + (size_t)nclass * 2 * a.tpad;
    if (lds > 64 * 1024) {           // long clips with many classes only: at 16 classes x 2048 frames k_event_counts needs 82 KB
                                     // and k_psds_counts (32 KB of events + 65 KB of decode buffers) 97 KB of the CU's 160 KB
        static thread_local SedAttrOnce once;
        if (once.need())
            SED_CHECK_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              SC_MAXNC * SC_MAXEV * SLOT + HEAD + SC_MAXNC * 2 * ((PP_MAXT + 16) / 16 * 16)));
    }
    KERNEL<<<dim3(n_clips, n_points), nclass * 64, lds, (hipStream_t)stream>>>(a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_event_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                                const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                                const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                                double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_counts,
                                int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* stream) {
    SED_CHECK_ARG(ev_total && seg_total && err, "sed_event_counts: null argument");
    SED_CHECK_ARG(t_collar >= 0.0 && percentage_of_length >= 0.0 && time_resolution > 0.0,
                  "sed_event_counts: need t_collar >= 0, percentage_of_length >= 0, time_resolution > 0");
    EvArgs a;
    SED_TRY(sc_fill(a.s, "sed_event_counts", strong, n_clips, T, nclass, n_points, thr, win, num, den, est_ptr, est_on,
                    est_off, ref_ptr, ref_on, ref_off));
    a.t_collar = t_collar; a.pct = percentage_of_length; a.res = time_resolution;
    a.ev_counts = ev_counts; a.seg_counts = seg_counts;
    a.ev_total = (unsigned long long*)ev_total; a.seg_total = (unsigned long long*)seg_total; a.err = err;
    a.tpad = sc_tpad(strong, T);
    return sc_launch<EvArgs, k_event_counts, 16>(a, n_clips, n_points, stream);
}

extern "C" int sed_error_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                                const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                                const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                                double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_overall,
                                int32_t* seg_overall, int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err,
                                void* stream) {
    SED_CHECK_ARG(ev_overall_total && seg_overall_total && err, "sed_error_counts: null argument");
    SED_CHECK_ARG(t_collar >= 0.0 && percentage_of_length >= 0.0 && time_resolution > 0.0,
                  "sed_error_counts: need t_collar >= 0, percentage_of_length >= 0, time_resolution > 0");
    ErArgs a;
    SED_TRY(sc_fill(a.s, "sed_error_counts", strong, n_clips, T, nclass, n_points, thr, win, num, den, est_ptr, est_on,
                    est_off, ref_ptr, ref_on, ref_off));
    a.t_collar = t_collar; a.pct = percentage_of_length; a.res = time_resolution;
    a.ev_overall = ev_overall; a.seg_overall = seg_overall;
    a.ev_total = (unsigned long long*)ev_overall_total; a.seg_total = (unsigned long long*)seg_overall_total; a.err = err;
    a.tpad = sc_tpad(strong, T) > ER_TPAD ? sc_tpad(strong, T) : ER_TPAD;
    return sc_launch<ErArgs, k_error_counts, 32, ER_HEAD>(a, n_clips, n_points, stream);
}

extern "C" int sed_psds_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                               const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                               const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                               double dtc, double gtc, double cttc, int32_t* columns, int64_t* totals, int32_t* err,
                               void* stream) {
    SED_CHECK_ARG(totals && err, "sed_psds_counts: null argument");
    SED_CHECK_ARG(dtc >= 0.0 && dtc <= 1.0 && gtc >= 0.0 && gtc <= 1.0 && cttc >= 0.0 && cttc <= 1.0,
                  "sed_psds_counts: need dtc, gtc and cttc in [0, 1]");
    PsArgs a;
    SED_TRY(sc_fill(a.s, "sed_psds_counts", strong, n_clips, T, nclass, n_points, thr, win, num, den, est_ptr, est_on,
                    est_off, ref_ptr, ref_on, ref_off));
    a.dtc = dtc; a.gtc = gtc; a.cttc = cttc;
    a.columns = columns; a.totals = (unsigned long long*)totals; a.err = err;
    a.tpad = sc_tpad(strong, T);
    return sc_launch<PsArgs, k_psds_counts, 32>(a, n_clips, n_points, stream);
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
