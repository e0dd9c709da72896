// lscore.hip - scoring of long recordings on the device: event-based, segment-based and PSDS counts of (recording, class)
// columns of ANY length (sed_long_event_counts, sed_long_psds_counts; the definitions are those of score.hip, stated in
// include/dcase_sed.h, without the limit of 64 events per column).  The estimated events are sed_stitch_decode's table
// (ev_ptr / ev_pairs, frames) or CSR fp64 seconds; both sides of a column are sorted by onset.
//
// The sweep calls (sed_long_sweep_*) score K estimated tables - one CSR over the columns (k, rec, c) - against ONE reference
// side with the same kernels: an estimated column's reference column is its index modulo n_rec * NC, and everything that
// derives from the reference alone is done once per call.  The one-point calls are K = 1.
//
// Every launch has one kind of worker and no data passes between workgroups inside a launch:
//   k_ls_prep      one workgroup per estimated column of every point and per reference column: validates the CSR offsets, turns frames into seconds, checks that the
//                  onsets do not decrease and writes pmax[i] = max(offset[0 .. i]) (a workgroup scan, 1024 events per step);
//                  the only pass that walks a column in sequence
//   k_ls_match     one wave per tile of LS_TILE reference events.  "i starts a cluster" is a local test (two bisections in
//                  the estimated onsets), so a wave finds the clusters that START in its tile with one ballot, their ends with
//                  a second ballot over the next tile (further ones only on the error path), and solves each with sc_max_matching
//                  (score.h: sc_match_tile, which k_error_counts runs on a clip's merged lists as well)
//   k_ls_segments  one thread per segment: segment s is covered iff the last event whose first segment is <= s has
//                  seg(pmax) > s - two bisections, no bitmap, no events x segments loop
//   k_lp_detect    one thread per detection: DTC and, for the non-relevant ones, CTTC against every other class
//   k_lp_truth     one thread per ground truth: GTC over the relevant detections
//   k_ls_final / k_lp_final   per-column outputs and the class totals
//   k_le_*         the overall error rate with substitutions (sed_long_error_counts, sed_long_sweep_error_counts): further down
// The PSDS sums skip events that cannot overlap (bisection on the onsets for the upper end, on pmax for the lower end):
// every skipped term is +0.0 and the sum starts at 0.0, so the bits are those of the full sequential sum.
// Counts are integers, the atomics are integer atomics: results are bit-reproducible.  Every offset is validated against the
// capacities the caller passed before it is used as an index.
#pragma clang fp contract(off)       // seconds are formed as (double)frame * num / den, exactly the host's two operations
#include "common.h"
#include "kernels.h"
#include "score.h"

#define LS_TILE 64                   // reference events per wave of k_ls_match: one lane / one mask bit each
static_assert(LS_TILE == SC_MAXEV, "a tile of references is one adjacency mask's worth of lanes");
#define LS_CW 20                     // int32 counters per column: [0] Ntp, [1..3] segment tp / fp / fn, [4] k_ls_match's err bits; PSDS: [0 .. 2 + NC)
#define LS_PREP_THREADS 1024
#define LS_SEG_SPLIT 16              // workgroups of 256 segments per column and step

struct LsArgs {
    const int64_t* est_ptr; const int32_t* ev_pairs; double num, den;
    const double *est_on, *est_off;  // the given seconds, or the workspace copies of the frames
    const int64_t* ref_ptr; const double *ref_on, *ref_off;
    long long est_cap, ref_cap;
    int n_rec, NC, n_slots;          // n_slots: tiles of reference events, per point
    int K;                           // operating points: estimated column (k, rec, c) is scored against reference column (rec, c)
    double t_collar, pct, res, dtc, gtc, cttc;
    int32_t* flags;                  // ws [K * ncols]: err bits of an estimated column, written by k_ls_prep
    int32_t* rflags;                 // ws [ncols]: the same of a reference column
    int32_t* cnt;                    // ws [K * ncols][LS_CW]
    double *ws_on, *ws_off;          // ws [est_cap] each (frames mode)
    double *est_pmax, *ref_pmax;     // ws [est_cap], [ref_cap]
    uint8_t* rel;                    // ws [est_cap]: detection is relevant (PSDS)
    int32_t *out_a, *out_b;          // ev_counts / seg_counts, or columns / unused
    unsigned long long *tot_a, *tot_b;
    int32_t* err;
};

// validated range of a column: false (and an empty range) when the offsets are malformed
__device__ __forceinline__ bool ls_range(const int64_t* ptr, long long col, long long cap, long long& p0, int& n) {
    const long long a = ptr[col], b = ptr[col + 1];
    const bool ok = a >= 0 && b >= a && b <= cap;
    p0 = ok ? a : 0;
    n = ok ? (int)(b - a) : 0;
    return ok;
}
// the reference column of an estimated column, and the err bits that keep the pair from being scored
__device__ __forceinline__ long long ls_rcol(const LsArgs& a, long long ecol) { return ecol % ((long long)a.n_rec * a.NC); }
__device__ __forceinline__ int ls_col_flags(const LsArgs& a, long long ecol) { return a.flags[ecol] | a.rflags[ls_rcol(a, ecol)]; }

__global__ __launch_bounds__(LS_PREP_THREADS) void k_ls_prep(LsArgs a) {
    __shared__ double part[LS_PREP_THREADS / 64];
    __shared__ double s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_est_cols = (long long)a.K * a.n_rec * a.NC;
    const int side = blockIdx.x >= n_est_cols;                       // 0: estimated (every point's columns), 1: reference (once)
    const long long col = side ? blockIdx.x - n_est_cols : blockIdx.x;
    const bool frames = side == 0 && a.ev_pairs != nullptr;
    long long p0;
    int n, flags = 0;
    if (!ls_range(side ? a.ref_ptr : a.est_ptr, col, side ? a.ref_cap : a.est_cap, p0, n)) flags = SC_ERR_OFFSETS;
    const double* src_on = side ? a.ref_on : a.est_on;
    const double* src_off = side ? a.ref_off : a.est_off;
    double* pmax = side ? a.ref_pmax : a.est_pmax;
    if (tid == 0) s_carry = -INFINITY;
    if (side == 0)
        for (int i = tid; i < LS_CW; i += LS_PREP_THREADS) a.cnt[col * LS_CW + i] = 0;
    __syncthreads();
    const double num = a.num, den = a.den;
    int unsorted = 0;
    for (int k0 = 0; k0 < n; k0 += LS_PREP_THREADS) {
        const int k = k0 + tid;
        const bool valid = k < n;
        const long long i = p0 + k;
        double on = 0.0, off = -INFINITY;
        if (valid) {
            double prev;
            if (frames) {
                on = (double)a.ev_pairs[2 * i] * num / den;
                off = (double)a.ev_pairs[2 * i + 1] * num / den;
                prev = k > 0 ? (double)a.ev_pairs[2 * i - 2] * num / den : on;
                a.ws_on[i] = on;
                a.ws_off[i] = off;
            } else {
                on = src_on[i];
                off = src_off[i];
                prev = k > 0 ? src_on[i - 1] : on;
            }
            unsorted |= on < prev;
        }
        double incl = off;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double m = __shfl_up(incl, o);
            if (lane >= o) incl = fmax(incl, m);
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        double v = s_carry;
        for (int w = 0; w < wave; ++w) v = fmax(v, part[w]);
        v = fmax(v, incl);
        if (valid) pmax[i] = v;
        __syncthreads();
        if (tid == LS_PREP_THREADS - 1) s_carry = v;
        __syncthreads();
    }
    if (__syncthreads_or(unsorted)) flags |= SC_ERR_UNSORTED;
    if (tid == 0) {
        (side ? a.rflags : a.flags)[col] = flags;
        if (flags) atomicOr(a.err, flags);
    }
}

// The clusters between the valid cuts of a column and their matching: sc_match_tile (score.h).
__global__ __launch_bounds__(256) void k_ls_match(LsArgs a) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (long long)a.K * a.n_slots) return;
    const int kp = (int)(g / a.n_slots);
    const long long gl = g - (long long)kp * a.n_slots;
    const long long ncols = (long long)a.n_rec * a.NC;
    long long lo_c = 0, hi_c = ncols - 1;
    while (lo_c < hi_c) {                                            // the last column with slot0(col) <= g
        const long long mid = (lo_c + hi_c + 1) >> 1;
        if (a.ref_ptr[mid] / LS_TILE + mid <= gl) lo_c = mid;
        else hi_c = mid - 1;
    }
    const long long rcol = lo_c, col = kp * ncols + rcol;
    if (a.flags[col] | a.rflags[rcol]) return;                       // not scored (k_ls_prep reported it)
    long long pr, pe;
    int n_ref, n_est;
    ls_range(a.ref_ptr, rcol, a.ref_cap, pr, n_ref);
    ls_range(a.est_ptr, col, a.est_cap, pe, n_est);
    const long long kt = gl - (pr / LS_TILE + rcol);
    if (kt < 0 || kt * LS_TILE >= n_ref) return;
    const int i_base = (int)kt * LS_TILE;
    int flags = 0;
    const int ntp = sc_match_tile(a.ref_on + pr, a.ref_off + pr, n_ref, a.est_on + pe, a.est_off + pe, n_est, i_base, a.t_collar,
                                  a.pct, lane, flags);
    if (lane == 0) {
        if (ntp > 0) atomicAdd(a.cnt + col * LS_CW, ntp);
        if (flags) {
            atomicOr(a.cnt + col * LS_CW + 4, flags);    // only k_ls_final, a later launch, reads it
            atomicOr(a.err, flags);
        }
    }
}

// ceil(max offset / res) of one estimated column and its reference column, and of the whole recording at one point
// (rec = k * n_rec + recording)
__device__ __forceinline__ int ls_col_segments(const LsArgs& a, long long col) {
    long long p0;
    int n, seg = 0;
    if (ls_range(a.est_ptr, col, a.est_cap, p0, n) && n > 0) seg = sc_seg_index(ceil(a.est_pmax[p0 + n - 1] / a.res));
    if (ls_range(a.ref_ptr, ls_rcol(a, col), a.ref_cap, p0, n) && n > 0)
        seg = max(seg, sc_seg_index(ceil(a.ref_pmax[p0 + n - 1] / a.res)));
    return seg;
}
__device__ __forceinline__ int ls_file_segments(const LsArgs& a, long long rec) {
    int seg = 0;
    for (int c = 0; c < a.NC; ++c) seg = max(seg, ls_col_segments(a, rec * a.NC + c));
    return seg;
}
// is segment s covered by the events on[0 .. n) (sorted), pmax their running maximum offset
__device__ __forceinline__ bool ls_covered(const double* on, const double* pmax, int n, int s, double res) {
    int lo = 0, hi = n;
    while (lo < hi) {                                                // the number of events whose first segment is <= s
        const int mid = (lo + hi) >> 1;
        if (sc_seg_index(floor(on[mid] / res)) <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && sc_seg_index(ceil(pmax[lo - 1] / res)) > s;
}

__global__ __launch_bounds__(256) void k_ls_segments(LsArgs a) {
    const long long col = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int file_seg = ls_file_segments(a, col / a.NC);
    if (file_seg > SC_MAXSEG) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicOr(a.err, SC_ERR_SEGMENTS);
        return;
    }
    if (ls_col_flags(a, col)) return;
    const int col_seg = ls_col_segments(a, col);
    long long pr, pe;
    int n_ref, n_est;
    ls_range(a.ref_ptr, ls_rcol(a, col), a.ref_cap, pr, n_ref);
    ls_range(a.est_ptr, col, a.est_cap, pe, n_est);
    int tp = 0, fp = 0, fn = 0;
    for (int s0 = blockIdx.y * 256; s0 < col_seg; s0 += LS_SEG_SPLIT * 256) {
        const int s = s0 + threadIdx.x;
        const bool in = s < col_seg;
        const bool ra = in && ls_covered(a.ref_on + pr, a.ref_pmax + pr, n_ref, s, a.res);
        const bool ea = in && ls_covered(a.est_on + pe, a.est_pmax + pe, n_est, s, a.res);
        tp += __popcll(__ballot(ra && ea));
        fp += __popcll(__ballot(ea && !ra));
        fn += __popcll(__ballot(ra && !ea));
    }
    if (lane == 0) {
        if (tp) atomicAdd(a.cnt + col * LS_CW + 1, tp);
        if (fp) atomicAdd(a.cnt + col * LS_CW + 2, fp);
        if (fn) atomicAdd(a.cnt + col * LS_CW + 3, fn);
    }
}

// one thread per column: the per-column outputs and the class totals
__global__ __launch_bounds__(256) void k_ls_final(LsArgs a) {
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ncols = (long long)a.n_rec * a.NC;
    if (col >= ncols * a.K) return;
    const int c = (int)(col % a.NC) + (int)(col / ncols) * a.NC;     // the row of the totals: (point, class)
    const int32_t* k = a.cnt + col * LS_CW;
    const int file_seg = ls_file_segments(a, col / a.NC);
    const bool ok = (ls_col_flags(a, col) | k[4]) == 0 && file_seg <= SC_MAXSEG;
    long long p0;
    int n_ref, n_est;
    ls_range(a.ref_ptr, ls_rcol(a, col), a.ref_cap, p0, n_ref);
    ls_range(a.est_ptr, col, a.est_cap, p0, n_est);
    const int ev[3] = {ok ? k[0] : 0, n_ref, n_est};
    int sg[4] = {0, 0, 0, 0};
    if (ok) {
        sg[0] = k[1]; sg[1] = k[2]; sg[2] = k[3];
        sg[3] = file_seg - sg[0] - sg[1] - sg[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (a.out_a) a.out_a[col * 3 + i] = ev[i];
        if (ev[i] > 0) atomicAdd(a.tot_a + c * 3 + i, (unsigned long long)ev[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (a.out_b) a.out_b[col * 4 + i] = sg[i];
        if (sg[i] > 0) atomicAdd(a.tot_b + c * 4 + i, (unsigned long long)sg[i]);
    }
}

// ---- PSDS -------------------------------------------------------------------------------------------------------------------
// the events x[lo .. hi) that can overlap (q_on, q_off): those before lo end at or before q_on, those from hi on start at or
// after q_off - every term left out is +0.0
__device__ __forceinline__ void lp_window(const double* on, const double* pmax, int n, double q_on, double q_off, int& lo,
                                          int& hi) {
    int l = 0, h = n;
    while (l < h) {                                                  // first i with on[i] >= q_off
        const int mid = (l + h) >> 1;
        if (on[mid] >= q_off) h = mid;
        else l = mid + 1;
    }
    hi = l;
    l = 0; h = hi;
    while (l < h) {                                                  // first i with pmax[i] > q_on
        const int mid = (l + h) >> 1;
        if (pmax[mid] > q_on) h = mid;
        else l = mid + 1;
    }
    lo = l;
}
// sum of I(d, g) over the ground truths g of reference column rcol: sequential over the window in stored order, from 0.0
__device__ __forceinline__ double lp_ref_sum(const LsArgs& a, long long rcol, double d_on, double d_off) {
    long long pr;
    int n_ref, lo, hi;
    ls_range(a.ref_ptr, rcol, a.ref_cap, pr, n_ref);
    lp_window(a.ref_on + pr, a.ref_pmax + pr, n_ref, d_on, d_off, lo, hi);
    double sum = 0.0;
    for (int g = lo; g < hi; ++g) sum += sc_overlap(d_on, d_off, a.ref_on[pr + g], a.ref_off[pr + g]);
    return sum;
}
// the column of event i of a CSR table of ncols columns (the last column whose offset is <= i); -1 when i is outside it
__device__ __forceinline__ long long lp_column(const int64_t* ptr, long long ncols, long long cap, long long i, long long& p0,
                                               int& n) {
    long long lo = 0, hi = ncols - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    if (!ls_range(ptr, lo, cap, p0, n) || i < p0 || i >= p0 + n) return -1;
    return lo;
}
// cnt[col][slot] += 1 for the lanes with `flag`: one atomic per wave when all its lanes are in one column
__device__ __forceinline__ void lp_count(const LsArgs& a, long long col, bool uniform, int slot, bool flag) {
    if (uniform) {
        const int n = __popcll(__ballot(flag));
        if (n && (threadIdx.x & 63) == 0) atomicAdd(a.cnt + col * LS_CW + slot, n);
    } else if (flag) {
        atomicAdd(a.cnt + col * LS_CW + slot, 1);
    }
}

__global__ __launch_bounds__(256) void k_lp_detect(LsArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long pe = 0;
    int n_est = 0;
    const long long ncols = (long long)a.n_rec * a.NC;
    long long col = i < a.est_cap ? lp_column(a.est_ptr, ncols * a.K, a.est_cap, i, pe, n_est) : -1;
    if (col >= 0 && ls_col_flags(a, col)) col = -1;                  // not scored (k_ls_prep reported it)
    const bool active = col >= 0;
    const long long rcol = active ? col % ncols : 0;
    const long long col0 = __shfl(col, 0);
    const bool uniform = __ballot(col == col0) == ~0ull && col0 >= 0;
    bool relevant = false;
    double d_on = 0.0, d_off = 0.0;
    if (active) {
        d_on = a.est_on[i];
        d_off = a.est_off[i];
        relevant = sc_passes(lp_ref_sum(a, rcol, d_on, d_off), d_off - d_on, a.dtc);
        a.rel[i] = relevant ? 1 : 0;
    }
    const bool cross = active && !relevant;
    lp_count(a, col, uniform, 1, cross);
    const int c = active ? (int)(col % a.NC) : -1;
    for (int j = 0; j < a.NC; ++j) {
        bool ct = false;
        if (cross && j != c) {
            const long long cj = rcol - c + j;
            // (a malformed or unsorted reference column raised err)
            if (a.rflags[cj] == 0) ct = sc_passes(lp_ref_sum(a, cj, d_on, d_off), d_off - d_on, a.cttc);
        }
        lp_count(a, col, uniform, 2 + j, ct);
    }
}

__global__ __launch_bounds__(256) void k_lp_truth(LsArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long pr = 0, pe;
    int n_ref = 0, n_est;
    const long long ncols = (long long)a.n_rec * a.NC;
    const long long rcol = i < a.ref_cap ? lp_column(a.ref_ptr, ncols, a.ref_cap, i, pr, n_ref) : -1;
    long long col = rcol >= 0 ? (long long)blockIdx.y * ncols + rcol : -1;       // blockIdx.y: the operating point
    if (col >= 0 && ls_col_flags(a, col)) col = -1;
    const bool active = col >= 0;
    const long long col0 = __shfl(col, 0);
    const bool uniform = __ballot(col == col0) == ~0ull && col0 >= 0;
    bool found = false;
    if (active) {
        const double g_on = a.ref_on[i], g_off = a.ref_off[i];
        ls_range(a.est_ptr, col, a.est_cap, pe, n_est);
        int lo, hi;
        lp_window(a.est_on + pe, a.est_pmax + pe, n_est, g_on, g_off, lo, hi);
        double sum = 0.0;
        for (int e = lo; e < hi; ++e)
            if (a.rel[pe + e]) sum += sc_overlap(a.est_on[pe + e], a.est_off[pe + e], g_on, g_off);
        found = sc_passes(sum, g_off - g_on, a.gtc);
    }
    lp_count(a, col, uniform, 0, found);
}

// one thread per (column, value)
__global__ __launch_bounds__(256) void k_lp_final(LsArgs a) {
    const int W = 2 + a.NC;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ncols = (long long)a.n_rec * a.NC;
    if (t >= ncols * a.K * W) return;
    const long long col = t / W;
    const int v = (int)(t - col * W), c = (int)(col % a.NC) + (int)(col / ncols) * a.NC;
    const bool ok = ls_col_flags(a, col) == 0;
    const int mine = ok ? a.cnt[col * LS_CW + v] : 0;
    if (a.out_a) a.out_a[t] = mine;
    if (mine > 0) atomicAdd(a.tot_a + c * W + v, (unsigned long long)mine);
}

// ---- overall error rate with substitutions ----------------------------------------------------------------------------------
// (include/dcase_sed.h, "overall error rate".)  Nany of a recording is a ONE-CLASS problem on the onset-sorted union of its
// class columns, so after k_ls_prep (the class columns, as for the other calls):
//   k_le_columns   one thread per merged column - (point, recording) on the estimated side, recording on the reference side:
//                  its offsets, the OR of its class columns' err bits, its counters zeroed
//   k_le_merge     one thread per event: its rank in the union is its index in its own column plus a bisection count in each
//                  other column of the recording (ties by class, then index), so every slot of the merged table has exactly
//                  one writer and there is no atomic.  The reference side is merged once, whatever K is
//   k_ls_match     the kernel of the class-wise calls, on the merged table with nclass = 1
//   k_le_segments  one thread per segment: ls_covered per class gives a 16-bit mask per side, sc_segment_sdi the segment's
//                  part of (S, D, I)
//   k_le_final     one thread per (point, recording): outputs and totals
struct LeArgs {
    LsArgs c;                        // the class columns, as k_ls_prep validated them
    int64_t *m_eptr, *m_rptr;        // ws [K * n_rec + 1], [n_rec + 1]: CSR offsets of the merged columns
    double *m_eon, *m_eoff;          // ws [est_cap] each: a (point, recording)'s events of all classes by onset
    double *m_ron, *m_roff;          // ws [ref_cap] each
    int32_t *m_flags, *m_rflags;     // ws [K * n_rec], [n_rec]
    int32_t* m_cnt;                  // ws [K * n_rec][LS_CW]: [0] Nany, [1..3] S / D / I, [4] k_ls_match's err bits
    int32_t *ev_out, *seg_out;
    unsigned long long *ev_tot, *seg_tot;
};

__global__ __launch_bounds__(256) void k_le_columns(LeArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n_e = (long long)a.c.K * a.c.n_rec;
    if (t >= n_e + a.c.n_rec) return;
    const int side = t >= n_e;
    const long long mc = side ? t - n_e : t;
    const int32_t* flags = side ? a.c.rflags : a.c.flags;
    const int64_t* ptr = side ? a.c.ref_ptr : a.c.est_ptr;
    int64_t* m_ptr = side ? a.m_rptr : a.m_eptr;
    int f = 0;
    for (int c = 0; c < a.c.NC; ++c) f |= flags[mc * a.c.NC + c];
    (side ? a.m_rflags : a.m_flags)[mc] = f;
    m_ptr[mc] = ptr[mc * a.c.NC];
    if (mc + 1 == (side ? a.c.n_rec : n_e)) m_ptr[mc + 1] = ptr[(mc + 1) * a.c.NC];
    if (!side)
        for (int i = 0; i < LS_CW; ++i) a.m_cnt[mc * LS_CW + i] = 0;
}

// the number of x[0 .. n) (sorted) that are < v, or <= v
__device__ __forceinline__ int le_count(const double* x, int n, double v, bool or_equal) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] < v || (or_equal && x[mid] == v)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_le_merge(LeArgs a, unsigned est_blocks) {
    const int side = blockIdx.x >= est_blocks;
    const long long i = (long long)(blockIdx.x - (side ? est_blocks : 0)) * 256 + threadIdx.x;
    const int NC = a.c.NC;
    const int64_t* ptr = side ? a.c.ref_ptr : a.c.est_ptr;
    const long long cap = side ? a.c.ref_cap : a.c.est_cap;
    const long long ncols = (long long)a.c.n_rec * NC * (side ? 1 : a.c.K);
    const int32_t* flags = side ? a.c.rflags : a.c.flags;
    const double* on = side ? a.c.ref_on : a.c.est_on;
    const double* off = side ? a.c.ref_off : a.c.est_off;
    if (i >= cap) return;
    long long p0;
    int n;
    const long long col = lp_column(ptr, ncols, cap, i, p0, n);
    if (col < 0) return;
    const long long col0 = col - col % NC;                           // the recording's first column
    int f = 0;
    for (int c = 0; c < NC; ++c) f |= flags[col0 + c];
    if (f) return;                                                   // not scored (k_ls_prep reported it): nothing reads its slots
    const int c = (int)(col - col0);
    const double v = on[i];
    long long rank = i - p0;
    for (int c2 = 0; c2 < NC; ++c2) {
        if (c2 == c) continue;
        long long q0;
        int m;
        ls_range(ptr, col0 + c2, cap, q0, m);
        rank += le_count(on + q0, m, v, c2 < c);
    }
    // every column of the recording is valid, so its events are [ptr[col0], ptr[col0 + NC]) and rank is below their number
    const long long at = ptr[col0] + rank;
    (side ? a.m_ron : a.m_eon)[at] = v;
    (side ? a.m_roff : a.m_eoff)[at] = off[i];
}

__global__ __launch_bounds__(256) void k_le_segments(LeArgs a) {
    const long long mc = blockIdx.x;                                 // (point, recording)
    const int lane = threadIdx.x & 63, NC = a.c.NC;
    const int file_seg = ls_file_segments(a.c, mc);
    if (file_seg > SC_MAXSEG) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicOr(a.c.err, SC_ERR_SEGMENTS);
        return;
    }
    if (a.m_flags[mc] | a.m_rflags[mc % a.c.n_rec]) return;
    int S = 0, D = 0, I = 0;
    for (int s = blockIdx.y * 256 + threadIdx.x; s < file_seg; s += LS_SEG_SPLIT * 256) {
        unsigned ref_mask = 0, est_mask = 0;
        for (int c = 0; c < NC; ++c) {
            const long long col = mc * NC + c;
            long long pr, pe;
            int n_ref, n_est;
            ls_range(a.c.ref_ptr, ls_rcol(a.c, col), a.c.ref_cap, pr, n_ref);
            ls_range(a.c.est_ptr, col, a.c.est_cap, pe, n_est);
            ref_mask |= (unsigned)ls_covered(a.c.ref_on + pr, a.c.ref_pmax + pr, n_ref, s, a.c.res) << c;
            est_mask |= (unsigned)ls_covered(a.c.est_on + pe, a.c.est_pmax + pe, n_est, s, a.c.res) << c;
        }
        sc_segment_sdi(ref_mask, est_mask, S, D, I);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S += __shfl_xor(S, o);
        D += __shfl_xor(D, o);
        I += __shfl_xor(I, o);
    }
    if (lane == 0) {
        if (S) atomicAdd(a.m_cnt + mc * LS_CW + 1, S);
        if (D) atomicAdd(a.m_cnt + mc * LS_CW + 2, D);
        if (I) atomicAdd(a.m_cnt + mc * LS_CW + 3, I);
    }
}

__global__ __launch_bounds__(256) void k_le_final(LeArgs a) {
    const long long mc = (long long)blockIdx.x * 256 + threadIdx.x;
    if (mc >= (long long)a.c.K * a.c.n_rec) return;
    const int kp = (int)(mc / a.c.n_rec), NC = a.c.NC;
    const int32_t* k = a.m_cnt + mc * LS_CW;
    const bool ok = (a.m_flags[mc] | a.m_rflags[mc % a.c.n_rec] | k[4]) == 0 && ls_file_segments(a.c, mc) <= SC_MAXSEG;
    int n_ref = 0, n_est = 0;
    for (int c = 0; c < NC; ++c) {
        long long p0;
        int n;
        ls_range(a.c.ref_ptr, ls_rcol(a.c, mc * NC + c), a.c.ref_cap, p0, n);
        n_ref += n;
        ls_range(a.c.est_ptr, mc * NC + c, a.c.est_cap, p0, n);
        n_est += n;
    }
    const int ev[3] = {n_ref, n_est, ok ? k[0] : 0};
    const int sg[3] = {ok ? k[1] : 0, ok ? k[2] : 0, ok ? k[3] : 0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (a.ev_out) a.ev_out[mc * 3 + i] = ev[i];
        if (ev[i] > 0) atomicAdd(a.ev_tot + kp * 3 + i, (unsigned long long)ev[i]);
        if (a.seg_out) a.seg_out[mc * 3 + i] = sg[i];
        if (sg[i] > 0) atomicAdd(a.seg_tot + kp * 3 + i, (unsigned long long)sg[i]);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int sed_long_tile_events(void) { return LS_TILE; }

static size_t ls_align(size_t v) { return (v + 15) / 16 * 16; }
#define LS_MAXK 4096                 // operating points per call (k_lp_truth's second grid dimension)
struct LsWs { size_t flags, rflags, cnt, on, off, epmax, rpmax, rel, total; };
// (for K = 1 the two flag arrays take the bytes of the former [ncols][2] array: sed_long_score_ws_bytes is unchanged)
static LsWs ls_ws(long long est_cap, long long ref_cap, long long ncols, int K) {
    LsWs w;
    size_t o = 0;
    w.flags = o;  o += (size_t)K * ncols * sizeof(int32_t);
    w.rflags = o; o = ls_align(o + (size_t)ncols * sizeof(int32_t));
    w.cnt = o;   o += ls_align((size_t)K * ncols * LS_CW * sizeof(int32_t));
    w.on = o;    o += ls_align((size_t)est_cap * sizeof(double));
    w.off = o;   o += ls_align((size_t)est_cap * sizeof(double));
    w.epmax = o; o += ls_align((size_t)est_cap * sizeof(double));
    w.rpmax = o; o += ls_align((size_t)ref_cap * sizeof(double));
    w.rel = o;   o += ls_align((size_t)est_cap);
    w.total = o;
    return w;
}
static const char* const LS_NEED = "need 0 <= est_capacity, ref_events < 2^31 - 1024, n_rec >= 1, 1 <= nclass <= 16, "
                                   "1 <= n_points <= 4096, n_points * n_rec * nclass < 2^26, n_points * reference tiles < 2^31";
static bool ls_sizes_ok(long long est_cap, long long ref_cap, int n_rec, int nclass, int K) {
    return est_cap >= 0 && ref_cap >= 0 && est_cap < (1ll << 31) - 1024 && ref_cap < (1ll << 31) - 1024 && n_rec >= 1 &&
           nclass >= 1 && nclass <= SC_MAXNC && K >= 1 && K <= LS_MAXK && (long long)K * n_rec * nclass < (1ll << 26) &&
           (ref_cap / LS_TILE + (long long)n_rec * nclass + 1) * K < (1ll << 31);
}

extern "C" size_t sed_long_sweep_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass, int n_points) {
    if (!ls_sizes_ok(est_capacity, ref_events, n_rec, nclass, n_points)) {
        sed_set_error("sed_long_sweep_ws_bytes: %s", LS_NEED);
        return 0;
    }
    return ls_ws(est_capacity, ref_events, (long long)n_rec * nclass, n_points).total;
}

extern "C" size_t sed_long_score_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass) {
    if (!ls_sizes_ok(est_capacity, ref_events, n_rec, nclass, 1)) {
        sed_set_error("sed_long_score_ws_bytes: need 0 <= est_capacity, ref_events < 2^31 - 1024, n_rec >= 1, 1 <= nclass <= 16, "
                      "n_rec * nclass < 2^26");
        return 0;
    }
    return ls_ws(est_capacity, ref_events, (long long)n_rec * nclass, 1).total;
}

static int ls_fill(LsArgs& a, const char* what, const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                   const double* est_on, const double* est_off, long long est_cap, const int64_t* ref_ptr, const double* ref_on,
                   const double* ref_off, long long ref_cap, int n_rec, int nclass, int K, int32_t* err, void* ws,
                   size_t ws_bytes) {
    if (!(ev_ptr && ref_ptr && ref_on && ref_off && err && ws)) {
        sed_set_error("%s: null argument", what);
        return SED_ERR_BAD_ARG;
    }
    if (!ls_sizes_ok(est_cap, ref_cap, n_rec, nclass, K)) {
        sed_set_error("%s: %s", what, LS_NEED);
        return SED_ERR_BAD_ARG;
    }
    if (ev_pairs ? !(num > 0.0 && den > 0.0) : !(est_on && est_off)) {
        sed_set_error("%s: estimated events are frames (ev_pairs, num / den > 0) or seconds (est_on, est_off)", what);
        return SED_ERR_BAD_ARG;
    }
    if (((uintptr_t)ws % 8) != 0) {
        sed_set_error("%s: ws must be 8-byte aligned", what);
        return SED_ERR_BAD_ARG;
    }
    const long long ncols = (long long)n_rec * nclass;
    const LsWs w = ls_ws(est_cap, ref_cap, ncols, K);
    if (ws_bytes < w.total) {
        sed_set_error("%s: workspace of %zu bytes is too small (%zu needed)", what, ws_bytes, w.total);
        return SED_ERR_WORKSPACE;
    }
    char* b = (char*)ws;
    a = LsArgs{};
    a.est_ptr = ev_ptr; a.ev_pairs = ev_pairs; a.num = num; a.den = den;
    a.ws_on = (double*)(b + w.on); a.ws_off = (double*)(b + w.off);
    a.est_on = ev_pairs ? a.ws_on : est_on; a.est_off = ev_pairs ? a.ws_off : est_off;
    a.ref_ptr = ref_ptr; a.ref_on = ref_on; a.ref_off = ref_off;
    a.est_cap = est_cap; a.ref_cap = ref_cap; a.n_rec = n_rec; a.NC = nclass; a.K = K;
    a.n_slots = (int)(ref_cap / LS_TILE + ncols + 1);
    a.flags = (int32_t*)(b + w.flags); a.rflags = (int32_t*)(b + w.rflags); a.cnt = (int32_t*)(b + w.cnt);
    a.est_pmax = (double*)(b + w.epmax); a.ref_pmax = (double*)(b + w.rpmax); a.rel = (uint8_t*)(b + w.rel);
    a.err = err;
    return SED_OK;
}

static unsigned ls_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

// Four launches whatever n_points is; k_ls_prep walks every point's estimated columns and the reference columns ONCE.
static int ls_event_counts(const char* what, const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                           const double* est_on, const double* est_off, long long est_capacity, const int64_t* ref_ptr,
                           const double* ref_on, const double* ref_off, long long ref_events, int n_rec, int nclass, int K,
                           double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_counts,
                           int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* ws, size_t ws_bytes,
                           void* stream) {
    if (!(ev_total && seg_total)) {
        sed_set_error("%s: null argument", what);
        return SED_ERR_BAD_ARG;
    }
    if (!(t_collar >= 0.0 && percentage_of_length >= 0.0 && time_resolution > 0.0)) {
        sed_set_error("%s: need t_collar >= 0, percentage_of_length >= 0, time_resolution > 0", what);
        return SED_ERR_BAD_ARG;
    }
    LsArgs a;
    SED_TRY(ls_fill(a, what, ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on, ref_off, ref_events,
                    n_rec, nclass, K, err, ws, ws_bytes));
    a.t_collar = t_collar; a.pct = percentage_of_length; a.res = time_resolution;
    a.out_a = ev_counts; a.out_b = seg_counts;
    a.tot_a = (unsigned long long*)ev_total; a.tot_b = (unsigned long long*)seg_total;
    const long long ncols = (long long)n_rec * nclass, ecols = ncols * K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ls_prep, dim3((unsigned)(ecols + ncols)), dim3(LS_PREP_THREADS), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ls_match, dim3(ls_blocks((long long)a.n_slots * K, 4)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ls_segments, dim3((unsigned)ecols, LS_SEG_SPLIT), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ls_final, dim3(ls_blocks(ecols, 256)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

static int ls_psds_counts(const char* what, const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                          const double* est_on, const double* est_off, long long est_capacity, const int64_t* ref_ptr,
                          const double* ref_on, const double* ref_off, long long ref_events, int n_rec, int nclass, int K,
                          double dtc, double gtc, double cttc, int32_t* columns, int64_t* totals, int32_t* err, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!totals) {
        sed_set_error("%s: null argument", what);
        return SED_ERR_BAD_ARG;
    }
    if (!(dtc >= 0.0 && dtc <= 1.0 && gtc >= 0.0 && gtc <= 1.0 && cttc >= 0.0 && cttc <= 1.0)) {
        sed_set_error("%s: need dtc, gtc and cttc in [0, 1]", what);
        return SED_ERR_BAD_ARG;
    }
    LsArgs a;
    SED_TRY(ls_fill(a, what, ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on, ref_off, ref_events,
                    n_rec, nclass, K, err, ws, ws_bytes));
    a.dtc = dtc; a.gtc = gtc; a.cttc = cttc;
    a.out_a = columns; a.tot_a = (unsigned long long*)totals;
    const long long ncols = (long long)n_rec * nclass, ecols = ncols * K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ls_prep, dim3((unsigned)(ecols + ncols)), dim3(LS_PREP_THREADS), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lp_detect, dim3(ls_blocks(est_capacity, 256)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lp_truth, dim3(ls_blocks(ref_events, 256), (unsigned)K), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lp_final, dim3(ls_blocks(ecols * (2 + nclass), 256)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

// the merged tables behind the workspace of the class-wise calls
struct LeWs { size_t eptr, rptr, eon, eoff, ron, roff, flags, rflags, cnt, total; };
static LeWs le_ws(long long est_cap, long long ref_cap, int n_rec, int nclass, int K) {
    LeWs w;
    size_t o = ls_align(ls_ws(est_cap, ref_cap, (long long)n_rec * nclass, K).total);
    const size_t n_e = (size_t)K * n_rec;
    w.eptr = o;   o += ls_align((n_e + 1) * sizeof(int64_t));
    w.rptr = o;   o += ls_align(((size_t)n_rec + 1) * sizeof(int64_t));
    w.eon = o;    o += ls_align((size_t)est_cap * sizeof(double));
    w.eoff = o;   o += ls_align((size_t)est_cap * sizeof(double));
    w.ron = o;    o += ls_align((size_t)ref_cap * sizeof(double));
    w.roff = o;   o += ls_align((size_t)ref_cap * sizeof(double));
    w.flags = o;  o += ls_align(n_e * sizeof(int32_t));
    w.rflags = o; o += ls_align((size_t)n_rec * sizeof(int32_t));
    w.cnt = o;    o += ls_align(n_e * LS_CW * sizeof(int32_t));
    w.total = o;
    return w;
}

extern "C" size_t sed_long_sweep_error_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass,
                                                int n_points) {
    if (!ls_sizes_ok(est_capacity, ref_events, n_rec, nclass, n_points)) {
        sed_set_error("sed_long_sweep_error_ws_bytes: %s", LS_NEED);
        return 0;
    }
    return le_ws(est_capacity, ref_events, n_rec, nclass, n_points).total;
}

extern "C" size_t sed_long_error_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass) {
    if (!ls_sizes_ok(est_capacity, ref_events, n_rec, nclass, 1)) {
        sed_set_error("sed_long_error_ws_bytes: %s", LS_NEED);
        return 0;
    }
    return le_ws(est_capacity, ref_events, n_rec, nclass, 1).total;
}

// Six launches whatever n_points is; the reference side is validated (k_ls_prep) and merged (k_le_merge) ONCE.
static int ls_error_counts(const char* what, const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                           const double* est_on, const double* est_off, long long est_capacity, const int64_t* ref_ptr,
                           const double* ref_on, const double* ref_off, long long ref_events, int n_rec, int nclass, int K,
                           double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_overall,
                           int32_t* seg_overall, int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err, void* ws,
                           size_t ws_bytes, void* stream) {
    if (!(ev_overall_total && seg_overall_total)) {
        sed_set_error("%s: null argument", what);
        return SED_ERR_BAD_ARG;
    }
    if (!(t_collar >= 0.0 && percentage_of_length >= 0.0 && time_resolution > 0.0)) {
        sed_set_error("%s: need t_collar >= 0, percentage_of_length >= 0, time_resolution > 0", what);
        return SED_ERR_BAD_ARG;
    }
    LeArgs a;
    SED_TRY(ls_fill(a.c, what, ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on, ref_off, ref_events,
                    n_rec, nclass, K, err, ws, ws_bytes));
    const LeWs w = le_ws(est_capacity, ref_events, n_rec, nclass, K);
    if (ws_bytes < w.total) {
        sed_set_error("%s: workspace of %zu bytes is too small (%zu needed)", what, ws_bytes, w.total);
        return SED_ERR_WORKSPACE;
    }
    a.c.t_collar = t_collar; a.c.pct = percentage_of_length; a.c.res = time_resolution;
    char* b = (char*)ws;
    a.m_eptr = (int64_t*)(b + w.eptr); a.m_rptr = (int64_t*)(b + w.rptr);
    a.m_eon = (double*)(b + w.eon); a.m_eoff = (double*)(b + w.eoff);
    a.m_ron = (double*)(b + w.ron); a.m_roff = (double*)(b + w.roff);
    a.m_flags = (int32_t*)(b + w.flags); a.m_rflags = (int32_t*)(b + w.rflags); a.m_cnt = (int32_t*)(b + w.cnt);
    a.ev_out = ev_overall; a.seg_out = seg_overall;
    a.ev_tot = (unsigned long long*)ev_overall_total; a.seg_tot = (unsigned long long*)seg_overall_total;
    // the merged table as k_ls_match sees it: one class, the same recordings and points
    LsArgs m = LsArgs{};
    m.est_ptr = a.m_eptr; m.est_on = a.m_eon; m.est_off = a.m_eoff;
    m.ref_ptr = a.m_rptr; m.ref_on = a.m_ron; m.ref_off = a.m_roff;
    m.est_cap = est_capacity; m.ref_cap = ref_events; m.n_rec = n_rec; m.NC = 1; m.K = K;
    m.n_slots = (int)(ref_events / LS_TILE + n_rec + 1);
    m.t_collar = t_collar; m.pct = percentage_of_length; m.res = time_resolution;
    m.flags = a.m_flags; m.rflags = a.m_rflags; m.cnt = a.m_cnt; m.err = err;
    const long long ncols = (long long)n_rec * nclass, ecols = ncols * K, mcols = (long long)n_rec * K;
    const unsigned est_blocks = ls_blocks(est_capacity, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ls_prep, dim3((unsigned)(ecols + ncols)), dim3(LS_PREP_THREADS), 0, st, a.c);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_le_columns, dim3(ls_blocks(mcols + n_rec, 256)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_le_merge, dim3(est_blocks + ls_blocks(ref_events, 256)), dim3(256), 0, st, a, est_blocks);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ls_match, dim3(ls_blocks((long long)m.n_slots * K, 4)), dim3(256), 0, st, m);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_le_segments, dim3((unsigned)mcols, LS_SEG_SPLIT), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_le_final, dim3(ls_blocks(mcols, 256)), dim3(256), 0, st, a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_long_error_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                                     const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                                     const double* ref_off, long long ref_events, int n_rec, int nclass, double t_collar,
                                     double percentage_of_length, double time_resolution, int32_t* ev_overall,
                                     int32_t* seg_overall, int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err,
                                     void* ws, size_t ws_bytes, void* stream) {
    return ls_error_counts("sed_long_error_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on,
                           ref_off, ref_events, n_rec, nclass, 1, t_collar, percentage_of_length, time_resolution, ev_overall,
                           seg_overall, ev_overall_total, seg_overall_total, err, ws, ws_bytes, stream);
}

extern "C" int sed_long_sweep_error_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                                           const double* est_on, const double* est_off, long long est_capacity,
                                           const int64_t* ref_ptr, const double* ref_on, const double* ref_off,
                                           long long ref_events, int n_rec, int nclass, int n_points, double t_collar,
                                           double percentage_of_length, double time_resolution, int32_t* ev_overall,
                                           int32_t* seg_overall, int64_t* ev_overall_total, int64_t* seg_overall_total,
                                           int32_t* err, void* ws, size_t ws_bytes, void* stream) {
    return ls_error_counts("sed_long_sweep_error_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr,
                           ref_on, ref_off, ref_events, n_rec, nclass, n_points, t_collar, percentage_of_length, time_resolution,
                           ev_overall, seg_overall, ev_overall_total, seg_overall_total, err, ws, ws_bytes, stream);
}

extern "C" int sed_long_event_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                                     const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                                     const double* ref_off, long long ref_events, int n_rec, int nclass, double t_collar,
                                     double percentage_of_length, double time_resolution, int32_t* ev_counts,
                                     int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* ws,
                                     size_t ws_bytes, void* stream) {
    return ls_event_counts("sed_long_event_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on,
                           ref_off, ref_events, n_rec, nclass, 1, t_collar, percentage_of_length, time_resolution, ev_counts,
                           seg_counts, ev_total, seg_total, err, ws, ws_bytes, stream);
}

extern "C" int sed_long_sweep_event_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                                           const double* est_on, const double* est_off, long long est_capacity,
                                           const int64_t* ref_ptr, const double* ref_on, const double* ref_off,
                                           long long ref_events, int n_rec, int nclass, int n_points, double t_collar,
                                           double percentage_of_length, double time_resolution, int32_t* ev_counts,
                                           int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* ws,
                                           size_t ws_bytes, void* stream) {
    return ls_event_counts("sed_long_sweep_event_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr,
                           ref_on, ref_off, ref_events, n_rec, nclass, n_points, t_collar, percentage_of_length, time_resolution,
                           ev_counts, seg_counts, ev_total, seg_total, err, ws, ws_bytes, stream);
}

extern "C" int sed_long_psds_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                                    const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                                    const double* ref_off, long long ref_events, int n_rec, int nclass, double dtc, double gtc,
                                    double cttc, int32_t* columns, int64_t* totals, int32_t* err, void* ws, size_t ws_bytes,
                                    void* stream) {
    return ls_psds_counts("sed_long_psds_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr, ref_on,
                          ref_off, ref_events, n_rec, nclass, 1, dtc, gtc, cttc, columns, totals, err, ws, ws_bytes, stream);
}

extern "C" int sed_long_sweep_psds_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                                          const double* est_on, const double* est_off, long long est_capacity,
                                          const int64_t* ref_ptr, const double* ref_on, const double* ref_off,
                                          long long ref_events, int n_rec, int nclass, int n_points, double dtc, double gtc,
                                          double cttc, int32_t* columns, int64_t* totals, int32_t* err, void* ws, size_t ws_bytes,
                                          void* stream) {
    return ls_psds_counts("sed_long_sweep_psds_counts", ev_ptr, ev_pairs, num, den, est_on, est_off, est_capacity, ref_ptr,
                          ref_on, ref_off, ref_events, n_rec, nclass, n_points, dtc, gtc, cttc, columns, totals, err, ws,
                          ws_bytes, stream);
}
