// score.h - the scoring definitions that clip scoring (score.hip) and long-recording scoring (lscore.hip) share: the limits,
// the error bits, the event-based compatibility test and the matcher, the segment index and the PSDS intersection and test.
// include/dcase_sed.h states the definitions; each exists in code once, here.
#pragma once
// Seconds are formed as (double)frame * num / den and PSDS sums as sum += I(d, g): exactly the host's operations, never a
// fused one.  Both including files open with this pragma as well: hipcc carries a file-scope pragma across an #include in
// both directions (profiles/score_helpers.md), but neither the helpers nor the kernels should depend on the include order.
#pragma clang fp contract(off)
#include "common.h"

#define SC_MAXEV 64                  // events per side of one matching (a clip's column, a long recording's cluster): one lane /
                                     // one mask bit each
#define SC_MAXSEG 65536              // segments per file
#define SC_MAXNC 16                  // classes

// bits of the device error word (bit 128, an invalid decoded table, is only ever set by the Python layer)
enum : int {
    SC_ERR_MANY_REF = 1,             // more than SC_MAXEV reference events in a column (clips) / cluster (long recordings)
    SC_ERR_MANY_EST = 2,             // the same of the estimated events
    SC_ERR_SEGMENTS = 4,             // a file has more than SC_MAXSEG segments
    SC_ERR_WINDOW = 8,               // a median window outside 1 .. 63
    SC_ERR_OFFSETS = 16,             // malformed event offsets
    SC_ERR_UNSORTED = 64,            // a column whose onsets decrease (long recordings)
};

__device__ __forceinline__ int sc_lane_read(int v, int src) {
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src));
}
// segment index of a time, clamped to [0, SC_MAXSEG + 1] (NaN -> 0) so that the cast is defined
__device__ __forceinline__ int sc_seg_index(double x) {
    return !(x > 0.0) ? 0 : (x > (double)SC_MAXSEG ? SC_MAXSEG + 1 : (int)x);
}

// ---- event-based ------------------------------------------------------------------------------------------------------------
// reference r and estimated e are compatible iff |r.on - e.on| <= t_collar and |r.off - e.off| <= sc_offset_tolerance(r)
__device__ __forceinline__ double sc_offset_tolerance(double r_on, double r_off, double t_collar, double pct) {
    return fmax(t_collar, pct * (r_off - r_on));
}
// (estimated event e of the arrays e_on / e_off: its offset is only read when the onset test holds)
__device__ __forceinline__ bool sc_compatible(double r_on, double r_off, double tol_off, const double* e_on,
                                              const double* e_off, int e, double t_collar) {
    return fabs(r_on - e_on[e]) <= t_collar && fabs(r_off - e_off[e]) <= tol_off;
}

// Size of a maximum bipartite matching between up to 64 reference events and n_est <= 64 estimated events, called by a
// whole wave: lane r passes the mask `adj` of the estimated events compatible with reference r (0 for a lane without one),
// n_est is wave-uniform.  One breadth-first augmenting-path search per estimated event, every level of it one ballot - the
// frontier, the visited set and the matched set are wave-uniform 64-bit masks in SGPRs, so all variable-trip-count loops run
// on scalar control flow.
__device__ __forceinline__ int sc_max_matching(unsigned long long adj, int n_est, int lane) {
    int size = 0;
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
                    const int e = sc_lane_read(parent, r);
                    const int prev = sc_lane_read(m_est, e);
                    if (lane == e) m_est = r;
                    if (prev < 0) break;
                    r = prev;
                }
                ++size;
                break;
            }
            visited |= new_ref;
            frontier = __ballot(m_est >= 0 && ((new_ref >> (m_est & 63)) & 1));
        }
    }
    return size;
}

// ---- clusters of two onset-sorted lists --------------------------------------------------------------------------------------
// first j in [0, n) with !(x[j] far below r), i.e. the number of j with r - x[j] > tol (x sorted)
__device__ __forceinline__ int sc_count_below(const double* x, int n, double r, double tol) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r - x[mid] > tol) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// first j in [0, n] with x[j] - r > tol (x sorted)
__device__ __forceinline__ int sc_first_above(const double* x, int n, double r, double tol) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] - r > tol) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// A cut in front of reference i is a pair (i, j): the first i references and the first j estimated events lie before it.  It
// is valid iff jlo(i) <= j <= jhi(i), jlo(i) = first j with E[j] - R[i - 1] > t_collar, jhi(i) = number of j with
// R[i] - E[j] > t_collar - the differences are formed as the compatibility test forms them, so that no pair the test accepts
// can straddle a cut whatever the rounding.  The cluster of references i0 .. i1 - 1 (i0, i1 consecutive indices with a
// valid cut) holds the estimated events jhi(i0) .. jlo(i1) - 1; estimated events outside these ranges match nothing.
//
// sc_match_tile, called by a whole wave: the sum of the maximum matchings of the clusters that START among the references
// i_base .. i_base + 63 of R / Roff[0 .. n_ref) against E / Eoff[0 .. n_est), both sorted by onset.  "i starts a cluster" is a
// local test (two bisections in the estimated onsets), so the wave finds the starts with one ballot and their ends with a
// second ballot over the next 64 references (further ones only on the error path).  A cluster of more than SC_MAXEV per side
// raises SC_ERR_MANY_REF / SC_ERR_MANY_EST in `flags` and is not matched.
__device__ __forceinline__ int sc_match_tile(const double* R, const double* Roff, int n_ref, const double* E, const double* Eoff,
                                             int n_est, int i_base, double tc, double pct, int lane, int& flags) {
    // lane l: reference i_base + l (first ballot) and i_base + 64 + l (second); index n_ref is the column's end
    int jlo[2], jhi[2];
    unsigned long long starts[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = i_base + h * SC_MAXEV + lane;
        bool bnd = false;
        jlo[h] = jhi[h] = 0;
        if (i <= n_ref) {
            jlo[h] = i > 0 ? sc_first_above(E, n_est, R[i - 1], tc) : 0;
            jhi[h] = i < n_ref ? sc_count_below(E, n_est, R[i], tc) : n_est;
            bnd = jlo[h] <= jhi[h];
        }
        starts[h] = __ballot(bnd);
    }
    unsigned long long todo = starts[0];
    if (n_ref - i_base < 64) todo &= (1ull << (n_ref - i_base)) - 1;     // a cluster starts at a reference, not at the end
    int ntp = 0;
    while (todo) {
        const int s = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const unsigned long long later = starts[0] & ((~0ull << s) << 1);
        int nr, j1;
        if (later) {
            const int t = __ffsll((long long)later) - 1;
            nr = t - s;
            j1 = sc_lane_read(jlo[0], t);
        } else if (starts[1]) {
            const int t = __ffsll((long long)starts[1]) - 1;
            nr = 64 + t - s;
            j1 = sc_lane_read(jlo[1], t);
        } else {                               // more than 64 references (bit 1): walk on to the cluster's end for bit 2
            nr = 0;
            j1 = 0;
            for (int base = i_base + 2 * SC_MAXEV; nr == 0; base += SC_MAXEV) {     // ends: index n_ref is always a cut
                const int i = base + lane;
                const int jl = i <= n_ref ? sc_first_above(E, n_est, R[i - 1], tc) : 0;
                const int jh = i < n_ref ? sc_count_below(E, n_est, R[i], tc) : n_est;
                const unsigned long long m = __ballot(i <= n_ref && jl <= jh);
                if (m) {
                    const int t = __ffsll((long long)m) - 1;
                    nr = base + t - (i_base + s);
                    j1 = sc_lane_read(jl, t);
                }
            }
        }
        const int j0 = sc_lane_read(jhi[0], s);
        const int ne = j1 - j0;
        if (nr > SC_MAXEV) flags |= SC_ERR_MANY_REF;
        if (ne > SC_MAXEV) flags |= SC_ERR_MANY_EST;
        if (nr > SC_MAXEV || ne > SC_MAXEV || ne <= 0) continue;
        // ---- the cluster: lane r holds reference i0 + r and the mask of the estimated events compatible with it ----------
        const int i0 = i_base + s;
        const bool has_ref = lane < nr;
        double r_on = 0.0, r_off = 0.0;
        if (has_ref) {
            r_on = R[i0 + lane];
            r_off = Roff[i0 + lane];
        }
        const double tol_off = sc_offset_tolerance(r_on, r_off, tc, pct);
        unsigned long long adj = 0;
        for (int e = 0; e < ne; ++e) {
            const bool hit = has_ref && sc_compatible(r_on, r_off, tol_off, E, Eoff, j0 + e, tc);
            adj |= (unsigned long long)hit << e;
        }
        ntp += sc_max_matching(adj, ne, lane);
    }
    return ntp;
}

// ---- segment-based overall error rate ---------------------------------------------------------------------------------------
// one segment's part of (S, D, I) from the masks of the classes active in it on each side
__device__ __forceinline__ void sc_segment_sdi(unsigned ref_mask, unsigned est_mask, int& S, int& D, int& I) {
    const int fn = __popc(ref_mask & ~est_mask), fp = __popc(est_mask & ~ref_mask);
    S += min(fn, fp);
    D += max(0, fn - fp);
    I += max(0, fp - fn);
}

// ---- PSDS -------------------------------------------------------------------------------------------------------------------
// I(a, b) = max(0, min(a.off, b.off) - max(a.on, b.on))
__device__ __forceinline__ double sc_overlap(double a_on, double a_off, double b_on, double b_off) {
    return fmax(0.0, fmin(a_off, b_off) - fmax(a_on, b_on));
}
// sum / len >= threshold: the division first; an event of length <= 0 and a NaN ratio fail
__device__ __forceinline__ bool sc_passes(double sum, double len, double threshold) {
    return len > 0.0 && sum / len >= threshold;
}
