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

// ---- PSDS -------------------------------------------------------------------------------------------------------------------
// I(a, b) = max(0, min(a.off, b.off) - max(a.on, b.on))
__device__ __forceinline__ double sc_overlap(double a_on, double a_off, double b_on, double b_off) {
    return fmax(0.0, fmin(a_off, b_off) - fmax(a_on, b_on));
}
// sum / len >= threshold: the division first; an event of length <= 0 and a NaN ratio fail
__device__ __forceinline__ bool sc_passes(double sum, double len, double threshold) {
    return len > 0.0 && sum / len >= threshold;
}
