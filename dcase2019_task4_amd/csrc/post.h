// post.h - the per-column decode of a strong posterior, shared by k_postprocess (post.hip: event lists out) and
// k_event_counts / k_psds_counts (score.hip: events stay in LDS and are scored there).  One wave owns one (clip, class) column.
#pragma once
#include "common.h"

#define PP_MAXT 2048      // frames per column held in LDS (T/8: clips up to 16 384 input frames)

// The rules every decode shares (k_stitch_tile<VEC, PASS, SWEEP> of stitch.hip, the one tile kernel of sed_stitch_decode and
// sed_stitch_sweep, holds a column in tiles and applies the same ones):
// the decision is p > threshold (dcase_util's global_threshold binarization, strict);
__device__ __forceinline__ uint8_t pp_decision(float p, float threshold) { return (p > threshold) ? 1 : 0; }
// scipy's "reflect" of an index into [0, T): -1 -> 0, -2 -> 1, T -> T-1, T+1 -> T-2, repeatedly for windows longer than the column;
__device__ __forceinline__ int pp_reflect(int i, int T) {
    while (i < 0 || i >= T) i = (i < 0) ? -i - 1 : 2 * T - i - 1;
    return i;
}
// and the run-length decode of one 64-frame chunk: lane `lane` holds frame t, active or not, and whether its two neighbours
// are (a frame outside the column is not).  Onset where 0 -> 1, (exclusive) offset where 1 -> 0; n_on / n_off are the
// running counts of the column, so sink(k, frame, is_offset) gets the k-th onset and the k-th offset.
template <class Sink>
__device__ __forceinline__ void pp_emit_chunk(bool act, bool prev, bool next, int t, int lane, int& n_on, int& n_off, Sink sink) {
    const bool is_on = act && !prev, is_off = act && !next;
    const unsigned long long m_on = __ballot(is_on), m_off = __ballot(is_off);
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (is_on) sink(n_on + __popcll(m_on & below), t, false);
    if (is_off) sink(n_off + __popcll(m_off & below), t + 1, true);
    n_on += __popcll(m_on);
    n_off += __popcll(m_off);
}

// Threshold -> median filter (reflect) -> run-length decode of the column p[t * stride], t < T.  Called by all 64 lanes of
// every wave of the workgroup (it contains workgroup barriers); raw[T] and flt[T + 1] are this wave's own LDS.  When
// `binary` is not null the filtered decisions go to binary[t * stride].  sink(k, frame, is_offset) receives the k-th onset
// frame and the k-th (exclusive) offset frame, from the lane that found it; returns the number of events.
template <class Sink>
__device__ __forceinline__ int pp_decode_column(const float* __restrict__ p, int T, int stride, float threshold, int window,
                                                uint8_t* raw, uint8_t* flt, uint8_t* __restrict__ binary, Sink sink) {
    const int lane = threadIdx.x & 63;
    for (int t = lane; t < T; t += 64) raw[t] = pp_decision(p[(size_t)t * stride], threshold);
    __syncthreads();
    // scipy rank filter: origin 0 -> window covers [t - w/2, t - w/2 + w); reflect: -1 -> 0, -2 -> 1, T -> T-1, T+1 -> T-2;
    // median = sorted[w/2]: for 0/1 data that is 1 iff #ones >= w - w/2
    const int lo = window / 2, need = window - window / 2;
    for (int t = lane; t < T; t += 64) {
        int ones = 0;
        for (int d = 0; d < window; ++d) {
            ones += raw[pp_reflect(t - lo + d, T)];
        }
        const uint8_t v = ones >= need ? 1 : 0;
        flt[t] = v;
        if (binary) binary[(size_t)t * stride] = v;
    }
    if (lane == 0) flt[T] = 0;
    __syncthreads();
    // find_contiguous_regions: onset where 0 -> 1 (or t = 0 active), offset (exclusive) where 1 -> 0 (or the end).
    // Onsets and offsets alternate along the column, so the k-th onset pairs with the k-th offset; two running counters
    // because an event may span a 64-frame chunk boundary.
    int n_on = 0, n_off = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool act = t < T && flt[t];
        const bool prev = act && t > 0 && flt[t - 1];
        const bool next = act && flt[t + 1];              // flt[T] = 0
        pp_emit_chunk(act, prev, next, t, lane, n_on, n_off, sink);
    }
    return n_on;
}
