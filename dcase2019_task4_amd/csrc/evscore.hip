// evscore.hip - confidence scores of decoded events and a select by score, in the event domain (the definitions are in
// include/dcase_sed.h).  The third and fourth event-domain operators beside hyst.hip and evproc.hip, on the flat geometry
// of evtable.h: a thread owns one index of `pairs`.
//
// sed_events_scores   per event the maximum and the mean of the blended timeline over its frames.  ONE launch:
//   k_evs_score   a thread finds the column of its index (hy_column / hy_bounds), from it the recording and the class,
//                 validates the recording's frame range and the event against it.  An event of at most EVS_SHORT_FRAMES
//                 frames is reduced by its own thread in increasing u.  A longer one is flagged: the wave takes its flagged
//                 events one at a time from the ballot word, the owner's (base, length) are broadcast, lane l reduces the
//                 frames l, l + 64, ... in increasing order, a fixed butterfly combines the 64 partials and the owner
//                 writes.  The order of the fp64 sum is a function of the event's length alone: the mean is the same bits
//                 wherever the event lies, from call to call and under graph replay.
//                 Thread c < n_cols validates column c's bounds, thread r < n_rec recording r's (err 16).
//   No LDS, no workspace, no atomics but the OR into err.  The timeline is read with a stride of NC floats: it is a few MB
//   and cache-resident in the project's workloads.
// sed_events_select   keeps the events whose score exceeds the minimum of their (point, class).  Three launches, the
//   compaction of evtable.h: k_evs_flag (wave ballots, one count per workgroup), the scan of evproc.hip (one workgroup),
//   k_evs_write (the kept pairs and their scores at their rank; thread c <= n_cols writes out_ptr[c] and validates column c).
// sed_events_tag_scores   per event the largest span tag among the spans it touches: k_evs_score<EvsTagArgs>, the same kernel
//   over the coordinate map rows = spans (the tag gate is this score and sed_events_select with key 0).
// Every ptr entry is validated before it is used as an index; the timeline is addressed only inside a validated recording.
#include "common.h"
#include "kernels.h"
#include "evtable.h"

#ifndef EVS_SHORT_FRAMES
#define EVS_SHORT_FRAMES 32          // the longest event a single thread reduces (tools/long_bench.py --scores, part d)
#endif

struct EvsArgs {
    const float* tl;             // [total][NC]
    long long total;
    const int64_t* f0;           // rec_frame0 [n_rec + 1]
    int n_rec, NC;
    const int64_t* ptr;
    const int32_t* pairs;
    long long cap, n_cols;
    float *smax, *smean;         // [cap], either may be null
    int32_t* err;
};

// The running maximum that skips NaN: m is NaN until the first non-NaN value.  Comparisons and copies only.
__device__ __forceinline__ float evs_max(float m, float v) { return (v == v && (m != m || v > m)) ? v : m; }

// sed_events_tag_scores is the same kernel over another coordinate map: the "timeline" is the span tags [total_spans][NC], the
// recording table rec_span0, and an event [on, off) in frames touches the rows on / span3 .. (off - 1) / span3 of its recording.
// evs_unit is the frames per row: the constant 1 for the scores (the map folds away), span3 for the tag scores.
struct EvsTagArgs {
    EvsArgs e;                   // tl = tags, total = total_spans, f0 = rec_span0, smean = null
    int span3;
};
__device__ __forceinline__ const EvsArgs& evs_args(const EvsArgs& a) { return a; }
__device__ __forceinline__ const EvsArgs& evs_args(const EvsTagArgs& a) { return a.e; }
__device__ __forceinline__ long long evs_unit(const EvsArgs&) { return 1; }
__device__ __forceinline__ long long evs_unit(const EvsTagArgs& a) { return a.span3; }

template <class Args>
__global__ __launch_bounds__(HY_THREADS) void k_evs_score(Args args) {
    const EvsArgs& e = evs_args(args);
    const long long unit = evs_unit(args);
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    const float nan = __builtin_nanf("");
    long long a, b;
    if (i < e.n_cols && !hy_bounds(e.ptr, i, e.cap, a, b)) atomicOr(e.err, 16);
    if (i < e.n_rec) {
        const long long fa = e.f0[i], fb = e.f0[i + 1];
        if (!(fa >= 0 && fa <= fb && fb <= e.total)) atomicOr(e.err, 16);
    }
    bool is_long = false;
    long long base = 0, len = 0;
    if (i < e.cap) {
        const long long c = hy_column(e.ptr, e.n_cols, i);
        if (hy_bounds(e.ptr, c, e.cap, a, b) && i >= a && i < b) {                   // i is event i - a of column c
            const long long rec = (c / e.NC) % e.n_rec, cls = c % e.NC;
            const long long fa = e.f0[rec], fb = e.f0[rec + 1];
            if (fa >= 0 && fa <= fb && fb <= e.total) {
                const hy_i32x2 ev = *(const hy_i32x2*)(e.pairs + 2 * (size_t)i);
                const long long on = ev.x, off = ev.y;
                if (on < 0 || off > (fb - fa) * unit || on >= off) {
                    atomicOr(e.err, 64);
                    if (e.smax) e.smax[i] = nan;
                    if (e.smean) e.smean[i] = nan;
                } else {
                    const long long lo = on / unit, hi = (off - 1) / unit;           // the rows the event touches: hi < fb - fa
                    base = (fa + lo) * e.NC + cls;                                   // < total * NC < 2^31, and so is the last row
                    len = hi - lo + 1;
                    if (len <= EVS_SHORT_FRAMES) {
                        const float* p = e.tl + base;
                        float m = nan;
                        double s = 0.0;
                        for (long long u = 0; u < len; ++u) {
                            const float v = p[u * e.NC];
                            m = evs_max(m, v);
                            s += (double)v;
                        }
                        if (e.smax) e.smax[i] = m;
                        if (e.smean) e.smean[i] = (float)(s / (double)len);
                    } else {
                        is_long = true;
                    }
                }
            }
        }
    }
    uint64_t todo = __ballot(is_long);
    while (todo) {                                                                   // (wave-uniform)
        const int owner = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const long long o_base = __shfl(base, owner), o_len = __shfl(len, owner);
        const float* p = e.tl + o_base;
        float m = nan;
        double s = 0.0;
        for (long long u = lane; u < o_len; u += 64) {
            const float v = p[u * e.NC];
            m = evs_max(m, v);
            s += (double)v;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {                                          // x + y == y + x: every lane ends with the same bits
            s += __shfl_xor(s, o);
            m = evs_max(m, __shfl_xor(m, o));
        }
        if (lane == owner) {
            if (e.smax) e.smax[i] = m;
            if (e.smean) e.smean[i] = (float)(s / (double)o_len);
        }
    }
}


extern "C" int sed_events_scores_short_frames(void) { return EVS_SHORT_FRAMES; }

// What sed_events_scores and sed_events_tag_scores share behind their own null checks: the other checks and the launch.
// `who`: the entry's name, `rows`: its name for e.total, `out`: its word for an output; span3 = 0: the event scores.
static int evs_launch(const char* who, const char* rows, const char* out, const EvsArgs& e, int span3, hipStream_t st) {
    EV_NEED(who, e.NC >= 1 && e.NC <= 16 && e.n_rec >= 1, "need 1 <= NC <= 16 and n_rec >= 1");
    EV_NEED(who, e.n_cols >= 1 && e.n_cols < (1ll << 26) && e.n_cols % ((long long)e.n_rec * e.NC) == 0,
            "need 1 <= n_cols < 2^26, a multiple of n_rec * NC (K * n_rec * NC columns)");
    EV_NEED(who, e.cap >= 0 && e.cap < (1ll << 31), "need 0 <= pairs_capacity < 2^31");
    EV_NEED(who, e.total >= 0 && e.total * e.NC < (1ll << 31), "need 0 <= %s and %s * NC < 2^31", rows, rows);
    EV_NEED(who, ((uintptr_t)e.pairs % 8) == 0, "ev_pairs must be 8-byte aligned");
    const size_t out_bytes = (size_t)e.cap * sizeof(float);
    const void* in[4] = {e.tl, e.f0, e.ptr, e.pairs};
    const size_t in_bytes[4] = {(size_t)e.total * e.NC * sizeof(float), (size_t)(e.n_rec + 1) * sizeof(int64_t),
                                (size_t)(e.n_cols + 1) * sizeof(int64_t), (size_t)e.cap * 2 * sizeof(int32_t)};
    for (int k = 0; k < 4; ++k)
        EV_NEED(who, (!e.smax || ev_disjoint(e.smax, out_bytes, in[k], in_bytes[k])) &&
                         (!e.smean || ev_disjoint(e.smean, out_bytes, in[k], in_bytes[k])),
                "%s output overlaps an input", out);
    EV_NEED(who, !e.smax || !e.smean || ev_disjoint(e.smax, out_bytes, e.smean, out_bytes), "score_max overlaps score_mean");
    if (e.cap == 0) return SED_OK;
    const dim3 grid((unsigned)ev_blocks(e.cap > e.n_cols ? e.cap : e.n_cols));
    const EvsTagArgs a = {e, span3};
    if (span3) hipLaunchKernelGGL(k_evs_score<EvsTagArgs>, grid, dim3(HY_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_evs_score<EvsArgs>, grid, dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_events_scores(const float* timeline, long long total_frames, const int64_t* rec_frame0, int n_rec, int NC,
                                 const int64_t* ev_ptr, const int32_t* ev_pairs, long long pairs_capacity, long long n_cols,
                                 float* score_max, float* score_mean, int32_t* err, void* stream) {
    const char* who = "sed_events_scores";
    EV_NEED(who, timeline && rec_frame0 && ev_ptr && ev_pairs && err, "null argument");
    EV_NEED(who, score_max || score_mean, "score_max and score_mean are both null");
    return evs_launch(who, "total_frames", "an", {timeline, total_frames, rec_frame0, n_rec, NC, ev_ptr, ev_pairs, pairs_capacity,
                                                  n_cols, score_max, score_mean, err}, 0, (hipStream_t)stream);
}

extern "C" int sed_events_tag_scores(const float* tags, long long total_spans, const int64_t* rec_span0, int span3, int n_rec,
                                     int NC, const int64_t* ev_ptr, const int32_t* ev_pairs, long long pairs_capacity,
                                     long long n_cols, float* tag_score, int32_t* err, void* stream) {
    const char* who = "sed_events_tag_scores";
    EV_NEED(who, tags && rec_span0 && ev_ptr && ev_pairs && tag_score && err, "null argument");
    EV_NEED(who, span3 >= 1, "need span3 >= 1");
    return evs_launch(who, "total_spans", "the", {tags, total_spans, rec_span0, n_rec, NC, ev_ptr, ev_pairs, pairs_capacity,
                                                 n_cols, tag_score, nullptr, err}, span3, (hipStream_t)stream);
}

// ---- select by score ---------------------------------------------------------------------------------------------------

struct EvsSelArgs {
    EvTable t;                           // bal / cnt: the keep decisions and their counts
    const float *key, *smax, *smean;     // key: the array compared; smax / smean: what is compacted alongside (or null)
    long long span;                      // n_rec * NC: the columns of one point
    int NC;
    const float* min_score;              // [n_cols / span][NC]
    float *out_smax, *out_smean;
};

__global__ __launch_bounds__(HY_THREADS) void k_evs_flag(EvsSelArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + (int)threadIdx.x;
    bool keep = false;
    if (i < e.t.cap) {
        long long a, b;
        const long long c = hy_column(e.t.ptr, e.t.n_cols, i);
        if (hy_bounds(e.t.ptr, c, e.t.cap, a, b) && i >= a && i < b)                 // (a NaN score compares false)
            keep = e.key[i] > e.min_score[ev_param(e.span, e.NC, c)];
    }
    ev_ballot_count(keep, e.t.bal, e.t.cnt);
}

__global__ __launch_bounds__(HY_THREADS) void k_evs_write(EvsSelArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (i < e.t.cap && ev_bit(e.t.bal, i)) {
        const long long dst = hy_flagged_before(e.t.bal, e.t.cnt, e.t.n_blocks, i);
        if (dst < e.t.out_cap) {
            *(hy_i32x2*)(e.t.out_pairs + 2 * (size_t)dst) = *(const hy_i32x2*)(e.t.pairs + 2 * (size_t)i);
            if (e.smax) e.out_smax[dst] = e.smax[i];
            if (e.smean) e.out_smean[dst] = e.smean[i];
        }
    }
    long long a, b;
    ev_write_ptr(e.t, i, a, b);
}

extern "C" size_t sed_events_select_ws_bytes(long long pairs_capacity, long long n_cols) {
    return ev_ws_bytes("sed_events_select", pairs_capacity, n_cols, 1);
}

extern "C" int sed_events_select(const int64_t* ev_ptr, const int32_t* ev_pairs, const float* score_max, const float* score_mean,
                                 long long pairs_capacity, long long n_cols, int n_rec, int NC, int key, const float* min_score,
                                 int64_t* out_ptr, int32_t* out_pairs, float* out_score_max, float* out_score_mean,
                                 long long out_capacity, void* ws, size_t ws_bytes, int32_t* err, void* stream) {
    const char* who = "sed_events_select";
    EV_NEED(who, ev_ptr && ev_pairs && min_score && out_ptr && out_pairs && ws && err, "null argument");
    EV_NEED(who, key == 0 || key == 1, "key must be 0 (score_max) or 1 (score_mean)");
    EV_NEED(who, key == 0 ? score_max != nullptr : score_mean != nullptr, "the key's score array is null");
    EV_NEED(who, (score_max != nullptr) == (out_score_max != nullptr) && (score_mean != nullptr) == (out_score_mean != nullptr),
            "a score array and its output go together or are both null");
    EV_NEED(who, (!score_max || out_score_max != score_max) && (!score_mean || out_score_mean != score_mean),
            "an out_score array must not be its input (the select does not run in place)");
    EvsSelArgs e = {{ev_ptr, ev_pairs, pairs_capacity, n_cols, out_ptr, out_pairs, out_capacity, nullptr, nullptr, err,
                     ev_blocks(pairs_capacity)}, key == 0 ? score_max : score_mean, score_max, score_mean, (long long)n_rec * NC,
                    NC, min_score, out_score_max, out_score_mean};
    if (const int rc = ev_check(who, "ev_pairs", "select", e.t, n_rec, NC, ws, ws_bytes, 1)) return rc;
    return ev_launch_compact(k_evs_flag, k_evs_write, e, (hipStream_t)stream);
}
