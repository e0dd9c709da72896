// evtable.h - what an event-domain operator needs of a CSR event table, stated once for evproc.hip, evscore.hip and raster.hip: the
// geometry of a flat pass over the indices of its pairs array, the column lookup, the validation of a column's bounds, the
// rank of an index among the flagged ones, and the compaction built from them.  A flat pass gives every index of pairs one
// thread; a wave's decisions are one ballot word, a workgroup's count is the popcounts of its four words, a one-workgroup
// scan turns the counts into offsets (err 2), and a write pass puts the flagged rows at their rank while thread
// c <= n_cols writes out_ptr[c] and validates column c (err 16).  Behind the device helpers: the host's sizes, the
// workspace, the argument checks and the launch sequence of such an entry.  hyst.hip, where the pass was written first, is
// the only file that keeps its own copies (it is left exactly as it was).
#pragma once
#include <stdint.h>
#include "common.h"

#define HY_THREADS 256
#define HY_WAVES (HY_THREADS / 64)
typedef __attribute__((ext_vector_type(2))) int32_t hy_i32x2;   // one (onset, offset) pair: an 8-byte load / store

// What the passes of a compacting operator share; an operator's argument struct embeds it beside its own fields.
struct EvTable {
    const int64_t* ptr;
    const int32_t* pairs;
    long long cap, n_cols;       // pairs_capacity; columns
    int64_t* out_ptr;
    int32_t* out_pairs;
    long long out_cap;
    uint64_t* bal;               // ws: [n_blocks][HY_WAVES] the flags of 64 indices that decide what is written
    int32_t* cnt;                // ws: [n_blocks + 1] flags per workgroup; after the scan those in front of it, then the total
    int32_t* err;
    long long n_blocks;          // ceil(cap / HY_THREADS)
};

// The column that may hold index i: the last c in [0, n_cols) with ptr[c] <= i (column 0 when there is none).  Reads
// ptr[0 .. n_cols - 1] only; the caller validates the column's bounds.  The last column is tried first: the grid covers the
// capacity, so most indices lie behind every event and end here after one load instead of a whole bisection.
__device__ __forceinline__ long long hy_column(const int64_t* ptr, long long n_cols, long long i) {
    long long lo = 0, hi = n_cols - 1;
    if (ptr[hi] <= i) return hi;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Column c of ptr is [a, b) with 0 <= a <= b <= cap: the only columns whose events are addressed.
__device__ __forceinline__ bool hy_bounds(const int64_t* ptr, long long c, long long cap, long long& a, long long& b) {
    a = ptr[c];
    b = ptr[c + 1];
    return a >= 0 && a <= b && b <= cap;
}

// The flagged indices among [0, p) of pairs, 0 <= p <= cap, from the scanned workgroup counts (cnt[n_blocks] = the total) and
// the ballot words.
__device__ __forceinline__ long long hy_flagged_before(const uint64_t* bal, const int32_t* cnt, long long n_blocks, long long p) {
    const long long blk = p / HY_THREADS;
    if (blk >= n_blocks) return cnt[n_blocks];                                       // p == cap on a workgroup edge
    long long n = cnt[blk];
    const long long w1 = p >> 6;
    for (long long w = blk * HY_WAVES; w < w1; ++w) n += __popcll(bal[w]);
    if (p & 63) n += __popcll(bal[w1] & ((1ull << (p & 63)) - 1ull));
    return n;
}

__device__ __forceinline__ bool ev_bit(const uint64_t* bal, long long i) { return (bal[i >> 6] >> (i & 63)) & 1ull; }

// The parameters' entry of column c: (point, class); span = n_rec * NC, the columns of one point.
__device__ __forceinline__ long long ev_param(long long span, int NC, long long c) { return (c / span) * NC + c % NC; }

// The end of a flag pass (every thread of the workgroup calls it): the wave's ballot word, the workgroup's count.
__device__ __forceinline__ void ev_ballot_count(bool flag, uint64_t* bal, int32_t* cnt) {
    __shared__ int s_cnt[HY_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t word = __ballot(flag);
    if (lane == 0) {
        bal[(size_t)blockIdx.x * HY_WAVES + wave] = word;
        s_cnt[wave] = __popcll(word);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < HY_WAVES; ++w) n += s_cnt[w];
        cnt[blockIdx.x] = n;
    }
}

// The end of a write pass: thread i <= n_cols writes out_ptr[i], the flagged indices in front of ptr[i], and validates
// column i (err 16).  True for a column with valid bounds [a, b).
__device__ __forceinline__ bool ev_write_ptr(const EvTable& t, long long i, long long& a, long long& b) {
    if (i <= t.n_cols) {
        const long long p = t.ptr[i];
        t.out_ptr[i] = hy_flagged_before(t.bal, t.cnt, t.n_blocks, p < 0 ? 0 : (p > t.cap ? t.cap : p));
        if (i < t.n_cols) {
            if (hy_bounds(t.ptr, i, t.cap, a, b)) return true;
            atomicOr(t.err, 16);
        }
    }
    return false;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static long long ev_blocks(long long n) { return (n + HY_THREADS - 1) / HY_THREADS; }
static size_t ev_bal_bytes(long long cap) { return (size_t)ev_blocks(cap) * HY_WAVES * sizeof(uint64_t); }
static size_t ev_cnt_bytes(long long cap) { return (size_t)(ev_blocks(cap) + 1) * sizeof(int32_t); }

// The workspace of `who` (an entry's name): `planes` ballot planes, then one [n_blocks + 1] array for each.
static size_t ev_ws_bytes(const char* who, long long pairs_capacity, long long n_cols, int planes) {
    if (!(pairs_capacity >= 0 && pairs_capacity < (1ll << 31) && n_cols >= 1 && n_cols < (1ll << 26))) {
        sed_set_error("%s_ws_bytes: need 0 <= pairs_capacity < 2^31 and 1 <= n_cols < 2^26", who);
        return 0;
    }
    return planes * (ev_bal_bytes(pairs_capacity) + ev_cnt_bytes(pairs_capacity));
}

// The byte ranges [x, x + nx) and [y, y + ny) share nothing (an empty range shares nothing with anything).
static bool ev_disjoint(const void* x, size_t nx, const void* y, size_t ny) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return nx == 0 || ny == 0 || a + nx <= b || b + ny <= a;
}

#define EV_NEED(who, cond, fmt, ...)                                \
    do {                                                            \
        if (!(cond)) {                                              \
            sed_set_error("%s: " fmt, who, ##__VA_ARGS__);          \
            return SED_ERR_BAD_ARG;                                 \
        }                                                           \
    } while (0)

// The argument checks the compacting entries share, behind an entry's own (its pointers among them): `who` is the entry's
// name, `pairs_name` its name for t.pairs and `what` its word for itself in the messages.  Then t.bal / t.cnt: the last
// ballot plane of ws and the last array behind the planes (an entry's other planes lie in front of them).
static int ev_check(const char* who, const char* pairs_name, const char* what, EvTable& t, int n_rec, int NC, void* ws,
                    size_t ws_bytes, int planes) {
    const size_t need = ev_ws_bytes(who, t.cap, t.n_cols, planes);
    EV_NEED(who, need != 0, "need 0 <= pairs_capacity < 2^31 and 1 <= n_cols < 2^26");
    EV_NEED(who, n_rec >= 1 && NC >= 1, "n_rec and NC must be >= 1");
    EV_NEED(who, t.n_cols % ((long long)n_rec * NC) == 0, "n_cols must be a multiple of n_rec * NC (K * n_rec * NC columns)");
    EV_NEED(who, t.out_cap >= 0, "out_capacity must be >= 0");
    EV_NEED(who, ((uintptr_t)t.pairs % 8) == 0 && ((uintptr_t)t.out_pairs % 8) == 0 && ((uintptr_t)ws % 8) == 0,
            "%s, out_pairs and ws must be 8-byte aligned", pairs_name);
    EV_NEED(who, t.out_pairs != t.pairs, "out_pairs must not be %s (the %s does not run in place)", pairs_name, what);
    if (ws_bytes != need) {
        sed_set_error("%s: ws_bytes must be the value %s_ws_bytes returned for these sizes", who, who);
        return SED_ERR_WORKSPACE;
    }
    t.bal = (uint64_t*)((char*)ws + (planes - 1) * ev_bal_bytes(t.cap));
    t.cnt = (int32_t*)((char*)ws + planes * ev_bal_bytes(t.cap) + (planes - 1) * ev_cnt_bytes(t.cap));
    return SED_OK;
}

// The one-workgroup exclusive sum of cnt[0 .. n_blocks), the total behind it, the capacity check (err 2); evproc.hip.
int launch_ev_scan(const EvTable& t, hipStream_t st);

// The compaction of the flags `flag` decides: flag (an empty pairs array has nothing to flag), scan, write.  Args embeds
// the table as its member t.
template <class Args>
static int ev_launch_compact(void (*flag)(Args), void (*write)(Args), const Args& e, hipStream_t st) {
    const EvTable& t = e.t;
    if (t.n_blocks) {
        hipLaunchKernelGGL(flag, dim3((unsigned)t.n_blocks), dim3(HY_THREADS), 0, st, e);
        SED_CHECK_LAUNCH();
    }
    if (const int rc = launch_ev_scan(t, st)) return rc;
    const long long items = t.cap > t.n_cols + 1 ? t.cap : t.n_cols + 1;
    hipLaunchKernelGGL(write, dim3((unsigned)ev_blocks(items)), dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
