// hyst.hip - two-threshold (hysteresis) decode in the event domain: sed_events_hysteresis keeps the events of a LOW-threshold
// table that an event of a HIGH-threshold table confirms (the definition is in include/dcase_sed.h).  Both tables are columns
// of one CSR event array as sed_stitch_sweep leaves it: the decision P > thr is monotone in thr and the binary median filter
// is monotone in its input, so with one median window every high event lies inside exactly one low event, and hysteresis is
// "a low event [on, off) survives iff some high event starts in [on, off)".  No timeline, no tile carry, no halo: a
// select-and-compact over two sorted tables.
//
// The work is flat over the indices of `pairs`, not over columns (a column has no length limit):
//   k_hyst_flag    a thread owns index i: it finds the low column that holds i by bisection over lo_ptr, bisects that column of
//                  the high table for the first onset >= on and keeps the event iff that onset exists and is < off.  A wave's
//                  decisions are one ballot word, a workgroup's count is the popcounts of its four words.  The same thread
//                  checks that the onsets around i strictly increase inside its low and inside its high column (err 64).
//   k_hyst_scan    one workgroup: exclusive scan of the workgroup counts in place, the total behind them; capacity check
//   k_hyst_write   index i again: a kept event goes to (offset of its workgroup) + (kept ones in front of it in the workgroup),
//                  both from the ballot words; thread c <= n_cols writes out_ptr[c] = the kept events in front of lo_ptr[c]
//                  and validates column c's four bounds (err 16).
// Three launches whatever the number of columns; the grids are sized from pairs_capacity (the true count is device data).
// Every ptr entry is validated before it is used as an index: the bisections only ever read lo_ptr / hi_ptr [0, n_cols] and
// pairs [0, pairs_capacity), whatever the tables hold.  No atomics but the OR into err, integer results only.
#include "common.h"
#include "kernels.h"

#define HY_THREADS 256
#define HY_WAVES (HY_THREADS / 64)
typedef __attribute__((ext_vector_type(2))) int32_t hy_i32x2;   // one (onset, offset) pair: an 8-byte load / store

struct HyArgs {
    const int64_t *lo_ptr, *hi_ptr;
    const int32_t* pairs;
    long long cap, n_cols;       // pairs_capacity; columns
    int64_t* out_ptr;
    int32_t* out_pairs;
    long long out_cap;
    uint64_t* bal;               // ws: [n_blocks][HY_WAVES] the keep decisions of 64 indices
    int32_t* cnt;                // ws: [n_blocks + 1] kept per workgroup; after the scan the kept in front of it, then the total
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

__global__ __launch_bounds__(HY_THREADS) void k_hyst_flag(HyArgs h) {
    __shared__ int s_cnt[HY_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * HY_THREADS + tid;
    bool keep = false;
    if (i < h.cap) {
        const int on = h.pairs[2 * (size_t)i], off = h.pairs[2 * (size_t)i + 1];
        bool unsorted = false;
        long long a, b, ha, hb;
        const long long c = hy_column(h.lo_ptr, h.n_cols, i);
        if (hy_bounds(h.lo_ptr, c, h.cap, a, b) && i >= a && i < b) {               // i is event i - a of low column c
            if (i + 1 < b && h.pairs[2 * (size_t)(i + 1)] <= on) unsorted = true;
            if (hy_bounds(h.hi_ptr, c, h.cap, ha, hb)) {
                long long lo = ha, hi = hb;                                          // the first high event with onset >= on
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (h.pairs[2 * (size_t)mid] < on) lo = mid + 1;
                    else hi = mid;
                }
                keep = lo < hb && h.pairs[2 * (size_t)lo] < off;
            }
        }
        const long long ch = hy_column(h.hi_ptr, h.n_cols, i);
        if (hy_bounds(h.hi_ptr, ch, h.cap, ha, hb) && i >= ha && i + 1 < hb && h.pairs[2 * (size_t)(i + 1)] <= on) unsorted = true;
        if (unsorted) atomicOr(h.err, 64);
    }
    const uint64_t word = __ballot(keep);
    if (lane == 0) {
        h.bal[(size_t)blockIdx.x * HY_WAVES + wave] = word;
        s_cnt[wave] = __popcll(word);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < HY_WAVES; ++w) n += s_cnt[w];
        h.cnt[blockIdx.x] = n;
    }
}

// cnt[b] = the kept events in front of workgroup b, cnt[n_blocks] = all of them (one workgroup; a fixed order).  The total
// stays below 2^31: an index is kept at most once.
__global__ __launch_bounds__(1024) void k_hyst_scan(HyArgs h) {
    __shared__ int part[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = h.n_blocks;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < n; i0 += 1024) {
        const long long i = i0 + tid;
        const int v = i < n ? h.cnt[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int m = __shfl_up(incl, o);
            if (lane >= o) incl += m;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int before = s_carry;
        for (int k = 0; k < wave; ++k) before += part[k];
        if (i < n) h.cnt[i] = before + incl - v;
        __syncthreads();
        if (tid == 1023) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        h.cnt[n] = s_carry;
        if (s_carry > h.out_cap) atomicOr(h.err, 2);
    }
}

// The kept events among the indices [0, p) of pairs, 0 <= p <= cap, from the scanned counts and the ballot words.
__device__ __forceinline__ long long hy_kept_before(const HyArgs& h, long long p) {
    const long long blk = p / HY_THREADS;
    if (blk >= h.n_blocks) return h.cnt[h.n_blocks];                                 // p == cap on a workgroup edge
    long long n = h.cnt[blk];
    const long long w1 = p >> 6;
    for (long long w = blk * HY_WAVES; w < w1; ++w) n += __popcll(h.bal[w]);
    if (p & 63) n += __popcll(h.bal[w1] & ((1ull << (p & 63)) - 1ull));
    return n;
}

__global__ __launch_bounds__(HY_THREADS) void k_hyst_write(HyArgs h) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (i < h.cap && ((h.bal[i >> 6] >> (i & 63)) & 1ull)) {
        const long long dst = hy_kept_before(h, i);
        if (dst < h.out_cap) *(hy_i32x2*)(h.out_pairs + 2 * (size_t)dst) = *(const hy_i32x2*)(h.pairs + 2 * (size_t)i);
    }
    if (i <= h.n_cols) {
        const long long p = h.lo_ptr[i];
        h.out_ptr[i] = hy_kept_before(h, p < 0 ? 0 : (p > h.cap ? h.cap : p));
        long long a, b;
        if (i < h.n_cols && !(hy_bounds(h.lo_ptr, i, h.cap, a, b) && hy_bounds(h.hi_ptr, i, h.cap, a, b))) atomicOr(h.err, 16);
    }
}

static long long hy_blocks(long long cap) { return (cap + HY_THREADS - 1) / HY_THREADS; }
static size_t hy_bal_bytes(long long cap) { return (size_t)hy_blocks(cap) * HY_WAVES * sizeof(uint64_t); }

static bool hy_sizes_ok(long long pairs_capacity, long long n_cols) {
    return pairs_capacity >= 0 && pairs_capacity < (1ll << 31) && n_cols >= 1 && n_cols < (1ll << 26);
}

extern "C" size_t sed_events_hysteresis_ws_bytes(long long pairs_capacity, long long n_cols) {
    if (!hy_sizes_ok(pairs_capacity, n_cols)) {
        sed_set_error("sed_events_hysteresis_ws_bytes: need 0 <= pairs_capacity < 2^31 and 1 <= n_cols < 2^26");
        return 0;
    }
    return hy_bal_bytes(pairs_capacity) + (size_t)(hy_blocks(pairs_capacity) + 1) * sizeof(int32_t);
}

#define HY_NEED(cond, msg)                                          \
    do {                                                            \
        if (!(cond)) {                                              \
            sed_set_error("sed_events_hysteresis: %s", msg);        \
            return SED_ERR_BAD_ARG;                                 \
        }                                                           \
    } while (0)

extern "C" int sed_events_hysteresis(const int64_t* lo_ptr, const int64_t* hi_ptr, const int32_t* pairs, long long pairs_capacity,
                                     long long n_cols, int64_t* out_ptr, int32_t* out_pairs, long long out_capacity, void* ws,
                                     size_t ws_bytes, int32_t* err, void* stream) {
    HY_NEED(lo_ptr && hi_ptr && pairs && out_ptr && out_pairs && ws && err, "null argument");
    HY_NEED(hy_sizes_ok(pairs_capacity, n_cols), "need 0 <= pairs_capacity < 2^31 and 1 <= n_cols < 2^26");
    HY_NEED(out_capacity >= 0, "out_capacity must be >= 0");
    HY_NEED(((uintptr_t)pairs % 8) == 0 && ((uintptr_t)out_pairs % 8) == 0 && ((uintptr_t)ws % 8) == 0,
            "pairs, out_pairs and ws must be 8-byte aligned");
    HY_NEED(out_pairs != pairs, "out_pairs must not be pairs (the select does not run in place)");
    if (ws_bytes != sed_events_hysteresis_ws_bytes(pairs_capacity, n_cols)) {
        sed_set_error("sed_events_hysteresis: ws_bytes must be the value sed_events_hysteresis_ws_bytes returned for these sizes");
        return SED_ERR_WORKSPACE;
    }
    const long long n_blocks = hy_blocks(pairs_capacity);
    const HyArgs h = {lo_ptr, hi_ptr, pairs, pairs_capacity, n_cols, out_ptr, out_pairs, out_capacity, (uint64_t*)ws,
                      (int32_t*)((char*)ws + hy_bal_bytes(pairs_capacity)), err, n_blocks};
    hipStream_t st = (hipStream_t)stream;
    if (n_blocks) {                                                                  // (an empty pairs array has nothing to flag)
        hipLaunchKernelGGL(k_hyst_flag, dim3((unsigned)n_blocks), dim3(HY_THREADS), 0, st, h);
        SED_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_hyst_scan, dim3(1), dim3(1024), 0, st, h);
    SED_CHECK_LAUNCH();
    const long long items = pairs_capacity > n_cols + 1 ? pairs_capacity : n_cols + 1;
    hipLaunchKernelGGL(k_hyst_write, dim3((unsigned)hy_blocks(items)), dim3(HY_THREADS), 0, st, h);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
