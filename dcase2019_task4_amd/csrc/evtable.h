// evtable.h - what an event-domain operator needs of a CSR event table: the geometry of a flat pass over the indices of its
// pairs array, the column lookup, the validation of a column's bounds and the rank of an index among the flagged ones.  A
// flat pass gives every index of pairs one thread; a wave's decisions are one ballot word, a workgroup's count is the
// popcounts of its four words, and a one-workgroup scan turns the counts into offsets.  evproc.hip includes it; hyst.hip,
// where these helpers were written first, keeps its own identical copies (it is left exactly as it was).
#pragma once
#include <stdint.h>

#define HY_THREADS 256
#define HY_WAVES (HY_THREADS / 64)
typedef __attribute__((ext_vector_type(2))) int32_t hy_i32x2;   // one (onset, offset) pair: an 8-byte load / store

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
