// raster.hip - a CSR event table turned back into label rows, in place in a label pool (the definition is in
// include/dcase_sed.h).  The fifth event-domain operator beside hyst.hip, evproc.hip and evscore.hip, and the only one whose
// output is in the frame domain.  Two launches:
//   k_ras_check   flat over the indices of ev_pairs (the geometry of evtable.h): a thread finds the column of its index
//                 (hy_column / hy_bounds) and, when the column is the one `point` selects for its class, validates the event
//                 against its recording and its predecessor (err 64).  Thread c < n_cols validates column c's bounds, thread
//                 r < n_rec recording r's frame range and destination rows (err 16), thread c < NC point[c] (err 8).  It
//                 writes nothing but err.
//   k_ras_rows    a gather, flat over the timeline rows: a thread finds the recording of its row by the same bisection over
//                 rec_frame0 and, per class, the last event of the selected column with on <= u by bisection over the
//                 column's onsets.  Every addressed element is written exactly once (replace) or read once and written at
//                 most once (maximum); the destination is not cleared first.  A class, column or recording the check pass
//                 rejects is skipped silently here.  16-byte stores when NC % 4 == 0 and dst is 16-byte aligned.
// Values and old contents are moved as 32-bit words: a NaN payload, -0.0f and denormals pass through bit for bit; the only
// floating-point operation is the comparison v > old of the maximum.
// No LDS, no workspace, no atomics but the OR into err.  Every ev_ptr / rec_frame0 / dst_row0 entry is validated before it is
// used as an index; a bisection over a column that is not sorted still ends inside the column.
#include "common.h"
#include "kernels.h"
#include "evtable.h"

typedef __attribute__((ext_vector_type(4))) uint32_t ras_u32x4;

struct RasArgs {
    const int64_t* ptr;
    const int32_t* pairs;
    const uint32_t* value;       // [cap] the bits of the fp32 values, or null: 1.0f
    long long cap, n_cols;
    int n_points;
    const int32_t* point;        // [NC] or null: 0
    const int64_t* f0;           // rec_frame0 [n_rec + 1]
    int n_rec, NC;
    uint32_t* dst;               // [dst_rows][NC]
    long long dst_rows;
    const int64_t* row0;         // dst_row0 [n_rec] or null: rec_frame0
    int combine;
    int32_t* err;
};

#define RAS_ONE 0x3f800000u      // 1.0f

// Recording r is [fa, fb) in the flat row index, 0 <= fa <= fb <= dst_rows: the rows of distinct destinations cannot number
// more than dst_rows, which bounds the flat index without a total of its own.
__device__ __forceinline__ bool ras_rec(const RasArgs& e, long long r, long long& fa, long long& fb) {
    return hy_bounds(e.f0, r, e.dst_rows, fa, fb);
}

// The first destination row of a recording with valid frames [fa, fb): true when all its rows lie inside dst.
__device__ __forceinline__ bool ras_rows(const RasArgs& e, long long r, long long fa, long long fb, long long& d0) {
    d0 = e.row0 ? e.row0[r] : fa;
    return d0 >= 0 && d0 <= e.dst_rows - (fb - fa);
}

__device__ __forceinline__ int ras_point(const RasArgs& e, int c) { return e.point ? e.point[c] : 0; }

__global__ __launch_bounds__(HY_THREADS) void k_ras_check(RasArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    long long a, b, fa, fb, d0;
    if (i < e.n_cols && !hy_bounds(e.ptr, i, e.cap, a, b)) atomicOr(e.err, 16);
    if (i < e.n_rec && !(ras_rec(e, i, fa, fb) && ras_rows(e, i, fa, fb, d0))) atomicOr(e.err, 16);
    if (i < e.NC) {
        const int k = ras_point(e, (int)i);
        if (k < 0 || k >= e.n_points) atomicOr(e.err, 8);
    }
    if (i < e.cap) {
        const long long c = hy_column(e.ptr, e.n_cols, i);
        if (hy_bounds(e.ptr, c, e.cap, a, b) && i >= a && i < b) {                   // i is event i - a of column c
            const long long rec = (c / e.NC) % e.n_rec, k = c / ((long long)e.n_rec * e.NC);
            if (k == ras_point(e, (int)(c % e.NC)) && ras_rec(e, rec, fa, fb)) {
                const hy_i32x2 ev = *(const hy_i32x2*)(e.pairs + 2 * (size_t)i);
                bool bad = ev.x < 0 || ev.x >= ev.y || ev.y > fb - fa;
                if (i > a) bad = bad || ev.x < e.pairs[2 * (size_t)(i - 1) + 1];     // touching the previous event is valid
                if (bad) atomicOr(e.err, 64);
            }
        }
    }
}

// What element (u, c) of recording rec becomes: true when it is written, `w` the word.  `old` is read only by the maximum.
__device__ __forceinline__ bool ras_element(const RasArgs& e, long long rec, long long u, int c, const uint32_t* old, uint32_t& w) {
    const int k = ras_point(e, c);
    if (k < 0 || k >= e.n_points) return false;
    long long a, b;
    if (!hy_bounds(e.ptr, ((long long)k * e.n_rec + rec) * e.NC + c, e.cap, a, b)) return false;
    long long lo = a, hi = b;                                                        // the events [a, lo) have on <= u
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (e.pairs[2 * (size_t)mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    bool covered = false;
    if (lo > a) {
        const hy_i32x2 ev = *(const hy_i32x2*)(e.pairs + 2 * (size_t)(lo - 1));
        covered = ev.x <= u && u < ev.y;
    }
    if (e.combine == 0) {
        w = covered ? (e.value ? e.value[lo - 1] : RAS_ONE) : 0u;
        return true;
    }
    if (!covered) return false;
    const uint32_t v = e.value ? e.value[lo - 1] : RAS_ONE, o = *old;
    w = v;
    return __uint_as_float(v) > __uint_as_float(o);                                  // false for a NaN on either side
}

template <bool VEC>
__global__ __launch_bounds__(HY_THREADS) void k_ras_rows(RasArgs e) {
    const long long t = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (t >= e.dst_rows) return;
    const long long rec = hy_column(e.f0, e.n_rec, t);
    long long fa, fb, d0;
    if (!(ras_rec(e, rec, fa, fb) && t >= fa && t < fb && ras_rows(e, rec, fa, fb, d0))) return;
    const long long u = t - fa;
    uint32_t* row = e.dst + (size_t)(d0 + u) * e.NC;                                 // (d0 + u + 1) * NC <= dst_rows * NC < 2^31
    if (VEC) {
        for (int c0 = 0; c0 < e.NC; c0 += 4) {
            ras_u32x4 w = {0u, 0u, 0u, 0u};
            bool wr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t x = 0u;
                wr[j] = ras_element(e, rec, u, c0 + j, row + c0 + j, x);
                w[j] = x;
            }
            if (wr[0] && wr[1] && wr[2] && wr[3]) {
                *(ras_u32x4*)(row + c0) = w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (wr[j]) row[c0 + j] = w[j];
            }
        }
    } else {
        for (int c = 0; c < e.NC; ++c) {
            uint32_t w = 0u;
            if (ras_element(e, rec, u, c, row + c, w)) row[c] = w;
        }
    }
}

extern "C" int sed_events_rasterize(const int64_t* ev_ptr, const int32_t* ev_pairs, const float* value, long long pairs_capacity,
                                    int n_points, const int32_t* point, const int64_t* rec_frame0, int n_rec, int NC, float* dst,
                                    long long dst_rows, const int64_t* dst_row0, int combine, int32_t* err, void* stream) {
    const char* who = "sed_events_rasterize";
    hipStream_t st = (hipStream_t)stream;
    EV_NEED(who, ev_ptr && ev_pairs && rec_frame0 && dst && err, "null argument");
    EV_NEED(who, NC >= 1 && NC <= 16 && n_rec >= 1 && n_points >= 1 && n_points <= 4096,
            "need 1 <= NC <= 16, n_rec >= 1 and 1 <= n_points <= 4096");
    const long long n_cols = (long long)n_points * n_rec * NC;
    EV_NEED(who, n_cols < (1ll << 26), "need n_points * n_rec * NC < 2^26");
    EV_NEED(who, pairs_capacity >= 0 && pairs_capacity < (1ll << 31), "need 0 <= pairs_capacity < 2^31");
    EV_NEED(who, dst_rows >= 0 && dst_rows * NC < (1ll << 31), "need 0 <= dst_rows and dst_rows * NC < 2^31");
    EV_NEED(who, ((uintptr_t)ev_pairs % 8) == 0, "ev_pairs must be 8-byte aligned");
    EV_NEED(who, ((uintptr_t)dst % 4) == 0, "dst must be 4-byte aligned");
    EV_NEED(who, combine == 0 || combine == 1, "combine must be 0 (replace) or 1 (maximum)");
    const size_t dst_bytes = (size_t)dst_rows * NC * sizeof(float);
    const void* in[7] = {ev_ptr, ev_pairs, value, point, rec_frame0, dst_row0, err};
    const size_t in_bytes[7] = {(size_t)(n_cols + 1) * sizeof(int64_t), (size_t)pairs_capacity * 2 * sizeof(int32_t),
                                (size_t)pairs_capacity * sizeof(float), (size_t)NC * sizeof(int32_t),
                                (size_t)(n_rec + 1) * sizeof(int64_t), (size_t)n_rec * sizeof(int64_t), sizeof(int32_t)};
    for (int k = 0; k < 7; ++k) EV_NEED(who, !in[k] || ev_disjoint(dst, dst_bytes, in[k], in_bytes[k]), "dst overlaps an input");
    const RasArgs e = {ev_ptr, ev_pairs, (const uint32_t*)value, pairs_capacity, n_cols, n_points, point, rec_frame0, n_rec, NC,
                       (uint32_t*)dst, dst_rows, dst_row0, combine, err};
    hipLaunchKernelGGL(k_ras_check, dim3((unsigned)ev_blocks(pairs_capacity > n_cols ? pairs_capacity : n_cols)),
                       dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    if (dst_rows == 0) return SED_OK;
    const dim3 grid((unsigned)ev_blocks(dst_rows));
    if (NC % 4 == 0 && ((uintptr_t)dst % 16) == 0) hipLaunchKernelGGL(k_ras_rows<true>, grid, dim3(HY_THREADS), 0, st, e);
    else hipLaunchKernelGGL(k_ras_rows<false>, grid, dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
