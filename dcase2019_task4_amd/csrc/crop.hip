// crop.hip - event-aware crop starts for windowed training, drawn from the label pool where it lives (the definition is in
// include/dcase_sed.h).  Two entries:
//   sed_window_activity      one segmented scan over the label pool, flat over its rows, of the triples (n, a, b) with
//                            (n1, a1, b1) o (n2, a2, b2) = (n1 + n2, a1 + a2, b1 + b2 + a1 * n2), reset at every item's first row:
//                            in front of row x of an item it leaves A(x), the active rows before x, and B(x), the sum of
//                            A(0 .. x - 1).  Three passes - k_crop_partial (a tile of CROP_TILE rows per workgroup: the tile's
//                            reduction), k_crop_tiles (one workgroup: the exclusive scan of the tiles' reductions, the
//                            project's one-workgroup scan) and k_crop_write (the tile's scan again, behind the tile's
//                            carry) - and k_crop_weights, a thread per item: W and the present-class mask from three reads of
//                            B per class.  No item is walked by one thread or one workgroup; an item of any length costs
//                            what its rows cost.
//   sed_window_event_starts  a thread per window slot: the class from the mask, the start by bisection over C_c, which is
//                            three reads of B per probe (one of them, B(T3), hoisted).
// Wave steps are shuffles, waves are combined through LDS, the only atomic is the OR into err.  All arithmetic is integer:
// the results do not depend on the launch geometry.  Every row0 / slot_item / start_hi entry is validated before it is
// used as an index; a bisection ends inside [0, hi] whatever the tables hold.
#include "common.h"
#include "kernels.h"
#include "evtable.h"

#define CROP_TILE HY_THREADS
#define CROP_MAX_NC 16

// A scan element: f = an item starts inside what the element covers (the sums are those behind the last such start).
struct CropT {
    int f, n, a;
    long long b;
};

struct CropArgs {
    const float* pool;           // [total][NC]
    const int64_t* row0;         // [n_items + 1]
    long long total, n_tiles;
    int n_items, NC, T3;
    const int32_t* hi;           // start_hi [n_items]
    int32_t* A;                  // [total + n_items][NC]: item i's A(0 .. R_i) from row row0[i] + i
    int64_t* B;
    int64_t* W;                  // [n_items][NC]
    uint32_t* present;           // [n_items]
    int64_t* tb;                 // ws: [n_tiles][NC] a tile's b, after k_crop_tiles the b in front of the tile
    int32_t* ta;                 // ws: [n_tiles][NC]
    int32_t* tn;                 // ws: [n_tiles] a tile's n and f (the same for every class)
    int32_t* tf;
    int32_t* err;
};

__device__ __forceinline__ CropT crop_none() { return CropT{0, 0, 0, 0ll}; }

__device__ __forceinline__ CropT crop_comb(const CropT& l, const CropT& r) {
    if (r.f) return r;
    return CropT{l.f, l.n + r.n, l.a + r.a, l.b + r.b + (long long)l.a * r.n};
}

__device__ __forceinline__ CropT crop_shfl_up(const CropT& v, int o) {
    return CropT{__shfl_up(v.f, o), __shfl_up(v.n, o), __shfl_up(v.a, o), __shfl_up(v.b, o)};
}

// The inclusive scan of a wave.
__device__ __forceinline__ CropT crop_wave_scan(CropT v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const CropT p = crop_shfl_up(v, o);
        if (lane >= o) v = crop_comb(p, v);
    }
    return v;
}

// The inclusive scan of a workgroup of HY_THREADS (every thread calls it); part: HY_WAVES elements of LDS that no wave
// still reads.
__device__ __forceinline__ CropT crop_block_scan(CropT v, CropT* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = crop_wave_scan(v, lane);
    if (lane == 63) part[wave] = v;
    __syncthreads();
    CropT before = crop_none();
#pragma unroll
    for (int k = 0; k < HY_WAVES - 1; ++k)
        if (k < wave) before = crop_comb(before, part[k]);
    return crop_comb(before, v);
}

// What a thread of the partial and the write pass knows of its row x.  A row that no item with valid bounds owns starts a
// segment of its own and is inactive: nothing flows across it, nothing is written for it.
struct CropRow {
    bool in, ok, head, last;
    long long item;
    uint32_t act;                // bit c: label_pool[x][c] > 0
};

__device__ __forceinline__ CropRow crop_row(const CropArgs& e, long long x) {
    CropRow r = {x < e.total, false, false, false, 0, 0u};
    if (!r.in) return r;
    long long a, b;
    r.item = hy_column(e.row0, e.n_items, x);
    r.ok = hy_bounds(e.row0, r.item, e.total, a, b) && x >= a && x < b;
    r.head = !r.ok || x == a;
    r.last = r.ok && x == b - 1;
    if (r.ok) {
        const float* row = e.pool + (size_t)x * e.NC;
        for (int c = 0; c < e.NC; ++c) r.act |= (row[c] > 0.0f ? 1u : 0u) << c;      // false for a NaN
    }
    return r;
}

__device__ __forceinline__ CropT crop_element(const CropRow& r, int c) {
    return r.in ? CropT{r.head ? 1 : 0, 1, (int)((r.act >> c) & 1u), 0ll} : crop_none();
}

__global__ __launch_bounds__(HY_THREADS) void k_crop_partial(CropArgs e) {
    __shared__ CropT part[2][HY_WAVES];
    const long long tile = blockIdx.x;
    const CropRow r = crop_row(e, tile * CROP_TILE + threadIdx.x);
    for (int c = 0; c < e.NC; ++c) {
        const CropT v = crop_block_scan(crop_element(r, c), part[c & 1]);
        if (threadIdx.x == HY_THREADS - 1) {
            e.ta[tile * e.NC + c] = v.a;
            e.tb[tile * e.NC + c] = v.b;
            if (c == 0) {
                e.tn[tile] = v.n;
                e.tf[tile] = v.f;
            }
        }
    }
}

// One workgroup, a fixed order, class after class: (ta, tb)[t][c] = the sums of the tiles in front of tile t that reach it.
__global__ __launch_bounds__(1024) void k_crop_tiles(CropArgs e) {
    __shared__ CropT part[16];
    __shared__ CropT s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = 0; c < e.NC; ++c) {
        if (tid == 0) s_carry = crop_none();
        __syncthreads();
        for (long long i0 = 0; i0 < e.n_tiles; i0 += 1024) {
            const long long i = i0 + tid;
            const CropT own = i < e.n_tiles ? CropT{e.tf[i], e.tn[i], e.ta[i * e.NC + c], e.tb[i * e.NC + c]} : crop_none();
            const CropT incl = crop_wave_scan(own, lane);
            CropT excl = crop_shfl_up(incl, 1);
            if (lane == 0) excl = crop_none();
            if (lane == 63) part[wave] = incl;
            __syncthreads();
            CropT before = s_carry;
            for (int k = 0; k < wave; ++k) before = crop_comb(before, part[k]);
            if (i < e.n_tiles) {
                excl = crop_comb(before, excl);
                e.ta[i * e.NC + c] = excl.a;
                e.tb[i * e.NC + c] = excl.b;
            }
            __syncthreads();
            if (tid == 1023) s_carry = crop_comb(before, incl);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(HY_THREADS) void k_crop_write(CropArgs e) {
    __shared__ CropT part[2][HY_WAVES];
    const long long tile = blockIdx.x, x = tile * CROP_TILE + threadIdx.x;
    const CropRow r = crop_row(e, x);
    for (int c = 0; c < e.NC; ++c) {
        const CropT v = crop_block_scan(crop_element(r, c), part[c & 1]);
        if (!r.ok) continue;
        const int act = (int)((r.act >> c) & 1u);
        long long A = 0, B = 0;
        if (!r.head) {                                                               // v = (what lies in front) o (1, act, 0)
            A = v.a - act;
            B = v.b - A;
            if (!v.f) {                                                              // the item began in an earlier tile
                const long long ca = e.ta[tile * e.NC + c];
                B += e.tb[tile * e.NC + c] + ca * (v.n - 1);
                A += ca;
            }
        }
        const size_t o = (size_t)(x + r.item) * e.NC + c;
        e.A[o] = (int32_t)A;
        e.B[o] = B;
        if (r.last) {
            e.A[o + e.NC] = (int32_t)(A + act);
            e.B[o + e.NC] = B + A;
        }
    }
}

// B(x) of (item, class), x >= 0: `at` = the element of A / B that holds the pair's A(0) / B(0), R the item's rows.
__device__ __forceinline__ long long crop_B(const int32_t* A, const int64_t* B, size_t at, int NC, long long R, long long x) {
    if (x <= R) return B[at + (size_t)x * NC];
    return B[at + (size_t)R * NC] + (x - R) * (long long)A[at + (size_t)R * NC];
}

// C_c(s) + B(T3): the activity that the windows starting at 0 .. s cover, 0 <= s.
__device__ __forceinline__ long long crop_C(const int32_t* A, const int64_t* B, size_t at, int NC, long long R, int T3, long long s) {
    return crop_B(A, B, at, NC, R, s + 1 + T3) - crop_B(A, B, at, NC, R, s + 1);
}

__global__ __launch_bounds__(HY_THREADS) void k_crop_weights(CropArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (i >= e.n_items) return;
    long long a, b;
    if (!(hy_bounds(e.row0, i, e.total, a, b) && a < b)) {
        atomicOr(e.err, 16);
        return;
    }
    const long long hi = e.hi[i];
    if (hi < 0) {
        atomicOr(e.err, 32);
        return;
    }
    uint32_t mask = 0u;
    for (int c = 0; c < e.NC; ++c) {
        const size_t at = (size_t)(a + i) * e.NC + c;
        const long long w = crop_C(e.A, e.B, at, e.NC, b - a, e.T3, hi) - crop_B(e.A, e.B, at, e.NC, b - a, e.T3);
        e.W[i * e.NC + c] = w;
        mask |= (w > 0 ? 1u : 0u) << c;
    }
    e.present[i] = mask;
}

__global__ void k_crop_err(int32_t* err, int bit) { atomicOr(err, bit); }

struct CropStartArgs {
    const uint64_t* u;
    const int32_t* v;
    const uint8_t* m;
    const int32_t* slot_item;
    long long n_slots;
    const int32_t* hi;
    const int32_t* clip_frames;
    int pool_ratio;
    const int64_t* row0;
    long long total;
    int n_items, NC, T3;
    const int32_t* A;
    const int64_t* B;
    const int64_t* W;
    const uint32_t* present;
    int32_t* start3;
    int32_t* cls;
    int32_t* err;
};

__global__ __launch_bounds__(HY_THREADS) void k_crop_starts(CropStartArgs e) {
    const long long j = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (j >= e.n_slots) return;
    const long long i = e.slot_item[j];
    long long a, b;
    if (i < 0 || i >= e.n_items || !(hy_bounds(e.row0, i, e.total, a, b) && a < b)) {
        atomicOr(e.err, 16);
        return;
    }
    const long long hi = e.hi[i];
    if (hi < 0 || hi * e.pool_ratio >= e.clip_frames[i]) {
        atomicOr(e.err, 32);
        return;
    }
    const uint64_t u = e.u[j];
    const uint32_t mask = e.present[i] & ((1u << e.NC) - 1u);
    const int P = __popc(mask);
    long long start;
    int c = -1;
    if (!e.m[j] || P == 0) {
        start = (long long)__umul64hi(u, (uint64_t)(hi + 1));
    } else {
        int k = (int)((uint32_t)e.v[j] % (uint32_t)P);
        for (c = 0; c < e.NC - 1; ++c)
            if ((mask >> c) & 1u) {
                if (k == 0) break;
                --k;
            }
        const long long w = e.W[i * e.NC + c];
        const size_t at = (size_t)(a + i) * e.NC + c;
        const long long target = (long long)__umul64hi(u, (uint64_t)(w > 0 ? w : 0)) + crop_B(e.A, e.B, at, e.NC, b - a, e.T3);
        long long lo = 0, h = hi;                                                    // C(h) > target: C(hi) = W
        while (lo < h) {
            const long long mid = (lo + h) >> 1;
            if (crop_C(e.A, e.B, at, e.NC, b - a, e.T3, mid) > target) h = mid;
            else lo = mid + 1;
        }
        start = lo;
    }
    e.start3[j] = (int32_t)start;
    e.cls[j] = c;
}

static long long crop_tiles(long long total_rows) { return (total_rows + CROP_TILE - 1) / CROP_TILE; }

extern "C" size_t sed_window_activity_ws_bytes(long long total_label_rows, int n_items, int nclass) {
    if (!(total_label_rows >= 1 && total_label_rows < (1ll << 31) && n_items >= 1 && n_items < (1 << 26) && nclass >= 1)) {
        sed_set_error("sed_window_activity_ws_bytes: need 1 <= total_label_rows < 2^31, 1 <= n_items < 2^26 and nclass >= 1");
        return 0;
    }
    const size_t t = (size_t)crop_tiles(total_label_rows);
    return t * nclass * (sizeof(int64_t) + sizeof(int32_t)) + t * 2 * sizeof(int32_t);
}

extern "C" int sed_window_activity(const float* label_pool, const int64_t* label_row0, long long total_label_rows, int n_items,
                                   int nclass, const int32_t* start_hi, int T3, int32_t* A, int64_t* B, int64_t* W,
                                   uint32_t* present, void* ws, size_t ws_bytes, int32_t* err, void* stream) {
    const char* who = "sed_window_activity";
    hipStream_t st = (hipStream_t)stream;
    EV_NEED(who, label_pool && label_row0 && start_hi && A && B && W && present && ws && err, "null argument");
    const size_t need = sed_window_activity_ws_bytes(total_label_rows, n_items, nclass);
    EV_NEED(who, need != 0, "need 1 <= total_label_rows < 2^31, 1 <= n_items < 2^26 and nclass >= 1");
    EV_NEED(who, T3 >= 1, "T3 must be >= 1");
    EV_NEED(who, ((uintptr_t)B % 8) == 0 && ((uintptr_t)W % 8) == 0 && ((uintptr_t)ws % 8) == 0, "B, W and ws must be 8-byte aligned");
    if (ws_bytes != need) {
        sed_set_error("%s: ws_bytes must be the value %s_ws_bytes returned for these sizes", who, who);
        return SED_ERR_WORKSPACE;
    }
    if (nclass > CROP_MAX_NC) {                                                      // the mask's limit: nothing else is launched
        hipLaunchKernelGGL(k_crop_err, dim3(1), dim3(1), 0, st, err, 8);
        SED_CHECK_LAUNCH();
        return SED_OK;
    }
    const long long t = crop_tiles(total_label_rows);
    int64_t* tb = (int64_t*)ws;
    int32_t* ta = (int32_t*)(tb + (size_t)t * nclass);
    int32_t* tn = ta + (size_t)t * nclass;
    const CropArgs e = {label_pool, label_row0, total_label_rows, t, n_items, nclass, T3, start_hi, A, B, W, present,
                        tb, ta, tn, tn + t, err};
    hipLaunchKernelGGL(k_crop_partial, dim3((unsigned)t), dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_crop_tiles, dim3(1), dim3(1024), 0, st, e);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_crop_write, dim3((unsigned)t), dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_crop_weights, dim3((unsigned)ev_blocks(n_items)), dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_window_event_starts(const uint64_t* u, const int32_t* v, const uint8_t* m, const int32_t* slot_item,
                                       long long n_slots, const int32_t* start_hi, const int32_t* clip_frames, int pool_ratio,
                                       const int64_t* label_row0, long long total_label_rows, int n_items, int nclass, int T3,
                                       const int32_t* A, const int64_t* B, const int64_t* W, const uint32_t* present,
                                       int32_t* start3, int32_t* chosen, int32_t* err, void* stream) {
    const char* who = "sed_window_event_starts";
    hipStream_t st = (hipStream_t)stream;
    EV_NEED(who, u && v && m && slot_item && start_hi && clip_frames && label_row0 && A && B && W && present && start3 && chosen && err,
            "null argument");
    EV_NEED(who, total_label_rows >= 1 && total_label_rows < (1ll << 31) && n_items >= 1 && n_items < (1 << 26) && nclass >= 1,
            "need 1 <= total_label_rows < 2^31, 1 <= n_items < 2^26 and nclass >= 1");
    EV_NEED(who, T3 >= 1 && pool_ratio >= 1, "T3 and pool_ratio must be >= 1");
    EV_NEED(who, n_slots >= 0 && n_slots < (1ll << 31), "need 0 <= n_slots < 2^31");
    EV_NEED(who, ((uintptr_t)u % 8) == 0 && ((uintptr_t)B % 8) == 0 && ((uintptr_t)W % 8) == 0, "u, B and W must be 8-byte aligned");
    if (nclass > CROP_MAX_NC) {
        hipLaunchKernelGGL(k_crop_err, dim3(1), dim3(1), 0, st, err, 8);
        SED_CHECK_LAUNCH();
        return SED_OK;
    }
    if (n_slots == 0) return SED_OK;
    const CropStartArgs e = {u, v, m, slot_item, n_slots, start_hi, clip_frames, pool_ratio, label_row0, total_label_rows,
                             n_items, nclass, T3, A, B, W, present, start3, chosen, err};
    hipLaunchKernelGGL(k_crop_starts, dim3((unsigned)ev_blocks(n_slots)), dim3(HY_THREADS), 0, st, e);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
