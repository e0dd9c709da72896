#pragma clang fp contract(off)       // file-wide: the blend's products and sums are individually rounded (see augment.hip)
// stitch.hip - long-recording inference: the posteriors of overlapping windows are blended into one timeline per recording,
// then thresholded, median-filtered and run-length decoded over the WHOLE timeline (sed_stitch_decode; the definitions are
// in include/dcase_sed.h and are the project's own - the reference scores 10-s clips only).
//
// A column (recording, class) has no length limit, so it is split along time: a workgroup owns ST_TILE timeline frames of
// one recording, all classes (the NC floats of a frame are contiguous in the window posteriors and in the timeline).
//   k_stitch_tile<VEC, 0, SWEEP>  blends its frames plus a halo of ST_HALO frames per side (or the reflection at a recording
//                          end) into 0/1 decisions in LDS, median-filters them there (the true neighbours across tile
//                          edges), writes timeline / binary, and counts the onsets of every class with wave ballots
//   k_stitch_scan_cols     one wave per column: exclusive scan of the tile counts in place, the column's total
//   k_stitch_scan_ptr      one workgroup: ev_ptr = exclusive scan of the column totals; capacity check
//   k_stitch_tile<VEC, 1, SWEEP>  recomputes the tile and writes its (onset, offset) frames at ev_ptr[col] + rank
// sed_stitch_sweep decodes K operating points from ONE blend per workgroup with the same four launches and the same
// kernels: SWEEP = true keeps the blend in LDS and loops over a group of points, a column is then (point, recording, class);
// sed_stitch_decode is SWEEP = false, one point.  Both entries go through one host path (st_run); all four entries share the
// host front (st_front, st_ws_slots) and, on the device, StTables with st_rec / st_tile / st_blend.
// Onsets and offsets alternate along a column, so the offsets in front of a tile are the onsets in front of it minus one
// when an event is open across the tile's first edge: one count per (tile, class) is enough.
// sed_stitch_weak (at the end of the file) pools recording-level weak tags over the same tiles and slots: the same blend of the
// posteriors and of the attention, fp64 sums in a fixed order, two launches, no timeline.  sed_stitch_weak_backward (behind it) is
// its transpose: the gradient of a loss on the pooled tags w.r.t. both window tensors, a clear and one tile pass, no atomics.
// sed_stitch_span_tags pools the same tags per span of span3 frames, slots span * ceil(span3 / ST_TILE) + k, and
// sed_stitch_piece_span_tags per span of a PIECE of a recording - some consecutive spans and exactly the windows that cover
// them, the first span at local frame rec_span_off[r], the frames in front of the first and behind the last span in no span.
// All six pooled entries are the same four kernels over one argument struct per direction (StPoolArgs, StPoolBwdArgs); which row
// of tags / sums / g a frame belongs to is said once, by StRows: the rule that validates a recording's rows (st_rec_rows), the
// frames of a span (st_span_frames) and the row of a frame (st_frame_row).  Rows per recording or per span is a template
// parameter of the kernels (SPANS); spans or pieces is rows.rec_span_off at run time.
//
// Where a tile lives: the tiles of recording r take slots slot0(r) + k, slot0(r) = floor(rec_frame0[r] / ST_TILE) + r.  That
// is strictly increasing in (r, k) for increasing rec_frame0, needs no table of its own and at most
// total / ST_TILE + n_rec + 1 slots; a workgroup finds its recording by bisection over rec_frame0, an empty slot returns.
// Every table entry is validated before it is used as an index (st_rec): no table content can address outside
// win_strong[0 .. rec_win0[n_rec]) or timeline[0 .. rec_frame0[n_rec]).  Integer results only depend on the inputs: no
// float atomics, the only atomic is the OR into the error word.
#include "common.h"
#include "kernels.h"
#include "post.h"

#define ST_TILE 512          // timeline frames per workgroup
#define ST_HALO 32           // 63 / 2 + 1: the widest median window's reach plus the neighbour the edge predicates read
#define ST_THREADS 256
#define ST_EXT (ST_TILE + 2 * ST_HALO)
#define ST_FLT (ST_TILE + 2)  // filtered decisions of frames s - 1 .. e
#define ST_MAXC 16

__device__ __forceinline__ float st_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float st_add(float a, float b) { return a + b; }
__device__ __forceinline__ float st_div(float a, float b) { return a / b; }      // correctly rounded (the compiler's default for HIP)

// What every entry's kernels share: the tables, the window geometry and the tile slots (st_rec, st_slot_rec, st_tile, st_blend).
// Every entry's argument struct is this (checked and filled by st_front) plus its own fields.
struct StTables {
    const int32_t* rec_win0;
    const int64_t* rec_frame0;
    int32_t* err;
    int n_rec, T3, NC, hop3, weighting, n_slots;
};

struct StArgs {              // sed_stitch_decode, sed_stitch_sweep
    StTables t;
    const float *win_strong, *thr;
    const int32_t* win;
    float* timeline;
    uint8_t* binary;
    int64_t* ev_ptr;
    int32_t* ev_pairs;
    long long capacity;
    int64_t* col_total;      // ws: [K * n_rec * NC]
    int32_t* cnt;            // ws: [K][n_slots][NC] onsets per (point, tile, class); after the scan, the onsets in front of the tile
    int K;                   // operating points: 1 for sed_stitch_decode; thr / win are [K][NC], cnt is [K][n_slots][NC]
};

// The tile slots that tables of total_frames frames in n_rec recordings can occupy (the head of the file: where a tile lives).
__host__ __device__ inline long long st_slot_count(long long total_frames, int n_rec) { return total_frames / ST_TILE + n_rec + 1; }

struct StRec {
    long long f0;            // first timeline frame of the recording
    int L3, w0, nw;          // its frames, first window, windows
    int slot0, tiles;
    int bad;                 // 0, or the err bits that keep the recording from being decoded
};

__device__ __forceinline__ StRec st_rec(const StTables& a, int r) {
    StRec R;
    const long long f0 = a.rec_frame0[r], f1 = a.rec_frame0[r + 1], ft = a.rec_frame0[a.n_rec];
    const long long w0 = a.rec_win0[r], w1 = a.rec_win0[r + 1], wt = a.rec_win0[a.n_rec];
    R.bad = 0;
    if (f0 < 0 || f1 <= f0 || f1 > ft || f1 - f0 > 0x7fffffffll - ST_EXT || w0 < 0 || w1 < w0 || w1 > wt) R.bad = 16;
    R.f0 = f0;
    R.L3 = R.bad ? 0 : (int)(f1 - f0);
    R.w0 = (int)w0;
    R.nw = R.bad ? 0 : (int)(w1 - w0);
    const long long slot0 = f0 / ST_TILE + r;
    R.tiles = (R.L3 + ST_TILE - 1) / ST_TILE;
    if (!R.bad && slot0 + R.tiles > a.n_slots) { R.bad = 16; R.tiles = 0; }       // the workspace was sized for other tables
    R.slot0 = R.bad ? 0 : (int)slot0;
    // hop3 <= T3: the windows' ranges are contiguous, so the recording is covered iff the last window reaches its end
    if (!R.bad && !(R.nw >= 1 && (long long)(R.nw - 1) * a.hop3 + a.T3 >= R.L3)) R.bad = 32;
    return R;
}

// The recording whose tiles may hold slot g: the last r with slot0(r) <= g (workgroup-uniform; the caller validates it).
__device__ __forceinline__ int st_slot_rec(const StTables& a, long long g) {
    int lo_r = 0, hi_r = a.n_rec - 1;
    while (lo_r < hi_r) {
        const int mid = (lo_r + hi_r + 1) >> 1;
        if (a.rec_frame0[mid] / ST_TILE + mid <= g) lo_r = mid;
        else hi_r = mid - 1;
    }
    return lo_r;
}

// Slot g is a tile of recording r, the frames [s, e) of its timeline (s = 0: its first) - or nothing to do (false): an empty slot,
// or a recording the tables do not describe or cover (the entry's column / clear kernel reports that one).  Workgroup-uniform.
struct StTile { StRec R; int r, s, e; };
__device__ __forceinline__ bool st_tile(const StTables& a, long long g, StTile& T) {
    T.r = st_slot_rec(a, g);
    T.R = st_rec(a, T.r);
    const long long kt = g - T.R.slot0;
    if (T.R.bad || kt < 0 || kt >= T.R.tiles) return false;
    T.s = (int)kt * ST_TILE;
    T.e = min(T.s + ST_TILE, T.R.L3);
    return true;
}

// The windows st_cover_lo .. st_cover_hi cover timeline frame u of recording R: the j with 0 <= u - j hop3 < T3 that it owns;
// window j holds the frame at v = u - j hop3 with the integer weight st_weight(v).  For the blend and for its transpose.
__device__ __forceinline__ int st_cover_lo(const StTables& a, int u) { return u >= a.T3 ? (u - a.T3) / a.hop3 + 1 : 0; }
__device__ __forceinline__ int st_cover_hi(const StTables& a, const StRec& R, int u) { return min(u / a.hop3, R.nw - 1); }
__device__ __forceinline__ int st_weight(const StTables& a, int v) { return a.weighting ? min(v + 1, a.T3 - v) : 1; }

// Blended value(s) of timeline frame u of recording R from the window tensor `win` [n_win][T3][NC] (the posteriors, or the
// attention of sed_stitch_weak): class q (VEC = false) or classes 4q .. 4q + 3 (VEC = true).
template <bool VEC>
__device__ __forceinline__ f32x4 st_blend(const StTables& a, const float* win, const StRec& R, int u, int q) {
    const int T3 = a.T3, hop3 = a.hop3, NC = a.NC;
    const int j_lo = st_cover_lo(a, u), j_hi = st_cover_hi(a, R, u);
    const int col = VEC ? 4 * q : q;
    const float* src = win + ((size_t)(R.w0 + j_lo) * T3 + (u - j_lo * hop3)) * NC + col;
    f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j_lo == j_hi) {                                                          // one window: its value, copied exactly
        if (VEC) p = *(const f32x4*)src;
        else p[0] = *src;
        return p;
    }
    const ptrdiff_t step = (ptrdiff_t)(T3 - hop3) * NC;                          // window j + 1, local frame v - hop3
    int wsum = 0;
    for (int j = j_lo; j <= j_hi; ++j, src += step) {
        const int v = u - j * hop3;
        const int wi = st_weight(a, v);
        const float w = (float)wi;
        wsum += wi;
        if (VEC) {
            const f32x4 x = *(const f32x4*)src;
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = st_add(p[k], st_mul(w, x[k]));
        } else {
            p[0] = st_add(p[0], st_mul(w, *src));
        }
    }
    const float ws = (float)wsum;                                                // an integer below 2^24: exact
#pragma unroll
    for (int k = 0; k < (VEC ? 4 : 1); ++k) p[k] = st_div(p[k], ws);
    return p;
}

// ---- K operating points from one blend --------------------------------------------------------------------------------------
// The blend does not depend on the threshold or the median window, so sed_stitch_sweep's workgroup (SWEEP = true) blends its
// tile's ST_EXT frames ONCE into LDS (fp32, all classes) and takes the decisions, filters and counts of ST_SWEEP_GROUP points
// from it, one point after the other through the same raw / flt arrays.  The grid's second dimension is the point group:
// blockIdx.y owns the points y * ST_SWEEP_GROUP .. and blends again.  cnt is [K][n_slots][NC] and a column is (point,
// recording, class).  sed_stitch_decode is the SWEEP = false instantiation: one point, no fp32 array, the decisions are
// written straight from the blend.
#ifndef ST_SWEEP_GROUP
#define ST_SWEEP_GROUP 8
#endif
#define ST_SWEEP_MAXK 4096

template <bool SWEEP> struct StBlendLds { float v[ST_MAXC * ST_EXT]; };
template <> struct StBlendLds<false> {};

template <bool VEC, int PASS, bool SWEEP>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_tile(StArgs a) {
    __shared__ StBlendLds<SWEEP> pst;
    __shared__ uint8_t raw[ST_MAXC * ST_EXT];
    __shared__ uint8_t flt[ST_MAXC * ST_FLT];
    __shared__ float s_thr[ST_MAXC];
    __shared__ int s_win[ST_MAXC];       // 0: outside 1 .. 63, the column is not decoded
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NC = a.t.NC;
    const long long g = blockIdx.x;
    StTile T;
    if (!st_tile(a.t, g, T)) return;
    const StRec& R = T.R;
    const int r = T.r, L3 = R.L3, s = T.s, e = T.e;
    const int ext_lo = max(s - ST_HALO, 0), ext_n = min(e + ST_HALO, L3) - ext_lo;
    const int k_lo = SWEEP ? blockIdx.y * ST_SWEEP_GROUP : 0, k_hi = SWEEP ? min(k_lo + ST_SWEEP_GROUP, a.K) : 1;
    auto load_point = [&](int kp) {                                              // threshold and window of point kp, per class
        if (tid < NC) {
            const int w = a.win[kp * NC + tid];
            s_thr[tid] = a.thr[kp * NC + tid];
            s_win[tid] = (w >= 1 && w <= 63) ? w : 0;
            if (PASS == 0 && s == 0 && !(w >= 1 && w <= 63)) atomicOr(a.t.err, 8);
        }
        __syncthreads();
    };
    if constexpr (!SWEEP) load_point(0);
    // ---- the blend, once: frames ext_lo .. ext_lo + ext_n - 1, all classes; the decode's decisions straight from it --------
    {
        const int G = VEC ? NC >> 2 : NC;
        float* tl = (PASS == 0 && a.timeline && (!SWEEP || blockIdx.y == 0)) ? a.timeline + (size_t)R.f0 * NC : nullptr;
        auto keep = [&](int c, int fl, float p) {
            if constexpr (SWEEP) pst.v[c * ST_EXT + fl] = p;
            else raw[c * ST_EXT + fl] = pp_decision(p, s_thr[c]);
        };
        for (int it = tid; it < ext_n * G; it += ST_THREADS) {
            const int fl = it / G, q = it - fl * G, u = ext_lo + fl;
            const f32x4 p = st_blend<VEC>(a.t, a.win_strong, R, u, q);
            if (VEC) {
#pragma unroll
                for (int k = 0; k < 4; ++k) keep(4 * q + k, fl, p[k]);
                if (tl && u >= s && u < e) *(f32x4*)(tl + (size_t)u * NC + 4 * q) = p;
            } else {
                keep(q, fl, p[0]);
                if (tl && u >= s && u < e) tl[(size_t)u * NC + q] = p[0];
            }
        }
    }
    const int n_flt = e - s + 2;
    for (int kp = k_lo; kp < k_hi; ++kp) {
        if constexpr (SWEEP) {
            load_point(kp);                                                      // (the first barrier also publishes pst)
            for (int it = tid; it < NC * ext_n; it += ST_THREADS) {
                const int c = it / ext_n, fl = it - c * ext_n;
                raw[c * ST_EXT + fl] = pp_decision(pst.v[c * ST_EXT + fl], s_thr[c]);
            }
        }
        __syncthreads();
        // ---- median filter of frames s - 1 .. e (post.h's rule; reflection only at the recording's two ends) ----------------
        for (int it = tid; it < NC * n_flt; it += ST_THREADS) {
            const int c = it / n_flt, k = it - c * n_flt, t = s - 1 + k;
            const int window = s_win[c];
            uint8_t v = 0;
            if (t >= 0 && t < L3 && window) {
                const int lo = window / 2, need = window - window / 2;
                const uint8_t* col = raw + c * ST_EXT - ext_lo;
                int ones = 0;
                for (int d = 0; d < window; ++d) ones += col[pp_reflect(t - lo + d, L3)];
                v = ones >= need ? 1 : 0;
            }
            flt[c * ST_FLT + k] = v;
        }
        __syncthreads();
        if (!SWEEP && PASS == 0 && a.binary) {                                   // (the sweep has none: it would be K timelines)
            uint8_t* bin = a.binary + (size_t)R.f0 * NC;
            for (int it = tid; it < (e - s) * NC; it += ST_THREADS) {
                const int fl = it / NC, c = it - fl * NC;
                if (s_win[c]) bin[(size_t)(s + fl) * NC + c] = flt[c * ST_FLT + fl + 1];
            }
        }
        // ---- onsets / offsets of the tile: one wave per class, 64 frames per ballot -----------------------------------------
        const size_t slot = ((size_t)kp * a.t.n_slots + (size_t)g) * NC;
        for (int c = wave; c < NC; c += ST_THREADS / 64) {
            const uint8_t* f = flt + c * ST_FLT + 1;                             // f[t - s], t = s - 1 .. e
            const long long col = ((long long)kp * a.t.n_rec + r) * NC + c;
            int n_on = 0, n_off = 0;
            long long base = 0;
            if (PASS == 1) {
                n_on = a.cnt[slot + c];
                n_off = n_on - ((f[-1] && f[0]) ? 1 : 0);                        // an event open across the tile's first edge
                base = a.ev_ptr[col];
            }
            const int first = n_on;
            for (int t0 = s; t0 < e; t0 += 64) {
                const int t = t0 + lane;
                const bool act = t < e && f[t - s];
                const bool prev = act && f[t - s - 1];
                const bool next = act && f[t - s + 1];
                pp_emit_chunk(act, prev, next, t, lane, n_on, n_off, [&](int k, int frame, bool is_offset) {
                    if (PASS == 1) {
                        const long long dst = base + k;
                        if (dst >= 0 && dst < a.capacity) a.ev_pairs[2 * dst + (is_offset ? 1 : 0)] = frame;
                    }
                });
            }
            if (PASS == 0 && lane == 0) a.cnt[slot + c] = n_on - first;
        }
        // (the next point's s_thr / raw / flt writes are each behind a barrier that every wave reaches after its reads here)
    }
}

// One wave per column (point, recording, class): the tile counts become the onsets in front of each tile; the total goes to
// col_total.
__global__ __launch_bounds__(ST_THREADS) void k_stitch_scan_cols(StArgs a) {
    const int lane = threadIdx.x & 63, NC = a.t.NC;
    const long long col = (long long)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
    const long long per_point = (long long)a.t.n_rec * NC;
    if (col >= per_point * a.K) return;
    const int kp = (int)(col / per_point);
    const long long rc = col - kp * per_point;
    const int r = (int)(rc / NC), c = (int)(rc - (long long)r * NC);
    const StRec R = st_rec(a.t, r);
    const int w = a.win[kp * NC + c];
    if (R.bad && c == 0 && lane == 0) atomicOr(a.t.err, R.bad);
    long long carry = 0;
    if (!R.bad && w >= 1 && w <= 63) {
        int32_t* cnt = a.cnt + (size_t)kp * a.t.n_slots * NC;
        for (int k0 = 0; k0 < R.tiles; k0 += 64) {
            const int k = k0 + lane;
            int32_t* p = cnt + ((size_t)R.slot0 + k) * NC + c;
            const int v = k < R.tiles ? *p : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int n = __shfl_up(incl, o);
                if (lane >= o) incl += n;
            }
            if (k < R.tiles) *p = (int)carry + incl - v;
            carry += __shfl(incl, 63);
        }
    }
    if (lane == 0) a.col_total[col] = carry;
}

// ev_ptr = exclusive scan of the column totals (one workgroup; integer sums in a fixed order).
__global__ __launch_bounds__(1024) void k_stitch_scan_ptr(StArgs a) {
    __shared__ long long part[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = (long long)a.t.n_rec * a.t.NC * a.K;
    if (tid == 0) { s_carry = 0; a.ev_ptr[0] = 0; }
    __syncthreads();
    for (long long i0 = 0; i0 < n; i0 += 1024) {
        const long long i = i0 + tid;
        const long long v = i < n ? a.col_total[i] : 0;
        long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long m = __shfl_up(incl, o);
            if (lane >= o) incl += m;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        long long before = s_carry;
        for (int k = 0; k < wave; ++k) before += part[k];
        if (i < n) a.ev_ptr[i + 1] = before + incl;
        __syncthreads();
        if (tid == 1023) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0 && s_carry > a.capacity) atomicOr(a.t.err, 2);
}

extern "C" int sed_stitch_tile_frames(void) { return ST_TILE; }

// The workspace: col_total [K * n_rec * NC] int64, then cnt [K][n_slots][NC] int32 (K = 1: sed_stitch_decode's layout).
static size_t st_ws_head(int n_rec, int NC, int K) { return (size_t)K * n_rec * NC * sizeof(int64_t); }
static size_t st_ws_per_slot(int NC, int K) { return (size_t)K * NC * sizeof(int32_t); }

// Slots for tables of total_frames frames, or 0 where the sizes are out of range (the sweep's ranges are the narrower ones).
static size_t st_ws_slot_count(long long total_frames, int n_rec, int NC, int K, bool sweep) {
    if (total_frames < 1 || n_rec < 1 || NC < 1 || NC > ST_MAXC || K < 1 || K > ST_SWEEP_MAXK || total_frames * NC >= (1ll << 31) ||
        (long long)K * n_rec * NC >= (1ll << (sweep ? 26 : 31))) return 0;
    const long long n_slots = st_slot_count(total_frames, n_rec);
    return sweep && n_slots * K >= (1ll << 31) ? 0 : (size_t)n_slots;
}

extern "C" size_t sed_stitch_decode_ws_bytes(long long total_frames, int n_rec, int nclass) {
    const size_t n = st_ws_slot_count(total_frames, n_rec, nclass, 1, false);
    if (!n) sed_set_error("sed_stitch_decode_ws_bytes: need total_frames >= 1, n_rec >= 1, 1 <= nclass <= 16, "
                          "total_frames * nclass < 2^31");
    return n ? st_ws_head(n_rec, nclass, 1) + n * st_ws_per_slot(nclass, 1) : 0;
}

extern "C" size_t sed_stitch_sweep_ws_bytes(long long total_frames, int n_rec, int nclass, int n_points) {
    const size_t n = st_ws_slot_count(total_frames, n_rec, nclass, n_points, true);
    if (!n) sed_set_error("sed_stitch_sweep_ws_bytes: need total_frames >= 1, n_rec >= 1, 1 <= nclass <= 16, 1 <= n_points <= %d, "
                          "total_frames * nclass < 2^31, n_points * n_rec * nclass < 2^26, n_points * slots < 2^31", ST_SWEEP_MAXK);
    return n ? st_ws_head(n_rec, nclass, n_points) + n * st_ws_per_slot(nclass, n_points) : 0;
}

extern "C" int sed_stitch_sweep_point_group(void) { return ST_SWEEP_GROUP; }

template <int PASS>
static void st_launch_tile(bool vec, bool sweep, dim3 grid, hipStream_t st, const StArgs& a) {
    const dim3 thr256(ST_THREADS);
    if (sweep && vec) hipLaunchKernelGGL((k_stitch_tile<true, PASS, true>), grid, thr256, 0, st, a);
    else if (sweep) hipLaunchKernelGGL((k_stitch_tile<false, PASS, true>), grid, thr256, 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_stitch_tile<true, PASS, false>), grid, thr256, 0, st, a);
    else hipLaunchKernelGGL((k_stitch_tile<false, PASS, false>), grid, thr256, 0, st, a);
}

#define ST_NEED(cond, msg)                          \
    do {                                            \
        if (!(cond)) {                              \
            sed_set_error("%s: %s", what, msg);     \
            return SED_ERR_BAD_ARG;                 \
        }                                           \
    } while (0)

// The host front of all four entries (`what` names the entry in every message): the geometry checks - n_points * n_rec * NC
// columns, n_points = 1 but for the sweep, stay below 2^col_bits - and the tables struct, still without its slot count.
static int st_front(const char* what, const int32_t* rec_win0, const int64_t* rec_frame0, int32_t* err, int n_rec, int T3, int NC,
                    int hop3, int weighting, int n_points, int col_bits, StTables* t) {
    ST_NEED(n_rec >= 1 && NC >= 1 && NC <= ST_MAXC && (long long)n_points * n_rec * NC < (1ll << col_bits),
            col_bits == 26 ? "need n_rec >= 1, 1 <= NC <= 16 and n_points * n_rec * NC < 2^26"
                           : "need n_rec >= 1, 1 <= NC <= 16 and n_rec * NC < 2^31");
    ST_NEED(T3 >= 1 && T3 <= 4096, "need 1 <= T3 <= 4096 (the taper's weight sum stays exact in fp32)");
    ST_NEED(hop3 >= 1 && hop3 <= T3, "need 1 <= hop3 <= T3");
    ST_NEED(weighting == 0 || weighting == 1, "weighting is 0 (uniform) or 1 (taper)");
    *t = StTables{rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, 0};
    return SED_OK;
}

// t->n_slots from the workspace's size: `bytes` of it hold the slots of K points, per_slot each.  whole: only a size the entry's
// _ws_bytes function returns describes whole slots for the tables (the sweep's layout, sed_stitch_weak); sed_stitch_decode
// takes any size that holds the tables.  The slots bound the tile grid and the frames the tables may hold.
static int st_ws_slots(const char* what, size_t bytes, size_t per_slot, bool whole, int K, StTables* t) {
    const size_t n_slots = bytes / per_slot;
    if (whole && (bytes % per_slot != 0 || n_slots < (size_t)st_slot_count(1, t->n_rec))) {
        sed_set_error("%s: ws_bytes must be the value %s_ws_bytes returned for these tables", what, what);
        return SED_ERR_BAD_ARG;
    }
    ST_NEED(n_slots * K < (1ull << 31), "workspace too large for the tile grid (slots, times n_points in a sweep, < 2^31)");
    ST_NEED((long long)(n_slots - t->n_rec - 1) * ST_TILE * t->NC < (1ll << 31) + (long long)ST_TILE * t->NC,
            "sum L3 * NC must stay below 2^31");
    t->n_slots = (int)n_slots;
    return SED_OK;
}

// sed_stitch_decode and sed_stitch_sweep: sweep = false is n_points = 1 with the looser workspace rule and the binary output.
static int st_run(const char* what, bool sweep, const float* win_strong, const int32_t* rec_win0, const int64_t* rec_frame0,
                  int n_rec, int T3, int NC, int hop3, int weighting, int n_points, const float* thr, const int32_t* win,
                  float* timeline, uint8_t* binary, int64_t* ev_ptr, int32_t* ev_pairs, long long capacity, void* ws,
                  size_t ws_bytes, int32_t* err, void* stream) {
    ST_NEED(win_strong && rec_win0 && rec_frame0 && thr && win && ev_ptr && ev_pairs && ws && err, "null argument");
    ST_NEED(n_points >= 1 && n_points <= ST_SWEEP_MAXK, "need 1 <= n_points <= 4096");
    StTables t;
    SED_TRY(st_front(what, rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, n_points, sweep ? 26 : 31, &t));
    ST_NEED(capacity >= 0, "capacity must be >= 0");
    ST_NEED(((uintptr_t)ws % 8) == 0, "ws must be 8-byte aligned");
    const size_t head = st_ws_head(n_rec, NC, n_points), per_slot = st_ws_per_slot(NC, n_points);
    if (ws_bytes < head + (size_t)st_slot_count(1, n_rec) * per_slot) {                  // the fewest slots any tables take
        sed_set_error("%s: workspace of %zu bytes is too small (%s_ws_bytes)", what, ws_bytes, what);
        return SED_ERR_WORKSPACE;
    }
    SED_TRY(st_ws_slots(what, ws_bytes - head, per_slot, sweep, n_points, &t));
    const StArgs a = {t, win_strong, thr, win, timeline, binary, ev_ptr, ev_pairs, capacity, (int64_t*)ws,
                      (int32_t*)((char*)ws + head), n_points};
    const bool vec = NC % 4 == 0 && ((uintptr_t)win_strong % 16) == 0 && (!timeline || ((uintptr_t)timeline % 16) == 0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles((unsigned)t.n_slots, sweep ? (unsigned)((n_points + ST_SWEEP_GROUP - 1) / ST_SWEEP_GROUP) : 1u);
    st_launch_tile<0>(vec, sweep, tiles, st, a);
    SED_CHECK_LAUNCH();
    const long long n_cols = (long long)n_points * n_rec * NC;
    hipLaunchKernelGGL(k_stitch_scan_cols, dim3((unsigned)((n_cols + 3) / 4)), dim3(ST_THREADS), 0, st, a);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stitch_scan_ptr, dim3(1), dim3(1024), 0, st, a);
    SED_CHECK_LAUNCH();
    st_launch_tile<1>(vec, sweep, tiles, st, a);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_stitch_decode(const float* win_strong, const int32_t* rec_win0, const int64_t* rec_frame0, int n_rec, int T3,
                                 int NC, int hop3, int weighting, const float* thr, const int32_t* win, float* timeline,
                                 uint8_t* binary, int64_t* ev_ptr, int32_t* ev_pairs, long long capacity, void* ws,
                                 size_t ws_bytes, int32_t* err, void* stream) {
    return st_run("sed_stitch_decode", false, win_strong, rec_win0, rec_frame0, n_rec, T3, NC, hop3, weighting, 1, thr, win,
                  timeline, binary, ev_ptr, ev_pairs, capacity, ws, ws_bytes, err, stream);
}

extern "C" int sed_stitch_sweep(const float* win_strong, const int32_t* rec_win0, const int64_t* rec_frame0, int n_rec, int T3,
                                int NC, int hop3, int weighting, int n_points, const float* thr, const int32_t* win,
                                float* timeline, int64_t* ev_ptr, int32_t* ev_pairs, long long capacity, void* ws,
                                size_t ws_bytes, int32_t* err, void* stream) {
    return st_run("sed_stitch_sweep", true, win_strong, rec_win0, rec_frame0, n_rec, T3, NC, hop3, weighting, n_points, thr, win,
                  timeline, nullptr, ev_ptr, ev_pairs, capacity, ws, ws_bytes, err, stream);
}

// ---- recording-level weak tags (sed_stitch_weak) ------------------------------------------------------------------------------
// weak[r, c] = (sum_u P[u, c] A[u, c]) / (sum_u A[u, c]) over the WHOLE timeline of recording r: P the blend of the windows'
// posteriors, A the same blend of their attention, the products and both sums in fp64 (include/dcase_sed.h).  No timeline is
// written: a tile's workgroup blends both tensors for its ST_TILE frames (st_blend, no halo) and leaves one (num, den) pair per
// class in its slot of the workspace; a second launch adds a column's tile pairs.
// The order of every sum is a function of (L3, NC) alone:
//   an item is one frame x W classes, W = 4 when NC % 4 == 0, else 1 (VEC only decides whether the four come in one 16-byte
//     load, so alignment does not change the result); thread (row, q) of the first rows * G threads, G = NC / W,
//     rows = ST_THREADS / G, adds the items of class group q at frames s + row, s + row + rows, ... in that order;
//   thread (c, i) adds the rows i, i + 16, ... of class c, thread c the sixteen of those: the tile's pair;
//   lane l of a column's wave adds the tiles l, l + 64, ..., then an xor butterfly (both partners form the same sum).
#define SW_FOLD 16

// Which row of tags / sums / g a timeline frame of recording r belongs to: the one description of all three levels.
//   rec_span0 null: one row per recording, row r (sed_stitch_weak); the other fields are not used.
//   rec_span0 set, rec_span_off null: recording r owns the n_r = rec_span0[r + 1] - rec_span0[r] rows from rec_span0[r] on, row k
//     the SPAN of local frames [k * span3, min((k + 1) * span3, L3_r)), and the spans tile the recording: n_r = ceil(L3_r / span3)
//     (sed_stitch_span_tags).
//   rec_span_off set: the tables describe PIECES.  Piece r owns the windows and local frames 0 .. L3_r of its table rows like a
//     recording, its span k covers [off_r + k * span3, min(off_r + (k + 1) * span3, L3_r)), off_r = rec_span_off[r] >= 0, and n_r >= 1
//     need not be the ceiling, only off_r + (n_r - 1) * span3 < L3_r (the last span holds a frame): the frames below off_r and
//     from off_r + n_r * span3 on belong to no span (sed_stitch_piece_span_tags).
// In the forward a span's tile is ST_TILE frames counted from the span's first frame, its slot is span * tps + k
// (tps = ceil(span3 / ST_TILE)), and the order of a span's sums is the order above with L3 = the span's length.
struct StRows {
    const int64_t* rec_span0;            // [n_rec + 1] or null
    const int32_t* rec_span_off;         // [n_rec] or null
    long long total_spans;
    int span3, tps;
};
struct StPoolArgs {          // sed_stitch_weak, sed_stitch_span_tags, sed_stitch_piece_span_tags
    StTables t;              // span level: n_slots is not used (no recording-slot layout)
    const float *win_strong, *win_att;
    double* part;            // ws: [n_slots][NC][2] (num, den) of a tile; span level [total_spans * tps][NC][2]
    float* weak;             // [rows][NC], rows = n_rec or total_spans
    double* sums;            // [rows][NC][2] or null
    StRows rows;
};

// The rows of recording r (R = st_rec of it), validated before any is used as an index: 0 and Q - its n rows from row0 on, which
// its local frames [off, end) belong to, span by span -, or the err bits that keep the recording out: R.bad, or 16 for span tables
// that break the level's rule.  `spans` is rows.rec_span0 != null (a compile-time constant in the tile kernels).
struct StRecRows { int row0, n, off, end; };    // (rows are < 2^31: total_spans is)
__device__ __forceinline__ int st_rec_rows(const StRows& w, bool spans, const StRec& R, int r, StRecRows& Q) {
    Q = StRecRows{r, 1, 0, R.L3};
    if (R.bad || !spans) return R.bad;
    const long long p0 = w.rec_span0[r], p1 = w.rec_span0[r + 1];
    // (in this order: 0 <= p0 < p1 <= total_spans < 2^31 first, so the product below stays under 2^62)
    if (p0 < 0 || p1 > w.total_spans || p1 <= p0) return 16;
    const long long off = w.rec_span_off ? w.rec_span_off[r] : 0, last = off + (p1 - p0 - 1) * w.span3, end = last + w.span3;
    if (off < 0 || last >= R.L3) return 16;                                      // the last span holds a frame
    if (!w.rec_span_off && end < R.L3) return 16;                                // ... and reaches the end: n = ceil(L3 / span3)
    Q = StRecRows{(int)p0, (int)(p1 - p0), (int)off, (int)min(end, (long long)R.L3)};
    return 0;
}
// Span k, 0 <= k < Q.n, of a recording st_rec_rows accepted covers its local frames [s, e), s < L3 by either rule.
__device__ __forceinline__ void st_span_frames(const StRows& w, const StRecRows& Q, int k, int& s, int& e) {
    const long long s0 = Q.off + (long long)k * w.span3;
    s = (int)s0;
    e = (int)min(s0 + w.span3, (long long)Q.end);
}
// The row that local frame u of such a recording reads; false: the frame belongs to no span (pieces only).
__device__ __forceinline__ bool st_frame_row(const StRows& w, bool spans, const StRecRows& Q, int u, size_t& row) {
    row = (size_t)Q.row0 + (spans ? (u - Q.off) / w.span3 : 0);
    return !spans || (u >= Q.off && u < Q.end);
}

// Span g of the tables: the recording that holds it (one bisection over rec_span0: the last r with rec_span0[r] <= g), validated
// (st_rec_rows, and g inside its rows), and the span's frames [s, e) of that recording's timeline.  bad: 0, or the err bits that
// make the span's row NaN.  Wave-uniform.
struct StSpan { StRec R; int r, s, e, bad; };
__device__ __forceinline__ StSpan st_span(const StTables& a, const StRows& w, long long g) {
    int lo_r = 0, hi_r = a.n_rec - 1;
    while (lo_r < hi_r) {
        const int mid = (lo_r + hi_r + 1) >> 1;
        if (w.rec_span0[mid] <= g) lo_r = mid;
        else hi_r = mid - 1;
    }
    StSpan S;
    StRecRows Q;
    S.r = lo_r;
    S.R = st_rec(a, lo_r);
    S.s = S.e = 0;
    S.bad = st_rec_rows(w, true, S.R, lo_r, Q);
    if (!S.bad && (g < Q.row0 || g >= Q.row0 + Q.n)) S.bad = 16;
    if (!S.bad) st_span_frames(w, Q, (int)(g - Q.row0), S.s, S.e);
    return S;
}

template <bool VEC, int W, bool SPANS>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_weak_tile(StPoolArgs wa) {
    __shared__ double red[ST_THREADS * W * 2];                                   // [rows][NC][2], rows * NC <= ST_THREADS * W
    __shared__ double fold[ST_MAXC * SW_FOLD * 2];
    const StTables& a = wa.t;
    const int tid = threadIdx.x, NC = a.NC;
    StTile T;
    if constexpr (SPANS) {                                                       // frame 0 of the tile walk is the span's first frame
        const int tps = wa.rows.tps;
        const long long g = blockIdx.x / tps, kt = blockIdx.x - g * tps;
        const StSpan S = st_span(a, wa.rows, g);
        const long long s = (long long)S.s + kt * ST_TILE;
        if (S.bad || s >= S.e) return;
        T.R = S.R;
        T.r = S.r;
        T.s = (int)s;
        T.e = (int)min(s + ST_TILE, (long long)S.e);
    } else {
        if (!st_tile(a, blockIdx.x, T)) return;
    }
    const int G = NC / W, rows = ST_THREADS / G, row = tid / G, q = tid - row * G;
    if (row < rows) {
        double num[W], den[W];
#pragma unroll
        for (int k = 0; k < W; ++k) { num[k] = 0.0; den[k] = 0.0; }
        for (int u = T.s + row; u < T.e; u += rows) {
            f32x4 p, at;
            if (VEC) {
                p = st_blend<true>(a, wa.win_strong, T.R, u, q);
                at = st_blend<true>(a, wa.win_att, T.R, u, q);
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    p[k] = st_blend<false>(a, wa.win_strong, T.R, u, W * q + k)[0];
                    at[k] = st_blend<false>(a, wa.win_att, T.R, u, W * q + k)[0];
                }
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                num[k] += (double)p[k] * (double)at[k];                          // (24 x 24 bits: the product is exact)
                den[k] += (double)at[k];
            }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            red[((size_t)row * NC + W * q + k) * 2] = num[k];
            red[((size_t)row * NC + W * q + k) * 2 + 1] = den[k];
        }
    }
    __syncthreads();
    {
        const int c = tid / SW_FOLD, i = tid - c * SW_FOLD;                      // ST_THREADS = ST_MAXC * SW_FOLD
        if (c < NC) {
            double n = 0.0, d = 0.0;
            for (int rr = i; rr < rows; rr += SW_FOLD) { n += red[(rr * NC + c) * 2]; d += red[(rr * NC + c) * 2 + 1]; }
            fold[(c * SW_FOLD + i) * 2] = n;
            fold[(c * SW_FOLD + i) * 2 + 1] = d;
        }
    }
    __syncthreads();
    if (tid < NC) {
        double n = 0.0, d = 0.0;
        for (int i = 0; i < SW_FOLD; ++i) { n += fold[(tid * SW_FOLD + i) * 2]; d += fold[(tid * SW_FOLD + i) * 2 + 1]; }
        double* out = wa.part + ((size_t)blockIdx.x * NC + tid) * 2;
        out[0] = n;
        out[1] = d;
    }
}
static_assert(ST_THREADS == ST_MAXC * SW_FOLD, "k_stitch_weak_tile folds the rows with one thread per (class, fold lane)");

// One wave per column (recording, class) - or per row (span, class) of the span tags: the tile pairs in the fixed order above; a
// recording the tables do not describe or cover raises its err bits and has NaN rows, and so has a span that no valid
// recording holds.  In a span call wave r < n_rec moreover validates recording r (a recording whose spans own no row).
template <bool SPANS>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_weak_cols(StPoolArgs wa) {
    const StTables& a = wa.t;
    const int lane = threadIdx.x & 63;
    const long long col = (long long)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
    long long n_rows = a.n_rec, slot0 = 0;
    int bad = 0, tiles = 0;
    if constexpr (SPANS) {
        n_rows = wa.rows.total_spans;
        if (col < a.n_rec && lane == 0) {
            StRecRows Q;
            const int rec_bad = st_rec_rows(wa.rows, true, st_rec(a, (int)col), (int)col, Q);
            if (rec_bad) atomicOr(a.err, rec_bad);
        }
    }
    if (col >= n_rows * a.NC) return;
    const long long r = col / a.NC;
    const int c = (int)(col - r * a.NC);
    if constexpr (SPANS) {
        const StSpan S = st_span(a, wa.rows, r);
        bad = S.bad;
        tiles = (S.e - S.s + ST_TILE - 1) / ST_TILE;
        slot0 = r * wa.rows.tps;
    } else {
        const StRec R = st_rec(a, (int)r);
        bad = R.bad;
        tiles = R.tiles;
        slot0 = R.slot0;
    }
    double n = 0.0, d = 0.0;
    if (bad) {
        if (c == 0 && lane == 0) atomicOr(a.err, bad);
        n = d = __builtin_nan("");
    } else {
        for (int k = lane; k < tiles; k += 64) {
            const double* p = wa.part + (((size_t)slot0 + k) * a.NC + c) * 2;
            n += p[0];
            d += p[1];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            n += __shfl_xor(n, o);
            d += __shfl_xor(d, o);
        }
    }
    if (lane == 0) {
        wa.weak[col] = bad ? __builtin_nanf("") : (float)(n / d);
        if (wa.sums) { wa.sums[2 * col] = n; wa.sums[2 * col + 1] = d; }
    }
}

static size_t sw_ws_per_slot(int NC) { return (size_t)NC * 2 * sizeof(double); }

// The two launches of the three forward entries: n_tiles workgroups of the tile pass, one wave per column of the column pass.
template <bool SPANS>
static int sw_launch(const StPoolArgs& wa, unsigned n_tiles, long long n_waves, void* stream) {
    const int NC = wa.t.NC;
    const bool vec = NC % 4 == 0 && ((uintptr_t)wa.win_strong % 16) == 0 && ((uintptr_t)wa.win_att % 16) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(n_tiles), thr256(ST_THREADS);
    if (vec) hipLaunchKernelGGL((k_stitch_weak_tile<true, 4, SPANS>), tiles, thr256, 0, st, wa);
    else if (NC % 4 == 0) hipLaunchKernelGGL((k_stitch_weak_tile<false, 4, SPANS>), tiles, thr256, 0, st, wa);
    else hipLaunchKernelGGL((k_stitch_weak_tile<false, 1, SPANS>), tiles, thr256, 0, st, wa);
    SED_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stitch_weak_cols<SPANS>, dim3((unsigned)((n_waves + 3) / 4)), thr256, 0, st, wa);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" size_t sed_stitch_weak_ws_bytes(long long total_frames, int n_rec, int nclass) {
    const size_t n = st_ws_slot_count(total_frames, n_rec, nclass, 1, false);
    if (!n) sed_set_error("sed_stitch_weak_ws_bytes: need total_frames >= 1, n_rec >= 1, 1 <= nclass <= 16, "
                          "total_frames * nclass < 2^31, n_rec * nclass < 2^31");
    return n * sw_ws_per_slot(nclass);
}

extern "C" int sed_stitch_weak(const float* win_strong, const float* win_att, const int32_t* rec_win0, const int64_t* rec_frame0,
                               int n_rec, int T3, int NC, int hop3, int weighting, float* weak, double* sums, void* ws,
                               size_t ws_bytes, int32_t* err, void* stream) {
    const char* what = "sed_stitch_weak";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && weak && ws && err, "null argument");
    StTables t;
    SED_TRY(st_front(what, rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, 1, 31, &t));
    ST_NEED(((uintptr_t)ws % 8) == 0, "ws must be 8-byte aligned");
    SED_TRY(st_ws_slots(what, ws_bytes, sw_ws_per_slot(NC), true, 1, &t));
    const StPoolArgs wa = {t, win_strong, win_att, (double*)ws, weak, sums, StRows{}};
    return sw_launch<false>(wa, (unsigned)t.n_slots, (long long)n_rec * NC, stream);
}

// ---- span-level weak tags (sed_stitch_span_tags) ------------------------------------------------------------------------------
// The slots of a call: tps = ceil(span3 / ST_TILE) per span, or 0 where a size is out of range.
static long long sp_tps(int span3) { return ((long long)span3 + ST_TILE - 1) / ST_TILE; }
static size_t sp_slot_count(long long total_frames, long long total_spans, int n_rec, int NC, int span3) {
    if (total_frames < 1 || n_rec < 1 || NC < 1 || NC > ST_MAXC || span3 < 1 || total_spans < n_rec || total_spans > total_frames ||
        total_frames * NC >= (1ll << 31) || total_spans * NC >= (1ll << 31) || total_spans * sp_tps(span3) >= (1ll << 31)) return 0;
    return (size_t)(total_spans * sp_tps(span3));
}

static size_t sp_ws_bytes(const char* what, long long total_frames, long long total_spans, int n_rec, int nclass, int span3) {
    const size_t n = sp_slot_count(total_frames, total_spans, n_rec, nclass, span3);
    if (!n) sed_set_error("%s: need span3 >= 1, 1 <= n_rec <= total_spans <= total_frames, "
                          "1 <= nclass <= 16, total_frames * nclass < 2^31, total_spans * ceil(span3 / %d) < 2^31", what, ST_TILE);
    return n * sw_ws_per_slot(nclass);
}

extern "C" size_t sed_stitch_span_tags_ws_bytes(long long total_frames, long long total_spans, int n_rec, int nclass, int span3) {
    return sp_ws_bytes("sed_stitch_span_tags_ws_bytes", total_frames, total_spans, n_rec, nclass, span3);
}

// The host side of sed_stitch_span_tags (rec_span_off null) and of sed_stitch_piece_span_tags.
static int sp_run(const char* what, const float* win_strong, const float* win_att, const int32_t* rec_win0, const int64_t* rec_frame0,
                  const int64_t* rec_span0, const int32_t* rec_span_off, long long total_frames, long long total_spans, int n_rec,
                  int T3, int NC, int hop3, int weighting, int span3, float* tags, double* sums, void* ws, size_t ws_bytes,
                  int32_t* err, void* stream) {
    StTables t;
    SED_TRY(st_front(what, rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, 1, 31, &t));
    ST_NEED(((uintptr_t)ws % 8) == 0, "ws must be 8-byte aligned");
    const size_t n_slots = sp_slot_count(total_frames, total_spans, n_rec, NC, span3);
    ST_NEED(n_slots, "need span3 >= 1, n_rec <= total_spans <= total_frames, total_frames * NC < 2^31 and "
                     "total_spans * ceil(span3 / tile) < 2^31");
    if (ws_bytes != n_slots * sw_ws_per_slot(NC)) {
        sed_set_error("%s: ws_bytes must be the value %s_ws_bytes returned for these sizes", what, what);
        return SED_ERR_BAD_ARG;
    }
    t.n_slots = 0x7fffffff;                                                      // (st_rec's slot check is the recording layout's)
    const StPoolArgs wa = {t, win_strong, win_att, (double*)ws, tags, sums,
                           StRows{rec_span0, rec_span_off, total_spans, span3, (int)sp_tps(span3)}};
    const long long rows = total_spans * NC;
    return sw_launch<true>(wa, (unsigned)n_slots, rows > n_rec ? rows : n_rec, stream);
}

extern "C" int sed_stitch_span_tags(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                    const int64_t* rec_frame0, const int64_t* rec_span0, long long total_frames,
                                    long long total_spans, int n_rec, int T3, int NC, int hop3, int weighting, int span3,
                                    float* tags, double* sums, void* ws, size_t ws_bytes, int32_t* err, void* stream) {
    const char* what = "sed_stitch_span_tags";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && rec_span0 && tags && ws && err, "null argument");
    return sp_run(what, win_strong, win_att, rec_win0, rec_frame0, rec_span0, nullptr, total_frames, total_spans, n_rec, T3, NC,
                  hop3, weighting, span3, tags, sums, ws, ws_bytes, err, stream);
}

// ---- span tags of pieces (sed_stitch_piece_span_tags) ------------------------------------------------------------------------
extern "C" size_t sed_stitch_piece_span_tags_ws_bytes(long long total_frames, long long total_spans, int n_rec, int nclass,
                                                      int span3) {
    return sp_ws_bytes("sed_stitch_piece_span_tags_ws_bytes", total_frames, total_spans, n_rec, nclass, span3);
}

extern "C" int sed_stitch_piece_span_tags(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                          const int64_t* rec_frame0, const int64_t* rec_span0, long long total_frames,
                                          long long total_spans, int n_rec, int T3, int NC, int hop3, int weighting, int span3,
                                          const int32_t* rec_span_off, float* tags, double* sums, void* ws, size_t ws_bytes,
                                          int32_t* err, void* stream) {
    const char* what = "sed_stitch_piece_span_tags";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && rec_span0 && rec_span_off && tags && ws && err, "null argument");
    return sp_run(what, win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, total_frames, total_spans, n_rec, T3,
                  NC, hop3, weighting, span3, tags, sums, ws, ws_bytes, err, stream);
}

// ---- backward through the pooled tag (sed_stitch_weak_backward) ---------------------------------------------------------------
// The transpose of the blend-and-pool above, for a loss on weak[r, c] = num / den: with g = dLoss/dweak[r, c] and t = num / den,
//   dLoss/dP[u, c] = g A[u, c] / den,   dLoss/dA[u, c] = g (P[u, c] - t) / den,
// and a blended frame hands window j, local frame v = u - j hop3, the share w / W of either (w the window's weight at v, W the
// integer sum over the windows covering u): the formulas and their rounding order are in include/dcase_sed.h.
// A tile's workgroup owns its ST_TILE timeline frames as in k_stitch_weak_tile (no halo): an item is one frame x (1 or 4)
// classes, it blends both tensors once (st_blend) and scatters to its <= ceil(T3 / hop3) covering windows.  A window element
// (j, v, c) belongs to exactly one timeline element u = j hop3 + v, so every element has one writer: no atomics, and the bytes
// do not depend on the tiling or on VEC.  What no timeline frame owns - the tail u >= L3 of a recording's last windows, the
// windows of a rejected recording - is +0.0f from k_stitch_weak_bwd_zero, which runs first on the same stream and clears both
// outputs over [0, rec_win0[n_rec]) (the window count lives on the device; a host-side memset would need it).
// The call has no workspace to derive the slot count from, and the tables are device data: both kernels take it from
// rec_frame0[n_rec] (sb_tables: st_slot_count of it, the smallest count that st_rec accepts every well-formed table with) and
// walk the slots with a grid-stride loop over a fixed grid.
// At the span level the tiles stay the recordings' - a window element's owner is a timeline frame whatever the spans are - and
// only the ROW that a frame takes g, num and den from changes (st_frame_row); a frame of a piece that belongs to no span leaves
// its window elements at the clear pass's +0.0f.
struct StPoolBwdArgs {       // sed_stitch_weak_backward, sed_stitch_span_tags_backward, sed_stitch_piece_span_tags_backward
    StTables t;              // n_slots is filled in on the device (sb_tables)
    const float *win_strong, *win_att;
    const double* sums;      // [rows][NC][2] (num, den) of the forward, rows = n_rec or total_spans
    const float* g_weak;     // [rows][NC]
    float *d_win_strong, *d_win_att;      // [n_win][T3][NC]
    StRows rows;             // (tps is not used)
};
#define SB_GRID 512

// The tables with the tile slots of their own total, or 0 slots (st_rec then rejects every recording) when that total is outside
// the forward's limits.
__device__ __forceinline__ StTables sb_tables(StTables a) {
    const long long ft = a.rec_frame0[a.n_rec];
    a.n_slots = (ft < 1 || ft >= (1ll << 31) || ft * a.NC >= (1ll << 31)) ? 0 : (int)st_slot_count(ft, a.n_rec);
    return a;
}

template <bool VEC>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_weak_bwd_zero(StPoolBwdArgs wa) {
    const StTables a = sb_tables(wa.t);
    const size_t i0 = (size_t)blockIdx.x * ST_THREADS + threadIdx.x, stride = (size_t)gridDim.x * ST_THREADS;
    for (size_t r = i0; r < (size_t)a.n_rec; r += stride) {
        StRecRows Q;
        const int bad = st_rec_rows(wa.rows, wa.rows.rec_span0 != nullptr, st_rec(a, (int)r), (int)r, Q);
        if (bad) atomicOr(a.err, bad);
    }
    const long long wt = a.rec_win0[a.n_rec];
    if (wt <= 0) return;
    const size_t n = (size_t)wt * a.T3 * a.NC;
    if (VEC) {
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        for (size_t i = i0; i < n / 4; i += stride) {
            ((f32x4*)wa.d_win_strong)[i] = z;
            ((f32x4*)wa.d_win_att)[i] = z;
        }
    } else {
        for (size_t i = i0; i < n; i += stride) {
            wa.d_win_strong[i] = 0.0f;
            wa.d_win_att[i] = 0.0f;
        }
    }
}

template <bool VEC, bool SPANS>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_weak_bwd_tile(StPoolBwdArgs wa) {
    const StTables a = sb_tables(wa.t);
    const int tid = threadIdx.x, NC = a.NC, T3 = a.T3, hop3 = a.hop3;
    constexpr int W = VEC ? 4 : 1;
    const int G = VEC ? NC >> 2 : NC;
    for (long long g = blockIdx.x; g < a.n_slots; g += gridDim.x) {
        StTile T;
        if (!st_tile(a, g, T)) continue;
        StRecRows Q;
        if (st_rec_rows(wa.rows, SPANS, T.R, T.r, Q)) continue;
        for (int it = tid; it < (T.e - T.s) * G; it += ST_THREADS) {
            const int fl = it / G, q = it - fl * G, u = T.s + fl, col = W * q;
            size_t row;
            if (!st_frame_row(wa.rows, SPANS, Q, u, row)) continue;
            const f32x4 p = st_blend<VEC>(a, wa.win_strong, T.R, u, q);
            const f32x4 at = st_blend<VEC>(a, wa.win_att, T.R, u, q);
            double dP[W], dA[W];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const size_t rc = row * NC + col + k;
                const double gk = (double)wa.g_weak[rc], num = wa.sums[2 * rc], den = wa.sums[2 * rc + 1];
                const double t = num / den;
                dP[k] = (gk * (double)at[k]) / den;
                dA[k] = (gk * ((double)p[k] - t)) / den;
            }
            const int j_lo = st_cover_lo(a, u), j_hi = st_cover_hi(a, T.R, u);
            int wsum = 0;
            for (int j = j_lo; j <= j_hi; ++j) wsum += st_weight(a, u - j * hop3);
            const double Ws = (double)wsum;
            for (int j = j_lo; j <= j_hi; ++j) {
                const int v = u - j * hop3;
                const double w = (double)st_weight(a, v);
                const size_t o = ((size_t)(T.R.w0 + j) * T3 + v) * NC + col;
                f32x4 ds, da;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    ds[k] = (float)((dP[k] * w) / Ws);
                    da[k] = (float)((dA[k] * w) / Ws);
                }
                if (VEC) {
                    *(f32x4*)(wa.d_win_strong + o) = ds;
                    *(f32x4*)(wa.d_win_att + o) = da;
                } else {
                    wa.d_win_strong[o] = ds[0];
                    wa.d_win_att[o] = da[0];
                }
            }
        }
    }
}

// The two launches of the three backward entries.
template <bool SPANS>
static int sb_launch(const StPoolBwdArgs& wa, void* stream) {
    const bool vec = wa.t.NC % 4 == 0 && ((uintptr_t)wa.win_strong % 16) == 0 && ((uintptr_t)wa.win_att % 16) == 0 &&
                     ((uintptr_t)wa.d_win_strong % 16) == 0 && ((uintptr_t)wa.d_win_att % 16) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(SB_GRID), thr256(ST_THREADS);
    if (vec) hipLaunchKernelGGL(k_stitch_weak_bwd_zero<true>, grid, thr256, 0, st, wa);
    else hipLaunchKernelGGL(k_stitch_weak_bwd_zero<false>, grid, thr256, 0, st, wa);
    SED_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL((k_stitch_weak_bwd_tile<true, SPANS>), grid, thr256, 0, st, wa);
    else hipLaunchKernelGGL((k_stitch_weak_bwd_tile<false, SPANS>), grid, thr256, 0, st, wa);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" int sed_stitch_weak_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                        const int64_t* rec_frame0, int n_rec, int T3, int NC, int hop3, int weighting,
                                        const double* sums, const float* g_weak, float* d_win_strong, float* d_win_att,
                                        int32_t* err, void* stream) {
    const char* what = "sed_stitch_weak_backward";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && sums && g_weak && d_win_strong && d_win_att && err, "null argument");
    StTables t;
    SED_TRY(st_front(what, rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, 1, 31, &t));
    ST_NEED(((uintptr_t)sums % 8) == 0, "sums must be 8-byte aligned");
    const StPoolBwdArgs wa = {t, win_strong, win_att, sums, g_weak, d_win_strong, d_win_att, StRows{}};
    return sb_launch<false>(wa, stream);
}

// ---- backward through the span tags (sed_stitch_span_tags_backward, sed_stitch_piece_span_tags_backward) ---------------------
// The host side of both: rec_span_off null is the span entry.
static int sb_run(const char* what, const float* win_strong, const float* win_att, const int32_t* rec_win0, const int64_t* rec_frame0,
                  const int64_t* rec_span0, const int32_t* rec_span_off, long long total_spans, int n_rec, int T3, int NC, int hop3,
                  int weighting, int span3, const double* sums, const float* g_tags, float* d_win_strong, float* d_win_att,
                  int32_t* err, void* stream) {
    StTables t;
    SED_TRY(st_front(what, rec_win0, rec_frame0, err, n_rec, T3, NC, hop3, weighting, 1, 31, &t));
    ST_NEED(span3 >= 1 && total_spans >= n_rec && total_spans < (1ll << 31) && total_spans * NC < (1ll << 31),
            "need span3 >= 1, n_rec <= total_spans and total_spans * NC < 2^31");
    ST_NEED(((uintptr_t)sums % 8) == 0, "sums must be 8-byte aligned");
    const StPoolBwdArgs wa = {t, win_strong, win_att, sums, g_tags, d_win_strong, d_win_att,
                              StRows{rec_span0, rec_span_off, total_spans, span3, 0}};
    return sb_launch<true>(wa, stream);
}

extern "C" int sed_stitch_span_tags_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                             const int64_t* rec_frame0, const int64_t* rec_span0, long long total_spans, int n_rec,
                                             int T3, int NC, int hop3, int weighting, int span3, const double* sums,
                                             const float* g_tags, float* d_win_strong, float* d_win_att, int32_t* err,
                                             void* stream) {
    const char* what = "sed_stitch_span_tags_backward";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && rec_span0 && sums && g_tags && d_win_strong && d_win_att && err,
            "null argument");
    return sb_run(what, win_strong, win_att, rec_win0, rec_frame0, rec_span0, nullptr, total_spans, n_rec, T3, NC, hop3, weighting,
                  span3, sums, g_tags, d_win_strong, d_win_att, err, stream);
}

extern "C" int sed_stitch_piece_span_tags_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                                   const int64_t* rec_frame0, const int64_t* rec_span0, long long total_spans,
                                                   int n_rec, int T3, int NC, int hop3, int weighting, int span3,
                                                   const int32_t* rec_span_off, const double* sums, const float* g_tags,
                                                   float* d_win_strong, float* d_win_att, int32_t* err, void* stream) {
    const char* what = "sed_stitch_piece_span_tags_backward";
    ST_NEED(win_strong && win_att && rec_win0 && rec_frame0 && rec_span0 && rec_span_off && sums && g_tags && d_win_strong &&
                d_win_att && err, "null argument");
    return sb_run(what, win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, total_spans, n_rec, T3, NC, hop3,
                  weighting, span3, sums, g_tags, d_win_strong, d_win_att, err, stream);
}
