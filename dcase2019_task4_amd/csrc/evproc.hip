// evproc.hip - minimum event length and gap merging on a CSR event table: sed_events_process drops the events of a column
// that are shorter than min_len and fuses consecutive events whose gap is at most max_gap, in either order (the definition
// is in include/dcase_sed.h).  An event-domain operator on the flat geometry and the compaction of evtable.h, which the
// select of evscore.hip shares (hyst.hip alone keeps its own copies): a thread owns one index of `pairs`, a wave's decisions
// are one ballot word, one-workgroup scans carry them across workgroups.  The scan kernel of both files lives here.
//
// Both orders are the same two questions, asked of two flag words A and B per index:
//   "the last index < p with A set"      the A words of p's workgroup, then the scanned per-workgroup maximum (ev_last_before)
//   "the indices < p with B set"         the B words of p's workgroup and the scanned per-workgroup count (hy_flagged_before)
// order 0, DROP then MERGE: A = the event is kept (off - on >= min_len).  The predecessor of a kept event is the last A index
//   in front of it, cut off at the column start - however many dropped events lie between.  B = head: a kept event with no
//   predecessor or with on - off_pred > max_gap.  A head's rank among the heads is its output slot: it writes its onset there
//   and its predecessor's offset into the slot before; the thread of column c writes the offset of the column's last kept
//   event into the column's last slot.
// order 1, MERGE then DROP: A = head of a chain (the column's first event, or on - off of the event before > max_gap).
//   B = a chain's last event whose merged event [on of the last A index at or before it, its own off) is at least min_len
//   long: it writes that pair to its rank among the B indices.
// Five launches whatever K, n_cols and the column lengths are:
//   k_evp_flag   A, its ballot words, per workgroup the last A index (-1: none); the column's order is checked here (err 64)
//   k_evp_scan   one workgroup: exclusive running maximum of those
//   k_evp_link   B from A, its ballot words, the workgroup counts
//   k_evp_scan   one workgroup: exclusive sum of the counts, the total behind them; capacity check (err 2)
//   k_evp_write  the events; thread c <= n_cols writes out_ptr[c] and validates column c's bounds (err 16)
// No thread's work grows with a column, a chain or a run of dropped events: a lookup reads at most HY_WAVES ballot words and
// one carry.  Every ptr entry is validated before it is used as an index: the kernels read ev_ptr [0, n_cols], pairs
// [0, pairs_capacity) and the parameters of an existing (point, class) only, and write the outputs inside their sizes,
// whatever the table holds.  No atomics but the OR into err, integer results only.
#include "common.h"
#include "kernels.h"
#include "evtable.h"

struct EvpArgs {
    EvTable t;                   // bal / cnt: the flags B and their counts
    uint64_t* bal_a;             // ws: [n_blocks][HY_WAVES] the flags A of 64 indices
    int32_t* last_a;             // ws: [n_blocks + 1] the last A index of a workgroup; after the scan that of all workgroups before it
    long long span;              // n_rec * NC: the columns of one point
    int NC;
    const int32_t *min_len, *max_gap;                // [n_cols / span][NC]
};

// The last index < p with its A flag set, -1 when there is none; 0 <= p <= cap.  At most HY_WAVES words and one carry.
__device__ __forceinline__ long long ev_last_before(const EvpArgs& e, long long p) {
    if (p <= 0) return -1;
    const long long q = p - 1, w0 = (q / HY_THREADS) * HY_WAVES;
    long long w = q >> 6;
    uint64_t word = e.bal_a[w] & (~0ull >> (63 - (int)(q & 63)));
    while (word == 0 && w > w0) word = e.bal_a[--w];
    return word ? w * 64 + 63 - __clzll((long long)word) : (long long)e.last_a[q / HY_THREADS];
}

template <int ORDER>
__global__ __launch_bounds__(HY_THREADS) void k_evp_flag(EvpArgs e) {
    __shared__ uint64_t s_word[HY_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * HY_THREADS + tid;
    bool flag = false;
    if (i < e.t.cap) {
        long long a, b;
        const long long c = hy_column(e.t.ptr, e.t.n_cols, i);
        if (hy_bounds(e.t.ptr, c, e.t.cap, a, b) && i >= a && i < b) {               // i is event i - a of column c
            const hy_i32x2 ev = *(const hy_i32x2*)(e.t.pairs + 2 * (size_t)i);
            const long long on = ev.x, off = ev.y;
            if (on >= off || (i + 1 < b && e.t.pairs[2 * (size_t)(i + 1)] < off)) atomicOr(e.t.err, 64);
            if (ORDER == 0) {
                const long long m = e.min_len[ev_param(e.span, e.NC, c)];
                flag = m <= 0 || off - on >= m;
            } else {
                flag = i == a || on - (long long)e.t.pairs[2 * (size_t)(i - 1) + 1] > (long long)e.max_gap[ev_param(e.span, e.NC, c)];
            }
        }
    }
    const uint64_t word = __ballot(flag);
    if (lane == 0) {
        e.bal_a[(size_t)blockIdx.x * HY_WAVES + wave] = word;
        s_word[wave] = word;
    }
    __syncthreads();
    if (tid == 0) {
        long long last = -1;
#pragma unroll
        for (int w = 0; w < HY_WAVES; ++w)
            if (s_word[w]) last = (long long)blockIdx.x * HY_THREADS + w * 64 + 63 - __clzll((long long)s_word[w]);
        e.last_a[blockIdx.x] = (int32_t)last;
    }
}

template <int ORDER>
__global__ __launch_bounds__(HY_THREADS) void k_evp_link(EvpArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    bool flag = false;
    if (ORDER == 0) {
        if (i < e.t.cap && ev_bit(e.bal_a, i)) {                                     // kept: its column's bounds were valid
            const long long c = hy_column(e.t.ptr, e.t.n_cols, i);
            const long long pred = ev_last_before(e, i);
            flag = pred < e.t.ptr[c] ||
                   (long long)e.t.pairs[2 * (size_t)i] - (long long)e.t.pairs[2 * (size_t)pred + 1] >
                       (long long)e.max_gap[ev_param(e.span, e.NC, c)];
        }
    } else if (i < e.t.cap) {
        long long a, b;
        const long long c = hy_column(e.t.ptr, e.t.n_cols, i);
        if (hy_bounds(e.t.ptr, c, e.t.cap, a, b) && i >= a && i < b) {
            const long long par = ev_param(e.span, e.NC, c), off = e.t.pairs[2 * (size_t)i + 1];
            if (i + 1 == b || (long long)e.t.pairs[2 * (size_t)(i + 1)] - off > (long long)e.max_gap[par]) {   // a chain ends here
                const long long head = ev_last_before(e, i + 1), m = e.min_len[par];
                flag = head >= a && (m <= 0 || off - (long long)e.t.pairs[2 * (size_t)head] >= m);
            }
        }
    }
    ev_ballot_count(flag, e.t.bal, e.t.cnt);
}

// One workgroup, a fixed order: v[b] = the maximum (MAX; -1 for none) or the sum of v[0 .. b - 1], v[n] = that of all n.  The
// sum stays below 2^31 (an index is flagged at most once) and is checked against the output capacity.
template <bool MAX>
__global__ __launch_bounds__(1024) void k_evp_scan(int32_t* v, long long n, long long out_cap, int32_t* err) {
    __shared__ int part[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int none = MAX ? -1 : 0;
    if (tid == 0) s_carry = none;
    __syncthreads();
    for (long long i0 = 0; i0 < n; i0 += 1024) {
        const long long i = i0 + tid;
        int incl = i < n ? v[i] : none;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int m = __shfl_up(incl, o);
            if (lane >= o) incl = MAX ? max(incl, m) : incl + m;
        }
        int excl = __shfl_up(incl, 1);                                               // (of the wave: what lies in front of this lane)
        if (lane == 0) excl = none;
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int before = s_carry;
        for (int k = 0; k < wave; ++k) before = MAX ? max(before, part[k]) : before + part[k];
        if (i < n) v[i] = MAX ? max(before, excl) : before + excl;
        __syncthreads();
        if (tid == 1023) s_carry = MAX ? max(before, incl) : before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        v[n] = s_carry;
        if (!MAX && s_carry > out_cap) atomicOr(err, 2);
    }
}

template <int ORDER>
__global__ __launch_bounds__(HY_THREADS) void k_evp_write(EvpArgs e) {
    const long long i = (long long)blockIdx.x * HY_THREADS + threadIdx.x;
    if (i < e.t.cap && ev_bit(e.t.bal, i)) {
        const long long dst = hy_flagged_before(e.t.bal, e.t.cnt, e.t.n_blocks, i);
        if (ORDER == 0) {                                                            // a head: its onset, its predecessor's offset
            if (dst < e.t.out_cap) e.t.out_pairs[2 * (size_t)dst] = e.t.pairs[2 * (size_t)i];
            const long long pred = ev_last_before(e, i);
            if (pred >= 0 && dst >= 1 && dst - 1 < e.t.out_cap && pred >= e.t.ptr[hy_column(e.t.ptr, e.t.n_cols, i)])
                e.t.out_pairs[2 * (size_t)(dst - 1) + 1] = e.t.pairs[2 * (size_t)pred + 1];
        } else if (dst < e.t.out_cap) {                                              // a chain's last event: the merged pair
            const long long head = ev_last_before(e, i + 1);                         // (>= its column's start: k_evp_link saw it)
            if (head >= 0) {
                const hy_i32x2 ev = {e.t.pairs[2 * (size_t)head], e.t.pairs[2 * (size_t)i + 1]};
                *(hy_i32x2*)(e.t.out_pairs + 2 * (size_t)dst) = ev;
            }
        }
    }
    long long a, b;
    if (ev_write_ptr(e.t, i, a, b) && ORDER == 0) {                                  // the column's last kept event closes its last slot
        const long long last = ev_last_before(e, b), dst = hy_flagged_before(e.t.bal, e.t.cnt, e.t.n_blocks, b) - 1;
        if (last >= a && dst >= 0 && dst < e.t.out_cap) e.t.out_pairs[2 * (size_t)dst + 1] = e.t.pairs[2 * (size_t)last + 1];
    }
}

int launch_ev_scan(const EvTable& t, hipStream_t st) {
    hipLaunchKernelGGL(k_evp_scan<false>, dim3(1), dim3(1024), 0, st, t.cnt, t.n_blocks, t.out_cap, t.err);
    SED_CHECK_LAUNCH();
    return SED_OK;
}

extern "C" size_t sed_events_process_ws_bytes(long long pairs_capacity, long long n_cols) {
    return ev_ws_bytes("sed_events_process", pairs_capacity, n_cols, 2);
}

template <int ORDER>
static int evp_launch(const EvpArgs& e, hipStream_t st) {
    if (e.t.n_blocks) {                                                              // (an empty pairs array has nothing to flag)
        hipLaunchKernelGGL(k_evp_flag<ORDER>, dim3((unsigned)e.t.n_blocks), dim3(HY_THREADS), 0, st, e);
        SED_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_evp_scan<true>, dim3(1), dim3(1024), 0, st, e.last_a, e.t.n_blocks, e.t.out_cap, e.t.err);
    SED_CHECK_LAUNCH();
    return ev_launch_compact(k_evp_link<ORDER>, k_evp_write<ORDER>, e, st);
}

extern "C" int sed_events_process(const int64_t* ev_ptr, const int32_t* pairs, long long pairs_capacity, long long n_cols,
                                  int n_rec, int NC, const int32_t* min_len, const int32_t* max_gap, int order,
                                  int64_t* out_ptr, int32_t* out_pairs, long long out_capacity, void* ws, size_t ws_bytes,
                                  int32_t* err, void* stream) {
    const char* who = "sed_events_process";
    EV_NEED(who, ev_ptr && pairs && min_len && max_gap && out_ptr && out_pairs && ws && err, "null argument");
    EV_NEED(who, order == 0 || order == 1, "order must be 0 (drop, then merge) or 1 (merge, then drop)");
    EvpArgs e = {{ev_ptr, pairs, pairs_capacity, n_cols, out_ptr, out_pairs, out_capacity, nullptr, nullptr, err,
                  ev_blocks(pairs_capacity)}, (uint64_t*)ws, nullptr, (long long)n_rec * NC, NC, min_len, max_gap};
    if (const int rc = ev_check(who, "pairs", "call", e.t, n_rec, NC, ws, ws_bytes, 2)) return rc;
    e.last_a = (int32_t*)((char*)ws + 2 * ev_bal_bytes(pairs_capacity));             // (behind the planes A and B)
    return order == 0 ? evp_launch<0>(e, (hipStream_t)stream) : evp_launch<1>(e, (hipStream_t)stream);
}

