"""TEST INFRASTRUCTURE ONLY - a plain-loop statement of the rule that lets ``sed_long_event_counts`` split a long column: the
valid cuts of the merged onset order and the clusters between them (include/dcase_sed.h), plus the builders of the columns
the long-scoring tests use.  Nothing here shares code with the kernels: the merge is a sort, the cut test a loop over merged
positions, the matching of a cluster is ``sed_eval_np.optimal_ntp``.

Events are ``(onset, offset)`` tuples of Python floats, one list per (recording, class) column, sorted by onset.
"""
import math

import numpy as np

from tests import sed_eval_np as se

INF = float("inf")


def clusters(ref, est, t_collar=0.200):
    """The clusters of one column as ``(ref_indices, est_indices)`` lists, in merged order.  A cut after merged position p is
    valid iff ``last reference onset at or before p + t_collar < first estimated onset after p`` and ``last estimated onset at
    or before p + t_collar < first reference onset after p`` (a missing side: minus / plus infinity)."""
    merged = sorted([(on, 0, i) for i, (on, _) in enumerate(ref)] + [(on, 1, i) for i, (on, _) in enumerate(est)],
                    key=lambda m: m[0])
    n = len(merged)
    first_after = [[INF, INF] for _ in range(n + 1)]                 # [p][side]: first onset of `side` at a position >= p
    for p in range(n - 1, -1, -1):
        first_after[p] = list(first_after[p + 1])
        first_after[p][merged[p][1]] = merged[p][0]
    out, cur, last = [], ([], []), [-INF, -INF]
    for p, (on, side, i) in enumerate(merged):
        cur[side].append(i)
        last[side] = on
        if last[0] + t_collar < first_after[p + 1][1] and last[1] + t_collar < first_after[p + 1][0]:
            out.append(cur)
            cur = ([], [])
    assert cur == ([], [])                                            # the cut after the last position is always valid
    return out


def cluster_sizes(ref, est, t_collar=0.200):
    """(largest number of reference events, largest number of estimated events) over the clusters; (0, 0) when empty."""
    cl = clusters(ref, est, t_collar)
    return (max((len(r) for r, _ in cl), default=0), max((len(e) for _, e in cl), default=0))


def cluster_ntp(ref, est, t_collar=0.200, percentage_of_length=0.2):
    """Sum over the clusters of the size of a maximum matching inside the cluster."""
    return sum(se.optimal_ntp([ref[i] for i in r], [est[j] for j in e], t_collar, percentage_of_length)
               for r, e in clusters(ref, est, t_collar) if r and e)


def decreasing(col):
    return any(b[0] < a[0] for a, b in zip(col, col[1:]))


def expected_err(ref_cols, est_cols, t_collar=0.200, res=1.0):
    """The error word the cluster statement gives for ``cols[recording][class]``: 64 for a column with a decreasing onset
    (that column is then not clustered), 1 / 2 for a cluster of more than 64 reference / estimated events, 4 for a recording
    of more than 65 536 segments."""
    err = 0
    for r_file, e_file in zip(ref_cols, est_cols):
        offs = [off for cols in (r_file, e_file) for col in cols for _, off in col]
        if offs and math.ceil(max(offs) / res) > 65536:
            err |= 4
        for r, e in zip(r_file, e_file):
            if decreasing(r) or decreasing(e):
                err |= 64
                continue
            nr, ne = cluster_sizes(r, e, t_collar)
            err |= (1 if nr > 64 else 0) | (2 if ne > 64 else 0)
    return err


# ---- builders -------------------------------------------------------------------------------------------------------------------
def burst_column(rs, n_bursts=30, n_max=60, span=3.0, gap=8.0):
    """(ref, est): ``n_bursts`` bursts of ``sed_eval_np.dense_events(n_max, span)`` placed ``gap`` seconds apart - about
    ``n_bursts * n_max / 2`` heavily overlapping events per side, compatibility graphs with long augmenting paths (both greedy
    first-fit orders lose matches on them), clusters of at most one burst."""
    ref, est = [], []
    for b in range(n_bursts):
        for side in (ref, est):
            side += [(on + b * gap, off + b * gap) for on, off in se.dense_events(rs, 1, 1, n_max, span)[0][0]]
    return sorted(ref), sorted(est)


def spaced_column(rs, n, gap=0.75, p_drop=0.1, p_extra=0.1, p_zero=0.05):
    """(ref, est) with exactly ``n`` reference events about ``gap`` seconds apart, lengths 0.2 .. 2 s (neighbours overlap), a few
    of length zero; the estimated events are the references jittered by up to 0.3 s, some dropped, some extra ones."""
    ref, est = [], []
    for k in range(n):
        on = k * gap + float(rs.uniform(0.0, 0.1))
        length = 0.0 if rs.uniform() < p_zero else float(rs.uniform(0.2, 2.0))
        ref.append((on, on + length))
        if rs.uniform() >= p_drop:
            a = max(0.0, on + float(rs.uniform(-0.3, 0.3)))
            est.append((a, max(a, on + length + float(rs.uniform(-0.3, 0.3)))))
        if rs.uniform() < p_extra:
            a = on + float(rs.uniform(0.0, gap))
            est.append((a, a + float(rs.uniform(0.0, 1.0))))
    return sorted(ref), sorted(est)


def tile_edge_column(rs, tile, n):
    """``spaced_column`` of ``n`` references in which references ``tile - 3 .. tile + 2`` (and ``2 * tile - 1 .. 2 * tile`` when
    there are that many) are moved to within 0.05 s of each other, with as many estimated events among them: clusters that
    straddle the edges between the tiles of ``tile`` reference events."""
    ref, est = spaced_column(rs, n)
    for lo, hi in ((tile - 3, tile + 3), (2 * tile - 1, 2 * tile + 1)):
        if hi > n:
            continue
        t0 = ref[lo][0]
        est = [e for e in est if not (t0 - 0.6 <= e[0] <= ref[hi - 1][0] + 0.6)]
        for k in range(lo, hi):
            on = t0 + 0.05 * (k - lo)
            ref[k] = (on, on + 1.0 + 0.01 * k)
            est.append((on + 0.02, on + 1.0))
    assert not decreasing(ref)
    return ref, sorted(est)


def chained_pair(n, delta, step=1.0 / 64, t_collar=0.25):
    """(ref, est): two chains of ``n`` references and ``n`` estimated events each (onsets ``step`` apart, all dyadic: every sum
    and difference below is exact), the first reference of the second chain ``t_collar + delta`` after the last estimated
    onset of the first.  ``delta = 0``: the pair is compatible, no cut, ONE cluster of 2n per side; ``delta`` = one ulp: cut."""
    ref = [(k * step, k * step + 0.5) for k in range(n)]
    est = [(k * step + step / 2, k * step + step / 2 + 0.5) for k in range(n)]
    start = est[-1][0] + t_collar + delta
    ref += [(start + k * step, start + k * step + 0.5) for k in range(n)]
    est += [(start + k * step + step / 2, start + k * step + step / 2 + 0.5) for k in range(n)]
    return ref, est


def pack(cols):
    """cols[recording][class] -> CSR (ptr int64, onset, offset) in stored order (no sorting: the caller's order)."""
    flat = [col for file_cols in cols for col in file_cols]
    ptr = np.r_[0, np.cumsum([len(c) for c in flat])].astype(np.int64)
    on = np.array([e[0] for c in flat for e in c], dtype=np.float64)
    off = np.array([e[1] for c in flat for e in c], dtype=np.float64)
    return ptr, on, off


def main_columns(tile, seed=0):
    """The 3 recordings x 3 classes the exact-agreement test scores: reference lengths 0, 1, 64, 65, the burst column,
    tile - 1, tile, tile + 1 and 2 * tile + 5 (the last three with clusters across tile edges)."""
    rs = np.random.RandomState(seed)
    builders = [lambda: spaced_column(rs, 0), lambda: spaced_column(rs, 1), lambda: spaced_column(rs, 64),
                lambda: spaced_column(rs, 65), lambda: burst_column(rs), lambda: spaced_column(rs, tile - 1),
                lambda: tile_edge_column(rs, tile, tile), lambda: tile_edge_column(rs, tile, tile + 1),
                lambda: tile_edge_column(rs, tile, 2 * tile + 5)]
    pairs = [b() for b in builders]
    pairs[0] = ([], [(0.5, 1.0), (3.0, 3.0)])                         # no reference: estimated events alone
    ref = [[pairs[3 * f + c][0] for c in range(3)] for f in range(3)]
    est = [[pairs[3 * f + c][1] for c in range(3)] for f in range(3)]
    return ref, est


def small_columns(n_rec, nclass, seed, n_max=90):
    rs = np.random.RandomState(seed)
    pairs = [[spaced_column(rs, int(rs.randint(0, n_max + 1))) for _ in range(nclass)] for _ in range(n_rec)]
    return [[p[0] for p in f] for f in pairs], [[p[1] for p in f] for f in pairs]


# ---- a decoded table without a GPU: the patterns the frames-mode test feeds sed_stitch_decode (window 1: run-length decode) -----
def stitch_lengths(stitch_tile):
    return [stitch_tile + 9, 5, 1500]


def stitch_patterns(L3s, nclass=3, seed=8):
    """Per recording a [L3, nclass] bool activity: two-state chains - a flicker, short events, long events."""
    rs = np.random.RandomState(seed)
    chains = [(0.2, 0.6), (0.15, 0.3), (0.05, 0.05)]
    out = []
    for L3 in L3s:
        a = np.zeros((L3, nclass), dtype=bool)
        for c in range(nclass):
            p_on, p_off = chains[c % len(chains)]
            state = False
            for t in range(L3):
                state = (rs.uniform() >= p_off) if state else (rs.uniform() < p_on)
                a[t, c] = state
        out.append(a)
    return out


def stitch_columns(patterns, num, den):
    """cols[recording][class] = the runs of the pattern as (onset frame * num / den, exclusive offset frame * num / den)."""
    cols = []
    for a in patterns:
        file_cols = []
        for c in range(a.shape[1]):
            edges = np.flatnonzero(np.diff(np.r_[0, a[:, c].astype(np.int8), 0]))
            file_cols.append([(int(on) * num / den, int(off) * num / den) for on, off in zip(edges[0::2], edges[1::2])])
        cols.append(file_cols)
    return cols


def sorted_jittered_references(cols, seed):
    return [[sorted(c) for c in f] for f in se.jittered_references(cols, np.random.RandomState(seed))]
