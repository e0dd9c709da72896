"""TEST INFRASTRUCTURE ONLY - a plain-loop statement of the OVERALL error rate with substitutions (include/dcase_sed.h,
"overall error rate"), for lists of any length.  Nothing here shares code or structure with the kernels: the segment part
builds a set of classes per segment, the event part a double-loop time-compatibility matrix (the label ignored) over ALL the
file's events and scipy's Hopcroft-Karp on it.  ``greedy_nsubs`` restates sed_eval's own substitution count - a greedy pass
over what a label-wise matching left over - for the inequality the project's definition rests on.

Events are ``(onset, offset)`` tuples of Python floats; ``cols[c]`` is the list of class c of one file.
"""
import math

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching


def time_compatible(r, e, t_collar=0.200, percentage_of_length=0.2):
    return (math.fabs(r[0] - e[0]) <= t_collar
            and math.fabs(r[1] - e[1]) <= max(t_collar, percentage_of_length * (r[1] - r[0])))


def _matching(ref, est, t_collar, percentage_of_length):
    """est index matched to each reference (-1: none) in a maximum matching of the time-compatibility relation."""
    if not ref or not est:
        return [-1] * len(ref)
    h = np.zeros((len(ref), len(est)), dtype=np.int8)
    for j, r in enumerate(ref):
        for i, e in enumerate(est):
            h[j, i] = time_compatible(r, e, t_collar, percentage_of_length)
    if not h.any():
        return [-1] * len(ref)
    return [int(v) for v in maximum_bipartite_matching(csr_matrix(h), perm_type="column")]


def flat(cols):
    return [ev for col in cols for ev in col]


def n_any(ref_cols, est_cols, t_collar=0.200, percentage_of_length=0.2):
    """Size of a maximum bipartite matching over all events of the file, labels ignored."""
    return sum(m >= 0 for m in _matching(flat(ref_cols), flat(est_cols), t_collar, percentage_of_length))


def n_tp(ref_cols, est_cols, t_collar=0.200, percentage_of_length=0.2):
    """Sum over the classes of the label-wise maximum matching (today's Ntp)."""
    return sum(sum(m >= 0 for m in _matching(r, e, t_collar, percentage_of_length)) for r, e in zip(ref_cols, est_cols))


def event_overall(ref_cols, est_cols, t_collar=0.200, percentage_of_length=0.2):
    """One file -> (Nref, Nsys, Nany)."""
    return (len(flat(ref_cols)), len(flat(est_cols)), n_any(ref_cols, est_cols, t_collar, percentage_of_length))


def greedy_nsubs(ref_cols, est_cols, t_collar=0.200, percentage_of_length=0.2):
    """sed_eval's substitutions: after the label-wise matching (scipy's, here), every leftover reference, in (class, onset)
    order, takes the first leftover estimated event, in (class, onset) order, that is time-compatible and still free."""
    ref_left, est_left = [], []
    for r, e in zip(ref_cols, est_cols):
        r, e = sorted(r), sorted(e)
        m = _matching(r, e, t_collar, percentage_of_length)
        ref_left += [ev for ev, k in zip(r, m) if k < 0]
        est_left += [ev for i, ev in enumerate(e) if i not in set(m)]
    used, n = set(), 0
    for r in ref_left:
        for i, e in enumerate(est_left):
            if i not in used and time_compatible(r, e, t_collar, percentage_of_length):
                used.add(i)
                n += 1
                break
    return n


def segment_overall(ref_cols, est_cols, res=1.0):
    """One file -> (S, D, I): per segment the SETS of active classes on each side."""
    offsets = [off for cols in (ref_cols, est_cols) for col in cols for _, off in col]
    n_seg = max(0, int(math.ceil(max(offsets) / res))) if offsets else 0
    active = []
    for cols in (ref_cols, est_cols):
        per_seg = [set() for _ in range(n_seg)]
        for c, col in enumerate(cols):
            for on, off in col:
                for s in range(max(0, int(math.floor(on / res))), max(0, int(math.ceil(off / res)))):
                    per_seg[s].add(c)
        active.append(per_seg)
    S = D = I = 0
    for R, E in zip(*active):
        fn, fp = len(R - E), len(E - R)
        S += min(fn, fp)
        D += max(0, fn - fp)
        I += max(0, fp - fn)
    return S, D, I


def set_overall(ref_cols, est_cols, t_collar=0.200, percentage_of_length=0.2, res=1.0):
    """All files: (ev [N, 3] (Nref, Nsys, Nany), seg [N, 3] (S, D, I)) int64."""
    ev = [event_overall(r, e, t_collar, percentage_of_length) for r, e in zip(ref_cols, est_cols)]
    seg = [segment_overall(r, e, res) for r, e in zip(ref_cols, est_cols)]
    return np.array(ev, np.int64).reshape(-1, 3), np.array(seg, np.int64).reshape(-1, 3)


def merged_clusters(ref_cols, est_cols, t_collar=0.200):
    """The clusters of the file's MERGED lists as ``(rank of its first reference among the file's references by onset,
    reference events, estimated events)``: the valid-cut rule of the header, restated on a sort of all onsets.  A cut after
    merged position p is valid iff the first estimated onset still to come - the last reference onset so far > t_collar,
    and the same with the sides swapped."""
    merged = sorted([(ev[0], 0) for ev in flat(ref_cols)] + [(ev[0], 1) for ev in flat(est_cols)])
    inf = float("inf")
    nxt = [[inf, inf] for _ in range(len(merged) + 1)]
    for p in range(len(merged) - 1, -1, -1):
        nxt[p] = list(nxt[p + 1])
        nxt[p][merged[p][1]] = merged[p][0]
    out, cur, last, seen_ref = [], [0, 0], [-inf, -inf], 0
    for p, (on, side) in enumerate(merged):
        cur[side] += 1
        last[side] = on
        if nxt[p + 1][1] - last[0] > t_collar and nxt[p + 1][0] - last[1] > t_collar:
            out.append((seen_ref, cur[0], cur[1]))
            seen_ref += cur[0]
            cur = [0, 0]
    assert cur == [0, 0]
    return out


def merged_cluster_sizes(ref_cols, est_cols, t_collar=0.200):
    """(most reference events, most estimated events) in one merged cluster of the file; (0, 0) when empty."""
    cl = merged_clusters(ref_cols, est_cols, t_collar)
    return (max((c[1] for c in cl), default=0), max((c[2] for c in cl), default=0))


def rates(n_ref, subs, dele, ins):
    """(ER, S, D, I rates); NaN when there is no reference."""
    if n_ref <= 0:
        return (float("nan"),) * 4
    return ((subs + dele + ins) / n_ref, subs / n_ref, dele / n_ref, ins / n_ref)
