"""TEST INFRASTRUCTURE ONLY - a deliberately naive statement, in Python floats (IEEE float64) and plain loops, of the PSDS
definitions that ``dcase2019_task4_amd.metrics`` and ``csrc/score.hip`` restate from Bilen et al. (ICASSP 2020).  psds_eval
itself is absent from this image: parity with it is unpinned; this file is the independent statement the device counts and the
host curve are pinned to.  It shares no code with ``metrics.py``.

Events are ``(onset, offset)`` tuples of Python floats, one list per (file, class) column, as in ``tests/sed_eval_np.py``.  A
column is scored in the order the packed arrays hold it: sorted by onset, then offset.
"""
import math


def intersection(d, g):
    return max(0.0, min(d[1], g[1]) - max(d[0], g[0]))


def length(e):
    return e[1] - e[0]


def covered(total, span, threshold):
    """``total / span >= threshold``: the division first; a span <= 0 and a NaN ratio fail."""
    if not span > 0.0:
        return False
    ratio = total / span
    return (not math.isnan(ratio)) and ratio >= threshold


def overlap_sum(event, others):
    total = 0.0
    for o in others:
        total = total + intersection(event, o)
    return total


def relevant_mask(dets, gts, dtc):
    return [covered(overlap_sum(d, gts), length(d), dtc) for d in dets]


def found_mask(dets, gts, relevant, gtc):
    out = []
    for g in gts:
        total = 0.0
        for d, rel in zip(dets, relevant):
            if rel:
                total = total + intersection(d, g)
        out.append(covered(total, length(g), gtc))
    return out


def file_counts(ref_cols, est_cols, dtc=0.5, gtc=0.5, cttc=0.3):
    """One file: ``ref_cols[c]`` / ``est_cols[c]`` = event lists of class c -> rows ``[TP, FP, CT[c][0], .., CT[c][NC - 1]]``."""
    nc = len(ref_cols)
    ref_cols = [sorted(col) for col in ref_cols]
    est_cols = [sorted(col) for col in est_cols]
    rows = []
    for c in range(nc):
        relevant = relevant_mask(est_cols[c], ref_cols[c], dtc)
        tp = sum(found_mask(est_cols[c], ref_cols[c], relevant, gtc))
        fp = sum(1 for rel in relevant if not rel)
        ct = [0] * nc
        for d, rel in zip(est_cols[c], relevant):
            if rel:
                continue
            for k in range(nc):
                if k != c and covered(overlap_sum(d, ref_cols[k]), length(d), cttc):
                    ct[k] += 1
        rows.append([tp, fp] + ct)
    return rows


def set_counts(ref_cols, est_cols, **kw):
    """All files: nested lists ``[N][NC][2 + NC]``."""
    return [file_counts(r, e, **kw) for r, e in zip(ref_cols, est_cols)]


def psd_roc(totals, n_gt, gt_duration, dataset_duration, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0):
    """``totals[o][c] = [TP, FP, CT[c][0 .. NC - 1]]`` of K operating points -> ``(axis, eff_tpr, efpr[o][c])``, rates per hour."""
    unit = 3600.0
    K, nc = len(totals), len(n_gt)
    for c in range(nc):
        if n_gt[c] == 0:
            raise ValueError(f"class {c} has no reference events")
    tpr = [[totals[o][c][0] / n_gt[c] for c in range(nc)] for o in range(K)]
    efpr = [[0.0] * nc for _ in range(K)]
    for o in range(K):
        for c in range(nc):
            cross = 0.0
            for k in range(nc):
                if k != c and gt_duration[k] != 0:
                    cross += unit * totals[o][c][2 + k] / gt_duration[k]
            efpr[o][c] = unit * totals[o][c][1] / dataset_duration + (alpha_ct * cross / (nc - 1) if nc > 1 else 0.0)
    axis = sorted({efpr[o][c] for o in range(K) for c in range(nc) if efpr[o][c] <= max_efpr})
    eff = []
    for x in axis:
        values = [max([tpr[o][c] for o in range(K) if efpr[o][c] <= x], default=0.0) for c in range(nc)]
        mu = sum(values) / nc
        sigma = math.sqrt(sum((v - mu) ** 2 for v in values) / nc)
        eff.append(max(0.0, mu - alpha_st * sigma))
    return axis, eff, efpr


def psds(totals, n_gt, gt_duration, dataset_duration, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0):
    axis, eff, _ = psd_roc(totals, n_gt, gt_duration, dataset_duration, alpha_ct, alpha_st, max_efpr)
    area = 0.0
    for i, x in enumerate(axis):
        area += eff[i] * ((axis[i + 1] if i + 1 < len(axis) else max_efpr) - x)
    return area / max_efpr
