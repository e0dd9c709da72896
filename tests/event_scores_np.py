"""TEST INFRASTRUCTURE ONLY - plain-loop statement of the event scores and of the select by score (include/dcase_sed.h):
per event the largest non-NaN posterior and the mean of the posteriors over its frames, and the events whose score exceeds
the minimum of their (point, class).  Written event by event and frame by frame: no vectorised reduction, so it is independent
both of how the kernel splits the work and of the numpy reduceat route that tools/long_bench.py --scores times."""
import math

import numpy as np


def event_max(values):
    """The largest non-NaN value (the stored float32 itself), NaN when there is none."""
    best = None
    for v in values:
        if v != v:
            continue
        if best is None or v > best:
            best = v
    return np.float32(np.nan) if best is None else np.float32(best)


def event_mean(values):
    """float32(exact sum of the widened values / n): math.fsum is the correctly rounded sum.  NaN if any frame is NaN."""
    wide = [float(v) for v in values]
    for v in wide:
        if v != v:
            return np.float32(np.nan)
    return np.float32(math.fsum(wide) / len(wide))


def column_of(col, n_rec, NC):
    """(point, recording, class) of a column in the sweep's order (k * n_rec + rec) * NC + c."""
    return col // (n_rec * NC), (col // NC) % n_rec, col % NC


def scores(timeline, rec_frame0, n_rec, NC, ev_ptr, ev_pairs):
    """(score_max, score_mean) float32 [ev_ptr[-1]] of a valid table on ``timeline`` [total, NC] float32.  An event outside
    0 <= on < off <= L3 scores NaN twice (the kernel's err bit 64)."""
    timeline = np.asarray(timeline, np.float32).reshape(-1, NC)
    n = int(ev_ptr[-1])
    smax, smean = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    for col in range(len(ev_ptr) - 1):
        _, rec, c = column_of(col, n_rec, NC)
        f0, L3 = int(rec_frame0[rec]), int(rec_frame0[rec + 1]) - int(rec_frame0[rec])
        for i in range(int(ev_ptr[col]), int(ev_ptr[col + 1])):
            on, off = int(ev_pairs[i][0]), int(ev_pairs[i][1])
            if on < 0 or off > L3 or on >= off:
                continue
            values = [timeline[f0 + u, c] for u in range(on, off)]
            smax[i], smean[i] = event_max(values), event_mean(values)
    return smax, smean


def select(ev_ptr, ev_pairs, score_max, score_mean, n_rec, NC, min_score, key):
    """The events with score_key > min_score[k][c] (strict; NaN never), column by column: (out_ptr int64 [n_cols + 1], out_pairs
    int32 [kept, 2], out_score_max, out_score_mean float32 [kept] - None where the input is None)."""
    min_score = np.asarray(min_score, np.float32).reshape(-1, NC)
    score = (score_max, score_mean)[key]
    counts, kept = [], []
    for col in range(len(ev_ptr) - 1):
        k, _, c = column_of(col, n_rec, NC)
        n = 0
        for i in range(int(ev_ptr[col]), int(ev_ptr[col + 1])):
            if score[i] > min_score[k, c]:
                kept.append(i)
                n += 1
        counts.append(n)
    out_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out_pairs = np.asarray([ev_pairs[i] for i in kept], np.int32).reshape(-1, 2)
    pick = lambda s: None if s is None else np.asarray([s[i] for i in kept], np.float32)
    return out_ptr, out_pairs, pick(score_max), pick(score_mean)
