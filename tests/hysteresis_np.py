"""TEST INFRASTRUCTURE ONLY - plain-loop statement of the two-threshold (hysteresis) decode (include/dcase_sed.h): per column
the events of the low-threshold decode that hold the onset of an event of the high-threshold decode, both decodes by
tests/stitch_np.py with the same median window.  Written event by event, independent of how the kernels split the work."""
import numpy as np

from tests import stitch_np


def smooth_timeline(seed, L, NC=3):
    """Smooth random posteriors in (0, 1): uniform noise through a moving average of a random width, stretched to [0, 1]."""
    rs = np.random.RandomState(seed)
    w = int(rs.randint(1, 24))
    x = rs.uniform(size=(L + w - 1, NC))
    y = np.stack([np.convolve(x[:, c], np.ones(w) / w, mode="valid") for c in range(NC)], axis=1)
    y = (y - y.min(0)) / np.maximum(y.max(0) - y.min(0), 1e-9)
    return (0.02 + 0.96 * y).astype(np.float32)


def select(lo_ptr, lo_pairs, hi_ptr, hi_pairs):
    """The double loop on two event tables (ptr [n_cols + 1], pairs [n, 2]): a low event [on, off) is kept iff
    any(on <= on_hi < off) over the high events of the same column.  Returns (ptr [n_cols + 1] int64, pairs [kept, 2] int32)."""
    counts, kept = [], []
    for col in range(len(lo_ptr) - 1):
        n = 0
        for on, off in lo_pairs[int(lo_ptr[col]):int(lo_ptr[col + 1])]:
            if any(on <= b_on < off for b_on, _ in hi_pairs[int(hi_ptr[col]):int(hi_ptr[col + 1])]):
                kept.append((int(on), int(off)))
                n += 1
        counts.append(n)
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(kept, dtype=np.int32).reshape(-1, 2))


def decode(timeline, rec_frame0, thr_lo, thr_hi, win):
    """One threshold pair (thr_lo [NC] <= thr_hi [NC], win [NC]) on a blended timeline [sum L3, NC]: (ev_ptr
    [n_rec * NC + 1] int64, ev_pairs [n_events, 2] int32), plus the two plain decodes it selects from."""
    _, lo_ptr, lo_pairs = stitch_np.decode(timeline, rec_frame0, thr_lo, win)
    _, hi_ptr, hi_pairs = stitch_np.decode(timeline, rec_frame0, thr_hi, win)
    ev_ptr, ev_pairs = select(lo_ptr, lo_pairs, hi_ptr, hi_pairs)
    return ev_ptr, ev_pairs, (lo_ptr, lo_pairs), (hi_ptr, hi_pairs)


def decode_pairs(timeline, rec_frame0, thr_lo, thr_hi, win):
    """K pairs (arrays [K, NC]) as one table in column order (k, rec, c), like inference.stitch_hysteresis."""
    ptrs, pairs, base = [np.zeros(1, np.int64)], [], 0
    for k in range(len(thr_lo)):
        ev_ptr, ev_pairs, _, _ = decode(timeline, rec_frame0, thr_lo[k], thr_hi[k], win[k])
        ptrs.append(ev_ptr[1:] + base)
        pairs.append(ev_pairs)
        base += int(ev_ptr[-1])
    return np.concatenate(ptrs), np.concatenate(pairs)
