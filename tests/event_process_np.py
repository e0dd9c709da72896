"""TEST INFRASTRUCTURE ONLY - plain-loop statement of minimum event length and gap merging on event lists
(include/dcase_sed.h, sed_events_process), written event by event and independent of how the kernels split the work, plus an
independent frame-domain statement (rasterise, clear short 1-runs, fill short interior 0-runs, relabel with
scipy.ndimage.label) that agrees with it on lists whose gaps are at least 1 frame."""
import numpy as np

ORDERS = {"drop_merge": 0, "merge_drop": 1}


def drop(events, m):
    """DROP(m): the events with off - on >= m; m <= 0 keeps everything."""
    return [(int(on), int(off)) for on, off in events if m <= 0 or int(off) - int(on) >= m]


def merge(events, g):
    """MERGE(g): consecutive events of THIS list join when on_next - off_prev <= g; g < 0 merges nothing."""
    out = []
    for on, off in events:
        on, off = int(on), int(off)
        if out and g >= 0 and on - out[-1][1] <= g:
            out[-1] = (out[-1][0], off)
        else:
            out.append((on, off))
    return out


def process(events, m, g, order):
    """order 0: DROP then MERGE; order 1: MERGE then DROP."""
    if order == 0:
        return merge(drop(events, m), g)
    if order == 1:
        return drop(merge(events, g), m)
    raise ValueError(order)


def process_table(ev_ptr, ev_pairs, n_rec, NC, min_len, max_gap, order):
    """A CSR table of K * n_rec * NC columns in the order (k * n_rec + rec) * NC + c with [K, NC] parameters:
    (out_ptr [n_cols + 1] int64, out_pairs [n, 2] int32)."""
    n_cols = len(ev_ptr) - 1
    assert n_cols % (n_rec * NC) == 0
    K = n_cols // (n_rec * NC)
    min_len = np.asarray(min_len).reshape(K, NC)
    max_gap = np.asarray(max_gap).reshape(K, NC)
    counts, rows = [], []
    for col in range(n_cols):
        k, c = col // (n_rec * NC), col % NC
        ev = process([tuple(e) for e in ev_pairs[int(ev_ptr[col]):int(ev_ptr[col + 1])]], int(min_len[k, c]), int(max_gap[k, c]),
                     order)
        counts.append(len(ev))
        rows += ev
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def _runs(binary):
    """The 1-runs of a 0/1 vector as (on, off) by scipy.ndimage.label (1-D: face connectivity)."""
    from scipy import ndimage
    lab, n = ndimage.label(binary)
    return [(int(np.flatnonzero(lab == k)[0]), int(np.flatnonzero(lab == k)[-1]) + 1) for k in range(1, n + 1)]


def _clear_short_ones(binary, m):
    out = binary.copy()
    for on, off in _runs(binary):
        if m > 0 and off - on < m:
            out[on:off] = 0
    return out


def _fill_short_gaps(binary, g):
    """Interior 0-runs of at most g frames become 1 (the 0-runs that touch either end of the vector are no gaps)."""
    out = binary.copy()
    for on, off in _runs(1 - binary):
        if on > 0 and off < len(binary) and off - on <= g:
            out[on:off] = 1
    return out


def process_raster(events, m, g, order, length):
    """The frame-domain statement on `length` frames; equals `process` when every gap of `events` is at least 1 frame."""
    binary = np.zeros(length, dtype=np.uint8)
    for on, off in events:
        binary[on:off] = 1
    if order == 0:
        binary = _fill_short_gaps(_clear_short_ones(binary, m), g)
    else:
        binary = _clear_short_ones(_fill_short_gaps(binary, g), m)
    return _runs(binary)


def process_table_fast(ev_ptr, ev_pairs, n_rec, NC, min_len, max_gap, order):
    """`process_table` without a Python loop over events (numpy over the whole flat array), for tables too large for the loops
    and for the host route of tools/long_bench.py; pinned to `process_table` by the tests."""
    ev_ptr = np.asarray(ev_ptr, dtype=np.int64)
    n_cols, n = len(ev_ptr) - 1, int(ev_ptr[-1])
    K = n_cols // (n_rec * NC)
    per_col = np.diff(ev_ptr)
    col = np.repeat(np.arange(n_cols), per_col)
    par = (col // (n_rec * NC)) * NC + col % NC
    m, g = np.asarray(min_len, np.int64).reshape(K * NC)[par], np.asarray(max_gap, np.int64).reshape(K * NC)[par]
    on, off = ev_pairs[:n, 0].astype(np.int64), ev_pairs[:n, 1].astype(np.int64)

    def merged(on, off, col, g):
        head = np.ones(len(on), bool)
        head[1:] = (col[1:] != col[:-1]) | (on[1:] - off[:-1] > g[1:])
        tail = np.r_[head[1:], True] if len(on) else head
        return on[head], off[tail], col[head]

    if order == 0:
        keep = (m <= 0) | (off - on >= m)
        on, off, col = merged(on[keep], off[keep], col[keep], g[keep])
    else:
        on, off, col = merged(on, off, col, g)
        m_head = np.asarray(min_len, np.int64).reshape(K * NC)[(col // (n_rec * NC)) * NC + col % NC]
        keep = (m_head <= 0) | (off - on >= m_head)
        on, off, col = on[keep], off[keep], col[keep]
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int64)
    return out_ptr, np.stack([on, off], 1).astype(np.int32).reshape(-1, 2)
