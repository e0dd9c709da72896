"""The plain-loop statement of sed_events_rasterize (include/dcase_sed.h): for every class, recording and event of the
selected column, ``for u in range(on, off)``.  Values and old contents are handled as fp32 numpy scalars and stored as they
are, so NaN payloads, -0.0f and denormals pass through; the only arithmetic is the comparison ``v > old`` of the maximum.

``rasterize`` returns ``(dst, err, unspecified)``: the destination after the call, the error word as a function of the
inputs, and a boolean mask of the elements whose content the definition leaves open (the rows of a column that holds a bad
event).  Everything outside the addressed rows, and every column / class / recording the definition rejects, comes back as
it went in."""
import numpy as np

REPLACE, MAXIMUM = 0, 1


def column_errors(events, L3):
    """True when the events [(on, off), ...] of one column are not valid for a recording of L3 rows (err bit 64)."""
    prev_off = None
    for on, off in events:
        on, off = int(on), int(off)
        if on < 0 or on >= off or off > L3:
            return True
        if prev_off is not None and on < prev_off:
            return True
        prev_off = off
    return False


def rasterize(ev_ptr, ev_pairs, rec_frame0, n_rec, NC, dst, dst_row0=None, value=None, point=None, combine=REPLACE, n_points=1):
    ev_ptr = np.asarray(ev_ptr, dtype=np.int64)
    ev_pairs = np.asarray(ev_pairs, dtype=np.int64).reshape(-1, 2)
    f0 = np.asarray(rec_frame0, dtype=np.int64)
    out = np.array(dst, dtype=np.float32, copy=True).reshape(-1, NC)
    bits = out.view(np.uint32)
    dst_rows, cap = out.shape[0], ev_pairs.shape[0]
    unspecified = np.zeros(out.shape, dtype=bool)
    vbits = None if value is None else np.ascontiguousarray(value, dtype=np.float32).view(np.uint32)
    one = np.array([1.0], dtype=np.float32).view(np.uint32)[0]
    pts = np.zeros(NC, dtype=np.int64) if point is None else np.asarray(point, dtype=np.int64).reshape(NC)
    n_cols = n_points * n_rec * NC
    assert ev_ptr.size == n_cols + 1 and f0.size == n_rec + 1
    err = 0
    col_ok = np.zeros(n_cols, dtype=bool)
    for col in range(n_cols):
        a, b = int(ev_ptr[col]), int(ev_ptr[col + 1])
        col_ok[col] = 0 <= a <= b <= cap
        if not col_ok[col]:
            err |= 16
    frames_ok, rows_ok, row0 = [], [], []
    for r in range(n_rec):
        fa, fb = int(f0[r]), int(f0[r + 1])
        ok = 0 <= fa <= fb <= dst_rows
        d0 = fa if dst_row0 is None else int(dst_row0[r])
        ok_d = ok and d0 >= 0 and d0 + (fb - fa) <= dst_rows
        if not ok_d:
            err |= 16
        frames_ok.append(ok)
        rows_ok.append(ok_d)
        row0.append(d0)
    for c in range(NC):
        k = int(pts[c])
        if not 0 <= k < n_points:
            err |= 8
            continue
        for r in range(n_rec):
            col = (k * n_rec + r) * NC + c
            if not frames_ok[r] or not col_ok[col]:
                continue
            L3 = int(f0[r + 1] - f0[r])
            a, b = int(ev_ptr[col]), int(ev_ptr[col + 1])
            bad = column_errors(ev_pairs[a:b], L3)
            if bad:
                err |= 64
            if not rows_ok[r]:
                continue
            d0 = row0[r]
            if bad:
                unspecified[d0:d0 + L3, c] = True
                continue
            if combine == REPLACE:
                bits[d0:d0 + L3, c] = 0                                      # +0.0f in every row of the recording
            for i in range(a, b):
                v = one if vbits is None else vbits[i]
                vf = np.array([v], dtype=np.uint32).view(np.float32)[0]
                for u in range(int(ev_pairs[i, 0]), int(ev_pairs[i, 1])):
                    if combine == REPLACE or vf > out[d0 + u, c]:
                        bits[d0 + u, c] = v
    return out, err, unspecified


def table(cols, pad=0, fill=-7):
    """Columns (lists of (on, off)) as ``ev_ptr`` int64 and ``ev_pairs`` int32 [events + pad, 2] with ``pad`` rows of ``fill``."""
    ptr = np.r_[0, np.cumsum([len(c) for c in cols])].astype(np.int64)
    rows = [e for c in cols for e in c] + [(fill, fill)] * pad
    return ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
