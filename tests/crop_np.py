"""The plain-loop statement of event-aware crop sampling (include/dcase_sed.h): activity counted row by row,
running sums, Python integers throughout.  Nothing here is vectorised on purpose: the device's scan and bisection are pinned
to this, exactly."""
import numpy as np


def active(x):
    """label > 0: False for NaN, -0.0, 0.0 and negatives."""
    return bool(float(x) > 0.0)


def prefix_tables(label, nclass):
    """``label`` [R, nclass] -> (A, B), each a list of R + 1 rows of nclass ints: A[x][c] the active rows of class c before
    row x, B[x][c] the sum of A[0 .. x - 1][c]."""
    R = len(label)
    A = [[0] * nclass for _ in range(R + 1)]
    B = [[0] * nclass for _ in range(R + 1)]
    for c in range(nclass):
        a = b = 0
        for x in range(R + 1):
            A[x][c], B[x][c] = a, b
            b += a
            if x < R and active(label[x][c]):
                a += 1
    return A, B


def window_activity(label, nclass, T3, hi):
    """a[c][s] for s in [0, hi]: the active rows of class c in [s, min(s + T3, R)) - a triple loop."""
    R = len(label)
    a = [[0] * (hi + 1) for _ in range(nclass)]
    for c in range(nclass):
        act = [active(label[x][c]) for x in range(R)]
        for s in range(hi + 1):
            n = 0
            for x in range(s, min(s + T3, R)):
                if act[x]:
                    n += 1
            a[c][s] = n
    return a


def cumulative(a):
    """C[c][s] = a[c][0] + ... + a[c][s]."""
    C = []
    for row in a:
        run, out = 0, []
        for n in row:
            run += n
            out.append(run)
        C.append(out)
    return C


def item_weights(label, nclass, T3, hi):
    """(C, W, mask) of one item: W[c] = C[c][hi], bit c of mask set when W[c] > 0."""
    C = cumulative(window_activity(label, nclass, T3, hi))
    W = [C[c][hi] for c in range(nclass)]
    mask = 0
    for c in range(nclass):
        if W[c] > 0:
            mask |= 1 << c
    return C, W, mask


def draws(seed, epoch, n_slots, event_fraction):
    rng = np.random.default_rng([seed, epoch])
    u = rng.integers(0, 2 ** 64, n_slots, dtype=np.uint64)
    v = rng.integers(0, 2 ** 31, n_slots)
    m = rng.random(n_slots) < event_fraction
    return u, v, m


def slot_start(C, W, hi, windowed, u, v, m):
    """(start, chosen class) of one slot of an item with the tables ``C`` / ``W`` of ``item_weights``."""
    u, v = int(u), int(v)
    if not windowed:
        return 0, -1
    present = [c for c in range(len(W)) if W[c] > 0]
    if not m or not present:
        return (u * (hi + 1)) >> 64, -1
    c = present[v % len(present)]
    target = (u * W[c]) >> 64
    for s in range(hi + 1):
        if C[c][s] > target:
            return s, c
    raise AssertionError("target below W has a start")


def starts(labels, nclass, T3, his, windowed, slot_item, u, v, m):
    """Every slot's (start, class) as int64 arrays, plus the per-item (W [n_items, nclass], mask [n_items]).  ``his[i]`` is
    the item's start_hi; an item of a non-windowed stream is weighed at hi = 0."""
    tables = [item_weights(lab, nclass, T3, int(hi) if w else 0) for lab, hi, w in zip(labels, his, windowed)]
    out = [slot_start(tables[i][0], tables[i][1], int(his[i]) if windowed[i] else 0, windowed[i], u[j], v[j], m[j])
           for j, i in enumerate(slot_item)]
    W = np.array([t[1] for t in tables], dtype=np.int64).reshape(len(labels), nclass)
    mask = np.array([t[2] for t in tables], dtype=np.uint32)
    return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.int64), W, mask


def set_starts(ws, epoch, labels=None):
    """The statement on a ``WindowedFeatureSet``: its slots, its draws' definition restated, ``labels`` (default: the
    timelines its label pool holds now, read back) -> (start, class, W, mask)."""
    if labels is None:
        pool = ws.label_pool.cpu().numpy()
        labels = [pool[o:o + r] for o, r in zip(ws.label_offset_host, ws.label_rows_host)]
    u, v, m = draws(ws.seed, int(epoch), len(ws.slot_item), ws.event_fraction)
    return starts(labels, ws.nclass, ws.T3, ws.start_hi_host, [bool(w) for w in ws.item_windowed], ws.slot_item, u, v, m)
