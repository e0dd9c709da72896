"""A plain-loop numpy float32 statement of the batch-augmentation definitions (include/dcase_sed.h, sed_batch_augment),
independent of the product code: the oracle of tests/test_gpu_augment.py.

Table row of clip b: {partner, lambda_bits, shift_x, shift_y, f0, fw, t0, tw} (int32; lambda_bits = bits of an fp32)."""
import numpy as np


def _r(s, n):
    return ((int(s) % n) + n) % n                  # Python's % is already non-negative for n > 0; written as the definition


def _mix(A, table, shift_col):
    """lambda (x) own rolled clip (+) (1 - lambda) (x) partner's rolled clip, every operation rounded to float32; the
    partner is not touched when it is the clip itself or lambda == 1."""
    A = np.asarray(A, dtype=np.float32)
    B, n, w = A.shape
    out = np.empty_like(A)
    one = np.float32(1.0)
    for b in range(B):
        p = min(max(int(table[b, 0]), 0), B - 1)
        lam = np.array([table[b, 1]], dtype=np.int32).view(np.float32)[0]
        s_own, s_oth = int(table[b, shift_col]), int(table[p, shift_col])
        for t in range(n):
            own = A[b, _r(t - s_own, n)]
            if p == b or lam == one:
                out[b, t] = own
                continue
            oth = A[p, _r(t - s_oth, n)]
            om = np.float32(one - lam)
            for m in range(w):
                out[b, t, m] = np.float32(np.float32(lam * own[m]) + np.float32(om * oth[m]))
    return out


def _features(X, table):
    X = np.asarray(X, dtype=np.float32)
    shape = X.shape
    X = X.reshape(shape[0], shape[-2], shape[-1])
    B, T, M = X.shape
    out = _mix(X, table, 2)
    for b in range(B):
        f0, fw, t0, tw = (int(v) for v in table[b, 4:8])
        for t in range(T):
            for m in range(M):
                if (fw > 0 and f0 <= m < f0 + fw) or (tw > 0 and t0 <= t < t0 + tw):
                    out[b, t, m] = np.float32(0.0)
    return out.reshape(shape)


def augment(X, Xe, G, table):
    """(X', Xe' or None, G' or None) for X [B, T, M] (or [B, 1, T, M]), Xe the same or None, G [B, T3, NC] or None."""
    table = np.asarray(table, dtype=np.int32)
    with np.errstate(all="ignore"):
        return (_features(X, table), None if Xe is None else _features(Xe, table),
                None if G is None else _mix(G, table, 3))
