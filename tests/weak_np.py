"""TEST INFRASTRUCTURE ONLY - plain-loop statement of sed_stitch_weak's definition (include/dcase_sed.h): the recording-level
weak tags of long recordings.  The posteriors and the attention of the windows are blended by tests/stitch_np.blend (the
float32 statement of the blend), then pooled per (recording, class) over the recording's whole timeline:
num = sum_u P[u, c] * A[u, c], den = sum_u A[u, c], both exactly rounded sums (math.fsum) of float64 values - a product of two
float32 values is exact in float64 -, weak = float32(num / den).  Independent of how the kernel tiles the work."""
import math

import numpy as np

from tests import stitch_np


def pool_timelines(P, A, rec_frame0):
    """Blended timelines P, A [sum L3, NC] float32 -> (weak [n_rec, NC] float32, sums [n_rec, NC, 2] float64 (num, den))."""
    P, A = np.asarray(P, dtype=np.float32), np.asarray(A, dtype=np.float32)
    n_rec, NC = len(rec_frame0) - 1, P.shape[1]
    weak = np.empty((n_rec, NC), dtype=np.float32)
    sums = np.empty((n_rec, NC, 2), dtype=np.float64)
    for r in range(n_rec):
        f0, f1 = int(rec_frame0[r]), int(rec_frame0[r + 1])
        for c in range(NC):
            num = math.fsum(float(P[u, c]) * float(A[u, c]) for u in range(f0, f1))
            den = math.fsum(float(A[u, c]) for u in range(f0, f1))
            sums[r, c] = num, den
            with np.errstate(invalid="ignore", divide="ignore"):
                weak[r, c] = np.float32(np.float64(num) / np.float64(den))
    return weak, sums


def pool(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting):
    """Window posteriors and attention [n_win, T3, NC] float32 -> (weak, sums) as pool_timelines."""
    P = stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting)
    return pool_timelines(P, A, rec_frame0)


def attention(rs, n_win, T3, NC):
    """A clamped class-softmax [n_win, T3, NC] float32 of random logits as the heads produce it: wide logits, so that some
    entries sit at the 1e-7 clamp and (NC > 1) some frames put all their mass, 1.0, on one class."""
    logits = rs.standard_normal((n_win, T3, NC)) * 8.0
    hot = rs.uniform(size=(n_win, T3)) < 0.1
    logits[hot, rs.randint(0, NC, size=int(hot.sum()))] += 60.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return np.clip((e / e.sum(-1, keepdims=True)).astype(np.float32), np.float32(1e-7), np.float32(1.0))
