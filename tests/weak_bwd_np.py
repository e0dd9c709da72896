"""TEST INFRASTRUCTURE ONLY - plain-loop float64 statement of sed_stitch_weak_backward's definition (include/dcase_sed.h):
the gradient of a loss on the recording-level weak tags w.r.t. the windows' posteriors and attention.  P and A are the float32
blends of tests/stitch_np.blend, (num, den) the pooled sums (tests/weak_np.pool_timelines, or the ones a caller hands in), and
per (recording r, class c, window j, local frame v), u = j * hop3 + v < L3_r:
    t = num / den;  dP = (g * A[u, c]) / den;  dA = (g * (P[u, c] - t)) / den
    d_win_strong[j, v, c] = float32((dP * w) / W),  d_win_att[j, v, c] = float32((dA * w) / W)
every operation one float64 operation, w the window's weight at v and W the integer sum of the weights of the windows that
cover u; everything else is +0.0.  Independent of how the kernel tiles the work.  ``forward64`` is the same pooling with every
operation in float64 (no float32 rounding of the blend): the function whose finite differences the statement is checked
against."""
import numpy as np

from tests import stitch_np, weak_np


def _cover(u, nw, T3, hop3):
    return [j for j in range(nw) if 0 <= u - j * hop3 < T3]


def _w(v, T3, weighting):
    return 1 if weighting == 0 else min(v + 1, T3 - v)


def backward(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting, g_weak, sums=None):
    """-> (d_win_strong, d_win_att) float32 [n_win, T3, NC].  ``sums`` [n_rec, NC, 2] float64 (num, den): the forward's, or
    None for the fsum values of tests/weak_np."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float32), np.asarray(win_att, dtype=np.float32)
    _, T3, NC = win_strong.shape
    P = stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting)
    if sums is None:
        _, sums = weak_np.pool_timelines(P, A, rec_frame0)
    sums, g_weak = np.asarray(sums, dtype=np.float64), np.asarray(g_weak, dtype=np.float32)
    ds, da = np.zeros(win_strong.shape, dtype=np.float32), np.zeros(win_strong.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(len(rec_win0) - 1):
            w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
            f0, L3 = int(rec_frame0[r]), int(rec_frame0[r + 1] - rec_frame0[r])
            g = g_weak[r].astype(np.float64)
            num, den = sums[r, :, 0], sums[r, :, 1]
            t = num / den
            for u in range(L3):
                cover = _cover(u, nw, T3, hop3)
                W = np.float64(sum(_w(u - j * hop3, T3, weighting) for j in cover))
                dP = (g * A[f0 + u].astype(np.float64)) / den
                dA = (g * (P[f0 + u].astype(np.float64) - t)) / den
                for j in cover:
                    v = u - j * hop3
                    w = np.float64(_w(v, T3, weighting))
                    ds[w0 + j, v] = ((dP * w) / W).astype(np.float32)
                    da[w0 + j, v] = ((dA * w) / W).astype(np.float32)
    return ds, da


def forward64(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting):
    """weak [n_rec, NC] float64 of float64 window tensors, every operation in float64 (one covering window: its value)."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float64), np.asarray(win_att, dtype=np.float64)
    _, T3, NC = win_strong.shape
    weak = np.empty((len(rec_win0) - 1, NC), dtype=np.float64)
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        L3 = int(rec_frame0[r + 1] - rec_frame0[r])
        num, den = np.zeros(NC), np.zeros(NC)
        for u in range(L3):
            cover = _cover(u, nw, T3, hop3)
            ws = [_w(u - j * hop3, T3, weighting) for j in cover]
            if len(cover) == 1:
                p, a = win_strong[w0 + cover[0], u - cover[0] * hop3], win_att[w0 + cover[0], u - cover[0] * hop3]
            else:
                p = sum(w * win_strong[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
                a = sum(w * win_att[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
            num += p * a
            den += a
        weak[r] = num / den
    return weak
