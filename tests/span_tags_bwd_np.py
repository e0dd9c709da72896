"""TEST INFRASTRUCTURE ONLY - plain-loop float64 statement of sed_stitch_span_tags_backward's definition
(include/dcase_sed.h): the gradient of a loss on the span-level weak tags w.r.t. the windows' posteriors and attention.  It is
tests/weak_bwd_np.backward with ONE change: timeline frame u of recording r takes g, num and den from row
rec_span0[r] + u // span3, not from row r.  P and A are the float32 blends of tests/stitch_np.blend, (num, den) the pooled sums
per span (tests/span_tags_np.pool_timelines, or the ones a caller hands in), and per (recording r, class c, window j, local
frame v), u = j * hop3 + v < L3_r:
    t = num / den;  dP = (g * A[u, c]) / den;  dA = (g * (P[u, c] - t)) / den
    d_win_strong[j, v, c] = float32((dP * w) / W),  d_win_att[j, v, c] = float32((dA * w) / W)
every operation one float64 operation; everything else is +0.0.  Independent of how the kernel tiles the work.  ``forward64``
is the same pooling per span with every operation in float64: the function whose finite differences the statement is checked
against."""
import numpy as np

from tests import span_tags_np, stitch_np
from tests.weak_bwd_np import _cover, _w


def backward(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting, span3, g_tags, sums=None, rec_span0=None, blends=None):
    """-> (d_win_strong, d_win_att) float32 [n_win, T3, NC].  ``sums`` [total_spans, NC, 2] float64 (num, den): the forward's,
    or None for the fsum values of tests/span_tags_np; ``rec_span0``: the span offsets, or None for span_tags_np.span_table;
    ``blends``: (P, A) of stitch_np.blend where the caller has them already."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float32), np.asarray(win_att, dtype=np.float32)
    _, T3, NC = win_strong.shape
    if blends is None:
        blends = (stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting),
                  stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting))
    P, A = blends
    if sums is None:
        _, sums, _ = span_tags_np.pool_timelines(P, A, rec_frame0, span3)
    if rec_span0 is None:
        rec_span0 = span_tags_np.span_table(np.diff(np.asarray(rec_frame0, dtype=np.int64)), span3)
    sums, g_tags = np.asarray(sums, dtype=np.float64), np.asarray(g_tags, dtype=np.float32)
    ds, da = np.zeros(win_strong.shape, dtype=np.float32), np.zeros(win_strong.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(len(rec_win0) - 1):
            w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
            f0, L3 = int(rec_frame0[r]), int(rec_frame0[r + 1] - rec_frame0[r])
            for u in range(L3):
                row = int(rec_span0[r]) + u // span3
                g = g_tags[row].astype(np.float64)
                num, den = sums[row, :, 0], sums[row, :, 1]
                t = num / den
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


def frame_rows(rec_win0, rec_frame0, T3, hop3, weighting, span3, rec_span0=None):
    """Per window element (j, v): ``row`` int64 [n_win, T3] - the span row its timeline frame reads, -1 in the tails - and
    ``share`` float64 [n_win, T3] = w / W (0 in the tails).  What the finite-difference bound is built from."""
    if rec_span0 is None:
        rec_span0 = span_tags_np.span_table(np.diff(np.asarray(rec_frame0, dtype=np.int64)), span3)
    n_win = int(rec_win0[-1])
    row, share = np.full((n_win, T3), -1, dtype=np.int64), np.zeros((n_win, T3))
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        L3 = int(rec_frame0[r + 1] - rec_frame0[r])
        for u in range(L3):
            cover = _cover(u, nw, T3, hop3)
            W = sum(_w(u - j * hop3, T3, weighting) for j in cover)
            for j in cover:
                row[w0 + j, u - j * hop3] = int(rec_span0[r]) + u // span3
                share[w0 + j, u - j * hop3] = _w(u - j * hop3, T3, weighting) / W
    return row, share


def forward64(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting, span3):
    """tags [total_spans, NC] float64 of float64 window tensors, every operation in float64 (one covering window: its value)."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float64), np.asarray(win_att, dtype=np.float64)
    _, T3, NC = win_strong.shape
    rec_span0 = span_tags_np.span_table(np.diff(np.asarray(rec_frame0, dtype=np.int64)), span3)
    num, den = np.zeros((int(rec_span0[-1]), NC)), np.zeros((int(rec_span0[-1]), NC))
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        L3 = int(rec_frame0[r + 1] - rec_frame0[r])
        for u in range(L3):
            cover = _cover(u, nw, T3, hop3)
            ws = [_w(u - j * hop3, T3, weighting) for j in cover]
            if len(cover) == 1:
                p, a = win_strong[w0 + cover[0], u - cover[0] * hop3], win_att[w0 + cover[0], u - cover[0] * hop3]
            else:
                p = sum(w * win_strong[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
                a = sum(w * win_att[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
            row = int(rec_span0[r]) + u // span3
            num[row] += p * a
            den[row] += a
    return num / den
