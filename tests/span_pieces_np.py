"""TEST INFRASTRUCTURE ONLY - plain-loop statement of the span tags of PIECES (include/dcase_sed.h:
sed_stitch_piece_span_tags, sed_stitch_piece_span_tags_backward).  A "recording" of the tables is a piece: it owns the windows
rec_win0[r] .. rec_win0[r + 1], the local frames 0 .. L3_r from rec_frame0 and n_r = rec_span0[r + 1] - rec_span0[r] spans;
span k covers the local frames [off_r + k * span3, min(off_r + (k + 1) * span3, L3_r)), off_r = rec_span_off[r]; a frame below
off_r or from off_r + n_r * span3 on belongs to no span.  Everything else is tests/span_tags_np.py and
tests/span_tags_bwd_np.py: the blends are tests/stitch_np.blend over the piece's tables, the sums math.fsum, the backward the
same float64 operations with the row looked up through the offset.  Independent of how the kernels tile the work, and of
longrec.span_pieces: ``pieces_of`` below restates the plan's rule with its own loops for the tests that need some pieces."""
import numpy as np

from tests import span_tags_np, stitch_np
from tests.span_tags_bwd_np import _cover, _w


def cover_lo(u, T3, hop3):
    """The first window j with 0 <= u - j * hop3 < T3."""
    j = 0
    while u - j * hop3 >= T3:
        j += 1
    return j


def cover_hi(u, n_w, hop3):
    """The last window j < n_w with u - j * hop3 >= 0."""
    j = n_w - 1
    while u - j * hop3 < 0:
        j -= 1
    return j


def n_windows(L3, T3, hop3):
    return 1 if L3 <= T3 else 1 + -(-(L3 - T3) // hop3)


def pieces_of(n_w, L3, T3, hop3, span3, max_windows):
    """The pieces of ONE recording that has more than max_windows windows, greedily over its spans:
    [(s0, s1, j0, j1, off, L3')], spans s0 .. s1 - 1, windows j0 .. j1 inclusive.  None where a span alone does not fit."""
    n_spans = -(-L3 // span3)
    out, s0 = [], 0
    while s0 < n_spans:
        j0 = cover_lo(s0 * span3, T3, hop3)
        s1, j1 = s0, None
        while s1 < n_spans:
            hi = cover_hi(min((s1 + 1) * span3, L3) - 1, n_w, hop3)
            if hi - j0 + 1 > max_windows:
                break
            s1, j1 = s1 + 1, hi
        if j1 is None:
            return None
        out.append((s0, s1, j0, j1, s0 * span3 - j0 * hop3, min(L3, j1 * hop3 + T3) - j0 * hop3))
        s0 = s1
    return out


def span_frames(rec_frame0, rec_span0, rec_span_off, span3, r, k):
    """Local frames [u0, u1) of span k of piece r."""
    L3 = int(rec_frame0[r + 1] - rec_frame0[r])
    u0 = int(rec_span_off[r]) + k * span3
    return u0, min(u0 + span3, L3)


def pool(win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3):
    """Window tensors [n_win, T3, NC] float32 of the pieces -> (tags [total_spans, NC] float32, sums [total_spans, NC, 2]
    float64 (num, den)), the sums exactly rounded: the pieces' blended timelines from local frame off_r to the end of the last
    span, pooled by tests/span_tags_np.pool_timelines as a recording of that length."""
    P = stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting)
    tags, sums = [], []
    for r in range(len(rec_win0) - 1):
        n = int(rec_span0[r + 1] - rec_span0[r])
        u0, _ = span_frames(rec_frame0, rec_span0, rec_span_off, span3, r, 0)
        _, u1 = span_frames(rec_frame0, rec_span0, rec_span_off, span3, r, n - 1)
        assert n >= 1 and 0 <= u0 and u0 + (n - 1) * span3 < u1
        f0 = int(rec_frame0[r])
        t, s, span0 = span_tags_np.pool_timelines(P[f0 + u0:f0 + u1], A[f0 + u0:f0 + u1], np.array([0, u1 - u0], np.int64), span3)
        assert int(span0[-1]) == n
        tags.append(t)
        sums.append(s)
    return np.concatenate(tags), np.concatenate(sums)


def frame_row(rec_span0, rec_span_off, span3, r, u):
    """The row of g / sums that local frame u of piece r reads, or -1: the frame belongs to no span."""
    k = u - int(rec_span_off[r])
    if k < 0 or k // span3 >= int(rec_span0[r + 1] - rec_span0[r]):
        return -1
    return int(rec_span0[r]) + k // span3


def backward(win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3, g_tags, sums=None):
    """-> (d_win_strong, d_win_att) float32 [n_win, T3, NC]: tests/span_tags_bwd_np.backward's operations with the row of
    ``frame_row``; a frame without a row, like the tails, leaves +0.0.  ``sums``: the forward's, or None for ``pool``'s."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float32), np.asarray(win_att, dtype=np.float32)
    _, T3, NC = win_strong.shape
    P = stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting)
    if sums is None:
        _, sums = pool(win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3)
    sums, g_tags = np.asarray(sums, dtype=np.float64), np.asarray(g_tags, dtype=np.float32)
    ds, da = np.zeros(win_strong.shape, dtype=np.float32), np.zeros(win_strong.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(len(rec_win0) - 1):
            w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
            f0, L3 = int(rec_frame0[r]), int(rec_frame0[r + 1] - rec_frame0[r])
            for u in range(L3):
                row = frame_row(rec_span0, rec_span_off, span3, r, u)
                if row < 0:
                    continue
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


def frame_rows(rec_win0, rec_frame0, rec_span0, rec_span_off, T3, hop3, weighting, span3):
    """Per window element (j, v): ``row`` int64 [n_win, T3] (-1: the tails and the frames of no span) and ``share`` = w / W."""
    n_win = int(rec_win0[-1])
    row, share = np.full((n_win, T3), -1, dtype=np.int64), np.zeros((n_win, T3))
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        for u in range(int(rec_frame0[r + 1] - rec_frame0[r])):
            g = frame_row(rec_span0, rec_span_off, span3, r, u)
            if g < 0:
                continue
            cover = _cover(u, nw, T3, hop3)
            W = sum(_w(u - j * hop3, T3, weighting) for j in cover)
            for j in cover:
                row[w0 + j, u - j * hop3] = g
                share[w0 + j, u - j * hop3] = _w(u - j * hop3, T3, weighting) / W
    return row, share


def forward64(win_strong, win_att, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3):
    """tags [total_spans, NC] float64 of float64 window tensors, every operation in float64 (tests/span_tags_bwd_np.forward64
    with the row of ``frame_row``)."""
    win_strong, win_att = np.asarray(win_strong, dtype=np.float64), np.asarray(win_att, dtype=np.float64)
    _, T3, NC = win_strong.shape
    num, den = np.zeros((int(rec_span0[-1]), NC)), np.zeros((int(rec_span0[-1]), NC))
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        for u in range(int(rec_frame0[r + 1] - rec_frame0[r])):
            row = frame_row(rec_span0, rec_span_off, span3, r, u)
            if row < 0:
                continue
            cover = _cover(u, nw, T3, hop3)
            ws = [_w(u - j * hop3, T3, weighting) for j in cover]
            if len(cover) == 1:
                p, a = win_strong[w0 + cover[0], u - cover[0] * hop3], win_att[w0 + cover[0], u - cover[0] * hop3]
            else:
                p = sum(w * win_strong[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
                a = sum(w * win_att[w0 + j, u - j * hop3] for j, w in zip(cover, ws)) / sum(ws)
            num[row] += p * a
            den[row] += a
    return num / den


def piece_tables(piece):
    """The one-piece tables of (s0, s1, j0, j1, off, L3'): (rec_win0, rec_frame0, rec_span0, rec_span_off)."""
    s0, s1, j0, j1, off, L3p = piece
    return (np.array([0, j1 - j0 + 1], np.int32), np.array([0, L3p], np.int64), np.array([0, s1 - s0], np.int64),
            np.array([off], np.int32))
