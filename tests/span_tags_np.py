"""TEST INFRASTRUCTURE ONLY - plain-loop statement of the span-level weak tags, of an event's tag score and of the tag gate
(include/dcase_sed.h).  The posteriors and the attention of the windows are blended by tests/stitch_np.blend, then pooled per
(span, class) over the span's frames with exactly rounded sums (math.fsum), as tests/weak_np.pool_timelines does per
recording.  The tag score and the gate are double loops over events and spans.  Independent of how the kernels tile the work."""
import math

import numpy as np

from tests import stitch_np
from tests.event_scores_np import column_of, event_max


def span_table(L3s, span3):
    """rec_span0 [n_rec + 1] int64: recording r has ceil(L3_r / span3) spans."""
    counts = [(int(L) + span3 - 1) // span3 for L in L3s]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def pool_timelines(P, A, rec_frame0, span3):
    """Blended timelines P, A [sum L3, NC] float32 -> (tags [total_spans, NC] float32, sums [total_spans, NC, 2] float64 (num,
    den), rec_span0): span s of recording r covers its frames s * span3 .. min((s + 1) * span3, L3_r) - 1."""
    P, A = np.asarray(P, dtype=np.float32), np.asarray(A, dtype=np.float32)
    n_rec, NC = len(rec_frame0) - 1, P.shape[1]
    rec_span0 = span_table(np.diff(np.asarray(rec_frame0, dtype=np.int64)), span3)
    tags = np.empty((int(rec_span0[-1]), NC), dtype=np.float32)
    sums = np.empty((int(rec_span0[-1]), NC, 2), dtype=np.float64)
    for r in range(n_rec):
        f0, f1 = int(rec_frame0[r]), int(rec_frame0[r + 1])
        for s in range(int(rec_span0[r + 1] - rec_span0[r])):
            u0, u1 = f0 + s * span3, min(f0 + (s + 1) * span3, f1)
            g = int(rec_span0[r]) + s
            for c in range(NC):
                num = math.fsum(float(P[u, c]) * float(A[u, c]) for u in range(u0, u1))
                den = math.fsum(float(A[u, c]) for u in range(u0, u1))
                sums[g, c] = num, den
                with np.errstate(invalid="ignore", divide="ignore"):
                    tags[g, c] = np.float32(np.float64(num) / np.float64(den))
    return tags, sums, rec_span0


def pool(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting, span3):
    """Window posteriors and attention [n_win, T3, NC] float32 -> (tags, sums, rec_span0) as pool_timelines."""
    P = stitch_np.blend(win_strong, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(win_att, rec_win0, rec_frame0, hop3, weighting)
    return pool_timelines(P, A, rec_frame0, span3)


def tag_scores(tags, rec_span0, span3, n_rec, NC, ev_ptr, ev_pairs):
    """tag_score float32 [ev_ptr[-1]]: per event [on, off) of column (k, rec, c) the largest non-NaN tag of the spans
    on // span3 .. (off - 1) // span3 of its recording (the stored float32 itself), NaN when there is none.  An event outside
    0 <= on < off <= S_rec * span3 scores NaN (the kernel's err bit 64)."""
    tags = np.asarray(tags, np.float32).reshape(-1, NC)
    score = np.full(int(ev_ptr[-1]), np.nan, np.float32)
    for col in range(len(ev_ptr) - 1):
        _, rec, c = column_of(col, n_rec, NC)
        g0, n_spans = int(rec_span0[rec]), int(rec_span0[rec + 1]) - int(rec_span0[rec])
        for i in range(int(ev_ptr[col]), int(ev_ptr[col + 1])):
            on, off = int(ev_pairs[i][0]), int(ev_pairs[i][1])
            if on < 0 or on >= off or off > n_spans * span3:
                continue
            score[i] = event_max([tags[g0 + s, c] for s in range(on // span3, (off - 1) // span3 + 1)])
    return score


def gate(ev_ptr, ev_pairs, tag_score, n_rec, NC, min_tag):
    """The events with tag_score > min_tag[k][c] (strict; NaN never), column by column: (out_ptr int64 [n_cols + 1], out_pairs
    int32 [kept, 2], the kept events' tag scores float32 [kept])."""
    min_tag = np.asarray(min_tag, np.float32).reshape(-1, NC)
    counts, kept = [], []
    for col in range(len(ev_ptr) - 1):
        k, _, c = column_of(col, n_rec, NC)
        n = 0
        for i in range(int(ev_ptr[col]), int(ev_ptr[col + 1])):
            if tag_score[i] > min_tag[k, c]:
                kept.append(i)
                n += 1
        counts.append(n)
    out_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return out_ptr, np.asarray([ev_pairs[i] for i in kept], np.int32).reshape(-1, 2), \
        np.asarray([tag_score[i] for i in kept], np.float32)


def mask_then_decode(timeline, rec_frame0, tags, rec_span0, span3, min_tag, thr, win):
    """What the gate is NOT: the posteriors of every span whose tag does not exceed min_tag[c] set to 0, then decoded
    (stitch_np.decode).  For the header's hand example of the difference."""
    timeline = np.array(timeline, dtype=np.float32)
    for r in range(len(rec_frame0) - 1):
        f0, f1 = int(rec_frame0[r]), int(rec_frame0[r + 1])
        for s in range(int(rec_span0[r + 1] - rec_span0[r])):
            for c in range(timeline.shape[1]):
                if not tags[int(rec_span0[r]) + s, c] > min_tag[c]:
                    timeline[f0 + s * span3:min(f0 + (s + 1) * span3, f1), c] = 0.0
    return stitch_np.decode(timeline, rec_frame0, thr, win)
