"""TEST INFRASTRUCTURE ONLY - plain-loop numpy float32 statement of sed_stitch_decode's definitions (include/dcase_sed.h):
the blend of overlapping windows' posteriors into one timeline per recording, and the reference decode of that timeline
(oracle.postprocess_np: scipy's median filter + the restated dcase_util run-length decode, which have no length limit).
Written frame by frame, independent of how the kernel tiles the work."""
import numpy as np

from oracle import postprocess_np as pp


def weight(v, T3, weighting):
    """0: uniform, 1: taper min(v + 1, T3 - v); an integer held as float32."""
    return np.float32(1.0) if weighting == 0 else np.float32(min(v + 1, T3 - v))


def blend(win_strong, rec_win0, rec_frame0, hop3, weighting):
    """win_strong [n_win, T3, NC] float32 -> timeline [sum L3, NC] float32.  Frame u of a recording is covered by its windows
    j with 0 <= u - j * hop3 < T3, in increasing j; one covering window: its value copied; otherwise the sequential float32
    sum of w * p from 0.0, divided by the (exact) weight sum - every operation rounded to float32 on its own."""
    win_strong = np.asarray(win_strong, dtype=np.float32)
    _, T3, NC = win_strong.shape
    out = np.full((int(rec_frame0[-1]), NC), np.nan, dtype=np.float32)
    for r in range(len(rec_win0) - 1):
        w0, nw = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r])
        f0, L3 = int(rec_frame0[r]), int(rec_frame0[r + 1] - rec_frame0[r])
        starts = np.arange(nw) * hop3
        for u in range(L3):
            cover = [int(j) for j in np.flatnonzero((starts <= u) & (u - starts < T3))]
            assert cover, f"recording {r}: frame {u} is covered by no window"
            for c in range(NC):
                if len(cover) == 1:
                    j = cover[0]
                    out[f0 + u, c] = win_strong[w0 + j, u - j * hop3, c]
                    continue
                num, den = np.float32(0.0), np.float32(0.0)
                for j in cover:
                    v = u - j * hop3
                    w = weight(v, T3, weighting)
                    num = np.float32(num + np.float32(w * win_strong[w0 + j, v, c]))
                    den = np.float32(den + w)
                out[f0 + u, c] = np.float32(num / den)
    return out


def decode(timeline, rec_frame0, thr, win):
    """Reference decode of every (recording, class) column of the whole timeline: (binary [sum L3, NC] uint8,
    ev_ptr [n_rec * NC + 1] int64, ev_pairs [n_events, 2] int32)."""
    timeline = np.asarray(timeline, dtype=np.float32)
    NC = timeline.shape[1]
    binary = np.zeros(timeline.shape, dtype=np.uint8)
    counts, pairs = [], []
    for r in range(len(rec_frame0) - 1):
        seg = timeline[int(rec_frame0[r]):int(rec_frame0[r + 1])]
        for c in range(NC):
            col = pp.filter_decisions(seg[:, c:c + 1], np.float32(thr[c]), int(win[c]))[:, 0]
            binary[int(rec_frame0[r]):int(rec_frame0[r + 1]), c] = col
            regions = pp.DecisionEncoder().find_contiguous_regions(col)
            counts.append(len(regions))
            pairs.append(np.asarray(regions, dtype=np.int32).reshape(-1, 2))
    ev_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return binary, ev_ptr, np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int32)
