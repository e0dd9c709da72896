"""CPU checks of the span-level weak tags and the tag gate: the numpy statement (tests/span_tags_np.py) against the
recording-level statement and on hand cases, ``inference.span_table``, the span-tag table and the argument errors that must be
raised before any forward.  The kernels are pinned against the same statement in tests/test_gpu_span_tags.py."""
import math

import numpy as np
import pytest
import torch

from tests import long_score_np as ls
from tests import span_tags_np as sp
from tests import stitch_np, weak_np
from tests.long_util import _tables


def _inputs(n_win, T3, NC, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(size=(n_win, T3, NC)).astype(np.float32), weak_np.attention(rs, n_win, T3, NC)


@pytest.mark.parametrize("hop3,weighting", [(3, 0), (3, 1), (8, 1)])
def test_one_span_per_recording_is_the_recording_level_statement(hop3, weighting):
    T3, NC, L3s = 8, 3, [1, 7, 8, 9, 30]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(rec_win0[-1], T3, NC, 1)
    tags, sums, rec_span0 = sp.pool(p, a, rec_win0, rec_frame0, hop3, weighting, max(L3s))
    weak, wsums = weak_np.pool(p, a, rec_win0, rec_frame0, hop3, weighting)
    assert list(rec_span0) == list(range(len(L3s) + 1))
    assert tags.tobytes() == weak.tobytes() and sums.tobytes() == wsums.tobytes()


def test_disjoint_windows_and_window_spans_give_each_window_its_own_ratio():
    T3, NC, n_w = 8, 4, [1, 3, 2]
    n = sum(n_w)
    p, a = _inputs(n, T3, NC, 2)
    edges = np.r_[0, np.cumsum(n_w)]
    tags, sums, rec_span0 = sp.pool(p, a, edges, edges * T3, T3, 1, T3)
    assert list(rec_span0) == list(edges)
    for w in range(n):
        for c in range(NC):
            num = math.fsum(float(p[w, v, c]) * float(a[w, v, c]) for v in range(T3))
            den = math.fsum(float(a[w, v, c]) for v in range(T3))
            assert sums[w, c, 0] == num and sums[w, c, 1] == den and tags[w, c] == np.float32(num / den)


def test_the_gate_at_one_span_per_recording_is_the_clip_level_weak_mask():
    """Columns are kept whole or dropped whole, exactly where the recording-level tag exceeds min_tag."""
    T3, NC, hop3, L3s = 8, 3, 4, [20, 9, 33]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(rec_win0[-1], T3, NC, 3)
    tl = stitch_np.blend(p, rec_win0, rec_frame0, hop3, 1)
    _, ev_ptr, ev_pairs = stitch_np.decode(tl, rec_frame0, [0.5] * NC, [1] * NC)
    assert (np.diff(ev_ptr) > 0).all()
    span3 = max(L3s)
    tags, _, rec_span0 = sp.pool(p, a, rec_win0, rec_frame0, hop3, 1, span3)
    weak, _ = weak_np.pool(p, a, rec_win0, rec_frame0, hop3, 1)
    min_tag = np.median(weak, axis=0).astype(np.float32)
    score = sp.tag_scores(tags, rec_span0, span3, len(L3s), NC, ev_ptr, ev_pairs)
    out_ptr, out_pairs, kept = sp.gate(ev_ptr, ev_pairs, score, len(L3s), NC, min_tag)
    keep_col = (weak > min_tag[None, :]).reshape(-1)
    assert keep_col.any() and not keep_col.all()
    np.testing.assert_array_equal(np.diff(out_ptr), np.where(keep_col, np.diff(ev_ptr), 0))
    want = np.concatenate([ev_pairs[ev_ptr[c]:ev_ptr[c + 1]] for c in np.flatnonzero(keep_col)])
    np.testing.assert_array_equal(out_pairs, want)


def _hand():
    """span3 = 4, one recording of 8 frames, one class: tags (0.9, 0.1); the posteriors are above 0.5 on the frames 2 .. 6."""
    tl = np.full((8, 1), 0.1, np.float32)
    tl[2:7] = 0.8
    return tl, np.array([0, 8]), np.array([[0.9], [0.1]], np.float32), np.array([0, 2]), 4


def test_an_event_across_a_span_boundary_is_kept_when_either_side_is_confident():
    tl, rec_frame0, tags, rec_span0, span3 = _hand()
    _, ev_ptr, ev_pairs = stitch_np.decode(tl, rec_frame0, [0.5], [1])
    assert ev_pairs.tolist() == [[2, 7]]
    for t in (tags, tags[::-1].copy()):                                          # the confident span on either side
        score = sp.tag_scores(t, rec_span0, span3, 1, 1, ev_ptr, ev_pairs)
        assert score.tolist() == [np.float32(0.9)]
        out_ptr, out_pairs, _ = sp.gate(ev_ptr, ev_pairs, score, 1, 1, [0.5])
        assert out_ptr.tolist() == [0, 1] and out_pairs.tolist() == [[2, 7]]
    score = sp.tag_scores(np.array([[0.4], [0.1]], np.float32), rec_span0, span3, 1, 1, ev_ptr, ev_pairs)
    assert sp.gate(ev_ptr, ev_pairs, score, 1, 1, [0.5])[0].tolist() == [0, 0]
    # an event that ends ON the boundary touches span 0 only; strict comparison; NaN tags are skipped, all-NaN is never kept
    on_edge = np.array([[1, 4]], np.int32)
    assert sp.tag_scores(tags[::-1].copy(), rec_span0, span3, 1, 1, ev_ptr, on_edge).tolist() == [np.float32(0.1)]
    assert sp.gate(ev_ptr, ev_pairs, np.array([0.5], np.float32), 1, 1, [0.5])[0].tolist() == [0, 0]
    nan = np.float32(np.nan)
    assert sp.tag_scores(np.array([[nan], [0.3]], np.float32), rec_span0, span3, 1, 1, ev_ptr, ev_pairs).tolist() == [np.float32(0.3)]
    all_nan = sp.tag_scores(np.array([[nan], [nan]], np.float32), rec_span0, span3, 1, 1, ev_ptr, ev_pairs)
    assert np.isnan(all_nan).all() and sp.gate(ev_ptr, ev_pairs, all_nan, 1, 1, [-np.inf])[0].tolist() == [0, 0]


def test_the_gate_is_not_masking_the_posteriors_of_unconfident_spans():
    """The header's hand example: the gate keeps [2, 7) whole, masking span 1 and decoding gives [2, 4)."""
    tl, rec_frame0, tags, rec_span0, span3 = _hand()
    _, ev_ptr, ev_pairs = stitch_np.decode(tl, rec_frame0, [0.5], [1])
    score = sp.tag_scores(tags, rec_span0, span3, 1, 1, ev_ptr, ev_pairs)
    assert sp.gate(ev_ptr, ev_pairs, score, 1, 1, [0.5])[1].tolist() == [[2, 7]]
    _, m_ptr, m_pairs = sp.mask_then_decode(tl, rec_frame0, tags, rec_span0, span3, [0.5], [0.5], [1])
    assert m_ptr.tolist() == [0, 1] and m_pairs.tolist() == [[2, 4]]


def test_span_table_on_ragged_lengths():
    from dcase2019_task4_amd.inference import span_table
    L3s = [1, 3, 8, 9, 16, 17]
    host, dev, total, span3 = span_table(L3s, 8)
    assert dev is None and span3 == 8 and host.dtype == np.int64
    assert np.diff(host).tolist() == [1, 1, 1, 2, 2, 3] and total == 10          # L3 < span3, L3 % span3 == 0, a short last span
    np.testing.assert_array_equal(host, sp.span_table(L3s, 8))
    assert np.diff(span_table(L3s, 1)[0]).tolist() == L3s
    for big in (17, 18, 10 ** 12, float("inf")):                                 # the clamp: one span per recording
        host, _, total, span3 = span_table(L3s, big)
        assert span3 == 17 and total == len(L3s) and host.tolist() == list(range(len(L3s) + 1))
    for bad in (0, -3, 2.5, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            span_table(L3s, bad)
    with pytest.raises(ValueError):
        span_table([], 4)
    with pytest.raises(ValueError):
        span_table([5, 0], 4)


def test_tag_span_seconds_round_down_to_whole_frames():
    from dcase2019_task4_amd.inference import tag_span_frames
    fs = 8 * 511 / 44100
    assert tag_span_frames(10.0, fs) == 107 and tag_span_frames(108 * fs, fs) == 108 and tag_span_frames(0.01, fs) == 1
    assert tag_span_frames(float("inf"), fs) == float("inf")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            tag_span_frames(bad, fs)


def test_span_tags_dataframe_layout():
    from dcase2019_task4_amd.inference import span_tags_dataframe
    labels = ["Dog", "Cat"]
    tags = np.array([[0.9, 0.2], [0.6, 0.7], [0.1, 0.2]], np.float32)
    df = span_tags_dataframe(tags, [0, 2, 3], 4, ["a.wav", "b.wav"], labels, 0.5, frame_seconds=0.5, L3s=[7, 3])
    assert list(df.columns) == ["filename", "onset", "offset", "event_labels"]
    assert df.filename.tolist() == ["a.wav", "a.wav", "b.wav"] and df.event_labels.tolist() == ["Dog", "Dog,Cat", ""]
    assert df.onset.tolist() == [0.0, 2.0, 0.0] and df.offset.tolist() == [2.0, 3.5, 1.5]
    df = span_tags_dataframe(torch.from_numpy(tags), [0, 2, 3], 4, ["a.wav", "b.wav"], labels, [0.95, 0.15], frame_seconds=0.5)
    assert df.event_labels.tolist() == ["Cat", "Cat", "Cat"] and df.offset.tolist() == [2.0, 4.0, 2.0]
    with pytest.raises(ValueError):
        span_tags_dataframe(tags, [0, 2, 4], 4, ["a.wav", "b.wav"], labels)


def _ref():
    from dcase2019_task4_amd.metrics import RefEvents
    cols = [[[(0.0, 1.0)], [], [(0.5, 0.6)]], [[], [], []]]
    ptr, on, off = ls.pack(cols)
    return RefEvents(ptr, on, off, ["a", "b"], ["x", "y", "z"], device="cpu")


def test_argument_errors_come_before_any_forward():
    from dcase2019_task4_amd import inference, metrics
    for kw in (dict(min_span_tag=0.5), dict(return_span_tags=True), dict(tag_span=0.0), dict(tag_span=-1.0),
               dict(tag_span=10.0, min_span_tag=float("nan")), dict(tag_span=10.0, min_span_tag=[0.5, float("nan")])):
        with pytest.raises(ValueError):
            inference.get_long_predictions(None, None, ["x", "y"], **kw)
    ref = _ref()
    for kw in (dict(tag_span=10.0), dict(min_span_tags=[0.5]), dict(tag_span=0.0, min_span_tags=[0.5]),
               dict(tag_span=10.0, min_span_tags=[0.5, 0.6, 0.7], thresholds=[0.5, 0.6]),
               dict(tag_span=10.0, min_span_tags=[float("nan")]), dict(tag_span=10.0, min_span_tags=[[0.5, 0.5]])):
        with pytest.raises(ValueError):
            metrics.validate_long(None, None, ref, **kw)
