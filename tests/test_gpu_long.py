"""-m gpu tests of the long-recording path: sed_stitch_decode (blend bitwise against tests/stitch_np.py, decode exact against
scipy + the restated dcase_util decode, error bits, reproducibility, graph replay, agreement with sed_postprocess on
single-window recordings) and LongRecordingSet + get_long_predictions end to end on a small model."""

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import postprocess_np as pp
from tests import gpu_util as gu
from tests import stitch_np
from tests.long_util import SENT, StitchCall, _n_windows, _Scaler, _tables, _tile

pytestmark = pytest.mark.gpu

SENT_I = SENT


def _lengths(hop3=8):
    t = _tile()
    return [1, 7, 8, 9, 8 + hop3, t - 1, t, t + 1, 2 * t + 5]


def _check_decode(got, timeline, rec_frame0, thr, win, capacity):
    binary, ev_ptr, ev_pairs = stitch_np.decode(timeline, rec_frame0, thr, win)
    assert got["err"] == 0
    np.testing.assert_array_equal(got["binary"], binary)
    np.testing.assert_array_equal(got["ev_ptr"], ev_ptr)
    assert ev_ptr[-1] <= capacity
    np.testing.assert_array_equal(got["ev_pairs"][:ev_ptr[-1]], ev_pairs)
    assert (got["ev_pairs"][ev_ptr[-1]:] == SENT_I).all()


# ---- blend, bitwise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(3, False), (10, False), (12, False), (12, True)])
def test_blend_is_bitwise_the_numpy_statement(NC, misalign, hop3, weighting):
    """Scalar path (NC = 3, 10; NC = 12 off 16-byte alignment) and 16-byte path (NC = 12), every length around the window and
    the tile, all as recordings of ONE call; then the decode of the same call against the reference on the numpy timeline."""
    T3 = 8
    L3s = _lengths(hop3)
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(100 * NC + 10 * hop3 + weighting)
    p = rs.uniform(size=(rec_win0[-1], T3, NC)).astype(np.float32)
    thr = (0.35 + 0.02 * np.arange(NC)).astype(np.float32)
    win = np.array([1, 5, 63][:NC] * 6)[:NC]
    call = StitchCall(p, rec_win0, rec_frame0, hop3, weighting, thr, win, misalign=misalign)
    got = call.run()
    want = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting)
    np.testing.assert_array_equal(got["timeline"].view(np.uint32), want.view(np.uint32))
    # the single-window recordings (L3 <= T3) are their windows, byte for byte
    for r, L3 in enumerate(L3s):
        if L3 <= T3:
            np.testing.assert_array_equal(got["timeline"][rec_frame0[r]:rec_frame0[r + 1]].view(np.uint32),
                                          p[rec_win0[r], :L3].view(np.uint32))
    _check_decode(got, want, rec_frame0, thr, win, call.capacity)


def test_blend_at_the_baseline_geometry_and_mixed_recordings_in_one_call():
    """T3 = 78, NC = 10, hop3 = 39 (the default hop at frames = 628): four recordings of mixed lengths, one single-window."""
    T3, NC, hop3 = 78, 10, 39
    L3s = [200, 78, 41, _tile() + 30]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p = np.random.RandomState(5).uniform(size=(rec_win0[-1], T3, NC)).astype(np.float32)
    thr, win = np.full(NC, 0.5, np.float32), np.full(NC, 5)
    for weighting in (0, 1):
        got = StitchCall(p, rec_win0, rec_frame0, hop3, weighting, thr, win).run()
        want = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting)
        np.testing.assert_array_equal(got["timeline"].view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(got["timeline"][rec_frame0[1]:rec_frame0[2]].view(np.uint32), p[rec_win0[1]].view(np.uint32))
        _check_decode(got, want, rec_frame0, thr, win, NC * sum((L + 1) // 2 for L in L3s))


# ---- decode, exact -----------------------------------------------------------------------------------------------------------
NC_D = 10
WIN_D = np.array([1, 5, 63, 1, 5, 1, 63, 5, 1, 5])
THR_D = (0.3 + 0.04 * np.arange(NC_D)).astype(np.float32)


def _pattern(name, L3, rs):
    """A [L3, NC_D] float32 timeline; active = 0.9, inactive = 0.1 (every threshold lies between)."""
    tile = _tile()
    a = np.zeros((L3, NC_D), dtype=bool)
    if name == "random_with_ties":
        x = rs.uniform(size=(L3, NC_D)).astype(np.float32)
        ties = rs.uniform(size=(L3, NC_D)) < 0.2
        return np.where(ties, THR_D[None, :], x).astype(np.float32)            # exactly the threshold: NOT active (strict >)
    if name == "tile_edges":
        for E in range(tile, L3 + 1, tile):
            for c, (lo, hi) in enumerate([(E - 3, E), (E, E + 3), (E - 2, E + 2), (E - 1, E), (E, E + 1), (E - 1, E + 1),
                                          (E - 40, E + 40), (E - 5, E), (E, E + 5), (E - 1, E + 4)]):
                a[max(lo, 0):min(hi, L3), c] = True
        a[0:2, 0] = True
        a[L3 - 1:, 3] = True
        if L3 > tile:
            a[:, 5] = False
            a[tile - 1:L3, 5] = True                                           # from the last frame of tile 0 to the very end
    elif name == "all_active":
        a[:] = True
    elif name == "alternating":
        a[0::2] = True
    elif name == "all_zero":
        pass
    elif name == "last_tile_head":
        s_last = ((L3 - 1) // tile) * tile                                     # frames the previous tile sees only as its halo
        a[s_last:min(L3, s_last + 20)] = True
        a[s_last:min(L3, s_last + 1), 3] = True
    return np.where(a, np.float32(0.9), np.float32(0.1)).astype(np.float32)


@pytest.mark.parametrize("name", ["random_with_ties", "tile_edges", "all_active", "alternating", "all_zero", "last_tile_head"])
def test_decode_patterns_are_exact(name):
    """hop3 = T3: every frame has one window, so the timeline IS the prescribed pattern; windows 1 / 5 / 63 mixed over the
    classes (63 is longer than the short columns), per-class thresholds, all lengths as recordings of one call."""
    T3 = 8
    L3s = _lengths(T3)
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    rs = np.random.RandomState(len(name))
    tls = [_pattern(name, L3, rs) for L3 in L3s]
    p = np.concatenate([np.concatenate([t, np.full((-len(t) % T3, NC_D), 0.95, np.float32)]).reshape(-1, T3, NC_D) for t in tls])
    win = np.ones(NC_D, dtype=int) if name == "alternating" else WIN_D
    call = StitchCall(p, rec_win0, rec_frame0, T3, 1, THR_D, win)
    got = call.run()
    timeline = np.concatenate(tls)
    np.testing.assert_array_equal(got["timeline"].view(np.uint32), timeline.view(np.uint32))
    _check_decode(got, timeline, rec_frame0, THR_D, win, call.capacity)
    per_col = np.diff(got["ev_ptr"]).reshape(len(L3s), NC_D)
    if name == "alternating":
        assert got["ev_ptr"][-1] == call.capacity                              # ceil(L3 / 2) events per column: the bound
        assert (per_col == ((np.array(L3s) + 1) // 2)[:, None]).all()
    if name == "all_active":
        assert (per_col == 1).all()
        ev = got["ev_pairs"][:got["ev_ptr"][-1]].reshape(len(L3s), NC_D, 2)
        assert (ev[:, :, 0] == 0).all() and (ev[:, :, 1] == np.array(L3s)[:, None]).all()
    if name == "all_zero":
        assert got["ev_ptr"][-1] == 0


# ---- errors and limits -------------------------------------------------------------------------------------------------------
def _alternating_call(**kw):
    T3, NC = 8, 3
    L3s = [9, _tile() + 3]
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    # 0.9, 0.1, 0.9, ... from frame 0 of every recording
    p = np.concatenate([np.resize(np.array([[0.9] * NC, [0.1] * NC], np.float32), (_n_windows(L, T3, T3) * T3, NC)).reshape(-1, T3, NC)
                        for L in L3s])
    total = NC * sum((L + 1) // 2 for L in L3s)
    return StitchCall(p, rec_win0, rec_frame0, T3, 0, np.full(NC, 0.5, np.float32), np.ones(NC, int), **kw), total, rec_frame0


def test_capacity_one_short_raises_bit_2_and_writes_nothing_beyond():
    full, total, rec_frame0 = _alternating_call()
    ref = full.run()
    assert ref["err"] == 0 and ref["ev_ptr"][-1] == total
    short, _, _ = _alternating_call(capacity=total - 1)
    got = short.run()
    assert got["err"] == 2
    np.testing.assert_array_equal(got["ev_ptr"], ref["ev_ptr"])                # still the true counts
    assert (got["ev_pairs"][total - 1:] == SENT_I).all()                       # nothing at or beyond capacity
    np.testing.assert_array_equal(got["ev_pairs"][:total - 1], ref["ev_pairs"][:total - 1])


@pytest.mark.parametrize("bad", [0, 64])
def test_a_window_outside_1_63_raises_bit_8(bad):
    call, total, _ = _alternating_call()
    call.win = torch.tensor([1, bad, 1], dtype=torch.int32, device="cuda")
    got = call.run()
    assert got["err"] == 8
    per_col = np.diff(got["ev_ptr"]).reshape(2, 3)
    assert (per_col[:, 1] == 0).all() and (per_col[:, 0] > 0).all()            # that class is not decoded


def test_too_few_windows_raise_bit_32_without_touching_anything_else():
    """Recording 1 needs 4 windows and is given 2: bit 32, it is not decoded, and the kernel reads no window of recording 2."""
    T3, NC = 8, 3
    rec_win0 = np.array([0, 1, 3, 4], dtype=np.int32)
    rec_frame0 = np.array([0, 8, 38, 46], dtype=np.int64)
    p = np.full((4, T3, NC), 0.9, dtype=np.float32)
    got = StitchCall(p, rec_win0, rec_frame0, T3, 0, np.full(NC, 0.5, np.float32), np.ones(NC, int)).run()
    assert got["err"] == 32
    per_col = np.diff(got["ev_ptr"]).reshape(3, NC)
    assert (per_col[1] == 0).all() and (per_col[0] == 1).all() and (per_col[2] == 1).all()
    assert np.isnan(got["timeline"][8:38]).all() and (got["binary"][8:38] == 0xEE).all()
    assert (got["timeline"][:8] == np.float32(0.9)).all() and (got["timeline"][38:] == np.float32(0.9)).all()


def test_malformed_tables_raise_bit_16():
    T3, NC = 8, 3
    p = np.full((3, T3, NC), 0.9, dtype=np.float32)
    for rec_win0, rec_frame0 in [([0, 1, 3], [0, 8, 8]), ([0, 2, 1], [0, 8, 16]), ([0, 1, 2], [0, 20, 16])]:
        got = StitchCall(p, np.array(rec_win0, np.int32), np.array(rec_frame0, np.int64), T3, 0, np.full(NC, 0.5, np.float32),
                    np.ones(NC, int), capacity=64).run()
        assert got["err"] & 16, (rec_win0, rec_frame0)


def test_bad_host_arguments_return_bad_arg_before_any_launch():
    from dcase2019_task4_amd import _lib
    call, _, _ = _alternating_call()
    call.fill()
    l, ptr = call.l, _lib.ptr

    def go(T3=8, NC=3, hop3=8, weighting=0, n_rec=2, capacity=call.capacity, p=call.p, ws=call.ws, ws_bytes=None):
        return l.sed_stitch_decode(ptr(p), ptr(call.rec_win0), ptr(call.rec_frame0), n_rec, T3, NC, hop3, weighting, ptr(call.thr),
                                   ptr(call.win), ptr(call.timeline), ptr(call.binary), ptr(call.ev_ptr), ptr(call.ev_pairs),
                                   capacity, ptr(ws), call.ws_bytes if ws_bytes is None else ws_bytes, ptr(call.err),
                                   _lib.stream_ptr())

    for kw in (dict(NC=17), dict(NC=0), dict(hop3=0), dict(hop3=9), dict(T3=0), dict(weighting=2), dict(n_rec=0),
               dict(capacity=-1), dict(p=None), dict(ws=None)):
        assert go(**kw) == -1, kw                                              # SED_ERR_BAD_ARG
    assert go(ws_bytes=8) == -2                                                # SED_ERR_WORKSPACE
    assert l.sed_stitch_decode_ws_bytes(1 << 28, 1, 10) == 0 and l.sed_stitch_decode_ws_bytes(100, 1, 17) == 0
    torch.cuda.synchronize()
    assert int(call.ev_ptr[0].item()) == SENT_I and int(call.err[0].item()) == 0  # nothing ran
    with pytest.raises(ValueError):
        from dcase2019_task4_amd.inference import stitch_decode
        stitch_decode(call.p.view(-1, 8, 3), call.rec_win0, call.rec_frame0, call.total, 8, weighting="hann")


def test_two_calls_and_a_graph_replay_give_identical_bytes():
    T3, NC, hop3 = 8, 10, 3
    L3s = [_tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p = np.random.RandomState(9).uniform(size=(rec_win0[-1], T3, NC)).astype(np.float32)
    call = StitchCall(p, rec_win0, rec_frame0, hop3, 1, np.full(NC, 0.5, np.float32), np.array([1, 3, 5, 7, 9] * 2))
    a = call.run()
    b = call.run()
    for k in ("timeline", "binary", "ev_ptr", "ev_pairs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["err"] == 0 and a["ev_ptr"][-1] > 0
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    c = call.get()
    for k in ("timeline", "binary", "ev_ptr", "ev_pairs"):
        assert a[k].tobytes() == c[k].tobytes(), k
    assert c["err"] == 0


# ---- single-window agreement with sed_postprocess -------------------------------------------------------------------------------
@pytest.mark.parametrize("T3,NC,win", [(78, 10, 5), (600, 4, 7)])
def test_single_window_recordings_agree_with_sed_postprocess(T3, NC, win):
    from dcase2019_task4_amd.inference import postprocess
    n = 5
    p = np.random.RandomState(T3).uniform(size=(n, T3, NC)).astype(np.float32)
    rec_win0, rec_frame0 = np.arange(n + 1, dtype=np.int32), np.arange(n + 1, dtype=np.int64) * T3
    got = StitchCall(p, rec_win0, rec_frame0, T3, 1, np.full(NC, 0.5, np.float32), np.full(NC, win)).run()
    cnt, pairs = postprocess(torch.from_numpy(p).cuda(), 0.5, win)
    cnt, pairs = cnt.cpu().numpy().reshape(-1), pairs.cpu().numpy().reshape(n * NC, -1, 2)
    assert got["err"] == 0
    np.testing.assert_array_equal(np.diff(got["ev_ptr"]), cnt)
    for col in range(n * NC):
        np.testing.assert_array_equal(got["ev_pairs"][got["ev_ptr"][col]:got["ev_ptr"][col + 1]], pairs[col, :cnt[col]])
    np.testing.assert_array_equal(got["timeline"].view(np.uint32), p.reshape(-1, NC).view(np.uint32))


# ---- end to end, small model ---------------------------------------------------------------------------------------------------
class _Enc:
    def __init__(self, labels):
        self.labels = labels

    def decode_strong(self, m):
        return pp.decode_strong(m, self.labels)


LABELS = [f"c{i}" for i in range(10)]
FRAMES = 64


def _recordings(lengths, seed=21):
    rs = np.random.RandomState(seed)
    return [(np.abs(rs.standard_normal((L, 64))) ** 2 * np.exp(rs.uniform(-6, 2, (L, 1))) + 1e-6).astype(np.float32) for L in lengths]


@pytest.fixture(scope="module")
def e2e():
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions
    model, _ = gu.make_model(0)
    model.eval()
    feats = _recordings([40, 64, 300])
    sc = _Scaler(64)
    ls = LongRecordingSet.from_arrays(feats, FRAMES, scaler=sc, filenames=["a.wav", "b.wav", "c.wav"])
    _, timelines, win_strong = get_long_predictions(model, ls, LABELS, batch_size=4, return_posteriors=True)
    # thresholds that make events: each class's median blended posterior
    thr = np.median(torch.cat(timelines).cpu().numpy(), axis=0).astype(np.float32)
    return dict(model=model, feats=feats, sc=sc, ls=ls, thr=thr, get=get_long_predictions)


def test_e2e_window_inputs_equal_host_sliced_clips(e2e):
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    ls = e2e["ls"]
    assert ls.n_clips == 11 and len(ls) == 11 and ls.hop_frames == 32
    slices = []
    for f in e2e["feats"]:
        L3 = max(1, len(f) // 8)
        for j in range(_n_windows(L3, 8, 4)):
            slices.append(f[32 * j:32 * j + FRAMES])
    assert len(slices) == ls.n_clips
    ref = ResidentFeatureSet.from_arrays(slices, None, frames=FRAMES, scaler=e2e["sc"], augment_type=None)
    a, b = ls.eval_batch(0, ls.n_clips), ref.eval_batch(0, ref.n_clips)
    assert a.shape == (11, 1, FRAMES, 64)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert ls.eval_batch(3, 2).cpu().numpy().tobytes() == b[3:5].cpu().numpy().tobytes()


@pytest.mark.parametrize("weighting", ["taper", "uniform"])
def test_e2e_table_equals_numpy_blend_and_reference_decode(e2e, weighting, tmp_path):
    ls, thr = e2e["ls"], e2e["thr"]
    win = [3, 1, 5, 3, 3, 7, 3, 1, 3, 5]
    path = str(tmp_path / "long.tsv")
    model = e2e["model"]
    model.train()
    df, timelines, win_strong = e2e["get"](model, ls, _Enc(LABELS).decode_strong, 8, save_predictions=path, batch_size=4,
                                           threshold=thr, median_window=win, weighting=weighting, return_posteriors=True)
    assert model.training                                                      # the training flag is restored
    model.eval()
    assert tuple(win_strong.shape) == (11, 8, 10) and [tuple(t.shape) for t in timelines] == [(5, 10), (8, 10), (37, 10)]
    p = win_strong.cpu().numpy()
    want_tl = stitch_np.blend(p, ls.rec_win0_host, ls.rec_frame0_host, ls.hop3, {"uniform": 0, "taper": 1}[weighting])
    got_tl = torch.cat(timelines).cpu().numpy()
    np.testing.assert_array_equal(got_tl.view(np.uint32), want_tl.view(np.uint32))
    _, ev_ptr, ev_pairs = stitch_np.decode(want_tl, ls.rec_frame0_host, thr, win)
    assert ev_ptr[-1] > 0
    rows = []
    for col in range(3 * 10):
        for on, off in ev_pairs[ev_ptr[col]:ev_ptr[col + 1]]:
            rows.append((LABELS[col % 10], int(on) * 8 / (44100 / 511), int(off) * 8 / (44100 / 511), ls.filenames[col // 10]))
    assert list(df.columns) == ["event_label", "onset", "offset", "filename"] and len(df) == len(rows)
    assert df.event_label.tolist() == [r[0] for r in rows] and df.filename.tolist() == [r[3] for r in rows]
    np.testing.assert_array_equal(df.onset.to_numpy(dtype=np.float64), np.array([r[1] for r in rows]))
    np.testing.assert_array_equal(df.offset.to_numpy(dtype=np.float64), np.array([r[2] for r in rows]))
    back = pd.read_csv(path, sep="\t")
    assert list(back.columns) == list(df.columns) and len(back) == len(df)


def test_e2e_clip_long_recordings_equal_get_predictions(e2e):
    """Recordings of exactly `frames` frames are single windows: same batches, same forwards, same table as get_predictions."""
    from dcase2019_task4_amd.inference import LongRecordingSet, get_predictions
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    feats = _recordings([FRAMES] * 5, seed=33)
    names = [f"clip_{i}.wav" for i in range(5)]
    ls = LongRecordingSet.from_arrays(feats, FRAMES, scaler=e2e["sc"], filenames=names)
    rs = ResidentFeatureSet.from_arrays(feats, None, frames=FRAMES, scaler=e2e["sc"], augment_type=None)
    rs.filenames = pd.Series(names)
    enc = _Enc(LABELS).decode_strong
    thr = float(np.median(e2e["get"](e2e["model"], ls, enc, 8, batch_size=2, return_posteriors=True)[2].cpu().numpy()))
    want = get_predictions(e2e["model"], rs, enc, 8, batch_size=2, threshold=thr)
    got = e2e["get"](e2e["model"], ls, enc, 8, batch_size=2, threshold=thr)
    assert len(want) > 0
    pd.testing.assert_frame_equal(got, want)


def test_e2e_per_class_thresholds_reach_the_kernel(e2e):
    ls, thr = e2e["ls"], e2e["thr"]
    base = e2e["get"](e2e["model"], ls, LABELS, batch_size=4, threshold=thr, median_window=3)
    thr2 = thr.copy()
    thr2[4] = 2.0                                                              # no posterior exceeds it
    other = e2e["get"](e2e["model"], ls, LABELS, batch_size=4, threshold=thr2, median_window=3)
    assert (base.event_label == "c4").any() and not (other.event_label == "c4").any()
    pd.testing.assert_frame_equal(base[base.event_label != "c4"].reset_index(drop=True), other.reset_index(drop=True))
    win2 = [3] * 10
    win2[7] = 9
    third = e2e["get"](e2e["model"], ls, LABELS, batch_size=4, threshold=thr, median_window=win2)
    pd.testing.assert_frame_equal(base[base.event_label != "c7"].reset_index(drop=True),
                                  third[third.event_label != "c7"].reset_index(drop=True))


def test_e2e_cpu_model_and_error_word_raise(e2e):
    from dcase2019_task4_amd import _lib
    cpu_model, _ = gu.make_model(0, device="cpu")
    with pytest.raises(_lib.SedError):
        e2e["get"](cpu_model, e2e["ls"], LABELS)
    with pytest.raises(_lib.SedError, match="bit 8"):
        e2e["get"](e2e["model"], e2e["ls"], LABELS, median_window=64)


def test_from_waveforms_pool_is_the_extractors_mel():
    from dcase2019_task4_amd.features import FeatureConfig, FeatureExtractor
    from dcase2019_task4_amd.inference import LongRecordingSet
    cfg = FeatureConfig.baseline_16k()
    fx = FeatureExtractor(cfg)
    t = np.arange(25 * cfg.sample_rate) / cfg.sample_rate
    wave = (0.3 * np.sin(2 * np.pi * 440 * t * (1 + 0.1 * t)) + 0.05 * np.random.RandomState(1).standard_normal(t.size)).astype(np.float32)
    ls = LongRecordingSet.from_waveforms([wave, wave[:30000]], fx, 628)
    mel = fx.calculate_mel_spec(wave)
    L = 1 + wave.size // cfg.hop_length
    assert mel.shape == (L, 64) and ls.pool.device.type == "cuda"
    np.testing.assert_array_equal(ls.pool[:L * 64].cpu().numpy().view(np.uint32), mel.reshape(-1).view(np.uint32))
    np.testing.assert_array_equal(ls.pool[L * 64:].cpu().numpy(), fx.calculate_mel_spec(wave[:30000]).reshape(-1))
    np.testing.assert_array_equal(ls.rec_frames_host, [L, 1 + 30000 // cfg.hop_length])
    L3 = L // 8
    assert ls.n_clips == 1 + -(-(L3 - 78) // 39) + 1 and ls.eval_batch(0, ls.n_clips).shape == (ls.n_clips, 1, 628, 64)
