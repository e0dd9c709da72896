"""CPU checks of the event scores and the select by score: the plain-loop statement (tests/event_scores_np.py) on hand
cases, its NaN rules, the select at -inf / +inf / an exact tie, the ABI of the four new symbols and their argument checks
that need no GPU, and - on the grid tests/test_gpu_event_scores.py uses - that at median window 1 the select keyed on the
maximum with min_score = thr_hi is the two-threshold decode of tests/hysteresis_np.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import event_scores_np as es
from tests import hysteresis_np as hy
from tests import stitch_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)
SYMBOLS = ("sed_events_scores_short_frames", "sed_events_scores", "sed_events_select_ws_bytes", "sed_events_select")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_hand_cases_of_the_statement():
    tl = np.array([[0.25, 0.5], [0.75, 0.125], [0.5, 1.0], [0.1, 0.3]], np.float32)
    f0 = np.array([0, 4], np.int64)
    ptr = np.array([0, 2, 4], np.int64)
    pairs = np.array([[0, 1], [1, 4], [0, 4], [3, 4]], np.int32)
    smax, smean = es.scores(tl, f0, 1, 2, ptr, pairs)
    assert _bits(smax) == _bits([0.25, 0.75, 1.0, 0.3])
    want = [0.25, (np.float64(np.float32(0.75)) + 0.5 + np.float64(np.float32(0.1))) / 3,
            (0.5 + 0.125 + 1.0 + np.float64(np.float32(0.3))) / 4, np.float32(0.3)]
    assert _bits(smean) == _bits(np.asarray(want, np.float64).astype(np.float32))
    # a one-frame event: max == mean == the frame, bitwise, whatever the value
    rs = np.random.RandomState(0)
    for v in rs.uniform(size=40).astype(np.float32):
        assert _bits(es.event_max([v])) == _bits(es.event_mean([v])) == _bits(v)
    # a constant event of 2^m frames: the mean is the constant
    for m in range(0, 13):
        for v in (np.float32(0.1), np.float32(0.7310586), np.float32(1e-30)):
            assert _bits(es.event_mean([v] * 2 ** m)) == _bits(v) == _bits(es.event_max([v] * 2 ** m))
    # the mean is the exact sum, rounded once: 2^24 + 1 + 1 loses nothing in fp64
    assert es.event_mean([np.float32(2 ** 24), np.float32(1), np.float32(1)]) == np.float32((2 ** 24 + 2) / 3)


def test_two_recordings_and_points_address_their_own_frames():
    K, n_rec, NC = 2, 2, 3
    f0 = np.array([0, 5, 12], np.int64)
    rs = np.random.RandomState(1)
    tl = rs.uniform(size=(12, NC)).astype(np.float32)
    cols = [[(0, 2)], [], [(1, 5)], [(0, 7)], [(2, 3), (4, 6)], [], [], [(4, 5)], [], [(6, 7)], [], [(0, 1)]]
    ptr = np.r_[0, np.cumsum([len(c) for c in cols])].astype(np.int64)
    pairs = np.asarray([e for c in cols for e in c], np.int32)
    smax, smean = es.scores(tl, f0, n_rec, NC, ptr, pairs)
    i = 0
    for col, events in enumerate(cols):
        k, rec, c = es.column_of(col, n_rec, NC)
        assert (k, rec, c) == (col // 6, (col // 3) % 2, col % 3)
        for on, off in events:
            span = tl[f0[rec] + on:f0[rec] + off, c]
            assert smax[i] == span.max() and abs(float(smean[i]) - span.astype(np.float64).mean()) <= np.spacing(smean[i])
            i += 1


def test_the_nan_rules():
    v = np.float32(0.5)
    assert _bits(es.event_max([NAN, v, NAN])) == _bits(v) and np.isnan(es.event_mean([NAN, v, NAN]))
    assert np.isnan(es.event_max([NAN, NAN])) and np.isnan(es.event_mean([NAN]))
    assert es.event_max([v, NAN, np.float32(0.75)]) == np.float32(0.75)
    # an event outside its recording scores NaN twice
    tl, f0 = np.full((4, 1), 0.5, np.float32), np.array([0, 4], np.int64)
    smax, smean = es.scores(tl, f0, 1, 1, np.array([0, 4], np.int64), np.array([[0, 5], [2, 2], [-1, 2], [1, 3]], np.int32))
    assert np.isnan(smax[:3]).all() and np.isnan(smean[:3]).all() and smax[3] == smean[3] == 0.5


def test_the_select_at_infinities_a_tie_and_nan():
    ptr = np.array([0, 3, 3, 5], np.int64)
    pairs = np.array([[0, 1], [2, 3], [4, 9], [0, 2], [5, 6]], np.int32)
    smax = np.array([0.5, 0.25, NAN, 0.75, 0.5], np.float32)
    smean = np.array([0.4, 0.25, 0.1, NAN, 0.5], np.float32)
    inf = np.float32(np.inf)
    out = es.select(ptr, pairs, smax, smean, 1, 3, [-inf] * 3, 0)              # -inf keeps everything but NaN
    assert out[0].tolist() == [0, 2, 2, 4] and out[1].tolist() == [[0, 1], [2, 3], [0, 2], [5, 6]]
    assert _bits(out[2]) == _bits(smax[[0, 1, 3, 4]]) and _bits(out[3]) == _bits(smean[[0, 1, 3, 4]])
    out = es.select(ptr, pairs, smax, smean, 1, 3, [inf] * 3, 0)
    assert out[0].tolist() == [0, 0, 0, 0] and out[1].shape == (0, 2) and out[2].shape == (0,)
    out = es.select(ptr, pairs, smax, None, 1, 3, [0.5, 0.0, 0.5], 0)          # strict: a tie is dropped
    assert out[0].tolist() == [0, 0, 0, 1] and out[1].tolist() == [[0, 2]] and out[3] is None
    out = es.select(ptr, pairs, smax, smean, 1, 3, [np.nextafter(np.float32(0.5), np.float32(0)), 0.0, 0.5], 0)
    assert out[0].tolist() == [0, 1, 1, 2]
    out = es.select(ptr, pairs, smax, smean, 1, 3, [0.2, 0.0, 0.2], 1)         # keyed on the mean: its NaN drops the event
    assert out[1].tolist() == [[0, 1], [2, 3], [5, 6]]
    # the minimum of the column's (point, class)
    ptr2 = np.array([0, 1, 2, 3, 4], np.int64)                                 # K = 2, n_rec = 1, NC = 2
    s = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    out = es.select(ptr2, pairs[:4], s, None, 1, 2, [[0.4, 0.6], [0.6, 0.4]], 0)
    assert out[0].tolist() == [0, 1, 1, 1, 2]


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_bound_and_declared():
    from dcase2019_task4_amd import _lib
    header = open(os.path.join(REPO, "include", "dcase_sed.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    l = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.exported_symbols() and hasattr(l, name)
    assert l.sed_events_scores_short_frames() >= 1
    assert l.sed_events_select_ws_bytes(1 << 31, 4) == 0 and l.sed_events_select_ws_bytes(8, 0) == 0
    assert l.sed_events_select_ws_bytes(-1, 4) == 0 and l.sed_events_select_ws_bytes(8, 1 << 26) == 0
    assert b"pairs_capacity" in l.sed_last_error()
    assert l.sed_events_select_ws_bytes(0, 1) == 4 and l.sed_events_select_ws_bytes(257, 6) == 2 * 4 * 8 + 3 * 4
    assert l.sed_events_select_ws_bytes(257, 6) == l.sed_events_hysteresis_ws_bytes(257, 6)


class _HostArgs:
    """Host buffers behind every pointer: a call that passes its argument checks on a machine without a GPU would be a
    launch, so every call made here must be refused (SED_ERR_BAD_ARG = -1, SED_ERR_WORKSPACE = -2) by the checks alone."""

    def __init__(self):
        self.keep = {n: (C.c_double * 64)() for n in ("tl", "f0", "ptr", "pairs", "smax", "smean", "err", "mins", "optr",
                                                      "opairs", "omax", "omean", "ws")}
        self.p = {n: C.cast(b, C.c_void_p) for n, b in self.keep.items()}

    def scores(self, **kw):
        from dcase2019_task4_amd import _lib
        a = dict(self.p, total=8, n_rec=1, NC=2, cap=4, n_cols=2)
        a.update(kw)
        return _lib.lib().sed_events_scores(a["tl"], a["total"], a["f0"], a["n_rec"], a["NC"], a["ptr"], a["pairs"], a["cap"],
                                            a["n_cols"], a["smax"], a["smean"], a["err"], None)

    def select(self, **kw):
        from dcase2019_task4_amd import _lib
        l = _lib.lib()
        a = dict(self.p, n_rec=1, NC=2, cap=4, n_cols=2, key=0, out_cap=4)
        a.update(kw)
        ws_bytes = a.get("ws_bytes", l.sed_events_select_ws_bytes(4, 2))
        return l.sed_events_select(a["ptr"], a["pairs"], a["smax"], a["smean"], a["cap"], a["n_cols"], a["n_rec"], a["NC"],
                                   a["key"], a["mins"], a["optr"], a["opairs"], a["omax"], a["omean"], a["out_cap"], a["ws"],
                                   ws_bytes, a["err"], None)


def test_every_bad_argument_of_sed_events_scores_returns_before_a_launch():
    from dcase2019_task4_amd import _lib
    h, l = _HostArgs(), _lib.lib()
    for name in ("tl", "f0", "ptr", "pairs", "err"):
        assert h.scores(**{name: None}) == -1 and b"null" in l.sed_last_error(), name
    assert h.scores(smax=None, smean=None) == -1 and b"both null" in l.sed_last_error()
    for kw in (dict(NC=0), dict(NC=17), dict(n_rec=0), dict(n_cols=0), dict(n_cols=1 << 26), dict(n_cols=3), dict(n_cols=6, n_rec=2),
               dict(cap=-1), dict(cap=1 << 31), dict(total=-1), dict(total=1 << 30), dict(total=(1 << 31) // 2)):
        assert h.scores(**kw) == -1, kw
    assert h.scores(pairs=C.c_void_p(h.p["pairs"].value + 4)) == -1 and b"aligned" in l.sed_last_error()
    for name in ("tl", "f0", "ptr", "pairs"):                                  # an output on top of an input, whole or in part
        assert h.scores(smax=h.p[name]) == -1 and b"overlaps" in l.sed_last_error(), name
        assert h.scores(smean=C.c_void_p(h.p[name].value + 8)) == -1 and b"overlaps" in l.sed_last_error(), name
    assert h.scores(smean=h.p["smax"]) == -1 and b"overlaps" in l.sed_last_error()
    assert h.scores(smax=C.c_void_p(h.p["tl"].value + 8 * 2 * 4 - 4)) == -1    # the timeline's last float
    assert h.scores(cap=0) == 0                                                # nothing to launch: SED_OK without a device


def test_every_bad_argument_of_sed_events_select_returns_before_a_launch():
    from dcase2019_task4_amd import _lib
    h, l = _HostArgs(), _lib.lib()
    for name in ("ptr", "pairs", "mins", "optr", "opairs", "ws", "err"):
        assert h.select(**{name: None}) == -1 and b"null" in l.sed_last_error(), name
    assert h.select(key=2) == -1 and h.select(key=-1) == -1
    assert h.select(smax=None, omax=None) == -1 and b"key" in l.sed_last_error()          # key 0 needs score_max
    assert h.select(key=1, smean=None, omean=None) == -1 and b"key" in l.sed_last_error()
    for kw in (dict(smean=None), dict(omean=None), dict(key=1, smax=None), dict(key=1, omax=None)):
        assert h.select(**kw) == -1 and b"together" in l.sed_last_error(), kw
    for kw in (dict(cap=-1), dict(cap=1 << 31), dict(n_cols=0), dict(n_cols=1 << 26), dict(n_cols=3), dict(n_rec=0), dict(NC=0),
               dict(out_cap=-1)):
        assert h.select(**kw) == -1, kw
    for name in ("pairs", "opairs", "ws"):
        assert h.select(**{name: C.c_void_p(h.p[name].value + 4)}) == -1 and b"aligned" in l.sed_last_error(), name
    assert h.select(opairs=h.p["pairs"]) == -1 and b"in place" in l.sed_last_error()
    assert h.select(omax=h.p["smax"]) == -1 and b"in place" in l.sed_last_error()
    assert h.select(ws_bytes=l.sed_events_select_ws_bytes(4, 2) + 8) == -2 and b"ws_bytes" in l.sed_last_error()
    assert h.select(ws_bytes=0) == -2


def test_the_python_fronts_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.inference import events_scores, events_select, score_decoded, select_decoded
    ptr, pairs = torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32)
    tl, f0, s = torch.zeros(4, 1), torch.tensor([0, 4]), torch.zeros(1)
    with pytest.raises(_lib.SedError):
        events_scores((ptr, pairs), tl, f0, 1, 1)
    with pytest.raises(_lib.SedError):
        events_select(ptr, pairs, s, None, 1, 1, 0.5)
    with pytest.raises(ValueError):
        events_scores((ptr, pairs), tl, f0, 1, 1, want=("median",))
    with pytest.raises(ValueError):
        events_scores((ptr, pairs), tl, f0, 1, 1, want=())
    with pytest.raises(ValueError):
        events_select(ptr, pairs, s, None, 1, 1, 0.5, key="median")
    out = {"ev_ptr": ptr, "ev_pairs": pairs, "err": torch.zeros(1, dtype=torch.int32), "timeline": None, "binary": None}
    with pytest.raises(ValueError, match="timeline"):
        score_decoded(out, f0, 1, 1)
    with pytest.raises(ValueError, match="timeline"):
        select_decoded(out, f0, 1, 1, 0.5)


# ---- the select on the maximum is hysteresis at window 1, on the grid of the GPU test -----------------------------------------
HYST_GRID = [(NC, hop3, weighting) for NC in (3, 4) for hop3 in (8, 16) for weighting in (0, 1)]
T3_E = 16
HYST_LENGTHS = [1, 2, 255, 256, 257, 1100]


def hysteresis_case(NC, hop3, weighting, K=3):
    """Window posteriors (slices of a smooth timeline plus noise, as in tests/test_gpu_hysteresis.py), their tables, the numpy
    blend and K threshold pairs from its quantiles, all at median window 1."""
    L3s = HYST_LENGTHS
    n_win = [1 if L <= T3_E else 1 + -(-(L - T3_E) // hop3) for L in L3s]
    rec_win0, rec_frame0 = np.r_[0, np.cumsum(n_win)].astype(np.int32), np.r_[0, np.cumsum(L3s)].astype(np.int64)
    rs = np.random.RandomState(70 + 10 * NC + hop3)
    p = rs.uniform(size=(rec_win0[-1], T3_E, NC)).astype(np.float32)
    for r, L in enumerate(L3s):
        base = hy.smooth_timeline(300 + 10 * r + NC, L, NC)
        for j in range(n_win[r]):
            n = min(T3_E, L - j * hop3)
            p[rec_win0[r] + j, :n] = base[j * hop3:j * hop3 + n] + rs.uniform(-0.02, 0.02, size=(n, NC)).astype(np.float32)
    tl = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting)
    thr_lo = np.stack([np.quantile(tl, q, axis=0) for q in (0.35, 0.5, 0.6)[:K]]).astype(np.float32)
    thr_hi = np.maximum(np.stack([np.quantile(tl, q, axis=0) for q in (0.8, 0.75, 0.95)[:K]]).astype(np.float32), thr_lo)
    return p, rec_win0, rec_frame0, tl, thr_lo, thr_hi


def decode_points(tl, rec_frame0, thr, NC):
    """K one-window-1 decodes as one table in column order (k, rec, c)."""
    ptrs, pairs, base = [np.zeros(1, np.int64)], [], 0
    for k in range(len(thr)):
        _, ptr, ev = stitch_np.decode(tl, rec_frame0, thr[k], np.ones(NC, np.int32))
        ptrs.append(ptr[1:] + base)
        pairs.append(ev)
        base += int(ptr[-1])
    return np.concatenate(ptrs), np.concatenate(pairs).astype(np.int32).reshape(-1, 2)


@pytest.mark.parametrize("NC,hop3,weighting", HYST_GRID)
def test_select_on_the_maximum_is_the_two_threshold_decode_at_window_1(NC, hop3, weighting):
    p, rec_win0, rec_frame0, tl, thr_lo, thr_hi = hysteresis_case(NC, hop3, weighting)
    n_rec, K = len(rec_frame0) - 1, len(thr_lo)
    lo_ptr, lo_pairs = decode_points(tl, rec_frame0, thr_lo, NC)
    smax, smean = es.scores(tl, rec_frame0, n_rec, NC, lo_ptr, lo_pairs)
    got = es.select(lo_ptr, lo_pairs, smax, smean, n_rec, NC, thr_hi, 0)
    want_ptr, want_pairs = hy.decode_pairs(tl, rec_frame0, thr_lo, thr_hi, np.ones((K, NC), np.int32))
    assert got[0].tobytes() == want_ptr.tobytes() and got[1].tobytes() == want_pairs.tobytes()
    assert 0.1 * lo_ptr[-1] < want_ptr[-1] < 0.9 * lo_ptr[-1] and lo_ptr[-1] > 60          # both branches of the rule
