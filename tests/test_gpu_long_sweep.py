"""-m gpu tests of the K-operating-point sweep over long recordings: sed_stitch_sweep (exact against tests/stitch_np.py and byte
for byte against K calls of sed_stitch_decode, error bits, bad arguments), sed_long_sweep_event_counts /
sed_long_sweep_psds_counts (exact against tests/sed_eval_np.py and tests/psds_np.py, byte for byte against K one-point
calls, error isolation between points), the three calls in one graph, and validate_long(one_blend=True) against
validate_long(one_blend=False) and the oracle.  Every buffer a kernel writes starts as sentinel / NaN bytes."""
import functools

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import long_score_np as ls
from tests import psds_np
from tests import sed_eval_np as se
from tests import stitch_np
from tests.long_util import (SENT, ScoreCall, StitchCall, _group, _l, _n_windows, _ref_events, _Scaler, _stitch_inputs, _tables,
                             _tile)

pytestmark = pytest.mark.gpu

NUM, DEN = 8.0, 44100 / 511
_Sweep = functools.partial(StitchCall, sweep=True)       # sed_stitch_sweep on sentinel-filled outputs; thr / win are [K, NC]


def _lengths():
    return [_tile() + 9, 5, 1500]          # one tile edge, a recording shorter than a halo, a multi-tile recording


def _np_sweep(timeline, rec_frame0, thr, win):
    """The concatenation of stitch_np.decode per point: (ev_ptr [K * n_rec * NC + 1], ev_pairs)."""
    ptrs, pairs, base = [np.zeros(1, np.int64)], [], 0
    for k in range(len(thr)):
        _, ev_ptr, ev_pairs = stitch_np.decode(timeline, rec_frame0, thr[k], win[k])
        ptrs.append(ev_ptr[1:] + base)
        pairs.append(ev_pairs)
        base += int(ev_ptr[-1])
    return np.concatenate(ptrs), np.concatenate(pairs)


# ---- 1. decode against the numpy statement ----------------------------------------------------------------------------------------
T3_B = 16


@functools.lru_cache(maxsize=None)
def _blend_case(NC, hop3, weighting):
    """(p, rec_win0, rec_frame0, thr [6, NC], win [6, NC], numpy timeline, numpy ev_ptr, numpy ev_pairs), computed once."""
    rec_win0, rec_frame0 = _tables(_lengths(), T3_B, hop3)
    rs = np.random.RandomState(1000 + 100 * NC + 10 * hop3 + weighting)
    p = rs.uniform(size=(rec_win0[-1], T3_B, NC)).astype(np.float32)
    K = 6
    win = rs.choice([1, 5, 63], size=(K, NC)).astype(np.int32)
    thr = rs.uniform(0.3, 0.7, size=(K, NC)).astype(np.float32)
    thr[2] = 2.0                                                               # above every posterior: empty columns between full ones
    thr[4], win[4] = thr[1], win[1]                                            # two identical points
    timeline = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting)
    ev_ptr, ev_pairs = _np_sweep(timeline, rec_frame0, thr, win)
    return p, rec_win0, rec_frame0, thr, win, timeline, ev_ptr, ev_pairs


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(3, False), (10, False), (12, False), (12, True)])
def test_sweep_is_the_numpy_statement_at_every_point(NC, misalign, hop3, weighting):
    p, rec_win0, rec_frame0, thr, win, timeline, ev_ptr, ev_pairs = _blend_case(NC, hop3, weighting)
    call = _Sweep(p, rec_win0, rec_frame0, hop3, weighting, thr, win, misalign=misalign)
    got = call.run()
    assert got["err"] == 0
    np.testing.assert_array_equal(got["timeline"].view(np.uint32), timeline.view(np.uint32))
    np.testing.assert_array_equal(got["ev_ptr"], ev_ptr)
    total = int(ev_ptr[-1])
    assert 0 < total <= call.capacity
    np.testing.assert_array_equal(got["ev_pairs"][:total], ev_pairs)
    assert (got["ev_pairs"][total:] == SENT).all()
    n = call.n_rec * NC
    per_point = np.diff(got["ev_ptr"]).reshape(6, n)
    assert (per_point[2] == 0).all() and per_point[1].sum() > 0 and per_point[3].sum() > 0
    np.testing.assert_array_equal(per_point[1], per_point[4])
    a = got["ev_pairs"][got["ev_ptr"][n]:got["ev_ptr"][2 * n]]
    b = got["ev_pairs"][got["ev_ptr"][4 * n]:got["ev_ptr"][5 * n]]
    assert a.tobytes() == b.tobytes()


# ---- 2. decode against K calls of stitch_decode -------------------------------------------------------------------------------------
NC_D = 10
WIN_D = np.array([1, 5, 63, 1, 5, 1, 63, 5, 1, 5])
THR_D = (0.3 + 0.04 * np.arange(NC_D)).astype(np.float32)


def _pattern(name, L3):
    """[L3, NC_D] float32 timelines of tests/test_gpu_long.py: active = 0.9, inactive = 0.1."""
    tile = _tile()
    a = np.zeros((L3, NC_D), dtype=bool)
    if name == "tile_edges":
        for E in range(tile, L3 + 1, tile):
            for c, (lo, hi) in enumerate([(E - 3, E), (E, E + 3), (E - 2, E + 2), (E - 1, E), (E, E + 1), (E - 1, E + 1),
                                          (E - 40, E + 40), (E - 5, E), (E, E + 5), (E - 1, E + 4)]):
                a[max(lo, 0):min(hi, L3), c] = True
        a[0:2, 0] = True
        a[L3 - 1:, 3] = True
        if L3 > tile:
            a[:, 5] = False
            a[tile - 1:L3, 5] = True
    elif name == "alternating":
        a[0::2] = True
    return np.where(a, np.float32(0.9), np.float32(0.1)).astype(np.float32)


def _points(K, name):
    """K points around THR_D / WIN_D: windows rotated over the classes, some thresholds above 0.9 (empty columns), some below
    0.1 (one event per column)."""
    thr = np.stack([np.roll(THR_D, k) for k in range(K)]).astype(np.float32)
    win = np.stack([np.roll(WIN_D, k) for k in range(K)]).astype(np.int32)
    if name == "alternating":
        win[0::2] = 1                                                          # the event bound itself at every other point
    for k in range(K):
        thr[k, (3 * k) % NC_D] = 0.95
        thr[k, (3 * k + 1) % NC_D] = 0.05
    return thr, win


@pytest.mark.parametrize("name", ["tile_edges", "alternating"])
@pytest.mark.parametrize("k_case", [0, 1, 2])
def test_sweep_equals_k_calls_of_stitch_decode_byte_for_byte(name, k_case):
    from dcase2019_task4_amd.inference import stitch_decode, stitch_sweep
    G = _group()
    assert 1 <= G < 2048                                                       # a group size, not the limit of n_points
    K = [1, G + 1, 2 * G + 1][k_case]
    T3 = 8
    L3s = _lengths()
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    tls = [_pattern(name, L3) for L3 in L3s]
    p = np.concatenate([np.concatenate([t, np.full((-len(t) % T3, NC_D), 0.95, np.float32)]).reshape(-1, T3, NC_D) for t in tls])
    thr, win = _points(K, name)
    dev_p = torch.from_numpy(p).cuda()
    w0, f0 = torch.from_numpy(rec_win0).cuda(), torch.from_numpy(rec_frame0).cuda()
    total = int(rec_frame0[-1])
    out = stitch_sweep(dev_p, w0, f0, total, T3, torch.from_numpy(thr).cuda(), torch.from_numpy(win).cuda(), "taper",
                       want_timeline=True)
    assert out["n_points"] == K and out["binary"] is None and int(out["err"].item()) == 0
    ev_ptr, ev_pairs = out["ev_ptr"].cpu().numpy(), out["ev_pairs"].cpu().numpy()
    n = len(L3s) * NC_D
    assert ev_ptr.shape == (K * n + 1,) and ev_ptr[0] == 0
    for k in range(K):
        one = stitch_decode(dev_p, w0, f0, total, T3, torch.from_numpy(thr[k]).cuda(), torch.from_numpy(win[k]).cuda(), "taper")
        assert int(one["err"].item()) == 0
        one_ptr, one_pairs = one["ev_ptr"].cpu().numpy(), one["ev_pairs"].cpu().numpy()
        got_ptr = ev_ptr[k * n:(k + 1) * n + 1]
        assert (got_ptr - got_ptr[0]).tobytes() == one_ptr.tobytes(), k
        assert ev_pairs[got_ptr[0]:got_ptr[-1]].tobytes() == one_pairs[:one_ptr[-1]].tobytes(), k
        assert one_ptr[-1] > 0
        if k == 0:
            assert out["timeline"].cpu().numpy().tobytes() == one["timeline"].cpu().numpy().tobytes()
    assert out["timeline"].cpu().numpy().tobytes() == np.concatenate(tls).tobytes()


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("NC,misalign", [(3, False), (12, False), (12, True)])
def test_decode_and_one_point_sweep_agree_in_both_load_paths(NC, misalign, weighting):
    """The two instantiations of the one tile kernel on the same inputs: sed_stitch_decode and sed_stitch_sweep at K = 1, in
    the scalar path (NC = 3), the 16-byte path (NC = 12) and the scalar path taken by alignment (NC = 12, posteriors and
    timeline one float off), across a tile edge, a recording shorter than a halo and a multi-tile recording."""
    T3, hop3 = 8, 3
    rec_win0, rec_frame0 = _tables(_lengths(), T3, hop3)
    rs = np.random.RandomState(7000 + 10 * NC + weighting)
    p = rs.uniform(size=(rec_win0[-1], T3, NC)).astype(np.float32)
    thr = rs.uniform(0.3, 0.7, size=NC).astype(np.float32)
    win = rs.choice([1, 5, 63], size=NC).astype(np.int32)
    one = StitchCall(p, rec_win0, rec_frame0, hop3, weighting, thr, win, misalign=misalign).run()
    swp = _Sweep(p, rec_win0, rec_frame0, hop3, weighting, thr, win, misalign=misalign).run()
    assert one["err"] == 0 and swp["err"] == 0
    n = int(one["ev_ptr"][-1])
    assert n > 0 and not np.isnan(one["timeline"]).any()
    assert one["timeline"].tobytes() == swp["timeline"].tobytes()
    assert one["ev_ptr"].tobytes() == swp["ev_ptr"].tobytes()
    assert one["ev_pairs"][:n].tobytes() == swp["ev_pairs"][:n].tobytes()


# ---- 3. decoder errors ------------------------------------------------------------------------------------------------------------------
def _alternating_sweep(K=3, **kw):
    T3, NC = 8, 3
    L3s = [9, _tile() + 3]
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    p = np.concatenate([np.resize(np.array([[0.9] * NC, [0.1] * NC], np.float32), (_n_windows(L, T3, T3) * T3, NC)).reshape(-1, T3, NC)
                        for L in L3s])
    total = K * NC * sum((L + 1) // 2 for L in L3s)
    thr, win = kw.pop("thr", np.full((K, NC), 0.5, np.float32)), kw.pop("win", np.ones((K, NC), np.int32))
    return _Sweep(p, rec_win0, rec_frame0, T3, 0, thr, win, **kw), total, rec_frame0, p


def test_capacity_one_short_over_all_points_raises_bit_2_and_writes_nothing_beyond():
    full, total, _, _ = _alternating_sweep()
    ref = full.run()
    assert ref["err"] == 0 and ref["ev_ptr"][-1] == total == full.capacity
    short, _, _, _ = _alternating_sweep(capacity=total - 1)
    got = short.run()
    assert got["err"] == 2
    np.testing.assert_array_equal(got["ev_ptr"], ref["ev_ptr"])                # still the true counts
    assert (got["ev_pairs"][total - 1:] == SENT).all()                         # nothing at or beyond capacity
    np.testing.assert_array_equal(got["ev_pairs"][:total - 1], ref["ev_pairs"][:total - 1])


@pytest.mark.parametrize("bad", [0, 64])
def test_a_window_outside_1_63_at_one_point_and_class_raises_bit_8(bad):
    win = np.ones((3, 3), np.int32)
    win[1, 2] = bad
    call, total, rec_frame0, p = _alternating_sweep(win=win)
    got = call.run()
    assert got["err"] == 8
    good = win.copy()
    good[1, 2] = 1
    tl = p.reshape(-1, 3)                                                      # hop3 = T3: the timeline is the windows in order
    tl = np.concatenate([tl[:9], tl[16:16 + _tile() + 3]])
    np.testing.assert_array_equal(got["timeline"].view(np.uint32), tl.view(np.uint32))
    want_ptr, want_pairs = _np_sweep(tl, rec_frame0, np.full((3, 3), 0.5, np.float32), good)
    per_col, want = np.diff(got["ev_ptr"]).reshape(3, 2, 3), np.diff(want_ptr).reshape(3, 2, 3).copy()
    assert (per_col[1, :, 2] == 0).all() and (want[1, :, 2] > 0).all()         # that column is not decoded ...
    want[1, :, 2] = 0
    np.testing.assert_array_equal(per_col, want)                               # ... and every other one is, exactly
    keep = np.ones(len(want_pairs), bool)
    for r in range(2):
        col = (1 * 2 + r) * 3 + 2
        keep[want_ptr[col]:want_ptr[col + 1]] = False
    np.testing.assert_array_equal(got["ev_pairs"][:got["ev_ptr"][-1]], want_pairs[keep])
    assert (got["ev_pairs"][got["ev_ptr"][-1]:] == SENT).all()


def test_malformed_and_short_tables_raise_bits_16_and_32():
    T3, NC, K = 8, 3, 2
    thr, win = np.full((K, NC), 0.5, np.float32), np.ones((K, NC), np.int32)
    p = np.full((4, T3, NC), 0.9, dtype=np.float32)
    got = _Sweep(p[:3], np.array([0, 1, 2], np.int32), np.array([0, 20, 16], np.int64), T3, 0, thr, win, capacity=64).run()
    assert got["err"] & 16                                                     # a decreasing rec_frame0
    # recording 1 needs 4 windows and is given 2: bit 32 for that recording only, at every point
    got = _Sweep(p, np.array([0, 1, 3, 4], np.int32), np.array([0, 8, 38, 46], np.int64), T3, 0, thr, win).run()
    assert got["err"] == 32
    per_col = np.diff(got["ev_ptr"]).reshape(K, 3, NC)
    assert (per_col[:, 1] == 0).all() and (per_col[:, 0] == 1).all() and (per_col[:, 2] == 1).all()
    assert np.isnan(got["timeline"][8:38]).all()
    assert (got["timeline"][:8] == np.float32(0.9)).all() and (got["timeline"][38:] == np.float32(0.9)).all()


def test_bad_host_arguments_return_bad_arg_before_any_launch():
    call, _, _, _ = _alternating_sweep()
    call.fill()
    l = call.l
    for kw, what in ((dict(n_points=0), b"n_points"), (dict(thr=None), b"null argument"),
                     (dict(ws_bytes=call.ws_bytes - 1), b"ws_bytes"), (dict(n_points=4097), b"n_points")):
        assert call.launch(**kw) == -1, kw                                     # SED_ERR_BAD_ARG
        assert b"sed_stitch_sweep:" in l.sed_last_error() and what in l.sed_last_error(), kw
    assert l.sed_stitch_sweep_ws_bytes(100, 1, 3, 0) == 0 and l.sed_stitch_sweep_ws_bytes(100, 1, 17, 2) == 0
    assert l.sed_stitch_sweep_ws_bytes(100, 1 << 20, 16, 4) == 0               # K * n_rec * NC = 2^26
    assert l.sed_stitch_sweep_ws_bytes(1 << 28, 1, 10, 2) == 0                 # total * NC >= 2^31
    torch.cuda.synchronize()
    assert (call.ev_ptr == SENT).all() and (call.ev_pairs == SENT).all() and torch.isnan(call._tl).all()
    assert int(call.err[0].item()) == 0 and (call.ws == 0xFF).all()            # nothing ran


# ---- 4. / 5. the scorers, given events -----------------------------------------------------------------------------------------------------
def _one_point(est, ref, n_rec, NC):
    """The one-point C calls on the same events: (ev, seg, ps, ev_t, seg_t, ps_t) as numpy."""
    from dcase2019_task4_amd import _lib
    l, p, dev = _lib.lib(), _lib.ptr, "cuda"
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)
    est_ptr, on, off = t(est[0], np.int64), t(np.r_[est[1], 0.0], np.float64), t(np.r_[est[2], 0.0], np.float64)
    ref_ptr, ron, roff = t(ref[0], np.int64), t(np.r_[ref[1], 0.0], np.float64), t(np.r_[ref[2], 0.0], np.float64)
    ncols, W = n_rec * NC, 2 + NC
    ev, seg, ps = (torch.full((ncols * w,), SENT, dtype=torch.int32, device=dev) for w in (3, 4, W))
    ev_t, seg_t, ps_t = (torch.zeros(NC * w, dtype=torch.int64, device=dev) for w in (3, 4, W))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.full((l.sed_long_score_ws_bytes(len(est[1]), len(ref[1]), n_rec, NC),), 0xFF, dtype=torch.uint8, device=dev)
    head = (p(est_ptr), None, 0.0, 0.0, p(on), p(off), len(est[1]), p(ref_ptr), p(ron), p(roff), len(ref[1]), n_rec, NC)
    assert l.sed_long_event_counts(*head, 0.2, 0.2, 1.0, p(ev), p(seg), p(ev_t), p(seg_t), p(err), p(ws), ws.numel(),
                                   _lib.stream_ptr()) == 0
    assert l.sed_long_psds_counts(*head, 0.5, 0.5, 0.3, p(ps), p(ps_t), p(err), p(ws), ws.numel(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (ev, seg, ps, ev_t, seg_t, ps_t)] + [int(err.item())]


@functools.lru_cache(maxsize=None)
def _score_case(name):
    """(ref_cols, [est_cols of point k], [(ev, seg, ps) of point k]): K = 3 points against ONE reference side, the oracle's
    per-column counts computed once."""
    tile = int(_l().sed_long_tile_events())
    if name == "main":
        ests = [ls.main_columns(tile, seed=k)[1] for k in range(3)]
        ref = ls.sorted_jittered_references(ests[0], 5)
    else:
        nc, seed = {"nc1": (1, 11), "nc16": (16, 12)}[name]
        ref = ls.small_columns(3, nc, seed)[0]
        ests = [ls.small_columns(3, nc, seed + 100 * k)[1] for k in range(3)]
    for est in ests:                                                           # the reference alone must not break the limit
        sizes = [ls.cluster_sizes(r, e) for rf, ef in zip(ref, est) for r, e in zip(rf, ef)]
        assert max(s[0] for s in sizes) <= 64 and max(s[1] for s in sizes) <= 64
    want = [se.set_counts(ref, est) + (np.array(psds_np.set_counts(ref, est)),) for est in ests]
    return ref, ests, want


@pytest.mark.parametrize("name", ["main", "nc1", "nc16"])
def test_sweep_scorers_are_exact_per_point_and_equal_one_point_calls(name):
    ref, ests, want = _score_case(name)
    n_rec, NC = len(ref), len(ref[0])
    raw = ScoreCall([ls.pack(e) for e in ests], ls.pack(ref), n_rec, NC)
    a = raw.run()
    assert a["err"] == 0
    for k, (ev, seg, ps) in enumerate(want):
        np.testing.assert_array_equal(a["ev"][k], ev)
        np.testing.assert_array_equal(a["seg"][k], seg)
        np.testing.assert_array_equal(a["ps"][k], ps)
        np.testing.assert_array_equal(a["ev_t"][k], ev.sum(0))
        np.testing.assert_array_equal(a["seg_t"][k], seg.sum(0))
        np.testing.assert_array_equal(a["ps_t"][k], ps.sum(0))
    if name == "main":
        assert want[0][0][1, 1, 0] > 250 and want[1][0][1, 1, 0] > 100          # the burst column was matched at every point
        assert any(not np.array_equal(want[0][i], want[1][i]) for i in range(3))
    # the bytes of three one-point calls
    for k, est in enumerate(ests):
        ev, seg, ps, ev_t, seg_t, ps_t, err = _one_point(ls.pack(est), ls.pack(ref), n_rec, NC)
        assert err == 0
        for key, one in (("ev", ev), ("seg", seg), ("ps", ps), ("ev_t", ev_t), ("seg_t", seg_t), ("ps_t", ps_t)):
            assert np.ascontiguousarray(a[key][k]).tobytes() == one.tobytes(), (k, key)
    # a second call doubles the totals and rewrites the same columns
    assert raw.launch_events() == 0 and raw.launch_psds() == 0
    b = raw.get()
    for key in ("ev", "seg", "ps"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for key in ("ev_t", "seg_t", "ps_t"):
        np.testing.assert_array_equal(b[key], 2 * a[key])


def test_python_route_on_given_events_fills_rows_from_point0():
    from dcase2019_task4_amd import metrics as M
    ref_cols, ests, want = _score_case("nc16")
    names, labels = [f"r{i}" for i in range(3)], [f"c{i}" for i in range(16)]
    mk = lambda cols: M.RefEvents(*ls.pack(cols), names, labels)
    ref, est = mk(ref_cols), [mk(e) for e in ests]
    c = M.long_sweep_event_counts_from_events(est, ref, point0=1, per_column=True)
    q = M.long_sweep_psds_counts_from_events(est, ref, point0=1, per_column=True)
    assert c.K == 4 and tuple(c.ev_columns.shape) == (3, 3, 16, 3) and tuple(q.columns.shape) == (3, 3, 16, 18)
    ev, seg = c.host()
    ps = q.host()
    assert (ev[0] == 0).all() and (ps[0] == 0).all()
    for k in range(3):
        np.testing.assert_array_equal(ev[1 + k], want[k][0].sum(0))
        np.testing.assert_array_equal(seg[1 + k], want[k][1].sum(0))
        np.testing.assert_array_equal(ps[1 + k], want[k][2].sum(0))
        np.testing.assert_array_equal(c.seg_columns[k].cpu().numpy(), want[k][1])
    with pytest.raises(ValueError):
        M.long_sweep_event_counts_from_events(est, ref, counts=M.Counts(3, 16, "cuda"), point0=1)


INSIDE = [(1.0 + k / 1024.0, 2.0) for k in range(65)]                 # 65 onsets inside one collar
ONE = [(1.01, 2.0)]


@pytest.mark.parametrize("side", ["est", "ref"])
def test_an_oversized_cluster_in_one_point_leaves_the_other_points_scored(side):
    ok_ref, ok_est = ls.spaced_column(np.random.RandomState(2), 30)
    ok_est2 = ls.spaced_column(np.random.RandomState(3), 30)[1]
    if side == "est":
        ref_cols = [[ok_ref, ONE]]
        ests = [[[ok_est, ONE]], [[ok_est2, INSIDE]], [[ok_est, ONE]]]
    else:
        ref_cols = [[ok_ref, INSIDE]]
        ests = [[[ok_est, ONE]], [[ok_est2, ONE]], [[ok_est, ONE]]]
    assert [ls.expected_err(ref_cols, e) for e in ests] == ([0, 2, 0] if side == "est" else [1, 1, 1])
    got = ScoreCall([ls.pack(e) for e in ests], ls.pack(ref_cols), 1, 2).run(psds=False)
    assert got["err"] == (2 if side == "est" else 1)
    for k, est in enumerate(ests):
        ev, seg = se.set_counts([[ok_ref]], [[est[0][0]]])
        np.testing.assert_array_equal(got["ev"][k, 0, 0], ev[0, 0])            # the healthy column, at every point
        if side == "est" and k != 1:
            ev, seg = se.set_counts(ref_cols, est)
            np.testing.assert_array_equal(got["ev"][k], ev)
            np.testing.assert_array_equal(got["seg"][k], seg)
        else:                                                                  # not scored, not truncated
            assert tuple(got["ev"][k, 0, 1]) == (0, len(ref_cols[0][1]), len(est[0][1])) and (got["seg"][k, 0, 1] == 0).all()
    ps = ScoreCall([ls.pack(e) for e in ests], ls.pack(ref_cols), 1, 2).run(events=False)
    assert ps["err"] == 0                                                      # no matching in PSDS
    for k, est in enumerate(ests):
        np.testing.assert_array_equal(ps["ps"][k], np.array(psds_np.set_counts(ref_cols, est)))


def test_scorer_bad_host_arguments_return_before_any_launch():
    cols = [[[(0.0, 1.0)]]]
    raw = ScoreCall([ls.pack(cols)] * 2, ls.pack(cols), 1, 1)
    raw.fill()
    l, p = raw.l, raw._lib.ptr
    head = list(raw._head())
    tail = [p(raw.ev_c), p(raw.seg_c), p(raw.ev_t), p(raw.seg_t), p(raw.err), p(raw.ws), raw.ws.numel(), raw._lib.stream_ptr()]
    assert l.sed_long_sweep_event_counts(*head[:13], 0, 0.2, 0.2, 1.0, *tail) == -1
    assert l.sed_long_sweep_event_counts(*head[:13], 4097, 0.2, 0.2, 1.0, *tail) == -1
    assert l.sed_long_sweep_event_counts(*head, 0.2, 0.2, 1.0, *tail[:6], 8, tail[7]) == -2
    assert l.sed_long_sweep_psds_counts(*head, 1.5, 0.5, 0.3, p(raw.ps_c), p(raw.ps_t), *tail[4:]) == -1
    assert l.sed_long_sweep_ws_bytes(10, 10, 1, 1, 0) == 0 and l.sed_long_sweep_ws_bytes(10, 10, 1 << 20, 16, 4) == 0
    assert l.sed_long_sweep_ws_bytes(10, 10, 3, 3, 1) == l.sed_long_score_ws_bytes(10, 10, 3, 3)
    got = raw.get()
    assert got["err"] == 0 and (got["ev"] == SENT).all() and (got["ps"] == SENT).all()                # nothing ran


# ---- 6. pipeline and graph -------------------------------------------------------------------------------------------------------------------
def test_sweep_pipeline_equals_the_oracle_and_replays_in_one_graph():
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import stitch_sweep
    p, rec_win0, rec_frame0, L3s, T3, NC, patterns = _stitch_inputs()
    total, n_rec = int(sum(L3s)), len(L3s)
    thresholds, windows = [0.05, 0.5, 0.95], [1]
    # the host's doubles of what each point decodes: everything active, the pattern, nothing
    est_cols = [ls.stitch_columns([np.ones_like(a) for a in patterns], NUM, DEN), ls.stitch_columns(patterns, NUM, DEN),
                ls.stitch_columns([np.zeros_like(a) for a in patterns], NUM, DEN)]
    ref_cols = ls.sorted_jittered_references(est_cols[1], 5)
    for e in est_cols:
        assert all(max(ls.cluster_sizes(r, c)) <= 64 for rf, ef in zip(ref_cols, e) for r, c in zip(rf, ef))
    want = [se.set_counts(ref_cols, e) + (np.array(psds_np.set_counts(ref_cols, e)),) for e in est_cols]
    ref = _ref_events(ref_cols)
    out = stitch_sweep(p, rec_win0, rec_frame0, total, T3, thresholds, windows, "uniform")
    assert int(out["err"].item()) == 0 and out["timeline"] is None and out["n_points"] == 3
    ev_ptr, ev_pairs = out["ev_ptr"].cpu().numpy(), out["ev_pairs"].cpu().numpy()
    for k in range(3):
        cols = [[[(int(a) * NUM / DEN, int(b) * NUM / DEN)
                  for a, b in ev_pairs[ev_ptr[(k * n_rec + r) * NC + c]:ev_ptr[(k * n_rec + r) * NC + c + 1]]]
                 for c in range(NC)] for r in range(n_rec)]
        assert cols == est_cols[k], k
    assert ev_pairs.shape[0] > ev_ptr[-1]                                      # capacity, not the true count
    c = M.long_sweep_event_counts(out, ref, 8, per_column=True)
    q = M.long_sweep_psds_counts(out, ref, 8, per_column=True)
    for k in range(3):
        np.testing.assert_array_equal(c.ev_columns[k].cpu().numpy(), want[k][0])
        np.testing.assert_array_equal(c.seg_columns[k].cpu().numpy(), want[k][1])
        np.testing.assert_array_equal(q.columns[k].cpu().numpy(), want[k][2])
    eager = (c.buf.cpu().numpy().copy(), q.buf.cpu().numpy().copy(), ev_ptr.copy(), ev_pairs[:ev_ptr[-1]].copy())
    ev, seg = c.host()
    for k in range(3):
        np.testing.assert_array_equal(ev[k], want[k][0].sum(0))
        np.testing.assert_array_equal(seg[k], want[k][1].sum(0))
        np.testing.assert_array_equal(q.host()[k], want[k][2].sum(0))
    # ONE capture of the three calls on one stream, replayed onto sentinels
    thr = torch.tensor(thresholds, device="cuda").reshape(3, 1).repeat(1, NC).contiguous()
    win = torch.ones(3, NC, dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = stitch_sweep(p, rec_win0, rec_frame0, total, T3, thr, win, "uniform")
        c_g = M.long_sweep_event_counts(out_g, ref, 8, per_column=True)
        q_g = M.long_sweep_psds_counts(out_g, ref, 8, per_column=True)
    for t in (out_g["ev_ptr"], out_g["ev_pairs"], c_g.ev_columns, c_g.seg_columns, q_g.columns):
        t.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert c_g.buf.cpu().numpy().tobytes() == eager[0].tobytes() and q_g.buf.cpu().numpy().tobytes() == eager[1].tobytes()
    g_ptr = out_g["ev_ptr"].cpu().numpy()
    assert g_ptr.tobytes() == eager[2].tobytes()
    assert out_g["ev_pairs"].cpu().numpy()[:g_ptr[-1]].tobytes() == eager[3].tobytes()
    assert (out_g["ev_pairs"].cpu().numpy()[g_ptr[-1]:] == SENT).all()
    for k in range(3):
        np.testing.assert_array_equal(c_g.ev_columns[k].cpu().numpy(), want[k][0])
        np.testing.assert_array_equal(q_g.columns[k].cpu().numpy(), want[k][2])


# ---- 7. validate_long ---------------------------------------------------------------------------------------------------------------------------
def test_validate_long_one_blend_equals_the_loop_and_the_oracle():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions, long_window_posteriors, stitch_sweep
    from dcase2019_task4_amd.longrec import sweep_chunks
    labels = [f"c{i}" for i in range(10)]
    model, _ = gu.make_model(0)
    model.eval()
    rs = np.random.RandomState(21)
    feats = [(np.abs(rs.standard_normal((L, 64))) ** 2 * np.exp(rs.uniform(-6, 2, (L, 1))) + 1e-6).astype(np.float32)
             for L in (40, 64, 900)]
    names = ["a.wav", "b.wav", "c.wav"]
    lset = LongRecordingSet.from_arrays(feats, 64, scaler=_Scaler(64), filenames=names)
    _, timelines, _ = get_long_predictions(model, lset, labels, batch_size=8, return_posteriors=True)
    tl = torch.cat(timelines).cpu().numpy()
    points = [(np.median(tl, axis=0).astype(np.float32), [3, 1, 5, 3, 3, 7, 3, 1, 3, 5]), (float(np.quantile(tl, 0.6)), 1),
              (float(np.quantile(tl, 0.8)), 5)]
    K = len(points)
    dfs = [get_long_predictions(model, lset, labels, batch_size=8, threshold=t, median_window=w) for t, w in points]
    cols = [se.columns_from_rows(df[["event_label", "onset", "offset", "filename"]].itertuples(index=False), names, labels)
            for df in dfs]
    assert all(len(df) > 5 for df in dfs)
    ref_cols = ls.sorted_jittered_references(cols[0], 6)
    ref = M.RefEvents.from_dataframe(se.to_dataframe(ref_cols, names, labels), names, labels)
    thr, win = [p[0] for p in points], [p[1] for p in points]
    cap = lset.capacity(10)
    small = 8 * cap * 2                                                        # two points per chunk: two chunks of K = 3
    assert len(sweep_chunks(K, cap, 1 << 30)) == 1 and len(sweep_chunks(K, cap, small)) == 2
    runs = {}
    for name, kw in (("loop", dict(one_blend=False)), ("one", dict(one_blend=True)),
                     ("chunks", dict(one_blend=True, max_table_bytes=small))):
        psds = M.PSDSCounts(K, 10, "cuda")
        runs[name] = (M.validate_long(model, lset, ref, thr, win, batch_size=8, psds=psds, **kw), psds.host())
    for k in range(K):
        ev, seg = se.set_counts(ref_cols, cols[k])
        ps = np.array(psds_np.set_counts(ref_cols, cols[k]))
        want_e, want_s = M.EventMetrics(labels, ev.sum(0)), M.SegmentMetrics(labels, seg.sum(0))
        for name, (res, totals) in runs.items():
            assert res[k][0].class_wise == want_e.class_wise and res[k][1].class_wise == want_s.class_wise, (name, k)
            assert res[k][1].Ntn == want_s.Ntn, (name, k)
            np.testing.assert_array_equal(totals[k], ps.sum(0))
    assert runs["loop"][1].tobytes() == runs["one"][1].tobytes() == runs["chunks"][1].tobytes()
    # a decoder error (capacity forced small) reaches host() without a synchronisation of its own
    win_strong = long_window_posteriors(model, lset, 10, 8)
    out = stitch_sweep(win_strong, lset.rec_win0, lset.rec_frame0, lset.total_frames, lset.hop3, thr, win, capacity=3)
    c = M.long_sweep_event_counts(out, ref, 8)
    with pytest.raises(_lib.SedError, match="decoded event table is invalid"):
        c.host()
    with pytest.raises(_lib.SedError, match="sed_long_sweep_psds_counts.*decoded event table"):
        M.long_sweep_psds_counts(out, ref, 8).host()
    with pytest.raises(ValueError):
        M.validate_long(model, lset, ref, [0.5, [0.1, 0.2]], [1], one_blend=True)
