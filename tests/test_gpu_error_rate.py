"""-m gpu tests of the overall error rate with substitutions: sed_error_counts, sed_long_error_counts and
sed_long_sweep_error_counts EXACT against the plain-loop statement tests/error_rate_np.py (integers: no tolerance), against the
existing class-wise calls on the same events under one label, and end to end through validate / validate_long.
tests/test_error_rate_cpu.py confirms on the statement that every case here but the deliberate ones stays within 64 events
per side and merged cluster (tests/error_rate_cases.py builds them without a GPU)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import postprocess_np as pp
from tests import error_rate_cases as ec
from tests import error_rate_np as er
from tests import gpu_util as gu
from tests import long_score_np as ls
from tests import sed_eval_np as se
from tests.long_util import SENT, TAIL, ScoreCall, _ref_events, _Scaler

pytestmark = pytest.mark.gpu


def _tile():
    from dcase2019_task4_amd import _lib
    return int(_lib.lib().sed_long_tile_events())


@functools.lru_cache(maxsize=None)
def _clip_case(nclass):
    ref, est = ec.clip_events(nclass)
    return ref, est, er.set_overall(ref, est)


@functools.lru_cache(maxsize=None)
def _long_case():
    ref, est = ec.long_events(_tile())
    return ref, est, er.set_overall(ref, est)


def _np(t):
    return t.cpu().numpy()


def _check_files(counts, want, k=None):
    ev, seg = _np(counts.ev_files), _np(counts.seg_files)
    if k is not None:
        ev, seg = ev[k], seg[k]
    np.testing.assert_array_equal(ev, want[0])
    np.testing.assert_array_equal(seg, want[1])


# ---- clips ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nclass", ec.CLIP_CLASSES)
def test_clips_given_events_equal_the_statement_and_the_class_wise_call_under_one_label(nclass):
    from dcase2019_task4_amd import metrics as M
    ref_cols, est_cols, want = _clip_case(nclass)
    ref, est = _ref_events(ref_cols), _ref_events(est_cols)
    c = M.error_counts_from_events(est, ref, per_file=True)
    _check_files(c, want, 0)
    ev_t, seg_t = c.host()
    np.testing.assert_array_equal(ev_t[0], want[0].sum(0))
    np.testing.assert_array_equal(seg_t[0], want[1].sum(0))
    # on the device alone: Nany is the class-wise Ntp of the same events under ONE label ...
    one = M.event_counts_from_events(_ref_events(ec.one_class(est_cols)), _ref_events(ec.one_class(ref_cols)), per_column=True)
    one_ev = _np(one.ev_columns)[0, :, 0]                             # [clip, (Ntp, Nref, Nsys)]
    one.check()
    np.testing.assert_array_equal(_np(c.ev_files)[0], one_ev[:, [1, 2, 0]])
    # ... and against the class-wise call on the same inputs: Ntp <= Nany, the two segment identities, Nref and Nsys
    cls = M.event_counts_from_events(est, ref, per_column=True)
    cls_ev, cls_seg = _np(cls.ev_columns)[0].sum(1), _np(cls.seg_columns)[0].sum(1)      # [clip, .] over the classes
    cls.check()
    ours_ev, ours_seg = _np(c.ev_files)[0], _np(c.seg_files)[0]
    np.testing.assert_array_equal(ours_ev[:, :2], cls_ev[:, 1:])
    assert (cls_ev[:, 0] <= ours_ev[:, 2]).all() and (ours_ev[:, 2] <= ours_ev[:, :2].min(1)).all()
    np.testing.assert_array_equal(ours_seg[:, 0] + ours_seg[:, 1], cls_seg[:, 2])        # S + D = sum Nfn
    np.testing.assert_array_equal(ours_seg[:, 0] + ours_seg[:, 2], cls_seg[:, 1])        # S + I = sum Nfp
    if nclass == 1:
        np.testing.assert_array_equal(ours_ev[:, 2], cls_ev[:, 0])                       # Nany = Ntp
        assert (ours_seg[:, 0] == 0).all()
    else:
        assert (ours_ev[:, 2] - cls_ev[:, 0]).sum() > 0 and ours_seg[:, 0].sum() > 0     # there are substitutions
    # other collars and a finer segment grid
    kw = dict(t_collar=0.5, percentage_of_length=0.5)
    c2 = M.error_counts_from_events(est, ref, time_resolution=0.25, per_file=True, **kw)
    _check_files(c2, er.set_overall(ref_cols, est_cols, res=0.25, **kw), 0)
    c2.check()


@pytest.mark.parametrize("nclass", ec.CLIP_CLASSES)
def test_clips_decoded_at_two_operating_points_equal_the_statement_and_batches_accumulate(nclass):
    from dcase2019_task4_amd import metrics as M
    post, ref_cols, ests = ec.decoded_case(nclass)
    ref = _ref_events(ref_cols)
    dev = torch.from_numpy(post).cuda()
    thr, win = [p[0] for p in ec.POINTS], [p[1] for p in ec.POINTS]
    c = M.error_counts(dev, ref, thr, win, ec.PTR, per_file=True)
    wants = [er.set_overall(ref_cols, e) for e in ests]
    for k, want in enumerate(wants):
        _check_files(c, want, k)
    ev_t, seg_t = c.host()
    np.testing.assert_array_equal(ev_t, np.stack([w[0].sum(0) for w in wants]))
    np.testing.assert_array_equal(seg_t, np.stack([w[1].sum(0) for w in wants]))
    assert sum(w[0][:, 2].sum() for w in wants) > 0
    # one point alone == its row of the sweep; clip by clip into one set of totals == the batch; a second pass doubles them
    one = M.error_counts(dev, ref, thr[1:], win[1:], ec.PTR, per_file=True)
    assert torch.equal(one.ev_files[0], c.ev_files[1]) and torch.equal(one.ev[0], c.ev[1]) and torch.equal(one.seg[0], c.seg[1])
    chained = None
    for i in range(ec.N_CLIPS):
        chained = M.error_counts(dev[i:i + 1], ref, thr, win, ec.PTR, clip_offset=i, counts=chained)
    assert torch.equal(chained.buf, c.buf)
    M.error_counts(dev, ref, thr, win, ec.PTR, counts=chained)
    assert torch.equal(chained.buf[:-1], 2 * c.buf[:-1])
    # under one label the class-wise decode is another decode (the union is not the per-class decode): only given events
    # serve that comparison (the test above); here the class-wise call pins Nref / Nsys and the identities
    cls = M.event_counts(dev, ref, thr, win, ec.PTR)
    ev_c, seg_c = cls.host()
    np.testing.assert_array_equal(ev_t[:, :2], ev_c[:, :, 1:].sum(1))
    np.testing.assert_array_equal(seg_t[:, 0] + seg_t[:, 1], seg_c[:, :, 2].sum(1))
    np.testing.assert_array_equal(seg_t[:, 0] + seg_t[:, 2], seg_c[:, :, 1].sum(1))
    assert (ev_c[:, :, 0].sum(1) <= ev_t[:, 2]).all()


def test_a_merged_cluster_of_64_is_scored_and_one_of_65_raises_without_touching_the_other_clips():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    ref_cols, est_cols = ec.chain_case(64)
    c = M.error_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols), per_file=True)
    want = er.set_overall(ref_cols, est_cols)
    _check_files(c, want, 0)
    c.check()
    assert tuple(want[0][1]) == (64, 64, 64)
    for n_ref, n_est, bit, text in ((65, 64, 1, "more than 64 reference events"), (64, 65, 2, "more than 64 estimated events")):
        ref_cols, est_cols = ec.chain_case(n_ref, n_est)
        c = M.error_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols), per_file=True)
        assert int(c.err[0].item()) == bit
        with pytest.raises(_lib.SedError, match=text + ".*merged"):
            c.host()
        want = er.set_overall(ref_cols, est_cols)
        ev, seg = _np(c.ev_files)[0], _np(c.seg_files)[0]
        for clip in (0, 2):
            np.testing.assert_array_equal(ev[clip], want[0][clip])
            np.testing.assert_array_equal(seg[clip], want[1][clip])
        assert tuple(ev[1]) == (n_ref, n_est, 0) and tuple(seg[1]) == (0, 0, 0)           # not scored, not truncated
        # the class-wise call has no quarrel with these columns
        M.event_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols)).check()


def test_the_clip_call_writes_only_its_outputs_and_replays_in_a_graph():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    post, ref_cols, ests = ec.decoded_case(3)
    ref = _ref_events(ref_cols)
    dev = torch.from_numpy(post).cuda()
    thr, win = M.operating_points([p[0] for p in ec.POINTS], [p[1] for p in ec.POINTS], "cuda")
    K, N = 2, ec.N_CLIPS
    ev_f = torch.full((K * N * 3 + TAIL,), SENT, dtype=torch.int32, device="cuda")
    seg_f = torch.full((K * N * 3 + TAIL,), SENT, dtype=torch.int32, device="cuda")
    tot = torch.full((2 * K * 3 + TAIL,), SENT, dtype=torch.int64, device="cuda")
    tot[:2 * K * 3].zero_()
    err = torch.tensor([0, SENT], dtype=torch.int32, device="cuda")
    p, l = _lib.ptr, _lib.lib()
    args = (p(dev), N, ec.T, 3, K, p(thr), p(win), float(ec.PTR), ec.SR / ec.HOP, None, None, None, p(ref.ptr), p(ref.onset),
            p(ref.offset), 0.2, 0.2, 1.0)
    assert l.sed_error_counts(*args, p(ev_f), p(seg_f), p(tot), p(tot[K * 3:]), p(err), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    wants = [er.set_overall(ref_cols, e) for e in ests]
    np.testing.assert_array_equal(_np(ev_f)[:K * N * 3].reshape(K, N, 3), np.stack([w[0] for w in wants]))
    np.testing.assert_array_equal(_np(seg_f)[:K * N * 3].reshape(K, N, 3), np.stack([w[1] for w in wants]))
    assert (_np(ev_f)[K * N * 3:] == SENT).all() and (_np(seg_f)[K * N * 3:] == SENT).all() and (_np(tot)[2 * K * 3:] == SENT).all()
    assert _np(err).tolist() == [0, SENT]
    # bad host arguments return before any launch
    assert l.sed_error_counts(*args[:15], -0.1, 0.2, 1.0, None, None, p(tot), p(tot[K * 3:]), p(err), _lib.stream_ptr()) == -1
    assert l.sed_error_counts(*args, None, None, None, p(tot[K * 3:]), p(err), _lib.stream_ptr()) == -1
    assert l.sed_error_counts(*args[:3], 17, *args[4:], None, None, p(tot), p(tot[K * 3:]), p(err), _lib.stream_ptr()) == -1
    # two calls and one graph replay: identical bytes
    eager = M.error_counts(dev, ref, thr, win, ec.PTR)
    again = M.error_counts(dev, ref, thr, win, ec.PTR)
    assert torch.equal(eager.buf, again.buf)
    counts = M.ErrorCounts(K, 3, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.error_counts(dev, ref, thr, win, ec.PTR, counts=counts)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.error_counts(dev, ref, thr, win, ec.PTR, counts=counts)
    for _ in range(2):
        counts.buf.zero_()
        graph.replay()
        assert torch.equal(counts.buf, eager.buf)
    np.testing.assert_array_equal(_np(eager.buf)[:K * 3].reshape(K, 3), _np(tot)[:K * 3].reshape(K, 3))


# ---- long recordings ------------------------------------------------------------------------------------------------------------
class ErrorCall(ScoreCall):
    """``ScoreCall``'s inputs for sed_long_error_counts / sed_long_sweep_error_counts: sentinel-filled outputs with a tail that
    must come back untouched, a 0xFF workspace of exactly the size the library asks for."""

    def __init__(self, est, ref, n_rec, NC, **kw):
        super().__init__(est, ref, n_rec, NC, **kw)
        K = self.K
        mk = lambda n, dt: torch.empty(n + TAIL, dtype=dt, device="cuda")
        self.o_ev, self.o_seg = mk(K * n_rec * 3, torch.int32), mk(K * n_rec * 3, torch.int32)
        self.o_ev_t, self.o_seg_t = mk(K * 3, torch.int64), mk(K * 3, torch.int64)
        fn = self.l.sed_long_sweep_error_ws_bytes if self.sweep else self.l.sed_long_error_ws_bytes
        nbytes = fn(self.est_cap, self.ref_cap, n_rec, NC, *self.lead)
        assert nbytes > 0, self.l.sed_last_error()
        self.ews = torch.empty(nbytes + TAIL, dtype=torch.uint8, device="cuda")

    def fill_error(self):
        for t in (self.o_ev, self.o_seg):
            t.fill_(SENT)
        for t in (self.o_ev_t, self.o_seg_t):
            t.fill_(SENT)
            t[:self.K * 3].zero_()
        self.err.fill_(SENT)
        self.err[:1].zero_()
        self.ews.fill_(0xFF)

    def launch_error(self, t_collar=0.2, pct=0.2, res=1.0, files=True, ws_bytes=None):
        p = self._lib.ptr
        fn = self.l.sed_long_sweep_error_counts if self.sweep else self.l.sed_long_error_counts
        return fn(*self._head(), float(t_collar), float(pct), float(res), p(self.o_ev) if files else None,
                  p(self.o_seg) if files else None, p(self.o_ev_t), p(self.o_seg_t), p(self.err), p(self.ews),
                  self.ews.numel() - TAIL if ws_bytes is None else ws_bytes, self._lib.stream_ptr())

    def get_error(self):
        torch.cuda.synchronize()
        K, n_rec, out = self.K, self.n_rec, {}
        for name, t, n, shape in (("ev", self.o_ev, K * n_rec * 3, (n_rec, 3)), ("seg", self.o_seg, K * n_rec * 3, (n_rec, 3)),
                                  ("ev_t", self.o_ev_t, K * 3, (3,)), ("seg_t", self.o_seg_t, K * 3, (3,))):
            h = t.cpu().numpy()
            assert (h[n:] == SENT).all(), name
            out[name] = h[:n].reshape(self.lead + shape)
        assert int(self.err[1].item()) == SENT and (self.ews[-TAIL:] == 0xFF).all()
        out["err"] = int(self.err[0].item())
        return out

    def run_error(self, **kw):
        self.fill_error()
        assert self.launch_error(**kw) == 0, self.l.sed_last_error()
        return self.get_error()


def _check_long(got, want):
    assert got["err"] == 0
    np.testing.assert_array_equal(got["ev"], want[0])
    np.testing.assert_array_equal(got["seg"], want[1])
    np.testing.assert_array_equal(got["ev_t"], want[0].sum(0))
    np.testing.assert_array_equal(got["seg_t"], want[1].sum(0))


def test_long_given_seconds_equal_the_statement_twice_and_accumulate():
    """3 recordings x 4 classes: one empty, middle classes empty, equal onsets across classes, a column of 300 events, a
    merged cluster across the edge between two tiles of references."""
    from dcase2019_task4_amd import metrics as M
    ref_cols, est_cols, want = _long_case()
    raw = ErrorCall(ls.pack(est_cols), ls.pack(ref_cols), 3, ec.LONG_CLASSES)
    a = raw.run_error()
    _check_long(a, want)
    assert tuple(a["ev"][1]) == (0, 0, 0) and a["ev"][0, 0] > 300 and (a["seg"][:, 0] > 0).any()
    b = raw.run_error()
    for k in ("ev", "seg", "ev_t", "seg_t"):
        assert a[k].tobytes() == b[k].tobytes(), k
    raw.fill_error()                                                  # totals accumulate; NULL per-file outputs
    assert raw.launch_error(files=False) == 0 and raw.launch_error(files=False) == 0
    c = raw.get_error()
    np.testing.assert_array_equal(c["ev_t"], 2 * want[0].sum(0))
    np.testing.assert_array_equal(c["seg_t"], 2 * want[1].sum(0))
    assert (c["ev"] == SENT).all() and (c["seg"] == SENT).all()
    # on the device alone: Nany is sed_long_event_counts' Ntp of the same events under ONE label; identities; Nref / Nsys
    ref, est = _ref_events(ref_cols), _ref_events(est_cols)
    one = M.long_event_counts_from_events(_ref_events(ec.one_class(est_cols)), _ref_events(ec.one_class(ref_cols)), per_column=True)
    one.check()
    np.testing.assert_array_equal(a["ev"], _np(one.ev_columns)[:, 0][:, [1, 2, 0]])
    cls = M.long_event_counts_from_events(est, ref, per_column=True)
    cls.check()
    cls_ev, cls_seg = _np(cls.ev_columns).sum(1), _np(cls.seg_columns).sum(1)
    np.testing.assert_array_equal(a["ev"][:, :2], cls_ev[:, 1:])
    assert (cls_ev[:, 0] <= a["ev"][:, 2]).all() and (a["ev"][:, 2] - cls_ev[:, 0]).sum() > 10
    np.testing.assert_array_equal(a["seg"][:, 0] + a["seg"][:, 1], cls_seg[:, 2])
    np.testing.assert_array_equal(a["seg"][:, 0] + a["seg"][:, 2], cls_seg[:, 1])
    # the Python route, other criteria
    kw = dict(t_collar=0.5, percentage_of_length=0.5)
    c2 = M.long_error_from_events(est, ref, time_resolution=0.25, per_file=True, point=1, **kw)
    want2 = er.set_overall(ref_cols, est_cols, res=0.25, **kw)
    assert max(max(er.merged_cluster_sizes(r, e, 0.5)) for r, e in zip(ref_cols, est_cols)) <= 64
    _check_files(c2, want2)
    ev_t, seg_t = c2.host()
    np.testing.assert_array_equal(ev_t[1], want2[0].sum(0))
    assert (ev_t[0] == 0).all() and (seg_t[0] == 0).all()


def test_long_one_class_gives_nany_equal_ntp():
    from dcase2019_task4_amd import metrics as M
    ref_cols, est_cols = ls.small_columns(3, 1, 11)
    assert max(max(er.merged_cluster_sizes(r, e)) for r, e in zip(ref_cols, est_cols)) <= 64
    c = M.long_error_from_events(_ref_events(est_cols), _ref_events(ref_cols), per_file=True)
    cls = M.long_event_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols), per_column=True)
    c.check(), cls.check()
    np.testing.assert_array_equal(_np(c.ev_files), _np(cls.ev_columns)[:, 0][:, [1, 2, 0]])
    _check_files(c, er.set_overall(ref_cols, est_cols))
    assert (_np(c.seg_files)[:, 0] == 0).all()


def test_long_frames_mode_equals_the_statement_on_the_hosts_doubles_and_replays_in_a_graph():
    from dcase2019_task4_amd import metrics as M
    ptr, pairs, est_cols = ec.frame_table()
    ref_cols = ec.frame_references(est_cols)
    want = er.set_overall(ref_cols, est_cols)
    pairs_dev = torch.cat([torch.from_numpy(pairs), torch.full((37, 2), SENT, dtype=torch.int32)]).cuda()   # capacity > count
    raw = ErrorCall((ptr, pairs_dev, ec.NUM, ec.DEN), ls.pack(ref_cols), 3, ec.LONG_CLASSES)
    assert raw.est_cap == len(pairs) + 37
    _check_long(raw.run_error(), want)
    ref = _ref_events(ref_cols)
    decoded = {"ev_ptr": torch.from_numpy(ptr).cuda(), "ev_pairs": pairs_dev, "err": torch.zeros(2, dtype=torch.int32, device="cuda")}
    eager = M.long_error_counts(decoded, ref, ec.PTR, per_file=True)
    _check_files(eager, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = M.long_error_counts(decoded, ref, ec.PTR, per_file=True)
    for _ in range(2):
        g.buf.zero_()
        g.ev_files.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert _np(g.buf).tobytes() == _np(eager.buf).tobytes()
        assert torch.equal(g.ev_files, eager.ev_files) and torch.equal(g.seg_files, eager.seg_files)
    np.testing.assert_array_equal(eager.host()[0][0], want[0].sum(0))
    # a decoder error reaches host() through the error word
    decoded["err"][0] = 1
    with pytest.raises(Exception, match="decoded event table is invalid"):
        M.long_error_counts(decoded, ref, ec.PTR).host()


def test_long_error_bits_a_decreasing_onset_and_a_merged_cluster_of_65():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    rs = np.random.RandomState(2)
    ok_ref, ok_est = ls.spaced_column(rs, 30)
    ok = ([[ok_ref, []]], [[[], ok_est]])                             # every detection under the other label
    want_ok = er.set_overall(*ok)
    assert want_ok[0][0, 2] > 10 and want_ok[1][0, 0] > 10            # substitutions only: every match crosses the labels
    bad_ref, bad_est = [[(2.0, 3.0), (1.0, 1.5)], [(1.2, 2.0)]], [[(1.01, 2.0)], []]
    for swap in (False, True):
        r, e = (bad_est, bad_ref) if swap else (bad_ref, bad_est)
        ref_cols, est_cols = ok[0] + [r], ok[1] + [e]
        got = ErrorCall(ls.pack(est_cols), ls.pack(ref_cols), 2, 2).run_error()
        assert got["err"] == 64
        np.testing.assert_array_equal(got["ev"][0], want_ok[0][0])
        np.testing.assert_array_equal(got["seg"][0], want_ok[1][0])
        assert tuple(got["ev"][1]) == (len(r[0]) + len(r[1]), len(e[0]) + len(e[1]), 0) and tuple(got["seg"][1]) == (0, 0, 0)
        with pytest.raises(_lib.SedError, match="onsets decrease"):
            M.long_error_from_events(_ref_events(est_cols), _ref_events(ref_cols)).host()
    # 65 references inside one collar, spread over two classes: no class-wise cluster is over the limit, the merged one is
    many = [(1.0 + k / 1024.0, 2.0) for k in range(65)]
    ref_cols, est_cols = ok[0] + [[many[:33], many[33:]]], ok[1] + [[[(1.01, 2.0)], []]]
    assert er.merged_cluster_sizes(ref_cols[1], est_cols[1]) == (65, 1) and ls.expected_err(ref_cols, est_cols) == 0
    got = ErrorCall(ls.pack(est_cols), ls.pack(ref_cols), 2, 2).run_error()
    assert got["err"] == 1 and tuple(got["ev"][1]) == (65, 1, 0)
    np.testing.assert_array_equal(got["ev"][0], want_ok[0][0])
    with pytest.raises(_lib.SedError, match="more than 64 reference events, all classes merged"):
        M.long_error_from_events(_ref_events(est_cols), _ref_events(ref_cols)).host()
    M.long_event_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols)).check()
    # malformed offsets stay inside the arrays (bit 16); bad host arguments return before any launch
    good = ls.pack(ok[0])
    raw = ErrorCall((np.array([0, 5, 3], np.int64), good[1], good[2]), good, 1, 2)
    assert raw.run_error()["err"] == 16
    raw = ErrorCall(ls.pack(ok[1]), good, 1, 2)
    raw.fill_error()
    assert raw.launch_error(t_collar=-0.1) == -1 and raw.launch_error(res=0.0) == -1
    assert raw.launch_error(ws_bytes=raw.l.sed_long_score_ws_bytes(raw.est_cap, raw.ref_cap, 1, 2)) == -2
    got = raw.get_error()
    assert got["err"] == 0 and (got["ev"] == SENT).all() and (got["ev_t"] == 0).all()


@pytest.mark.parametrize("K", [1, 9])
def test_sweep_is_byte_identical_to_k_one_point_calls_and_equals_the_statement(K):
    """K = 9 is past one group of 8 points.  (The reference side is merged once: tests/test_error_rate_cpu.py pins that the
    workspace K points add does not depend on the reference events.)"""
    from dcase2019_task4_amd import metrics as M
    ref_cols, ests = ec.sweep_events(K, _tile())
    ref_p = ls.pack(ref_cols)
    sweep = ErrorCall([ls.pack(e) for e in ests], ref_p, 3, ec.LONG_CLASSES).run_error()
    assert sweep["err"] == 0 and sweep["ev"].shape == (K, 3, 3)
    for k, e in enumerate(ests):
        one = ErrorCall(ls.pack(e), ref_p, 3, ec.LONG_CLASSES).run_error()
        for name in ("ev", "seg", "ev_t", "seg_t"):
            assert one[name].tobytes() == sweep[name][k].tobytes(), (name, k)
        if k in (0, K - 1):
            want = er.set_overall(ref_cols, e)
            np.testing.assert_array_equal(sweep["ev"][k], want[0])
            np.testing.assert_array_equal(sweep["seg"][k], want[1])
    # the Python route into rows point0 ..
    ref = _ref_events(ref_cols)
    c = M.long_sweep_error_from_events([_ref_events(e) for e in ests], ref, point0=1, per_file=True)
    np.testing.assert_array_equal(_np(c.ev_files).reshape(K, 3, 3), sweep["ev"])
    ev_t, seg_t = c.host()
    np.testing.assert_array_equal(ev_t[1:], sweep["ev_t"])
    np.testing.assert_array_equal(seg_t[1:], sweep["seg_t"])
    assert (ev_t[0] == 0).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
class _DS:
    def __init__(self, x):
        self.x = x
        self.filenames = pd.Series([f"clip_{i}.wav" for i in range(len(x))])

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(1)


class _Enc:
    def __init__(self, labels):
        self.labels = labels

    def decode_strong(self, m):
        return pp.decode_strong(m, self.labels)


def _want_rates(labels, ref_cols, est_cols):
    """(event error_rate dict, segment error_rate dict) from the two statements."""
    ev, seg = se.set_counts(ref_cols, est_cols)
    ev_o, seg_o = er.set_overall(ref_cols, est_cols)
    assert max(max(er.merged_cluster_sizes(r, e)) for r, e in zip(ref_cols, est_cols)) <= 64
    keys = ("error_rate", "substitution_rate", "deletion_rate", "insertion_rate")
    nref, nsys, nany = (int(v) for v in ev_o.sum(0))
    ntp = int(ev[:, :, 0].sum())
    S, D, I = (int(v) for v in seg_o.sum(0))
    return (dict(zip(keys, er.rates(nref, nany - ntp, nref - nany, nsys - nany))),
            dict(zip(keys, er.rates(int(seg[:, :, 0].sum() + seg[:, :, 2].sum()), S, D, I))))


def _same(got, want):
    return all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in want) and set(got) == set(want)


def test_validate_reports_the_overall_error_rate_of_the_statement_on_get_predictions():
    from dcase2019_task4_amd.inference import get_predictions
    from dcase2019_task4_amd.metrics import RefEvents, compute_strong_metrics, validate
    N, T = 5, 160
    rs = np.random.RandomState(4)
    xs = []
    for k in range(N):
        gain = np.repeat(rs.choice([0.02, 1.0, 30.0], size=(T + 15) // 16), 16)[:T]          # level steps: posteriors that move
        xs.append(torch.tensor((rs.standard_normal((1, T, 64)) * gain[None, :, None]).astype(np.float32)))
    ds = _DS(xs)
    model, _ = gu.make_model(0)
    model.eval()
    files, labels = ds.filenames.tolist(), [f"c{i}" for i in range(10)]
    with torch.no_grad():
        post = model(torch.stack(xs).cuda())[0]
    thr = float(post.median())
    df = get_predictions(model, ds, _Enc(labels).decode_strong, ec.PTR, batch_size=2, threshold=thr)
    est_cols = se.columns_from_rows(df[["event_label", "onset", "offset", "filename"]].itertuples(index=False), files, labels)
    assert sum(len(c) for f in est_cols for c in f) > 10
    rs2 = np.random.RandomState(5)
    ref_cols = [ec.estimate_of(f, rs2, 10, 3.0) for f in est_cols]
    valid_df = se.to_dataframe(ref_cols, files, labels)
    ref = RefEvents.from_dataframe(valid_df, files, labels)
    want_e, want_s = _want_rates(labels, ref_cols, est_cols)
    assert want_e["substitution_rate"] > 0 and want_s["substitution_rate"] > 0
    [(ev_m, seg_m)] = validate(model, ds, ref, ec.PTR, (thr,), batch_size=2, error_rate=True)
    assert _same(ev_m.results_overall_metrics()["error_rate"], want_e)
    assert _same(seg_m.results_overall_metrics()["error_rate"], want_s)
    assert "Overall error rate" in str(ev_m) and "Overall error rate" in str(seg_m)
    [(ev_0, seg_0)] = validate(model, ds, ref, ec.PTR, (thr,), batch_size=2)
    for m in (ev_0, seg_0):
        assert all(np.isnan(v) for v in m.results_overall_metrics()["error_rate"].values()) and "Overall error rate" not in str(m)
    assert ev_0.class_wise == ev_m.class_wise and seg_0.class_wise == seg_m.class_wise
    # the DataFrame route knows the classes of its two tables only: the overall rates do not depend on that
    df_m = compute_strong_metrics(df, valid_df, error_rate=True)
    assert _same(df_m.results_overall_metrics()["error_rate"], want_e)
    assert all(np.isnan(v) for v in compute_strong_metrics(df, valid_df).results_overall_metrics()["error_rate"].values())


@pytest.mark.parametrize("one_blend", [True, False])
def test_validate_long_reports_the_overall_error_rate_at_every_point(one_blend):
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions
    labels = [f"c{i}" for i in range(10)]
    model, _ = gu.make_model(0)
    model.eval()
    rs = np.random.RandomState(21)
    feats = [(np.abs(rs.standard_normal((L, 64))) ** 2 * np.exp(rs.uniform(-6, 2, (L, 1))) + 1e-6).astype(np.float32)
             for L in (40, 64, 300)]
    names = ["a.wav", "b.wav", "c.wav"]
    lset = LongRecordingSet.from_arrays(feats, 64, scaler=_Scaler(64), filenames=names)
    _, timelines, _ = get_long_predictions(model, lset, labels, batch_size=8, return_posteriors=True)
    tl = torch.cat(timelines).cpu().numpy()
    points = [(float(np.median(tl)), 3), (float(np.quantile(tl, 0.6)), 1)]
    dfs = [get_long_predictions(model, lset, labels, batch_size=8, threshold=t, median_window=w) for t, w in points]
    cols = [se.columns_from_rows(df[["event_label", "onset", "offset", "filename"]].itertuples(index=False), names, labels)
            for df in dfs]
    assert all(len(df) > 5 for df in dfs)
    rs2 = np.random.RandomState(6)
    ref_cols = [[sorted(c) for c in ec.estimate_of(f, rs2, 10, 10.0)] for f in cols[0]]
    ref = M.RefEvents.from_dataframe(se.to_dataframe(ref_cols, names, labels), names, labels)
    kw = dict(batch_size=8, one_blend=one_blend)
    res = M.validate_long(model, lset, ref, [p[0] for p in points], [p[1] for p in points], error_rate=True, **kw)
    plain = M.validate_long(model, lset, ref, [p[0] for p in points], [p[1] for p in points], **kw)
    for k in range(2):
        want_e, want_s = _want_rates(labels, ref_cols, cols[k])
        assert _same(res[k][0].results_overall_metrics()["error_rate"], want_e), k
        assert _same(res[k][1].results_overall_metrics()["error_rate"], want_s), k
        assert res[k][0].class_wise == plain[k][0].class_wise and res[k][1].class_wise == plain[k][1].class_wise
        for m in plain[k]:
            assert all(np.isnan(v) for v in m.results_overall_metrics()["error_rate"].values())
    assert _want_rates(labels, ref_cols, cols[0])[0]["substitution_rate"] > 0
    # with the weak tags in the same copy
    both, weak = M.validate_long(model, lset, ref, [points[0][0]], [points[0][1]], weak_labels="from_ref", error_rate=True, **kw)
    assert _same(both[0][0].results_overall_metrics()["error_rate"], _want_rates(labels, ref_cols, cols[0])[0])
    assert weak["counts"].shape == (1, 10, 4)
