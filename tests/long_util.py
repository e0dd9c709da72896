"""Helpers shared by the -m gpu tests of the long-recording path (test_gpu_long.py, test_gpu_long_score.py,
test_gpu_long_sweep.py): window tables, prescribed stitch inputs, and the two sentinel-buffer harnesses around the C calls.
Every buffer a kernel writes starts as sentinel / NaN bytes and carries a tail that must come back untouched."""
import numpy as np
import torch

from tests import long_score_np as ls

SENT = -7
TAIL = 8


def _l():
    from dcase2019_task4_amd import _lib
    return _lib.lib()


def _tile():
    return int(_l().sed_stitch_tile_frames())


def _group():
    return int(_l().sed_stitch_sweep_point_group())


def _n_windows(L3, T3, hop3):
    return 1 if L3 <= T3 else 1 + -(-(L3 - T3) // hop3)


def _tables(L3s, T3, hop3):
    return (np.r_[0, np.cumsum([_n_windows(L, T3, hop3) for L in L3s])].astype(np.int32),
            np.r_[0, np.cumsum(L3s)].astype(np.int64))


class _Scaler:
    def __init__(self, n_mels):
        rs = np.random.RandomState(11)
        self.mean_ = rs.uniform(-30, -10, n_mels)
        self.std_ = rs.uniform(5, 15, n_mels)


def _stitch_inputs():
    """Window posteriors whose timeline is a prescribed 0.9 / 0.1 pattern (hop3 = T3), three recordings, three classes."""
    T3, NC = 8, 3
    L3s = ls.stitch_lengths(_tile())
    patterns = ls.stitch_patterns(L3s, NC)
    tls = [np.where(a, np.float32(0.9), np.float32(0.1)) for a in patterns]
    n_w = [-(-L // T3) for L in L3s]
    p = np.concatenate([np.concatenate([t, np.full((-len(t) % T3, NC), 0.1, np.float32)]).reshape(-1, T3, NC) for t in tls])
    return (torch.from_numpy(p).cuda(), torch.from_numpy(np.r_[0, np.cumsum(n_w)].astype(np.int32)).cuda(),
            torch.from_numpy(np.r_[0, np.cumsum(L3s)].astype(np.int64)).cuda(), L3s, T3, NC, patterns)


def _ref_events(cols):
    from dcase2019_task4_amd.metrics import RefEvents
    ptr, on, off = ls.pack(cols)
    return RefEvents(ptr, on, off, [f"r{i}" for i in range(len(cols))], [f"c{i}" for i in range(len(cols[0]))])


class StitchCall:
    """One sed_stitch_decode (``sweep=False``: thr / win [NC]) or sed_stitch_sweep (``sweep=True``: thr / win [K, NC]) call on
    sentinel-filled outputs (NaN timeline, 0xEE binary, -7 integers, 0xFF workspace); ``misalign`` shifts the window
    posteriors and the timeline off 16-byte alignment.  ``get()`` checks what no call may touch: the tails of ev_ptr and
    the workspace, the second error word and, for the sweep, the binary buffer it is not given."""

    def __init__(self, p, rec_win0, rec_frame0, hop3, weighting, thr, win, capacity=None, misalign=False, sweep=False):
        from dcase2019_task4_amd import _lib
        self._lib, self.l, self.sweep = _lib, _lib.lib(), sweep
        p = np.ascontiguousarray(p, dtype=np.float32)
        self.n_win, self.T3, self.NC = p.shape
        self.n_rec, self.total = len(rec_win0) - 1, int(rec_frame0[-1])
        self.hop3, self.weighting = int(hop3), int(weighting)
        thr, win = np.asarray(thr, np.float32).reshape(-1, self.NC), np.asarray(win, np.int32).reshape(-1, self.NC)
        self.K = thr.shape[0]
        assert sweep or self.K == 1
        off = 1 if misalign else 0
        self._p = torch.empty(p.size + off, dtype=torch.float32, device="cuda")
        self.p = self._p[off:]
        self.p.copy_(torch.from_numpy(p.reshape(-1)))
        self.rec_win0 = torch.from_numpy(np.asarray(rec_win0, dtype=np.int32)).cuda()
        self.rec_frame0 = torch.from_numpy(np.asarray(rec_frame0, dtype=np.int64)).cuda()
        self.thr, self.win = torch.from_numpy(thr).cuda(), torch.from_numpy(win).cuda()
        L3 = np.diff(np.asarray(rec_frame0, dtype=np.int64))
        self.capacity = int(self.K * self.NC * ((np.maximum(L3, 0) + 1) // 2).sum()) if capacity is None else int(capacity)
        self._tl = torch.empty(self.total * self.NC + off, dtype=torch.float32, device="cuda")
        self.timeline = self._tl[off:]
        self.binary = torch.empty(self.total * self.NC, dtype=torch.uint8, device="cuda")
        self.ev_ptr = torch.empty(self.K * self.n_rec * self.NC + 1 + TAIL, dtype=torch.int64, device="cuda")
        self.ev_pairs = torch.empty(self.capacity + TAIL, 2, dtype=torch.int32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")
        self.ws_bytes = (self.l.sed_stitch_sweep_ws_bytes(self.total, self.n_rec, self.NC, self.K) if sweep
                         else self.l.sed_stitch_decode_ws_bytes(self.total, self.n_rec, self.NC))
        assert self.ws_bytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(self.ws_bytes + TAIL, dtype=torch.uint8, device="cuda")
        assert (self.p.data_ptr() % 16 != 0) == bool(misalign)

    def fill(self):
        self._tl.fill_(float("nan"))
        self.binary.fill_(0xEE)
        self.ev_ptr.fill_(SENT)
        self.ev_pairs.fill_(SENT)
        self.ws.fill_(0xFF)
        self.err.fill_(SENT)
        self.err[:1].zero_()

    def launch(self, **kw):
        ptr = self._lib.ptr
        a = dict(n_points=self.K, thr=self.thr, ws_bytes=self.ws_bytes, timeline=self.timeline)
        a.update(kw)
        head = (ptr(self.p), ptr(self.rec_win0), ptr(self.rec_frame0), self.n_rec, self.T3, self.NC, self.hop3, self.weighting)
        tail = (ptr(self.ev_ptr), ptr(self.ev_pairs), self.capacity, ptr(self.ws), a["ws_bytes"], ptr(self.err),
                self._lib.stream_ptr())
        if self.sweep:
            return self.l.sed_stitch_sweep(*head, a["n_points"], ptr(a["thr"]), ptr(self.win), ptr(a["timeline"]), *tail)
        return self.l.sed_stitch_decode(*head, ptr(a["thr"]), ptr(self.win), ptr(a["timeline"]), ptr(self.binary), *tail)

    def run(self):
        self.fill()
        assert self.launch() == 0, self.l.sed_last_error()
        return self.get()

    def get(self):
        torch.cuda.synchronize()
        n = self.K * self.n_rec * self.NC + 1
        ev_ptr = self.ev_ptr.cpu().numpy()
        assert (ev_ptr[n:] == SENT).all() and int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        assert not self.sweep or (self.binary == 0xEE).all()
        return {"timeline": self.timeline.cpu().numpy().reshape(self.total, self.NC),
                "binary": self.binary.cpu().numpy().reshape(self.total, self.NC), "ev_ptr": ev_ptr[:n],
                "ev_pairs": self.ev_pairs.cpu().numpy(), "err": int(self.err[0].item())}


class ScoreCall:
    """The two scorer C calls on sentinel-filled outputs with a tail of TAIL elements.  ``est`` a tuple: the one-point
    entries (sed_long_event_counts / sed_long_psds_counts) on given events (ptr, on, off) in seconds or on frames (ptr, pairs,
    num, den), per-column outputs [n_rec, NC, .].  ``est`` a list of K tuples (ptr, on, off): the sweep entries
    (sed_long_sweep_*) on their concatenation into one CSR in column order (k, rec, c), outputs [K, n_rec, NC, .].
    ``ref`` = (ptr, on, off).  Arrays are numpy; ptr int64."""

    def __init__(self, est, ref, n_rec, NC, est_cap=None, ref_cap=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        self.n_rec, self.NC = n_rec, NC
        self.sweep = isinstance(est, list)
        self.K = len(est) if self.sweep else 1
        self.lead = (self.K,) if self.sweep else ()
        dev = "cuda"
        if self.sweep:
            base = np.r_[0, np.cumsum([len(e[1]) for e in est])]
            ptr = np.concatenate([np.asarray(e[0], np.int64)[:-1] + base[k] for k, e in enumerate(est)] + [base[-1:]])
            est = (ptr, np.concatenate([np.asarray(e[1], np.float64) for e in est]),
                   np.concatenate([np.asarray(e[2], np.float64) for e in est]))
        self.est_ptr = torch.from_numpy(np.asarray(est[0], np.int64)).to(dev)
        if len(est) == 4:                                             # the device table as sed_stitch_decode left it
            self.pairs, self.num, self.den, self.on, self.off = est[1], float(est[2]), float(est[3]), None, None
            n_est = est[1].shape[0]                                   # its capacity, not the true count
        else:
            self.pairs, self.num, self.den = None, 0.0, 0.0
            self.on = torch.from_numpy(np.r_[np.asarray(est[1], np.float64), 0.0]).to(dev)
            self.off = torch.from_numpy(np.r_[np.asarray(est[2], np.float64), 0.0]).to(dev)
            n_est = len(est[1])
        self.est_cap = n_est if est_cap is None else est_cap
        self.ref_ptr = torch.from_numpy(np.asarray(ref[0], np.int64)).to(dev)
        self.ref_on = torch.from_numpy(np.r_[np.asarray(ref[1], np.float64), 0.0]).to(dev)
        self.ref_off = torch.from_numpy(np.r_[np.asarray(ref[2], np.float64), 0.0]).to(dev)
        self.ref_cap = len(ref[1]) if ref_cap is None else ref_cap
        K, ncols, W = self.K, n_rec * NC, 2 + NC
        mk = lambda n, dt: torch.empty(n + TAIL, dtype=dt, device=dev)
        self.ev_c, self.seg_c, self.ps_c = mk(K * ncols * 3, torch.int32), mk(K * ncols * 4, torch.int32), mk(K * ncols * W, torch.int32)
        self.ev_t, self.seg_t, self.ps_t = mk(K * NC * 3, torch.int64), mk(K * NC * 4, torch.int64), mk(K * NC * W, torch.int64)
        self.err = torch.empty(2, dtype=torch.int32, device=dev)
        ws_fn = self.l.sed_long_sweep_ws_bytes if self.sweep else self.l.sed_long_score_ws_bytes
        nbytes = ws_fn(self.est_cap, self.ref_cap, n_rec, NC, *self.lead)
        assert nbytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(nbytes + TAIL, dtype=torch.uint8, device=dev)

    def fill(self):
        K, NC, W = self.K, self.NC, 2 + self.NC
        for t in (self.ev_c, self.seg_c, self.ps_c):
            t.fill_(SENT)
        for t, n in ((self.ev_t, K * NC * 3), (self.seg_t, K * NC * 4), (self.ps_t, K * NC * W)):
            t.fill_(SENT)
            t[:n].zero_()
        self.err.fill_(SENT)
        self.err[:1].zero_()
        self.ws.fill_(0xFF)

    def _head(self):
        p = self._lib.ptr
        return (p(self.est_ptr), p(self.pairs), self.num, self.den, p(self.on), p(self.off), self.est_cap, p(self.ref_ptr),
                p(self.ref_on), p(self.ref_off), self.ref_cap, self.n_rec, self.NC, *self.lead)

    def launch_events(self, t_collar=0.2, pct=0.2, res=1.0, columns=True):
        p = self._lib.ptr
        fn = self.l.sed_long_sweep_event_counts if self.sweep else self.l.sed_long_event_counts
        return fn(*self._head(), float(t_collar), float(pct), float(res), p(self.ev_c) if columns else None,
                  p(self.seg_c) if columns else None, p(self.ev_t), p(self.seg_t), p(self.err), p(self.ws),
                  self.ws.numel() - TAIL, self._lib.stream_ptr())

    def launch_psds(self, dtc=0.5, gtc=0.5, cttc=0.3, columns=True):
        p = self._lib.ptr
        fn = self.l.sed_long_sweep_psds_counts if self.sweep else self.l.sed_long_psds_counts
        return fn(*self._head(), float(dtc), float(gtc), float(cttc), p(self.ps_c) if columns else None, p(self.ps_t),
                  p(self.err), p(self.ws), self.ws.numel() - TAIL, self._lib.stream_ptr())

    def get(self):
        """Everything as numpy, after checking that nothing beyond the owned elements was written."""
        torch.cuda.synchronize()
        K, n_rec, NC, W = self.K, self.n_rec, self.NC, 2 + self.NC
        ncols, out = n_rec * NC, {}
        for name, t, n, shape in (("ev", self.ev_c, K * ncols * 3, (n_rec, NC, 3)), ("seg", self.seg_c, K * ncols * 4, (n_rec, NC, 4)),
                                  ("ps", self.ps_c, K * ncols * W, (n_rec, NC, W)), ("ev_t", self.ev_t, K * NC * 3, (NC, 3)),
                                  ("seg_t", self.seg_t, K * NC * 4, (NC, 4)), ("ps_t", self.ps_t, K * NC * W, (NC, W))):
            h = t.cpu().numpy()
            assert (h[n:] == SENT).all(), name
            out[name] = h[:n].reshape(self.lead + shape)
        assert int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        out["err"] = int(self.err[0].item())
        return out

    def run(self, events=True, psds=True, **kw):
        self.fill()
        if events:
            assert self.launch_events(**{k: v for k, v in kw.items() if k in ("t_collar", "pct", "res")}) == 0, self.l.sed_last_error()
        if psds:
            assert self.launch_psds(**{k: v for k, v in kw.items() if k in ("dtc", "gtc", "cttc")}) == 0, self.l.sed_last_error()
        return self.get()
