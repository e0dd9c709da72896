"""Validation scoring on the GPU: event-based, segment-based and clip-level (weak) F-measures - the half of the reference's
epoch that follows ``get_predictions`` (baseline/main.py:328-352, evaluation_measures.py:19-102,124-182,234-246).

The reference turns the device posteriors into a pandas table, then into per-file lists of dicts, and lets ``sed_eval`` match
the events in Python, once per epoch.  Here ``sed_event_counts`` decodes the posteriors with the code of ``sed_postprocess``,
keeps the events on the device, matches them against reference annotations that live there too (``RefEvents``) and returns
integer counts; any number of operating points (threshold, median window) is one more grid dimension of the same launch.
``sed_weak_counts`` does the same for the clip-level tags.  There is no CPU fallback.

Provenance: ``sed_eval`` is third-party, absent from this image and from the reference tree, so the event / segment
definitions are restated from its published algorithm - **parity with ``sed_eval`` itself is unpinned**, exactly as
``oracle/postprocess_np.py`` states for ``dcase_util``.  What is pinned is exact agreement with an independent numpy / scipy
statement of those definitions (``tests/sed_eval_np.py``).

Definitions (per file and class; label equality is the column):

* event-based: reference event r and estimated event e are compatible iff ``|r.on - e.on| <= t_collar`` and
  ``|r.off - e.off| <= max(t_collar, percentage_of_length * (r.off - r.on))``; ``Ntp`` is the size of a maximum bipartite
  matching (sed_eval's ``event_matching_type='optimal'``), ``Nfp = Nsys - Ntp``, ``Nfn = Nref - Ntp``.
* segment-based: an event covers segments ``max(0, floor(on / res)) .. ceil(off / res) - 1``; a file has
  ``ceil(max offset over both lists and all classes / res)`` segments.
* ``P = Ntp / Nsys`` (0 when ``Nsys == 0``: ``empty_system_output_handling='zero_score'``), ``R = Ntp / Nref`` (NaN when
  ``Nref == 0``), ``F = 2PR / (P + R)`` (0 when both are 0); class-wise average = ``nanmean`` over classes; overall = micro
  over the summed counts; class-wise ``ER = (Nfn + Nfp) / Nref``.

Limits: at most 64 reference and 64 estimated events per (file, class) - a column beyond that raises, it is never
truncated -, ``T <= 2048`` output frames, at most 16 classes.

Overall error rate *with substitutions* (``error_counts``, ``long_error_counts``, ``long_sweep_error_counts`` and their
``*_from_events`` forms -> ``ErrorCounts``; ``error_rate=True`` of ``validate`` / ``validate_long`` /
``compute_strong_metrics``; ``EventMetrics`` / ``SegmentMetrics(overall=...)``).  It needs a second, label-agnostic pass
over each file, which the default paths do not launch: without it ``results_overall_metrics()['error_rate']`` holds NaN.

* segment-based (sed_eval's, exactly): per segment ``fn_s`` / ``fp_s`` = the classes active only in the reference / only in
  the estimate; ``S += min(fn_s, fp_s)``, ``D += max(0, fn_s - fp_s)``, ``I += max(0, fp_s - fn_s)``;
  ``ER = (S + D + I) / Nref``, ``Nref = sum_c (Ntp_c + Nfn_c)``.  ``S + D = sum_c Nfn_c`` and ``S + I = sum_c Nfp_c``.
* event-based: ``Nany`` = the size of a maximum bipartite matching over ALL events of the file under the compatibility test
  with the label ignored; ``Nsubs = Nany - Ntp``, ``Nfn = Nref - Nany``, ``Nfp = Nsys - Nany``,
  ``ER = (Nsubs + Nfn + Nfp) / Nref``; ``Ntp <= Nany <= min(Nref, Nsys)``.  A decision: sed_eval finds substitutions by a
  greedy pass over what its label-wise matching left over, a count that depends on the list order and on which maximum
  matching its matcher returned - not a function of the two event sets, so it cannot be pinned.  That pass is itself a
  time-compatible matching: sed_eval's ``Nsubs`` is never larger than this one and its ER never smaller; they agree
  whenever the greedy pass is maximum.  Pinned: exact agreement with ``tests/error_rate_np.py``.
* limit: at most 64 events per side in one CLUSTER of the file's events of all classes merged by onset (clips and long
  recordings alike); beyond that the call raises, nothing is truncated.

Long recordings (``long_event_counts``, ``long_psds_counts``, ``validate_long``, ``long_*_from_events``): the same definitions
on the event table ``inference.stitch_decode`` leaves on the device, or on two ``RefEvents``, WITHOUT the limit per column
(``sed_long_event_counts`` / ``sed_long_psds_counts``, csrc/lscore.hip).  Both sides of a column must be sorted by onset
(checked on the device).  The matching is exact per CLUSTER - the runs of the merged onset order between cuts across which no
pair can be compatible (include/dcase_sed.h) -, and a cluster holds at most 64 events per side: beyond that the call raises,
nothing is truncated.  K operating points: ``long_sweep_event_counts`` / ``long_sweep_psds_counts`` score the table of
``inference.stitch_sweep`` (or K ``RefEvents``) against ONE preparation of the reference side, four launches whatever K is
(``sed_long_sweep_*``); ``validate_long(one_blend=True)`` uses them.  Recording-level weak tags: ``validate_long(weak_labels=...)``
pools them once (``inference.stitch_weak``) and scores them with ``weak_counts``.  The overall error rate:
``validate_long(error_rate=True)`` (``sed_long_error_counts`` / ``sed_long_sweep_error_counts``, six launches whatever K is, the
reference side merged once).  Two-threshold decode: ``validate_long(thresholds_high=...)`` scores the table of
``inference.stitch_hysteresis`` with the same sweep scorers.  Minimum event length and gap merging:
``validate_long(min_event_lengths=..., min_event_gaps=...)`` puts every decoded table through ``inference.events_process``
in front of the same scorers.  Not provided there: an exact matching of clusters beyond 64 per
side.

PSDS (polyphonic sound detection score, Bilen et al., ICASSP 2020): ``sed_psds_counts`` scores the same (operating point,
clip) grid with the three intersection criteria and returns integer class totals (``psds_counts``, ``PSDSCounts``); the
PSD-ROC and its area are host arithmetic on those totals (``PSDS``), which also works without a GPU.  ``psds_eval`` is
third-party and absent from this image and from the reference tree, so the definitions are restated from the paper and,
where the package's behaviour was uncertain, decided here - **parity with ``psds_eval`` itself is unpinned**; pinned is
exact agreement of the counts with an independent numpy statement (``tests/psds_np.py``).

* ``I(d, g) = max(0, min(d.off, g.off) - max(d.on, g.on))``, ``len(e) = e.off - e.on``; every sum is a sequential fp64 sum
  over the other side's events in stored order (references: sorted by onset, then offset), every test is
  ``sum / len >= threshold``; an event with ``len <= 0`` or a NaN ratio fails every test.
* DTC: detection ``d`` of class ``c`` is relevant iff ``sum_{g in G_c} I(d, g) / len(d) >= dtc``; ``FP[c]`` counts the
  detections that are not relevant (cross-triggers included).
* GTC: ground truth ``g`` is a true positive iff ``sum_{relevant d in D_c} I(d, g) / len(g) >= gtc``.
* CTTC: a non-relevant detection ``d`` of class ``c`` adds 1 to ``CT[c][k]``, ``k != c``, iff
  ``sum_{g in G_k} I(d, g) / len(d) >= cttc``.
* With ``u = 3600`` (rates per hour): ``TPR = TP / n_gt``, ``FPR = u FP / T_data``, ``CTR[c][k] = u CT[c][k] / T_gt[k]`` (0
  where ``T_gt[k] == 0``), ``eFPR[c] = FPR[c] + alpha_ct * mean_{k != c} CTR[c][k]``; per class the curve is the running
  maximum of TPR over the points sorted by eFPR (0 below the first); on the union of all eFPR values ``<= e_max`` the
  effective TPR is ``max(0, mean_c - alpha_st * std_c)`` (population std) and PSDS is the area of that left-continuous
  staircase up to ``e_max``, over ``e_max``.
"""
import logging

import numpy as np
import torch

from . import _lib
from .inference import _Cfg, eval_batches

LOG = logging.getLogger(__name__)
MAX_EVENTS = 64
MAX_CLASSES = 16
_ERR_BITS = {1: "a (file, class) column has more than 64 reference events",
             2: "a (file, class) column has more than 64 estimated events",
             4: "a file has more than 65 536 segments",
             8: "a median window outside 1 .. 63",
             16: "malformed event offsets"}
# the long calls (sed_long_event_counts / sed_long_psds_counts): no limit per column, the limit is per cluster
_LONG_ERR_BITS = {1: "a cluster of more than 64 reference events whose onsets chain within t_collar",
                  2: "a cluster of more than 64 estimated events whose onsets chain within t_collar",
                  4: "a recording has more than 65 536 segments",
                  16: "malformed event offsets",
                  64: "a column whose onsets decrease (both sides must be sorted by onset)",
                  128: "the decoded event table is invalid (sed_stitch_decode reported an error)"}

# the overall-error-rate calls: the matching runs on the file's events of ALL classes merged by onset
_ERROR_ERR_BITS = {**_ERR_BITS,
                   1: "more than 64 reference events in a (file, class) column or in one cluster of the file's merged events",
                   2: "more than 64 estimated events in a (file, class) column or in one cluster of the file's merged events"}
_LONG_ERROR_ERR_BITS = {**_LONG_ERR_BITS,
                        1: "a cluster of more than 64 reference events, all classes merged, whose onsets chain within t_collar",
                        2: "a cluster of more than 64 estimated events, all classes merged, whose onsets chain within t_collar"}


def _pack(df, filenames, labels):
    """(filename, onset, offset, event_label) rows -> CSR arrays: column (clip, class) = clip * len(labels) + class, events
    sorted by onset inside a column.  Rows with a NaN label carry no event (get_event_list_current_file,
    evaluation_measures.py:105-121); rows of files outside ``filenames`` are ignored, as the reference's per-file loop does."""
    filenames, labels = list(filenames), list(labels)
    if len(set(filenames)) != len(filenames):
        raise ValueError("duplicate file names")
    file_ix = {f: i for i, f in enumerate(filenames)}
    label_ix = {l: i for i, l in enumerate(labels)}
    nc = len(labels)
    ncol = len(filenames) * nc
    d = df[df["event_label"].notna() & df["filename"].isin(file_ix)] if len(df) else df
    if len(d) == 0:
        return np.zeros(ncol + 1, np.int32), np.zeros(0, np.float64), np.zeros(0, np.float64)
    unknown = sorted(set(d["event_label"]) - set(label_ix))
    if unknown:
        raise ValueError(f"event labels outside the label list: {unknown}")
    col = d["filename"].map(file_ix).to_numpy(np.int64) * nc + d["event_label"].map(label_ix).to_numpy(np.int64)
    on = d["onset"].to_numpy(np.float64)
    off = d["offset"].to_numpy(np.float64)
    order = np.lexsort((off, on, col))
    ptr = np.zeros(ncol + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=ncol), out=ptr[1:])
    return ptr.astype(np.int32), np.ascontiguousarray(on[order]), np.ascontiguousarray(off[order])


class RefEvents:
    """Reference annotations of a validation set on the device, in the CSR form ``sed_event_counts`` reads:
    ``ptr [N * nclass + 1]`` int32, ``onset / offset [n_events]`` fp64 seconds.  On a CPU device it holds the arrays (what can
    be checked without a GPU) and refuses to score."""

    def __init__(self, ptr, onset, offset, filenames, labels, device="cuda"):
        self.filenames, self.labels = list(filenames), list(labels)
        if not 1 <= len(self.labels) <= MAX_CLASSES:
            raise _lib.SedError(f"need 1 .. {MAX_CLASSES} classes, got {len(self.labels)}")
        ptr = np.asarray(ptr, np.int32)
        if ptr.shape != (len(self.filenames) * len(self.labels) + 1,) or ptr[0] != 0 or np.any(np.diff(ptr) < 0) \
                or ptr[-1] != len(onset) or len(onset) != len(offset):
            raise ValueError("malformed CSR arrays")
        self.device = torch.device(device)
        self.max_per_column = int(np.diff(ptr).max()) if len(ptr) > 1 else 0
        # host copies of the CSR arrays (PSDS.from_counts reads the per-class reference counts and durations from them)
        self.ptr_host = ptr.copy()
        self.onset_host, self.offset_host = np.array(onset, np.float64), np.array(offset, np.float64)
        self.ptr = torch.as_tensor(ptr).to(self.device)
        self.ptr64 = torch.as_tensor(ptr.astype(np.int64)).to(self.device)     # what the long calls read
        # one trailing element: an empty event list still has an address the library accepts
        self.onset = torch.as_tensor(np.r_[np.asarray(onset, np.float64), 0.0]).to(self.device)
        self.offset = torch.as_tensor(np.r_[np.asarray(offset, np.float64), 0.0]).to(self.device)

    @classmethod
    def from_dataframe(cls, valid_df, filenames, labels, device="cuda"):
        """``valid_df``: the reference's annotation frame (``filename, onset, offset, event_label``); clips in ``filenames``
        order (``valid_synth_data.filenames``), classes in ``labels`` order (``many_hot_encoder.labels``).  A file with a
        single NaN-label row, or absent from the frame, has no events."""
        ptr, on, off = _pack(valid_df, filenames, labels)
        return cls(ptr, on, off, filenames, labels, device)

    def __len__(self):
        return len(self.filenames)

    def weak_labels(self):
        """``[n_files, nclass]`` uint8: 1 where the file has at least one reference event of the class (the weak tags the
        strong annotations imply)."""
        return (np.diff(self.ptr_host).reshape(len(self.filenames), len(self.labels)) > 0).astype(np.uint8)

    @property
    def nclass(self):
        return len(self.labels)


class _DeviceCounts:
    """What ``Counts`` and ``PSDSCounts`` share: ``buf`` - int64 class totals of ``width`` values per (operating point,
    class) and, last, the error word ``err`` - in ONE device buffer, so that ``host()`` is one copy."""

    def __init__(self, n_points, nclass, width, device, err_what):
        self.K, self.NC = n_points, nclass
        self.buf = torch.zeros(n_points * nclass * width + 1, dtype=torch.int64, device=device)
        self.err = self.buf[-1:].view(torch.int32)
        self.err_what, self.err_bits = err_what, _ERR_BITS                    # (the long calls put their own wording here)

    def _totals_to_host(self, extra=None):
        """The buffer without its error word - one device -> host copy; raises when the word is set.  ``extra``: an int64
        device vector that travels in the same copy; the result is then ``(totals, extra on the host)``."""
        n = self.buf.numel()
        h = (self.buf if extra is None else torch.cat([self.buf, extra])).cpu().numpy()
        err = int(h[n - 1:n].view(np.int32)[0])
        if err:
            raise _lib.SedError(self.err_what + ": " + "; ".join(m for b, m in self.err_bits.items() if err & b)
                                + " - nothing was truncated, the counts are invalid")
        return h[:n - 1] if extra is None else (h[:n - 1], h[n:])

    def check(self):
        return self.host()


class Counts(_DeviceCounts):
    """Class totals of one or more ``event_counts`` calls, on the device: ``ev [K, nclass, 3]`` (Ntp, Nref, Nsys) and
    ``seg [K, nclass, 4]`` (Ntp, Nfp, Nfn, Ntn) int64, and the error word, all in ONE buffer so that ``host()`` is one copy.
    ``ev_columns [K, N, nclass, 3]`` / ``seg_columns [K, N, nclass, 4]`` int32 hold the last call's per-column counts when it
    was asked for them."""

    def __init__(self, n_points, nclass, device):
        _DeviceCounts.__init__(self, n_points, nclass, 7, device, "sed_event_counts")
        n3 = n_points * nclass * 3
        self.ev = self.buf[:n3].view(n_points, nclass, 3)
        self.seg = self.buf[n3:-1].view(n_points, nclass, 4)
        self.ev_columns = self.seg_columns = None

    def host(self, extra=None):
        """(ev, seg) as numpy arrays - one device -> host copy; raises when a column was over a limit.  ``extra``: an int64
        device vector taken along in that copy and returned third."""
        h, n3 = self._totals_to_host(extra), self.K * self.NC * 3
        h, tail = h if extra is not None else (h, None)
        ev, seg = h[:n3].reshape(self.K, self.NC, 3), h[n3:].reshape(self.K, self.NC, 4)
        return (ev, seg) if extra is None else (ev, seg, tail)


class PSDSCounts(_DeviceCounts):
    """Class totals of one or more ``psds_counts`` calls, on the device: ``totals [K, nclass, 2 + nclass]`` int64 - per class
    (TP, FP, CT[.][0 .. nclass - 1]) - and the error word, in ONE buffer so that ``host()`` is one copy.  ``columns
    [K, N, nclass, 2 + nclass]`` int32 holds the last call's per-column counts when it was asked for them.  The criteria
    ``dtc / gtc / cttc`` belong to the totals: every call that accumulates into them uses these."""

    def __init__(self, n_points, nclass, device, dtc=0.5, gtc=0.5, cttc=0.3):
        for name, v in (("dtc", dtc), ("gtc", gtc), ("cttc", cttc)):
            if not 0.0 <= v <= 1.0:                     # (NaN fails too)
                raise ValueError(f"{name} must be in [0, 1], got {v}")
        _DeviceCounts.__init__(self, n_points, nclass, 2 + nclass, device, "sed_psds_counts")
        self.dtc, self.gtc, self.cttc = float(dtc), float(gtc), float(cttc)
        self.totals = self.buf[:-1].view(n_points, nclass, 2 + nclass)
        self.columns = None

    def host(self):
        """``totals`` as a numpy array - one device -> host copy; raises when a column was over a limit."""
        return self._totals_to_host().reshape(self.K, self.NC, 2 + self.NC)


class ErrorCounts(_DeviceCounts):
    """Totals of one or more ``error_counts`` calls, on the device: ``ev [K, 3]`` (Nref, Nsys, Nany) and ``seg [K, 3]``
    (S, D, I) int64 per operating point - the counts of the OVERALL error rate (module docstring) -, and the error word, in
    ONE buffer so that ``host()`` is one copy.  ``ev_files [K, N, 3]`` / ``seg_files [K, N, 3]`` int32 hold the last call's
    per-file counts when it was asked for them."""

    def __init__(self, n_points, nclass, device):
        _DeviceCounts.__init__(self, n_points, 1, 6, device, "sed_error_counts")
        self.NC = nclass
        self.err_bits = _ERROR_ERR_BITS
        self.ev = self.buf[:n_points * 3].view(n_points, 3)
        self.seg = self.buf[n_points * 3:-1].view(n_points, 3)
        self.ev_files = self.seg_files = None

    def parse(self, h):
        """(ev, seg) from a host copy of ``buf`` (int64 numpy, the error word last); raises when the word is set."""
        h = np.asarray(h, np.int64)
        err = int(h[-1:].view(np.int32)[0])
        if err:
            raise _lib.SedError(self.err_what + ": " + "; ".join(m for b, m in self.err_bits.items() if err & b)
                                + " - nothing was truncated, the counts are invalid")
        return h[:self.K * 3].reshape(self.K, 3), h[self.K * 3:-1].reshape(self.K, 3)

    def host(self):
        """(ev, seg) as numpy arrays - one device -> host copy; raises when a file was over a limit."""
        return self.parse(self.buf.cpu().numpy())


def operating_points(thresholds=(0.5,), median_windows=(5,), device="cuda"):
    """K operating points as device arrays ``(thr [K] float32, win [K] int32)``: sequences of equal length, or one of them of
    length 1.  Build them once outside a loop or a graph capture."""
    if torch.is_tensor(thresholds) and torch.is_tensor(median_windows):
        return thresholds, median_windows
    thr = np.atleast_1d(np.asarray(thresholds, np.float32))
    win = np.atleast_1d(np.asarray(median_windows, np.int32))
    K = max(len(thr), len(win))
    if len(thr) not in (1, K) or len(win) not in (1, K) or K < 1:
        raise ValueError("thresholds and median_windows must have equal lengths (or length 1)")
    if win.min() < 1 or win.max() > 63:
        raise _lib.SedError("median windows must be in [1, 63]")
    thr, win = np.broadcast_to(thr, K).copy(), np.broadcast_to(win, K).copy()
    return torch.as_tensor(thr).to(device), torch.as_tensor(win).to(device)


# ---- clips: posteriors of a batch (or given events) against the RefEvents of the same clips -----------------------------------
# One helper family serves ``sed_event_counts`` and ``sed_psds_counts``, whose leading arguments - the estimated side, then the
# reference side - are the same.  ``est`` = (those arguments: strong, n, T, NC, K, thr, win, num, den, est_ptr, est_on, est_off,
# ref_ptr, ref_on, ref_off; n; K; NC; the device; the tensors behind the pointers that only this tuple keeps alive until the
# launch).
def _posterior_args(strong, ref, thresholds, median_windows, pooling_time_ratio, cfg, clip_offset, what):
    if strong.device.type != "cuda" or ref.device.type != "cuda":
        raise _lib.SedError(f"{what} needs GPU tensors and a RefEvents on the GPU (no CPU fallback)")
    cfg = cfg or _Cfg
    strong = strong.contiguous().float()
    n, T, NC = strong.shape
    if NC != ref.nclass or clip_offset < 0 or clip_offset + n > len(ref):
        raise ValueError(f"posteriors [{n}, {T}, {NC}] at clip {clip_offset} do not fit the reference ({len(ref)} clips, "
                         f"{ref.nclass} classes)")
    thr, win = operating_points(thresholds, median_windows, strong.device)
    K, p = thr.numel(), _lib.ptr
    # (the offsets of clip clip_offset by address: a view of ref.ptr per batch costs more host time than the rest of this call)
    ref_ptr = _lib.C.c_void_p(ref.ptr.data_ptr() + clip_offset * NC * ref.ptr.element_size())
    args = (p(strong), n, T, NC, K, p(thr), p(win), float(pooling_time_ratio), float(cfg.sample_rate / cfg.hop_length),
            None, None, None, ref_ptr, p(ref.onset), p(ref.offset))
    return args, n, K, NC, strong.device, (strong, thr, win)


def _given_args(est, ref, what):
    if est.device.type != "cuda" or ref.device.type != "cuda":
        raise _lib.SedError(f"{what} needs both event sets on the GPU (no CPU fallback)")
    if est.filenames != ref.filenames or est.labels != ref.labels:
        raise ValueError("estimated and reference events must cover the same files and classes, in the same order")
    n, NC, p = len(ref), ref.nclass, _lib.ptr
    return (None, n, 0, NC, 1, None, None, 0.0, 0.0, p(est.ptr), p(est.onset), p(est.offset), p(ref.ptr), p(ref.onset),
            p(ref.offset)), n, 1, NC, ref.device, ()


def _event_target(est, t_collar, percentage_of_length, time_resolution, counts, per_column):
    args, n, K, NC, device, _ = est
    if counts is None:
        counts = Counts(K, NC, device)
    if (counts.K, counts.NC) != (K, NC):
        raise ValueError("counts was built for another number of operating points / classes")
    if per_column:
        counts.ev_columns = torch.empty(K, n, NC, 3, dtype=torch.int32, device=device)
        counts.seg_columns = torch.empty(K, n, NC, 4, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().sed_event_counts(
        *args, float(t_collar), float(percentage_of_length), float(time_resolution),
        _lib.ptr(counts.ev_columns) if per_column else None, _lib.ptr(counts.seg_columns) if per_column else None,
        _lib.ptr(counts.ev), _lib.ptr(counts.seg), _lib.ptr(counts.err), _lib.stream_ptr()), "sed_event_counts")
    return counts


def _psds_target(est, dtc, gtc, cttc, counts, per_column):
    args, n, K, NC, device, _ = est
    if counts is None:
        counts = PSDSCounts(K, NC, device, dtc, gtc, cttc)
    if (counts.K, counts.NC) != (K, NC):
        raise ValueError("counts was built for another number of operating points / classes")
    if (counts.dtc, counts.gtc, counts.cttc) != (float(dtc), float(gtc), float(cttc)):
        raise ValueError("counts was built for other criteria (dtc, gtc, cttc)")
    if per_column:
        counts.columns = torch.empty(K, n, NC, 2 + NC, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().sed_psds_counts(
        *args, counts.dtc, counts.gtc, counts.cttc, _lib.ptr(counts.columns) if per_column else None, _lib.ptr(counts.totals),
        _lib.ptr(counts.err), _lib.stream_ptr()), "sed_psds_counts")
    return counts


def event_counts(strong, ref, thresholds=(0.5,), median_windows=(5,), pooling_time_ratio=1, cfg=None, t_collar=0.200,
                 percentage_of_length=0.2, time_resolution=1.0, clip_offset=0, counts=None, per_column=False):
    """``strong [n, T, nclass]`` cuda float32 posteriors of clips ``clip_offset .. clip_offset + n - 1`` of ``ref`` -> ``Counts``
    (device tensors, no synchronisation; pass ``counts`` to accumulate batches).  ``thresholds`` / ``median_windows``: see
    ``operating_points`` (device tensors are taken as they are).  ``cfg`` supplies sample_rate / hop_length (default
    baseline/config.py): seconds = frame * pooling_time_ratio / (sample_rate / hop_length), evaluation_measures.py:226-227."""
    est = _posterior_args(strong, ref, thresholds, median_windows, pooling_time_ratio, cfg, clip_offset, "event_counts")
    return _event_target(est, t_collar, percentage_of_length, time_resolution, counts, per_column)


def event_counts_from_events(est, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, per_column=False):
    """The matching stage alone: ``est`` is a ``RefEvents`` holding the ESTIMATED events of the same files and classes (they
    need not be disjoint).  One operating point."""
    return _event_target(_given_args(est, ref, "event_counts_from_events"), t_collar, percentage_of_length, time_resolution,
                         None, per_column)


def psds_counts(strong, ref, thresholds=(0.5,), median_windows=(5,), pooling_time_ratio=1, cfg=None, dtc=0.5, gtc=0.5,
                cttc=0.3, clip_offset=0, counts=None, per_column=False):
    """``event_counts`` for the PSDS criteria: ``strong [n, T, nclass]`` cuda float32 posteriors of clips ``clip_offset ..
    clip_offset + n - 1`` of ``ref`` -> ``PSDSCounts`` (device tensors, no synchronisation; pass ``counts`` to accumulate
    batches - its criteria must be these).  Operating points, ``cfg`` and the seconds as in ``event_counts``."""
    est = _posterior_args(strong, ref, thresholds, median_windows, pooling_time_ratio, cfg, clip_offset, "psds_counts")
    return _psds_target(est, dtc, gtc, cttc, counts, per_column)


def psds_counts_from_events(est, ref, dtc=0.5, gtc=0.5, cttc=0.3, per_column=False):
    """The criteria alone: ``est`` is a ``RefEvents`` holding the DETECTIONS of the same files and classes.  One operating
    point."""
    return _psds_target(_given_args(est, ref, "psds_counts_from_events"), dtc, gtc, cttc, None, per_column)


def _error_target(est, t_collar, percentage_of_length, time_resolution, counts, per_file):
    args, n, K, NC, device, _ = est
    if counts is None:
        counts = ErrorCounts(K, NC, device)
    if (counts.K, counts.NC) != (K, NC):
        raise ValueError("counts was built for another number of operating points / classes")
    if per_file:
        counts.ev_files = torch.empty(K, n, 3, dtype=torch.int32, device=device)
        counts.seg_files = torch.empty(K, n, 3, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().sed_error_counts(
        *args, float(t_collar), float(percentage_of_length), float(time_resolution),
        _lib.ptr(counts.ev_files) if per_file else None, _lib.ptr(counts.seg_files) if per_file else None,
        _lib.ptr(counts.ev), _lib.ptr(counts.seg), _lib.ptr(counts.err), _lib.stream_ptr()), "sed_error_counts")
    return counts


def error_counts(strong, ref, thresholds=(0.5,), median_windows=(5,), pooling_time_ratio=1, cfg=None, t_collar=0.200,
                 percentage_of_length=0.2, time_resolution=1.0, clip_offset=0, counts=None, per_file=False):
    """``event_counts`` for the OVERALL error rate: the same posteriors, operating points and seconds -> ``ErrorCounts``
    (device tensors, no synchronisation; pass ``counts`` to accumulate batches).  ``per_file``: ``counts.ev_files /
    seg_files [K, n, 3]`` of this call."""
    est = _posterior_args(strong, ref, thresholds, median_windows, pooling_time_ratio, cfg, clip_offset, "error_counts")
    return _error_target(est, t_collar, percentage_of_length, time_resolution, counts, per_file)


def error_counts_from_events(est, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, per_file=False):
    """The scoring stage alone: ``est`` is a ``RefEvents`` holding the ESTIMATED events of the same files and classes.  One
    operating point."""
    return _error_target(_given_args(est, ref, "error_counts_from_events"), t_collar, percentage_of_length, time_resolution,
                         None, per_file)


def weak_counts(weak, labels, thresholds, counts=None):
    """``weak [n, nclass]`` cuda float32, ``labels [n, nclass]`` 0/1, ``thresholds [K, nclass]`` (or ``[nclass]``) ->
    ``[K, nclass, 4]`` int64 (tp, fp, fn, tn) with ``pred = weak > thr`` (intermediate_at_measures,
    evaluation_measures.py:86-102), on the device, no synchronisation.  Pass ``counts`` to accumulate batches."""
    if weak.device.type != "cuda":
        raise _lib.SedError("weak_counts needs GPU tensors (no CPU fallback)")
    weak = weak.contiguous().float()
    n, NC = weak.shape
    labels = labels.to(weak.device).ne(0).to(torch.uint8).contiguous()
    thr = torch.as_tensor(thresholds, dtype=torch.float32).to(weak.device).reshape(-1, NC).contiguous()
    if labels.shape != weak.shape:
        raise ValueError(f"labels {tuple(labels.shape)} do not match the posteriors {tuple(weak.shape)}")
    K = thr.shape[0]
    if counts is None:
        counts = torch.zeros(K, NC, 4, dtype=torch.int64, device=weak.device)
    if tuple(counts.shape) != (K, NC, 4) or counts.dtype != torch.int64 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int64 [K, nclass, 4] tensor")
    _lib.check(_lib.lib().sed_weak_counts(_lib.ptr(weak), _lib.ptr(labels), n, NC, _lib.ptr(thr), K, _lib.ptr(counts),
                                          _lib.stream_ptr()), "sed_weak_counts")
    return counts


# ---- the numbers main.py and its logs read, with sed_eval's key names ------------------------------------------------------
def _ratio(num, den, empty):
    return float(num) / float(den) if den > 0 else empty


def _f_measure(p, r):
    if p == 0 and r == 0:
        return 0.0
    return 2 * p * r / (p + r)


def f_measure_from_counts(counts):
    """Clip-level F1 per (point, class) from ``weak_counts`` totals ``[..., 4]`` (tp, fp, fn, tn): ``2 tp / (2 tp + fp + fn)``, 0
    where that denominator is 0 (evaluation_measures.py:73-83)."""
    tp, fp, fn = (np.asarray(counts)[..., i].astype(np.float64) for i in range(3))
    den = 2 * tp + fp + fn
    return np.divide(2 * tp, den, out=np.zeros_like(den), where=den != 0)


def _nanmean(values):
    v = np.asarray(values, np.float64)
    return float(np.nansum(v) / np.count_nonzero(~np.isnan(v))) if np.any(~np.isnan(v)) else float("nan")


class _Metrics:
    """Ratios from per-class (Ntp, Nref, Nsys, Nfp, Nfn[, Ntn]) with sed_eval's result layout."""
    name = ""

    def __init__(self, labels, ntp, nref, nsys, nfp, nfn):
        self.event_label_list = list(labels)
        self.class_wise = {l: {"Ntp": int(a), "Nref": int(b), "Nsys": int(c), "Nfp": int(d), "Nfn": int(e)}
                           for l, a, b, c, d, e in zip(self.event_label_list, ntp, nref, nsys, nfp, nfn)}
        if len(self.class_wise) != len(self.event_label_list) or len(ntp) != len(self.event_label_list):
            raise ValueError("one row of counts per (distinct) label")

    @staticmethod
    def _scores(c):
        p = _ratio(c["Ntp"], c["Nsys"], 0.0)                    # empty_system_output_handling = 'zero_score'
        r = _ratio(c["Ntp"], c["Nref"], float("nan"))
        return {"f_measure": {"f_measure": _f_measure(p, r), "precision": p, "recall": r},
                "error_rate": {"error_rate": _ratio(c["Nfn"] + c["Nfp"], c["Nref"], float("nan")),
                               "deletion_rate": _ratio(c["Nfn"], c["Nref"], float("nan")),
                               "insertion_rate": _ratio(c["Nfp"], c["Nref"], float("nan"))}}

    def results_class_wise_metrics(self):
        out = {}
        for l, c in self.class_wise.items():
            out[l] = dict(self._scores(c), count={"Nref": c["Nref"], "Nsys": c["Nsys"]})
        return out

    def results_class_wise_average_metrics(self):
        cw = list(self.results_class_wise_metrics().values())
        return {g: {k: _nanmean([c[g][k] for c in cw]) for k in keys}
                for g, keys in (("f_measure", ("f_measure", "precision", "recall")),
                                ("error_rate", ("error_rate", "deletion_rate", "insertion_rate")))}

    overall_sdi = None               # (Nsubs, Nfn, Nfp) of the overall error rate, when the object was given ``overall=``

    def _totals(self):
        return {k: sum(c[k] for c in self.class_wise.values()) for k in ("Ntp", "Nref", "Nsys", "Nfp", "Nfn")}

    def results_overall_metrics(self):
        """Micro-averaged F-measure over the summed counts.  The overall error rate of sed_eval counts substitutions, which
        needs a second, label-agnostic matching (``error_counts`` and its long forms): built with ``overall=`` its totals,
        the four error-rate keys hold ``(S + D + I) / Nref`` and its three parts, NaN when ``Nref == 0``; without, NaN."""
        tot = self._totals()
        nan = float("nan")
        er = {"error_rate": nan, "substitution_rate": nan, "deletion_rate": nan, "insertion_rate": nan}
        if self.overall_sdi is not None:
            s, d, i = self.overall_sdi
            er = {"error_rate": _ratio(s + d + i, tot["Nref"], nan), "substitution_rate": _ratio(s, tot["Nref"], nan),
                  "deletion_rate": _ratio(d, tot["Nref"], nan), "insertion_rate": _ratio(i, tot["Nref"], nan)}
        return {"f_measure": self._scores(tot)["f_measure"], "error_rate": er}

    def results(self):
        return {"overall": self.results_overall_metrics(), "class_wise": self.results_class_wise_metrics(),
                "class_wise_average": self.results_class_wise_average_metrics()}

    def __str__(self):
        ov, av = self.results_overall_metrics()["f_measure"], self.results_class_wise_average_metrics()
        lines = [f"{self.name} metrics ({self._params()})",
                 "  Overall (micro-average): F {:6.2f} %  P {:6.2f} %  R {:6.2f} %".format(
                     100 * ov["f_measure"], 100 * ov["precision"], 100 * ov["recall"])]
        if self.overall_sdi is not None:
            er = self.results_overall_metrics()["error_rate"]
            lines.append("  Overall error rate: ER {:5.2f}  S {:5.2f}  D {:5.2f}  I {:5.2f}".format(
                er["error_rate"], er["substitution_rate"], er["deletion_rate"], er["insertion_rate"]))
        lines += ["  Class-wise average (macro-average): F {:6.2f} %  P {:6.2f} %  R {:6.2f} %  ER {:5.2f}".format(
                     100 * av["f_measure"]["f_measure"], 100 * av["f_measure"]["precision"], 100 * av["f_measure"]["recall"],
                     av["error_rate"]["error_rate"]),
                 "  {:30s} {:>6s} {:>6s} {:>8s} {:>8s} {:>8s} {:>6s}".format("Event label", "Nref", "Nsys", "F", "Pre", "Rec", "ER")]
        for l, c in self.results_class_wise_metrics().items():
            f, e = c["f_measure"], c["error_rate"]
            lines.append("  {:30s} {:6d} {:6d} {:7.1f}% {:7.1f}% {:7.1f}% {:6.2f}".format(
                str(l)[:30], c["count"]["Nref"], c["count"]["Nsys"], 100 * f["f_measure"], 100 * f["precision"],
                100 * f["recall"], e["error_rate"]))
        return "\n".join(lines)


class EventMetrics(_Metrics):
    """Event-based metrics from class totals ``[nclass, 3]`` (Ntp, Nref, Nsys) - what ``sed_eval``'s ``EventBasedMetrics``
    reports to main.py and its logs (``Nfp = Nsys - Ntp``, ``Nfn = Nref - Ntp``)."""
    name = "Event based"

    def __init__(self, labels, counts, t_collar=0.200, percentage_of_length=0.2, overall=None):
        c = np.asarray(counts, np.int64).reshape(-1, 3)
        self.t_collar, self.percentage_of_length = t_collar, percentage_of_length
        super().__init__(labels, c[:, 0], c[:, 1], c[:, 2], c[:, 2] - c[:, 0], c[:, 1] - c[:, 0])
        if overall is not None:
            # (Nref, Nsys, Nany) of the same files, ``ErrorCounts.host()[0][k]``: Nany = size of a maximum matching with the
            # labels ignored, so Nsubs = Nany - Ntp, Nfn = Nref - Nany, Nfp = Nsys - Nany
            nref, nsys, nany = (int(v) for v in np.asarray(overall, np.int64).reshape(3))
            tot = self._totals()
            if (nref, nsys) != (tot["Nref"], tot["Nsys"]) or not tot["Ntp"] <= nany <= min(nref, nsys):
                raise ValueError(f"overall (Nref, Nsys, Nany) = {(nref, nsys, nany)} does not belong to these class counts "
                                 f"(Nref {tot['Nref']}, Nsys {tot['Nsys']}, Ntp {tot['Ntp']})")
            self.overall_sdi = (nany - tot["Ntp"], nref - nany, nsys - nany)

    def _params(self):
        return f"onset-offset, t_collar {self.t_collar:.2f} s, offset (length) {100 * self.percentage_of_length:.0f} %"


class SegmentMetrics(_Metrics):
    """Segment-based metrics from class totals ``[nclass, 4]`` (Ntp, Nfp, Nfn, Ntn) - ``sed_eval``'s ``SegmentBasedMetrics``
    (``Nref = Ntp + Nfn``, ``Nsys = Ntp + Nfp``)."""
    name = "Segment based"

    def __init__(self, labels, counts, time_resolution=1.0, overall=None):
        c = np.asarray(counts, np.int64).reshape(-1, 4)
        self.time_resolution = time_resolution
        self.Ntn = {l: int(v) for l, v in zip(labels, c[:, 3])}
        super().__init__(labels, c[:, 0], c[:, 0] + c[:, 2], c[:, 0] + c[:, 1], c[:, 1], c[:, 2])
        if overall is not None:
            # (S, D, I) of the same files, ``ErrorCounts.host()[1][k]``: S + D = sum Nfn, S + I = sum Nfp
            s_, d_, i_ = (int(v) for v in np.asarray(overall, np.int64).reshape(3))
            tot = self._totals()
            if min(s_, d_, i_) < 0 or s_ + d_ != tot["Nfn"] or s_ + i_ != tot["Nfp"]:
                raise ValueError(f"overall (S, D, I) = {(s_, d_, i_)} does not belong to these class counts "
                                 f"(Nfn {tot['Nfn']}, Nfp {tot['Nfp']})")
            self.overall_sdi = (s_, d_, i_)

    def _params(self):
        return f"time resolution {self.time_resolution:.2f} s"


class PSDS:
    """The PSD-ROC and its area from class totals of K operating points - host arithmetic, no GPU needed.

    ``totals [K, nclass, 2 + nclass]`` (TP, FP, CT[.][k]) as ``PSDSCounts.host()`` returns them, ``n_gt [nclass]`` reference
    events per class, ``gt_duration [nclass]`` their summed lengths in seconds, ``dataset_duration`` the summed file
    durations in seconds.  Rates are per hour.  Arrays for logging: ``tpr [K, nclass]``, ``fpr [K, nclass]``,
    ``ctr [K, nclass, nclass]`` and ``efpr(alpha_ct) [K, nclass]``.  Parity with ``psds_eval`` is unpinned (module docstring)."""
    UNIT = 3600.0

    def __init__(self, labels, totals, n_gt, gt_duration, dataset_duration):
        self.labels = list(labels)
        nc = len(self.labels)
        t = np.asarray(totals, np.int64)
        if t.ndim != 3 or t.shape[1:] != (nc, 2 + nc):
            raise ValueError(f"totals must be [K, {nc}, {2 + nc}], got {t.shape}")
        self.n_gt = np.asarray(n_gt, np.int64).reshape(nc)
        self.gt_duration = np.asarray(gt_duration, np.float64).reshape(nc)
        self.dataset_duration = float(dataset_duration)
        empty = [l for l, n in zip(self.labels, self.n_gt) if n <= 0]
        if empty:
            raise ValueError(f"PSDS is undefined: no reference events of class {', '.join(map(str, empty))}")
        if not self.dataset_duration > 0.0:
            raise ValueError("the dataset duration must be positive")
        self.tp, self.fp, self.ct = t[:, :, 0], t[:, :, 1], t[:, :, 2:]
        self.tpr = self.tp / self.n_gt[None, :].astype(np.float64)
        self.fpr = self.UNIT * self.fp / self.dataset_duration
        has = self.gt_duration > 0.0
        self.ctr = np.zeros(self.ct.shape, np.float64)
        self.ctr[:, :, has] = self.UNIT * self.ct[:, :, has] / self.gt_duration[has]

    @classmethod
    def from_counts(cls, counts, ref, durations):
        """``counts``: a ``PSDSCounts`` (read with ``host()``) or its totals array; ``n_gt`` and ``gt_duration`` come from the
        ``RefEvents``; ``durations``: seconds per file as one number, or a sequence aligned with ``ref.filenames``."""
        totals = counts.host() if hasattr(counts, "host") else counts
        nc = ref.nclass
        per_column = np.diff(ref.ptr_host.astype(np.int64))
        n_gt = per_column.reshape(len(ref), nc).sum(0)
        cls_of_event = np.repeat(np.arange(len(per_column)) % nc, per_column)
        gt_duration = np.bincount(cls_of_event, weights=ref.offset_host - ref.onset_host, minlength=nc)
        if np.ndim(durations) == 0:
            total = float(durations) * len(ref)
        else:
            if len(durations) != len(ref):
                raise ValueError(f"{len(durations)} durations for {len(ref)} files")
            total = float(np.sum(np.asarray(durations, np.float64)))
        return cls(ref.labels, totals, n_gt, gt_duration, total)

    def efpr(self, alpha_ct=0.0):
        """``[K, nclass]``: ``FPR + alpha_ct * mean over the other classes of CTR`` (no other class: the term is 0)."""
        nc = len(self.labels)
        if nc == 1:
            return self.fpr.copy()
        other = self.ctr.sum(2) - np.einsum("kcc->kc", self.ctr)
        return self.fpr + alpha_ct * other / (nc - 1)

    def class_curves(self, axis, alpha_ct=0.0):
        """``[nclass, len(axis)]``: per class the largest TPR among the operating points with ``eFPR <= axis`` (0 below the
        first) - a left-continuous, monotone staircase."""
        e = self.efpr(alpha_ct)
        axis = np.asarray(axis, np.float64)
        out = np.zeros((len(self.labels), len(axis)), np.float64)
        for c in range(len(self.labels)):
            order = np.argsort(e[:, c], kind="stable")
            xs, best = e[order, c], np.maximum.accumulate(self.tpr[order, c])
            at = np.searchsorted(xs, axis, side="right")             # points with eFPR <= x
            out[c] = np.where(at > 0, best[np.maximum(at, 1) - 1], 0.0)
        return out

    def psd_roc(self, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0):
        """``(axis, eff_tpr)``: the sorted union of all classes' eFPR values ``<= max_efpr`` and, at each,
        ``max(0, mean - alpha_st * std)`` of the class curves (population standard deviation)."""
        e = self.efpr(alpha_ct)
        axis = np.unique(e[e <= max_efpr])
        curves = self.class_curves(axis, alpha_ct)
        return axis, np.maximum(0.0, curves.mean(0) - alpha_st * curves.std(0))

    def psds(self, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0):
        """Area under the PSD-ROC up to ``max_efpr`` (nothing below the first axis value), normalised by ``max_efpr``."""
        axis, eff = self.psd_roc(alpha_ct, alpha_st, max_efpr)
        return float(np.sum(eff * np.diff(np.r_[axis, float(max_efpr)])) / max_efpr)


# ---- drop-ins with the reference's signatures -------------------------------------------------------------------------------
def compute_strong_metrics(predictions, valid_df, pooling_time_ratio=None, cfg=None, device="cuda", error_rate=False):
    """Drop-in for evaluation_measures.compute_strong_metrics (lines 234-246): event tables in, the event-based metric out,
    both metrics logged.  The two tables are packed and matched by ``sed_event_counts`` (given-events mode): the device
    matcher serves this route too.  Files = ``valid_df.filename.unique()``, classes = the labels of both tables.
    ``error_rate=True``: one ``sed_error_counts`` call more, and both metrics carry the overall error rate."""
    cfg = cfg or _Cfg
    if pooling_time_ratio is not None:
        LOG.warning("pooling_time_ratio is deprecated, use it in get_predictions() instead.")
        predictions.onset = predictions.onset * pooling_time_ratio / (cfg.sample_rate / cfg.hop_length)
        predictions.offset = predictions.offset * pooling_time_ratio / (cfg.sample_rate / cfg.hop_length)
    files = list(valid_df["filename"].unique())
    labels = sorted(set(valid_df.event_label.dropna().unique()) | set(predictions.event_label.dropna().unique()))
    ref = RefEvents.from_dataframe(valid_df, files, labels, device)
    est = RefEvents.from_dataframe(predictions, files, labels, device)
    ev, seg = event_counts_from_events(est, ref).host()
    ev_o, seg_o = error_counts_from_events(est, ref).host() if error_rate else ([None], [None])
    metric_event, metric_segment = EventMetrics(labels, ev[0], overall=ev_o[0]), SegmentMetrics(labels, seg[0], overall=seg_o[0])
    LOG.info(metric_event)
    LOG.info(metric_segment)
    return metric_event


def get_f_measure_by_class(torch_model, nb_tags, dataloader_, thresholds_=None):
    """Drop-in for evaluation_measures.get_f_measure_by_class (lines 19-83): per-class clip-level F1 of ``torch_model`` over
    ``dataloader_`` (batches ``(batch_x, y)``, ``y`` 0/1).  Forward in the loader's batches, ``sed_weak_counts`` per batch
    into running totals, one device -> host copy at the end."""
    dev = next(torch_model.parameters()).device
    if dev.type != "cuda":
        raise _lib.SedError("get_f_measure_by_class needs the model on the GPU (no CPU fallback)")
    if thresholds_ is None:
        thr = [0.5] * nb_tags
    else:
        assert type(thresholds_) is list
        thr = thresholds_
    thr = torch.tensor(thr, dtype=torch.float32, device=dev).reshape(1, nb_tags)
    counts = torch.zeros(1, nb_tags, 4, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for batch_x, y in dataloader_:
            _, pred_weak = torch_model(batch_x.to(dev))
            if pred_weak.dim() == 3:             # a model predicting only strong outputs (line 49-51)
                pred_weak = pred_weak.max(dim=1).values
            y = torch.as_tensor(y)
            if y.dim() == 3:                     # strong labels: max over time, binarised at 0.5 (lines 53-57)
                y = y.max(dim=1).values > 0.5
            weak_counts(pred_weak, y, thr, counts)
    return f_measure_from_counts(counts.cpu().numpy()[0])


def _metric_pairs(labels, ev, seg, overall=None):
    """One ``(EventMetrics, SegmentMetrics)`` per operating point; ``overall``: ``ErrorCounts.host()`` of the same points."""
    ev_o, seg_o = overall if overall is not None else ([None] * len(ev), [None] * len(ev))
    return [(EventMetrics(labels, ev[k], overall=ev_o[k]), SegmentMetrics(labels, seg[k], overall=seg_o[k]))
            for k in range(len(ev))]


def validate(model, dataset, ref, pooling_time_ratio, thresholds=(0.5,), median_windows=(5,), batch_size=64, cfg=None,
             psds=None, error_rate=False):
    """The fused route for the epoch loop (main.py:324-328 without the event table): ``dataset`` as
    ``inference.get_predictions`` accepts it, forward ``batch_size`` clips at a time, ``sed_event_counts`` per batch into
    running totals, ONE device -> host copy at the end.  ``ref``: the ``RefEvents`` of the same clips in the same order.
    Returns one ``(EventMetrics, SegmentMetrics)`` per operating point.  ``psds``: a ``PSDSCounts`` of the same operating
    points; every batch's posteriors then also go through ``sed_psds_counts`` into it (same forward, same operating-point
    tensors; read it with ``PSDS.from_counts``).  ``error_rate=True``: every batch also goes through ``sed_error_counts``, and
    the metrics carry the overall error rate (``results_overall_metrics()["error_rate"]``); still one copy at the end.  The
    default issues no launch more than before."""
    from .resident import ResidentFeatureSet
    if not getattr(model, "hot_path", False):
        raise _lib.SedError("validate needs a CRNN on the HIP hot path")
    if isinstance(dataset, ResidentFeatureSet) and dataset.noise:
        raise ValueError("validate needs a validation set without noise (ResidentFeatureSet.for_eval)")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.SedError("validate needs the model on the GPU (no CPU fallback)")
    if len(dataset) != len(ref):
        raise ValueError(f"{len(dataset)} clips but reference events of {len(ref)}")
    thr, win = operating_points(thresholds, median_windows, dev)
    counts = Counts(thr.numel(), ref.nclass, dev)
    errors = ErrorCounts(thr.numel(), ref.nclass, dev) if error_rate else None
    if psds is not None and (psds.K, psds.NC) != (counts.K, counts.NC):
        raise ValueError("psds was built for another number of operating points / classes")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i0, _, x in eval_batches(dataset, batch_size, dev):
                strong, _ = model(x)
                event_counts(strong, ref, thr, win, pooling_time_ratio, cfg, clip_offset=i0, counts=counts)
                if psds is not None:
                    psds_counts(strong, ref, thr, win, pooling_time_ratio, cfg, psds.dtc, psds.gtc, psds.cttc, clip_offset=i0,
                                counts=psds)
                if errors is not None:
                    error_counts(strong, ref, thr, win, pooling_time_ratio, cfg, clip_offset=i0, counts=errors)
    finally:
        model.train(was_training)
    if errors is None:
        ev, seg = counts.host()
        return _metric_pairs(ref.labels, ev, seg)
    ev, seg, tail = counts.host(errors.buf)
    return _metric_pairs(ref.labels, ev, seg, errors.parse(tail))


# ---- long recordings: the event table of sed_stitch_decode / sed_stitch_sweep (or given events) of any length ------------------
# One helper family serves the one-point functions (``long_*``: K = 1 into row ``point``, the ``sed_long_*`` entries) and the
# sweep functions (``long_sweep_*``: K points into rows ``point0 ..``, the ``sed_long_sweep_*`` entries, per-column outputs with
# a leading K).
def _long_counts_call(fn, ws_fn, points, est_args, est_cap, ref, tail, err):
    """One ``sed_long_*`` call: ``points`` = ``(K,)`` for the sweep entries, ``()`` for the one-point ones; ``est_args`` =
    (ev_ptr, ev_pairs, num, den, est_on, est_off); ``tail``: the arguments between ``nclass`` (``n_points``) and ``err``."""
    l = _lib.lib()
    n, NC, n_ref = len(ref), ref.nclass, len(ref.onset_host)
    ws_bytes = getattr(l, ws_fn)(int(est_cap), n_ref, n, NC, *points)
    if ws_bytes == 0:
        raise _lib.SedError(f"{ws_fn}: {l.sed_last_error().decode()}")
    ws = _lib.scratch(ws_bytes, ref.device)
    ev_ptr, ev_pairs, num, den, on, off = est_args
    _lib.check(getattr(l, fn)(_lib.ptr(ev_ptr), _lib.ptr(ev_pairs), float(num), float(den), _lib.ptr(on), _lib.ptr(off),
                              int(est_cap), _lib.ptr(ref.ptr64), _lib.ptr(ref.onset), _lib.ptr(ref.offset), n_ref, n, NC, *points,
                              *tail, _lib.ptr(err), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), fn)


def _decoded_args(decoded, ref, pooling_time_ratio, cfg, what, K=None):
    """``(est_args, capacity, K)`` of a decoded table; ``K`` None: the table's own ``n_points`` (1 for ``stitch_decode``'s)."""
    cfg = cfg or _Cfg
    ev_ptr, ev_pairs = decoded["ev_ptr"], decoded["ev_pairs"]
    if K is None:
        K = int(decoded.get("n_points", 1))
    if ev_ptr.device.type != "cuda" or ref.device.type != "cuda":
        raise _lib.SedError(f"{what} needs the decoded table and a RefEvents on the GPU (no CPU fallback)")
    if K < 1 or ev_ptr.dtype != torch.int64 or ev_pairs.dtype != torch.int32 or ev_ptr.numel() != K * len(ref) * ref.nclass + 1:
        raise ValueError(f"decoded: ev_ptr int64 [{K * len(ref) * ref.nclass + 1}] and ev_pairs int32 [capacity, 2] expected "
                         f"({K} points, {len(ref)} recordings, {ref.nclass} classes)")
    return (ev_ptr, ev_pairs.contiguous(), float(pooling_time_ratio), float(cfg.sample_rate / cfg.hop_length), None, None), \
        ev_pairs.shape[0], K


def _events_args(ests, ref, what):
    """K ``RefEvents`` as one CSR in column order (k, rec, c), assembled on the device (the sizes are known on the host); one
    set is taken as it is."""
    ests = list(ests)
    if not ests:
        raise ValueError(f"{what}: need at least one estimated event set")
    for est in ests:
        if est.device.type != "cuda" or ref.device.type != "cuda":
            raise _lib.SedError(f"{what} needs every event set on the GPU (no CPU fallback)")
        if est.filenames != ref.filenames or est.labels != ref.labels:
            raise ValueError("estimated and reference events must cover the same files and classes, in the same order")
    sizes = [len(est.onset_host) for est in ests]
    if len(ests) == 1:
        return (ests[0].ptr64, None, 0.0, 0.0, ests[0].onset, ests[0].offset), sizes[0], 1
    base = np.r_[0, np.cumsum(sizes)]
    ptr = torch.cat([est.ptr64[:-1] + int(base[k]) for k, est in enumerate(ests)] + [ests[-1].ptr64[-1:] + int(base[-2])])
    on = torch.cat([est.onset[:n] for est, n in zip(ests, sizes)] + [ests[-1].onset[-1:]])        # (one trailing element)
    off = torch.cat([est.offset[:n] for est, n in zip(ests, sizes)] + [ests[-1].offset[-1:]])
    return (ptr, None, 0.0, 0.0, on, off), int(base[-1]), len(ests)


def _fold_decode_err(counts, decoded):
    """The decoder's error word into the counts' (bit 128), on the device: ``host()`` raises it, nothing synchronises here."""
    counts.err[:1].bitwise_or_((decoded["err"].reshape(-1)[:1] != 0).to(torch.int32) * 128)


def _long_rows(counts, K, NC, point0, fn):
    """Checks that ``counts`` has the rows ``point0 .. point0 + K - 1`` and puts the long calls' error wording on it."""
    if counts.NC != NC or point0 < 0 or point0 + K > counts.K:
        raise ValueError(f"counts holds {counts.K} operating points of {counts.NC} classes: no rows {point0} .. "
                         f"{point0 + K - 1} of {NC} classes")
    counts.err_what, counts.err_bits = fn, _LONG_ERR_BITS


def _long_event_target(sweep, est_args, est_cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                       per_column):
    n, NC, dev = len(ref), ref.nclass, ref.device
    fn, ws_fn, lead = (("sed_long_sweep_event_counts", "sed_long_sweep_ws_bytes", (K,)) if sweep
                       else ("sed_long_event_counts", "sed_long_score_ws_bytes", ()))
    if counts is None:
        counts = Counts(point0 + K, NC, dev)
    _long_rows(counts, K, NC, point0, fn)
    if per_column:
        counts.ev_columns = torch.empty(*lead, n, NC, 3, dtype=torch.int32, device=dev)
        counts.seg_columns = torch.empty(*lead, n, NC, 4, dtype=torch.int32, device=dev)
    _long_counts_call(fn, ws_fn, lead, est_args, est_cap, ref,
                      (float(t_collar), float(percentage_of_length), float(time_resolution),
                       _lib.ptr(counts.ev_columns) if per_column else None, _lib.ptr(counts.seg_columns) if per_column else None,
                       _lib.ptr(counts.ev[point0]), _lib.ptr(counts.seg[point0])), counts.err)
    return counts


def _long_psds_target(sweep, est_args, est_cap, K, ref, dtc, gtc, cttc, counts, point0, per_column):
    n, NC, dev = len(ref), ref.nclass, ref.device
    fn, ws_fn, lead = (("sed_long_sweep_psds_counts", "sed_long_sweep_ws_bytes", (K,)) if sweep
                       else ("sed_long_psds_counts", "sed_long_score_ws_bytes", ()))
    if counts is None:
        counts = PSDSCounts(point0 + K, NC, dev, dtc, gtc, cttc)
    _long_rows(counts, K, NC, point0, fn)
    if (counts.dtc, counts.gtc, counts.cttc) != (float(dtc), float(gtc), float(cttc)):
        raise ValueError("counts was built for other criteria (dtc, gtc, cttc)")
    if per_column:
        counts.columns = torch.empty(*lead, n, NC, 2 + NC, dtype=torch.int32, device=dev)
    _long_counts_call(fn, ws_fn, lead, est_args, est_cap, ref,
                      (counts.dtc, counts.gtc, counts.cttc, _lib.ptr(counts.columns) if per_column else None,
                       _lib.ptr(counts.totals[point0])), counts.err)
    return counts


def _long_error_target(sweep, est_args, est_cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                       per_file):
    n, NC, dev = len(ref), ref.nclass, ref.device
    fn, ws_fn, lead = (("sed_long_sweep_error_counts", "sed_long_sweep_error_ws_bytes", (K,)) if sweep
                       else ("sed_long_error_counts", "sed_long_error_ws_bytes", ()))
    if counts is None:
        counts = ErrorCounts(point0 + K, NC, dev)
    _long_rows(counts, K, NC, point0, fn)
    counts.err_bits = _LONG_ERROR_ERR_BITS
    if per_file:
        counts.ev_files = torch.empty(*lead, n, 3, dtype=torch.int32, device=dev)
        counts.seg_files = torch.empty(*lead, n, 3, dtype=torch.int32, device=dev)
    _long_counts_call(fn, ws_fn, lead, est_args, est_cap, ref,
                      (float(t_collar), float(percentage_of_length), float(time_resolution),
                       _lib.ptr(counts.ev_files) if per_file else None, _lib.ptr(counts.seg_files) if per_file else None,
                       _lib.ptr(counts.ev[point0]), _lib.ptr(counts.seg[point0])), counts.err)
    return counts


def long_error_counts(decoded, ref, pooling_time_ratio, cfg=None, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0,
                      counts=None, point=0, per_file=False):
    """``long_event_counts`` for the OVERALL error rate: the totals ACCUMULATE into row ``point`` of an ``ErrorCounts``
    (None: a new one of ``point + 1`` rows); ``per_file``: ``counts.ev_files / seg_files [n_rec, 3]`` of this call.  The
    limit of 64 events per side holds per cluster of the recording's events of ALL classes merged by onset."""
    est_args, cap, _ = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_error_counts", K=1)
    counts = _long_error_target(False, est_args, cap, 1, ref, t_collar, percentage_of_length, time_resolution, counts, point,
                                per_file)
    _fold_decode_err(counts, decoded)
    return counts


def long_error_from_events(est, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, counts=None, point=0,
                           per_file=False):
    """The scoring stage alone on two ``RefEvents`` (both sorted by onset inside a column)."""
    est_args, cap, _ = _events_args([est], ref, "long_error_from_events")
    return _long_error_target(False, est_args, cap, 1, ref, t_collar, percentage_of_length, time_resolution, counts, point,
                              per_file)


def long_sweep_error_counts(decoded, ref, pooling_time_ratio, cfg=None, t_collar=0.200, percentage_of_length=0.2,
                            time_resolution=1.0, counts=None, point0=0, per_file=False):
    """``long_error_counts`` for the K operating points ``inference.stitch_sweep`` decoded: ONE ``sed_long_sweep_error_counts``
    call into rows ``point0 .. point0 + K - 1``, the reference side validated and merged once; ``per_file``: ``[K, n_rec, 3]``."""
    est_args, cap, K = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_sweep_error_counts")
    counts = _long_error_target(True, est_args, cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                                per_file)
    _fold_decode_err(counts, decoded)
    return counts


def long_sweep_error_from_events(ests, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, counts=None,
                                 point0=0, per_file=False):
    """The scoring stage alone: ``ests`` is a list of K ``RefEvents`` scored in one call against the one reference side."""
    est_args, cap, K = _events_args(ests, ref, "long_sweep_error_from_events")
    return _long_error_target(True, est_args, cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                              per_file)


def long_event_counts(decoded, ref, pooling_time_ratio, cfg=None, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0,
                      counts=None, point=0, per_column=False):
    """Event- and segment-based counts of long recordings: ``decoded`` is the dict ``inference.stitch_decode`` returns (the
    event table stays on the device), ``ref`` the ``RefEvents`` of the same recordings (files = recordings) and classes.
    The totals ACCUMULATE into row ``point`` of ``counts`` (a ``Counts`` of K operating points; None: a new one of
    ``point + 1`` rows); ``per_column``: ``counts.ev_columns [n_rec, nclass, 3]`` / ``seg_columns [n_rec, nclass, 4]`` of this
    call.  No synchronisation: ``decoded["err"]`` is folded into the counts' error word on the device, ``host()`` raises.
    Columns have no length limit; a CLUSTER (events whose onsets chain within ``t_collar``) holds at most 64 per side.
    Seconds as in ``event_counts``: ``frame * pooling_time_ratio / (sample_rate / hop_length)`` from ``cfg``."""
    est_args, cap, _ = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_event_counts", K=1)
    counts = _long_event_target(False, est_args, cap, 1, ref, t_collar, percentage_of_length, time_resolution, counts, point,
                                per_column)
    _fold_decode_err(counts, decoded)
    return counts


def long_psds_counts(decoded, ref, pooling_time_ratio, cfg=None, dtc=0.5, gtc=0.5, cttc=0.3, counts=None, point=0,
                     per_column=False):
    """``long_event_counts`` for the PSDS criteria: totals into row ``point`` of a ``PSDSCounts`` (its criteria must be
    these); ``per_column``: ``counts.columns [n_rec, nclass, 2 + nclass]``."""
    est_args, cap, _ = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_psds_counts", K=1)
    counts = _long_psds_target(False, est_args, cap, 1, ref, dtc, gtc, cttc, counts, point, per_column)
    _fold_decode_err(counts, decoded)
    return counts


def long_event_counts_from_events(est, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, counts=None, point=0,
                                  per_column=False):
    """The scoring stage alone on two ``RefEvents`` (``est``: the ESTIMATED events of the same files and classes; they need
    not be disjoint, both are sorted by onset as ``RefEvents.from_dataframe`` packs them).  No limit of 64 events per column."""
    est_args, cap, _ = _events_args([est], ref, "long_event_counts_from_events")
    return _long_event_target(False, est_args, cap, 1, ref, t_collar, percentage_of_length, time_resolution, counts, point,
                              per_column)


def long_psds_counts_from_events(est, ref, dtc=0.5, gtc=0.5, cttc=0.3, counts=None, point=0, per_column=False):
    """The PSDS criteria alone on two ``RefEvents``; no limit of 64 events per column."""
    est_args, cap, _ = _events_args([est], ref, "long_psds_counts_from_events")
    return _long_psds_target(False, est_args, cap, 1, ref, dtc, gtc, cttc, counts, point, per_column)


def long_sweep_event_counts(decoded, ref, pooling_time_ratio, cfg=None, t_collar=0.200, percentage_of_length=0.2,
                            time_resolution=1.0, counts=None, point0=0, per_column=False):
    """``long_event_counts`` for the K operating points ``inference.stitch_sweep`` decoded (``decoded["n_points"]``): ONE
    ``sed_long_sweep_event_counts`` call, the reference side prepared once.  The totals ACCUMULATE into rows ``point0 ..
    point0 + K - 1`` of ``counts`` (None: a new ``Counts`` of ``point0 + K`` rows); ``per_column``: ``counts.ev_columns
    [K, n_rec, nclass, 3]`` / ``seg_columns [K, n_rec, nclass, 4]``.  The decoder's error word is folded in on the device."""
    est_args, cap, K = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_sweep_event_counts")
    counts = _long_event_target(True, est_args, cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                                per_column)
    _fold_decode_err(counts, decoded)
    return counts


def long_sweep_psds_counts(decoded, ref, pooling_time_ratio, cfg=None, dtc=0.5, gtc=0.5, cttc=0.3, counts=None, point0=0,
                           per_column=False):
    """``long_sweep_event_counts`` for the PSDS criteria: rows ``point0 .. point0 + K - 1`` of a ``PSDSCounts`` (its criteria
    must be these); ``per_column``: ``counts.columns [K, n_rec, nclass, 2 + nclass]``."""
    est_args, cap, K = _decoded_args(decoded, ref, pooling_time_ratio, cfg, "long_sweep_psds_counts")
    counts = _long_psds_target(True, est_args, cap, K, ref, dtc, gtc, cttc, counts, point0, per_column)
    _fold_decode_err(counts, decoded)
    return counts


def long_sweep_event_counts_from_events(ests, ref, t_collar=0.200, percentage_of_length=0.2, time_resolution=1.0, counts=None,
                                        point0=0, per_column=False):
    """The scoring stage alone: ``ests`` is a list of K ``RefEvents``, the estimated events of K operating points (same files
    and classes as ``ref``, sorted by onset), scored in one call against the one reference side."""
    est_args, cap, K = _events_args(ests, ref, "long_sweep_event_counts_from_events")
    return _long_event_target(True, est_args, cap, K, ref, t_collar, percentage_of_length, time_resolution, counts, point0,
                              per_column)


def long_sweep_psds_counts_from_events(ests, ref, dtc=0.5, gtc=0.5, cttc=0.3, counts=None, point0=0, per_column=False):
    """The PSDS criteria alone on a list of K ``RefEvents`` against one reference side."""
    est_args, cap, K = _events_args(ests, ref, "long_sweep_psds_counts_from_events")
    return _long_psds_target(True, est_args, cap, K, ref, dtc, gtc, cttc, counts, point0, per_column)


def validate_long(model, long_set, ref, thresholds=(0.5,), median_windows=None, batch_size=64, cfg=None, weighting="taper",
                  psds=None, one_blend=True, max_table_bytes=1 << 30, weak_labels=None, weak_thresholds=None, error_rate=False,
                  thresholds_high=None, min_event_lengths=None, min_event_gaps=None, process_order="drop_merge", tag_span=None,
                  min_span_tags=None):
    """``validate`` for a ``LongRecordingSet``: the windows go through the model ONCE, then the K operating points are
    decoded and scored, and ONE device -> host copy ends the call.  ``one_blend=True``: the points are split into chunks
    (``longrec.sweep_chunks``: the event table of a chunk stays within ``max_table_bytes``); per chunk ONE
    ``inference.stitch_sweep`` blends once and decodes all its points, and one ``long_sweep_event_counts`` (and
    ``long_sweep_psds_counts``) scores them against one preparation of the reference.  ``one_blend=False``: per point one
    ``stitch_decode`` and ``long_event_counts`` into row k, the blend repeated per point.  The two routes return identical
    integers; one blend is the default because it measured faster on both workloads of tools/long_bench.py --sweep
    (profiles/long_sweep.json).  ``thresholds``: K entries, each
    a scalar or one value per class; ``median_windows``: the same (or one entry for all points; None: ``cfg.median_window``).
    ``ref``: the ``RefEvents`` of the recordings, in the set's order.  ``psds``: a ``PSDSCounts`` of the same K points, filled
    from the same decodes (read it with ``PSDS.from_counts(psds, ref, long_set.durations())``).
    Returns one ``(EventMetrics, SegmentMetrics)`` per operating point.
    ``weak_labels``: the recordings' reference tags, an ``[n_rec, nclass]`` 0/1 array or ``"from_ref"``
    (``ref.weak_labels()``).  The same forwards then also hand out their attention, the recording-level weak tags are pooled
    ONCE (``inference.stitch_weak``) and scored by ``weak_counts`` at ``weak_thresholds`` (entries as ``thresholds``, the
    default), and the call returns ``(that list, {"f_measure": [Kw, nclass] float64, "counts": [Kw, nclass, 4] int64 (tp, fp,
    fn, tn)})`` - still one device -> host copy.  With ``weak_labels=None`` nothing changes.
    ``error_rate=True``: every decode is also scored by ``long_sweep_error_counts`` (``one_blend``) / ``long_error_counts``
    (per point), and the metrics of every point carry the overall error rate; the default issues no launch more than before.
    ``thresholds_high``: K entries as ``thresholds`` (or one entry for all points), each ``>=`` its point's threshold: every
    point is decoded with two thresholds (``inference.stitch_hysteresis``: ``thresholds`` draws the events, an event is kept
    when the high threshold confirms it).  The chunks are then made of 2 x points sweep points, so a pair never straddles a
    chunk, and per chunk one ``sed_events_hysteresis`` runs between the sweep and the same scorers.  ``one_blend=False``
    raises: the two decodes of a pair come from one sweep.  With ``thresholds_high=None`` nothing changes and no launch is
    added.
    ``min_event_lengths`` / ``min_event_gaps``: seconds, K entries as ``thresholds`` (or one entry for all points; several
    points may share a threshold and differ only here), each a scalar or one value per class: every decoded table goes
    through ``inference.events_process`` (events shorter than the length dropped, events a gap of at most ``min_event_gaps``
    separates fused, in the order ``process_order``) before the scorers - per chunk one call on the chunk's whole table, after
    the two-threshold select; with ``one_blend=False`` one call per point.  Still one device -> host copy; both None: nothing
    changes and no launch is added.
    ``tag_span`` (seconds, as in ``inference.get_long_predictions``) with ``min_span_tags`` (K entries as ``thresholds``, or
    one entry for all points, each a scalar or one value per class; NaN raises): the tag gate.  The forwards also hand out their
    attention, the span-level weak tags are pooled ONCE per call (``inference.stitch_span_tags``), and every decoded table goes
    through ``inference.gate_decoded`` - an event is kept only when it touches a span whose tag exceeds its point's minimum -
    after the two-threshold select and before ``events_process`` and the scorers: per chunk one gate on the chunk's whole
    table, with ``one_blend=False`` one per point.  Still one device -> host copy: the gate's error bits are OR-ed into the
    decode's word and the span tags' word into the first table's.  One of the two without the other raises; both None: nothing
    changes and no launch is added."""
    from .inference import (_order_code, _per_class, gate_decoded, hysteresis_points, long_window_posteriors, process_decoded,
                            process_points, stitch_decode, stitch_error_text, stitch_hysteresis, stitch_span_tags, stitch_sweep,
                            stitch_weak, sweep_points, tag_span_frames)
    from .longrec import LongRecordingSet, sweep_chunks
    cfg = cfg or _Cfg
    thresholds = list(thresholds)
    median_windows = [cfg.median_window] if median_windows is None else list(median_windows)
    K = max(len(thresholds), len(median_windows))
    if len(thresholds) not in (1, K) or len(median_windows) not in (1, K) or K < 1:
        raise ValueError("thresholds and median_windows must have equal lengths (or length 1)")
    if thresholds_high is not None:
        thresholds_high = list(thresholds_high)
        if not one_blend:
            raise ValueError("thresholds_high needs one_blend=True: the two decodes of a pair come from one sweep")
        if len(thresholds_high) not in (1, K):
            raise ValueError(f"thresholds_high must have {K} entries (or one)")
    if (tag_span is None) != (min_span_tags is None):
        raise ValueError("tag_span and min_span_tags go together: the span length in seconds and the K minimum tags")
    gate = tag_span is not None
    if gate:
        min_span_tags = list(min_span_tags)
        if len(min_span_tags) not in (1, K):
            raise ValueError(f"min_span_tags must have {K} entries (or one)")
        tag_span = float(tag_span)
        if not tag_span > 0:
            raise ValueError(f"tag_span must be > 0 seconds, got {tag_span!r}")
        min_tag = np.stack([_per_class(min_span_tags[k % len(min_span_tags)], ref.nclass, np.float32, "a minimum span tag")
                            for k in range(K)])
        if np.isnan(min_tag).any():
            raise ValueError("min_span_tags: NaN keeps no event")
    if weak_labels is None:
        if weak_thresholds is not None:
            raise ValueError("weak_thresholds without weak_labels: there is nothing to score the tags against")
    else:
        if isinstance(weak_labels, str):
            if weak_labels != "from_ref":
                raise ValueError(f'weak_labels is an [n_rec, nclass] 0/1 array or "from_ref", got {weak_labels!r}')
            weak_labels = ref.weak_labels()
        weak_labels = np.asarray(weak_labels)
        if weak_labels.shape != (len(ref), ref.nclass):
            raise ValueError(f"weak_labels is {weak_labels.shape}, expected {(len(ref), ref.nclass)} (recordings, classes)")
        if not np.isin(weak_labels, (0, 1)).all():
            raise ValueError("weak_labels must hold 0 / 1")
        weak_thr = np.stack([_per_class(t, ref.nclass, np.float32, "a weak threshold")
                             for t in (thresholds if weak_thresholds is None else list(weak_thresholds))])
    if not isinstance(long_set, LongRecordingSet):
        raise TypeError(f"long_set must be a LongRecordingSet, got {type(long_set).__name__}")
    if not getattr(model, "hot_path", False):
        raise _lib.SedError("validate_long needs a CRNN on the HIP hot path")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.SedError("validate_long needs the model on the GPU (no CPU fallback)")
    if long_set.n_rec != len(ref):
        raise ValueError(f"{long_set.n_rec} recordings but reference events of {len(ref)}")
    NC = ref.nclass
    process = min_event_lengths is not None or min_event_gaps is not None
    if process:
        _order_code(process_order)
        min_len, max_gap = process_points(min_event_lengths, min_event_gaps, ref.nclass,
                                          long_set.pooling_time_ratio * cfg.hop_length / cfg.sample_rate, K)
    if gate:
        span3 = tag_span_frames(tag_span, long_set.pooling_time_ratio * cfg.hop_length / cfg.sample_rate)
    if psds is not None and (psds.K, psds.NC) != (K, NC):
        raise ValueError("psds was built for another number of operating points / classes")
    if thresholds_high is not None:
        thr_all, thr_high, win_all = hysteresis_points([thresholds[k % len(thresholds)] for k in range(K)], thresholds_high,
                                                       median_windows, NC)
    elif one_blend:
        thr_all, win_all = sweep_points(thresholds, median_windows, NC)
    counts = Counts(K, NC, dev)
    errors = ErrorCounts(K, NC, dev) if error_rate else None
    win_strong = long_window_posteriors(model, long_set, NC, batch_size, want_attention=weak_labels is not None or gate)
    if weak_labels is not None or gate:
        win_strong, win_att = win_strong
    if gate:                                                                     # pooled once; its word travels with the first table's
        span_tags = stitch_span_tags(win_strong, win_att, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames,
                                     long_set.hop3, span3, weighting, rec_frame0_host=long_set.rec_frame0_host)
        span_err = span_tags["err"]

    def gated(out, k0, k1):
        nonlocal span_err
        if span_err is not None:
            out["err"].bitwise_or_(span_err)
            span_err = None
        return gate_decoded(out, span_tags, long_set.n_rec, NC, min_tag[k0:k1])

    if one_blend:
        cap = long_set.capacity(NC)
        if thresholds_high is not None:                                          # chunks of 2 x points sweep points
            chunks = [(k0 // 2, k1 // 2) for k0, k1 in sweep_chunks(2 * K, cap, max_table_bytes, pair=True)]
        else:
            chunks = sweep_chunks(K, cap, max_table_bytes)
        for k0, k1 in chunks:
            if thresholds_high is not None:
                out = stitch_hysteresis(win_strong, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3,
                                        thr_all[k0:k1], thr_high[k0:k1], win_all[k0:k1], weighting, (k1 - k0) * cap)
            else:
                out = stitch_sweep(win_strong, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3,
                                   torch.from_numpy(thr_all[k0:k1]).to(dev), torch.from_numpy(win_all[k0:k1]).to(dev), weighting,
                                   (k1 - k0) * cap)
            if gate:
                out = gated(out, k0, k1)
            if process:
                out = process_decoded(out, long_set.n_rec, NC, min_len[k0:k1], max_gap[k0:k1], process_order)
            long_sweep_event_counts(out, ref, long_set.pooling_time_ratio, cfg, counts=counts, point0=k0)
            if errors is not None:
                long_sweep_error_counts(out, ref, long_set.pooling_time_ratio, cfg, counts=errors, point0=k0)
            if psds is not None:
                long_sweep_psds_counts(out, ref, long_set.pooling_time_ratio, cfg, psds.dtc, psds.gtc, psds.cttc, counts=psds,
                                       point0=k0)
    else:
        for k in range(K):
            out = stitch_decode(win_strong, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3,
                                thresholds[k % len(thresholds)], median_windows[k % len(median_windows)], weighting,
                                long_set.capacity(NC), want_timeline=False)
            if gate:
                out = gated(out, k, k + 1)
            if process:
                out = process_decoded(out, long_set.n_rec, NC, min_len[k:k + 1], max_gap[k:k + 1], process_order)
            long_event_counts(out, ref, long_set.pooling_time_ratio, cfg, counts=counts, point=k)
            if errors is not None:
                long_error_counts(out, ref, long_set.pooling_time_ratio, cfg, counts=errors, point=k)
            if psds is not None:
                long_psds_counts(out, ref, long_set.pooling_time_ratio, cfg, psds.dtc, psds.gtc, psds.cttc, counts=psds, point=k)
    n_err = errors.buf.numel() if errors is not None else 0          # the error totals travel last in the one copy
    if weak_labels is None:
        if errors is None:
            ev, seg = counts.host()
            return _metric_pairs(ref.labels, ev, seg)
        ev, seg, tail = counts.host(errors.buf)
        return _metric_pairs(ref.labels, ev, seg, errors.parse(tail))
    tags = stitch_weak(win_strong, win_att, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3, weighting)
    wc = weak_counts(tags["weak"], torch.from_numpy(weak_labels.astype(np.uint8)), weak_thr)
    ev, seg, tail = counts.host(torch.cat([wc.reshape(-1), tags["err"].to(torch.int64)] + ([errors.buf] if n_err else [])))
    overall = errors.parse(tail[len(tail) - n_err:]) if n_err else None
    tail = tail[:len(tail) - n_err]
    err = int(tail[-1])
    if err:
        raise _lib.SedError(stitch_error_text("sed_stitch_weak", err))
    wc = tail[:-1].reshape(len(weak_thr), NC, 4)
    return (_metric_pairs(ref.labels, ev, seg, overall), {"f_measure": f_measure_from_counts(wc), "counts": wc})
