"""Recordings longer than one clip: the window plan and the HBM-resident set of overlapping windows.

The BiGRU was trained on ``frames``-long clips, so a long recording is cut into overlapping windows of ``frames`` feature
frames, ``hop_frames`` apart; every window goes through the eval forward as a clip of its own, and
``inference.get_long_predictions`` blends the windows' posteriors into one timeline per recording and decodes that
(``sed_stitch_decode``, csrc/stitch.hip).  The windows cost no new extraction code: ``sed_gather_logmel_transform`` gathers
clips from a pool by arbitrary offset and length, so overlapping windows are overlapping clips of a ``ResidentFeatureSet``
whose clip tables point into the recordings.  The dB clamp is per window, as for a clip of its own: a window's input is
byte for byte what the same frames give as a clip, whatever else the recording holds.

Training on such recordings is ``WindowedFeatureSet``: the recordings and their label timelines stay in HBM once, a batch
position is a window ``(item, start label frame)`` gathered - features and sliced labels - by
``sed_gather_window_logmel_transform``, with a fixed number of windows per recording and epoch and fresh crop starts per epoch.
"""
import collections

import numpy as np
import torch

from . import _lib
from .augment import AugmentPolicy
from .resident import ResidentFeatureSet

WEIGHTINGS = {"uniform": 0, "taper": 1}


def default_hop_frames(frames, pooling_time_ratio=8):
    """The largest positive multiple of ``pooling_time_ratio`` not above ``frames // 2`` (half-overlapping windows)."""
    pool = int(pooling_time_ratio)
    if pool < 1 or int(frames) // pool < 1:
        raise ValueError(f"frames {frames} must hold at least one label frame of {pooling_time_ratio} feature frames")
    return max(pool, (int(frames) // 2) // pool * pool)


def check_hop_frames(hop_frames, frames, pooling_time_ratio=8):
    """``hop_frames`` (None: the default) as an int, or ValueError: a positive multiple of ``pooling_time_ratio``, at most
    ``(frames // pool) * pool`` - window and timeline label frames stay aligned and no timeline frame falls between windows."""
    pool = int(pooling_time_ratio)
    if hop_frames is None:
        return default_hop_frames(frames, pool)
    if pool < 1 or int(frames) // pool < 1:
        raise ValueError(f"frames {frames} must hold at least one label frame of {pooling_time_ratio} feature frames")
    if isinstance(hop_frames, bool) or int(hop_frames) != hop_frames:
        raise ValueError(f"hop_frames must be an integer, got {hop_frames!r}")
    hop = int(hop_frames)
    if hop < pool or hop % pool or hop > (int(frames) // pool) * pool:
        raise ValueError(f"hop_frames must be a positive multiple of {pool} and at most {(int(frames) // pool) * pool}, got {hop}")
    return hop


def window_plan(L, frames, pool=8, hop3=None):
    """The windows of a recording of ``L >= 1`` feature frames: a dict with
    ``L3``      timeline label frames, max(1, L // pool) (frames that exist only as padding are not decoded),
    ``n_w``     windows: 1 if L3 <= T3, else 1 + ceil((L3 - T3) / hop3), T3 = frames // pool,
    ``start``   [n_w] first feature frame of window j: j * hop3 * pool,
    ``real``    [n_w] real feature frames of window j: min(frames, L - start) (the gather pads the rest),
    ``t0``      [n_w] first timeline frame window j covers: j * hop3 (it covers T3 of them)."""
    L, T, pool = int(L), int(frames), int(pool)
    T3 = T // pool
    if L < 1 or T3 < 1:
        raise ValueError(f"need L >= 1 and frames >= pool, got L {L}, frames {frames}, pool {pool}")
    hop3 = check_hop_frames(None if hop3 is None else int(hop3) * pool, T, pool) // pool
    L3 = max(1, L // pool)
    n_w = 1 if L3 <= T3 else 1 + -(-(L3 - T3) // hop3)
    t0 = np.arange(n_w, dtype=np.int64) * hop3
    start = t0 * pool
    return {"L3": L3, "n_w": n_w, "T3": T3, "hop3": hop3, "start": start, "real": np.minimum(T, L - start), "t0": t0}


MAX_SWEEP_POINTS = 4096          # operating points per sed_stitch_sweep / sed_long_sweep_* call


def sweep_chunks(K, capacity_per_point, max_table_bytes, limit=2 ** 31 - 1024, pair=False):
    """The ranges ``[(k0, k1), ...]`` that split ``K`` operating points into ``sed_stitch_sweep`` calls: consecutive, covering
    ``0 .. K`` once, each as long as possible with its event table ``(k1 - k0) * capacity_per_point`` rows of 8 bytes
    (``ev_pairs``) within ``max_table_bytes`` and its capacity below ``limit`` (what the scorers accept); never fewer than one
    point per chunk, never more than ``MAX_SWEEP_POINTS``.  ``pair=True`` (the two-threshold decode: ``K`` is twice the number
    of threshold pairs): every chunk holds an even number of points, never fewer than two - the two decodes of whole pairs."""
    K, cap = int(K), int(capacity_per_point)
    if K < 1 or cap < 0 or (pair and K % 2):
        raise ValueError(f"need K >= 1 (even for pairs) and capacity_per_point >= 0, got {K}, {cap}")
    per = K if cap == 0 else min(int(max_table_bytes) // (8 * cap), (int(limit) - 1) // cap)
    per = max(1, min(per, K, MAX_SWEEP_POINTS))
    if pair:
        per = max(2, per - per % 2)
    return [(k0, min(k0 + per, K)) for k0 in range(0, K, per)]


def recording_tag_runs(n_windows, max_windows):
    """``n_windows`` [n_rec] windows per recording -> ``[(r0, r1), ...]``: runs of consecutive recordings covering
    ``0 .. n_rec`` once, packed greedily - a run takes recordings while its windows stay within ``max_windows``.  A recording
    with more than ``max_windows`` windows raises ``ValueError`` (it needs more than one forward: not provided)."""
    n_windows = np.asarray(n_windows, dtype=np.int64)
    max_windows = int(max_windows)
    if n_windows.ndim != 1 or n_windows.size < 1 or (n_windows < 1).any() or max_windows < 1:
        raise ValueError("need at least one recording, at least one window per recording and max_windows >= 1")
    if int(n_windows.max()) > max_windows:
        r = int(n_windows.argmax())
        raise ValueError(f"recording {r} has {int(n_windows[r])} windows, more than max_windows = {max_windows}: a recording "
                         "must fit in one forward")
    runs, r0, used = [], 0, 0
    for r, n in enumerate(n_windows):
        if used + int(n) > max_windows:
            runs.append((r0, r))
            r0, used = r, 0
        used += int(n)
    runs.append((r0, len(n_windows)))
    return runs


def cover_lo(u, T3, hop3):
    """The first window that covers timeline frame ``u`` (``st_cover_lo`` of csrc/stitch.hip, restated)."""
    u, T3, hop3 = int(u), int(T3), int(hop3)
    return (u - T3) // hop3 + 1 if u >= T3 else 0


def cover_hi(u, n_w, hop3):
    """The last window of a recording's ``n_w`` that covers timeline frame ``u`` (``st_cover_hi``, restated)."""
    return min(int(u) // int(hop3), int(n_w) - 1)


SpanPiece = collections.namedtuple("SpanPiece", "rec s0 s1 j0 j1 off L3")
SpanPiece.__doc__ = """A piece of recording ``rec``: its spans ``s0 .. s1 - 1`` and its windows ``j0 .. j1`` (both ends included),
exactly those that cover the spans' frames.  As a "recording" of ``sed_stitch_piece_span_tags`` it has ``L3`` local frames
(local frame 0 is the recording's frame ``j0 * hop3``) and its first span starts at local frame ``off``."""


def span_windows(s0, s1, n_w, L3, T3, hop3, span3):
    """``(j0, j1)``: the windows of a recording (``n_w`` windows, ``L3`` frames) that cover the frames of its spans
    ``s0 .. s1 - 1``; the piece that holds the last span takes the recording's last window."""
    n_spans = -(-int(L3) // int(span3))
    j0 = cover_lo(s0 * span3, T3, hop3)
    j1 = n_w - 1 if s1 >= n_spans else cover_hi(min(s1 * span3, L3) - 1, n_w, hop3)
    return j0, j1


def span_pieces(n_windows, L3s, T3, hop3, span3, max_windows):
    """The batches of one span-tag epoch over recordings of ANY length, pure numpy: a list of batches, a batch a list of
    ``SpanPiece``.  ``n_windows`` / ``L3s`` [n_rec]: windows and timeline frames per recording; ``span3`` label frames per
    span (as ``inference.span_table`` clamped it).

    A recording with at most ``max_windows`` windows is never split: runs of such recordings are packed exactly as
    ``recording_tag_runs`` packs them, a batch of them is one piece per recording with ``off = 0`` and all its spans.  A
    recording with more windows gets batches of its own, one piece each, formed greedily over its spans in order: spans join a
    piece while the windows that cover them (``span_windows``) stay within ``max_windows``.  The boundary windows of
    neighbouring pieces cover spans of both, so they are forwarded in both batches.  A span that alone needs more than
    ``max_windows`` windows raises ``ValueError``."""
    n_windows, L3s = np.asarray(n_windows, dtype=np.int64), np.asarray(L3s, dtype=np.int64)
    T3, hop3, span3, max_windows = int(T3), int(hop3), int(span3), int(max_windows)
    if n_windows.ndim != 1 or n_windows.size < 1 or L3s.shape != n_windows.shape or (n_windows < 1).any() or (L3s < 1).any() \
            or max_windows < 1:
        raise ValueError("need at least one recording, at least one window and one frame per recording and max_windows >= 1")
    if not 1 <= hop3 <= T3 or span3 < 1:
        raise ValueError(f"need 1 <= hop3 <= T3 and span3 >= 1, got hop3 {hop3}, T3 {T3}, span3 {span3}")
    if ((n_windows - 1) * hop3 + T3 < L3s).any():
        raise ValueError("a recording's windows do not cover its frames")
    batches, short = [], []

    def flush():
        if short:
            for r0, r1 in recording_tag_runs(n_windows[short[0]:short[-1] + 1], max_windows):
                batches.append([SpanPiece(r, 0, -(-int(L3s[r]) // span3), 0, int(n_windows[r]) - 1, 0, int(L3s[r]))
                                for r in range(short[0] + r0, short[0] + r1)])
            short.clear()

    for r, (n_w, L3) in enumerate(zip(n_windows.tolist(), L3s.tolist())):
        if n_w <= max_windows:
            short.append(r)
            continue
        flush()
        n_spans, s0 = -(-L3 // span3), 0
        while s0 < n_spans:
            j0, j1 = span_windows(s0, s0 + 1, n_w, L3, T3, hop3, span3)
            if j1 - j0 + 1 > max_windows:
                raise ValueError(f"span {s0} of recording {r} alone needs {j1 - j0 + 1} windows, more than max_windows = "
                                 f"{max_windows}")
            s1 = s0 + 1
            while s1 < n_spans and span_windows(s0, s1 + 1, n_w, L3, T3, hop3, span3)[1] - j0 + 1 <= max_windows:
                s1 += 1
            j1 = span_windows(s0, s1, n_w, L3, T3, hop3, span3)[1]
            batches.append([SpanPiece(r, s0, s1, j0, j1, s0 * span3 - j0 * hop3, min(L3, j1 * hop3 + T3) - j0 * hop3)])
            s0 = s1
    flush()
    return batches


def span_piece_tables(batch, rec_win0_host, rec_span0_host):
    """The tables of one ``span_pieces`` batch: ``(rec_win0 int32 [n + 1], rec_frame0 int64 [n + 1], rec_span0 int64 [n + 1],
    rec_span_off int32 [n], first window of the set, windows, first span row of the set, span rows)`` - the first three rebased
    to the batch, as ``sed_stitch_piece_span_tags`` takes them; the batch's windows and span rows are contiguous in the set."""
    n_w = [p.j1 - p.j0 + 1 for p in batch]
    w0 = int(rec_win0_host[batch[0].rec]) + batch[0].j0
    g0 = int(rec_span0_host[batch[0].rec]) + batch[0].s0
    for a, b in zip(batch[:-1], batch[1:]):              # (pieces of one batch are whole consecutive recordings)
        assert b.rec == a.rec + 1 and a.j1 + 1 == int(rec_win0_host[b.rec] - rec_win0_host[a.rec]) and b.j0 == b.s0 == 0
    return (np.concatenate([[0], np.cumsum(n_w)]).astype(np.int32),
            np.concatenate([[0], np.cumsum([p.L3 for p in batch])]).astype(np.int64),
            np.concatenate([[0], np.cumsum([p.s1 - p.s0 for p in batch])]).astype(np.int64),
            np.asarray([p.off for p in batch], dtype=np.int32), w0, int(sum(n_w)), g0, int(sum(p.s1 - p.s0 for p in batch)))


class LongRecordingSet(ResidentFeatureSet):
    """Recordings of any lengths, resident in one HBM pool; the set's "clips" are their overlapping windows.

    It is an evaluation set (no targets, no noise, no epoch tables): ``eval_batch(i0, n)``, ``n_clips`` and ``len()`` address the
    WINDOWS exactly as a ``for_eval`` set addresses its clips, so ``inference.eval_batches`` runs on it unchanged.  The windows
    of a recording are contiguous and in time order; ``rec_win0`` / ``rec_frame0`` (device, CSR) say which windows and which
    timeline frames belong to which recording."""

    @classmethod
    def from_arrays(cls, features, frames, hop_frames=None, pooling_time_ratio=8, scaler=None, filenames=None, device="cuda",
                    math_dtype="f64"):
        """``features``: sequence of linear-mel arrays [L_i, n_mels], any L_i >= 1; ``hop_frames``: feature frames between
        windows (``check_hop_frames``; default: about half a window); ``filenames``: one name per recording."""
        self = cls.__new__(cls)
        hop = check_hop_frames(hop_frames, frames, pooling_time_ratio)
        feats = list(features)
        self._setup(feats, None, [len(feats)], None, frames, scaler, None, device, None, math_dtype, 0)
        self._set_windows(self.clip_frames_host.astype(np.int64), hop, pooling_time_ratio, filenames)
        return self

    @classmethod
    def from_waveforms(cls, waves, extractor, frames, hop_frames=None, pooling_time_ratio=8, scaler=None, filenames=None,
                       math_dtype="f64"):
        """``waves``: list of 1-D sample arrays of any lengths; ``extractor``: a ``features.FeatureExtractor``.  One
        ``calculate_mel_spec_batch`` call per recording (any length whose reflect padding is defined); the linear mel stays on
        the extractor's device and becomes the pool."""
        hop = check_hop_frames(hop_frames, frames, pooling_time_ratio)
        mels = [extractor.calculate_mel_spec_batch(torch.as_tensor(np.asarray(w, dtype=np.float32)).reshape(1, -1))[0]
                for w in waves]
        if not mels:
            raise ValueError("no clips")
        n_mels = int(mels[0].shape[1])
        self = cls.__new__(cls)
        # every field but the pool comes from the base class (a one-frame placeholder pool, replaced below by the device one)
        self._setup([np.zeros((1, n_mels), dtype=np.float32)], None, [1], None, frames, scaler, None, extractor.device, None,
                    math_dtype, 0)
        lengths = np.array([int(m.shape[0]) for m in mels], dtype=np.int64)
        if lengths.min() < 1 or lengths.max() * n_mels >= 2 ** 31:
            raise ValueError(f"recordings of {lengths.min()} .. {lengths.max()} frames: need 1 <= frames and frames * n_mels < 2^31")
        self.pool = torch.cat([m.reshape(-1) for m in mels])
        self._set_windows(lengths, hop, pooling_time_ratio, filenames)
        return self

    def _set_windows(self, lengths, hop_frames, pooling_time_ratio, filenames):
        """Replace the base class's clip tables (one clip per recording) by the windows' and build the per-recording tables."""
        self.pooling_time_ratio = int(pooling_time_ratio)
        self.hop_frames = int(hop_frames)
        self.hop3 = self.hop_frames // self.pooling_time_ratio
        self.T3 = self.frames // self.pooling_time_ratio
        self.n_rec = len(lengths)
        self.rec_frames_host = np.asarray(lengths, dtype=np.int64)
        rec_offset = np.concatenate([[0], np.cumsum(self.rec_frames_host)[:-1]]).astype(np.int64)
        plans = [window_plan(L, self.frames, self.pooling_time_ratio, self.hop3) for L in self.rec_frames_host]
        self.rec_win0_host = np.concatenate([[0], np.cumsum([p["n_w"] for p in plans])]).astype(np.int32)
        self.rec_frame0_host = np.concatenate([[0], np.cumsum([p["L3"] for p in plans])]).astype(np.int64)
        self.total_frames = int(self.rec_frame0_host[-1])
        self.clip_offset_host = np.concatenate([o + p["start"] for o, p in zip(rec_offset, plans)]).astype(np.int64)
        self.clip_frames_host = np.concatenate([p["real"] for p in plans]).astype(np.int32)
        self.n_clips = int(self.rec_win0_host[-1])
        self.stream_sizes = [self.n_clips]
        self.max_clip_frames = int(self.clip_frames_host.max())          # <= frames
        self.clip_offset = torch.from_numpy(self.clip_offset_host).to(self.device)
        self.clip_frames = torch.from_numpy(self.clip_frames_host).to(self.device)
        self.rec_win0 = torch.from_numpy(self.rec_win0_host).to(self.device)
        self.rec_frame0 = torch.from_numpy(self.rec_frame0_host).to(self.device)
        self._all = None
        self._tag_batches = None
        self._span_tag_batches = None
        if filenames is None:
            filenames = [f"recording_{i}" for i in range(self.n_rec)]
        if len(filenames) != self.n_rec:
            raise ValueError(f"{len(filenames)} filenames for {self.n_rec} recordings")
        self.filenames = list(filenames)

    def tag_batches(self, max_windows):
        """The batches ``train.train_recording_tags`` runs over this set, built once per ``max_windows`` and kept:
        ``(runs, at, rec_win0, rec_frame0)`` - ``runs`` from ``recording_tag_runs``; the batch-local tables of every run
        (rebased to the run's first window / frame) concatenated into one device tensor each, run ``k``'s tables are the
        slices ``[at[k]:at[k + 1]]``."""
        if self._tag_batches is None or self._tag_batches[0] != int(max_windows):
            runs = recording_tag_runs(np.diff(self.rec_win0_host), max_windows)
            w = np.concatenate([self.rec_win0_host[r0:r1 + 1] - self.rec_win0_host[r0] for r0, r1 in runs]).astype(np.int32)
            f = np.concatenate([self.rec_frame0_host[r0:r1 + 1] - self.rec_frame0_host[r0] for r0, r1 in runs]).astype(np.int64)
            at = np.concatenate([[0], np.cumsum([r1 - r0 + 1 for r0, r1 in runs])])
            self._tag_batches = (int(max_windows), runs, at, torch.from_numpy(w).to(self.device), torch.from_numpy(f).to(self.device))
        return self._tag_batches[1:]

    def span_tag_batches(self, max_windows, span3):
        """The batches ``train.train_span_tags(split_long=True)`` runs over this set, built once per ``(max_windows, span3)``
        and kept: a dict with ``batches`` (``span_pieces``' - a recording with more than ``max_windows`` windows is cut into
        pieces, whose boundary windows are forwarded in both neighbours), ``at`` and the device tensors ``rec_win0``,
        ``rec_frame0``, ``rec_span0``, ``rec_span_off`` - the batch-local tables of ``span_piece_tables`` concatenated, batch
        ``k``'s are the slices ``[at[k]:at[k + 1]]`` (``rec_span_off`` carries one unused entry per batch to share ``at``) - and
        on the host ``tables`` (the same per batch), ``win`` [(first window, windows)] for ``eval_batch``, ``rows`` [(first span
        row, span rows)] of the set's span table and ``forwarded`` (windows forwarded per epoch / windows of the set).
        ``span3`` is taken as given (``inference.span_table`` clamps it to the longest recording)."""
        key = (int(max_windows), int(span3))
        if self._span_tag_batches is None or self._span_tag_batches[0] != key:
            L3s = np.diff(self.rec_frame0_host)
            batches = span_pieces(np.diff(self.rec_win0_host), L3s, self.T3, self.hop3, key[1], key[0])
            span0 = np.concatenate([[0], np.cumsum((L3s + key[1] - 1) // key[1])]).astype(np.int64)
            tables = [span_piece_tables(b, self.rec_win0_host, span0) for b in batches]
            dev = lambda i, pad: torch.from_numpy(np.concatenate([np.r_[t[i], pad] for t in tables])).to(self.device)
            self._span_tag_batches = (key, {
                "batches": batches, "at": np.concatenate([[0], np.cumsum([len(b) + 1 for b in batches])]),
                "rec_win0": dev(0, np.zeros(0, np.int32)), "rec_frame0": dev(1, np.zeros(0, np.int64)),
                "rec_span0": dev(2, np.zeros(0, np.int64)), "rec_span_off": dev(3, np.zeros(1, np.int32)),
                "tables": [t[:4] for t in tables], "win": [t[4:6] for t in tables], "rows": [t[6:8] for t in tables],
                "forwarded": sum(t[5] for t in tables) / float(self.n_clips)})
        return self._span_tag_batches[1]

    def capacity(self, nclass):
        """Events ``sed_stitch_decode`` can never exceed: sum over recordings of nclass * ceil(L3 / 2)."""
        L3 = np.diff(self.rec_frame0_host)
        return int(nclass) * int(((L3 + 1) // 2).sum())

    def durations(self, cfg=None):
        """Seconds of every recording's decoded timeline, ``L3 * pooling_time_ratio / (sample_rate / hop_length)`` - the scale
        of the event table's seconds; what ``metrics.PSDS.from_counts(..., durations=...)`` takes.  ``cfg``: sample_rate /
        hop_length (default: baseline/config.py's)."""
        if cfg is None:
            from .inference import _Cfg as cfg
        return np.diff(self.rec_frame0_host) * self.pooling_time_ratio / (cfg.sample_rate / cfg.hop_length)


def encode_timeline(events_of_file, n_rows, class_labels, cfg, pooling_time_ratio=8):
    """The label timeline [n_rows, nclass] float32 of one strongly labelled file - what the reference does to it, on a
    timeline of any length: onsets / offsets in seconds become label frames by
    ``x * cfg.sample_rate // cfg.hop_length // pooling_time_ratio`` (main.py:227-228: float floor division twice, then
    ``int()``), ``y[onset:offset, class] = 1`` with the offset row excluded and rows beyond the timeline dropped
    (utils.py:92-94), NaN labels skipped.  ``events_of_file``: a DataFrame with onset, offset, event_label columns, or an
    iterable of (onset, offset, event_label)."""
    labels = list(class_labels)
    y = np.zeros((int(n_rows), len(labels)), dtype=np.float32)
    if hasattr(events_of_file, "itertuples"):
        events_of_file = zip(events_of_file["onset"], events_of_file["offset"], events_of_file["event_label"])
    for onset, offset, label in events_of_file:
        if label is None or label != label:                    # NaN: a file without events
            continue
        on = int(float(onset) * cfg.sample_rate // cfg.hop_length // pooling_time_ratio)
        off = int(float(offset) * cfg.sample_rate // cfg.hop_length // pooling_time_ratio)
        y[on:off, labels.index(label)] = 1
    return y


SAMPLINGS = ("random", "grid", "events")
CROP_ERR_BITS = {8: "nclass above 16", 16: "an item index or an item's label rows out of range", 32: "a start_hi outside its item"}


class WindowedFeatureSet(ResidentFeatureSet):
    """A training set whose pool items may be recordings longer than one clip: every batch position is a WINDOW
    ``(item, start3)`` of ``frames`` feature frames starting at label frame ``start3`` of the item, its target sliced from the
    item's label timeline by the same launch (``sed_gather_window_logmel_transform``).  Features and timelines are uploaded
    once; fresh crops per epoch cost one small table.

    Per stream, ``windowed`` says how its items are used.  A non-windowed stream behaves as a ``ResidentFeatureSet``'s: one
    window at ``start3 = 0`` per item (truncated, padded or exactly ``frames``).  In a windowed stream item i contributes
    ``n_w(i) = window_plan(L_i, frames, pool, hop3)["n_w"]`` windows every epoch - as many as ``LongRecordingSet`` infers it
    with - so stream sizes, ``n_steps``, ``rampup_length`` and ``global_step`` are constants of the run.  With
    ``L3 = max(1, L_i // pool)`` and ``hi = max(0, L3 - T3)``, window j of the item starts at
      ``sampling="grid"``    ``min(j * hop3, hi)``, the same in every epoch;
      ``sampling="random"``  an integer uniform on ``[0, hi]``: ``np.random.default_rng([seed, epoch])`` draws ``n_w(i)`` of
                             them per windowed item, in item order, identically on every rank;
      ``sampling="events"``  event-aware: a slot is, with probability ``event_fraction``, given a class drawn uniformly
                             among the classes the item's timeline holds and then a start with probability proportional to
                             the active frames (label > 0) of that class its window covers - so the window holds at least
                             one; every other slot, and every slot of an item without events, is uniform on ``[0, hi]``.
                             The draws are the host's (``event_draws``: ``default_rng([seed, epoch])``, identical on every
                             rank); the starts come from the label pool where it lives (``sed_window_activity``,
                             ``sed_window_event_starts``; the definition is in include/dcase_sed.h), recomputed on every
                             call: labels rewritten in place by ``relabel`` move the next epoch's crops.  The set must be
                             on a GPU (``SedError`` otherwise: no CPU fallback).  ``event_weights()`` and
                             ``slot_classes(epoch)`` are its diagnostics.
    An item with ``L3 >= T3`` therefore never yields a window with padded label frames.  The stream permutations come from
    numpy's GLOBAL generator exactly as ``ResidentFeatureSet.epoch_rows`` draws them (over the streams' window slots; slot =
    item in a non-windowed stream): random crops never change the number of global draws.

    ``relabel(items, table, rec_frame0_host, ...)`` (inherited) rewrites the label timelines of whole items in place from a
    decoded event table on the device - pseudo strong labels for the next round (``inference.pseudo_label``).

    Not provided: ``from_waveforms``, crop starts finer than one label frame, class balance across the whole set (the
    event-aware draw balances the classes of each item), training on recordings that carry only weak labels (the pooled recording-level tag of ``inference.stitch_weak`` has no
    backward)."""

    row_shape = (2,)

    @classmethod
    def from_arrays(cls, features, labels, stream_sizes, batch_sizes, frames, windowed, pooling_time_ratio=8, hop_frames=None,
                    sampling="random", scaler=None, augment_type="noise", device="cuda", process_group=None, math_dtype="f64",
                    seed=0, augment=None, event_fraction=0.5):
        """``features[i]``: [L_i, n_mels], any L_i >= 1; ``labels[i]``: [R_i, nclass] float32, any R_i >= 1 - the label
        timeline of the whole item at label-frame rate (rows a window reaches beyond R_i are 0); ``windowed``: one bool per
        stream; ``hop_frames``: as ``LongRecordingSet`` (it only sets how many windows an item contributes, and the grid);
        ``event_fraction`` in [0, 1]: the share of slots ``sampling="events"`` draws event-aware."""
        self = cls.__new__(cls)
        feats, labels, sizes = list(features), list(labels), [int(s) for s in stream_sizes]
        if sampling not in SAMPLINGS:
            raise ValueError(f"sampling must be one of {SAMPLINGS}, got {sampling!r}")
        if not 0.0 <= float(event_fraction) <= 1.0:
            raise ValueError(f"event_fraction must lie in [0, 1], got {event_fraction!r}")
        if len(labels) != len(feats):
            raise ValueError(f"{len(labels)} label timelines for {len(feats)} items")
        windowed = [bool(w) for w in windowed]
        if len(windowed) != len(sizes):
            raise ValueError(f"windowed has {len(windowed)} entries for {len(sizes)} streams")
        if batch_sizes is None:
            raise ValueError("a WindowedFeatureSet is a training set: it needs batch sizes")
        if augment is not None and not isinstance(augment, AugmentPolicy):
            raise TypeError(f"augment must be an AugmentPolicy or None, got {type(augment).__name__}")
        pool = int(pooling_time_ratio)
        hop = check_hop_frames(hop_frames, frames, pool)
        # the pool, the scaler and the rank come from the base class (built as a gather-only set; the batch layout follows)
        self._setup(feats, None, sizes, None, frames, scaler, augment_type, device, process_group, math_dtype, seed)
        self.augment = augment
        self.pooling_time_ratio, self.hop_frames, self.hop3, self.T3 = pool, hop, hop // pool, self.frames // pool
        self.sampling, self.windowed, self.event_fraction, self._crop = sampling, windowed, float(event_fraction), None
        self.max_win_frames = min(self.frames, self.max_clip_frames)
        # the label pool: timelines concatenated along rows
        labels = [np.asarray(y, dtype=np.float32) for y in labels]
        nclass = labels[0].shape[1] if labels[0].ndim == 2 else -1
        for i, y in enumerate(labels):
            if y.ndim != 2 or y.shape[1] != nclass or y.shape[0] < 1:
                raise ValueError(f"item {i}: labels of shape {y.shape}, expected [rows >= 1, {nclass}]")
        rows = np.array([y.shape[0] for y in labels], dtype=np.int64)
        self.nclass = int(nclass)
        self.label_rows_host = rows.astype(np.int32)
        self.label_offset_host = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
        self.label_pool = torch.from_numpy(np.concatenate(labels, axis=0)).to(self.device)
        self.label_offset = torch.from_numpy(self.label_offset_host).to(self.device)
        self.label_rows = torch.from_numpy(self.label_rows_host).to(self.device)
        self.target_shape = (self.T3, self.nclass)
        # the window slots: (item, j) for j < n_w(item) in a windowed stream, (item, 0) otherwise - in item order
        L = self.clip_frames_host.astype(np.int64)
        self.start_hi_host = np.maximum(0, np.maximum(1, L // pool) - self.T3)
        in_windowed = np.repeat(np.array(windowed, dtype=bool), sizes)
        self.n_w_host = np.array([window_plan(l, self.frames, pool, self.hop3)["n_w"] if w else 1
                                  for l, w in zip(L, in_windowed)], dtype=np.int64)
        self.item_windowed = in_windowed
        self.slot_item = np.repeat(np.arange(self.n_clips, dtype=np.int64), self.n_w_host)
        self.slot_j = np.concatenate([np.arange(n, dtype=np.int64) for n in self.n_w_host])
        ends = np.cumsum(sizes)
        self.window_stream_sizes = [int(self.n_w_host[lo:hi].sum()) for lo, hi in zip(np.r_[0, ends[:-1]], ends)]
        self._set_batches(self.window_stream_sizes, batch_sizes)
        return self

    @classmethod
    def from_events(cls, features, events, filenames, class_labels, cfg, stream_sizes, batch_sizes, frames, windowed,
                    pooling_time_ratio=8, **kwargs):
        """Strongly labelled items: ``events`` is the reference's strong DataFrame (filename, onset, offset in SECONDS,
        event_label), ``filenames[i]`` names item i; every item's timeline has its ``L3 = max(1, L_i // pool)`` rows
        (``encode_timeline``).  The other arguments are ``from_arrays``'s."""
        feats = list(features)
        if len(filenames) != len(feats):
            raise ValueError(f"{len(filenames)} filenames for {len(feats)} items")
        by_file = {k: v for k, v in events.groupby("filename")}
        empty = events.iloc[:0]
        labels = [encode_timeline(by_file.get(name, empty), max(1, int(np.shape(f)[0]) // int(pooling_time_ratio)), class_labels,
                                  cfg, pooling_time_ratio) for f, name in zip(feats, filenames)]
        self = cls.from_arrays(feats, labels, stream_sizes, batch_sizes, frames, windowed, pooling_time_ratio, **kwargs)
        self.filenames = list(filenames)
        return self

    # ---- epoch tables --------------------------------------------------------------------------------------------------------
    def slot_starts(self, epoch):
        """start3 of every window slot in epoch ``epoch`` [n_slots] int64 (the same on every rank)."""
        hi = self.start_hi_host[self.slot_item]
        if self.sampling == "grid":
            return np.minimum(self.slot_j * self.hop3, hi)
        if self.sampling == "events":
            return self._event_slots(epoch)[0]
        rng = np.random.default_rng([self.seed, int(epoch)])
        start = np.zeros(len(self.slot_item), dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(self.n_w_host)[:-1]])
        for i in np.flatnonzero(self.item_windowed):
            start[first[i]:first[i] + self.n_w_host[i]] = rng.integers(0, self.start_hi_host[i] + 1, size=self.n_w_host[i])
        return start

    def event_draws(self, epoch):
        """The host draws of ``sampling="events"`` for epoch ``epoch``, over all window slots, in this order: ``u`` uint64
        uniform on [0, 2^64), ``v`` int64 uniform on [0, 2^31), ``m`` bool, true with probability ``event_fraction``."""
        n = len(self.slot_item)
        rng = np.random.default_rng([self.seed, int(epoch)])
        u = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        v = rng.integers(0, 2 ** 31, n)
        m = rng.random(n) < self.event_fraction
        return u, v, m

    def _crop_tables(self):
        """The device tables of the event-aware draw, built on first use and kept: the CSR label rows, ``start_hi`` (0 for an
        item of a non-windowed stream: its one window starts at 0), the slots' items, and the entries' outputs."""
        if self.device.type != "cuda":
            raise _lib.SedError('WindowedFeatureSet: sampling="events" needs the set on a GPU device (no CPU fallback)')
        if self._crop is None:
            n, nc, n_slots, dev = self.n_clips, self.nclass, len(self.slot_item), self.device
            total = int(self.label_rows_host.astype(np.int64).sum())
            ws_bytes = _lib.lib().sed_window_activity_ws_bytes(total, n, nc)
            if ws_bytes == 0:
                raise _lib.SedError(f"sed_window_activity_ws_bytes: {_lib.lib().sed_last_error().decode()}")
            self._crop = {
                "total": total,
                "row0": torch.from_numpy(np.r_[self.label_offset_host, total].astype(np.int64)).to(dev),
                "hi": torch.from_numpy(np.where(self.item_windowed, self.start_hi_host, 0).astype(np.int32)).to(dev),
                "slot_item": torch.from_numpy(self.slot_item.astype(np.int32)).to(dev),
                "A": torch.empty((total + n) * nc, dtype=torch.int32, device=dev),
                "B": torch.empty((total + n) * nc, dtype=torch.int64, device=dev),
                "W": torch.empty(n, nc, dtype=torch.int64, device=dev),
                "present": torch.empty(n, dtype=torch.int32, device=dev),
                "ws": _lib.scratch(ws_bytes, dev),
                "out": torch.empty(2 * n_slots + 1, dtype=torch.int32, device=dev),       # start3 | chosen class | err
            }
        return self._crop

    def _window_activity(self, t):
        p = _lib.ptr
        t["out"][-1:].zero_()
        _lib.check(_lib.lib().sed_window_activity(p(self.label_pool), p(t["row0"]), t["total"], self.n_clips, self.nclass, p(t["hi"]),
                                                  self.T3, p(t["A"]), p(t["B"]), p(t["W"]), p(t["present"]), p(t["ws"]),
                                                  t["ws"].numel(), p(t["out"][-1:]), _lib.stream_ptr()), "sed_window_activity")

    @staticmethod
    def _crop_err(err):
        if err:
            raise _lib.SedError("event-aware crop sampling: " + "; ".join(s for b, s in CROP_ERR_BITS.items() if err & b)
                                + f" (err {err})")

    def _event_slots(self, epoch):
        """(start3, chosen class) of every window slot in epoch ``epoch``, int64 [n_slots] each: the host draws, the two
        entries on the set's device, one copy back."""
        t = self._crop_tables()
        n_slots = len(self.slot_item)
        self._event_launch(t, *self._event_upload(epoch))
        host = t["out"].cpu().numpy().astype(np.int64)
        self._crop_err(int(host[-1]))
        return host[:n_slots], host[n_slots:2 * n_slots]

    def _event_upload(self, epoch):
        """The draws of ``epoch`` on the set's device: (u as the int64 of the same bits, v int32, m uint8 - false on the slots
        of non-windowed items, whose ``hi`` of 0 then gives start 0 and class -1)."""
        u, v, m = self.event_draws(epoch)
        m = m & self.item_windowed[self.slot_item]
        return (torch.from_numpy(u.view(np.int64)).to(self.device), torch.from_numpy(v.astype(np.int32)).to(self.device),
                torch.from_numpy(m.astype(np.uint8)).to(self.device))

    def _event_launch(self, t, u_d, v_d, m_d):
        """The two entries on the current stream; nothing synchronises."""
        n_slots, p, out = len(self.slot_item), _lib.ptr, t["out"]
        self._window_activity(t)
        _lib.check(_lib.lib().sed_window_event_starts(
            p(u_d), p(v_d), p(m_d), p(t["slot_item"]), n_slots, p(t["hi"]), p(self.clip_frames), self.pooling_time_ratio,
            p(t["row0"]), t["total"], self.n_clips, self.nclass, self.T3, p(t["A"]), p(t["B"]), p(t["W"]), p(t["present"]),
            p(out[:n_slots]), p(out[n_slots:2 * n_slots]), p(out[-1:]), _lib.stream_ptr()), "sed_window_event_starts")

    def slot_classes(self, epoch):
        """The class every window slot of epoch ``epoch`` was drawn for under ``sampling="events"``, int64 [n_slots]; -1: a
        uniform draw (a diagnostic: it runs the draw again)."""
        if self.sampling != "events":
            raise ValueError('slot_classes is defined for sampling="events"')
        return self._event_slots(epoch)[1]

    def event_weights(self):
        """``(W, present)`` of the label pool as it is now: ``W`` [n_items, nclass] int64, the activity of class c that the
        windows of item i starting on ``[0, hi]`` cover, counted once per window (``hi`` = 0 for an item of a non-windowed
        stream); ``present`` [n_items] uint32, bit c set when ``W[i, c] > 0``."""
        t = self._crop_tables()
        self._window_activity(t)
        err = int(t["out"][-1].item())
        self._crop_err(err)
        return t["W"].cpu().numpy(), t["present"].cpu().numpy().view(np.uint32)

    def epoch_windows(self, epoch, rng=None):
        """One epoch of GLOBAL batches [n_steps, sum(batch_sizes), 2] int64 = (item, start3): the stream permutations of
        ``epoch_rows`` over the window slots (from ``rng``, default numpy's global generator), the starts of ``epoch``."""
        rng = np.random if rng is None else rng
        parts, lo = [], 0
        for size, b in zip(self.window_stream_sizes, self.batch_sizes):
            perm = np.asarray(rng.permutation(range(lo, lo + size)), dtype=np.int64)
            parts.append(perm[:(size // b) * b].reshape(-1, b)[:self.n_steps])
            lo += size
        slots = np.concatenate(parts, axis=1)
        return np.stack([self.slot_item[slots], self.slot_starts(epoch)[slots]], axis=-1)

    def epoch_rows(self, rng=None):
        raise ValueError("a WindowedFeatureSet's epochs are tables of windows: epoch_windows(epoch, rng)")

    def check_windows(self, win):
        """``win`` [..., 2] as int64, every row checked: 0 <= item < n_items and 0 <= start3 * pool < L_item."""
        w = np.asarray(win, dtype=np.int64)
        if w.ndim < 1 or w.shape[-1] != 2 or w.size == 0:
            raise _lib.SedError(f"a window table is [..., 2] = (item, start3), got shape {w.shape}")
        item, start = w[..., 0], w[..., 1]
        if item.min() < 0 or item.max() >= self.n_clips:
            raise _lib.SedError(f"window table holds an item outside [0, {self.n_clips})")
        if start.min() < 0 or (start * self.pooling_time_ratio >= self.clip_frames_host[item]).any():
            raise _lib.SedError("window table holds a start outside its item")
        return w

    def epoch_table(self, epoch, rng=None):
        """This rank's share of epoch ``epoch`` [n_steps, batch, 2] as int32, every row checked (``check_windows``)."""
        t = self.check_windows(self.local_rows(self.epoch_windows(epoch, rng)))
        return np.ascontiguousarray(t, dtype=np.int32)

    def draw_table(self, epoch, rng=None):
        return self.epoch_table(epoch, rng)

    # ---- the gather ----------------------------------------------------------------------------------------------------------
    def gather(self, win, out_clean, out_noisy=None, key=None, out_target=None, ws=None):
        """Windows ``win`` (device int32 [B, 2] = (item, start3), validated by the caller) -> out_clean [B, 1, frames, n_mels]
        (+ out_noisy with the teacher's noise of the device key ``key``, + out_target [B, T3, nclass]) on the current stream."""
        if not torch.is_tensor(win) or win.dim() != 2 or win.shape[1] != 2 or win.dtype != torch.int32 or not win.is_contiguous():
            raise _lib.SedError("WindowedFeatureSet.gather takes a contiguous int32 [B, 2] table of (item, start3) windows, not "
                                "clip indices: its items are not clips")
        if self.device.type != "cuda":
            raise _lib.SedError("WindowedFeatureSet.gather needs the set on a GPU device (no CPU fallback)")
        B = win.shape[0]
        l = _lib.lib()
        if ws is None:
            ws = torch.empty(l.sed_logmel_transform_ws_bytes(B), device=self.device, dtype=torch.uint8)
        lab = out_target is not None
        _lib.check(l.sed_gather_window_logmel_transform(
            _lib.ptr(self.pool), _lib.ptr(self.clip_offset), _lib.ptr(self.clip_frames), self.n_clips, self.max_win_frames,
            _lib.ptr(win), B, self.n_mels, self.frames, self.pooling_time_ratio, _lib.ptr(self.mean), _lib.ptr(self.std),
            _lib.ptr(key), _lib.ptr(out_clean), _lib.ptr(out_noisy), _lib.ptr(self.label_pool) if lab else None,
            _lib.ptr(self.label_offset) if lab else None, _lib.ptr(self.label_rows) if lab else None, self.T3, self.nclass,
            _lib.ptr(out_target), _lib.ptr(ws), ws.numel(), self.math_dtype, _lib.stream_ptr()),
            "sed_gather_window_logmel_transform")

    def _label_layout(self):
        """The label pool of ``relabel`` / ``check_relabel`` (resident.py): item i owns the rows ``label_offset[i] ..
        label_offset[i] + label_rows[i] - 1`` of ``label_pool``."""
        return self.label_pool, self.label_offset_host, self.label_rows_host.astype(np.int64), self.nclass, "label_rows"

    def transform(self, windows, seed=None):
        """Convenience (tests, tools): host windows [[item, start3], ...] -> (clean[, noisy], target) as new device tensors;
        ``seed`` is the Philox key of the teacher's noise (a set built with augment_type='noise' requires it)."""
        w = self.check_windows(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
        win = torch.from_numpy(w.astype(np.int32)).to(self.device)
        B = win.shape[0]
        clean = torch.empty(B, 1, self.frames, self.n_mels, device=self.device, dtype=torch.float32)
        noisy = key = None
        if self.noise:
            if seed is None:
                raise ValueError("a set with augment_type='noise' needs a seed")
            noisy = torch.empty_like(clean)
            key = torch.tensor([int(seed)], dtype=torch.int64, device=self.device)
        tgt = torch.empty((B,) + self.target_shape, device=self.device, dtype=torch.float32)
        self.gather(win, clean, noisy, key, tgt)
        return ((clean, noisy) if self.noise else (clean,)) + (tgt,)

    def eval_batch(self, i0, n):
        raise _lib.SedError("a WindowedFeatureSet is a training set of windows: eval_batch would address its items as clips "
                            "(infer long recordings with LongRecordingSet)")
