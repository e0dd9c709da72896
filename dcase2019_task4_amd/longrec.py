"""Recordings longer than one clip: the window plan and the HBM-resident set of overlapping windows.

The BiGRU was trained on ``frames``-long clips, so a long recording is cut into overlapping windows of ``frames`` feature
frames, ``hop_frames`` apart; every window goes through the eval forward as a clip of its own, and
``inference.get_long_predictions`` blends the windows' posteriors into one timeline per recording and decodes that
(``sed_stitch_decode``, csrc/stitch.hip).  The windows cost no new extraction code: ``sed_gather_logmel_transform`` gathers
clips from a pool by arbitrary offset and length, so overlapping windows are overlapping clips of a ``ResidentFeatureSet``
whose clip tables point into the recordings.  The dB clamp is per window, as for a clip of its own: a window's input is
byte for byte what the same frames give as a clip, whatever else the recording holds.
"""
import numpy as np
import torch

from . import _lib
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


def sweep_chunks(K, capacity_per_point, max_table_bytes, limit=2 ** 31 - 1024):
    """The ranges ``[(k0, k1), ...]`` that split ``K`` operating points into ``sed_stitch_sweep`` calls: consecutive, covering
    ``0 .. K`` once, each as long as possible with its event table ``(k1 - k0) * capacity_per_point`` rows of 8 bytes
    (``ev_pairs``) within ``max_table_bytes`` and its capacity below ``limit`` (what the scorers accept); never fewer than one
    point per chunk, never more than ``MAX_SWEEP_POINTS``."""
    K, cap = int(K), int(capacity_per_point)
    if K < 1 or cap < 0:
        raise ValueError(f"need K >= 1 and capacity_per_point >= 0, got {K}, {cap}")
    per = K if cap == 0 else min(int(max_table_bytes) // (8 * cap), (int(limit) - 1) // cap)
    per = max(1, min(per, K, MAX_SWEEP_POINTS))
    return [(k0, min(k0 + per, K)) for k0 in range(0, K, per)]


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
        if filenames is None:
            filenames = [f"recording_{i}" for i in range(self.n_rec)]
        if len(filenames) != self.n_rec:
            raise ValueError(f"{len(filenames)} filenames for {self.n_rec} recordings")
        self.filenames = list(filenames)

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
