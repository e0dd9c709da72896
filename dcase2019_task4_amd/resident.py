"""Training and validation from linear-mel features resident in HBM.

The reference feeds precomputed features through ``DataLoadDf`` + ``get_transforms`` (one ``np.load``, one transform and
one host round trip per sample, a host collate and a host-to-device copy per step) behind a ``MultiStreamBatchSampler``
(DataLoad.py:539-577).  Here every clip's linear mel and encoded target are read ONCE (``ds.get_sample(i)``, so whatever
``encode_function`` the dataset holds applies) and uploaded into one pool; an epoch is a device-resident table of pool
indices, and each batch is gathered + transformed by one call of ``sed_gather_logmel_transform`` (csrc/feat.hip: the
arithmetic of ``sed_logmel_transform``, clips of any length, targets copied by the same launch).

* ``ResidentFeatureSet``: the pool + the epoch tables.  The tables follow ``MultiStreamBatchSampler`` exactly: per epoch one
  ``np.random.permutation(range(lo_i, hi_i))`` per stream, in stream order, from numpy's GLOBAL generator (the only draws the
  reference's main process makes with ``num_workers > 0``), ``grouper`` chunks of ``batch_sizes[i]`` (incomplete chunks
  dropped), zipped into concatenated sub-batches, ``min(len_i // bs_i)`` rows.  With a process group, rank r takes
  ``dist.shard_indices(row, batch_sizes, r, world)`` of every global row - each rank draws the rows itself, so every rank
  must seed numpy's global generator identically (``np.random.seed`` with the same value before the first epoch), as they
  must for the reference's sampler; the step then gets ``dist.local_masks`` (``step_masks``).
* ``ResidentFrontEnd``: the one-batch-ahead protocol of ``features.OneBatchAheadFrontEnd`` with the gather as extraction.
  Per step the host enqueues one 4 B x B device-to-device copy (the next row of the epoch table into the fixed index buffer
  the graph reads) and the replay; no feature or target crosses the host.  Tables are double-buffered: the one of epoch
  e + 1 is drawn and uploaded when epoch e's first batch is staged, so batch 0 of e + 1 can be gathered during the last
  step of e.
* ``augment=AugmentPolicy(...)`` on a training set (augment.py): mixup, circular time shift and time / frequency masks of
  the gathered batch.  The per-clip parameter rows of an epoch are drawn on the host from the policy's own generator and
  uploaded beside the index table; per step one more device-to-device row copy (32 B x B) stages the batch's rows, and the
  extraction becomes gather into staging buffers + one ``sed_batch_augment`` launch into the slot.  ``for_eval`` never
  augments.
* ``ResidentFeatureSet.for_eval``: the validation form (no noise) that ``inference.get_predictions`` gathers
  ``batch_size`` clips per launch from.
"""
import numpy as np
import torch

from . import _lib
from . import dist as sdist
from .augment import AugmentPolicy, augment_batch, validate_table      # noqa: F401  (the public names live here too)
from .features import OneBatchAheadFrontEnd

_UPLOAD_CHUNK = 1 << 26            # floats per host->device copy while building the pool (256 MB)


def local_step_masks(batch_sizes, world, weak_mask, strong_mask):
    """The (weak_mask, strong_mask) a rank's step needs, from the masks main.py builds for the GLOBAL batch (main.py:238-247:
    ``slice(B/4)`` and ``slice(3B/4, B)`` or None).  Global masks and the rank's own local masks (dist.local_masks) both map to
    the local masks, None keeps a loss term off, anything else raises ValueError: on a rank's share of the batch a global
    slice would mark unlabelled clips as weak and leave the strong range empty."""
    bs = [int(b) for b in batch_sizes]
    bg = sum(bs)
    bl = bg // int(world)
    glob = (slice(bs[0]), slice(bg - bs[-1], bg) if len(bs) == 3 else None)
    loc = sdist.local_masks(bs, world)
    out = []
    for name, m, g, l in zip(("weak", "strong"), (weak_mask, strong_mask), glob, loc):
        if m is None:
            out.append(None)
            continue
        if isinstance(m, slice) and ((g is not None and m.indices(bg) == g.indices(bg)) or
                                     (l is not None and m.indices(bl) == l.indices(bl))):
            out.append(l)
            continue
        raise ValueError(f"{name}_mask {m} is neither the global batch's {g} nor this rank's {l} (batch sizes {bs}, world {world})")
    return tuple(out)


class ResidentFeatureSet:
    """Linear-mel features and encoded targets of one or more datasets, resident on the GPU.

    ``ResidentFeatureSet([train_weak_data, unlabel_data, train_synth_data], batch_sizes, frames, scaler, augment_type="noise")``
    takes the reference's ``DataLoadDf`` objects (anything with ``__len__`` and ``get_sample(i) -> (features [L, n_mels],
    encoded target [T3, nclass])``) in stream order; ``from_arrays`` takes the clips directly."""

    def __init__(self, datasets, batch_sizes, frames, scaler=None, augment_type="noise", device="cuda", process_group=None,
                 math_dtype="f64", seed=0, augment=None):
        feats, tgts, sizes = [], [], []
        for ds in datasets:
            sizes.append(len(ds))
            for i in range(len(ds)):
                f, y = ds.get_sample(i)
                feats.append(f)
                tgts.append(y)
        self._setup(feats, tgts, sizes, batch_sizes, frames, scaler, augment_type, device, process_group, math_dtype, seed,
                    augment)

    @classmethod
    def from_arrays(cls, features, targets, stream_sizes=None, batch_sizes=None, frames=628, scaler=None, augment_type="noise",
                    device="cuda", process_group=None, math_dtype="f64", seed=0, augment=None):
        """``features``: sequence of float arrays [L_i, n_mels] (any L_i >= 1); ``targets``: sequence of [T3, nclass] arrays or
        None (no targets); ``stream_sizes``: clips per stream, in order (default: one stream); ``batch_sizes``: clips per stream
        and batch (None: a set for gather / evaluation only, no epoch tables); ``augment``: an ``AugmentPolicy`` (mixup, time
        shift, masks on the gathered batch: augment.py) or None - a training set's only, ``augment_type`` keeps its meaning."""
        self = cls.__new__(cls)
        self._setup(list(features), None if targets is None else list(targets),
                    [len(features)] if stream_sizes is None else list(stream_sizes), batch_sizes, frames, scaler, augment_type,
                    device, process_group, math_dtype, seed, augment)
        return self

    @classmethod
    def for_eval(cls, dataset, frames, scaler=None, device="cuda", math_dtype="f64"):
        """The validation form of ``dataset`` (get_transforms(frames, scaler): no noise) for inference.get_predictions; keeps
        ``dataset.filenames``."""
        feats = [dataset.get_sample(i)[0] for i in range(len(dataset))]
        self = cls.from_arrays(feats, None, None, None, frames, scaler, None, device, None, math_dtype)
        self.filenames = dataset.filenames
        return self

    # ---- construction --------------------------------------------------------------------------------------------------------
    def _setup(self, feats, tgts, sizes, batch_sizes, frames, scaler, augment_type, device, process_group, math_dtype, seed,
               augment=None):
        if augment_type not in (None, "noise"):
            raise NotImplementedError("only augment_type='noise' exists (utils.py:404-406)")
        if augment is not None and not isinstance(augment, AugmentPolicy):
            raise TypeError(f"augment must be an AugmentPolicy or None, got {type(augment).__name__}")
        if augment is not None and batch_sizes is None:
            raise ValueError("only a training set (built with batch sizes) takes an augmentation policy")
        self.augment = augment
        # (a set on a CPU device holds the pool, the targets and the tables - what can be checked without a GPU - and refuses
        # to gather: there is no CPU path)
        self.device = torch.device(device)
        self.math_dtype = _lib.FFT_DTYPES[math_dtype]
        self.noise = augment_type == "noise"
        self.frames = int(frames)
        self.seed = int(seed)
        if self.frames < 1:
            raise ValueError(f"frames must be >= 1, got {frames}")
        if not feats:
            raise ValueError("no clips")
        sizes = [int(s) for s in sizes]
        if any(s < 0 for s in sizes) or sum(sizes) != len(feats):
            raise ValueError(f"stream sizes {sizes} do not add up to the {len(feats)} clips")
        feats = [np.asarray(f, dtype=np.float32) for f in feats]
        n_mels = feats[0].shape[-1] if feats[0].ndim == 2 else -1
        for i, f in enumerate(feats):
            if f.ndim != 2 or f.shape[1] != n_mels or f.shape[0] < 1:
                raise ValueError(f"clip {i}: features of shape {f.shape}, expected [frames >= 1, {n_mels}]")
        self.n_mels = int(n_mels)
        self.n_clips = len(feats)
        self.stream_sizes = sizes
        lengths = np.array([f.shape[0] for f in feats], dtype=np.int64)
        if lengths.max() * self.n_mels >= 2 ** 31:
            raise ValueError(f"a clip of {lengths.max()} frames is too long")
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        self.clip_frames_host, self.clip_offset_host = lengths.astype(np.int32), offsets
        self.max_clip_frames = int(lengths.max())
        # the pool: clips concatenated along frames, uploaded in chunks of whole clips
        total = int(lengths.sum()) * self.n_mels
        self.pool = torch.empty(total, device=self.device, dtype=torch.float32)
        i0 = 0
        while i0 < len(feats):
            i1, n = i0, 0
            while i1 < len(feats) and (n == 0 or n + feats[i1].size <= _UPLOAD_CHUNK):
                n += feats[i1].size
                i1 += 1
            lo = int(offsets[i0]) * self.n_mels
            self.pool[lo:lo + n].copy_(torch.from_numpy(np.concatenate([f.reshape(-1) for f in feats[i0:i1]])))
            i0 = i1
        self.clip_offset = torch.from_numpy(offsets).to(self.device)
        self.clip_frames = torch.from_numpy(self.clip_frames_host).to(self.device)
        self.targets = None
        self.target_shape = None
        if tgts is not None:
            if len(tgts) != len(feats):
                raise ValueError(f"{len(tgts)} targets for {len(feats)} clips")
            tgts = [np.asarray(t, dtype=np.float32) for t in tgts]
            shp = tgts[0].shape
            for i, t in enumerate(tgts):
                if t.shape != shp or t.ndim != 2:
                    raise ValueError(f"clip {i}: target of shape {t.shape}, expected {shp} ([T3, nclass])")
            self.target_shape = tuple(int(v) for v in shp)
            self.targets = torch.from_numpy(np.stack(tgts)).to(self.device)
        self.mean = self.std = None
        if scaler is not None:
            self.mean = torch.tensor(np.asarray(scaler.mean_), dtype=torch.float64, device=self.device)
            self.std = torch.tensor(np.asarray(scaler.std_), dtype=torch.float64, device=self.device)
            if self.mean.numel() != self.n_mels or self.std.numel() != self.n_mels:
                raise ValueError(f"scaler has {self.mean.numel()} bands, the features {self.n_mels}")
        self.filenames = None
        self._all = None
        # the batch layout
        self.process_group = process_group
        self.world, self.rank = 1, 0
        if process_group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        self._set_batches(sizes, batch_sizes)

    def _set_batches(self, sizes, batch_sizes):
        """The batch layout of a training set whose streams hold ``sizes`` entries (clips here; a subclass may count
        something else); ``batch_sizes`` None: a set for gather / evaluation only."""
        self.batch_sizes = None
        self.n_steps = None
        if batch_sizes is not None:
            bs = [int(b) for b in batch_sizes]
            if len(bs) != len(sizes):
                raise ValueError(f"batch_sizes must be the same length as the number of datasets {len(bs)} != {len(sizes)}")
            if any(b < 1 for b in bs):
                raise ValueError(f"batch sizes must be >= 1: {bs}")
            sdist.local_batch_sizes(bs, self.world)                    # every stream divisible by the world size
            self.batch_sizes = bs
            self.n_steps = min(s // b for s, b in zip(sizes, bs))
            if self.n_steps < 1:
                raise ValueError(f"a stream has fewer clips than its batch size: {sizes} / {bs}")
            if self.target_shape is None:
                raise ValueError("a training set needs targets")
            self.batch = sum(bs) // self.world
            self.weak_mask, self.strong_mask = sdist.local_masks(bs, self.world)
            ends = np.cumsum(sdist.local_batch_sizes(bs, self.world))
            self.stream_slices = [slice(int(lo), int(hi)) for lo, hi in zip(np.r_[0, ends[:-1]], ends)]

    def step_masks(self, weak_mask, strong_mask):
        """The masks for this rank's step (local_step_masks); without a process group the caller's masks are used as given."""
        if self.process_group is None:
            return weak_mask, strong_mask
        return local_step_masks(self.batch_sizes, self.world, weak_mask, strong_mask)

    def __len__(self):
        """Steps per epoch (a training set), or clips (a set built without batch sizes)."""
        return self.n_steps if self.n_steps is not None else self.n_clips

    # ---- epoch tables --------------------------------------------------------------------------------------------------------
    def epoch_rows(self, rng=None):
        """One epoch of GLOBAL batches [n_steps, sum(batch_sizes)] - what MultiStreamBatchSampler yields (DataLoad.py:562-571),
        drawing from ``rng`` (default: numpy's global generator, as the sampler does)."""
        if self.batch_sizes is None:
            raise ValueError("this set was built without batch sizes")
        rng = np.random if rng is None else rng
        parts, lo = [], 0
        for size, b in zip(self.stream_sizes, self.batch_sizes):
            perm = np.asarray(rng.permutation(range(lo, lo + size)), dtype=np.int64)
            parts.append(perm[:(size // b) * b].reshape(-1, b)[:self.n_steps])
            lo += size
        return np.concatenate(parts, axis=1)

    def local_rows(self, rows, rank=None, world=None):
        """Rank ``rank``'s share of global rows (default: this set's rank / world): dist.shard_indices of every row."""
        rank = self.rank if rank is None else int(rank)
        world = self.world if world is None else int(world)
        cols = np.asarray(sdist.shard_indices(list(range(sum(self.batch_sizes))), self.batch_sizes, rank, world), dtype=np.int64)
        return np.asarray(rows)[:, cols]

    def epoch_table(self, rng=None):
        """This rank's share of one epoch [n_steps, batch] as int32, every entry checked against [0, n_clips)."""
        t = self.local_rows(self.epoch_rows(rng))
        if t.size and (t.min() < 0 or t.max() >= self.n_clips):
            raise _lib.SedError(f"epoch table holds an index outside [0, {self.n_clips})")
        return np.ascontiguousarray(t, dtype=np.int32)

    row_shape = ()               # what one batch position of a table row holds: a clip index

    def draw_table(self, epoch, rng=None):
        """What ResidentFrontEnd uploads for the ``epoch``-th epoch it draws, [n_steps, batch, *row_shape] int32.  Clip
        tables do not depend on the epoch number."""
        return self.epoch_table(rng)

    def augment_table(self, epoch):
        """This rank's augmentation rows of epoch ``epoch`` (0-based count of drawn epochs) [n_steps, batch, 8] int32, from
        the policy's own generator - pure host code; a set without a policy raises."""
        if self.augment is None:
            raise ValueError("this set was built without an augmentation policy")
        return self.augment.draw(epoch, self.n_steps, self.stream_slices, self.frames, self.target_shape[0], self.n_mels,
                                 rank=self.rank)

    # ---- the gather ----------------------------------------------------------------------------------------------------------
    def gather(self, idx, out_clean, out_noisy=None, key=None, out_target=None, ws=None):
        """Clips ``idx`` (device int32 [B], entries in [0, n_clips)) -> out_clean [B, 1, frames, n_mels] (+ out_noisy with the
        teacher's noise drawn with the device key ``key``, + out_target [B, T3, nclass]) on the current stream."""
        if self.device.type != "cuda":
            raise _lib.SedError("ResidentFeatureSet.gather needs the set on a GPU device (no CPU fallback)")
        B = idx.numel()
        if ws is None:
            ws = torch.empty(_lib.lib().sed_logmel_transform_ws_bytes(B), device=self.device, dtype=torch.uint8)
        if out_target is not None and self.targets is None:
            raise ValueError("this set holds no targets")
        tgt_elems = int(np.prod(self.target_shape)) if self.targets is not None else 0
        l = _lib.lib()
        _lib.check(l.sed_gather_logmel_transform(
            _lib.ptr(self.pool), _lib.ptr(self.clip_offset), _lib.ptr(self.clip_frames), self.n_clips, self.max_clip_frames,
            _lib.ptr(idx), B, self.n_mels, self.frames, _lib.ptr(self.mean), _lib.ptr(self.std), _lib.ptr(key),
            _lib.ptr(out_clean), _lib.ptr(out_noisy), _lib.ptr(self.targets) if out_target is not None else None, tgt_elems,
            _lib.ptr(out_target), _lib.ptr(ws), ws.numel(), self.math_dtype, _lib.stream_ptr()), "sed_gather_logmel_transform")

    # ---- labels rewritten in place --------------------------------------------------------------------------------------------
    def _label_layout(self):
        """Where this set's labels live: ``(pool, row0, rows, nclass, what)`` - the contiguous float32 tensor of label rows,
        per item the first row and the number of rows (host int64), and a word for an item's length in the messages."""
        if self.targets is None:
            raise ValueError("this set holds no targets: there is nothing to relabel")
        T3, nclass = self.target_shape
        n = np.arange(self.n_clips, dtype=np.int64)
        return self.targets, n * T3, np.full(self.n_clips, T3, dtype=np.int64), nclass, "T3"

    def check_relabel(self, items, rec_frame0_host, nclass=None):
        """The host checks of ``relabel``, before any launch (``ValueError``): ``items`` distinct and inside the set, every
        recording exactly as long as its item's labels, the classes equal.  Returns ``(items, the first pool row of each)``."""
        pool, row0, rows, n_cls, what = self._label_layout()
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        f0 = np.asarray(rec_frame0_host, dtype=np.int64).reshape(-1)
        if items.size < 1 or f0.size != items.size + 1:
            raise ValueError(f"relabel: {items.size} items for a table of {f0.size - 1} recordings")
        if items.min() < 0 or items.max() >= self.n_clips:
            raise ValueError(f"relabel: items must lie in [0, {self.n_clips})")
        if np.unique(items).size != items.size:
            raise ValueError("relabel: an item is named twice (two recordings would write the same label rows)")
        if nclass is not None and int(nclass) != n_cls:
            raise ValueError(f"relabel: the table has {int(nclass)} classes, the set's labels {n_cls}")
        L3 = np.diff(f0)
        for r in np.flatnonzero(L3 != rows[items]):
            raise ValueError(f"relabel: recording {r} has {int(L3[r])} label frames, item {int(items[r])} has {what} = "
                             f"{int(rows[items[r]])}")
        return items, row0[items]

    def relabel(self, items, out_or_table, rec_frame0_host, nclass=None, values=None, point=None, combine="replace", err=None):
        """Rewrite the strong labels of the items ``items`` IN PLACE from a decoded event table on the device
        (``inference.events_rasterize``, ``sed_events_rasterize``): recording r of the table becomes the labels of item
        ``items[r]``.  ``out_or_table``: the dict of a stitch entry / ``get_long_predictions(return_table=True)`` or a pair
        ``(ev_ptr, ev_pairs)``; ``rec_frame0_host`` [n_rec + 1]: the recordings' label-frame offsets on the host (a
        ``LongRecordingSet`` has them); ``values`` / ``point`` / ``combine`` / ``err`` as for ``events_rasterize`` (soft labels,
        per-class operating points, ``"replace"`` or ``"max"``).  Checked on the host before any launch (``ValueError``):
        ``items`` in range and distinct, every recording's length equal to its item's label rows, ``nclass`` (given, or the
        columns of the dict's timeline) equal to the set's; a set without targets raises.  The label tensor keeps its
        ``data_ptr()``: a captured step graph and the one-batch-ahead front-end read the new labels at their next gather - a
        batch the front-end has ALREADY gathered when ``relabel`` is called still carries the old labels, so relabelling
        during an epoch takes effect one batch later (between epochs, or before ``train.train``, nothing is in flight).  The
        other items keep their labels bit for bit.  Returns the device error word ``err`` [1] int32 (non-zero: the items'
        labels are invalid); nothing synchronises."""
        from . import inference
        if nclass is None and isinstance(out_or_table, dict) and out_or_table.get("timeline") is not None:
            nclass = out_or_table["timeline"].shape[-1]
        items, row0 = self.check_relabel(items, rec_frame0_host, nclass)
        pool, _, _, n_cls, _ = self._label_layout()
        f0 = np.ascontiguousarray(rec_frame0_host, dtype=np.int64).reshape(-1)
        ev_pairs = out_or_table["ev_pairs"] if isinstance(out_or_table, dict) else out_or_table[1]
        rec_frame0 = torch.from_numpy(f0).to(ev_pairs.device)
        _, err = inference.events_rasterize(out_or_table, rec_frame0, items.size, n_cls, dst=pool, dst_row0=row0, values=values,
                                            point=point, combine=combine, err=err, rec_frame0_host=f0)
        return err

    def transform(self, indices, seed=None):
        """Convenience (tests, tools): host indices -> (clean[, noisy], target or None) as new device tensors; ``seed`` is the
        Philox key of the teacher's noise (a set built with augment_type='noise' requires it)."""
        ind = np.asarray(indices, dtype=np.int64).reshape(-1)
        if ind.size == 0 or ind.min() < 0 or ind.max() >= self.n_clips:
            raise _lib.SedError(f"indices must be in [0, {self.n_clips})")
        idx = torch.from_numpy(ind.astype(np.int32)).to(self.device)
        B = idx.numel()
        clean = torch.empty(B, 1, self.frames, self.n_mels, device=self.device, dtype=torch.float32)
        noisy = key = None
        if self.noise:
            if seed is None:
                raise ValueError("a set with augment_type='noise' needs a seed")
            noisy = torch.empty_like(clean)
            key = torch.tensor([int(seed)], dtype=torch.int64, device=self.device)
        tgt = (torch.empty((B,) + self.target_shape, device=self.device, dtype=torch.float32)
               if self.targets is not None else None)
        self.gather(idx, clean, noisy, key, tgt)
        return ((clean, noisy) if self.noise else (clean,)) + (tgt,)

    def eval_batch(self, i0, n):
        """Clips i0 .. i0 + n - 1 in the validation form (no noise) -> device [n, 1, frames, n_mels]; no host copy."""
        if self._all is None:
            self._all = torch.arange(self.n_clips, device=self.device, dtype=torch.int32)
        if i0 < 0 or n < 1 or i0 + n > self.n_clips:
            raise _lib.SedError(f"clips {i0} .. {i0 + n - 1} outside [0, {self.n_clips})")
        out = torch.empty(n, 1, self.frames, self.n_mels, device=self.device, dtype=torch.float32)
        self.gather(self._all[i0:i0 + n], out)
        return out


class ResidentFrontEnd(OneBatchAheadFrontEnd):
    """MeanTeacherStep fed from a ResidentFeatureSet, one batch ahead (features.OneBatchAheadFrontEnd's protocol; the
    extraction is one sed_gather_logmel_transform launch - clean + noisy inputs and targets of the staged batch).

    ``run()`` trains on the next batch of the epoch sequence and gathers the one after it; the sequence runs on across epochs
    (epoch e's table is drawn when its predecessor's first batch is staged).  ``aug_epoch``: the epoch index the set's
    augmentation policy - and a WindowedFeatureSet's crop generator - is asked for when this front-end draws its first table
    (0; a resumed run passes its epoch)."""

    def __init__(self, step, rset, overlap=True, seed=None, rng=None, aug_epoch=0):
        if rset.batch_sizes is None:
            raise ValueError("ResidentFrontEnd needs a set built with batch sizes")
        if step.B != rset.batch or step.T != rset.frames or step.target.shape[1:] != rset.target_shape:
            raise ValueError(f"step of batch {step.B} x {step.T} frames x target {tuple(step.target.shape[1:])} against a set of "
                             f"{rset.batch} x {rset.frames} x {rset.target_shape}")
        if rset.n_mels != step.x.shape[-1]:
            raise ValueError(f"the set has {rset.n_mels} mel bands, the model {step.x.shape[-1]}")
        if step.teacher is not None and not rset.noise:
            raise ValueError("a mean-teacher step needs the teacher's noisy copy: build the set with augment_type='noise'")
        super().__init__(step, overlap=overlap, seed=rset.seed if seed is None else seed, fe_workgroups=0)
        self.rs = rset
        self.rng = np.random if rng is None else rng
        dev = step.device
        # the batch the next extraction gathers: one table row, [B] clip indices (a WindowedFeatureSet: [B, 2] windows)
        self.idx = torch.zeros((step.B,) + rset.row_shape, device=dev, dtype=torch.int32)
        self.ws_t = torch.empty(self.l.sed_logmel_transform_ws_bytes(step.B), device=dev, dtype=torch.uint8)
        self._tables = [torch.empty((rset.n_steps, step.B) + rset.row_shape, device=dev, dtype=torch.int32) for _ in range(2)]
        self._drawn = 0                                # epochs whose table has been drawn
        self._epoch, self._pos = 0, 0                  # the batch the next _stage() puts into self.idx
        self.host_tables = {}                          # epoch -> the host table (kept for the two live epochs)
        # With a policy on the set: per-epoch parameter tables beside the index tables, the staged batch's rows in a fixed
        # buffer, and staging tensors - extract = gather into staging, then sed_batch_augment into the slot.  Without one,
        # none of these exist and the captured graph is the plain one - also with a policy that has everything off.
        # The policy is asked for epoch aug_epoch + k when the front-end's k-th table is drawn: a front-end built in a resumed
        # run passes the epoch it resumes at (train.train does), or it would redraw epoch 0's rows.
        self.aug = rset.augment is not None and rset.augment.active
        self.aug_epoch = int(aug_epoch)
        if self.aug:
            self.aug_row = torch.zeros(step.B, 8, device=dev, dtype=torch.int32)
            self._aug_tables = [torch.empty(rset.n_steps, step.B, 8, device=dev, dtype=torch.int32) for _ in range(2)]
            self.host_aug_tables = {}
            self._stage_x = torch.empty_like(step.x)
            self._stage_x_ema = torch.empty_like(step.x) if rset.noise else None
            self._stage_target = torch.empty_like(step.target)

    def _draw(self, e):
        while self._drawn <= e:
            t = self.rs.draw_table(self.aug_epoch + self._drawn, self.rng)
            self.host_tables[self._drawn] = t
            self.host_tables.pop(self._drawn - 2, None)
            # stream order: every row copy of the epoch that used this buffer before was enqueued earlier on this stream
            self._tables[self._drawn % 2].copy_(torch.from_numpy(t).pin_memory(), non_blocking=True)
            if self.aug:
                a = validate_table(self.rs.augment_table(self.aug_epoch + self._drawn), self.step.B)
                self.host_aug_tables[self._drawn] = a
                self.host_aug_tables.pop(self._drawn - 2, None)
                self._aug_tables[self._drawn % 2].copy_(torch.from_numpy(a).pin_memory(), non_blocking=True)
            self._drawn += 1

    def _stage(self):
        """The next batch of the sequence into the index buffer: one device-to-device row copy, no sync."""
        e, i = self._epoch, self._pos
        if i == 0:
            self._draw(e + 1)
        self.idx.copy_(self._tables[e % 2][i], non_blocking=True)
        if self.aug:
            self.aug_row.copy_(self._aug_tables[e % 2][i], non_blocking=True)
        self._pos += 1
        if self._pos == self.rs.n_steps:
            self._epoch, self._pos = e + 1, 0

    def extract(self, x, x_ema, target, workgroups):
        if not self.aug:
            self.rs.gather(self.idx, x, x_ema if self.rs.noise else None, self.key, target, self.ws_t)
            return
        noisy = x_ema is not None and self.rs.noise
        sx, se, sg = self._stage_x, self._stage_x_ema if noisy else None, self._stage_target if target is not None else None
        self.rs.gather(self.idx, sx, se, self.key, sg, self.ws_t)
        st = self.step
        _lib.check(self.l.sed_batch_augment(_lib.ptr(sx), _lib.ptr(se), _lib.ptr(sg), _lib.ptr(self.aug_row), st.B, st.T,
                                            self.rs.n_mels, self.rs.target_shape[0], self.rs.target_shape[1], _lib.ptr(x),
                                            _lib.ptr(x_ema) if noisy else None, _lib.ptr(target), _lib.stream_ptr()),
                   "sed_batch_augment")

    def prime(self):
        self._stage()
        super().prime()

    def run(self):
        """One train step on the batch gathered last + the gather of the next batch of the sequence."""
        if not self._primed:
            self.prime()
        self._stage()
        super().run()
