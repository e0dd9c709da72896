"""Batched on-GPU inference + post-processing: the reference's ``get_predictions``
(baseline/evaluation_measures.py:203-231) with the same signature and the same DataFrame / TSV output.

The reference runs ONE clip per forward and post-processes it on the host (threshold, scipy median filter,
run-length decode) - 1 168 + ~400 forwards per epoch.  Here clips go through the eval-mode CRNN ``batch_size`` at a
time and ``sed_postprocess`` thresholds, median-filters and run-length-decodes the whole batch on the device; the host
only assembles the event table.  There is no CPU fallback: the model and its inputs live on the GPU.

Recordings longer than one clip: ``LongRecordingSet`` (longrec.py) holds them as overlapping windows and
``get_long_predictions`` blends the windows' posteriors and decodes each recording's whole timeline with one
``sed_stitch_decode`` call.  The device-resident event table it leaves is scored by ``metrics.long_event_counts`` /
``long_psds_counts`` / ``validate_long`` (``sed_long_event_counts``, ``sed_long_psds_counts``: columns of any length).
``stitch_sweep`` decodes K operating points from one blend (``sed_stitch_sweep``), scored by ``metrics.long_sweep_*``.
Training on windows of such recordings is ``WindowedFeatureSet`` (longrec.py, through ``train.train``).  Recording-level
weak tags: ``get_long_predictions(return_weak=True)`` / ``stitch_weak`` pool them over the whole blended timeline from the
windows' posteriors and attention (``CRNN.last_attention``, ``sed_stitch_weak``); ``weak_tags_dataframe`` is their table,
``metrics.validate_long(weak_labels=...)`` their score; ``pooled_tags`` is the same tag with a backward
(``sed_stitch_weak_backward``), what ``train.train_recording_tags`` trains on.  Two-threshold (hysteresis) decode:
``stitch_hysteresis`` / ``get_long_predictions(threshold_high=...)`` keep the low-threshold events in which a high-threshold
event starts (one ``stitch_sweep`` of both thresholds, then ``sed_events_hysteresis``).  Minimum event length and gap
merging: ``events_process`` / ``get_long_predictions(min_event_length=..., min_event_gap=...)`` drop short events and fuse
events across short gaps on any of these tables (``sed_events_process``; ``process_points`` turns seconds into frames).
Confidence scores: ``events_scores`` / ``get_long_predictions(event_scores=True)`` give every event of such a table the maximum
and the mean of the blended timeline over its frames (``sed_events_scores``), ``events_select`` /
``get_long_predictions(min_event_score=...)`` keep the events whose score exceeds a minimum (``sed_events_select``).
Span-level weak tags and the tag gate: ``stitch_span_tags`` / ``get_long_predictions(tag_span=...)`` pool the weak tag per span
of time (``sed_stitch_span_tags``, ``span_table``, ``span_tags_dataframe``), ``events_tag_scores`` gives every event the largest
tag of the spans it touches (``sed_events_tag_scores``) and ``gate_decoded`` / ``get_long_predictions(min_span_tag=...)`` keep
the events that touch a confident span (``events_select`` on that score); ``pooled_span_tags`` is the span tag with a backward.
Both take ``span_off``: the tables then describe PIECES of recordings - consecutive spans with exactly the windows that cover them
(``longrec.span_pieces``; ``sed_stitch_piece_span_tags`` and its backward) - which is how ``train.train_span_tags(split_long=True)``
trains on a recording with more windows than one forward holds.
Both levels of pooled tags share one forward call, one backward call and one autograd node, in which a row description
(``_tags_forward``) selects the level and with it the C entry.
Pseudo strong labels: ``events_rasterize`` / ``rasterize_decoded`` turn any of these tables back into label rows
(``sed_events_rasterize``), ``WindowedFeatureSet.relabel`` / ``ResidentFeatureSet.relabel`` write them in place into a training
set's label pool, and ``pseudo_label`` runs the whole chain of ``get_long_predictions`` and ends in the pool instead of a
DataFrame.
``get_predictions`` itself is unchanged.
"""
import ctypes as C

import numpy as np
import pandas as pd
import torch

from . import _lib
from .longrec import (WEIGHTINGS, LongRecordingSet, WindowedFeatureSet, check_hop_frames, default_hop_frames,      # noqa: F401
                      encode_timeline, sweep_chunks, window_plan)


class _Cfg:
    """The three config.py values get_predictions reads (config.py:17,19,39)."""
    sample_rate = 44100
    hop_length = 511
    median_window = 5


def postprocess(strong, threshold=0.5, median_window=5, want_binary=False):
    """strong [N, T, nclass] cuda float32 -> (ev_count [N, nclass] int32, ev_pairs [N, nclass, max_ev, 2] int32[, binary])."""
    if strong.device.type != "cuda":
        raise _lib.SedError("postprocess needs a GPU tensor (no CPU fallback)")
    strong = strong.contiguous().float()
    N, T, NC = strong.shape
    max_ev = (T + 1) // 2
    cnt = torch.empty(N, NC, dtype=torch.int32, device=strong.device)
    pairs = torch.zeros(N, NC, max_ev, 2, dtype=torch.int32, device=strong.device)
    binary = torch.empty(N, T, NC, dtype=torch.uint8, device=strong.device) if want_binary else None
    _lib.check(_lib.lib().sed_postprocess(_lib.ptr(strong), N, T, NC, float(threshold), int(median_window),
                                          _lib.ptr(binary) if want_binary else None, _lib.ptr(cnt), _lib.ptr(pairs), max_ev,
                                          _lib.stream_ptr()), "sed_postprocess")
    return (cnt, pairs, binary) if want_binary else (cnt, pairs)


def eval_batches(valid_dataset, batch_size, dev):
    """The clips of ``valid_dataset`` (a ``DataLoadDf``-like or a ``ResidentFeatureSet.for_eval``) ``batch_size`` at a time:
    yields ``(i0, range(i0, i0 + n), x [n, 1, T, F] float32 on dev)``."""
    from .resident import ResidentFeatureSet
    resident = isinstance(valid_dataset, ResidentFeatureSet)
    stage, copied = None, None
    n = len(valid_dataset)
    for i0 in range(0, n, batch_size):
        idx = range(i0, min(n, i0 + batch_size))
        if resident:
            x = valid_dataset.eval_batch(i0, len(idx))
        else:
            items = [torch.as_tensor(valid_dataset[i][0]) for i in idx]
            if stage is None or stage.shape[1:] != items[0].shape or stage.dtype != items[0].dtype:
                # one reusable pinned staging buffer: a fresh pageable torch.stack per batch cost more than the forward
                stage = torch.empty((batch_size,) + tuple(items[0].shape), dtype=items[0].dtype).pin_memory()
            if copied is not None:
                copied.synchronize()      # a caller that never synchronises (metrics.validate) must not overtake the last upload
            for k, it in enumerate(items):
                stage[k].copy_(it)
            x = stage[:len(items)].to(dev, non_blocking=True).float()
            copied = torch.cuda.Event()
            copied.record()
        yield i0, idx, x


def get_predictions(model, valid_dataset, decoder, pooling_time_ratio=1, save_predictions=None, batch_size=64, cfg=None,
                    threshold=0.5):
    """Drop-in for evaluation_measures.get_predictions.

    ``valid_dataset[i]`` yields ``(input [1, T, F], label)`` and has ``.filenames`` (DataLoadDf, DataLoad.py:47-72);
    ``decoder`` is ``many_hot_encoder.decode_strong`` (main.py:326): when it is a bound method of an object with
    ``.labels`` the run-length decode happens on the device, otherwise the callable gets the device-filtered 0/1 matrix
    of each clip, exactly as in the reference.  ``cfg`` supplies sample_rate / hop_length / median_window
    (default: the values of baseline/config.py).

    ``valid_dataset`` may also be a ``resident.ResidentFeatureSet.for_eval(...)``: its clips are then gathered and
    transformed ``batch_size`` per launch straight into the forward's input, with no host copy."""
    from .resident import ResidentFeatureSet
    resident = isinstance(valid_dataset, ResidentFeatureSet)
    if resident and valid_dataset.noise:
        raise ValueError("get_predictions needs a validation set without noise (ResidentFeatureSet.for_eval)")
    cfg = cfg or _Cfg
    labels = getattr(getattr(decoder, "__self__", None), "labels", None)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.SedError("get_predictions needs the model on the GPU (no CPU fallback)")
    was_training = model.training
    model.eval()
    frames, cols = [], []
    filenames = valid_dataset.filenames
    try:
        with torch.no_grad():
            for i0, idx, x in eval_batches(valid_dataset, batch_size, dev):
                strong, _ = model(x)
                if labels is not None:
                    cnt, pairs = postprocess(strong, threshold, cfg.median_window)
                    # compact on the device: rows ordered (clip, class, event) = the order of the reference's nested loops
                    keep = torch.arange(pairs.shape[2], device=dev)[None, None, :] < cnt[:, :, None]
                    k_idx, c_idx, _ = torch.nonzero(keep, as_tuple=True)
                    ev = pairs[keep]                                        # [n_events, 2]
                    cols.append((k_idx.cpu().numpy() + i0, c_idx.cpu().numpy(), ev.cpu().numpy()))
                else:
                    _, _, binary = postprocess(strong, threshold, cfg.median_window, want_binary=True)
                    binary = binary.cpu().numpy().astype(int)
                    for k, i in enumerate(idx):
                        pred = pd.DataFrame(decoder(binary[k]), columns=["event_label", "onset", "offset"])
                        pred["filename"] = filenames.iloc[i]
                        frames.append(pred)
    finally:
        model.train(was_training)
    if labels is not None:
        # ONE DataFrame for the whole set, equal to the reference's concatenation of per-clip frames (including its
        # per-clip 0..k-1 index); building 1 168 small DataFrames on the host cost more than all the device work
        clip = np.concatenate([c[0] for c in cols]) if cols else np.zeros(0, dtype=np.int64)
        cls = np.concatenate([c[1] for c in cols]) if cols else np.zeros(0, dtype=np.int64)
        ev = np.concatenate([c[2] for c in cols]) if cols else np.zeros((0, 2), dtype=np.int32)
        starts = np.r_[0, np.flatnonzero(np.diff(clip)) + 1] if len(clip) else np.zeros(0, dtype=np.int64)
        index = np.arange(len(clip)) - np.repeat(starts, np.diff(np.r_[starts, len(clip)])) if len(clip) else clip
        prediction_df = pd.DataFrame({"event_label": np.asarray(labels, dtype=object)[cls],
                                      "onset": ev[:, 0].astype(np.int64), "offset": ev[:, 1].astype(np.int64),
                                      "filename": np.asarray(filenames)[clip]}, index=index,
                                     columns=["event_label", "onset", "offset", "filename"])
    else:
        prediction_df = pd.concat(frames) if frames else pd.DataFrame(columns=["event_label", "onset", "offset", "filename"])
    # In seconds (evaluation_measures.py:225-227)
    prediction_df.onset = prediction_df.onset * pooling_time_ratio / (cfg.sample_rate / cfg.hop_length)
    prediction_df.offset = prediction_df.offset * pooling_time_ratio / (cfg.sample_rate / cfg.hop_length)
    if save_predictions is not None:
        prediction_df.to_csv(save_predictions, index=False, sep="\t")
    return prediction_df


STITCH_ERR_BITS = {2: "more events than the capacity of ev_pairs", 8: "a median window outside 1 .. 63",
                   16: "malformed rec_win0 / rec_frame0 tables", 32: "a recording with too few windows to cover it",
                   64: "events that are not sorted and disjoint inside a column (sed_events_hysteresis: onsets that do not "
                       "strictly increase; sed_events_process)"}


def stitch_error_text(entry, err):
    """The ``SedError`` text for the non-zero error word ``err`` that the stitch entry ``entry`` left."""
    return f"{entry} reported err " + ", ".join(f"bit {b} ({t})" for b, t in STITCH_ERR_BITS.items() if err & b) + f" (err = {err})"


def _weighting_code(weighting):
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting must be one of {sorted(WEIGHTINGS)}, got {weighting!r}")
    return WEIGHTINGS[weighting]


def _per_class(value, nclass, dtype, what):
    a = np.asarray(value, dtype=dtype).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, nclass)
    if a.size != nclass:
        raise ValueError(f"{what} must be a scalar or a sequence of {nclass} values, got {a.size}")
    return np.ascontiguousarray(a)


def _stitch_call(entry, win_strong, rec_win0, rec_frame0, total, hop3, thr, win, weighting, capacity, ws_bytes, want_timeline,
                 want_binary=False, n_points=None):
    """The call both stitch entries share: outputs, scratch and ``entry`` (``sed_stitch_sweep`` takes ``n_points``,
    ``sed_stitch_decode`` a binary timeline).  ``thr`` / ``win``: device tensors [points, nclass]; ``weighting``: its code."""
    dev = win_strong.device
    win_strong = win_strong.contiguous().float()
    n_win, T3, NC = win_strong.shape
    n_rec, K = rec_win0.numel() - 1, n_points or 1
    if capacity is None:
        capacity = K * NC * ((total + n_rec) // 2)          # >= K times the sum over recordings of NC * ceil(L3 / 2)
    out = {"ev_ptr": torch.empty(K * n_rec * NC + 1, dtype=torch.int64, device=dev),
           "ev_pairs": torch.empty(max(int(capacity), 1), 2, dtype=torch.int32, device=dev),
           "err": torch.zeros(1, dtype=torch.int32, device=dev),
           "timeline": torch.empty(total, NC, dtype=torch.float32, device=dev) if want_timeline else None,
           "binary": torch.empty(total, NC, dtype=torch.uint8, device=dev) if want_binary else None}
    ws = _lib.scratch(ws_bytes, dev)
    head = (_lib.ptr(win_strong), _lib.ptr(rec_win0), _lib.ptr(rec_frame0), n_rec, T3, NC, int(hop3), weighting)
    if n_points is None:
        points = (_lib.ptr(thr), _lib.ptr(win), _lib.ptr(out["timeline"]), _lib.ptr(out["binary"]))
    else:
        out["n_points"] = K
        points = (K, _lib.ptr(thr), _lib.ptr(win), _lib.ptr(out["timeline"]))
    _lib.check(getattr(_lib.lib(), entry)(*head, *points, _lib.ptr(out["ev_ptr"]), _lib.ptr(out["ev_pairs"]), int(capacity),
                                          _lib.ptr(ws), ws.numel(), _lib.ptr(out["err"]), _lib.stream_ptr()), entry)
    return out


def stitch_decode(win_strong, rec_win0, rec_frame0, total_frames, hop3, threshold=0.5, median_window=5, weighting="taper",
                  capacity=None, want_timeline=True, want_binary=False):
    """``sed_stitch_decode`` on window posteriors [n_win, T3, nclass] (cuda float32) with the device tables ``rec_win0``
    [n_rec + 1] int32 / ``rec_frame0`` [n_rec + 1] int64 of ``total_frames`` timeline frames in all: everything stays on the
    device and nothing synchronises.  Returns a dict: ``ev_ptr`` [n_rec * nclass + 1] int64, ``ev_pairs`` [capacity, 2] int32,
    ``err`` [1] int32 (non-zero: the outputs are invalid, ``STITCH_ERR_BITS``), ``timeline`` / ``binary``
    [total_frames, nclass] or None.  ``threshold`` / ``median_window``: scalars, per-class sequences or device tensors."""
    if win_strong.device.type != "cuda":
        raise _lib.SedError("stitch_decode needs GPU tensors (no CPU fallback)")
    weighting = _weighting_code(weighting)
    dev, NC, total = win_strong.device, win_strong.shape[2], int(total_frames)
    if total * NC >= 2 ** 31:
        raise ValueError(f"{total} timeline frames x {NC} classes: the product must stay below 2^31")
    thr = threshold if torch.is_tensor(threshold) else torch.from_numpy(_per_class(threshold, NC, np.float32, "threshold")).to(dev)
    win = (median_window if torch.is_tensor(median_window)
           else torch.from_numpy(_per_class(median_window, NC, np.int32, "median_window")).to(dev))
    ws_bytes = _lib.lib().sed_stitch_decode_ws_bytes(total, rec_win0.numel() - 1, NC)
    return _stitch_call("sed_stitch_decode", win_strong, rec_win0, rec_frame0, total, hop3, thr, win, weighting, capacity,
                        ws_bytes, want_timeline, want_binary)


def sweep_points(thresholds, median_windows, nclass):
    """K operating points as host arrays ``(thr [K, nclass] float32, win [K, nclass] int32)``: two sequences of K entries
    (one of length 1 is broadcast), every entry a scalar or one value per class.  ValueError otherwise."""
    thresholds, median_windows = list(thresholds), list(median_windows)
    K = max(len(thresholds), len(median_windows))
    if len(thresholds) not in (1, K) or len(median_windows) not in (1, K) or K < 1:
        raise ValueError("thresholds and median_windows must have equal lengths (or length 1)")
    thr = np.stack([_per_class(thresholds[k % len(thresholds)], nclass, np.float32, "a threshold") for k in range(K)])
    win = np.stack([_per_class(median_windows[k % len(median_windows)], nclass, np.int32, "a median window") for k in range(K)])
    return thr, win


def stitch_sweep(win_strong, rec_win0, rec_frame0, total_frames, hop3, thresholds, median_windows, weighting="taper",
                 capacity=None, want_timeline=False):
    """``stitch_decode`` at K operating points from ONE blend (``sed_stitch_sweep``: four launches whatever K is).
    ``thresholds`` / ``median_windows``: sequences of K entries, each a scalar or one value per class (a sequence of length
    1 is broadcast), or device tensors ``[K, nclass]`` float32 / int32.  Returns the dict of ``stitch_decode`` (``binary``
    is None: it would be K timelines) plus ``n_points``: ``ev_ptr`` [K * n_rec * nclass + 1] is one CSR over the columns
    ``(k * n_rec + rec) * nclass + c``, ``ev_pairs`` [capacity, 2] (default: K times ``stitch_decode``'s).  Nothing
    synchronises."""
    weighting = _weighting_code(weighting)
    if win_strong.dim() != 3:
        raise ValueError(f"win_strong must be [n_win, T3, nclass], got {tuple(win_strong.shape)}")
    NC = win_strong.shape[2]
    if torch.is_tensor(thresholds) != torch.is_tensor(median_windows):
        raise ValueError("thresholds and median_windows: both sequences or both device tensors [K, nclass]")
    if torch.is_tensor(thresholds):
        thr, win = thresholds, median_windows
        if thr.dim() != 2 or thr.shape[1] != NC or thr.shape != win.shape or thr.dtype != torch.float32 or win.dtype != torch.int32:
            raise ValueError(f"device operating points: thresholds float32 and median_windows int32, both [K, {NC}]")
    else:
        thr, win = sweep_points(thresholds, median_windows, NC)
    if win_strong.device.type != "cuda" or (torch.is_tensor(thr) and thr.device.type != "cuda"):
        raise _lib.SedError("stitch_sweep needs GPU tensors (no CPU fallback)")
    dev = win_strong.device
    if not torch.is_tensor(thr):
        thr, win = torch.from_numpy(thr).to(dev), torch.from_numpy(win).to(dev)
    thr, win = thr.contiguous(), win.contiguous()
    K, total = thr.shape[0], int(total_frames)
    l = _lib.lib()
    ws_bytes = l.sed_stitch_sweep_ws_bytes(total, rec_win0.numel() - 1, NC, K)
    if ws_bytes == 0:
        raise ValueError(f"sed_stitch_sweep_ws_bytes: {l.sed_last_error().decode()}")
    return _stitch_call("sed_stitch_sweep", win_strong, rec_win0, rec_frame0, total, hop3, thr, win, weighting, capacity,
                        ws_bytes, want_timeline, n_points=K)


def _table_shape(who, ev_ptr, ev_pairs, n_rec, nclass, *beside):
    """The checks every event-table front shares (``beside``: further tensors that have to be on the GPU).  Returns the
    contiguous table and its sizes: ``(ev_ptr, ev_pairs, n_cols, pairs_capacity, K)``."""
    if any(t.device.type != "cuda" for t in (ev_pairs,) + beside):
        raise _lib.SedError(f"{who} needs GPU tensors (no CPU fallback)")
    if (ev_ptr.dtype, ev_pairs.dtype) != (torch.int64, torch.int32) or ev_ptr.numel() < 2 or ev_pairs.dim() != 2 \
            or ev_pairs.shape[1] != 2:
        raise ValueError(f"{who}: ev_ptr int64 [n_cols + 1] and ev_pairs int32 [capacity, 2] expected")
    n_cols, pairs_cap = ev_ptr.numel() - 1, ev_pairs.shape[0]
    if n_rec < 1 or nclass < 1 or n_cols % (n_rec * nclass):
        raise ValueError(f"{who}: {n_cols} columns are no multiple of {n_rec} recordings x {nclass} classes")
    return ev_ptr.contiguous(), ev_pairs.contiguous(), n_cols, pairs_cap, n_cols // (n_rec * nclass)


def _compact_call(entry, head, n_cols, pairs_cap, dev, capacity, err, beside=()):
    """The call the compacting event-table entries share behind their own checks: the workspace size (``ValueError`` with
    the library's text), ``out_ptr``, ``out_pairs`` and one float32 array of ``capacity`` rows per entry of ``beside`` that is
    not None, ``err`` (a new zeroed word by default) and scratch, then ``entry(*head, the outputs, capacity, ws, its size, err,
    stream)``.  ``capacity`` defaults to ``pairs_cap``.  Returns ``(out_ptr, out_pairs, [the row arrays], err)``."""
    capacity = pairs_cap if capacity is None else int(capacity)
    l = _lib.lib()
    ws_bytes = getattr(l, entry + "_ws_bytes")(pairs_cap, n_cols)
    if ws_bytes == 0:
        raise ValueError(f"{entry}_ws_bytes: {l.sed_last_error().decode()}")
    out_ptr = torch.empty(n_cols + 1, dtype=torch.int64, device=dev)
    out_pairs = torch.empty(max(capacity, 1), 2, dtype=torch.int32, device=dev)
    rows = [None if s is None else torch.empty(max(capacity, 1), dtype=torch.float32, device=dev) for s in beside]
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _lib.scratch(ws_bytes, dev)
    _lib.check(getattr(l, entry)(*head, _lib.ptr(out_ptr), _lib.ptr(out_pairs), *map(_lib.ptr, rows), capacity, _lib.ptr(ws),
                                 ws.numel(), _lib.ptr(err), _lib.stream_ptr()), entry)
    return out_ptr, out_pairs, rows, err


def events_hysteresis(lo_ptr, hi_ptr, pairs, capacity=None, err=None):
    """``sed_events_hysteresis``: the events of the low table ``lo_ptr`` [n_cols + 1] that an event of the high table
    ``hi_ptr`` [n_cols + 1] confirms (some high onset inside the low event); both are int64 CSR offsets on the device into the
    one ``pairs`` [pairs_capacity, 2] int32 array.  Returns ``(out_ptr [n_cols + 1] int64, out_pairs [capacity, 2] int32,
    err [1] int32)``; ``capacity`` defaults to ``pairs_capacity`` (it cannot overflow), ``err`` to a new zeroed word - a given
    one is OR-ed into.  Three launches, nothing synchronises."""
    if pairs.device.type != "cuda":
        raise _lib.SedError("events_hysteresis needs GPU tensors (no CPU fallback)")
    if (lo_ptr.dtype, hi_ptr.dtype, pairs.dtype) != (torch.int64, torch.int64, torch.int32) or lo_ptr.numel() != hi_ptr.numel() \
            or lo_ptr.numel() < 2 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("events_hysteresis: lo_ptr / hi_ptr int64 [n_cols + 1] and pairs int32 [capacity, 2] expected")
    pairs, lo_ptr, hi_ptr = pairs.contiguous(), lo_ptr.contiguous(), hi_ptr.contiguous()
    n_cols, pairs_cap = lo_ptr.numel() - 1, pairs.shape[0]
    head = (_lib.ptr(lo_ptr), _lib.ptr(hi_ptr), _lib.ptr(pairs), pairs_cap, n_cols)
    out_ptr, out_pairs, _, err = _compact_call("sed_events_hysteresis", head, n_cols, pairs_cap, pairs.device, capacity, err)
    return out_ptr, out_pairs, err


def hysteresis_points(thresholds_low, thresholds_high, median_windows, nclass):
    """K threshold pairs as host arrays ``(thr_lo [K, nclass], thr_hi [K, nclass], win [K, nclass])``, entries as in
    ``sweep_points`` (a sequence of length 1 is broadcast).  ValueError where the lengths disagree or some ``thr_hi < thr_lo``
    (a NaN threshold included)."""
    lo, hi, mw = list(thresholds_low), list(thresholds_high), list(median_windows)
    K = max(len(lo), len(hi), len(mw))
    if K < 1 or any(len(x) not in (1, K) for x in (lo, hi, mw)):
        raise ValueError("thresholds_low, thresholds_high and median_windows must have equal lengths (or length 1)")
    thr_lo, win = sweep_points([lo[k % len(lo)] for k in range(K)], [mw[k % len(mw)] for k in range(K)], nclass)
    thr_hi, _ = sweep_points([hi[k % len(hi)] for k in range(K)], [1], nclass)
    if not (thr_hi >= thr_lo).all():
        k, c = np.argwhere(~(thr_hi >= thr_lo))[0]
        raise ValueError(f"hysteresis needs thr_hi >= thr_lo: pair {k}, class {c} has {thr_hi[k, c]} < {thr_lo[k, c]}")
    return thr_lo, thr_hi, win


def stitch_hysteresis(win_strong, rec_win0, rec_frame0, total_frames, hop3, thresholds_low, thresholds_high, median_windows,
                      weighting="taper", capacity=None, want_timeline=False):
    """Two-threshold decode at K threshold pairs: per (pair, recording, class) the events ``stitch_decode`` gives at the low
    threshold that hold the onset of an event it gives at the high threshold, both with the pair's ONE median window (the
    definition is in include/dcase_sed.h; at window 1 it is frame-domain hysteresis, for wider windows it is "filter both, then
    select").  ``thresholds_low`` / ``thresholds_high`` / ``median_windows``: host sequences of K entries as in
    ``sweep_points``; ``ValueError`` where some ``thr_hi < thr_lo``, before anything is launched.  ONE ``stitch_sweep`` of 2K
    points ordered ``[lo_0 .. lo_{K-1}, hi_0 .. hi_{K-1}]``, then ONE ``sed_events_hysteresis`` on its table.
    Returns the dict of ``stitch_sweep`` with ``n_points = K`` (``ev_ptr`` [K * n_rec * nclass + 1], ``ev_pairs``
    [capacity, 2]; default capacity: K times ``stitch_decode``'s), so every ``metrics.long_sweep_*`` call takes it unchanged;
    ``err`` is the sweep's word with the select's bits OR-ed in on the device.  Nothing synchronises.
    Clip sets need no path of their own: a batch of clip posteriors ``[n, T, nclass]`` is n one-window recordings
    (``rec_win0 = arange(n + 1)``, ``rec_frame0 = arange(n + 1) * T``, ``hop3 = T``)."""
    if win_strong.dim() != 3:
        raise ValueError(f"win_strong must be [n_win, T3, nclass], got {tuple(win_strong.shape)}")
    NC = win_strong.shape[2]
    thr_lo, thr_hi, win = hysteresis_points(thresholds_low, thresholds_high, median_windows, NC)
    if win_strong.device.type != "cuda":
        raise _lib.SedError("stitch_hysteresis needs GPU tensors (no CPU fallback)")
    dev, K, n_rec = win_strong.device, thr_lo.shape[0], rec_win0.numel() - 1
    if capacity is None:
        capacity = K * NC * ((int(total_frames) + n_rec) // 2)
    out = stitch_sweep(win_strong, rec_win0, rec_frame0, total_frames, hop3, torch.from_numpy(np.concatenate([thr_lo, thr_hi])).to(dev),
                       torch.from_numpy(np.concatenate([win, win])).to(dev), weighting, 2 * int(capacity), want_timeline)
    n_cols = K * n_rec * NC
    ev_ptr, ev_pairs, err = events_hysteresis(out["ev_ptr"][:n_cols + 1], out["ev_ptr"][n_cols:], out["ev_pairs"], int(capacity),
                                              out["err"])
    return {"ev_ptr": ev_ptr, "ev_pairs": ev_pairs, "err": err, "timeline": out["timeline"], "binary": None, "n_points": K}


PROCESS_ORDERS = {"drop_merge": 0, "merge_drop": 1}


def _order_code(order):
    if order not in PROCESS_ORDERS:
        raise ValueError(f"order must be one of {sorted(PROCESS_ORDERS)}, got {order!r}")
    return PROCESS_ORDERS[order]


def process_points(min_event_lengths, min_event_gaps, nclass, frame_seconds, K):
    """Minimum event lengths and gaps in seconds as the host arrays ``(min_len [K, nclass] int32, max_gap [K, nclass] int32)``
    in label frames of ``frame_seconds`` each, the parameters of ``events_process``.  Entries as in ``sweep_points``: sequences
    of K entries or one, every entry a scalar or one value per class; ``None`` disables that half (``min_len = 0``,
    ``max_gap = -1``).  ``min_len = ceil(length / frame_seconds - 1e-9)``: an event must last at least ``length``;
    ``max_gap = floor(gap / frame_seconds + 1e-9)``: gaps up to ``gap`` are closed.  ValueError for negative or NaN seconds
    and for wrong lengths."""
    K, frame_seconds = int(K), float(frame_seconds)
    if K < 1 or not frame_seconds > 0:
        raise ValueError("process_points: K >= 1 and frame_seconds > 0 expected")

    def frames(entries, what, disabled, to_frames):
        if entries is None:
            return np.full((K, nclass), disabled, dtype=np.int32)
        entries = list(entries)
        if len(entries) not in (1, K):
            raise ValueError(f"{what} must have {K} entries (or one)")
        sec = np.stack([_per_class(entries[k % len(entries)], nclass, np.float64, what) for k in range(K)])
        if not (sec >= 0).all() or not np.isfinite(sec).all():
            raise ValueError(f"{what}: finite seconds >= 0 expected")
        fr = to_frames(sec / frame_seconds)
        if (fr >= 2 ** 31).any():
            raise ValueError(f"{what}: more than 2^31 frames")
        return np.ascontiguousarray(fr.astype(np.int32))

    return (frames(min_event_lengths, "min_event_lengths", 0, lambda f: np.ceil(f - 1e-9)),
            frames(min_event_gaps, "min_event_gaps", -1, lambda f: np.floor(f + 1e-9)))


def events_process(ev_ptr, ev_pairs, n_rec, nclass, min_len, max_gap, order="drop_merge", capacity=None, err=None):
    """``sed_events_process``: minimum event length and gap merging on a CSR event table on the device - ``ev_ptr``
    [K * n_rec * nclass + 1] int64 in the sweep's column order, ``ev_pairs`` [pairs_capacity, 2] int32 (the table of
    ``stitch_decode``, ``stitch_sweep`` or ``stitch_hysteresis``).  ``min_len`` / ``max_gap``: label frames, host ``[K, nclass]``
    arrays (``process_points`` makes them from seconds) or device int32 tensors.  ``order``: ``"drop_merge"`` (drop the events
    shorter than ``min_len``, then fuse those a gap of at most ``max_gap`` separates) or ``"merge_drop"``; the definition is
    in include/dcase_sed.h.  Returns ``(out_ptr [n_cols + 1] int64, out_pairs [capacity, 2] int32, err [1] int32)``;
    ``capacity`` defaults to ``pairs_capacity`` (the result never has more events than the input), ``err`` to a new zeroed
    word - a given one is OR-ed into.  Five launches, nothing synchronises."""
    order, n_rec, nclass = _order_code(order), int(n_rec), int(nclass)
    ev_ptr, ev_pairs, n_cols, pairs_cap, K = _table_shape("events_process", ev_ptr, ev_pairs, n_rec, nclass)
    dev, params = ev_pairs.device, []
    for name, p in (("min_len", min_len), ("max_gap", max_gap)):
        if not torch.is_tensor(p):
            p = torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1))).to(dev)
        if p.device != dev or p.dtype != torch.int32 or p.numel() != K * nclass:
            raise ValueError(f"events_process: {name} must be int32 [{K}, {nclass}] (host array or tensor on the table's device)")
        params.append(p.contiguous())
    head = (_lib.ptr(ev_ptr), _lib.ptr(ev_pairs), pairs_cap, n_cols, n_rec, nclass, _lib.ptr(params[0]), _lib.ptr(params[1]),
            order)
    out_ptr, out_pairs, _, err = _compact_call("sed_events_process", head, n_cols, pairs_cap, dev, capacity, err)
    return out_ptr, out_pairs, err


def process_decoded(out, n_rec, nclass, min_len, max_gap, order="drop_merge"):
    """``events_process`` on the dict a stitch entry returned: the same dict with the processed table (same capacity), its
    ``err`` the decode's own word with the step's bits OR-ed in on the device."""
    ev_ptr, ev_pairs, err = events_process(out["ev_ptr"], out["ev_pairs"], n_rec, nclass, min_len, max_gap, order, err=out["err"])
    return dict(out, ev_ptr=ev_ptr, ev_pairs=ev_pairs, err=err)


SCORE_KEYS = {"max": 0, "mean": 1}


def _score_key_code(key):
    if key not in SCORE_KEYS:
        raise ValueError(f"key must be one of {sorted(SCORE_KEYS)}, got {key!r}")
    return SCORE_KEYS[key]


def _scores_call(who, out_or_table, rows, rec0, n_rec, nclass, wanted, err, expected, extra=()):
    """What ``events_scores`` and ``events_tag_scores`` share: the table from the dict of a stitch entry or a pair, its checks
    and those of ``rows`` [*, nclass] float32, ``rec0`` [n_rec + 1] int64 and ``extra``, the ints >= 1 the entry takes in front
    of ``n_rec`` (``ValueError`` with ``expected``), one float32 [pairs_capacity] output per true entry of ``wanted``, ``err``,
    and the call ``sed_<who>``.  Returns ``([the outputs or None], err)``."""
    ev_ptr, ev_pairs = (out_or_table["ev_ptr"], out_or_table["ev_pairs"]) if isinstance(out_or_table, dict) else out_or_table
    n_rec, nclass = int(n_rec), int(nclass)
    ev_ptr, ev_pairs, n_cols, pairs_cap, _ = _table_shape(who, ev_ptr, ev_pairs, n_rec, nclass, rows)
    if rows.dtype != torch.float32 or rows.numel() % nclass or rec0.dtype != torch.int64 or rec0.numel() != n_rec + 1 \
            or any(x < 1 for x in extra):
        raise ValueError(f"{who}: {expected.format(nclass=nclass, n_rec1=n_rec + 1)}")
    rows, rec0 = rows.contiguous(), rec0.contiguous()
    outs = [torch.empty(pairs_cap, dtype=torch.float32, device=ev_pairs.device) if w else None for w in wanted]
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=ev_pairs.device)
    _lib.check(getattr(_lib.lib(), "sed_" + who)(_lib.ptr(rows), rows.numel() // nclass, _lib.ptr(rec0), *extra, n_rec, nclass,
                                                 _lib.ptr(ev_ptr), _lib.ptr(ev_pairs), pairs_cap, n_cols, *map(_lib.ptr, outs),
                                                 _lib.ptr(err), _lib.stream_ptr()), "sed_" + who)
    return outs, err


def events_scores(out_or_table, timeline, rec_frame0, n_rec, nclass, want=("max", "mean"), err=None):
    """``sed_events_scores``: per event of a CSR table on the device the maximum and the mean of ``timeline``
    [total_frames, nclass] (cuda float32: what a stitch entry writes; a batch of clips is ``strong`` reshaped with
    ``rec_frame0 = arange(n + 1) * T3``) over the event's frames - the definition is in include/dcase_sed.h.
    ``out_or_table``: the dict a stitch entry returned or a pair ``(ev_ptr, ev_pairs)``, ``ev_ptr`` [K * n_rec * nclass + 1]
    int64 in the sweep's column order, ``ev_pairs`` [pairs_capacity, 2] int32.  ``want``: which of ``"max"`` / ``"mean"``.
    Returns ``(score_max, score_mean, err)``: float32 [pairs_capacity] device tensors indexed like ``ev_pairs`` (an unwanted
    one is None; entries at and beyond ``ev_ptr[-1]`` are not written), ``err`` [1] int32 - a new zeroed word by default, a
    given one is OR-ed into (``STITCH_ERR_BITS``).  One launch, nothing synchronises."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in SCORE_KEYS for w in want):
        raise ValueError(f"want must name one or both of {sorted(SCORE_KEYS)}, got {want!r}")
    (score_max, score_mean), err = _scores_call("events_scores", out_or_table, timeline, rec_frame0, n_rec, nclass,
                                                ("max" in want, "mean" in want), err,
                                                "timeline float32 [total_frames, {nclass}] and rec_frame0 int64 [{n_rec1}] expected")
    return score_max, score_mean, err


def events_select(ev_ptr, ev_pairs, score_max, score_mean, n_rec, nclass, min_score, key="max", capacity=None, err=None):
    """``sed_events_select``: the events of a CSR table whose score exceeds the minimum of their (point, class) - strictly,
    and a NaN score is never kept.  ``key``: ``"max"`` or ``"mean"``, the score that decides (it must be given); the other
    one may be None.  ``min_score``: a scalar, one value per class, a host ``[K, nclass]`` array or a device float32 tensor of
    K * nclass values.  Returns ``(out_ptr [n_cols + 1] int64, out_pairs [capacity, 2] int32, out_score_max, out_score_mean,
    err [1] int32)``: the kept events in order with their scores compacted alongside (None where the input was None);
    ``capacity`` defaults to the input's (it cannot overflow), ``err`` to a new zeroed word - a given one is OR-ed into.
    Three launches, nothing synchronises."""
    key, n_rec, nclass = _score_key_code(key), int(n_rec), int(nclass)
    ev_ptr, ev_pairs, n_cols, pairs_cap, K = _table_shape("events_select", ev_ptr, ev_pairs, n_rec, nclass)
    dev = ev_pairs.device
    if (score_max, score_mean)[key] is None:
        raise ValueError(f"events_select: key {('max', 'mean')[key]!r} needs that score array")
    scores = []
    for name, s in (("score_max", score_max), ("score_mean", score_mean)):
        if s is not None and (s.device != dev or s.dtype != torch.float32 or s.numel() != pairs_cap):
            raise ValueError(f"events_select: {name} must be float32 [{pairs_cap}] on the table's device")
        scores.append(None if s is None else s.contiguous())
    if not torch.is_tensor(min_score):
        m = np.asarray(min_score, dtype=np.float32)
        m = np.tile(_per_class(m, nclass, np.float32, "min_score"), (K, 1)) if m.size in (1, nclass) else m
        min_score = torch.from_numpy(np.ascontiguousarray(m.reshape(-1))).to(dev)
    if min_score.device != dev or min_score.dtype != torch.float32 or min_score.numel() != K * nclass:
        raise ValueError(f"events_select: min_score must be a scalar, {nclass} values or float32 [{K}, {nclass}] "
                         "(host array or tensor on the table's device)")
    min_score = min_score.contiguous()
    head = (_lib.ptr(ev_ptr), _lib.ptr(ev_pairs), _lib.ptr(scores[0]), _lib.ptr(scores[1]), pairs_cap, n_cols, n_rec, nclass, key,
            _lib.ptr(min_score))
    out_ptr, out_pairs, outs, err = _compact_call("sed_events_select", head, n_cols, pairs_cap, dev, capacity, err, scores)
    return out_ptr, out_pairs, outs[0], outs[1], err


def score_decoded(out, rec_frame0, n_rec, nclass, want=("max", "mean")):
    """``events_scores`` on the dict a stitch entry returned (decoded with ``want_timeline=True``; ``ValueError`` without a
    timeline): the same dict plus ``score_max`` / ``score_mean`` (None when not wanted), its ``err`` the decode's own word
    with the scorer's bits OR-ed in on the device."""
    if out.get("timeline") is None:
        raise ValueError("score_decoded needs the blended timeline: decode with want_timeline=True")
    score_max, score_mean, err = events_scores(out, out["timeline"], rec_frame0, n_rec, nclass, want, err=out["err"])
    return dict(out, score_max=score_max, score_mean=score_mean, err=err)


def select_decoded(out, rec_frame0, n_rec, nclass, min_score, key="max"):
    """``events_select`` on the dict a stitch entry returned: the same dict with the selected table and its compacted scores,
    same capacity.  A dict ``score_decoded`` has not scored yet is scored first (``ValueError`` without a timeline)."""
    _score_key_code(key)
    if out.get("score_" + key) is None:
        out = score_decoded(out, rec_frame0, n_rec, nclass)
    ev_ptr, ev_pairs, score_max, score_mean, err = events_select(out["ev_ptr"], out["ev_pairs"], out.get("score_max"),
                                                                 out.get("score_mean"), n_rec, nclass, min_score, key,
                                                                 err=out["err"])
    return dict(out, ev_ptr=ev_ptr, ev_pairs=ev_pairs, score_max=score_max, score_mean=score_mean, err=err)


def _weak_inputs(who, win_strong, win_att, rec_win0, total_frames, hop3, weighting, n_win=None):
    """The input checks of ``stitch_weak`` and ``pooled_tags`` (``who``; ``n_win``: the latter's host-side window count).
    Returns ``(total_frames, hop3, the weighting's code)`` as ints."""
    weighting = _weighting_code(weighting)
    if win_strong.dim() != 3 or win_att.shape != win_strong.shape:
        raise ValueError(f"win_strong and win_att must both be [n_win, T3, nclass], got {tuple(win_strong.shape)} and "
                         f"{tuple(win_att.shape)}")
    n_tensor, T3, NC = win_strong.shape
    if n_win is not None and int(n_win) != n_tensor:
        raise ValueError(f"the tables describe {int(n_win)} windows, the window tensors hold {n_tensor}")
    total, n_rec = int(total_frames), rec_win0.numel() - 1
    if not 1 <= NC <= 16 or not 1 <= int(hop3) <= T3 <= 4096 or n_rec < 1 or total < 1:
        raise ValueError(f"need 1 <= nclass <= 16, 1 <= hop3 <= T3 <= 4096, n_rec >= 1, total_frames >= 1; got nclass {NC}, "
                         f"hop3 {hop3}, T3 {T3}, n_rec {n_rec}, total_frames {total}")
    if total * NC >= 2 ** 31:
        raise ValueError(f"{total} timeline frames x {NC} classes: the product must stay below 2^31")
    if win_strong.device.type != "cuda" or win_att.device != win_strong.device:
        raise _lib.SedError(f"{who} needs GPU tensors on one device (no CPU fallback)")
    return total, int(hop3), weighting


# The rows being pooled, ``rows`` below: None - one row per recording (``sed_stitch_weak`` / ``sed_stitch_weak_backward``) - or
# ``(rec_span0 on the device, total_spans, span3, ws_bytes, rec_span_off on the device or None)``: ``sed_stitch_span_tags`` /
# ``sed_stitch_span_tags_backward`` without ``rec_span_off``, the piece entries ``sed_stitch_piece_span_tags`` /
# ``sed_stitch_piece_span_tags_backward`` with it.
def _tags_forward(win_strong, win_att, rec_win0, rec_frame0, total, hop3, weighting, rows, err, want_sums):
    """The one forward call of the pooled tags, on checked contiguous float32 window tensors: ``(tags, sums or None)``."""
    l = _lib.lib()
    n_win, T3, NC = win_strong.shape
    n_rec, dev = rec_win0.numel() - 1, win_strong.device
    n_rows = n_rec if rows is None else rows[1]
    tags = torch.empty(n_rows, NC, dtype=torch.float32, device=dev)
    sums = torch.empty(n_rows, NC, 2, dtype=torch.float64, device=dev) if want_sums else None
    ws = _lib.scratch(l.sed_stitch_weak_ws_bytes(total, n_rec, NC) if rows is None else rows[3], dev)
    head = (_lib.ptr(win_strong), _lib.ptr(win_att), _lib.ptr(rec_win0), _lib.ptr(rec_frame0))
    tail = (_lib.ptr(tags), _lib.ptr(sums), _lib.ptr(ws), ws.numel(), _lib.ptr(err), _lib.stream_ptr())
    if rows is None:
        _lib.check(l.sed_stitch_weak(*head, n_rec, T3, NC, hop3, weighting, *tail), "sed_stitch_weak")
    else:
        rec_span0, total_spans, span3, _, span_off = rows
        if span_off is None:
            _lib.check(l.sed_stitch_span_tags(*head, _lib.ptr(rec_span0), total, total_spans, n_rec, T3, NC, hop3, weighting, span3,
                                              *tail), "sed_stitch_span_tags")
        else:
            _lib.check(l.sed_stitch_piece_span_tags(*head, _lib.ptr(rec_span0), total, total_spans, n_rec, T3, NC, hop3, weighting,
                                                    span3, _lib.ptr(span_off), *tail), "sed_stitch_piece_span_tags")
    return tags, sums


def _tags_backward(win_strong, win_att, rec_win0, rec_frame0, hop3, weighting, rows, sums, g_tags, err):
    """The one backward call of the pooled tags, from the forward's sums: ``(d_win_strong, d_win_att)``."""
    l = _lib.lib()
    n_win, T3, NC = win_strong.shape
    n_rec = rec_win0.numel() - 1
    d_strong, d_att = torch.empty_like(win_strong), torch.empty_like(win_att)
    head = (_lib.ptr(win_strong), _lib.ptr(win_att), _lib.ptr(rec_win0), _lib.ptr(rec_frame0))
    tail = (_lib.ptr(sums), _lib.ptr(g_tags), _lib.ptr(d_strong), _lib.ptr(d_att), _lib.ptr(err), _lib.stream_ptr())
    if rows is None:
        _lib.check(l.sed_stitch_weak_backward(*head, n_rec, T3, NC, hop3, weighting, *tail), "sed_stitch_weak_backward")
    else:
        rec_span0, total_spans, span3, _, span_off = rows
        if span_off is None:
            _lib.check(l.sed_stitch_span_tags_backward(*head, _lib.ptr(rec_span0), total_spans, n_rec, T3, NC, hop3, weighting,
                                                       span3, *tail), "sed_stitch_span_tags_backward")
        else:
            _lib.check(l.sed_stitch_piece_span_tags_backward(*head, _lib.ptr(rec_span0), total_spans, n_rec, T3, NC, hop3, weighting,
                                                             span3, _lib.ptr(span_off), *tail),
                       "sed_stitch_piece_span_tags_backward")
    return d_strong, d_att


class _PooledTags(torch.autograd.Function):
    """forward = ``_tags_forward`` with the (num, den) sums kept, backward = ``_tags_backward``; ``rows`` selects the level."""

    @staticmethod
    def forward(ctx, win_strong, win_att, rec_win0, rec_frame0, total, hop3, weighting, rows, err):
        tags, sums = _tags_forward(win_strong, win_att, rec_win0, rec_frame0, total, hop3, weighting, rows, err, True)
        tables = () if rows is None else tuple(t for t in (rows[0], rows[4]) if t is not None)
        ctx.save_for_backward(win_strong, win_att, rec_win0, rec_frame0, sums, *tables)
        ctx.hop3, ctx.weighting, ctx.err = hop3, weighting, err          # (err: the library ORs into it, autograd never sees it)
        ctx.rows = None if rows is None else rows[1:4]
        return tags

    @staticmethod
    def backward(ctx, g_tags):
        win_strong, win_att, rec_win0, rec_frame0, sums, *tables = ctx.saved_tensors
        rows = None if ctx.rows is None else (tables[0],) + ctx.rows + (tables[1] if len(tables) > 1 else None,)
        return _tags_backward(win_strong, win_att, rec_win0, rec_frame0, ctx.hop3, ctx.weighting, rows, sums,
                              g_tags.contiguous().float(), ctx.err) + (None,) * 7


def _pooled(who, win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, weighting, n_win, span=None):
    """``pooled_tags`` and ``pooled_span_tags``: the input checks, the tables' dtype / device check, the rows - one per recording,
    or with ``span = (span3, rec_frame0_host, span_tables[, span_off])`` those of ``_span_rows`` - and the node.  Returns ``(tags, err,
    _span_rows' dict or None)``."""
    total, hop3, weighting = _weak_inputs(who, win_strong, win_att, rec_win0, total_frames, hop3, weighting, n_win)
    if rec_win0.dtype != torch.int32 or rec_frame0.dtype != torch.int64 or rec_frame0.numel() != rec_win0.numel() or \
            rec_win0.device != win_strong.device or rec_frame0.device != win_strong.device:
        raise ValueError("rec_win0 [n_rec + 1] int32 and rec_frame0 [n_rec + 1] int64 must be on the window tensors' device")
    spans, rows = (None, None) if span is None else _span_rows(win_strong, rec_win0, rec_frame0, total, *span)
    err = torch.zeros(1, dtype=torch.int32, device=win_strong.device)
    tags = _PooledTags.apply(win_strong.contiguous().float(), win_att.contiguous().float(), rec_win0.contiguous(),
                             rec_frame0.contiguous(), total, hop3, weighting, rows, err)
    return tags, err, spans


def stitch_weak(win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, weighting="taper", want_sums=False):
    """Recording-level weak tags (``sed_stitch_weak``): ``win_strong`` / ``win_att`` [n_win, T3, nclass] cuda float32 - the
    windows' posteriors and attention (``long_window_posteriors(want_attention=True)``) - are blended like ``stitch_decode``'s
    timeline and pooled over every recording's whole timeline in fp64, ``weak = sum(P * A) / sum(A)``; no timeline is written.
    Tables as for ``stitch_decode``.  Returns a dict, all on the device, nothing synchronises: ``weak`` [n_rec, nclass]
    float32, ``sums`` [n_rec, nclass, 2] float64 (num, den) or None, ``err`` [1] int32 (``STITCH_ERR_BITS`` 16 / 32: the rows
    of such a recording are NaN)."""
    total, hop3, weighting = _weak_inputs("stitch_weak", win_strong, win_att, rec_win0, total_frames, hop3, weighting)
    err = torch.zeros(1, dtype=torch.int32, device=win_strong.device)
    weak, sums = _tags_forward(win_strong.contiguous().float(), win_att.contiguous().float(), rec_win0, rec_frame0, total, hop3,
                               weighting, None, err, want_sums)
    return {"weak": weak, "sums": sums, "err": err}


def pooled_tags(win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, weighting="taper", n_win=None):
    """``stitch_weak``'s recording-level tags as a differentiable function of both window tensors: ``(weak, err)``, ``weak``
    [n_rec, nclass] float32 with an autograd node whose forward is ``sed_stitch_weak`` and whose backward is
    ``sed_stitch_weak_backward`` (the forward's fp64 sums are kept for it); ``err`` [1] int32 on the device, OR-ed into by both
    (``STITCH_ERR_BITS`` 16 / 32; nothing synchronises - read it when convenient, the tags and gradients are invalid when it
    is nonzero).  Arguments as for ``stitch_weak``.  The window tensors must hold exactly ``rec_win0[-1]`` windows: the
    backward writes every element of both gradients over the tables' own window count, which lives on the device.  ``n_win``:
    that count where the caller has it on the host (``train_recording_tags`` does) - checked against the tensors here, with
    no synchronisation; without it the requirement is the caller's."""
    return _pooled("pooled_tags", win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, weighting, n_win)[:2]


def weak_tags_dataframe(weak, filenames, labels, threshold=0.5):
    """The reference's weak-label table (``filename``, ``event_labels``: the labels with ``weak > threshold``, comma-joined in
    label order; empty for a recording without tags) from ``weak`` [n_rec, nclass] (a device tensor or an array).
    ``threshold``: a scalar or one value per class."""
    weak = weak.detach().cpu().numpy() if torch.is_tensor(weak) else np.asarray(weak)
    labels, filenames = list(labels), list(filenames)
    if weak.shape != (len(filenames), len(labels)):
        raise ValueError(f"weak is {weak.shape}, expected {(len(filenames), len(labels))} (recordings, labels)")
    on = weak > _per_class(threshold, len(labels), np.float32, "threshold")[None, :]
    return pd.DataFrame({"filename": filenames,
                         "event_labels": [",".join(l for l, k in zip(labels, row) if k) for row in on]},
                        columns=["filename", "event_labels"])


def span_table(long_set_or_L3s, span3, device=None):
    """The span offsets of recordings cut into spans of ``span3`` label frames (include/dcase_sed.h: recording r with L3_r
    frames has ceil(L3_r / span3) spans, only the last may be shorter).  ``long_set_or_L3s``: a ``LongRecordingSet`` or the
    recordings' lengths in label frames.  ``span3`` is clamped to the longest recording, so an "infinite" span is one span per
    recording.  Returns ``(rec_span0 host int64 [n_rec + 1], rec_span0 on the device, total_spans, span3 clamped)``; the device
    is the set's, or ``device`` - given lengths and no device, the device table is None and nothing touches a GPU."""
    if isinstance(long_set_or_L3s, LongRecordingSet):
        L3s = np.diff(long_set_or_L3s.rec_frame0_host)
        device = long_set_or_L3s.rec_frame0.device if device is None else device
    else:
        L3s = np.asarray(list(long_set_or_L3s), dtype=np.int64).reshape(-1)
    if L3s.size < 1 or (L3s < 1).any():
        raise ValueError("span_table: at least one recording, every length >= 1 label frame")
    if isinstance(span3, (float, np.floating)) and not np.isfinite(span3):
        if not span3 > 0:
            raise ValueError(f"span3 must be >= 1 label frame, got {span3!r}")
        span3 = int(L3s.max())
    if int(span3) != span3 or span3 < 1:
        raise ValueError(f"span3 must be a whole number of label frames >= 1, got {span3!r}")
    span3 = int(min(int(span3), int(L3s.max())))
    host = np.concatenate([[0], np.cumsum((L3s + span3 - 1) // span3)]).astype(np.int64)
    dev_table = None if device is None else torch.from_numpy(host).to(device)
    return host, dev_table, int(host[-1]), span3


def _span_rows(win_strong, rec_win0, rec_frame0, total, span3, rec_frame0_host=None, span_tables=None, span_off=None):
    """The span table of a span-level call, resolved once: the recordings' lengths from ``rec_frame0_host`` (without it
    ``rec_frame0`` is copied to the host), then ``span_table``'s table copied to the device - or, with ``span_tables = (rec_span0
    host, rec_span0 on the device)``, the caller's, checked against the lengths on the host and nothing copied - and the
    workspace size (0: ``ValueError`` with the library's reason).  Returns ``(the keys rec_span0, rec_span0_host, total_spans
    and span3 (clamped) of the fronts' dicts, the rows for _tags_forward)``.

    ``span_off`` - a device int32 [n_rec] tensor, or ``(host, device)`` where the caller has both - makes the call one over
    PIECES (include/dcase_sed.h: ``sed_stitch_piece_span_tags``): ``span_tables`` is then required and is the pieces' own
    table, ``span3`` is taken as given, and what is checked on the host is the piece rule - ``off >= 0``, at least one span
    per piece, ``off + (n - 1) * span3 < L3``."""
    if rec_frame0_host is None:
        rec_frame0_host = rec_frame0.cpu().numpy()
    L3s = np.diff(np.asarray(rec_frame0_host, dtype=np.int64).reshape(-1))
    n_rec, dev = rec_win0.numel() - 1, win_strong.device
    if L3s.size != n_rec:
        raise ValueError(f"rec_frame0_host describes {L3s.size} recordings, the tables {n_rec}")
    off_dev = None
    if span_off is not None:
        if span_tables is None:
            raise ValueError("span_off needs span_tables = (rec_span0 host, rec_span0 on the device): the pieces' own span table")
        off_host, off_dev = span_off if isinstance(span_off, tuple) else (span_off.cpu().numpy(), span_off)
        off_host = np.asarray(off_host, dtype=np.int64).reshape(-1)
        host, rec_span0 = np.asarray(span_tables[0], dtype=np.int64).reshape(-1), span_tables[1]
        if isinstance(span3, (float, np.floating)) and not np.isfinite(span3) or int(span3) != span3 or span3 < 1:
            raise ValueError(f"span3 must be a whole number of label frames >= 1, got {span3!r}")
        span3, n = int(span3), np.diff(host)
        if host.size != n_rec + 1 or off_host.size != n_rec or host[0] != 0 or (n < 1).any() or (off_host < 0).any() or \
                (off_host + (n - 1) * span3 >= L3s).any():
            raise ValueError("span_off / span_tables do not describe pieces: need rec_span0[0] == 0, off >= 0, at least one span "
                             "per piece and off + (n - 1) * span3 < L3")
        if off_dev.dtype != torch.int32 or off_dev.numel() != n_rec or off_dev.device != dev:
            raise ValueError("span_off must be [n_rec] int32 on the window tensors' device")
        total_spans, off_dev = int(host[-1]), off_dev.contiguous()
    elif span_tables is None:
        host, rec_span0, total_spans, span3 = span_table(L3s, span3, dev)
    else:
        host, _, total_spans, span3 = span_table(L3s, span3)
        given, rec_span0 = span_tables
        if not np.array_equal(np.asarray(given, dtype=np.int64).reshape(-1), host):
            raise ValueError("span_tables is not span_table's for these recordings and this span3")
    if span_tables is not None:
        if rec_span0.dtype != torch.int64 or rec_span0.numel() != n_rec + 1 or rec_span0.device != dev:
            raise ValueError("span_tables' device table must be [n_rec + 1] int64 on the window tensors' device")
    l = _lib.lib()
    ws_name = "sed_stitch_span_tags_ws_bytes" if off_dev is None else "sed_stitch_piece_span_tags_ws_bytes"
    ws_bytes = getattr(l, ws_name)(total, total_spans, n_rec, win_strong.shape[2], span3)
    if ws_bytes == 0:
        raise ValueError(f"{ws_name}: {l.sed_last_error().decode()}")
    return ({"rec_span0": rec_span0, "rec_span0_host": host, "total_spans": total_spans, "span3": span3},
            (rec_span0.contiguous(), total_spans, span3, ws_bytes, off_dev))


def stitch_span_tags(win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, span3, weighting="taper", want_sums=False,
                     rec_frame0_host=None, span_tables=None, span_off=None):
    """Span-level weak tags (``sed_stitch_span_tags``): ``stitch_weak``'s blend and fp64 pooling per span of ``span3`` label
    frames of every recording instead of per recording (the definition is in include/dcase_sed.h); arguments as for
    ``stitch_weak``.  The span table needs the recordings' lengths on the host: ``rec_frame0_host`` (a ``LongRecordingSet``
    has it) - without it ``rec_frame0`` is copied to the host once.  ``span3`` is clamped to the longest recording.  Returns a
    dict, the tensors on the device: ``tags`` [total_spans, nclass] float32, ``sums`` [total_spans, nclass, 2] float64 (num,
    den) or None, ``rec_span0`` [n_rec + 1] int64, ``rec_span0_host``, ``total_spans``, ``span3`` (clamped), ``err`` [1] int32
    (``STITCH_ERR_BITS`` 16 / 32: the rows of such a recording are NaN).  Two launches.

    ``span_off`` None: today's entry.  ``span_off`` [n_rec] int32 on the device: the tables describe PIECES of recordings
    (``longrec.span_pieces``, ``sed_stitch_piece_span_tags``) - a piece owns its table rows' windows and frames like a
    recording, ``span_tables = (rec_span0 host, rec_span0 on the device)`` (required) says how many spans it holds and
    ``span_off[r]`` at which local frame its first span starts; ``span3`` is not clamped.  A span's tags and sums are then
    bit-equal to the whole recording's, given the same window posteriors."""
    total, hop3, weighting = _weak_inputs("stitch_span_tags", win_strong, win_att, rec_win0, total_frames, hop3, weighting)
    spans, rows = _span_rows(win_strong, rec_win0, rec_frame0, total, span3, rec_frame0_host, span_tables, span_off)
    err = torch.zeros(1, dtype=torch.int32, device=win_strong.device)
    tags, sums = _tags_forward(win_strong.contiguous().float(), win_att.contiguous().float(), rec_win0, rec_frame0, total, hop3,
                               weighting, rows, err, want_sums)
    return {"tags": tags, "sums": sums, **spans, "err": err}


def pooled_span_tags(win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, span3, weighting="taper", n_win=None,
                     rec_frame0_host=None, span_tables=None, span_off=None):
    """``stitch_span_tags``'s span-level tags as a differentiable function of both window tensors: ``pooled_tags``' node with
    ``sed_stitch_span_tags`` (its fp64 sums are kept) as the forward and ``sed_stitch_span_tags_backward`` as the backward.
    Arguments and host checks as for ``pooled_tags`` (the window tensors must hold exactly ``rec_win0[-1]`` windows; ``n_win``:
    that count where the caller has it on the host), ``span3`` / ``rec_frame0_host`` as for ``stitch_span_tags``: the span
    table comes from ``span_table`` (``span3`` clamped to the longest recording) and is copied to the device - unless the
    caller has one for exactly these recordings already, ``span_tables = (rec_span0 host, rec_span0 on the device)``
    (``train_span_tags`` prepares its batches' once per epoch); it is then checked against the lengths on the host and
    nothing is copied.  Returns a dict like ``stitch_span_tags``'s: ``tags`` [total_spans, nclass] float32 (differentiable),
    ``rec_span0``, ``rec_span0_host``, ``total_spans``, ``span3`` (clamped), ``err`` [1] int32 on the device, OR-ed into by
    forward and backward (``STITCH_ERR_BITS`` 16 / 32: tags and gradients are invalid when it is nonzero).  With
    ``rec_frame0_host`` nothing synchronises.

    ``span_off`` (None: today's entries and bytes): as for ``stitch_span_tags`` - the tables describe pieces, the same node
    runs ``sed_stitch_piece_span_tags`` and ``sed_stitch_piece_span_tags_backward``, and the gradient is that of exactly the
    loss terms of the pieces' spans (window elements whose frame belongs to no span of the piece get +0.0).  A device tensor
    is copied to the host once for the check; ``(host, device)`` copies nothing."""
    tags, err, spans = _pooled("pooled_span_tags", win_strong, win_att, rec_win0, rec_frame0, total_frames, hop3, weighting, n_win,
                               (span3, rec_frame0_host, span_tables, span_off))
    return {"tags": tags, **spans, "err": err}


def events_tag_scores(out_or_table, tags, rec_span0, span3, n_rec, nclass, err=None):
    """``sed_events_tag_scores``: per event of a CSR table on the device the largest non-NaN span tag among the spans it
    touches (``tags`` [total_spans, nclass] cuda float32 and ``rec_span0`` [n_rec + 1] int64 as ``stitch_span_tags`` returns
    them, ``span3`` the clamped span length it used).  ``out_or_table`` as for ``events_scores``.  Returns ``(tag_score
    float32 [pairs_capacity], err [1] int32)``; a given ``err`` is OR-ed into.  One launch, nothing synchronises."""
    (tag_score,), err = _scores_call("events_tag_scores", out_or_table, tags, rec_span0, n_rec, nclass, (True,), err,
                                     "tags float32 [total_spans, {nclass}], rec_span0 int64 [{n_rec1}] and span3 >= 1 expected",
                                     extra=(int(span3),))
    return tag_score, err


def gate_decoded(out, span_tags, n_rec, nclass, min_tag):
    """The tag gate on the dict a stitch entry returned: an event is kept iff the largest tag of the spans it touches exceeds
    ``min_tag`` of its (point, class) - strictly, and an event whose spans are all NaN is never kept.  ``span_tags``: the dict
    of ``stitch_span_tags``; ``min_tag``: a scalar, one value per class, a host ``[K, nclass]`` array or a device float32
    tensor, as ``events_select``'s ``min_score``.  ``events_tag_scores``, then ``events_select`` with the tag score as the
    key: four launches, nothing synchronises.  Returns the same dict with the gated table (same capacity) and ``tag_score``,
    the kept events' scores; its ``err`` is the decode's own word with both steps' bits OR-ed in on the device.  Scores a
    ``score_decoded`` left in the dict belong to the table before the gate and are dropped."""
    tag_score, err = events_tag_scores(out, span_tags["tags"], span_tags["rec_span0"], span_tags["span3"], n_rec, nclass,
                                       err=out["err"])
    ev_ptr, ev_pairs, tag_score, _, err = events_select(out["ev_ptr"], out["ev_pairs"], tag_score, None, n_rec, nclass, min_tag,
                                                        "max", err=err)
    out = {k: v for k, v in out.items() if k not in ("score_max", "score_mean")}
    return dict(out, ev_ptr=ev_ptr, ev_pairs=ev_pairs, tag_score=tag_score, err=err)


RASTER_COMBINES = {"replace": 0, "max": 1}
RASTER_ERR_BITS = {8: "a class whose operating point lies outside the table's points",
                   16: "malformed ev_ptr / rec_frame0 tables or destination rows outside the pool",
                   64: "events that are not sorted and disjoint inside their recording"}


def _combine_code(combine):
    if combine not in RASTER_COMBINES:
        raise ValueError(f"combine must be one of {sorted(RASTER_COMBINES)}, got {combine!r}")
    return RASTER_COMBINES[combine]


def rows_overlap(row0, n_rows):
    """True when two of the row ranges ``[row0[r], row0[r] + n_rows[r])`` share a row (empty ranges share nothing)."""
    row0, n_rows = np.asarray(row0, dtype=np.int64).reshape(-1), np.asarray(n_rows, dtype=np.int64).reshape(-1)
    keep = n_rows > 0
    row0, n_rows = row0[keep], n_rows[keep]
    order = np.argsort(row0, kind="stable")
    return bool((row0[order][1:] < (row0 + n_rows)[order][:-1]).any())


def events_rasterize(out_or_table, rec_frame0, n_rec, nclass, dst=None, dst_row0=None, values=None, point=None,
                     combine="replace", err=None, rec_frame0_host=None):
    """``sed_events_rasterize``: a CSR event table on the device turned into label rows [*, nclass] float32, in place in
    ``dst`` - the definition is in include/dcase_sed.h.  ``out_or_table``: the dict a stitch entry returned or a pair
    ``(ev_ptr, ev_pairs)``, ``ev_ptr`` [K * n_rec * nclass + 1] int64 in the sweep's column order; ``rec_frame0`` [n_rec + 1]
    int64 on the device.  ``dst``: a contiguous cuda float32 tensor of ``dst_rows * nclass`` elements (a label pool); None
    allocates ``[total_frames, nclass]`` (the rows of the dict's timeline where it has one, else one host read of
    ``rec_frame0[-1]``).  ``dst_row0`` [n_rec]: the first ``dst`` row of every recording - a host sequence or a device int64
    tensor; None: ``rec_frame0`` itself, a contiguous timeline.  ``values`` [pairs_capacity] float32 on the device: the value
    of every event (``score_max`` / ``score_mean`` of ``events_scores`` for soft labels), None: 1.0.  ``point``: the operating
    point each class is taken from - None (point 0), an int, one int per class, or a device int32 tensor [nclass].
    ``combine``: ``"replace"`` (covered elements take the value, the recordings' other elements +0.0) or ``"max"`` (covered
    elements take the larger of value and old content, the others stay); anything else raises ``ValueError``.  Recordings
    whose destination rows overlap are refused (``ValueError``) when ``dst_row0`` is a host sequence and ``rec_frame0_host``
    is given; with device tables that is the caller's responsibility.  Returns ``(dst, err)``: ``err`` [1] int32 - a new zeroed
    word by default, a given one is OR-ed into (``RASTER_ERR_BITS``; non-zero: ``dst`` is invalid).  Two launches, nothing
    synchronises."""
    combine, n_rec, nclass = _combine_code(combine), int(n_rec), int(nclass)
    timeline = out_or_table.get("timeline") if isinstance(out_or_table, dict) else None
    ev_ptr, ev_pairs = (out_or_table["ev_ptr"], out_or_table["ev_pairs"]) if isinstance(out_or_table, dict) else out_or_table
    ev_ptr, ev_pairs, n_cols, pairs_cap, K = _table_shape("events_rasterize", ev_ptr, ev_pairs, n_rec, nclass, rec_frame0)
    dev = ev_pairs.device
    if rec_frame0.dtype != torch.int64 or rec_frame0.numel() != n_rec + 1:
        raise ValueError(f"events_rasterize: rec_frame0 int64 [{n_rec + 1}] expected")
    rec_frame0 = rec_frame0.contiguous()
    if values is not None and (not torch.is_tensor(values) or values.device != dev or values.dtype != torch.float32
                               or values.numel() != pairs_cap):
        raise ValueError(f"events_rasterize: values must be float32 [{pairs_cap}] on the table's device")
    values = None if values is None else values.contiguous()
    if point is not None and not torch.is_tensor(point):
        pts = _per_class(point, nclass, np.int64, "point")
        if (pts < 0).any() or (pts >= K).any():
            raise ValueError(f"events_rasterize: point must lie in [0, {K}), got {pts.tolist()}")
        point = torch.from_numpy(pts.astype(np.int32)).to(dev)
    if point is not None and (point.device != dev or point.dtype != torch.int32 or point.numel() != nclass):
        raise ValueError(f"events_rasterize: point must be int32 [{nclass}] (host values or a tensor on the table's device)")
    point = None if point is None else point.contiguous()
    if dst is None:
        total = timeline.shape[0] if timeline is not None else int(rec_frame0[-1].item())
        dst = torch.empty(total, nclass, dtype=torch.float32, device=dev)
    if not torch.is_tensor(dst) or dst.device != dev or dst.dtype != torch.float32 or not dst.is_contiguous() \
            or dst.numel() % nclass:
        raise ValueError(f"events_rasterize: dst must be a contiguous float32 tensor of rows x {nclass} on the table's device")
    dst_rows = dst.numel() // nclass
    if dst_row0 is not None and not torch.is_tensor(dst_row0):
        row0 = np.asarray(dst_row0, dtype=np.int64).reshape(-1)
        if row0.size != n_rec:
            raise ValueError(f"events_rasterize: dst_row0 must hold {n_rec} rows, got {row0.size}")
        if rec_frame0_host is not None:
            L3 = np.diff(np.asarray(rec_frame0_host, dtype=np.int64).reshape(-1))
            if L3.size != n_rec:
                raise ValueError(f"events_rasterize: rec_frame0_host must hold {n_rec + 1} entries")
            if (row0 < 0).any() or (row0 + L3 > dst_rows).any():
                raise ValueError(f"events_rasterize: a recording's rows reach outside the {dst_rows} rows of dst")
            if rows_overlap(row0, L3):
                raise ValueError("events_rasterize: two recordings' destination rows overlap")
        dst_row0 = torch.from_numpy(np.ascontiguousarray(row0)).to(dev)
    if dst_row0 is not None and (dst_row0.device != dev or dst_row0.dtype != torch.int64 or dst_row0.numel() != n_rec):
        raise ValueError(f"events_rasterize: dst_row0 must be int64 [{n_rec}] (host values or a tensor on the table's device)")
    dst_row0 = None if dst_row0 is None else dst_row0.contiguous()
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().sed_events_rasterize(_lib.ptr(ev_ptr), _lib.ptr(ev_pairs), _lib.ptr(values), pairs_cap, K,
                                               _lib.ptr(point), _lib.ptr(rec_frame0), n_rec, nclass, _lib.ptr(dst), dst_rows,
                                               _lib.ptr(dst_row0), combine, _lib.ptr(err), _lib.stream_ptr()),
               "sed_events_rasterize")
    return dst, err


def rasterize_decoded(out, rec_frame0, n_rec, nclass, soft=None, point=None):
    """``events_rasterize`` on the dict a stitch entry, ``process_decoded``, ``select_decoded`` or ``gate_decoded`` returned:
    the same dict plus ``labels`` [total_frames, nclass] float32, the table as a contiguous label timeline (hard 0 / 1 labels;
    ``soft="max"`` / ``"mean"``: every event carries that score of the dict's ``timeline`` - ``events_scores`` on the table
    as it is now; ``ValueError`` without a timeline).  ``point`` as for ``events_rasterize``.  Its ``err`` is the dict's own
    word with the bits of both steps OR-ed in on the device."""
    values, err = None, out["err"]
    if soft is not None:
        _score_key_code(soft)
        if out.get("timeline") is None:
            raise ValueError("rasterize_decoded(soft=...) needs the blended timeline: decode with want_timeline=True")
        score_max, score_mean, err = events_scores(out, out["timeline"], rec_frame0, n_rec, nclass, (soft,), err=err)
        values = score_max if soft == "max" else score_mean
    total = next((out[k].shape[0] for k in ("timeline", "binary") if out.get(k) is not None), None)
    dst = None if total is None else torch.empty(total, int(nclass), dtype=torch.float32, device=out["ev_pairs"].device)
    labels, err = events_rasterize(out, rec_frame0, n_rec, nclass, dst=dst, values=values, point=point, err=err)
    return dict(out, labels=labels, err=err)


def span_tags_dataframe(tags, rec_span0, span3, filenames, labels, threshold=0.5, frame_seconds=None, L3s=None):
    """The span-level twin of ``weak_tags_dataframe``: one row per (recording, span) with ``filename``, ``onset``, ``offset``
    (seconds: span s of a recording covers the label frames ``s * span3 .. (s + 1) * span3`` of ``frame_seconds`` each -
    default: the frame of baseline/config.py at pooling ratio 1; the last span's offset is cut at the recording's end when
    its length ``L3s`` in label frames is given) and ``event_labels``: the labels whose tag exceeds ``threshold`` (a scalar or
    one value per class), comma-joined in label order.  ``tags`` [total_spans, nclass]: a device tensor or an array;
    ``rec_span0`` [n_rec + 1]: the host table of ``span_table``."""
    tags = tags.detach().cpu().numpy() if torch.is_tensor(tags) else np.asarray(tags)
    rec_span0 = rec_span0.cpu().numpy() if torch.is_tensor(rec_span0) else np.asarray(rec_span0, dtype=np.int64)
    labels, filenames, span3 = list(labels), list(filenames), int(span3)
    if rec_span0.shape != (len(filenames) + 1,) or tags.shape != (int(rec_span0[-1]), len(labels)) or span3 < 1:
        raise ValueError(f"tags is {tags.shape}, rec_span0 {rec_span0.shape}: expected {(int(rec_span0[-1]), len(labels))} "
                         f"(spans, labels) and {(len(filenames) + 1,)}")
    frame_seconds = _Cfg.hop_length / _Cfg.sample_rate if frame_seconds is None else float(frame_seconds)
    per_rec = np.diff(rec_span0)
    rec = np.repeat(np.arange(len(filenames)), per_rec)
    s = np.arange(len(rec)) - np.repeat(rec_span0[:-1], per_rec)
    off = (s + 1) * span3
    if L3s is not None:
        off = np.minimum(off, np.asarray(list(L3s), dtype=np.int64)[rec])
    on = tags > _per_class(threshold, len(labels), np.float32, "threshold")[None, :]
    return pd.DataFrame({"filename": np.asarray(filenames, dtype=object)[rec], "onset": s * span3 * frame_seconds,
                         "offset": off * frame_seconds,
                         "event_labels": [",".join(l for l, k in zip(labels, row) if k) for row in on]},
                        columns=["filename", "onset", "offset", "event_labels"])


def tag_span_frames(tag_span, frame_seconds):
    """``tag_span`` seconds as whole label frames of ``frame_seconds`` each: rounded down, at least 1 (an infinite span stays
    infinite: ``span_table`` clamps it).  ValueError unless ``tag_span > 0``."""
    tag_span = float(tag_span)
    if not tag_span > 0:
        raise ValueError(f"tag_span must be > 0 seconds, got {tag_span!r}")
    if np.isinf(tag_span):
        return tag_span
    return max(int(np.floor(tag_span / float(frame_seconds) + 1e-9)), 1)


def long_window_posteriors(model, long_set, nclass, batch_size=64, want_attention=False):
    """The strong posteriors [n_win, T3, nclass] of every window of ``long_set``, from the eval-mode model ``batch_size``
    windows at a time; they stay on the device.  ``want_attention=True``: ``(win_strong, win_att)``, the attention of the same
    forwards (``CRNN.last_attention`` per batch), same shape."""
    dev = next(model.parameters()).device
    was_training = model.training
    model.eval()
    win_strong = win_att = None
    try:
        with torch.no_grad():
            for i0, idx, x in eval_batches(long_set, batch_size, dev):
                strong, _ = model(x)
                if win_strong is None:
                    if tuple(strong.shape[1:]) != (long_set.T3, nclass):
                        raise ValueError(f"the model gives {tuple(strong.shape[1:])} per window, the set and the labels "
                                         f"{(long_set.T3, nclass)}")
                    win_strong = torch.empty(long_set.n_clips, long_set.T3, nclass, dtype=torch.float32, device=dev)
                    win_att = torch.empty_like(win_strong) if want_attention else None
                win_strong[i0:i0 + len(idx)].copy_(strong)
                if want_attention:
                    win_att[i0:i0 + len(idx)].copy_(model.last_attention())
    finally:
        model.train(was_training)
    return (win_strong, win_att) if want_attention else win_strong


def get_long_predictions(model, long_set, decoder_or_labels, pooling_time_ratio=None, save_predictions=None, batch_size=64,
                         cfg=None, threshold=0.5, median_window=None, weighting="taper", return_posteriors=False,
                         return_weak=False, threshold_high=None, min_event_length=None, min_event_gap=None,
                         process_order="drop_merge", event_scores=False, min_event_score=None, score_key="max", tag_span=None,
                         min_span_tag=None, return_span_tags=False, return_table=False):
    """Events of recordings of any lengths (a ``LongRecordingSet``): the windows go through the eval-mode model
    ``batch_size`` at a time, their strong posteriors are blended into one timeline per recording (``weighting``: "taper"
    or "uniform"), and ONE threshold, median filter and run-length decode runs over each whole timeline
    (``sed_stitch_decode``), followed by one host copy of the event table.

    Returns the DataFrame of ``get_predictions`` (event_label, onset, offset, filename; seconds by its formula
    ``frame * pooling_time_ratio / (sample_rate / hop_length)`` from ``cfg``; the same TSV when ``save_predictions`` is
    given), rows ordered (recording, class, time).  ``threshold`` / ``median_window`` (default ``cfg.median_window``): a
    scalar or one value per class.  ``decoder_or_labels``: ``many_hot_encoder.decode_strong`` (the labels are its owner's)
    or a plain list of labels.  ``return_posteriors=True``: also the list of per-recording [L3_r, nclass] device views of
    the blended timeline and the [n_win, T3, nclass] window posteriors.  ``return_weak=True``: the recording-level weak tags
    [n_rec, nclass] (a device tensor; ``stitch_weak`` on the same single pass through the model) are appended to what is
    returned; ``weak_tags_dataframe`` turns them into the weak-label table.  ``threshold_high`` (a scalar or one value per
    class, ``>= threshold``): the two-threshold decode of ``stitch_hysteresis`` at one pair - ``threshold`` draws the events,
    an event is kept when ``threshold_high`` confirms it; None changes nothing.  ``min_event_length`` / ``min_event_gap``
    (seconds, each a scalar or one value per class): events shorter than the length are dropped and events a gap of at most
    ``min_event_gap`` separates are fused, in the order ``process_order`` ("drop_merge" or "merge_drop") - one
    ``events_process`` on the decoded table (after the two-threshold select when ``threshold_high`` is given), in frames of
    ``pooling_time_ratio * hop_length / sample_rate`` seconds (``process_points``).  Both None: no launch, the same frame.
    ``event_scores=True``: the final table (after the two-threshold select and ``events_process`` where asked for) is scored
    on the blended timeline (``events_scores``: the decode it already runs writes the timeline) and the columns ``score_max``
    / ``score_mean`` are appended to the frame and the TSV.  ``min_event_score`` (a scalar or one value per class; implies the
    scoring): only the events whose ``score_key`` ("max" or "mean") score exceeds it are kept (``events_select``, before the
    host copy).  ``tag_span`` (seconds, rounded down to whole label frames, at least 1; ``float("inf")``: one span per
    recording): span-level weak tags are pooled over spans of that length from the same single pass through the model
    (``stitch_span_tags``).  ``min_span_tag`` (a scalar or one value per class; NaN raises): the tag gate - an event is kept
    only when it touches a span whose tag exceeds it (``gate_decoded``), right after the decode (after the two-threshold
    select), BEFORE ``events_process`` and the event scores: mask, then post-process.  ``return_span_tags=True`` appends
    ``(tags [total_spans, nclass] device tensor, rec_span0 host, span3)`` to what is returned (``span_tags_dataframe`` makes
    their table).  ``min_span_tag`` or ``return_span_tags`` without ``tag_span``: ``ValueError`` before any forward.
    ``return_table=True`` appends the device dict of the FINAL table to what is returned: ``ev_ptr``, ``ev_pairs``,
    ``timeline`` (or None when nothing asked for it) and, when scored, ``score_max`` / ``score_mean`` indexed like
    ``ev_pairs`` - what ``events_rasterize`` and ``relabel`` take.  With the defaults nothing new is launched and the frame is
    column for column the same."""
    if not isinstance(return_table, (bool, np.bool_)):
        raise ValueError(f"return_table must be True or False, got {return_table!r}")
    s = _long_events(model, long_set, decoder_or_labels, pooling_time_ratio, batch_size, cfg, threshold, median_window, weighting,
                     return_posteriors, return_weak, threshold_high, min_event_length, min_event_gap, process_order, event_scores,
                     min_event_score, score_key, tag_span, min_span_tag, return_span_tags)
    labels, pool, cfg, NC, out, scored = s["labels"], s["pool"], s["cfg"], s["NC"], s["out"], s["scored"]
    ev_ptr = out["ev_ptr"].cpu().numpy()
    ev = out["ev_pairs"][:int(ev_ptr[-1])].cpu().numpy()
    per_col = np.diff(ev_ptr)
    col = np.repeat(np.arange(per_col.size), per_col)
    rec, cls = col // NC, col % NC
    per_rec = per_col.reshape(long_set.n_rec, NC).sum(1)
    index = np.arange(len(col)) - np.repeat(np.r_[0, np.cumsum(per_rec)[:-1]], per_rec)     # 0 .. k - 1 per recording
    prediction_df = pd.DataFrame({"event_label": np.asarray(labels, dtype=object)[cls],
                                  "onset": ev[:, 0].astype(np.int64), "offset": ev[:, 1].astype(np.int64),
                                  "filename": np.asarray(long_set.filenames, dtype=object)[rec]}, index=index,
                                 columns=["event_label", "onset", "offset", "filename"])
    prediction_df.onset = prediction_df.onset * pool / (cfg.sample_rate / cfg.hop_length)
    prediction_df.offset = prediction_df.offset * pool / (cfg.sample_rate / cfg.hop_length)
    if scored:
        prediction_df["score_max"] = s["score_max"][:len(ev)].cpu().numpy()
        prediction_df["score_mean"] = s["score_mean"][:len(ev)].cpu().numpy()
    if save_predictions is not None:
        prediction_df.to_csv(save_predictions, index=False, sep="\t")
    result = (prediction_df,)
    if return_posteriors:
        f0 = long_set.rec_frame0_host
        result += ([out["timeline"][int(f0[r]):int(f0[r + 1])] for r in range(long_set.n_rec)], s["win_strong"])
    if return_weak:
        result += (s["weak"],)
    if return_span_tags:
        span_tags = s["span_tags"]
        result += ((span_tags["tags"], span_tags["rec_span0_host"], span_tags["span3"]),)
    if return_table:
        result += (_final_table(s),)
    return result if len(result) > 1 else prediction_df


def _final_table(s):
    """The device dict of the final table of one ``_long_events`` chain (``get_long_predictions(return_table=True)``)."""
    table = {"ev_ptr": s["out"]["ev_ptr"], "ev_pairs": s["out"]["ev_pairs"], "timeline": s["out"]["timeline"]}
    if s["scored"]:
        table.update(score_max=s["score_max"], score_mean=s["score_mean"])
    return table


def _long_events(model, long_set, decoder_or_labels, pooling_time_ratio, batch_size, cfg, threshold, median_window, weighting,
                 return_posteriors, return_weak, threshold_high, min_event_length, min_event_gap, process_order, event_scores,
                 min_event_score, score_key, tag_span, min_span_tag, return_span_tags, known_tags=None):
    """The device chain ``get_long_predictions`` and ``pseudo_label`` share (the arguments are the former's): the checks, the
    forwards, the decode, the gate, ``events_process``, the scores and the select, and ONE check of every error word.
    ``known_tags`` [n_rec, nclass] (``pseudo_label``): the gate runs on these tags with one span per recording and a minimum of
    0.5 in the place of pooled span tags.  Returns a dict: ``out`` (the final table's dict), ``scored``, ``score_max`` /
    ``score_mean``, ``win_strong``, ``weak``, ``span_tags``, ``labels``, ``pool``, ``cfg``, ``NC``."""
    if tag_span is None and (min_span_tag is not None or return_span_tags):
        raise ValueError("min_span_tag / return_span_tags need tag_span: the length of a span in seconds")
    if tag_span is not None and not float(tag_span) > 0:
        raise ValueError(f"tag_span must be > 0 seconds, got {tag_span!r}")
    if min_span_tag is not None and np.isnan(np.asarray(min_span_tag, dtype=np.float64)).any():
        raise ValueError("min_span_tag: NaN keeps no event; pass None to keep all")
    if not isinstance(long_set, LongRecordingSet):
        raise TypeError(f"long_set must be a LongRecordingSet, got {type(long_set).__name__}")
    cfg = cfg or _Cfg
    labels = getattr(getattr(decoder_or_labels, "__self__", None), "labels", None)
    if labels is None:
        if callable(decoder_or_labels):
            raise ValueError("decoder_or_labels: a decode_strong bound to an object with .labels, or a list of labels")
        labels = list(decoder_or_labels)
    pool = long_set.pooling_time_ratio if pooling_time_ratio is None else int(pooling_time_ratio)
    if pool != long_set.pooling_time_ratio:
        raise ValueError(f"pooling_time_ratio {pool} against a set built with {long_set.pooling_time_ratio}")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.SedError("get_long_predictions needs the model on the GPU (no CPU fallback)")
    NC = len(labels)
    thr = _per_class(threshold, NC, np.float32, "threshold")
    win = _per_class(cfg.median_window if median_window is None else median_window, NC, np.int32, "median_window")
    if threshold_high is not None:
        hysteresis_points([thr], [threshold_high], [win], NC)                    # (ValueError before any forward)
    process = min_event_length is not None or min_event_gap is not None
    if process:
        _order_code(process_order)
        min_len, max_gap = process_points(None if min_event_length is None else [min_event_length],
                                          None if min_event_gap is None else [min_event_gap], NC,
                                          pool * cfg.hop_length / cfg.sample_rate, 1)
    _score_key_code(score_key)
    if not isinstance(event_scores, (bool, np.bool_)):
        raise ValueError(f"event_scores must be True or False, got {event_scores!r}")
    scored = bool(event_scores) or min_event_score is not None
    if min_event_score is not None:
        min_score = _per_class(min_event_score, NC, np.float32, "min_event_score").reshape(1, NC)
        if np.isnan(min_score).any():
            raise ValueError("min_event_score: NaN keeps no event; pass None to keep all")
    if not isinstance(return_span_tags, (bool, np.bool_)):
        raise ValueError(f"return_span_tags must be True or False, got {return_span_tags!r}")
    if tag_span is not None:
        span3 = tag_span_frames(tag_span, pool * cfg.hop_length / cfg.sample_rate)
        if min_span_tag is not None:
            min_tag = _per_class(min_span_tag, NC, np.float32, "min_span_tag").reshape(1, NC)
            if np.isnan(min_tag).any():
                raise ValueError("min_span_tag: NaN keeps no event; pass None to keep all")
    if known_tags is not None:
        if min_span_tag is not None:
            raise ValueError("known_tags and min_span_tag are two gates: pass one of them")
        known = known_tags.detach().cpu().numpy() if torch.is_tensor(known_tags) else np.asarray(known_tags)
        if known.shape != (long_set.n_rec, NC) or not np.isin(known, (0, 1)).all():
            raise ValueError(f"known_tags must be [{long_set.n_rec}, {NC}] of 0 / 1, got shape {known.shape}")
    want_timeline = return_posteriors or scored
    want_att = return_weak or tag_span is not None
    win_strong = long_window_posteriors(model, long_set, NC, batch_size, want_attention=want_att)
    if want_att:
        win_strong, win_att = win_strong
    if threshold_high is None:
        out = stitch_decode(win_strong, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3, thr, win,
                            weighting, long_set.capacity(NC), want_timeline=want_timeline)
        calls = [("sed_stitch_decode", out["err"])]
    else:
        out = stitch_hysteresis(win_strong, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3, [thr],
                                [threshold_high], [win], weighting, long_set.capacity(NC), want_timeline=want_timeline)
        calls = [("sed_stitch_sweep + sed_events_hysteresis", out["err"])]
    if tag_span is not None:
        span_tags = stitch_span_tags(win_strong, win_att, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames,
                                     long_set.hop3, span3, weighting, rec_frame0_host=long_set.rec_frame0_host)
        if min_span_tag is not None:                                             # mask, then post-process
            out = gate_decoded(out, span_tags, long_set.n_rec, NC, min_tag)
            calls = [(calls[0][0] + " + sed_events_tag_scores + sed_events_select (min_span_tag)", out["err"])]
    if known_tags is not None:                                                   # the same gate on given tags: one span each
        given = {"tags": torch.from_numpy(np.ascontiguousarray(known, dtype=np.float32)).to(dev),
                 "rec_span0": torch.arange(long_set.n_rec + 1, dtype=torch.int64, device=dev),
                 "span3": int(np.diff(long_set.rec_frame0_host).max())}
        out = gate_decoded(out, given, long_set.n_rec, NC, 0.5)
        calls = [(calls[0][0] + " + sed_events_tag_scores + sed_events_select (known_tags)", out["err"])]
    if process:
        out = process_decoded(out, long_set.n_rec, NC, min_len, max_gap, process_order)
        calls = [(calls[0][0] + " + sed_events_process", out["err"])]
    if scored:                                                                   # words of their own: the table's stays as it was
        score_max, score_mean, word = events_scores(out, out["timeline"], long_set.rec_frame0, long_set.n_rec, NC)
        calls.append(("sed_events_scores", word))
        if min_event_score is not None:
            ev_ptr, ev_pairs, score_max, score_mean, word = events_select(out["ev_ptr"], out["ev_pairs"], score_max, score_mean,
                                                                          long_set.n_rec, NC, min_score, score_key)
            out = dict(out, ev_ptr=ev_ptr, ev_pairs=ev_pairs)
            calls.append(("sed_events_select (min_event_score)", word))
    if return_weak:
        tags = stitch_weak(win_strong, win_att, long_set.rec_win0, long_set.rec_frame0, long_set.total_frames, long_set.hop3,
                           weighting)
        calls.append(("sed_stitch_weak", tags["err"]))
    if tag_span is not None:
        calls.append(("sed_stitch_span_tags", span_tags["err"]))
    for what, word in calls:
        err = int(word.item())
        if err:
            raise _lib.SedError(stitch_error_text(what, err))
    return {"out": out, "scored": scored, "score_max": score_max if scored else None, "score_mean": score_mean if scored else None,
            "win_strong": win_strong, "weak": tags["weak"] if return_weak else None,
            "span_tags": span_tags if tag_span is not None else None, "labels": labels, "pool": pool, "cfg": cfg, "NC": NC}


PSEUDO_LABEL_KWARGS = ("pooling_time_ratio", "batch_size", "cfg", "threshold", "median_window", "weighting", "threshold_high",
                       "tag_span", "min_span_tag", "min_event_length", "min_event_gap", "process_order", "min_event_score",
                       "score_key", "known_tags")


def pseudo_label(model, long_set, target_set, items, labels, soft=None, combine="replace", **decode_kwargs):
    """One self-training stage on the device: the recordings of ``long_set`` are inferred with ``model`` (the EMA teacher, as a
    rule), decoded, gated and cleaned exactly as ``get_long_predictions`` does with the same arguments, and the final table is
    written as strong labels into ``target_set`` (a ``WindowedFeatureSet`` or a ``ResidentFeatureSet`` holding targets):
    recording r becomes the labels of its pool item ``items[r]``, in place (``relabel``) - no DataFrame, no label upload, the
    set is not rebuilt.  ``labels``: the class labels (or a bound ``decode_strong``).  ``soft``: None (hard 0 / 1 labels),
    ``"max"`` or ``"mean"`` (every event carries that score of the blended timeline); ``combine``: ``"replace"`` or ``"max"``
    (keep given labels and add the pseudo events).  ``decode_kwargs`` are ``get_long_predictions``' own (``PSEUDO_LABEL_KWARGS``:
    threshold, median_window, weighting, threshold_high, tag_span / min_span_tag, min_event_length / min_event_gap /
    process_order, min_event_score / score_key, batch_size, cfg, pooling_time_ratio), and ``known_tags`` [n_rec, nclass] (a
    tensor or array of 0 / 1): the tags a weakly labelled recording is KNOWN to hold replace pooled tags in the gate, one span
    per recording - an event of a class the recording does not hold is dropped (``gate_decoded`` with these tags and a minimum
    of 0.5, right after the decode like the tag gate; not together with ``min_span_tag``).  ``relabel``'s refusals (items,
    lengths, classes) are raised before any forward; the chain's error words are checked once before the pool is touched, the
    rasterise's own word after it.  Returns a dict: ``events_per_class`` [n_rec, nclass] int64 (one host copy of the counts)
    and ``table``, the device dict of ``get_long_predictions(return_table=True)``."""
    unknown = sorted(set(decode_kwargs) - set(PSEUDO_LABEL_KWARGS))
    if unknown:
        raise TypeError(f"pseudo_label: unexpected arguments {unknown} (it takes {list(PSEUDO_LABEL_KWARGS)})")
    if soft is not None:
        _score_key_code(soft)
    _combine_code(combine)
    if not isinstance(long_set, LongRecordingSet):
        raise TypeError(f"long_set must be a LongRecordingSet, got {type(long_set).__name__}")
    if not hasattr(target_set, "relabel"):
        raise TypeError(f"target_set must be a set with a label pool (relabel), got {type(target_set).__name__}")
    kw = dict(pooling_time_ratio=None, batch_size=64, cfg=None, threshold=0.5, median_window=None, weighting="taper",
              threshold_high=None, min_event_length=None, min_event_gap=None, process_order="drop_merge", min_event_score=None,
              score_key="max", tag_span=None, min_span_tag=None, known_tags=None)
    kw.update(decode_kwargs)
    n_labels = len(getattr(getattr(labels, "__self__", None), "labels", None) or ([] if callable(labels) else list(labels)))
    target_set.check_relabel(items, long_set.rec_frame0_host, n_labels)          # (before any forward)
    s = _long_events(model, long_set, labels, return_posteriors=False, return_weak=False, event_scores=soft is not None,
                     return_span_tags=False, **kw)
    table = _final_table(s)
    err = target_set.relabel(items, table, long_set.rec_frame0_host, nclass=s["NC"],
                             values=None if soft is None else table["score_" + soft], combine=combine)
    counts = (table["ev_ptr"][1:] - table["ev_ptr"][:-1]).cpu().numpy().reshape(long_set.n_rec, s["NC"])
    word = int(err.item())
    if word:
        raise _lib.SedError("sed_events_rasterize reported err " + ", ".join(f"bit {b} ({t})" for b, t in RASTER_ERR_BITS.items()
                                                                              if word & b) + f" (err = {word}): the labels of "
                            "the items named are invalid")
    return {"events_per_class": counts, "table": table}
