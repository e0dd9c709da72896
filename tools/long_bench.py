"""What inference on recordings longer than one clip costs: inference.get_long_predictions (overlapping windows, blended
posteriors, ONE decode of the whole timeline) against the only route there was before it - the same recordings cut on the
host into disjoint `frames`-long clips, through ResidentFeatureSet.for_eval + get_predictions.  The cut-into-clips leg
produces a DIFFERENT event table (events are split at every cut and each piece is median-filtered with reflected edges): the
comparison is of cost, not of results.

Synthetic linear-mel recordings at the baseline geometry (frames = 628, 64 mel bands, 10 classes, pooling 8, batch 64):
  "1h"        one recording of 360 x 628 frames
  "100x3min"  100 recordings of 18 x 628 frames
Per workload, in ONE run, the legs alternate for --rounds rounds (default 5) after a warm-up round:
  clips        get_predictions on the for_eval set of the disjoint clips
  long_T3      get_long_predictions at hop3 = T3 (no overlap: the same number of forwards up to the padding of the last window)
  long_default get_long_predictions at the default hop (about half a window: about twice the windows)
each timed with a host clock around the call (it ends with the host copy of the event table, so it is synchronised); reported
are the median and the spread (max - min) / median of every leg.  The sets are built before the timed calls (build times are
reported once).  sed_stitch_decode alone: its four launches bracketed by a device-event pair on preallocated buffers, warm,
median of --decode-reps (default 30) single calls, for either hop.

The clips leg needs nothing this tool's commit added, so the tool also runs on a tree without the long path (it then reports
that leg only).

--scoring measures what scoring the long path's event table on the device adds (profiles/long_scoring.json), on the same two
workloads at the default hop, legs alternated in the same way:
  predictions       get_long_predictions (inference the user already pays; ends with the host copy of the event table)
  validate_1        metrics.validate_long at one operating point (forward, decode, sed_long_event_counts, one host copy)
  validate_50_psds  validate_long at 50 thresholds with a PSDSCounts, by its default route (profiles/long_scoring.json was
                    recorded with the per-point loop: 50 decodes, 50 + 50 scoring calls; the sweep legs below time both routes)
and metrics.long_event_counts / long_psds_counts alone on a decoded table (device-event pair around each call, median of
--decode-reps).  The references are the decoded events of the first operating point, jittered (dropped with p = 0.15, both
ends moved by up to 0.3 s, sorted by onset).  The thresholds are per-class quantiles of the blended posteriors: the lowest of
0.5 / 0.75 / 0.9 at which no cluster of the scored columns exceeds 64 events per side (the largest cluster is reported; the
50 points run from that quantile up to 0.99).  There is no earlier route to compare against: the clip scorer raises on these
columns.

--scoring also measures the K-point sweep (profiles/long_sweep.json; --sweep measures these legs alone), on the same two
workloads at the same 50 thresholds with PSDS:
  validate_long(one_blend=True) against validate_long(one_blend=False) - the per-point loop, the only route before the sweep -
    alternated in one run, --rounds rounds, medians; the results of the two routes are compared (they are integers).  One
    blend counts as faster only where the difference of the medians exceeds the larger of the two legs' (max - min).
  sed_stitch_sweep alone at K = 50 against 50 calls of sed_stitch_decode, and the two sweep scorers alone at K = 50 against 50
    calls of the one-point scorers: a device-event pair around the call(s), median of --decode-reps, same run.
  The library's point-group size (sed_stitch_sweep_point_group) is recorded; --sweep-decode-only measures sed_stitch_sweep alone
  (a variant build with another group size, SED_LIB), and --candidates FILE,... copies such runs into the result.

--weak measures the recording-level weak tags (profiles/long_weak.json), on the same two workloads at the default hop:
  predictions against predictions_with_weak - get_long_predictions without and with return_weak=True, alternated in one run,
    --rounds rounds, medians: what the tags add to inference already paid for (the attention of every batch, one
    sed_stitch_weak).  The addition counts as measured only where it exceeds the larger of the two legs' (max - min).
  sed_stitch_weak alone (the C call on preallocated buffers) against the only route that can be assembled from the parts
    there were before it - two stitch_decode(want_timeline=True) blends, of the posteriors and of the attention, and a torch
    fp64 segmented reduction (torch.segment_reduce) of their product -, a device-event pair around the call(s), median of --decode-reps, same run;
    the fused call counts as faster only where the difference of the medians exceeds the larger (max - min) of the two.
  sed_crnn_attention alone on the context of one forward of a full batch, the same way.

--tag-train measures training on recording-level tags (profiles/long_tag_train.json), same workloads and hop:
  sed_stitch_weak_backward alone, and the forward + backward pair, against a torch-autograd restatement of the blend (index_add_)
  and the fp64 pooling - the only route to the gradient before it - with the largest difference of the two routes' gradients;
  on 100x3min one train.train_recording_tags epoch against the same batches with a window-level loss, alternated.

--span-tag-train measures training on span-level tags (profiles/long_span_tag_train.json), same workloads and hop, tag_span 10 s:
  sed_stitch_span_tags_backward alone, and the forward + backward pair, against a torch-autograd restatement of the blend
    (index_add_) and a per-span fp64 segment_reduce - the only route to the gradient before it - with the largest difference of
    the two routes' gradients;
  the same call at one span per recording beside sed_stitch_weak_backward on the same sums (and whether their bytes are equal);
  on 100x3min one train.train_span_tags epoch against train.train_recording_tags over the same batches, alternated.

--span-pieces measures span-tag training of a recording longer than one forward (profiles/long_span_pieces.json), the 1 h
workload, tag_span 10 s, max_windows 64, every target known:
  one train.train_span_tags(split_long=True) epoch - the recording trained in pieces - against the only earlier route: the
    recording cut on the host at span boundaries into recordings of at most 64 windows (another set, another blend at every
    cut) and today's train.train_span_tags over those; the two legs alternated in one run, --rounds rounds, medians,
    spread = (max - min) / median; a difference counts only where it exceeds the larger (max - min) of the two legs.
  sed_stitch_piece_span_tags and its backward alone beside sed_stitch_span_tags and its backward on the same tables (the whole
    recording as one piece with off = 0), a device-event pair around the call, median of --decode-reps, and whether the bytes
    are equal.

--error-rate measures the overall error rate with substitutions (the "long" key of profiles/error_rate.json), same workloads,
references and hop as --scoring:
  validate_long(..., error_rate=True) against the same run's validate_long(...) at one operating point and at 50, the two legs
    alternated in one run, --rounds rounds, medians, spread = (max - min) / median; the difference counts only where it lies
    outside the larger (max - min) of its two legs.
  sed_long_error_counts beside sed_long_event_counts on one decoded table and sed_long_sweep_error_counts beside
    sed_long_sweep_event_counts on the K = 50 table: a device-event pair around the Python call, median of --decode-reps.
  The operating points start at the first of --scoring's 50 thresholds from which no cluster of a recording's events of ALL
  classes merged exceeds 64 per side; the largest merged cluster met is reported.

--hysteresis measures the two-threshold decode (profiles/long_hysteresis.json), same workloads, references, hop and 50 low
thresholds as --scoring; the high threshold of a pair lies halfway between its low one and the 0.99 quantile:
  validate_long(thresholds_high=...) at the 50 pairs against the same run's validate_long at the 50 low thresholds, the two legs
    alternated in one run, --rounds rounds, medians, spread = (max - min) / median: what hysteresis adds to work already paid
    for; the difference counts only where it lies outside the larger (max - min) of its two legs.
  sed_events_hysteresis alone on the table of one 100-point sweep (a device-event pair around the Python call, median of
    --decode-reps) against the only route there was before it: both tables copied to the host, a vectorised numpy select,
    the result uploaded again (host clock, same reps); the two routes' tables are compared.

--process measures minimum event length and gap merging (profiles/long_process.json), same workloads, references, hop and 50
thresholds as --scoring, min_event_length 0.25 s and min_event_gap 0.15 s at every point, order "drop_merge":
  validate_long(min_event_lengths=..., min_event_gaps=...) against the same run's validate_long without them, the two legs
    alternated in one run, --rounds rounds, medians, spread = (max - min) / median; the difference counts only where it lies
    outside the larger (max - min) of its two legs.
  sed_events_process alone on the table of one 50-point sweep (a device-event pair around the Python call, median of
    --decode-reps) against the only route there was before it: the table copied to the host, a vectorised numpy restatement,
    the result uploaded again (host clock, same reps); the two routes' tables are compared.

--scores measures the event scores and the select by score (profiles/long_scores.json), same workloads, hop and 50 thresholds as
--scoring, median window 7:
  get_long_predictions(event_scores=True) against the same run's plain call, the two legs alternated in one run, --rounds
    rounds, medians, spread = (max - min) / median; the difference counts only where it lies outside the larger (max - min)
    of its two legs.
  sed_events_scores alone on the table of one 50-point sweep (a device-event pair around the Python call, median of
    --decode-reps) against the only route there was before it: timeline and table copied to the host, np.maximum.reduceat /
    np.add.reduceat, the result uploaded again (host clock, same reps); the run asserts identical maxima and every mean
    within one fp32 step.
  sed_events_select alone (the maximum against the next point's thresholds) against a host boolean-mask select, compared.
  --boundary-libs A.so,B.so: the scorer alone on the same table under builds of the library with other short / long
    boundaries (-DEVS_SHORT_FRAMES=n for csrc/evscore.hip), each in a process of its own.

--rasterize measures the pseudo strong labels (profiles/long_rasterize.json), same workloads, hop and 50 thresholds:
  sed_events_rasterize alone on point 0 of the 50-point sweep table, the points given per class (a device-event pair around the
    Python call, median of --decode-reps), against the only earlier route: the table copied to the host, a vectorised numpy
    rasterise (difference array + cumsum) and an upload into the pool; the run asserts that the two routes' rows are identical.
  pseudo_label into a WindowedFeatureSet over the same recordings against the same run's get_long_predictions with the same
    arguments, alternated, --rounds rounds; a difference counts only outside the larger (max - min) of the two legs.

Usage: python tools/long_bench.py [--scoring | --sweep | --weak | --tag-train | --span-tag-train | --span-pieces | --error-rate | --hysteresis | --process | --scores | --span-tags | --rasterize] [--rounds 5] [--decode-reps 30] [--out profiles/long_inference.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench                                                    # noqa: E402  (build_models)
from dcase2019_task4_amd import _lib, inference  # noqa: E402
from dcase2019_task4_amd.features import Scaler  # noqa: E402
from dcase2019_task4_amd.resident import ResidentFeatureSet  # noqa: E402

T, N_MELS, NCLASS, POOL, BATCH = 628, 64, 10, 8, 64
WORKLOADS = {"1h": (1, 360), "100x3min": (100, 18)}            # recordings, clips of T frames per recording
HAVE_LONG = hasattr(inference, "get_long_predictions")


class _Clips:
    """DataLoadDf-like: what ResidentFeatureSet.for_eval reads."""

    def __init__(self, clips, names):
        self.clips, self.filenames = clips, pd.Series(names)

    def __len__(self):
        return len(self.clips)

    def get_sample(self, i):
        return self.clips[i], None


class _Enc:
    labels = [f"class_{i}" for i in range(NCLASS)]

    def decode_strong(self, m):
        raise RuntimeError("the device decode is used")


def recordings(n_rec, clips_per_rec, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random((clips_per_rec * T, N_MELS), dtype=np.float32) * 3.0 for _ in range(n_rec)]


def scaler_of(rec):
    from oracle import features_np
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(rec[k * T:(k + 1) * T], T) for k in range(min(16, len(rec) // T))])
    return sc


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return {"median_ms": med, "spread": float((v.max() - v.min()) / med), "samples_ms": [float(x) for x in v]}


def alternate_legs(legs, rounds):
    """One warm-up call of every leg, then the legs alternated for ``rounds`` rounds under the host clock: {leg: stats}."""
    for fn in legs.values():
        fn()
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            ms[leg].append(wall_ms(fn))
    return {leg: stats(ms[leg]) for leg in legs}


def addition(out, key, a, b):
    """What leg ``b`` adds to leg ``a`` (their ``stats``), written to ``out``: the difference of the medians as ``key``, the
    larger (max - min) of the two legs, and whether the difference exceeds it."""
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    out[key] = b["median_ms"] - a["median_ms"]
    out["larger_max_minus_min_ms"] = band
    out["addition_exceeds_spread"] = bool(out[key] > band)


def decode_alone(model, ls, reps):
    """The four launches of sed_stitch_decode on the set's real window posteriors, one device-event pair per call."""
    _, _, win_strong = inference.get_long_predictions(model, ls, _Enc.labels, batch_size=BATCH, return_posteriors=True)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    total, n_rec, cap = ls.total_frames, ls.n_rec, ls.capacity(NCLASS)
    thr = torch.full((NCLASS,), 0.5, device=dev)
    win = torch.full((NCLASS,), 5, dtype=torch.int32, device=dev)
    timeline = torch.empty(total, NCLASS, device=dev)
    ev_ptr = torch.empty(n_rec * NCLASS + 1, dtype=torch.int64, device=dev)
    ev_pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(l.sed_stitch_decode_ws_bytes(total, n_rec, NCLASS), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(l.sed_stitch_decode(ptr(win_strong), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, ls.T3, NCLASS, ls.hop3, 1,
                                       ptr(thr), ptr(win), ptr(timeline), None, ptr(ev_ptr), ptr(ev_pairs), cap, ptr(ws),
                                       ws.numel(), ptr(err), _lib.stream_ptr()), "sed_stitch_decode")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert int(err.item()) == 0
    s = stats(ms)
    return {"median_ms": s["median_ms"], "spread": s["spread"], "reps": reps, "timeline_frames": total, "windows": ls.n_clips,
            "events": int(ev_ptr[-1].item())}


def workload(name, model, rounds, reps):
    n_rec, per = WORKLOADS[name]
    recs = recordings(n_rec, per)
    sc = scaler_of(recs[0])
    names = [f"{name}_{r}.wav" for r in range(n_rec)]
    out = {"recordings": n_rec, "feature_frames_each": per * T, "seconds_each": per * T * 255 / 16000.0}
    t0 = time.perf_counter()
    clips = _Clips([rec[k * T:(k + 1) * T] for rec in recs for k in range(per)],
                   [f"{n}#{k}" for n in names for k in range(per)])
    cs = ResidentFeatureSet.for_eval(clips, T, scaler=sc)
    torch.cuda.synchronize()
    out["clips_set_build_ms"] = (time.perf_counter() - t0) * 1e3
    enc = _Enc().decode_strong
    legs = {"clips": lambda: inference.get_predictions(model, cs, enc, POOL, batch_size=BATCH)}
    rows = {}
    if HAVE_LONG:
        sets = {}
        for leg, hop in (("long_T3", (T // POOL) * POOL), ("long_default", None)):
            t0 = time.perf_counter()
            sets[leg] = inference.LongRecordingSet.from_arrays(recs, T, hop_frames=hop, scaler=sc, filenames=names)
            torch.cuda.synchronize()
            out[leg + "_set_build_ms"] = (time.perf_counter() - t0) * 1e3
            out[leg + "_windows"] = sets[leg].n_clips
            legs[leg] = (lambda s: lambda: inference.get_long_predictions(model, s, enc, POOL, batch_size=BATCH))(sets[leg])
    out["clips_forwarded"] = len(clips)
    for leg, fn in legs.items():                                 # warm-up round: every shape, every code object
        rows[leg] = len(fn())
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            ms[leg].append(wall_ms(fn))
    for leg in legs:
        out[leg] = dict(stats(ms[leg]), event_rows=rows[leg])
    if HAVE_LONG:
        for leg in ("long_T3", "long_default"):
            out[leg]["ratio_to_clips"] = out[leg]["median_ms"] / out["clips"]["median_ms"]
            out[leg]["stitch_decode_alone"] = decode_alone(model, sets[leg], reps)
        out["long_default"]["window_ratio_to_long_T3"] = out["long_default_windows"] / out["long_T3_windows"]
        out["long_default"]["ratio_to_long_T3"] = out["long_default"]["median_ms"] / out["long_T3"]["median_ms"]
    return out


def _columns(ev_ptr, on, off):
    return [(on[a:b], off[a:b]) for a, b in zip(ev_ptr[:-1], ev_ptr[1:])]


def largest_cluster(ref_on, est_on, t_collar=0.2):
    """(reference, estimated) events of the largest cluster of one column (include/dcase_sed.h: runs between valid cuts)."""
    on = np.r_[ref_on, est_on]
    side = np.r_[np.zeros(len(ref_on), np.int8), np.ones(len(est_on), np.int8)]
    if len(on) == 0:
        return 0, 0
    order = np.argsort(on, kind="stable")
    on, side = on[order], side[order]
    last = [np.maximum.accumulate(np.where(side == k, on, -np.inf)) for k in (0, 1)]
    nxt = [np.r_[np.minimum.accumulate(np.where(side == k, on, np.inf)[::-1])[::-1][1:], np.inf] for k in (0, 1)]
    cut = (last[0] + t_collar < nxt[1]) & (last[1] + t_collar < nxt[0])
    cluster = np.r_[0, np.cumsum(cut)[:-1]]
    n = cluster[-1] + 1
    return int(np.bincount(cluster[side == 0], minlength=n).max()), int(np.bincount(cluster[side == 1], minlength=n).max())


def scoring_workload(name, model, rounds, reps, setup_only=False):
    from dcase2019_task4_amd import metrics
    n_rec, per = WORKLOADS[name]
    recs = recordings(n_rec, per)
    sc = scaler_of(recs[0])
    names = [f"{name}_{r}.wav" for r in range(n_rec)]
    labels = _Enc.labels
    ls = inference.LongRecordingSet.from_arrays(recs, T, scaler=sc, filenames=names)
    win_strong = inference.long_window_posteriors(model, ls, NCLASS, BATCH)
    den = inference._Cfg.sample_rate / inference._Cfg.hop_length
    window = 7
    rs = np.random.RandomState(0)

    def decode(thr):
        return inference.stitch_decode(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thr, window, "taper",
                                       ls.capacity(NCLASS))
    timeline = decode(0.5)["timeline"]
    chosen = None
    for q in (0.5, 0.75, 0.9):
        thr = torch.quantile(timeline[:: max(1, timeline.shape[0] // 100000)], q, dim=0).cpu().numpy().astype(np.float32)
        out = decode(thr)
        assert int(out["err"].item()) == 0
        ev_ptr = out["ev_ptr"].cpu().numpy()
        ev = out["ev_pairs"][:int(ev_ptr[-1])].cpu().numpy().astype(np.int64)
        est = _columns(ev_ptr, ev[:, 0] * POOL / den, ev[:, 1] * POOL / den)
        ref = []
        for on, off in est:                                          # jittered references, sorted by onset
            keep = rs.uniform(size=len(on)) >= 0.15
            a = np.maximum(0.0, on[keep] + rs.uniform(-0.3, 0.3, keep.sum()))
            b = off[keep] + rs.uniform(-0.3, 0.3, keep.sum())
            a, b = np.minimum(a, b).clip(min=0.0), np.maximum(a, b)
            o = np.lexsort((b, a))
            ref.append((a[o], b[o]))
        sizes = [largest_cluster(r[0], e[0]) for r, e in zip(ref, est)]
        biggest = (max(s[0] for s in sizes), max(s[1] for s in sizes))
        if max(biggest) <= 64:
            chosen = q
            break
    if chosen is None:
        raise SystemExit(f"{name}: clusters beyond 64 events per side at every threshold tried ({biggest})")
    ref_ptr = np.r_[0, np.cumsum([len(r[0]) for r in ref])]
    ref_ev = metrics.RefEvents(ref_ptr, np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref]), names, labels)
    hi = torch.quantile(timeline[:: max(1, timeline.shape[0] // 100000)], 0.99, dim=0).cpu().numpy().astype(np.float32)
    thr50 = [thr + (hi - thr) * k / 49.0 for k in range(50)]
    out_info = {"recordings": n_rec, "windows": ls.n_clips, "timeline_frames": ls.total_frames, "threshold_quantile": chosen,
                "median_window": window, "estimated_events": int(ev_ptr[-1]), "reference_events": int(ref_ptr[-1]),
                "longest_column": {"estimated": int(np.diff(ev_ptr).max()), "reference": int(np.diff(ref_ptr).max())},
                "largest_cluster": {"reference": biggest[0], "estimated": biggest[1]}}
    ctx = {"ls": ls, "win_strong": win_strong, "ref_ev": ref_ev, "thr50": thr50, "window": window}
    if setup_only:                                                   # (--sweep-decode-only: the inputs, nothing timed here)
        return out_info, ctx
    state = {}

    def validate_50():
        psds = metrics.PSDSCounts(50, NCLASS, "cuda")
        state["v50"] = metrics.validate_long(model, ls, ref_ev, thr50, [window], batch_size=BATCH, psds=psds)
        state["psds"] = psds.host()
    legs = {"predictions": lambda: inference.get_long_predictions(model, ls, labels, POOL, batch_size=BATCH, threshold=thr,
                                                                  median_window=window),
            "validate_1": lambda: state.__setitem__("v1", metrics.validate_long(model, ls, ref_ev, [thr], [window],
                                                                                 batch_size=BATCH)),
            "validate_50_psds": validate_50}
    for leg, fn in list(legs.items()):
        try:
            fn()
        except _lib.SedError as e:                                    # e.g. a cluster beyond 64 at one of the 50 points
            out_info[leg] = {"error": str(e)}
            del legs[leg]
    out_info["event_f_overall_point_0"] = state["v1"][0][0].results_overall_metrics()["f_measure"]["f_measure"]
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            ms[leg].append(wall_ms(fn))
    for leg in legs:
        out_info[leg] = stats(ms[leg])
    for leg in ("validate_1", "validate_50_psds"):
        if leg not in legs:
            continue
        out_info[leg]["ratio_to_predictions"] = out_info[leg]["median_ms"] / out_info["predictions"]["median_ms"]
        out_info[leg]["added_ms"] = out_info[leg]["median_ms"] - out_info["predictions"]["median_ms"]
    decoded = decode(thr)
    alone = {"sed_long_event_counts": lambda: metrics.long_event_counts(decoded, ref_ev, POOL),
             "sed_long_psds_counts": lambda: metrics.long_psds_counts(decoded, ref_ev, POOL)}
    for what, call in alone.items():
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c = call()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        c.host()                                                     # raises when the error word is set
        st = stats(t)
        out_info[what + "_alone"] = {"median_ms": st["median_ms"], "spread": st["spread"], "reps": reps}
    return out_info, ctx


def event_ms(call, reps):
    """Median and spread of `reps` single device-event pairs around call(), after 5 warm calls."""
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    st = stats(t)
    return {"median_ms": st["median_ms"], "spread": st["spread"], "reps": reps}


def sweep_decode_alone(ctx, reps):
    """sed_stitch_sweep at K = 50 and 50 calls of sed_stitch_decode, the C calls on preallocated buffers."""
    ls, win_strong = ctx["ls"], ctx["win_strong"]
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    K, total, n_rec, cap = len(ctx["thr50"]), ls.total_frames, ls.n_rec, ls.capacity(NCLASS)
    thr = torch.from_numpy(np.stack(ctx["thr50"]).astype(np.float32)).to(dev)
    win = torch.full((K, NCLASS), ctx["window"], dtype=torch.int32, device=dev)
    ev_ptr = torch.empty(K * n_rec * NCLASS + 1, dtype=torch.int64, device=dev)
    ev_pairs = torch.empty(K * cap, 2, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(l.sed_stitch_sweep_ws_bytes(total, n_rec, NCLASS, K), dtype=torch.uint8, device=dev)
    ws1 = torch.empty(l.sed_stitch_decode_ws_bytes(total, n_rec, NCLASS), dtype=torch.uint8, device=dev)

    def sweep():
        _lib.check(l.sed_stitch_sweep(ptr(win_strong), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, ls.T3, NCLASS, ls.hop3, 1, K,
                                      ptr(thr), ptr(win), None, ptr(ev_ptr), ptr(ev_pairs), K * cap, ptr(ws), ws.numel(),
                                      ptr(err), _lib.stream_ptr()), "sed_stitch_sweep")

    def loop():
        for k in range(K):
            _lib.check(l.sed_stitch_decode(ptr(win_strong), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, ls.T3, NCLASS, ls.hop3,
                                           1, ptr(thr[k]), ptr(win[k]), None, None, ptr(ev_ptr), ptr(ev_pairs), cap, ptr(ws1),
                                           ws1.numel(), ptr(err), _lib.stream_ptr()), "sed_stitch_decode")
    out = {"point_group": int(l.sed_stitch_sweep_point_group()), "n_points": K, "sed_stitch_sweep": event_ms(sweep, reps)}
    events = int(ev_ptr[-1].item())
    out["events_all_points"] = events
    out["sed_stitch_decode_x50"] = event_ms(loop, reps)
    assert int(err.item()) == 0
    return out


def sweep_workload(name, ctx, model, rounds, reps, decode_only):
    from dcase2019_task4_amd import metrics
    ls, ref_ev, thr50, window = ctx["ls"], ctx["ref_ev"], ctx["thr50"], ctx["window"]
    out = sweep_decode_alone(ctx, reps)
    if decode_only:
        return out
    K = len(thr50)
    state = {}

    def validate(one_blend):
        def fn():
            psds = metrics.PSDSCounts(K, NCLASS, "cuda")
            res = metrics.validate_long(model, ls, ref_ev, thr50, [window], batch_size=BATCH, psds=psds, one_blend=one_blend)
            state[one_blend] = ([(e.class_wise, s.class_wise, s.Ntn) for e, s in res], psds.host().tobytes())
        return fn
    legs = {"validate_50_psds_loop": validate(False), "validate_50_psds_one_blend": validate(True)}
    for fn in legs.values():
        fn()
    out["routes_identical"] = state[True] == state[False]
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            ms[leg].append(wall_ms(fn))
    for leg in legs:
        out[leg] = stats(ms[leg])
    a, b = out["validate_50_psds_loop"], out["validate_50_psds_one_blend"]
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    out["one_blend_minus_loop_ms"] = b["median_ms"] - a["median_ms"]
    out["larger_max_minus_min_ms"] = band
    out["one_blend_faster"] = bool(a["median_ms"] - b["median_ms"] > band)
    # the scorers alone: the sweep table at K = 50 against 50 one-point tables (Python calls: workspace allocation + 4 launches)
    cap = ls.capacity(NCLASS)
    sweep_tab = inference.stitch_sweep(ctx["win_strong"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thr50, [window],
                                       "taper", K * cap)
    tabs = [inference.stitch_decode(ctx["win_strong"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, t, window, "taper",
                                    cap, want_timeline=False) for t in thr50]
    ec, pc = metrics.Counts(K, NCLASS, "cuda"), metrics.PSDSCounts(K, NCLASS, "cuda")

    def loop(fn):
        def call():
            for k, tab in enumerate(tabs):
                fn(tab, ref_ev, POOL, counts=ec if fn is metrics.long_event_counts else pc, point=k)
        return call
    out["sed_long_sweep_event_counts"] = event_ms(lambda: metrics.long_sweep_event_counts(sweep_tab, ref_ev, POOL, counts=ec), reps)
    out["sed_long_event_counts_x50"] = event_ms(loop(metrics.long_event_counts), reps)
    out["sed_long_sweep_psds_counts"] = event_ms(lambda: metrics.long_sweep_psds_counts(sweep_tab, ref_ev, POOL, counts=pc), reps)
    out["sed_long_psds_counts_x50"] = event_ms(loop(metrics.long_psds_counts), reps)
    ec.host(), pc.host()                                              # raise when an error word is set
    return out


def largest_merged_cluster(table, ref_ev, n_rec, K, den):
    """(reference, estimated) events of the largest cluster over all (point, recording) of a decoded table when the events of
    ALL classes are merged by onset - what bounds sed_long_error_counts (64 per side)."""
    ev_ptr = table["ev_ptr"].cpu().numpy()
    on = table["ev_pairs"][:int(ev_ptr[-1]), 0].cpu().numpy().astype(np.int64) * POOL / den
    ref_ptr = ref_ev.ptr_host.astype(np.int64)
    best = (0, 0)
    for k in range(K):
        for r in range(n_rec):
            a, b = ev_ptr[(k * n_rec + r) * NCLASS], ev_ptr[(k * n_rec + r + 1) * NCLASS]
            ra, rb = ref_ptr[r * NCLASS], ref_ptr[(r + 1) * NCLASS]
            s = largest_cluster(np.sort(ref_ev.onset_host[ra:rb]), np.sort(on[a:b]))
            best = (max(best[0], s[0]), max(best[1], s[1]))
    return best


def error_rate_workload(name, model, rounds, reps):
    """validate_long(..., error_rate=True) against the same run's validate_long(...) at one operating point and at 50, the two
    legs alternated; the three long entry points alone beside the class-wise ones.  The operating points start at the lowest
    of the scoring workload's 50 thresholds from which no MERGED cluster exceeds 64 events per side."""
    from dcase2019_task4_amd import metrics
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, ref_ev, window, win_strong = ctx["ls"], ctx["ref_ev"], ctx["window"], ctx["win_strong"]
    n_rec, cap = ls.n_rec, ls.capacity(NCLASS)
    den = inference._Cfg.sample_rate / inference._Cfg.hop_length

    def sweep_table(thrs):
        return inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thrs, [window], "taper",
                                      len(thrs) * cap)

    def one_table(thr):
        return inference.stitch_decode(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thr, window, "taper", cap,
                                       want_timeline=False)
    first = None
    for k, thr in enumerate(ctx["thr50"]):
        biggest = largest_merged_cluster(one_table(thr), ref_ev, n_rec, 1, den)
        if max(biggest) <= 64:
            first = k
            break
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window", "reference_events")}
    out["rounds"] = rounds
    if first is None:
        out["error"] = f"merged clusters beyond 64 events per side at every threshold tried (the last: {biggest})"
        return out
    lo, hi = ctx["thr50"][first], ctx["thr50"][-1]
    thr50 = [lo + (hi - lo) * k / 49.0 for k in range(50)]
    tab1, tab50 = one_table(lo), sweep_table(thr50)
    out["first_threshold_index_of_the_scoring_workload"] = first
    out["largest_merged_cluster"] = {"1_point": dict(zip(("reference", "estimated"), largest_merged_cluster(tab1, ref_ev, n_rec, 1, den))),
                                     "50_points": dict(zip(("reference", "estimated"),
                                                           largest_merged_cluster(tab50, ref_ev, n_rec, 50, den)))}
    out["estimated_events"] = {"1_point": int(tab1["ev_ptr"][-1].item()), "50_points": int(tab50["ev_ptr"][-1].item())}
    state = {}
    for what, thrs in (("1_point", [lo]), ("50_points", thr50)):
        def run(error_rate, thrs=thrs, what=what):
            def fn():
                state[what, error_rate] = metrics.validate_long(model, ls, ref_ev, thrs, [window], batch_size=BATCH,
                                                                error_rate=error_rate)
            return fn
        legs = {"validate_long": run(False), "validate_long_error_rate": run(True)}
        try:
            for fn in legs.values():
                fn()
        except _lib.SedError as e:                                    # e.g. a merged cluster beyond 64 at one of the points
            out[what] = {"error": str(e)}
            continue
        ms = {leg: [] for leg in legs}
        for _ in range(rounds):
            for leg, fn in legs.items():
                ms[leg].append(wall_ms(fn))
        t = {leg: stats(ms[leg]) for leg in legs}
        a, b = t["validate_long"], t["validate_long_error_rate"]
        band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
        t["difference"] = {"added_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                           "outside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) > band)}
        same = all(p[0].class_wise == q[0].class_wise and p[1].class_wise == q[1].class_wise
                   for p, q in zip(state[what, False], state[what, True]))
        t["class_wise_counts_identical"] = bool(same)
        e, s = state[what, True][0]
        t["overall_error_rate_point_0"] = {"event_based": e.results_overall_metrics()["error_rate"],
                                           "segment_based": s.results_overall_metrics()["error_rate"]}
        out[what] = t
    ec1, er1 = metrics.Counts(1, NCLASS, "cuda"), metrics.ErrorCounts(1, NCLASS, "cuda")
    ec50, er50 = metrics.Counts(50, NCLASS, "cuda"), metrics.ErrorCounts(50, NCLASS, "cuda")
    alone = {"sed_long_event_counts": lambda: metrics.long_event_counts(tab1, ref_ev, POOL, counts=ec1),
             "sed_long_error_counts": lambda: metrics.long_error_counts(tab1, ref_ev, POOL, counts=er1),
             "sed_long_sweep_event_counts": lambda: metrics.long_sweep_event_counts(tab50, ref_ev, POOL, counts=ec50),
             "sed_long_sweep_error_counts": lambda: metrics.long_sweep_error_counts(tab50, ref_ev, POOL, counts=er50)}
    out["alone"] = {what: event_ms(call, reps) for what, call in alone.items()}
    for c in (ec1, er1, ec50, er50):
        try:
            c.host()                                                  # raises when the error word is set
        except _lib.SedError as e:
            out["alone"]["error"] = str(e)
    return out


def host_select(ev_ptr, pairs, n_cols):
    """The two-threshold select on the host, vectorised: the table of 2 x n_cols columns [lo | hi] as numpy arrays ->
    (out_ptr, out_pairs).  One searchsorted over (column, onset) keys: the first high onset >= the low onset, in the same
    column and in front of the low offset."""
    n_lo, n_all = int(ev_ptr[n_cols]), int(ev_ptr[2 * n_cols])
    col = np.repeat(np.arange(2 * n_cols, dtype=np.int64), np.diff(ev_ptr))
    key = (col % n_cols) << 32
    lo_on, lo_off, hi_on = key[:n_lo] + pairs[:n_lo, 0], key[:n_lo] + pairs[:n_lo, 1], key[n_lo:n_all] + pairs[n_lo:n_all, 0]
    j = np.searchsorted(hi_on, lo_on, side="left")
    keep = (j < len(hi_on)) & (np.r_[hi_on, 0][j] < lo_off)
    out_ptr = np.r_[0, np.cumsum(keep)][ev_ptr[:n_cols + 1]]
    return out_ptr.astype(np.int64), pairs[:n_lo][keep]


def hysteresis_workload(name, model, rounds, reps):
    """(a) validate_long at 50 threshold pairs against the same run's validate_long at the same 50 low thresholds, alternated;
    (b) sed_events_hysteresis alone on the 100-point table against the host route (both tables copied down, the numpy select,
    the result uploaded).  The high threshold of a pair lies halfway between its low one and the workload's 0.99 quantile."""
    from dcase2019_task4_amd import metrics
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, ref_ev, window, win_strong = ctx["ls"], ctx["ref_ev"], ctx["window"], ctx["win_strong"]
    lo50 = ctx["thr50"]
    hi50 = [t + 0.5 * (lo50[-1] - t) for t in lo50]
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window", "reference_events")}
    out.update(rounds=rounds, pairs=50)
    state = {}
    legs = {"validate_long_50": lambda: state.__setitem__("plain", metrics.validate_long(model, ls, ref_ev, lo50, [window],
                                                                                          batch_size=BATCH)),
            "validate_long_50_hysteresis": lambda: state.__setitem__("hyst", metrics.validate_long(
                model, ls, ref_ev, lo50, [window], batch_size=BATCH, thresholds_high=hi50))}
    t = alternate_legs(legs, rounds)
    a, b = t["validate_long_50"], t["validate_long_50_hysteresis"]
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    t["difference"] = {"added_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                       "outside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) > band)}
    t["estimated_events_point_0"] = {what: int(sum(v["Nsys"] for v in state[what][0][0].class_wise.values()))
                                     for what in ("plain", "hyst")}
    out["validate_long"] = t
    # (b) the select alone, on the table of one sweep of 100 points [lo_0 .. lo_49, hi_0 .. hi_49]
    cap, n_cols = ls.capacity(NCLASS), 50 * ls.n_rec * NCLASS
    table = inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, lo50 + hi50, [window], "taper",
                                   100 * cap)
    assert int(table["err"].item()) == 0
    ev_ptr, pairs = table["ev_ptr"], table["ev_pairs"]
    lo_ptr, hi_ptr = ev_ptr[:n_cols + 1], ev_ptr[n_cols:]

    def device():
        state["dev"] = inference.events_hysteresis(lo_ptr, hi_ptr, pairs, 50 * cap)

    def host():
        p = ev_ptr.cpu().numpy()
        q = pairs[:int(p[-1])].cpu().numpy()
        out_ptr, out_pairs = host_select(p, q, n_cols)
        state["host"] = (torch.from_numpy(out_ptr).cuda(), torch.from_numpy(np.ascontiguousarray(out_pairs)).cuda())
    for _ in range(3):
        host()
    host_ms = stats([wall_ms(host) for _ in range(reps)])
    out["select_alone"] = {"sed_events_hysteresis": event_ms(device, reps),
                           "host_copy_numpy_select_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"],
                                                             "reps": reps, "timing": "host clock around the synchronised route"}}
    d_ptr, d_pairs, d_err = state["dev"]
    h_ptr, h_pairs = state["host"]
    n = int(h_ptr[-1].item())
    out["select_alone"].update(low_events=int(ev_ptr[n_cols].item()), high_events=int((ev_ptr[-1] - ev_ptr[n_cols]).item()),
                               kept_events=n, err=int(d_err.item()),
                               routes_identical=bool(torch.equal(d_ptr, h_ptr) and torch.equal(d_pairs[:n], h_pairs)))
    return out


def host_process(ev_ptr, pairs, n_rec, NC, min_len, max_gap):
    """Minimum length, then gap merging (order 0) on the host, vectorised over the whole flat table: numpy arrays ->
    (out_ptr, out_pairs)."""
    n_cols = len(ev_ptr) - 1
    col = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(ev_ptr))
    par = (col // (n_rec * NC)) * NC + col % NC
    on, off = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    m = min_len.reshape(-1).astype(np.int64)[par]
    keep = (m <= 0) | (off - on >= m)
    on, off, col = on[keep], off[keep], col[keep]
    g = max_gap.reshape(-1).astype(np.int64)[par[keep]]
    head = np.ones(len(on), dtype=bool)
    head[1:] = (col[1:] != col[:-1]) | (on[1:] - off[:-1] > g[1:])
    tail = np.r_[head[1:], True] if len(on) else head
    out_ptr = np.r_[0, np.cumsum(np.bincount(col[head], minlength=n_cols))].astype(np.int64)
    return out_ptr, np.stack([on[head], off[tail]], 1).astype(np.int32)


def process_workload(name, model, rounds, reps, seconds=(0.25, 0.15), order="drop_merge"):
    """(a) validate_long at 50 thresholds with a minimum event length and gap against the same run's validate_long without
    them, alternated; (b) sed_events_process alone on the 50-point table against the host route (the table copied down, the
    numpy restatement, the result uploaded)."""
    from dcase2019_task4_amd import metrics
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, ref_ev, window, win_strong, thr50 = ctx["ls"], ctx["ref_ev"], ctx["window"], ctx["win_strong"], ctx["thr50"]
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window", "reference_events")}
    frame_seconds = ls.pooling_time_ratio * inference._Cfg.hop_length / inference._Cfg.sample_rate
    min_len, max_gap = inference.process_points([seconds[0]], [seconds[1]], NCLASS, frame_seconds, 50)
    out.update(rounds=rounds, points=50, min_event_length_s=seconds[0], min_event_gap_s=seconds[1], order=order,
               min_len_frames=int(min_len[0, 0]), max_gap_frames=int(max_gap[0, 0]))
    state = {}
    legs = {"validate_long_50": lambda: state.__setitem__("plain", metrics.validate_long(model, ls, ref_ev, thr50, [window],
                                                                                          batch_size=BATCH)),
            "validate_long_50_process": lambda: state.__setitem__("proc", metrics.validate_long(
                model, ls, ref_ev, thr50, [window], batch_size=BATCH, min_event_lengths=[seconds[0]], min_event_gaps=[seconds[1]],
                process_order=order))}
    t = alternate_legs(legs, rounds)
    a, b = t["validate_long_50"], t["validate_long_50_process"]
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    t["difference"] = {"added_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                       "outside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) > band)}
    t["estimated_events_point_0"] = {what: int(sum(v["Nsys"] for v in state[what][0][0].class_wise.values()))
                                     for what in ("plain", "proc")}
    out["validate_long"] = t
    # (b) the call alone, on the table of one sweep of the 50 points
    cap = ls.capacity(NCLASS)
    table = inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thr50, [window], "taper", 50 * cap)
    assert int(table["err"].item()) == 0
    ev_ptr, pairs = table["ev_ptr"], table["ev_pairs"]
    d_len, d_gap = torch.from_numpy(min_len).cuda(), torch.from_numpy(max_gap).cuda()

    def device():
        state["dev"] = inference.events_process(ev_ptr, pairs, ls.n_rec, NCLASS, d_len, d_gap, order)

    def host():
        p = ev_ptr.cpu().numpy()
        q = pairs[:int(p[-1])].cpu().numpy()
        out_ptr, out_pairs = host_process(p, q, ls.n_rec, NCLASS, min_len, max_gap)
        state["host"] = (torch.from_numpy(out_ptr).cuda(), torch.from_numpy(np.ascontiguousarray(out_pairs)).cuda())
    for _ in range(3):
        host()
    host_ms = stats([wall_ms(host) for _ in range(reps)])
    out["process_alone"] = {"sed_events_process": event_ms(device, reps),
                            "host_copy_numpy_process_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"],
                                                               "reps": reps, "timing": "host clock around the synchronised route"}}
    d_ptr, d_pairs, d_err = state["dev"]
    h_ptr, h_pairs = state["host"]
    n = int(h_ptr[-1].item())
    out["process_alone"].update(pairs_capacity=int(pairs.shape[0]), input_events=int(ev_ptr[-1].item()), result_events=n,
                                err=int(d_err.item()),
                                routes_identical=bool(torch.equal(d_ptr, h_ptr) and torch.equal(d_pairs[:n], h_pairs)))
    return out


def host_scores(tl, f0, n_rec, NC, ev_ptr, pairs):
    """Maximum and mean per event on the host with reduceat over the class-major timeline: numpy arrays -> (max, mean) fp32."""
    total = tl.shape[0]
    col = np.repeat(np.arange(len(ev_ptr) - 1, dtype=np.int64), np.diff(ev_ptr))
    base = (col % NC) * total + f0[(col // NC) % n_rec]
    idx = np.stack([base + pairs[:, 0], base + pairs[:, 1]], 1).reshape(-1)
    x = np.r_[np.ascontiguousarray(tl.T).reshape(-1), np.float32(0)]                  # (an end index may be the array's length)
    if len(idx) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    smax = np.maximum.reduceat(x, idx)[::2]
    ssum = np.add.reduceat(x.astype(np.float64), idx)[::2]
    return smax, (ssum / (pairs[:, 1] - pairs[:, 0])).astype(np.float32)


def host_score_select(ev_ptr, pairs, smax, smean, n_rec, NC, mins):
    """The select by a boolean mask on the host: numpy arrays -> (out_ptr, out_pairs, out_max, out_mean)."""
    n_cols = len(ev_ptr) - 1
    col = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(ev_ptr))
    keep = smax > mins.reshape(-1)[(col // (n_rec * NC)) * NC + col % NC]
    out_ptr = np.r_[0, np.cumsum(np.bincount(col[keep], minlength=n_cols))].astype(np.int64)
    return out_ptr, pairs[keep], smax[keep], smean[keep]


def scores_alone(timeline, rec_frame0, n_rec, ev_ptr, pairs, reps):
    """sed_events_scores through its Python front, device events around the call."""
    state = {}

    def device():
        state["dev"] = inference.events_scores((ev_ptr, pairs), timeline, rec_frame0, n_rec, NCLASS)
    t = event_ms(device, reps)
    t["short_frames"] = int(_lib.lib().sed_events_scores_short_frames())
    return t, state["dev"]


def scores_child(path, reps):
    """Part (d) in a process of its own (another library through SED_LIB): the table and timeline the parent saved."""
    z = np.load(path)
    dev = lambda a: torch.from_numpy(a).cuda()
    t, (smax, smean, err) = scores_alone(dev(z["timeline"]), dev(z["rec_frame0"]), int(z["n_rec"]), dev(z["ev_ptr"]), dev(z["ev_pairs"]),
                                         reps)
    n = int(z["ev_ptr"][-1])
    t.update(err=int(err.item()), maxima_identical=bool(np.array_equal(smax[:n].cpu().numpy(), z["score_max"])),
             means_identical=bool(np.array_equal(smean[:n].cpu().numpy(), z["score_mean"])))
    print(json.dumps(t), flush=True)


def scores_workload(name, model, rounds, reps, boundary_libs):
    """(a) get_long_predictions with and without event_scores=True, alternated; (b) sed_events_scores alone on the 50-point
    sweep table against the host route (timeline and table copied down, numpy reduceat, the result uploaded); (c)
    sed_events_select alone against a host boolean-mask select; (d) part (b)'s device leg under the other short / long
    boundaries given as libraries."""
    import subprocess
    import tempfile
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, window, win_strong, thr50 = ctx["ls"], ctx["window"], ctx["win_strong"], ctx["thr50"]
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window")}
    out.update(rounds=rounds, points=50)
    enc = _Enc().decode_strong
    state = {}
    legs = {"get_long_predictions": lambda: state.__setitem__("plain", inference.get_long_predictions(
                model, ls, enc, POOL, batch_size=BATCH, median_window=window)),
            "get_long_predictions_event_scores": lambda: state.__setitem__("scored", inference.get_long_predictions(
                model, ls, enc, POOL, batch_size=BATCH, median_window=window, event_scores=True))}
    t = alternate_legs(legs, rounds)
    a, b = t["get_long_predictions"], t["get_long_predictions_event_scores"]
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    t["difference"] = {"added_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                       "outside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) > band)}
    t["event_rows"] = len(state["plain"])
    assert state["scored"][list(state["plain"].columns)].equals(state["plain"])
    out["get_long_predictions"] = t
    # (b) the scorer alone, on the table of one sweep of the 50 points
    cap = ls.capacity(NCLASS)
    table = inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, thr50, [window], "taper", 50 * cap,
                                   want_timeline=True)
    assert int(table["err"].item()) == 0
    ev_ptr, pairs, timeline = table["ev_ptr"], table["ev_pairs"], table["timeline"]
    f0_host = np.asarray(ls.rec_frame0_host, dtype=np.int64)

    def host():
        p = ev_ptr.cpu().numpy()
        q = pairs[:int(p[-1])].cpu().numpy().astype(np.int64)
        smax, smean = host_scores(timeline.cpu().numpy(), f0_host, ls.n_rec, NCLASS, p, q)
        state["host"] = (torch.from_numpy(smax).cuda(), torch.from_numpy(smean).cuda())
    for _ in range(3):
        host()
    host_ms = stats([wall_ms(host) for _ in range(reps)])
    dev_t, (d_max, d_mean, d_err) = scores_alone(timeline, ls.rec_frame0, ls.n_rec, ev_ptr, pairs, reps)
    n = int(ev_ptr[-1].item())
    h_max, h_mean = (x.cpu().numpy() for x in state["host"])
    g_max, g_mean = d_max[:n].cpu().numpy(), d_mean[:n].cpu().numpy()
    assert not np.isnan(h_max).any() and int(d_err.item()) == 0
    assert np.array_equal(g_max, h_max), "the maxima of the two routes differ"
    steps = np.abs(g_mean.astype(np.float64) - h_mean.astype(np.float64)) / np.spacing(h_mean)
    assert (steps <= 1).all(), "a mean of the two routes differs by more than one fp32 step"
    lengths = (pairs[:n, 1] - pairs[:n, 0]).cpu().numpy()
    out["scores_alone"] = {"sed_events_scores": dev_t,
                           "host_copy_numpy_reduceat_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"],
                                                               "reps": reps, "timing": "host clock around the synchronised route"},
                           "pairs_capacity": int(pairs.shape[0]), "events": n, "err": int(d_err.item()),
                           "event_frames": {"median": float(np.median(lengths)), "max": int(lengths.max()),
                                            "longer_than_short_frames": int((lengths > dev_t["short_frames"]).sum())},
                           "maxima_identical": True, "means_within_one_fp32_step": True,
                           "means_differing_by_one_step": int((steps > 0).sum())}
    # (c) the select alone: the maximum against the next point's threshold
    mins = np.stack(thr50[1:] + thr50[-1:]).astype(np.float32)
    d_mins = torch.from_numpy(mins).cuda()

    def device_select():
        state["sel"] = inference.events_select(ev_ptr, pairs, d_max, d_mean, ls.n_rec, NCLASS, d_mins)

    def host_select_route():
        p = ev_ptr.cpu().numpy()
        m = int(p[-1])
        res = host_score_select(p, pairs[:m].cpu().numpy(), d_max[:m].cpu().numpy(), d_mean[:m].cpu().numpy(), ls.n_rec, NCLASS, mins)
        state["host_sel"] = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in res]
    for _ in range(3):
        host_select_route()
    host_ms = stats([wall_ms(host_select_route) for _ in range(reps)])
    sel_t = event_ms(device_select, reps)
    s_ptr, s_pairs, s_max, s_mean, s_err = state["sel"]
    h = state["host_sel"]
    m = int(h[0][-1].item())
    out["select_alone"] = {"sed_events_select": sel_t,
                           "host_copy_numpy_mask_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"], "reps": reps,
                                                           "timing": "host clock around the synchronised route"},
                           "input_events": n, "kept_events": m, "err": int(s_err.item()),
                           "routes_identical": bool(torch.equal(s_ptr, h[0]) and torch.equal(s_pairs[:m], h[1]) and
                                                    torch.equal(s_max[:m], h[2]) and torch.equal(s_mean[:m], h[3]))}
    assert out["select_alone"]["routes_identical"]
    # (d) the other short / long boundaries, each library in a process of its own on the same table
    tried = {str(dev_t["short_frames"]): dict(dev_t, library="the build under test")}
    if boundary_libs:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "table.npz")
            np.savez(path, timeline=timeline.cpu().numpy(), rec_frame0=f0_host, n_rec=ls.n_rec, ev_ptr=ev_ptr.cpu().numpy(),
                     ev_pairs=pairs.cpu().numpy(), score_max=g_max, score_mean=g_mean)
            for lib in boundary_libs:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--scores-child", path, "--decode-reps", str(reps)],
                                   env=dict(os.environ, SED_LIB=os.path.abspath(lib), SED_ALLOW_VARIANT="1"), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"--scores-child under {lib} failed:\n{r.stdout}\n{r.stderr}")
                res = json.loads(r.stdout.strip().splitlines()[-1])
                assert res["err"] == 0 and res["maxima_identical"], res
                tried[str(res["short_frames"])] = res
    out["short_frames_tried"] = tried
    return out


def host_tag_gate(ev_ptr, pairs, tags, rec_span0, span3, n_rec, NC, mins):
    """The tag gate on the host: reduceat of the class-major tags over the events' span ranges, then a boolean mask: numpy arrays
    -> (out_ptr, out_pairs, kept tag scores)."""
    n_cols, total = len(ev_ptr) - 1, tags.shape[0]
    col = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(ev_ptr))
    base = (col % NC) * total + rec_span0[(col // NC) % n_rec]
    lo, hi = pairs[:, 0].astype(np.int64) // span3, (pairs[:, 1].astype(np.int64) - 1) // span3 + 1
    idx = np.stack([base + lo, base + hi], 1).reshape(-1)
    x = np.r_[np.ascontiguousarray(tags.T).reshape(-1), np.float32(0)]                # (an end index may be the array's length)
    score = np.maximum.reduceat(x, idx)[::2] if len(idx) else np.zeros(0, np.float32)
    keep = score > mins.reshape(-1)[(col // (n_rec * NC)) * NC + col % NC]
    out_ptr = np.r_[0, np.cumsum(np.bincount(col[keep], minlength=n_cols))].astype(np.int64)
    return out_ptr, pairs[keep], score[keep]


def span_tags_workload(name, model, rounds, reps, tag_span=10.0, min_tag=0.5):
    """--span-tags: (a) get_long_predictions(tag_span=10 s, min_span_tag=0.5) against the same run's plain call; (b) validate_long
    with the gate at 50 points against the same run's call without it; (c) sed_stitch_span_tags alone at span3 = T3, 1 and one
    span per recording against two stitch_decode(want_timeline=True) blends and a torch fp64 segment_reduce over the spans; (d)
    sed_events_tag_scores + sed_events_select alone on the 50-point table against the host route (tables and tags copied
    down, reduceat on the coarsened pairs, a boolean mask, upload)."""
    from dcase2019_task4_amd import metrics
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, ref_ev, window, win_strong, thr50 = ctx["ls"], ctx["ref_ev"], ctx["window"], ctx["win_strong"], ctx["thr50"]
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window", "reference_events")}
    frame_seconds = ls.pooling_time_ratio * inference._Cfg.hop_length / inference._Cfg.sample_rate
    span3 = inference.tag_span_frames(tag_span, frame_seconds)
    out.update(rounds=rounds, points=50, tag_span_s=tag_span, span3=span3, T3=ls.T3, hop3=ls.hop3, min_span_tag=min_tag)
    labels, state = _Enc.labels, {}

    def alternate(legs):
        t = alternate_legs(legs, rounds)
        a, b = (t[leg] for leg in legs)
        band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
        t["difference"] = {"added_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                           "outside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) > band)}
        return t
    out["get_long_predictions"] = alternate({
        "predictions": lambda: state.__setitem__("plain_df", inference.get_long_predictions(model, ls, labels, POOL, batch_size=BATCH)),
        "predictions_gated": lambda: state.__setitem__("gated_df", inference.get_long_predictions(
            model, ls, labels, POOL, batch_size=BATCH, tag_span=tag_span, min_span_tag=min_tag))})
    out["get_long_predictions"]["events"] = {"plain": len(state["plain_df"]), "gated": len(state["gated_df"])}
    out["validate_long"] = alternate({
        "validate_long_50": lambda: state.__setitem__("plain", metrics.validate_long(model, ls, ref_ev, thr50, [window], batch_size=BATCH)),
        "validate_long_50_gated": lambda: state.__setitem__("gated", metrics.validate_long(
            model, ls, ref_ev, thr50, [window], batch_size=BATCH, tag_span=tag_span, min_span_tags=[min_tag]))})
    out["validate_long"]["estimated_events_point_0"] = {what: int(sum(v["Nsys"] for v in state[what][0][0].class_wise.values()))
                                                        for what in ("plain", "gated")}
    # (c) the span tags alone
    _, win_att = inference.long_window_posteriors(model, ls, NCLASS, BATCH, want_attention=True)
    dev, total = win_strong.device, ls.total_frames
    thr = torch.full((NCLASS,), 0.5, device=dev)
    win = torch.full((NCLASS,), 1, dtype=torch.int32, device=dev)
    lengths_host = np.diff(ls.rec_frame0_host)
    out["span_tags_alone"] = {}
    for what, s3 in (("span3_T3", ls.T3), ("span3_1", 1), ("whole_recording", int(lengths_host.max()))):
        host, _, total_spans, s3 = inference.span_table(lengths_host, s3)
        span_len = torch.from_numpy(np.concatenate([np.minimum(s3, L - np.arange(0, L, s3)) for L in lengths_host])).to(dev)

        def fused(s3=s3):
            state["tags"] = inference.stitch_span_tags(win_strong, win_att, ls.rec_win0, ls.rec_frame0, total, ls.hop3, s3,
                                                       rec_frame0_host=ls.rec_frame0_host)

        def composed(span_len=span_len):
            tl = [inference.stitch_decode(w, ls.rec_win0, ls.rec_frame0, total, ls.hop3, thr, win, "taper", ls.capacity(NCLASS),
                                          want_timeline=True)["timeline"].double() for w in (win_strong, win_att)]
            num = torch.segment_reduce(tl[0] * tl[1], "sum", lengths=span_len, axis=0, unsafe=True)
            den = torch.segment_reduce(tl[1], "sum", lengths=span_len, axis=0, unsafe=True)
            state["composed"] = (num / den).float()
        t = {"total_spans": total_spans, "span3": s3, "sed_stitch_span_tags": event_ms(fused, reps), "composed_route": event_ms(composed, reps)}
        assert int(state["tags"]["err"].item()) == 0
        t["max_abs_difference_of_the_two_routes"] = float((state["tags"]["tags"] - state["composed"]).abs().max().item())
        band = max(x["spread"] * x["median_ms"] for x in (t["sed_stitch_span_tags"], t["composed_route"]))
        t["composed_minus_fused_ms"] = t["composed_route"]["median_ms"] - t["sed_stitch_span_tags"]["median_ms"]
        t["larger_max_minus_min_ms"] = band
        t["outside_the_band"] = bool(abs(t["composed_minus_fused_ms"]) > band)
        out["span_tags_alone"][what] = t
    # (d) the gate alone, on the table of one sweep of the 50 points
    cap = ls.capacity(NCLASS)
    table = inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, total, ls.hop3, thr50, [window], "taper", 50 * cap)
    assert int(table["err"].item()) == 0
    span_tags = inference.stitch_span_tags(win_strong, win_att, ls.rec_win0, ls.rec_frame0, total, ls.hop3, span3,
                                           rec_frame0_host=ls.rec_frame0_host)
    mins = np.full((50, NCLASS), min_tag, np.float32)
    d_mins = torch.from_numpy(mins).cuda()

    def device():
        state["dev"] = inference.gate_decoded(table, span_tags, ls.n_rec, NCLASS, d_mins)

    def host():
        p = table["ev_ptr"].cpu().numpy()
        q = table["ev_pairs"][:int(p[-1])].cpu().numpy()
        out_ptr, out_pairs, kept = host_tag_gate(p, q, span_tags["tags"].cpu().numpy(), span_tags["rec_span0"].cpu().numpy(),
                                                 span_tags["span3"], ls.n_rec, NCLASS, mins)
        state["host"] = (torch.from_numpy(out_ptr).cuda(), torch.from_numpy(np.ascontiguousarray(out_pairs)).cuda())
    for _ in range(3):
        host()
    host_ms = stats([wall_ms(host) for _ in range(reps)])
    g = {"sed_events_tag_scores_plus_sed_events_select": event_ms(device, reps),
         "host_copy_reduceat_mask_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"], "reps": reps,
                                            "timing": "host clock around the synchronised route"}}
    h_ptr, h_pairs = state["host"]
    n = int(h_ptr[-1].item())
    identical = bool(torch.equal(state["dev"]["ev_ptr"], h_ptr) and torch.equal(state["dev"]["ev_pairs"][:n], h_pairs))
    assert identical, "the device gate and the host route disagree"
    g.update(pairs_capacity=int(table["ev_pairs"].shape[0]), input_events=int(table["ev_ptr"][-1].item()), result_events=n,
             err=int(state["dev"]["err"].item()), routes_identical=identical)
    out["gate_alone"] = g
    return out


def host_rasterize(ev_ptr, pairs, rec_frame0, n_rec, NC, total):
    """Point 0 of a table as label rows on the host: a difference array over the flat rows and a cumsum: numpy arrays ->
    [total, NC] float32 of 0 / 1."""
    n_cols = n_rec * NC
    p = ev_ptr[:n_cols + 1]
    q = pairs[int(p[0]):int(p[-1])].astype(np.int64)
    col = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(p))
    base, cls = rec_frame0[col // NC], col % NC
    d = np.zeros((total + 1, NC), np.int32)
    np.add.at(d, (base + q[:, 0], cls), 1)
    np.add.at(d, (base + q[:, 1], cls), -1)
    return (np.cumsum(d[:-1], axis=0) > 0).astype(np.float32)


def rasterize_workload(name, model, rounds, reps):
    """--rasterize: (a) sed_events_rasterize alone on point 0 of the 50-point table against the host route (table copied down,
    difference array + cumsum, upload into the pool), rows asserted identical; (b) pseudo_label into a WindowedFeatureSet over
    the same recordings against the same run's get_long_predictions with the same arguments, alternated."""
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    info, ctx = scoring_workload(name, model, rounds, reps, setup_only=True)
    ls, window, win_strong, thr50 = ctx["ls"], ctx["window"], ctx["win_strong"], ctx["thr50"]
    out = {k: info[k] for k in ("recordings", "windows", "timeline_frames", "median_window")}
    out.update(rounds=rounds, points=50, label_rows=ls.total_frames, nclass=NCLASS)
    total, n_rec, state = ls.total_frames, ls.n_rec, {}
    table = inference.stitch_sweep(win_strong, ls.rec_win0, ls.rec_frame0, total, ls.hop3, thr50, [window], "taper",
                                   50 * ls.capacity(NCLASS))
    assert int(table["err"].item()) == 0
    pool = torch.full((total, NCLASS), float("nan"), device=win_strong.device)
    point = torch.zeros(NCLASS, dtype=torch.int32, device=win_strong.device)        # one point per class: here all point 0

    def device():
        state["err"] = inference.events_rasterize(table, ls.rec_frame0, n_rec, NCLASS, dst=pool, point=point)[1]

    def host():
        p = table["ev_ptr"][:n_rec * NCLASS + 1].cpu().numpy()
        q = table["ev_pairs"][:int(p[-1])].cpu().numpy()
        state["host_pool"].copy_(torch.from_numpy(host_rasterize(p, q, ls.rec_frame0_host, n_rec, NCLASS, total)))
    state["host_pool"] = torch.full_like(pool, float("nan"))
    for _ in range(3):
        host()
    host_ms = stats([wall_ms(host) for _ in range(reps)])
    g = {"sed_events_rasterize": event_ms(device, reps),
         "host_copy_cumsum_upload": {"median_ms": host_ms["median_ms"], "spread": host_ms["spread"], "reps": reps,
                                     "timing": "host clock around the synchronised route"}}
    identical = bool(torch.equal(pool.view(torch.int32), state["host_pool"].view(torch.int32)))
    assert identical and int(state["err"].item()) == 0, "the device rasterise and the host route disagree"
    g.update(pairs_capacity=int(table["ev_pairs"].shape[0]), table_events=int(table["ev_ptr"][-1].item()),
             point_0_events=int(table["ev_ptr"][n_rec * NCLASS].item()), covered_elements=int(pool.sum().item()),
             routes_identical=identical)
    out["rasterize_alone"] = g
    # (b) pseudo_label against get_long_predictions, the same arguments
    recs = recordings(*WORKLOADS[name])
    L3s = np.diff(ls.rec_frame0_host)
    target = WindowedFeatureSet.from_arrays(recs, [np.zeros((int(L), NCLASS), np.float32) for L in L3s], (n_rec,), (1,), T, [True],
                                            scaler=scaler_of(recs[0]), augment_type=None)
    items, labels = list(range(n_rec)), _Enc.labels
    kw = dict(pooling_time_ratio=POOL, batch_size=BATCH, threshold=thr50[0], median_window=window)
    legs = {"get_long_predictions": lambda: state.__setitem__("df", inference.get_long_predictions(model, ls, labels, **kw)),
            "pseudo_label": lambda: state.__setitem__("pl", inference.pseudo_label(model, ls, target, items, labels, **kw))}
    t = alternate_legs(legs, rounds)
    a, b = t["get_long_predictions"], t["pseudo_label"]
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (a, b))
    t["difference"] = {"pseudo_label_minus_predictions_ms": b["median_ms"] - a["median_ms"], "larger_max_minus_min_ms": band,
                       "inside_the_band": bool(abs(b["median_ms"] - a["median_ms"]) <= band)}
    t["events"] = {"frame_rows": len(state["df"]), "pseudo_label": int(state["pl"]["events_per_class"].sum())}
    assert t["events"]["frame_rows"] == t["events"]["pseudo_label"]
    assert torch.equal(target.label_pool.view(torch.int32), pool.view(torch.int32)), "pseudo_label's rows are not point 0's"
    out["pseudo_label"] = t
    return out


def weak_workload(name, model, rounds, reps):
    import ctypes as C
    n_rec, per = WORKLOADS[name]
    recs = recordings(n_rec, per)
    sc = scaler_of(recs[0])
    names = [f"{name}_{r}.wav" for r in range(n_rec)]
    labels = _Enc.labels
    ls = inference.LongRecordingSet.from_arrays(recs, T, scaler=sc, filenames=names)
    out = {"recordings": n_rec, "windows": ls.n_clips, "timeline_frames": ls.total_frames, "hop3": ls.hop3, "T3": ls.T3}
    legs = {"predictions": lambda: inference.get_long_predictions(model, ls, labels, POOL, batch_size=BATCH),
            "predictions_with_weak": lambda: inference.get_long_predictions(model, ls, labels, POOL, batch_size=BATCH,
                                                                            return_weak=True)}
    out.update(alternate_legs(legs, rounds))
    addition(out, "weak_adds_ms", out["predictions"], out["predictions_with_weak"])
    # ---- sed_stitch_weak alone against the route composed of earlier parts ----------------------------------------------------
    win_strong, win_att = inference.long_window_posteriors(model, ls, NCLASS, BATCH, want_attention=True)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    total = ls.total_frames
    weak = torch.empty(n_rec, NCLASS, device=dev)
    sums = torch.empty(n_rec, NCLASS, 2, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(l.sed_stitch_weak_ws_bytes(total, n_rec, NCLASS), dtype=torch.uint8, device=dev)

    def fused():
        _lib.check(l.sed_stitch_weak(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, ls.T3, NCLASS,
                                     ls.hop3, 1, ptr(weak), ptr(sums), ptr(ws), ws.numel(), ptr(err), _lib.stream_ptr()),
                   "sed_stitch_weak")
    lengths = ls.rec_frame0[1:] - ls.rec_frame0[:-1]
    thr = torch.full((NCLASS,), 0.5, device=dev)
    win = torch.full((NCLASS,), 1, dtype=torch.int32, device=dev)
    state = {}

    def composed():
        tl = [inference.stitch_decode(w, ls.rec_win0, ls.rec_frame0, total, ls.hop3, thr, win, "taper", ls.capacity(NCLASS),
                                      want_timeline=True)["timeline"].double() for w in (win_strong, win_att)]
        num = torch.segment_reduce(tl[0] * tl[1], "sum", lengths=lengths, axis=0, unsafe=True)
        den = torch.segment_reduce(tl[1], "sum", lengths=lengths, axis=0, unsafe=True)
        state["weak"] = (num / den).float()
    out["sed_stitch_weak_alone"] = event_ms(fused, reps)
    out["composed_route"] = event_ms(composed, reps)
    assert int(err.item()) == 0
    out["max_abs_difference_of_the_two_routes"] = float((weak - state["weak"]).abs().max().item())
    band = max(x["spread"] * x["median_ms"] for x in (out["sed_stitch_weak_alone"], out["composed_route"]))
    out["composed_minus_fused_ms"] = out["composed_route"]["median_ms"] - out["sed_stitch_weak_alone"]["median_ms"]
    out["larger_max_minus_min_alone_ms"] = band
    out["fused_faster"] = bool(out["composed_minus_fused_ms"] > band)
    # ---- sed_crnn_attention alone, on the context of one full batch ------------------------------------------------------------
    with torch.no_grad():
        model(ls.eval_batch(0, min(BATCH, ls.n_clips)))
    cbuf, dims = model._last_ctx
    att = torch.empty(dims.B, dims.T // 8, dims.nclass, device=dev)
    out["sed_crnn_attention_alone"] = dict(event_ms(lambda: _lib.check(l.sed_crnn_attention(
        C.byref(dims), ptr(cbuf), cbuf.numel(), ptr(att), _lib.stream_ptr()), "sed_crnn_attention"), reps), batch=int(dims.B))
    return out


def tag_train_setup(name, model):
    """What --tag-train and --span-tag-train start from: the workload's set, the common ``out`` fields, the windows' posteriors
    and attention in eval mode, gradient buffers for both and an error word."""
    n_rec, per = WORKLOADS[name]
    recs = recordings(n_rec, per)
    sc = scaler_of(recs[0])
    ls = inference.LongRecordingSet.from_arrays(recs, T, scaler=sc, filenames=[f"{name}_{r}.wav" for r in range(n_rec)])
    out = {"recordings": n_rec, "windows": ls.n_clips, "timeline_frames": ls.total_frames, "hop3": ls.hop3, "T3": ls.T3}
    model.eval()
    win_strong, win_att = inference.long_window_posteriors(model, ls, NCLASS, BATCH, want_attention=True)
    err = torch.zeros(1, dtype=torch.int32, device=win_strong.device)
    return ls, out, win_strong, win_att, torch.empty_like(win_strong), torch.empty_like(win_att), err


def blend_tables(ls, dev):
    """The index tables of the blend's torch restatement: per (window, local frame) that lies inside its recording the timeline
    frame and the taper weight, the kept elements' flat indices, and the weight sum of every timeline frame."""
    T3, hop3 = ls.T3, ls.hop3
    rec_of_win = np.repeat(np.arange(ls.n_rec), np.diff(ls.rec_win0_host))
    j = np.arange(ls.n_clips) - ls.rec_win0_host[rec_of_win]
    v = np.arange(T3)
    u = j[:, None] * hop3 + v[None, :]
    ok = u < np.diff(ls.rec_frame0_host)[rec_of_win][:, None]
    frame = torch.from_numpy((ls.rec_frame0_host[rec_of_win][:, None] + u)[ok]).to(dev)
    wt = torch.from_numpy(np.broadcast_to(np.minimum(v + 1, T3 - v).astype(np.float32), u.shape)[ok]).to(dev)
    keep = torch.from_numpy(np.flatnonzero(ok.reshape(-1))).to(dev)
    return frame, wt, keep, torch.zeros(ls.total_frames, device=dev).index_add_(0, frame, wt)


def fused_against_composed(out, ls, win_strong, win_att, g, pool, fused_fwd, fused_bwd, bwd_key, d_s, d_a, err, reps):
    """The fused backward call alone (``out[bwd_key]``), and the forward + backward pair, against the torch-autograd restatement:
    the blend by index_add_ over ``blend_tables``, then ``pool(P, A) -> (num, den)``, the workload's own fp64 pooling of the two
    blended timelines into the rows ``g`` weighs.  Writes the four timings, the largest difference of the two routes' gradients
    (the fused ones are in ``d_s`` / ``d_a``) and, for either pair, the difference, the band and whether fused is faster."""
    dev, total = win_strong.device, ls.total_frames
    frame, wt, keep, wsum = blend_tables(ls, dev)
    state = {}

    def composed_fwd():
        ps, pa = win_strong.detach().requires_grad_(True), win_att.detach().requires_grad_(True)
        tl = [torch.zeros(total, NCLASS, device=dev).index_add_(0, frame, wt[:, None] * x.reshape(-1, NCLASS)[keep]) / wsum[:, None]
              for x in (ps, pa)]
        num, den = pool(tl[0].double(), tl[1].double())
        state["in"], state["loss"] = (ps, pa), (g * (num / den).float()).sum()

    def composed_bwd():
        state["grads"] = torch.autograd.grad(state["loss"], state["in"], retain_graph=True)

    def both(a, b):
        def call():
            a()
            b()
        return call
    fused_fwd()
    composed_fwd()
    out[bwd_key] = event_ms(fused_bwd, reps)
    out["composed_backward_alone"] = event_ms(composed_bwd, reps)
    out["fused_forward_plus_backward"] = event_ms(both(fused_fwd, fused_bwd), reps)
    out["composed_forward_plus_backward"] = event_ms(both(composed_fwd, composed_bwd), reps)
    assert int(err.item()) == 0
    out["max_abs_difference_of_the_two_routes"] = {"d_win_strong": float((d_s - state["grads"][0]).abs().max().item()),
                                                   "d_win_att": float((d_a - state["grads"][1]).abs().max().item()),
                                                   "largest_gradient": [float(x.abs().max().item()) for x in state["grads"]]}
    for a, b, key in ((bwd_key, "composed_backward_alone", "backward"),
                      ("fused_forward_plus_backward", "composed_forward_plus_backward", "forward_plus_backward")):
        band = max(x["spread"] * x["median_ms"] for x in (out[a], out[b]))
        out[key + "_composed_minus_fused_ms"] = out[b]["median_ms"] - out[a]["median_ms"]
        out[key + "_larger_max_minus_min_ms"] = band
        out[key + "_fused_faster"] = bool(out[key + "_composed_minus_fused_ms"] > band)


def tag_epoch_setup(out, ls, model):
    """The optimizer and the runs of the epoch legs, or None (said in ``out``) where a recording does not fit one forward."""
    from dcase2019_task4_amd import train
    if int(np.diff(ls.rec_win0_host).max()) > BATCH:
        out["epoch"] = "not measured: a recording has more windows than one forward holds (max_windows)"
        return None
    runs, _ = train.recording_tag_batches(np.diff(ls.rec_win0_host), BATCH, 0, 0)
    out["batches_per_epoch"], out["max_windows"] = len(runs), BATCH
    return torch.optim.Adam(model.parameters(), lr=1e-5), runs


def tag_train_workload(name, model, rounds, reps):
    """--tag-train: (a) sed_stitch_weak_backward alone against the torch-autograd restatement of blend + fp64 pooling, the only
    route to the gradient before it; (b) where every recording fits one forward (100x3min): one train_recording_tags epoch
    against the same batches' forward + backward + step with a plain window-level loss - what the pooled loss adds."""
    from dcase2019_task4_amd import train
    ls, out, win_strong, win_att, d_s, d_a, err = tag_train_setup(name, model)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    n_rec, total, T3, hop3 = ls.n_rec, ls.total_frames, ls.T3, ls.hop3
    g = torch.randn(n_rec, NCLASS, device=dev, generator=torch.Generator(dev).manual_seed(1))
    weak = torch.empty(n_rec, NCLASS, device=dev)
    sums = torch.empty(n_rec, NCLASS, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(l.sed_stitch_weak_ws_bytes(total, n_rec, NCLASS), dtype=torch.uint8, device=dev)

    def fused_fwd():
        _lib.check(l.sed_stitch_weak(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, T3, NCLASS, hop3, 1,
                                     ptr(weak), ptr(sums), ptr(ws), ws.numel(), ptr(err), _lib.stream_ptr()), "sed_stitch_weak")

    def fused_bwd():
        _lib.check(l.sed_stitch_weak_backward(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, T3, NCLASS,
                                              hop3, 1, ptr(sums), ptr(g), ptr(d_s), ptr(d_a), ptr(err), _lib.stream_ptr()),
                   "sed_stitch_weak_backward")
    rec_of_frame = torch.from_numpy(np.repeat(np.arange(n_rec), np.diff(ls.rec_frame0_host))).to(dev)

    def pool(P, A):
        return (torch.zeros(n_rec, NCLASS, dtype=torch.float64, device=dev).index_add_(0, rec_of_frame, P * A),
                torch.zeros(n_rec, NCLASS, dtype=torch.float64, device=dev).index_add_(0, rec_of_frame, A))
    fused_against_composed(out, ls, win_strong, win_att, g, pool, fused_fwd, fused_bwd, "sed_stitch_weak_backward_alone", d_s, d_a,
                           err, reps)
    del win_strong, win_att, d_s, d_a
    # ---- (b) an epoch on recording tags against the same epoch with a window-level loss ------------------------------------------
    epoch_setup = tag_epoch_setup(out, ls, model)
    if epoch_setup is None:
        return out
    opt, runs = epoch_setup
    tags = (np.random.default_rng(2).random((n_rec, NCLASS)) < 0.2).astype(np.float32)
    tags_dev = torch.from_numpy(tags).to(dev)
    epoch = [0]

    def pooled():
        train.train_recording_tags(ls, tags, model, opt, epoch[0], max_windows=BATCH)
        epoch[0] += 1

    def windowed():
        model.train()
        loss_sum = torch.zeros((), device=dev)
        for r0, r1 in runs:
            w0, w1 = int(ls.rec_win0_host[r0]), int(ls.rec_win0_host[r1])
            opt.zero_grad()
            _, wk = model(ls.eval_batch(w0, w1 - w0))
            target = tags_dev[r0:r1].repeat_interleave(ls.rec_win0[r0 + 1:r1 + 1] - ls.rec_win0[r0:r1], dim=0, output_size=w1 - w0)
            loss = torch.nn.functional.binary_cross_entropy(wk, target)
            loss.backward()
            opt.step()
            loss_sum += loss.detach()
        loss_sum.item()
    out.update(alternate_legs({"epoch_window_level_loss": windowed, "epoch_recording_tags": pooled}, rounds))
    addition(out, "pooled_loss_adds_ms", out["epoch_window_level_loss"], out["epoch_recording_tags"])
    return out


def span_tag_train_workload(name, model, rounds, reps, tag_span=10.0):
    """--span-tag-train: (a) sed_stitch_span_tags_backward alone, and forward + backward, at ``tag_span`` seconds against the
    torch-autograd restatement of the blend (index_add_) and a per-span fp64 segment_reduce - the only route to this gradient
    before it; (b) the same call at one span per recording beside sed_stitch_weak_backward on the same sums; (c) where every
    recording fits one forward (100x3min): one train_span_tags epoch against train_recording_tags over the same batches."""
    from dcase2019_task4_amd import train
    ls, out, win_strong, win_att, d_s, d_a, err = tag_train_setup(name, model)
    out["tag_span_s"] = tag_span
    cfg = inference._Cfg
    span3 = inference.tag_span_frames(tag_span, POOL * cfg.hop_length / cfg.sample_rate)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    n_rec, total, T3, hop3 = ls.n_rec, ls.total_frames, ls.T3, ls.hop3

    def span_calls(span3):
        """(forward, backward, state) of the two C calls at this span length, on buffers of their own."""
        host, span0, n_spans, span3 = inference.span_table(ls, span3)
        g = torch.randn(n_spans, NCLASS, device=dev, generator=torch.Generator(dev).manual_seed(1))
        tags = torch.empty(n_spans, NCLASS, device=dev)
        sums = torch.empty(n_spans, NCLASS, 2, dtype=torch.float64, device=dev)
        ws = torch.empty(l.sed_stitch_span_tags_ws_bytes(total, n_spans, n_rec, NCLASS, span3), dtype=torch.uint8, device=dev)

        def fwd():
            _lib.check(l.sed_stitch_span_tags(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), ptr(span0), total,
                                              n_spans, n_rec, T3, NCLASS, hop3, 1, span3, ptr(tags), ptr(sums), ptr(ws), ws.numel(),
                                              ptr(err), _lib.stream_ptr()), "sed_stitch_span_tags")

        def bwd():
            _lib.check(l.sed_stitch_span_tags_backward(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), ptr(span0),
                                                       n_spans, n_rec, T3, NCLASS, hop3, 1, span3, ptr(sums), ptr(g), ptr(d_s),
                                                       ptr(d_a), ptr(err), _lib.stream_ptr()), "sed_stitch_span_tags_backward")
        return fwd, bwd, {"host": host, "n_spans": n_spans, "span3": span3, "g": g, "sums": sums}
    fused_fwd, fused_bwd, sp = span_calls(span3)
    out["span3"], out["total_spans"] = sp["span3"], sp["n_spans"]
    L3s = np.diff(ls.rec_frame0_host)
    lengths = torch.from_numpy(np.concatenate([np.minimum(sp["span3"], L - np.arange(0, L, sp["span3"])) for L in L3s])).to(dev)
    assert lengths.numel() == sp["n_spans"] and int(lengths.sum().item()) == total

    def pool(P, A):
        return (torch.segment_reduce(P * A, "sum", lengths=lengths, axis=0, unsafe=True),
                torch.segment_reduce(A, "sum", lengths=lengths, axis=0, unsafe=True))
    fused_against_composed(out, ls, win_strong, win_att, sp["g"], pool, fused_fwd, fused_bwd, "sed_stitch_span_tags_backward_alone",
                           d_s, d_a, err, reps)
    # ---- (b) one span per recording, beside sed_stitch_weak_backward in the same run ---------------------------------------------
    one_fwd, one_bwd, one = span_calls(int(L3s.max()))
    assert one["n_spans"] == n_rec
    one_fwd()

    def weak_bwd():
        _lib.check(l.sed_stitch_weak_backward(ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, T3, NCLASS,
                                              hop3, 1, ptr(one["sums"]), ptr(one["g"]), ptr(d_s), ptr(d_a), ptr(err),
                                              _lib.stream_ptr()), "sed_stitch_weak_backward")
    one_bwd()
    span_bytes = (d_s.clone(), d_a.clone())
    weak_bwd()
    b = {"one_span_per_recording_equals_weak_backward_bitwise":
         bool(torch.equal(span_bytes[0].view(torch.int32), d_s.view(torch.int32))
              and torch.equal(span_bytes[1].view(torch.int32), d_a.view(torch.int32)))}
    legs = {"sed_stitch_span_tags_backward_alone": one_bwd, "sed_stitch_weak_backward_alone": weak_bwd}
    for leg, fn in legs.items():
        b[leg] = event_ms(fn, reps)
    band = max(x["spread"] * x["median_ms"] for x in (b[k] for k in legs))
    b["span_minus_weak_ms"] = b["sed_stitch_span_tags_backward_alone"]["median_ms"] - b["sed_stitch_weak_backward_alone"]["median_ms"]
    b["larger_max_minus_min_ms"] = band
    b["difference_exceeds_spread"] = bool(abs(b["span_minus_weak_ms"]) > band)
    out["one_span_per_recording"] = b
    assert int(err.item()) == 0
    del span_bytes, win_strong, win_att, d_s, d_a
    # ---- (c) an epoch on span tags against the epoch on recording tags over the same batches -------------------------------------
    epoch_setup = tag_epoch_setup(out, ls, model)
    if epoch_setup is None:
        return out
    opt = epoch_setup[0]
    rng = np.random.default_rng(2)
    tags = (rng.random((n_rec, NCLASS)) < 0.2).astype(np.float32)
    span_tags = (rng.random((sp["n_spans"], NCLASS)) < 0.2).astype(np.float32)
    epoch = [0]

    def rec_level():
        train.train_recording_tags(ls, tags, model, opt, epoch[0], max_windows=BATCH)
        epoch[0] += 1

    def span_level():
        train.train_span_tags(ls, span_tags, model, opt, epoch[0], span3=sp["span3"], max_windows=BATCH)
        epoch[0] += 1
    out.update(alternate_legs({"epoch_recording_tags": rec_level, "epoch_span_tags": span_level}, rounds))
    addition(out, "span_tags_add_ms", out["epoch_recording_tags"], out["epoch_span_tags"])
    return out


def span_pieces_workload(name, model, rounds, reps, tag_span=10.0):
    """--span-pieces: (a) the piece entries alone beside the span entries on the whole recording's tables (one piece, off = 0);
    (b) one train_span_tags(split_long=True) epoch against the host-cut route - the recording cut at span boundaries into
    recordings of at most BATCH windows, today's train_span_tags over that set - alternated."""
    from dcase2019_task4_amd import train
    from dcase2019_task4_amd.longrec import window_plan
    ls, out, win_strong, win_att, d_s, d_a, err = tag_train_setup(name, model)
    cfg = inference._Cfg
    span3 = inference.tag_span_frames(tag_span, POOL * cfg.hop_length / cfg.sample_rate)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    n_rec, total, T3, hop3 = ls.n_rec, ls.total_frames, ls.T3, ls.hop3
    host, span0, n_spans, span3 = inference.span_table(ls, span3)
    out.update(tag_span_s=tag_span, span3=span3, total_spans=n_spans, max_windows=BATCH)
    # ---- (a) the entries alone ---------------------------------------------------------------------------------------------------
    g = torch.randn(n_spans, NCLASS, device=dev, generator=torch.Generator(dev).manual_seed(1))
    tags = torch.empty(n_spans, NCLASS, device=dev)
    sums = torch.empty(n_spans, NCLASS, 2, dtype=torch.float64, device=dev)
    off = torch.zeros(n_rec, dtype=torch.int32, device=dev)
    ws = torch.empty(l.sed_stitch_span_tags_ws_bytes(total, n_spans, n_rec, NCLASS, span3), dtype=torch.uint8, device=dev)
    assert ws.numel() == l.sed_stitch_piece_span_tags_ws_bytes(total, n_spans, n_rec, NCLASS, span3)
    head = (ptr(win_strong), ptr(win_att), ptr(ls.rec_win0), ptr(ls.rec_frame0), ptr(span0))
    geo = (n_rec, T3, NCLASS, hop3, 1, span3)
    f_tail = (ptr(tags), ptr(sums), ptr(ws), ws.numel(), ptr(err), _lib.stream_ptr())
    b_tail = (ptr(sums), ptr(g), ptr(d_s), ptr(d_a), ptr(err), _lib.stream_ptr())
    calls = {
        "sed_stitch_span_tags": lambda: _lib.check(l.sed_stitch_span_tags(*head, total, n_spans, *geo, *f_tail), "span forward"),
        "sed_stitch_piece_span_tags": lambda: _lib.check(l.sed_stitch_piece_span_tags(*head, total, n_spans, *geo, ptr(off), *f_tail),
                                                         "piece forward"),
        "sed_stitch_span_tags_backward": lambda: _lib.check(l.sed_stitch_span_tags_backward(*head, n_spans, *geo, *b_tail),
                                                            "span backward"),
        "sed_stitch_piece_span_tags_backward": lambda: _lib.check(
            l.sed_stitch_piece_span_tags_backward(*head, n_spans, *geo, ptr(off), *b_tail), "piece backward")}
    alone, kept = {}, {}
    for key, fn in calls.items():
        fn()
        kept[key] = [x.clone() for x in ((tags, sums) if "backward" not in key else (d_s, d_a))]
    alone["bytes_equal"] = bool(all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for a, b in
                                    (("sed_stitch_span_tags", "sed_stitch_piece_span_tags"),
                                     ("sed_stitch_span_tags_backward", "sed_stitch_piece_span_tags_backward"))
                                    for x, y in zip(kept[a], kept[b])))
    for key, fn in calls.items():
        alone[key] = event_ms(fn, reps)
    for a, b, key in (("sed_stitch_span_tags", "sed_stitch_piece_span_tags", "forward"),
                      ("sed_stitch_span_tags_backward", "sed_stitch_piece_span_tags_backward", "backward")):
        band = max(x["spread"] * x["median_ms"] for x in (alone[a], alone[b]))
        alone[key + "_piece_minus_span_ms"] = alone[b]["median_ms"] - alone[a]["median_ms"]
        alone[key + "_larger_max_minus_min_ms"] = band
        alone[key + "_difference_exceeds_spread"] = bool(abs(alone[key + "_piece_minus_span_ms"]) > band)
    assert int(err.item()) == 0
    out["entries_alone"] = alone
    del kept, win_strong, win_att, d_s, d_a
    # ---- (b) the epoch in pieces against the host-cut route ------------------------------------------------------------------------
    span_tags = (np.random.default_rng(2).random((n_spans, NCLASS)) < 0.2).astype(np.float32)
    plan = train.span_tag_plan(ls.rec_win0_host, ls.rec_frame0_host, span_tags, BATCH, span3, split_long=True, T3=T3, hop3=hop3)
    out["pieces"] = {"batches_per_epoch": len(plan["runs"]), "forwarded_windows": plan["forwarded_windows"],
                     "forwarded_over_windows": plan["forwarded"]}
    # the cut: as many whole spans per recording as give at most BATCH windows
    per = max(k for k in range(1, n_spans + 1) if window_plan(k * span3 * POOL, T, POOL, hop3)["n_w"] <= BATCH)
    n_rec_h, per_rec = WORKLOADS[name]
    recs = recordings(n_rec_h, per_rec)
    assert n_rec_h == 1
    cuts = [recs[0][a * POOL:min(a + per * span3, total) * POOL] for a in range(0, total, per * span3)]
    cut_set = inference.LongRecordingSet.from_arrays(cuts, T, scaler=scaler_of(recs[0]))
    assert inference.span_table(cut_set, span3)[2] == n_spans and int(np.diff(cut_set.rec_win0_host).max()) <= BATCH
    cut_plan = train.span_tag_plan(cut_set.rec_win0_host, cut_set.rec_frame0_host, span_tags, BATCH, span3)
    out["host_cut"] = {"recordings": cut_set.n_rec, "spans_per_recording": per, "batches_per_epoch": len(cut_plan["runs"]),
                       "forwarded_windows": cut_set.n_clips, "forwarded_over_windows": cut_set.n_clips / float(ls.n_clips)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    epoch = [0]

    def in_pieces():
        train.train_span_tags(ls, span_tags, model, opt, epoch[0], span3=span3, max_windows=BATCH, split_long=True)
        epoch[0] += 1

    def host_cut():
        train.train_span_tags(cut_set, span_tags, model, opt, epoch[0], span3=span3, max_windows=BATCH)
        epoch[0] += 1
    out.update(alternate_legs({"epoch_host_cut": host_cut, "epoch_in_pieces": in_pieces}, rounds))
    band = max(max(x["samples_ms"]) - min(x["samples_ms"]) for x in (out["epoch_host_cut"], out["epoch_in_pieces"]))
    out["pieces_minus_host_cut_ms"] = out["epoch_in_pieces"]["median_ms"] - out["epoch_host_cut"]["median_ms"]
    out["larger_max_minus_min_ms"] = band
    out["difference_exceeds_spread"] = bool(abs(out["pieces_minus_host_cut_ms"]) > band)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scoring", action="store_true", help="measure the scoring of the long path's event table instead")
    ap.add_argument("--sweep", action="store_true", help="measure the K-point sweep legs alone (profiles/long_sweep.json)")
    ap.add_argument("--weak", action="store_true", help="measure the recording-level weak tags (profiles/long_weak.json)")
    ap.add_argument("--tag-train", action="store_true",
                    help="measure the backward through the pooled tag and an epoch on recording tags (profiles/long_tag_train.json)")
    ap.add_argument("--span-tag-train", action="store_true",
                    help="measure the backward through the span tags and an epoch on span tags (profiles/long_span_tag_train.json)")
    ap.add_argument("--span-pieces", action="store_true",
                    help="measure a span-tag epoch over the 1 h recording in pieces against the host-cut route "
                         "(profiles/long_span_pieces.json)")
    ap.add_argument("--error-rate", action="store_true",
                    help="measure what validate_long(error_rate=True) adds (the \"long\" key of profiles/error_rate.json)")
    ap.add_argument("--hysteresis", action="store_true",
                    help="measure the two-threshold decode (profiles/long_hysteresis.json)")
    ap.add_argument("--process", action="store_true",
                    help="measure minimum event length and gap merging (profiles/long_process.json)")
    ap.add_argument("--scores", action="store_true",
                    help="measure the event scores and the select by score (profiles/long_scores.json)")
    ap.add_argument("--span-tags", action="store_true",
                    help="measure the span-level weak tags and the tag gate (profiles/long_span_tags.json)")
    ap.add_argument("--rasterize", action="store_true",
                    help="measure the pseudo strong labels: sed_events_rasterize and pseudo_label (profiles/long_rasterize.json)")
    ap.add_argument("--boundary-libs", default="",
                    help="with --scores: comma-separated builds of the library with other EVS_SHORT_FRAMES (csrc/evscore.hip)")
    ap.add_argument("--scores-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sweep-decode-only", action="store_true", help="with --sweep: sed_stitch_sweep alone (a variant build)")
    ap.add_argument("--sweep-out", default=os.path.join(REPO, "profiles", "long_sweep.json"))
    ap.add_argument("--candidates", default="", help="with --sweep: earlier --sweep-decode-only results to copy in")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode-reps", type=int, default=30)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "long_rasterize.json" if args.rasterize else "long_span_tags.json" if args.span_tags else "long_scores.json" if args.scores else "long_process.json" if args.process else
                                "long_hysteresis.json" if args.hysteresis else
                                "error_rate.json" if args.error_rate else
                                "long_span_pieces.json" if args.span_pieces else
                                "long_span_tag_train.json" if args.span_tag_train else
                                "long_tag_train.json" if args.tag_train else "long_weak.json" if args.weak else
                                "long_scoring.json" if args.scoring else "long_inference.json")
    if not torch.cuda.is_available():
        raise SystemExit("long_bench.py measures on the GPU: no device found (nothing is measured on a CPU)")
    if args.rounds < 5 or args.decode_reps < 20:
        raise SystemExit("need --rounds >= 5 and --decode-reps >= 20")
    if args.scores_child:
        return scores_child(args.scores_child, args.decode_reps)
    model, _ = bench.build_models("cuda", seed=0, mfma_dtype="f32")
    model.eval()
    result = {"tool": "tools/long_bench.py", "device": torch.cuda.get_device_name(0), "frames": T, "batch_size": BATCH,
              "model": "baseline CRNN, fp32 kernel set, eval mode", "rounds": args.rounds, "long_path_present": HAVE_LONG,
              "timing": "host clock around each synchronised call, legs alternated; decode alone: device events",
              "note": "the clips leg yields a different event table (events split at the cuts); rows are reported, not compared",
              "not_measured": ["from_waveforms / feature extraction", "other batch sizes, bf16 / wide models",
                               "recordings longer than 1 h", "a run with the GPU to itself (the host is shared)"],
              "workloads": {}}
    if args.rasterize:
        result["timing"] = ("sed_events_rasterize alone: a device-event pair around the Python call (no allocation: the pool is "
                            "given), warm, median of --decode-reps; the host route: host clock around the synchronised route, same "
                            "reps; pseudo_label / get_long_predictions: host clock around each synchronised call, the two legs "
                            "alternated in one run, --rounds rounds, medians, spread = (max - min) / median")
        result["note"] = ("the host route (table copied down, numpy difference array + cumsum, upload into the pool) is the only "
                          "route there was before; the run asserts that both routes' rows are identical bit for bit, and that "
                          "pseudo_label leaves the same rows in the set's label pool.  pseudo_label against get_long_predictions: "
                          "the same arguments (point 0's thresholds, median window 7); a difference counts only where it lies "
                          "outside the larger (max - min) of the two legs")
        result["not_measured"] += ["other nclass than 10", "combine=\"max\"", "soft values", "the two kernels one by one",
                                   "a scatter form (a clear, then one thread or wave per event): not written",
                                   "relabel while a training step is in flight"]
        for name in args.workloads.split(","):
            result["workloads"][name] = rasterize_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.span_tags:
        result["timing"] = ("get_long_predictions / validate_long legs: host clock around each synchronised call, the two legs "
                            "alternated in one run, --rounds rounds, medians, spread = (max - min) / median; the calls alone: a "
                            "device-event pair around the Python call (output and workspace allocation included), warm, median of "
                            "--decode-reps; the host route: host clock around the synchronised route, same reps")
        result["note"] = ("get_long_predictions(tag_span=10 s, min_span_tag=0.5) against the same run's plain call; validate_long "
                          "with the gate at 50 points against the same run's call without it; a difference counts only where it "
                          "lies outside the larger (max - min) of its two legs.  The composed route (two stitch_decode blends and "
                          "a torch fp64 segment_reduce over the spans) and the host gate are the only routes there were before")
        result["not_measured"] += ["other nclass than 10", "other hops than the default", "recordings beyond 1 h",
                                   "the kernels one by one", "other K than 50", "other span lengths through the two callers",
                                   "with a high threshold, events_process or the event scores behind the gate"]
        for name in args.workloads.split(","):
            result["workloads"][name] = span_tags_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.scores:
        result["timing"] = ("get_long_predictions legs: host clock around each synchronised call, the two legs alternated in one run, "
                            "--rounds rounds, medians, spread = (max - min) / median; sed_events_scores / sed_events_select alone: "
                            "a device-event pair around the Python call (output allocation included), warm, median of --decode-reps; "
                            "the host routes: host clock around the synchronised route, same reps")
        result["note"] = ("get_long_predictions(event_scores=True) against the same run's plain call, default hop, median window 7; "
                          "a difference counts only where it lies outside the larger (max - min) of its two legs.  The host routes "
                          "are the only ones there were before sed_events_scores / sed_events_select.  short_frames_tried: the "
                          "scorer alone on the same 50-point table under libraries built with other EVS_SHORT_FRAMES, each in a "
                          "process of its own")
        result["not_measured"] += ["the kernels one by one", "other K than 50", "other median windows", "the key score_mean",
                                   "min_event_score through get_long_predictions", "NaN posteriors"]
        libs = [x for x in args.boundary_libs.split(",") if x]
        for name in args.workloads.split(","):
            result["workloads"][name] = scores_workload(name, model, args.rounds, args.decode_reps, libs)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.process:
        result["timing"] = ("validate_long legs: host clock around each synchronised call, the two legs alternated in one run, "
                            "--rounds rounds, medians, spread = (max - min) / median; sed_events_process alone: a device-event "
                            "pair around the Python call (output and workspace allocation, five launches), warm, median of "
                            "--decode-reps; the host route: host clock around the synchronised route, same reps")
        result["note"] = ("validate_long(min_event_lengths=[0.25], min_event_gaps=[0.15]) at 50 points against the same run's "
                          "validate_long at the same points; a difference counts only where it lies outside the larger "
                          "(max - min) of its two legs.  The host route is the only one there was before sed_events_process.  "
                          "The order timed is drop_merge (order 0)")
        result["not_measured"] += ["the order merge_drop", "other K than 50", "other median windows", "other lengths and gaps",
                                   "the kernels one by one", "with PSDS, weak tags, the error rate or a high threshold",
                                   "max_table_bytes small enough to split the points into chunks"]
        for name in args.workloads.split(","):
            result["workloads"][name] = process_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.hysteresis:
        result["timing"] = ("validate_long legs: host clock around each synchronised call, the two legs alternated in one run, "
                            "--rounds rounds, medians, spread = (max - min) / median; sed_events_hysteresis alone: a device-event "
                            "pair around the Python call (output and workspace allocation, three launches), warm, median of "
                            "--decode-reps; the host route: host clock around the synchronised route, same reps")
        result["note"] = ("validate_long(thresholds_high=...) at 50 pairs against the same run's validate_long at the same 50 low "
                          "thresholds; a difference counts only where it lies outside the larger (max - min) of its two legs.  The "
                          "host route is the only one there was before sed_events_hysteresis")
        result["not_measured"] += ["other K than 50", "other median windows", "the kernels one by one", "with PSDS, weak tags or "
                                   "the error rate", "max_table_bytes small enough to split the pairs into chunks"]
        for name in args.workloads.split(","):
            result["workloads"][name] = hysteresis_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.error_rate:
        result["timing"] = ("validate_long legs: host clock around each synchronised call, the two legs alternated in one run, "
                            "--rounds rounds, medians, spread = (max - min) / median; the calls alone: a device-event pair around "
                            "the Python call (workspace allocation and the launches), warm, median of --decode-reps")
        result["note"] = ("validate_long(..., error_rate=True) against the same run's validate_long(...); a difference counts "
                          "only where it lies outside the larger (max - min) of its two legs")
        result["not_measured"] += ["the kernels one by one", "given-events mode", "other nclass than 10", "with PSDS or weak tags"]
        for name in args.workloads.split(","):
            result["workloads"][name] = error_rate_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        path, doc = args.out, {}
        if os.path.exists(path):                                      # tools/epoch_bench.py writes the "clips" key of the same file
            with open(path) as f:
                doc = json.load(f)
        doc["long"] = result
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        return
    if args.span_pieces:
        result["model"] = "baseline CRNN, fp32 kernel set; eval mode for the window tensors of the calls alone, train mode (dropout 0.5) in the epochs"
        result["timing"] = ("the calls alone: a device-event pair around the call, warm, median of --decode-reps; the epochs: host clock "
                            "around each synchronised epoch, the two legs alternated in one run, --rounds rounds, medians, "
                            "spread = (max - min) / median")
        result["note"] = ("tag_span 10 s, max_windows 64, every target known.  epoch_in_pieces: train_span_tags(split_long=True) over "
                          "the recording's own set - boundary windows of neighbouring pieces are forwarded in both batches "
                          "(forwarded_over_windows), tags and gradients are the whole recording's.  epoch_host_cut: the only earlier "
                          "route - the recording cut on the host at span boundaries into recordings of at most 64 windows, a second "
                          "set (a second pool), today's train_span_tags; frames near a cut lose covering windows, so its blend, tags "
                          "and gradients differ from the recording's.  The two legs do different arithmetic: the rows are times, "
                          "not a comparison of results.  A difference counts only where it exceeds the larger (max - min) of the "
                          "two legs")
        result["not_measured"] += ["other nclass than 10", "other hops than the default", "other span lengths than 10 s",
                                   "other max_windows than 64", "unknown (NaN) targets", "the 100x3min workload (no recording there "
                                   "has more windows than one forward holds: the plan is today's)", "per-kernel counters",
                                   "the uniform weighting", "f16 models", "ema_model given", "the loss curves of the two routes",
                                   "recording-level tags of such a recording: every window in one step, out of scope"]
        for name in [n for n in args.workloads.split(",") if WORKLOADS[n][0] == 1]:
            result["workloads"][name] = span_pieces_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.span_tag_train:
        result["model"] = "baseline CRNN, fp32 kernel set; eval mode for the window tensors of (a) and (b), train mode (dropout 0.5) in (c)"
        result["timing"] = ("the calls alone: a device-event pair around the call(s), warm, median of --decode-reps; the epochs: host "
                            "clock around each synchronised epoch, legs alternated, --rounds rounds")
        result["note"] = ("(a) tag_span 10 s; the composed route is a torch-autograd restatement of the taper blend (index_add_ over "
                          "the covered window frames) and a per-span fp64 segment_reduce, backward by autograd.grad on a kept graph - "
                          "the only route to this gradient before sed_stitch_span_tags_backward; (b) one span per recording: the "
                          "same call beside sed_stitch_weak_backward on the same sums and gradients, in the same run; (c) both "
                          "epochs run the same batches (runs of recordings within max_windows), forward + backward + Adam step "
                          "through the autograd nodes, every target known.  A difference counts only where it exceeds the larger "
                          "(max - min) of the two legs")
        result["not_measured"] += ["other nclass than 10", "other hops than the default", "other span lengths than 10 s and one span "
                                   "per recording", "per-kernel counters", "the uniform weighting", "unknown (NaN) targets",
                                   "an epoch over the 1 h recording (more windows than one forward holds)",
                                   "f16 models", "ema_model given", "LDS staging of a span row's g / num / den: not written"]
        for name in args.workloads.split(","):
            result["workloads"][name] = span_tag_train_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.tag_train:
        result["model"] = "baseline CRNN, fp32 kernel set; eval mode for the window tensors of (a), train mode (dropout 0.5) in (b)"
        result["timing"] = ("the calls alone: a device-event pair around the call(s), warm, median of --decode-reps; the epochs: host "
                            "clock around each synchronised epoch, legs alternated, --rounds rounds")
        result["note"] = ("(a) the composed route is a torch-autograd restatement of the taper blend (index_add_ over the covered "
                          "window frames) and the fp64 pooling, backward by autograd.grad on a kept graph - the only route to this "
                          "gradient before sed_stitch_weak_backward; (b) both epochs run the same batches (runs of recordings within "
                          "max_windows), forward + backward + Adam step through the autograd nodes; the window-level leg holds every "
                          "window's own weak output to its recording's tags.  A difference counts only where it exceeds the larger "
                          "(max - min) of the two legs")
        result["not_measured"] += ["other nclass than 10", "other hops than the default", "per-kernel counters", "the uniform weighting",
                                   "an epoch over the 1 h recording (more windows than one forward holds)",
                                   "f16 models", "ema_model given"]
        for name in args.workloads.split(","):
            result["workloads"][name] = tag_train_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.weak:
        result["timing"] = ("get_long_predictions legs: host clock around each synchronised call, alternated; the calls alone: a "
                            "device-event pair around the call(s), warm, median of --decode-reps")
        result["note"] = ("predictions_with_weak against the same run's predictions: what the tags add; the composed route is two "
                          "stitch_decode(want_timeline=True) blends and a torch fp64 segment_reduce, the only route before "
                          "sed_stitch_weak; a difference counts only where it exceeds the larger (max - min) of the two legs")
        result["not_measured"] += ["other nclass than 10", "other hops than the default", "per-kernel counters",
                                   "validate_long(weak_labels=...)"]
        for name in args.workloads.split(","):
            result["workloads"][name] = weak_workload(name, model, args.rounds, args.decode_reps)
            print(json.dumps({name: result["workloads"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        return
    if args.sweep:
        args.scoring, args.out = True, None
    sweep = dict(result, workloads={}, timing="validate_long legs: host clock around each synchronised call, alternated; the calls "
                 "alone: a device-event pair around the call(s), warm, median of --decode-reps",
                 note="the loop leg (one_blend=False) is the code path of the commit before the sweep; one blend counts as faster "
                 "only where the difference of the medians exceeds the larger of the two legs' (max - min)",
                 not_measured=result["not_measured"] + ["other K than 50", "other median windows",
                                                        "max_table_bytes small enough to split the points into chunks"])
    if args.scoring:
        result["timing"] = ("host clock around each synchronised call, legs alternated; the scoring calls alone: a device-event "
                            "pair around the Python call (workspace allocation and four launches)")
        result["note"] = ("validate_long against the same run's get_long_predictions: the cost scoring adds to inference; no "
                          "earlier route exists (sed_event_counts raises beyond 64 events per column)")
        result["not_measured"] += ["the kernels one by one", "given-events mode", "other t_collar / resolutions"]
    for name in args.workloads.split(","):
        if args.scoring:
            result["workloads"][name], ctx = scoring_workload(name, model, args.rounds, args.decode_reps, setup_only=args.sweep)
            sweep["workloads"][name] = sweep_workload(name, ctx, model, args.rounds, args.decode_reps, args.sweep_decode_only)
            print(json.dumps({"sweep_" + name: sweep["workloads"][name]}), flush=True)
            del ctx
        else:
            result["workloads"][name] = workload(name, model, args.rounds, args.decode_reps)
        if not args.sweep:
            print(json.dumps({name: result["workloads"][name]}), flush=True)
    if args.scoring:
        for path in filter(None, args.candidates.split(",")):
            with open(path) as f:
                other = json.load(f)
            for name, w in other["workloads"].items():
                sweep["workloads"][name].setdefault("point_group_candidates", []).append(
                    {"point_group": w["point_group"], "sed_stitch_sweep": w["sed_stitch_sweep"]})
        os.makedirs(os.path.dirname(os.path.abspath(args.sweep_out)), exist_ok=True)
        with open(args.sweep_out, "w") as f:
            f.write(json.dumps(sweep, indent=1) + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
