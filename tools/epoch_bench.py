"""What a training epoch on precomputed features costs per step - resident front-end against the resident-batch step and the
drop-in feeding path - at DESED's sizes (1 262 weak / 14 412 unlabelled / 1 637 synthetic clips, ragged lengths, some longer
than `frames`).  Device-event timing; prints one JSON object (and writes it to --out).

  (a) one full epoch through resident.ResidentFrontEnd (the gather of batch k + 1 inside step k's hipGraph), ms / step
  (a') the same epoch with an augmentation policy on the set (mixup of every clip, time shift, both masks: the gather goes
      into staging buffers and sed_batch_augment writes the slot), alternated with the plain epoch in the same run: ms / step
      of either (median of 5 rounds), their ratio and each leg's spread over the rounds, (max - min) / median (--only-aug: this
      pair only).  Part of the default run too: a second resident set and 5 + 5 epochs per shape.  The two front-ends draw
      their index tables alternately from numpy's global generator, so the plain leg's batches are not leg (a)'s - the same
      pool and shapes, which is what the timing needs
  (b) the resident-batch step of the same shape (bench.py's mt-* leg: one batch in HBM, MeanTeacherStep.run() replayed)
  (c) 20 steps of the drop-in path: DataLoadDf-style dataset (np.load per clip) + features.get_transforms, num_workers=0,
      host collate, step.step
  (d) get_predictions over 400 validation clips: per-clip dataset (np.load + get_transforms per clip) against the resident set
  (e) validation scoring over 1 168 and 400 resident clips: metrics.validate at one operating point and at 50 thresholds, the
      DataFrame route (get_predictions + compute_strong_metrics), sed_event_counts alone, and - next to them, in the same
      run - validate(..., psds=...) and sed_psds_counts alone at the same operating points (--only-e: this leg only)
      error_rate (with --only-e; --only-error-rate: alone, into the "clips" key of profiles/error_rate.json): validate(...,
      error_rate=True) against the same run's validate(...) at one point and at 50 thresholds, the two legs alternated, 5
      rounds, medians and spread = (max - min) / median; sed_error_counts alone beside sed_event_counts (device events, median
      of 30); the largest merged cluster met

Usage: python tools/epoch_bench.py [--shapes 24:f32,64:bf16] [--only-a | --only-aug | --only-e | --only-error-rate] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench                                                    # noqa: E402  (build_models / synthetic_batch of the mt-* legs)
from dcase2019_task4_amd.features import Scaler, get_transforms  # noqa: E402
from dcase2019_task4_amd.augment import AugmentPolicy  # noqa: E402
from dcase2019_task4_amd.resident import ResidentFeatureSet, ResidentFrontEnd  # noqa: E402
from dcase2019_task4_amd.train import MeanTeacherStep  # noqa: E402

SIZES = (1262, 14412, 1637)
T, N_MELS, NCLASS = 628, 64, 10


def synthetic_pool(seed=0):
    """Ragged linear-mel clips: 85 % of the full 628 frames, the rest 300 .. 900 frames; targets weak / -1 / strong."""
    rs = np.random.RandomState(seed)
    n = sum(SIZES)
    lengths = np.where(rs.uniform(size=n) < 0.85, T, rs.randint(300, 901, size=n))
    flat = np.random.default_rng(seed).random(int(lengths.sum()) * N_MELS, dtype=np.float32)
    flat *= 3.0
    offs = np.r_[0, np.cumsum(lengths)[:-1]] * N_MELS
    feats = [flat[o:o + l * N_MELS].reshape(l, N_MELS) for o, l in zip(offs, lengths)]
    T3 = T // 8
    weak = np.repeat((rs.uniform(size=(SIZES[0], 1, NCLASS)) < 0.2).astype(np.float32), T3, axis=1)
    strong = (rs.uniform(size=(SIZES[2], T3, NCLASS)) < 0.1).astype(np.float32)
    tgts = list(weak) + [-np.ones((T3, NCLASS), np.float32)] * SIZES[1] + list(strong)
    return feats, tgts, lengths


def scaler_of(feats):
    from oracle import features_np
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(f, T) for f in feats[:64]])
    return sc


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def leg_a(rs, B, dtype):
    student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
    st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, rs.weak_mask, rs.strong_mask, seed=1234)
    fe = ResidentFrontEnd(st, rs)
    for _ in range(10):                    # eager steps + capture of the two graphs + warm replays
        fe.run()
    torch.cuda.synchronize()
    n = len(rs)
    ms = event_ms(fe.run, n)               # one full epoch (it crosses into the next one: the table was drawn ahead)
    assert np.isfinite(st.meters()["loss"])
    st.close()
    return ms, n


def leg_a_aug(rs, rs_aug, B, dtype, rounds=5):
    """The plain and the augmented resident epoch, alternated: both front-ends are built and warmed first, then ``rounds``
    times one full plain epoch and one full augmented epoch are timed back to back (device events)."""
    fes = []
    for r in (rs, rs_aug):
        student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
        st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, r.weak_mask, r.strong_mask, seed=1234)
        fe = ResidentFrontEnd(st, r)
        for _ in range(10):
            fe.run()
        fes.append((st, fe))
    torch.cuda.synchronize()
    n = len(rs)
    plain, aug = [], []
    for _ in range(rounds):
        plain.append(event_ms(fes[0][1].run, n))
        aug.append(event_ms(fes[1][1].run, n))
    for st, _ in fes:
        assert np.isfinite(st.meters()["loss"])
        st.close()
    mp, ma = float(np.median(plain)), float(np.median(aug))
    return {"aug_policy": "mixup_alpha 0.2, mixup_prob 1, shift_std 8 label frames, freq_mask_max 8, time_mask_max 64",
            "aug_rounds": rounds,
            "a_plain_ms_per_step_rounds": [round(v, 4) for v in plain], "a_aug_ms_per_step_rounds": [round(v, 4) for v in aug],
            "a_plain_alternated_ms_per_step": round(mp, 4), "a_aug_ms_per_step": round(ma, 4),
            "a_aug_over_plain": round(ma / mp, 4),
            "a_plain_spread_max_minus_min_over_median": round((max(plain) - min(plain)) / mp, 4),
            "a_aug_spread_max_minus_min_over_median": round((max(aug) - min(aug)) / ma, 4)}


def leg_b(B, dtype, n):
    student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
    x, xe, tgt, wm, sm = bench.synthetic_batch(B, T, 1000, "cuda")
    st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, wm, sm, seed=1234)
    st.load_batch(x, xe, tgt)
    for _ in range(10):
        st.run()
    torch.cuda.synchronize()
    ms = event_ms(st.run, n)
    st.close()
    return ms


class _NpyDataset:
    """DataLoadDf.__getitem__ (DataLoad.py:120-140): np.load of the clip's feature file + transform((features, label))."""

    def __init__(self, paths, tgts, transform):
        self.paths, self.tgts, self.transform = paths, tgts, transform

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return self.transform((np.load(self.paths[i]), self.tgts[i]))


def leg_c(rs, feats, tgts, sc, B, dtype, tmp, n_steps=20):
    np.random.seed(3)
    rows = rs.epoch_table()[:n_steps + 2]
    used = sorted(set(rows.reshape(-1).tolist()))
    paths = {}
    for i in used:
        paths[i] = os.path.join(tmp, f"c{i}.npy")
        np.save(paths[i], feats[i])
    ds = _NpyDataset([paths.get(i) for i in range(len(feats))], tgts, get_transforms(T, sc, augment_type="noise"))
    loader = torch.utils.data.DataLoader(ds, batch_sampler=[list(r) for r in rows], num_workers=0)
    student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
    st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, rs.weak_mask, rs.strong_mask, seed=1234)
    it = iter(loader)
    for _ in range(2):
        x, xe, y = next(it)
        st.step(x.cuda(non_blocking=True), xe.cuda(non_blocking=True), y.cuda(non_blocking=True))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n_steps):
        x, xe, y = next(it)
        st.step(x.cuda(non_blocking=True), xe.cuda(non_blocking=True), y.cuda(non_blocking=True))
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / n_steps
    st.close()
    return e0.elapsed_time(e1) / n_steps, wall


def leg_d(feats, sc, tmp, n=400):
    import pandas as pd
    from dcase2019_task4_amd.inference import get_predictions
    from oracle import postprocess_np as pp
    base = sum(SIZES[:2])                             # 400 of the synthetic-stream clips as the validation set
    idx = list(range(base, base + n))
    paths = []
    for i in idx:
        p = os.path.join(tmp, f"v{i}.npy")
        np.save(p, feats[i])
        paths.append(p)

    class PerClip:
        def __init__(self):
            self.tr = get_transforms(T, sc)
            self.filenames = pd.Series([f"clip_{i}.wav" for i in idx])

        def __len__(self):
            return n

        def __getitem__(self, k):
            return self.tr((np.load(paths[k]), np.zeros(1)))

        def get_sample(self, k):
            return np.load(paths[k]), np.zeros(1)

    per = PerClip()
    res = ResidentFeatureSet.for_eval(per, T, sc)
    model, _ = bench.build_models("cuda", seed=0)
    model.eval()
    labels = [f"c{i}" for i in range(NCLASS)]
    enc = type("Enc", (), {"labels": labels, "decode_strong": lambda self, m: pp.decode_strong(m, labels)})()
    out = {}
    for name, ds in (("per_clip", per), ("resident", res)):
        get_predictions(model, ds, enc.decode_strong, 8, batch_size=64)           # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        df = get_predictions(model, ds, enc.decode_strong, 8, batch_size=64)
        torch.cuda.synchronize()
        out[name] = ((time.perf_counter() - t0) * 1e3, df)
    same = out["per_clip"][1].equals(out["resident"][1])
    return {"clips": n, "batch_size": 64, "per_clip_ms": round(out["per_clip"][0], 2), "resident_ms": round(out["resident"][0], 2),
            "same_dataframe": bool(same)}


def leg_e(feats, sc, sizes=(1168, 400), reps=20):
    """Median over ``reps`` of a host clock around calls that end in a device -> host copy (warmed up once each); the
    sed_event_counts share is device-event time of the launches alone on the set's posteriors."""
    import pandas as pd
    from dcase2019_task4_amd import metrics
    from dcase2019_task4_amd.inference import get_predictions
    from oracle import postprocess_np as pp
    model, _ = bench.build_models("cuda", seed=0)
    model.eval()
    labels = [f"c{i}" for i in range(NCLASS)]
    enc = type("Enc", (), {"labels": labels, "decode_strong": lambda self, m: pp.decode_strong(m, labels)})()
    base = sum(SIZES[:2])

    def wall_ms(fn):
        fn()
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(times)), 3)

    out = []
    for n in sizes:
        ds = type("DS", (), {"__len__": lambda self: n, "get_sample": lambda self, k: (feats[base + k], np.zeros(1)),
                             "filenames": pd.Series([f"clip_{i}.wav" for i in range(n)])})()
        res = ResidentFeatureSet.for_eval(ds, T, sc)
        files = res.filenames.tolist()
        rs = np.random.RandomState(n)                     # DESED-like annotations: 0 .. 5 events per clip, 0.25 .. 10 s
        rows = []
        for f in files:
            for _ in range(rs.randint(0, 6)):
                on = rs.uniform(0.0, 9.0)
                rows.append((f, on, min(10.0, on + rs.uniform(0.25, 5.0)), labels[rs.randint(NCLASS)]))
        valid_df = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
        ref = metrics.RefEvents.from_dataframe(valid_df, files, labels)
        thr50 = [float(v) for v in np.linspace(0.01, 0.99, 50)]
        with torch.no_grad():
            strong = torch.cat([model(res.eval_batch(i0, min(64, n - i0)))[0] for i0 in range(0, n, 64)])
        thr1, win1 = metrics.operating_points((0.5,), (5,), "cuda")
        thr_k, win_k = metrics.operating_points(thr50, (5,), "cuda")

        def count_launches(thr, win):
            counts = metrics.Counts(thr.numel(), NCLASS, "cuda")
            return lambda: [metrics.event_counts(strong[i0:i0 + 64], ref, thr, win, 8, clip_offset=i0, counts=counts)
                            for i0 in range(0, n, 64)]

        def psds_launches(thr, win):
            counts = metrics.PSDSCounts(thr.numel(), NCLASS, "cuda")
            return lambda: [metrics.psds_counts(strong[i0:i0 + 64], ref, thr, win, 8, clip_offset=i0, counts=counts)
                            for i0 in range(0, n, 64)]

        def validate_psds(thresholds):
            def run():                                      # what a user's epoch does: both sets of totals reach the host
                psds = metrics.PSDSCounts(len(thresholds), NCLASS, "cuda")
                metrics.validate(model, res, ref, 8, thresholds, (5,), batch_size=64, psds=psds)
                psds.host()
            return run
        n_est = int(count_launches(thr1, win1)()[-1].host()[0][0, :, 2].sum())
        count_launches(thr_k, win_k)()
        psds_1 = psds_launches(thr1, win1)()[-1].host()[0]
        psds_launches(thr_k, win_k)()
        # (a randomly initialised CRNN: posteriors nearly constant in time, so few estimated events per clip)
        leg = {"clips": n, "batch_size": 64, "reference_events": len(rows), "estimated_events_at_0.5": n_est,
               "i_validate_1_point_ms": wall_ms(lambda: metrics.validate(model, res, ref, 8, batch_size=64)),
               "ii_validate_50_thresholds_ms": wall_ms(lambda: metrics.validate(model, res, ref, 8, thr50, (5,), batch_size=64)),
               "iii_dataframe_route_ms": wall_ms(lambda: metrics.compute_strong_metrics(
                   get_predictions(model, res, enc.decode_strong, 8, batch_size=64), valid_df)),
               "iv_event_counts_only_1_point_ms": round(event_ms(count_launches(thr1, win1), 20), 4),
               "iv_event_counts_only_50_thresholds_ms": round(event_ms(count_launches(thr_k, win_k), 20), 4)}
        # PSDS: the same posteriors, references and operating points, timed in the same run as iv
        leg.update({"psds_tp_fp_ct_at_0.5": [int(psds_1[:, 0].sum()), int(psds_1[:, 1].sum()), int(psds_1[:, 2:].sum())],
                    "v_validate_with_psds_1_point_ms": wall_ms(validate_psds([0.5])),
                    "v_validate_with_psds_50_thresholds_ms": wall_ms(validate_psds(thr50)),
                    "vi_psds_counts_only_1_point_ms": round(event_ms(psds_launches(thr1, win1), 20), 4),
                    "vi_psds_counts_only_50_thresholds_ms": round(event_ms(psds_launches(thr_k, win_k), 20), 4)})
        leg["vi_over_iv_50_thresholds"] = round(leg["vi_psds_counts_only_50_thresholds_ms"]
                                                / leg["iv_event_counts_only_50_thresholds_ms"], 3)
        leg["iv_share_of_i"] = round(leg["iv_event_counts_only_1_point_ms"] / leg["i_validate_1_point_ms"], 4)
        leg["ii_over_i"] = round(leg["ii_validate_50_thresholds_ms"] / leg["i_validate_1_point_ms"], 3)
        out.append(leg)
        print(json.dumps(leg), flush=True)
    return out


def alternated(legs, rounds):
    """``legs``: name -> call ending in a device -> host copy.  One warm call each, then ``rounds`` rounds in which the legs
    alternate; per leg the median, spread = (max - min) / median and the samples of a host clock around the call."""
    for fn in legs.values():
        fn()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(float(np.median(v)), 3), "spread": round(float((max(v) - min(v)) / np.median(v)), 4),
                   "max_minus_min_ms": round(float(max(v) - min(v)), 3), "samples_ms": [round(x, 3) for x in v]}
            for name, v in ms.items()}


def difference(legs, plain, added):
    """What ``added`` costs over ``plain`` and whether that lies outside the larger (max - min) of the two legs."""
    d = legs[added]["median_ms"] - legs[plain]["median_ms"]
    band = max(legs[plain]["max_minus_min_ms"], legs[added]["max_minus_min_ms"])
    return {"added_ms": round(d, 3), "larger_max_minus_min_ms": band, "outside_the_band": bool(abs(d) > band)}


def events_alone(fn, reps=30):
    """Median and spread of ``reps`` single device-event pairs around fn(), after 3 warm calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(t)), 4), "spread": round(float((max(t) - min(t)) / np.median(t)), 4), "reps": reps}


def leg_e_error_rate(feats, sc, sizes=(1168, 400), rounds=5):
    """What the overall error rate adds to validation: validate(..., error_rate=True) against the same run's validate(...) at
    one operating point and at 50 thresholds, legs alternated, ``rounds`` rounds; and the sed_error_counts launches alone
    beside the sed_event_counts launches on the same posteriors (device events, median of 30).  The annotations are those of
    leg (e)."""
    import pandas as pd
    from dcase2019_task4_amd import metrics
    from long_bench import largest_cluster
    model, _ = bench.build_models("cuda", seed=0)
    model.eval()
    labels = [f"c{i}" for i in range(NCLASS)]
    base = sum(SIZES[:2])
    out = []
    for n in sizes:
        ds = type("DS", (), {"__len__": lambda self: n, "get_sample": lambda self, k: (feats[base + k], np.zeros(1)),
                             "filenames": pd.Series([f"clip_{i}.wav" for i in range(n)])})()
        res = ResidentFeatureSet.for_eval(ds, T, sc)
        files = res.filenames.tolist()
        rs = np.random.RandomState(n)
        rows = []
        for f in files:
            for _ in range(rs.randint(0, 6)):
                on = rs.uniform(0.0, 9.0)
                rows.append((f, on, min(10.0, on + rs.uniform(0.25, 5.0)), labels[rs.randint(NCLASS)]))
        valid_df = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
        ref = metrics.RefEvents.from_dataframe(valid_df, files, labels)
        thr50 = [float(v) for v in np.linspace(0.01, 0.99, 50)]
        with torch.no_grad():
            strong = torch.cat([model(res.eval_batch(i0, min(64, n - i0)))[0] for i0 in range(0, n, 64)])
        points = {"1_point": metrics.operating_points((0.5,), (5,), "cuda"), "50_thresholds": metrics.operating_points(thr50, (5,), "cuda")}
        leg = {"clips": n, "batch_size": 64, "reference_events": len(rows), "rounds": rounds}
        for name, (thr, win) in points.items():
            kw = dict(thresholds=thr, median_windows=win, batch_size=64)
            t = alternated({"validate": lambda: metrics.validate(model, res, ref, 8, **kw),
                            "validate_error_rate": lambda: metrics.validate(model, res, ref, 8, error_rate=True, **kw)}, rounds)
            t["difference"] = difference(t, "validate", "validate_error_rate")
            counts, errors = metrics.Counts(thr.numel(), NCLASS, "cuda"), metrics.ErrorCounts(thr.numel(), NCLASS, "cuda")
            t["sed_event_counts_alone"] = events_alone(lambda: [
                metrics.event_counts(strong[i0:i0 + 64], ref, thr, win, 8, clip_offset=i0, counts=counts) for i0 in range(0, n, 64)])
            t["sed_error_counts_alone"] = events_alone(lambda: [
                metrics.error_counts(strong[i0:i0 + 64], ref, thr, win, 8, clip_offset=i0, counts=errors) for i0 in range(0, n, 64)])
            counts.host(), errors.host()                      # raise when an error word is set
            # the merged clusters: a cluster holds at most the clip's events, so the per-clip totals bound it at every point
            per_file = metrics.error_counts(strong, ref, thr, win, 8, per_file=True).ev_files.cpu().numpy()
            t["most_events_in_a_clip"] = {"reference": int(per_file[..., 0].max()), "estimated": int(per_file[..., 1].max())}
            leg[name] = t
        m_e, m_s = metrics.validate(model, res, ref, 8, batch_size=64, error_rate=True)[0]
        leg["overall_error_rate_at_0.5"] = {"event_based": m_e.results_overall_metrics()["error_rate"],
                                            "segment_based": m_s.results_overall_metrics()["error_rate"]}
        # exactly, at the one point: the largest cluster of the clips' merged onsets (estimated events from a host decode)
        from dcase2019_task4_amd.inference import get_predictions
        from oracle import postprocess_np as pp
        enc = type("Enc", (), {"labels": labels, "decode_strong": lambda self, m: pp.decode_strong(m, labels)})()
        df = get_predictions(model, res, enc.decode_strong, 8, batch_size=64)
        est_on = {f: g["onset"].to_numpy(np.float64) for f, g in df.groupby("filename")}
        ref_on = {f: g["onset"].to_numpy(np.float64) for f, g in valid_df.groupby("filename")}
        none = np.zeros(0)
        sizes_1 = [largest_cluster(np.sort(ref_on.get(f, none)), np.sort(est_on.get(f, none))) for f in files]
        leg["largest_merged_cluster_at_0.5"] = {"reference": max(s[0] for s in sizes_1), "estimated": max(s[1] for s in sizes_1)}
        out.append(leg)
        print(json.dumps(leg), flush=True)
    return out


def update_json(path, key, value):
    """profiles/error_rate.json is written by two tools: each replaces its own key."""
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = value
    with open(path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="24:f32,64:bf16")
    ap.add_argument("--only-error-rate", action="store_true",
                    help="the error_rate leg of (e) only: validate(error_rate=True) against validate (--out: profiles/error_rate.json)")
    ap.add_argument("--only-a", action="store_true", help="leg (a) only (for a kernel trace of the resident epoch)")
    ap.add_argument("--only-aug", action="store_true", help="leg (a') only: the plain and the augmented resident epoch, alternated")
    ap.add_argument("--only-e", action="store_true", help="leg (e) only: validation scoring")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.cuda.get_device_properties(0)
    t0 = time.perf_counter()
    feats, tgts, lengths = synthetic_pool()
    sc = scaler_of(feats)
    result = {"device": dev.name, "pool": {"clips": list(SIZES), "frames_min": int(lengths.min()), "frames_max": int(lengths.max()),
                                           "longer_than_frames": int((lengths > T).sum()), "frames": T,
                                           "bytes": int(lengths.sum()) * N_MELS * 4}, "legs": []}
    build_s = None
    if a.only_error_rate:
        doc = {"tool": "tools/epoch_bench.py --only-error-rate", "device": dev.name, "frames": T,
               "timing": "validate legs: host clock around each synchronised call, the two legs alternated in one run, 5 rounds, "
                         "medians, spread = (max - min) / median; the calls alone: device events, median of 30",
               "sets": leg_e_error_rate(feats, sc)}
        print(json.dumps(doc))
        update_json(a.out or os.path.join(REPO, "profiles", "error_rate.json"), "clips", doc)
        return
    if a.only_aug:
        result["command"] = f"python tools/epoch_bench.py --only-aug --shapes {a.shapes}"
    with tempfile.TemporaryDirectory() as tmp:
        for shape in ([] if a.only_e else a.shapes.split(",")):
            B, dtype = int(shape.split(":")[0]), shape.split(":")[1]
            bs = [B // 4, B // 2, B // 4]
            tb = time.perf_counter()
            rs = ResidentFeatureSet.from_arrays(feats, tgts, SIZES, bs, frames=T, scaler=sc, augment_type="noise")
            torch.cuda.synchronize()
            build_s = build_s or round(time.perf_counter() - tb, 2)
            np.random.seed(0)
            leg = {"B": B, "mfma_dtype": dtype, "batch_sizes": bs, "steps_per_epoch": len(rs)}
            if not a.only_aug:
                ms_a, n = leg_a(rs, B, dtype)
                leg["a_resident_epoch_ms_per_step"] = round(ms_a, 4)
            if not a.only_a:
                # the same pool with a policy (worst case for partner reads: every clip mixes); the two sets share nothing
                rs_aug = ResidentFeatureSet.from_arrays(feats, tgts, SIZES, bs, frames=T, scaler=sc, augment_type="noise",
                                                        augment=AugmentPolicy(mixup_alpha=0.2, mixup_prob=1.0, shift_std=8.0,
                                                                              freq_mask_max=8, time_mask_max=64, seed=1))
                leg.update(leg_a_aug(rs, rs_aug, B, dtype))
                del rs_aug
            if not a.only_a and not a.only_aug:
                ms_b = leg_b(B, dtype, n)
                ms_c, wall_c = leg_c(rs, feats, tgts, sc, B, dtype, tmp)
                leg.update({"b_resident_batch_ms_per_step": round(ms_b, 4),
                            "a_over_b": round(ms_a / ms_b, 4),
                            "c_dropin_ms_per_step": round(ms_c, 3), "c_dropin_wall_ms_per_step": round(wall_c, 3),
                            "c_steps": 20})
            result["legs"].append(leg)
            print(json.dumps(leg), flush=True)
            del rs
            torch.cuda.empty_cache()
        if not a.only_a and not a.only_e and not a.only_aug:
            result["d_get_predictions"] = leg_d(feats, sc, tmp)
        if not a.only_a and not a.only_aug:
            result["e_validation_scoring"] = leg_e(feats, sc)
            if a.only_e:
                result["e_error_rate"] = leg_e_error_rate(feats, sc)
            result["command"] = "python tools/epoch_bench.py" + (" --only-e" if a.only_e else f" --shapes {a.shapes}")
    result["pool"]["build_s"] = build_s
    result["total_s"] = round(time.perf_counter() - t0, 1)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
