"""TEST INFRASTRUCTURE ONLY - the inputs of tests/test_gpu_error_rate.py, built without a GPU so that
tests/test_error_rate_cpu.py can confirm on the statement (tests/error_rate_np.py) what the device tests rely on: every case
but the deliberate one stays within 64 events per side and merged cluster, the straddling cluster straddles, the segments
with both kinds of error exist.

``cols[file][class]`` = ``[(onset, offset)]`` sorted by onset, Python floats.
"""
import numpy as np

from oracle import postprocess_np as pp
from tests import long_score_np as ls
from tests import sed_eval_np as se

PTR, SR, HOP = 8, 44100, 511                    # pooling_time_ratio, sample rate, hop (config.py:17,19)
N_CLIPS, T = 3, 96
POINTS = [(0.5, 5), (0.35, 3)]                  # (threshold, median window) of the decoded cases
CLIP_CLASSES = (1, 3, 16)


def names(n, nclass):
    return [f"clip_{i}.wav" for i in range(n)], [f"c{i}" for i in range(nclass)]


def estimate_of(ref_file, rs, nclass, span, p_drop=0.15, p_relabel=0.35, p_extra=0.25):
    """Estimated events of one file made from its references: dropped, moved by up to 0.3 s at both ends, RELABELLED to a
    random class (the substitutions), plus a few events of their own."""
    est = [[] for _ in range(nclass)]
    for c, col in enumerate(ref_file):
        for on, off in col:
            if rs.uniform() < p_drop:
                continue
            a, b = on + float(rs.uniform(-0.3, 0.3)), off + float(rs.uniform(-0.3, 0.3))
            a, b = (a, b) if a <= b else (b, a)
            c2 = int(rs.randint(nclass)) if rs.uniform() < p_relabel else c
            est[c2].append((a, b))
            if rs.uniform() < p_extra:
                x = float(rs.uniform(0.0, span))
                est[int(rs.randint(nclass))].append((x, x + float(rs.uniform(0.1, 2.5))))
    return [sorted(col) for col in est]


def clip_events(nclass, seed=0):
    """(ref_cols, est_cols) of 3 clips of about 9 s: clip 1 is empty on both sides; clip 0 holds a reference that starts
    before 0 and an estimated event that ends three segments after the last reference; several events per class overlap
    events of other classes."""
    rs = np.random.RandomState(100 + nclass + seed)
    ref, est = [], []
    for f in range(N_CLIPS):
        if f == 1:
            ref.append([[] for _ in range(nclass)])
            est.append([[] for _ in range(nclass)])
            continue
        file_cols = []
        for c in range(nclass):
            on = np.sort(rs.uniform(0.0, 8.0, size=rs.randint(0, 5 if nclass > 1 else 12)))
            file_cols.append([(float(a), float(a + l)) for a, l in zip(on, rs.uniform(0.1, 2.0, size=len(on)))])
        if f == 0:
            file_cols[0] = sorted(file_cols[0] + [(-0.15, 0.8)])
        ref.append(file_cols)
        e = estimate_of(file_cols, rs, nclass, 8.0)
        if f == 0:
            e[nclass - 1] = sorted(e[nclass - 1] + [(10.2, 12.6)])
        est.append(e)
    return ref, est


def posteriors(nclass, seed=0):
    """``[3, 96, nclass]`` float32: a few plateaus of 0.8 per column on a floor of 0.1, noise of +-0.3 (so the two operating
    points decode different events); clip 1 stays at 0.05: empty at both points."""
    rs = np.random.RandomState(200 + nclass + seed)
    p = np.full((N_CLIPS, T, nclass), 0.1, np.float32)
    for f in range(N_CLIPS):
        for c in range(nclass):
            for _ in range(rs.randint(1, 4)):
                a = rs.randint(0, T - 3)
                p[f, a:a + rs.randint(3, 25), c] = 0.8
    p += rs.uniform(-0.3, 0.3, size=p.shape).astype(np.float32)
    p[1] = 0.05
    return p


def decoded(post, thr, win):
    files, labels = names(post.shape[0], post.shape[2])
    return se.columns_from_rows(pp.predictions(post, files, labels, PTR, SR, HOP, np.float32(thr), win), files, labels)


def decoded_case(nclass):
    """(posteriors, ref_cols, [est_cols per operating point]): the references are the window-7 decode, jittered, a third of
    them relabelled."""
    post = posteriors(nclass)
    rs = np.random.RandomState(300 + nclass)
    base = decoded(post, 0.5, 7)
    ref = [[sorted(col) for col in estimate_of(f, rs, nclass, 8.0, p_extra=0.1)] for f in base]
    ref = [[[(max(0.0, a), b) for a, b in col] for col in f] for f in ref]
    return post, ref, [decoded(post, t, w) for t, w in POINTS]


def chain_case(n_ref, n_est=64, nclass=16):
    """3 clips; clip 1 holds ONE merged cluster of ``n_ref`` references and ``n_est`` estimated events spread over the 16
    classes (at most 5 per column): onsets 10 ms apart.  Clips 0 and 2 are ordinary."""
    ref, est = clip_events(nclass, seed=7)
    ref[1] = [[(1.0 + 0.01 * k, 2.0 + 0.01 * k) for k in range(n_ref) if k % nclass == c] for c in range(nclass)]
    est[1] = [[(1.005 + 0.01 * k, 2.0 + 0.01 * k) for k in range(n_est) if (k + 3) % nclass == c] for c in range(nclass)]
    return ref, est


# ---- long recordings --------------------------------------------------------------------------------------------------------
LONG_CLASSES = 4


def long_events(tile=64, seed=0):
    """(ref_cols, est_cols), 3 recordings x 4 classes.  Recording 0: a class-0 column of 300 references, classes 1 and 2
    empty, class 3 with references whose onsets EQUAL onsets of class 0 and estimated events relabelled across the two.
    Recording 1: empty.  Recording 2: class 0 is ``tile_edge_column`` (references ``tile - 3 .. tile + 2`` within 0.05 s of
    each other) and every other class starts later, so that this cluster straddles the merged tile edge as well."""
    rs = np.random.RandomState(400 + seed)
    r0, e0 = ls.spaced_column(rs, 300)
    r3 = [(on, on + 0.7) for on, _ in r0[10:200:9]]                   # equal onsets across classes
    e3 = [(on + 0.05, off) for on, off in r3[::2]]
    moved = e0[5::7]                                                  # class-0 detections reported as class 3: substitutions
    e0 = [e for i, e in enumerate(e0) if i % 7 != 5]
    rec0 = ([r0, [], [], r3], [e0, [], [], sorted(e3 + moved)])
    rec1 = ([[] for _ in range(LONG_CLASSES)], [[] for _ in range(LONG_CLASSES)])
    r, e = ls.tile_edge_column(rs, tile, 2 * tile + 20)
    late = r[-1][0] + 5.0
    others_r, others_e = [], []
    for c in range(1, LONG_CLASSES):
        a, b = ls.spaced_column(rs, 20 if c != 2 else 0)
        others_r.append([(on + late, off + late) for on, off in a])
        others_e.append([(on + late, off + late) for on, off in b])
    swap = others_e[0][::3]                                           # class-1 detections reported as class 3
    others_e[0] = [x for i, x in enumerate(others_e[0]) if i % 3 != 0]
    others_e[2] = sorted(others_e[2] + swap)
    rec2 = ([r] + others_r, [e] + others_e)
    ref = [rec0[0], rec1[0], rec2[0]]
    est = [rec0[1], rec1[1], rec2[1]]
    return ref, est


def sweep_events(K, tile=64):
    """(ref_cols, [est_cols] * K): point k drops every (k + 2)-th estimated event of ``long_events`` and shifts the rest by
    k ms."""
    ref, est = long_events(tile)
    ests = [[[[(on + 0.001 * k, off) for i, (on, off) in enumerate(col) if i % (k + 2) != 0] for col in f] for f in est]
            for k in range(K)]
    return ref, ests


NUM, DEN = 8.0, 44100 / 511


def frame_table(seed=5):
    """A decoded-style table: (ev_ptr int64 [3 * 4 + 1], ev_pairs int32 [n, 2]) of frames, columns sorted and disjoint as a
    run-length decode leaves them, one column of a few hundred events; and its columns in seconds, the host's doubles."""
    rs = np.random.RandomState(seed)
    cols, ptr, pairs = [], [0], []
    for r in range(3):
        file_cols = []
        for c in range(LONG_CLASSES):
            n = 0 if r == 1 or c == 2 else (400 if (r, c) == (0, 0) else int(rs.randint(5, 40)))
            gaps = rs.randint(4, 30, size=2 * n)                      # >= 4 frames of 0.093 s between edges: small clusters
            edges = np.cumsum(gaps)
            col = [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]
            pairs += col
            ptr.append(len(pairs))
            file_cols.append([(a * NUM / DEN, b * NUM / DEN) for a, b in col])
        cols.append(file_cols)
    return np.array(ptr, np.int64), np.array(pairs, np.int32).reshape(-1, 2), cols


def frame_references(cols, seed=6):
    """References for ``frame_table``: its events jittered, dropped, a third relabelled, sorted."""
    rs = np.random.RandomState(seed)
    out = []
    for f in cols:
        moved = estimate_of(f, rs, LONG_CLASSES, 60.0, p_extra=0.05)
        out.append([[(max(0.0, a), b) for a, b in col] for col in moved])
    return [[sorted(col) for col in f] for f in out]


def one_class(cols):
    """The same events relabelled to a single class: cols[file] = [all events sorted by onset]."""
    return [[sorted(ev for col in f for ev in col)] for f in cols]
