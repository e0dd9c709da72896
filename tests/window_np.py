"""Plain-loop statement of training windows over long pool items (longrec.WindowedFeatureSet,
sed_gather_window_logmel_transform): how many windows an item contributes, where they start, and what a window's features
and target are.  Written from the definitions in include/dcase_sed.h and DESIGN.md, sharing no code with the library."""
import numpy as np


def label_frames(L, pool):
    """L3: the label frames of an item of L feature frames (frames that exist only as padding are not labelled)."""
    return max(1, int(L) // int(pool))


def start_hi(L, frames, pool):
    """The last legal start3 of an item: max(0, L3 - T3)."""
    return max(0, label_frames(L, pool) - int(frames) // int(pool))


def n_windows(L, frames, pool, hop3):
    """Windows a windowed item contributes per epoch: the grid j * hop3 until a window reaches the item's last label frame."""
    L3, T3 = label_frames(L, pool), int(frames) // int(pool)
    n = 1
    while (n - 1) * hop3 + T3 < L3:
        n += 1
    return n


def item_starts(lengths, item_windowed, frames, pool, hop3, sampling, seed, epoch):
    """start3 of every window of every item, a list of lists in item order.  A non-windowed item has the one window at 0."""
    rng = np.random.default_rng([seed, epoch])
    out = []
    for L, w in zip(lengths, item_windowed):
        if not w:
            out.append([0])
            continue
        hi, n = start_hi(L, frames, pool), n_windows(L, frames, pool, hop3)
        if sampling == "grid":
            out.append([min(j * hop3, hi) for j in range(n)])
        else:
            out.append([int(v) for v in rng.integers(0, hi + 1, size=n)])
    return out


def cut_window(features, labels, start3, frames, pool):
    """(feature rows [s, s + n), target [T3, nclass]) of the window at label frame start3: s = start3 * pool,
    n = min(frames, L - s); target row u is timeline row start3 + u, 0.0 beyond the timeline."""
    features, labels = np.asarray(features, dtype=np.float32), np.asarray(labels, dtype=np.float32)
    T3 = int(frames) // int(pool)
    s = int(start3) * int(pool)
    n = min(int(frames), features.shape[0] - s)
    assert 0 <= s < features.shape[0] and n >= 1
    target = np.zeros((T3, labels.shape[1]), dtype=np.float32)
    for u in range(T3):
        if start3 + u < labels.shape[0]:
            for c in range(labels.shape[1]):
                target[u, c] = labels[start3 + u, c]
    return features[s:s + n].copy(), target
