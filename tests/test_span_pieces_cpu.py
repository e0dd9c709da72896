"""CPU tests of span-tag training in pieces: the plan (longrec.span_pieces) - every span in one piece, no batch above
max_windows, a piece's windows exactly those that cover its spans, maximal pieces, the packing of short recordings unchanged, the
refusal of a span too wide -, the plain-loop statement of the piece entries (tests/span_pieces_np.py) against the whole
recording's statements bit for bit and against central finite differences, and the host argument checks of
train.train_span_tags / train.span_tag_plan with split_long."""
import numpy as np
import pytest

from tests import span_pieces_np as pn
from tests import span_tags_bwd_np, span_tags_np, stitch_np
from tests.weak_np import attention

T3 = 8
HOPS = [3, 4, 8]
SPANS = [1, 3, 5, 8, 13]
WINDOWS = [1, 2, 7, 23]
TILE = 512                       # sed_stitch_tile_frames() (tests/test_gpu_span_pieces.py asserts it)


def lengths(hop3, windows=WINDOWS):
    """L3 of recordings with the given window counts whose last window is short (it reaches one frame beyond the end)."""
    L3s = [5 if n == 1 else T3 + (n - 1) * hop3 - 1 for n in windows]
    assert [pn.n_windows(L, T3, hop3) for L in L3s] == list(windows)
    return L3s


def min_windows(n_ws, L3s, hop3, span3):
    """The fewest max_windows the plan accepts: the most windows any one span of any recording needs (a recording that fits
    is not split, and one that does not needs every span of its own to fit)."""
    need = 0
    for n_w, L3 in zip(n_ws, L3s):
        for s in range(-(-L3 // span3)):
            need = max(need, pn.cover_hi(min((s + 1) * span3, L3) - 1, n_w, hop3) - pn.cover_lo(s * span3, T3, hop3) + 1)
    return need


def plan_cases():
    out = []
    for hop3 in HOPS:
        for span3 in SPANS:
            lo = min_windows(WINDOWS, lengths(hop3), hop3, span3)
            out += [(hop3, span3, m, list(WINDOWS)) for m in sorted({lo, 4, 6})]
    out.append((4, TILE + 1, 140, [300]))
    return out


def test_the_restated_cover_functions_are_the_loops():
    from dcase2019_task4_amd.longrec import cover_hi, cover_lo
    for hop3 in (1, 3, 4, 8):
        for n_w in (1, 2, 7):
            for u in range(T3 + (n_w - 1) * hop3):
                cover = [j for j in range(n_w) if 0 <= u - j * hop3 < T3]
                assert cover == list(range(cover_lo(u, T3, hop3), cover_hi(u, n_w, hop3) + 1)), (hop3, n_w, u)
                assert (cover[0], cover[-1]) == (pn.cover_lo(u, T3, hop3), pn.cover_hi(u, n_w, hop3))


@pytest.mark.parametrize("hop3,span3,max_windows,windows", plan_cases())
def test_plan_properties(hop3, span3, max_windows, windows):
    from dcase2019_task4_amd.longrec import cover_hi, cover_lo, recording_tag_runs, span_piece_tables, span_pieces
    L3s = lengths(hop3, windows)
    if max_windows < min_windows(windows, L3s, hop3, span3):
        with pytest.raises(ValueError, match=r"alone needs \d+ windows"):
            span_pieces(windows, L3s, T3, hop3, span3, max_windows)
        return
    batches = span_pieces(windows, L3s, T3, hop3, span3, max_windows)
    seen = {}
    for batch in batches:
        assert sum(p.j1 - p.j0 + 1 for p in batch) <= max_windows
        for p in batch:
            n_w, L3 = windows[p.rec], L3s[p.rec]
            n_spans = -(-L3 // span3)
            assert 0 <= p.s0 < p.s1 <= n_spans and 0 <= p.j0 <= p.j1 < n_w
            for s in range(p.s0, p.s1):
                seen[(p.rec, s)] = seen.get((p.rec, s), 0) + 1
            # the tables of the piece, and its spans inside it
            assert p.off == p.s0 * span3 - p.j0 * hop3 and p.L3 == min(L3, p.j1 * hop3 + T3) - p.j0 * hop3
            assert p.off >= 0 and p.off + (p.s1 - p.s0 - 1) * span3 < p.L3
            assert (p.j1 - p.j0) * hop3 + T3 >= p.L3                              # the piece's windows cover its local frames
            if p.s1 == n_spans:
                assert p.j1 == n_w - 1 and p.L3 == L3 - p.j0 * hop3
            # every frame of its spans: the same covering windows in the piece as in the whole recording
            for u in range(p.s0 * span3, min(p.s1 * span3, L3)):
                whole = range(cover_lo(u, T3, hop3), cover_hi(u, n_w, hop3) + 1)
                ul = u - p.j0 * hop3
                assert 0 <= ul < p.L3
                local = range(p.j0 + cover_lo(ul, T3, hop3), p.j0 + cover_hi(ul, p.j1 - p.j0 + 1, hop3) + 1)
                assert whole == local and len(whole) >= 1, (p, u)
            if n_w <= max_windows:                                                 # a short recording is never split
                assert (p.s0, p.s1, p.j0, p.j1, p.off, p.L3) == (0, n_spans, 0, n_w - 1, 0, L3)
            else:
                assert len(batch) == 1
                if p.s1 < n_spans:                                                 # maximal: the next span would not fit
                    hi = cover_hi(min((p.s1 + 1) * span3, L3) - 1, n_w, hop3)
                    assert hi - p.j0 + 1 > max_windows
    assert seen == {(r, s): 1 for r, L3 in enumerate(L3s) for s in range(-(-L3 // span3))}
    # the long recordings' pieces are the statement's own greedy loop; batches come in recording and span order
    for r, (n_w, L3) in enumerate(zip(windows, L3s)):
        if n_w > max_windows:
            mine = [tuple(b[0])[1:] for b in batches if b[0].rec == r]
            assert mine == pn.pieces_of(n_w, L3, T3, hop3, span3, max_windows)
    # short recordings between long ones are packed as recording_tag_runs packs them
    short = [r for r, n in enumerate(windows) if n <= max_windows]
    if short and short == list(range(short[0], short[-1] + 1)):
        runs = recording_tag_runs([windows[r] for r in short], max_windows)
        assert [[p.rec for p in b] for b in batches if b[0].rec in short] == [list(range(short[0] + a, short[0] + b)) for a, b in runs]
    # the tables: contiguous windows and span rows of the set
    win0 = np.r_[0, np.cumsum(windows)]
    span0 = span_tags_np.span_table(L3s, span3)
    rows = []
    for b in batches:
        w, f, s, off, w_first, n_win, g_first, n_rows = span_piece_tables(b, win0, span0)
        assert w.dtype == np.int32 and f.dtype == np.int64 and s.dtype == np.int64 and off.dtype == np.int32
        assert w[-1] == n_win <= max_windows and s[-1] == n_rows and len(off) == len(b)
        assert w_first == win0[b[0].rec] + b[0].j0 and g_first == span0[b[0].rec] + b[0].s0
        rows += list(range(g_first, g_first + n_rows))
    assert rows == list(range(int(span0[-1])))


@pytest.mark.parametrize("max_windows", [4, 6, 23])
def test_without_a_long_recording_the_batches_are_recording_tag_runs(max_windows):
    from dcase2019_task4_amd.longrec import recording_tag_runs, span_pieces
    windows = [1, 2, 3, 1, 4, 2, 2, 3][:8 if max_windows >= 4 else 4]
    for hop3 in HOPS:
        L3s = lengths(hop3, windows)
        for span3 in SPANS:
            batches = span_pieces(windows, L3s, T3, hop3, span3, max_windows)
            runs = recording_tag_runs(windows, max_windows)
            assert [(b[0].rec, b[-1].rec + 1) for b in batches] == runs
            for b in batches:
                for p in b:
                    assert p == (p.rec, 0, -(-L3s[p.rec] // span3), 0, windows[p.rec] - 1, 0, L3s[p.rec])


def test_a_span_too_wide_and_bad_arguments_raise():
    from dcase2019_task4_amd.longrec import span_pieces
    L3s = lengths(3)
    with pytest.raises(ValueError, match="span 1 of recording 2 alone needs 4 windows, more than max_windows = 2"):
        span_pieces(WINDOWS, L3s, T3, 3, 5, 2)
    assert span_pieces(WINDOWS, L3s, T3, 3, 5, min_windows(WINDOWS, L3s, 3, 5))
    for kw in (dict(max_windows=0), dict(hop3=0), dict(hop3=9), dict(span3=0)):
        a = dict(hop3=3, span3=5, max_windows=4)
        a.update(kw)
        with pytest.raises(ValueError):
            span_pieces(WINDOWS, L3s, T3, a["hop3"], a["span3"], a["max_windows"])
    with pytest.raises(ValueError, match="do not cover"):
        span_pieces([1, 2], [5, 30], T3, 3, 5, 4)
    with pytest.raises(ValueError):
        span_pieces([1, 0], [5, 8], T3, 3, 5, 4)


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _recording(hop3, weighting, n_w, NC, seed=0):
    L3 = lengths(hop3, [n_w])[0]
    rs = np.random.RandomState(700 + 10 * hop3 + weighting + seed)
    p = rs.uniform(0.02, 0.98, size=(n_w, T3, NC)).astype(np.float32)
    a = attention(rs, n_w, T3, NC)
    return L3, p, a, rs


def _whole(hop3, weighting, n_w, NC, span3):
    L3, p, a, rs = _recording(hop3, weighting, n_w, NC)
    w0, f0 = np.array([0, n_w], np.int32), np.array([0, L3], np.int64)
    P, A = stitch_np.blend(p, w0, f0, hop3, weighting), stitch_np.blend(a, w0, f0, hop3, weighting)
    tags, sums, span0 = span_tags_np.pool_timelines(P, A, f0, span3)
    return L3, p, a, rs, w0, f0, (P, A), tags, sums, span0


@pytest.mark.parametrize("span3", SPANS)
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3,NC", [(3, 10), (4, 8), (8, 3)])
def test_statement_of_the_pieces_is_the_whole_recording_bit_for_bit(hop3, NC, weighting, span3):
    """Recordings of 7 and 23 windows in pieces at the fewest windows the plan accepts, 4 and 6: tags and sums of every piece are
    the whole recording's rows; every window element of the recording belongs to the spans of exactly one piece; the
    element-wise sum of the pieces' backwards, each on its own rows of g, is the whole backward."""
    for n_w in (7, 23):
        L3, p, a, rs, w0, f0, blends, tags, sums, span0 = _whole(hop3, weighting, n_w, NC, span3)
        g = rs.standard_normal(tags.shape).astype(np.float32)
        ds, da = span_tags_bwd_np.backward(p, a, w0, f0, hop3, weighting, span3, g, sums=sums, blends=blends)
        lo = min_windows([n_w], [L3], hop3, span3)
        for max_windows in sorted({lo, 4, 6}):
            if max_windows < lo or max_windows >= n_w:
                continue
            pieces = pn.pieces_of(n_w, L3, T3, hop3, span3, max_windows)
            assert len(pieces) >= 2
            owners = np.zeros((n_w, T3), np.int64)
            sum_s, sum_a = np.zeros_like(ds), np.zeros_like(da)
            for piece in pieces:
                s0, s1, j0, j1, off, L3p = piece
                t = pn.piece_tables(piece)
                pt, ps = pn.pool(p[j0:j1 + 1], a[j0:j1 + 1], *t, hop3, weighting, span3)
                assert pt.tobytes() == tags[s0:s1].tobytes() and ps.tobytes() == sums[s0:s1].tobytes(), piece
                bs, ba = pn.backward(p[j0:j1 + 1], a[j0:j1 + 1], *t, hop3, weighting, span3, g[s0:s1], sums=ps)
                row, _ = pn.frame_rows(*t, T3, hop3, weighting, span3)
                owners[j0:j1 + 1] += row >= 0
                zero = np.zeros(NC, np.float32).tobytes()
                for j, v in zip(*np.nonzero(row < 0)):
                    assert bs[j, v].tobytes() == zero and ba[j, v].tobytes() == zero
                sum_s[j0:j1 + 1] += bs
                sum_a[j0:j1 + 1] += ba
            live, _ = span_tags_bwd_np.frame_rows(w0, f0, T3, hop3, weighting, span3)
            assert (owners == (live >= 0)).all()
            assert (sum_s == ds).all() and (sum_a == da).all() and np.abs(ds).max() > 0


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", HOPS)
def test_piece_backward_is_the_whole_backward_with_g_zeroed_outside_the_piece(hop3, weighting):
    """The 23-window recording, span3 = 5, at the fewest windows the plan accepts, 4 and 6 (those of them it accepts)."""
    n_w, NC, span3 = 23, 3, 5
    L3, p, a, rs, w0, f0, blends, tags, sums, span0 = _whole(hop3, weighting, n_w, NC, span3)
    lo = min_windows([n_w], [L3], hop3, span3)
    g = rs.standard_normal(tags.shape).astype(np.float32)
    pieces = [piece for m in sorted({lo, 4, 6}) if m >= lo for piece in pn.pieces_of(n_w, L3, T3, hop3, span3, m)]
    assert len(pieces) > 6
    for piece in pieces:
        s0, s1, j0, j1, off, L3p = piece
        gz = np.zeros_like(g)
        gz[s0:s1] = g[s0:s1]
        ws, wa = span_tags_bwd_np.backward(p, a, w0, f0, hop3, weighting, span3, gz, sums=sums, blends=blends)
        bs, ba = pn.backward(p[j0:j1 + 1], a[j0:j1 + 1], *pn.piece_tables(piece), hop3, weighting, span3, g[s0:s1])
        assert (bs == ws[j0:j1 + 1]).all() and (ba == wa[j0:j1 + 1]).all(), piece
        assert not ws[:j0].any() and not ws[j1 + 1:].any() and not wa[:j0].any() and not wa[j1 + 1:].any()


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", HOPS)
def test_statement_of_a_piece_matches_central_finite_differences(hop3, weighting):
    """One inner piece (frames in front of its first span and behind its last) of the 23-window recording, span3 = 5,
    max_windows 6: d/dx of sum(g * tags) by central differences of the all-float64 pooling (step 1e-6) against the statement,
    per element within tests/test_span_tags_bwd_cpu.py's bound 5e-6 |fd| + 1e-9 + 2^-22 |g[row, c]| (w / W) / den[row, c]."""
    n_w, NC, span3 = 23, 3, 5
    L3, p, _, rs = _recording(hop3, weighting, n_w, NC, seed=3)
    a = rs.uniform(0.05, 1.0, size=p.shape).astype(np.float32)                    # (the attention of the bound's own test)
    pieces = pn.pieces_of(n_w, L3, T3, hop3, span3, 6)
    piece = pieces[1]
    s0, s1, j0, j1, off, L3p = piece
    t = pn.piece_tables(piece)
    x32 = [p[j0:j1 + 1], a[j0:j1 + 1]]
    g = rs.standard_normal((s1 - s0, NC)).astype(np.float32)
    _, sums = pn.pool(x32[0], x32[1], *t, hop3, weighting, span3)
    ds, da = pn.backward(x32[0], x32[1], *t, hop3, weighting, span3, g, sums=sums)
    x = [x32[0].astype(np.float64), x32[1].astype(np.float64)]
    g64 = g.astype(np.float64)

    def loss():
        return float((g64 * pn.forward64(x[0], x[1], *t, hop3, weighting, span3)).sum())

    h = 1e-6
    fd = [np.zeros(x[0].shape), np.zeros(x[0].shape)]
    for k in range(2):
        for i in np.ndindex(*x[k].shape):
            keep = x[k][i]
            x[k][i] = keep + h
            up = loss()
            x[k][i] = keep - h
            dn = loss()
            x[k][i] = keep
            fd[k][i] = (up - dn) / (2 * h)
    row, share = pn.frame_rows(*t, T3, hop3, weighting, span3)
    live = row >= 0
    assert (~live).any() and live.any()
    extra = np.zeros(x[0].shape)
    extra[live] = 2.0 ** -22 * np.abs(g64[row[live]]) * share[live][:, None] / sums[row[live], :, 1]
    for name, got, want in (("d_win_strong", ds, fd[0]), ("d_win_att", da, fd[1])):
        bound = 5e-6 * np.abs(want) + 1e-9 + extra
        ratio = np.abs(got - want) / bound
        print(f"hop3 {hop3} weighting {weighting} {name}: max|statement - fd| {float(np.abs(got - want).max()):.3e}, worst element "
              f"at {float(ratio.max()):.2f} of the bound")
        assert (np.abs(got - want) <= bound).all(), name
        assert (want[~live] == 0).all() and not got[~live].any()


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def _long_set():
    from dcase2019_task4_amd.longrec import LongRecordingSet
    rs = np.random.RandomState(0)
    feats = [rs.standard_normal((n, 4)).astype(np.float32) for n in (64, 96, 128, 64, 248, 96)]
    s = LongRecordingSet.from_arrays(feats, 64, hop_frames=32, device="cpu")
    assert list(np.diff(s.rec_win0_host)) == [1, 2, 3, 1, 7, 2] and (s.T3, s.hop3) == (8, 4)
    return s


def test_train_span_tags_without_split_long_still_raises_and_argument_errors_are_todays():
    from dcase2019_task4_amd.inference import span_table
    from dcase2019_task4_amd.train import train_span_tags
    s = _long_set()
    total = span_table(s, 4)[2]
    ok = np.zeros((total, 10), np.float32)
    for kw in (dict(), dict(split_long=False)):
        with pytest.raises(ValueError, match="recording 4 has 7 windows, more than max_windows = 4"):
            train_span_tags(s, ok, None, None, 0, span3=4, max_windows=4, **kw)
    for split in (False, True):
        with pytest.raises(ValueError, match="LongRecordingSet"):
            train_span_tags([1, 2], ok, None, None, 0, span3=4, split_long=split)
        with pytest.raises(ValueError, match="exactly one of tag_span"):
            train_span_tags(s, ok, None, None, 0, split_long=split)
        with pytest.raises(ValueError, match="span3 must be"):
            train_span_tags(s, ok, None, None, 0, span3=0, split_long=split)
        with pytest.raises(ValueError, match=f"total_spans = {total}"):
            train_span_tags(s, ok[:-1], None, None, 0, span3=4, split_long=split)
        bad = ok.copy()
        bad[3, 2] = 1.5
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            train_span_tags(s, bad, None, None, 0, span3=4, split_long=split)
        with pytest.raises(ValueError, match="no known target"):
            train_span_tags(s, np.full_like(ok, np.nan), None, None, 0, span3=4, max_windows=8, split_long=split)
    with pytest.raises(ValueError, match="alone needs 2 windows, more than max_windows = 1"):
        train_span_tags(s, ok, None, None, 0, span3=4, max_windows=1, split_long=True)


def test_the_split_plan_counts_known_pairs_per_piece_and_reports_the_forwarded_windows():
    from dcase2019_task4_amd.inference import span_table
    from dcase2019_task4_amd.longrec import span_pieces
    from dcase2019_task4_amd.train import span_tag_plan
    s = _long_set()
    host, _, total, span3 = span_table(s, 4)
    t = np.random.RandomState(1).uniform(0, 1, size=(total, 10)).astype(np.float32)
    with pytest.raises(ValueError, match="T3 and hop3"):
        span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 4, 4, split_long=True)
    plan = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 4, 4, split_long=True, T3=s.T3, hop3=s.hop3)
    batches = span_pieces(np.diff(s.rec_win0_host), np.diff(s.rec_frame0_host), s.T3, s.hop3, 4, 4)
    assert plan["runs"] == batches and plan["rec_span0"].tolist() == host.tolist()
    long_ones = [k for k, b in enumerate(batches) if b[0].rec == 4]
    assert len(long_ones) >= 2 and all(len(batches[k]) == 1 for k in long_ones)
    forwarded = sum(p.j1 - p.j0 + 1 for b in batches for p in b)
    assert plan["forwarded_windows"] == forwarded > s.n_clips and plan["forwarded"] == forwarded / s.n_clips
    assert plan["counts"].sum() == t.size and plan["ran"] == list(range(len(batches)))
    # NaN targets that empty one piece skip exactly that batch
    k = long_ones[1]
    piece = batches[k][0]
    t[host[4] + piece.s0:host[4] + piece.s1] = np.nan
    plan = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 4, 4, split_long=True, T3=s.T3, hop3=s.hop3)
    assert plan["counts"][k] == 0 and plan["ran"] == [i for i in range(len(batches)) if i != k]
    # without a long recording the split plan is today's plan
    a = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 8, 4)
    b = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 8, 4, split_long=True, T3=s.T3, hop3=s.hop3)
    assert [(x[0].rec, x[-1].rec + 1) for x in b["runs"]] == a["runs"] and b["counts"].tolist() == a["counts"].tolist()
    assert b["forwarded"] == 1.0
    # the set's cached tables are the plan's batches
    tb = s.span_tag_batches(4, 4)
    assert tb["batches"] == batches and tb is s.span_tag_batches(4, 4) and tb["forwarded"] == forwarded / s.n_clips
    for k, b in enumerate(batches):
        lo, hi = tb["at"][k], tb["at"][k + 1]
        assert tb["rec_win0"][lo:hi].tolist() == tb["tables"][k][0].tolist() and len(tb["tables"][k][0]) == len(b) + 1
        assert tb["rec_span_off"][lo:hi - 1].tolist() == [p.off for p in b]
        assert tb["rec_frame0"][lo:hi].tolist() == np.r_[0, np.cumsum([p.L3 for p in b])].tolist()
        assert tb["rec_span0"][lo:hi].tolist() == np.r_[0, np.cumsum([p.s1 - p.s0 for p in b])].tolist()
