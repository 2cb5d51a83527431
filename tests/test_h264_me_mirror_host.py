"""Keeps tests/h264_me_mirror.py honest without a GPU.

The mirror is what tests/test_gpu_h264_me.py holds the GPU motion search
to, so it must not be a transcription of the kernel: its primitives are
checked against brute-force loops, planted translations must come back
exactly through each search pass, vectors must never leave the stripe,
and the hopeless life-cycle is walked frame by frame. The last test
guards the coverage of h264_content.me_frames with the previous source
frame standing in for the reconstructed reference."""

import functools

import numpy as np
import pytest

import h264_me_mirror as mm
from h264_content import (TIE_COLUMNS, bgrx_to_planes, me_frames, tex,
                          tie_frames)
from h264_me_mirror import INTER, INTRA, SKIP, MeMirror
from h264_ref_decoder import luma_mc

QP = 30


@functools.lru_cache(maxsize=None)
def big_plane(seed=3, size=320):
    """One textured plane, built once and never modified."""
    p = tex(np.random.default_rng(seed), size, size)[:, :, 0]
    p.setflags(write=False)
    return p


def shifted_pair(W, H, dx, dy, org=96):
    """(src, ref) with src[y][x] == ref[y + dy][x + dx]: planted vector
    (dx, dy) in whole samples."""
    big = big_plane()
    ref = big[org:org + H, org:org + W]
    src = big[org + dy:org + dy + H, org + dx:org + dx + W]
    return src, ref


def run_p(W, H, stripe_h, src, ref, qp=QP):
    """IDR on ref, then one P picture src against ref."""
    m = MeMirror(W, H, stripe_h, qp)
    m.encode(ref, None, idr=True)
    out = m.encode(src, ref)
    return m, out


def interior(m, qx, qy, sy0=0, sy1=None):
    """MBs whose interpolation window for (qx, qy) stays inside."""
    sy1 = m.mbh * 16 if sy1 is None else sy1
    return [(x, y) for y in range(m.mbh) for x in range(m.mbw)
            if mm.window_inside(x * 16, y * 16, qx, qy, m.mbw * 16, sy0, sy1)]


# ---- primitives against brute force -----------------------------------------

def test_ssd_sad_match_loops():
    rng = np.random.default_rng(1)
    for _ in range(20):
        a = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        b = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        s2 = s1 = 0
        for y in range(16):
            for x in range(16):
                d = int(a[y, x]) - int(b[y, x])
                s2 += d * d
                s1 += abs(d)
        assert mm.ssd(a, b) == s2
        assert mm.sad(a, b) == s1
    # the extremes: no wrap in uint8
    lo, hi = np.zeros((16, 16), np.uint8), np.full((16, 16), 255, np.uint8)
    assert mm.ssd(lo, hi) == 256 * 255 * 255
    assert mm.sad(hi, lo) == 256 * 255


@pytest.mark.parametrize("w,h", [(250, 90), (36, 20), (20, 3), (3, 20),
                                 (64, 32)])
def test_padded_source_and_pyramid_match_loops(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    pad = mm.padded_source(src, mbw, mbh)
    assert pad.shape == (mbh * 16, mbw * 16)
    for y in range(mbh * 16):
        for x in range(mbw * 16):
            assert pad[y, x] == src[min(y, h - 1), min(x, w - 1)]
    pyr = mm.pyramid(pad)
    assert pyr.shape == (mbh * 4, mbw * 4)

    def level1(y, x):
        return (int(pad[2 * y, 2 * x]) + int(pad[2 * y, 2 * x + 1])
                + int(pad[2 * y + 1, 2 * x]) + int(pad[2 * y + 1, 2 * x + 1])
                + 2) >> 2

    for y in range(mbh * 4):
        for x in range(mbw * 4):
            want = (level1(2 * y, 2 * x) + level1(2 * y, 2 * x + 1)
                    + level1(2 * y + 1, 2 * x) + level1(2 * y + 1, 2 * x + 1)
                    + 2) >> 2
            assert pyr[y, x] == want
    # the proxy: clamp to the last quarter sample inside the picture,
    # never below sample 0
    rmax, cmax = max(0, (h >> 2) - 1), max(0, (w >> 2) - 1)
    for mby in range(mbh):
        for mbx in range(mbw):
            P = mm.source_proxy(pyr, w, h, mbx, mby)
            for r in range(4):
                for c in range(4):
                    assert P[r, c] == pyr[min(mby * 4 + r, rmax),
                                          min(mbx * 4 + c, cmax)]
    # every proxy sample is a function of the picture alone: samples whose
    # footprint lies inside the picture equal the plain average there
    for y in range(h >> 2):
        for x in range(w >> 2):
            blk = src[4 * y:4 * y + 4, 4 * x:4 * x + 4].astype(int)
            l1 = [(blk[2 * j:2 * j + 2, 2 * i:2 * i + 2].sum() + 2) >> 2
                  for j in range(2) for i in range(2)]
            assert pyr[y, x] == (sum(l1) + 2) >> 2


def test_grid_order_and_validity():
    vs = mm.grid_vectors(6, -4)
    assert len(vs) == len(set(vs)) == 81
    assert vs[0] == (-2, -12) and vs[1] == (0, -12) and vs[9] == (-2, -10)
    assert vs[40] == (6, -4) and vs[80] == (14, 4)
    # validity is the block inside [0, W) x [sy0, sy1)
    assert mm.block_inside(16, 48, -16, 0, 64, 48, 96)
    assert not mm.block_inside(16, 48, -17, 0, 64, 48, 96)
    assert not mm.block_inside(16, 48, 0, -1, 64, 48, 96)
    assert mm.block_inside(16, 48, 32, 32, 64, 48, 96)
    assert not mm.block_inside(16, 48, 33, 32, 64, 48, 96)
    assert not mm.block_inside(16, 48, 32, 33, 64, 48, 96)


def brute_grid(S, ref, x0, y0, cx, cy, W, sy0, sy1, best):
    """score_grid by an independent loop: index order, strict '<'."""
    for idx in range(81):
        mx, my = cx + (idx % 9 - 4) * 2, cy + (idx // 9 - 4) * 2
        if x0 + mx < 0 or x0 + mx + 16 > W:
            continue
        if y0 + my < sy0 or y0 + my + 16 > sy1:
            continue
        s = 0
        for y in range(16):
            for x in range(16):
                d = int(S[y, x]) - int(ref[y0 + my + y, x0 + mx + x])
                s += d * d
        s += 4 * (abs(mx) + abs(my))
        if s < best[0]:
            best = (s, mx, my)
    return best


def test_score_grid_matches_brute_force_at_edges():
    src, ref = shifted_pair(64, 64, 3, -5)
    ref = ref.astype(np.int64)
    for x0, y0, cx, cy, sy0, sy1 in [(0, 0, 0, 0, 0, 64), (48, 48, 0, 0, 0, 64),
                                     (16, 32, -12, 8, 32, 64),
                                     (32, 16, 20, -20, 0, 48)]:
        S = src[y0:y0 + 16, x0:x0 + 16]
        best = (mm.NO_SCORE, 0, 0)
        assert mm.score_grid(S, ref, x0, y0, cx, cy, 64, sy0, sy1, best) == \
            brute_grid(S, ref, x0, y0, cx, cy, 64, sy0, sy1, best)
    # a carried best that nothing beats stays
    S = src[16:32, 16:32]
    assert mm.score_grid(S, ref, 16, 16, 0, 0, 64, 0, 64, (0, 5, 5)) == \
        (0, 5, 5)


def test_grid_tie_goes_to_first_in_index_order():
    """Columns of period 4, source = reference shifted by 2: vectors
    (-2, 0) and (2, 0) both have SSD 0 and the same bias. Index order has
    mx ascending inside my, and only a strictly smaller score wins, so
    (-2, 0) must be chosen."""
    col = np.array([40, 90, 200, 150] * 16)
    ref = np.tile(col, (64, 1)).astype(np.int64)
    src = np.roll(ref, -2, axis=1)
    S = src[16:32, 16:32]
    best = mm.score_grid(S, ref, 16, 16, 0, 0, 64, 0, 64, (mm.NO_SCORE, 0, 0))
    assert best == (8, -2, 0)
    # rows of period 4: (0, -2) precedes (0, 2)
    best = mm.score_grid(S.T, ref.T, 16, 16, 0, 0, 64, 0, 64,
                         (mm.NO_SCORE, 0, 0))
    assert best == (8, 0, -2)


def test_pyramid_seed_matches_brute_force_and_tie_rule():
    rng = np.random.default_rng(5)
    ref2 = rng.integers(0, 256, (16, 40)).astype(np.int64)
    for qx0, qy0, qsy0, qsy1 in [(0, 0, 0, 16), (36, 12, 0, 16),
                                 (16, 4, 4, 12), (20, 8, 0, 16)]:
        P = rng.integers(0, 256, (4, 4)).astype(np.int64)
        best = None
        for my in range(-12, 13):
            for mx in range(-12, 13):
                if not (0 <= qx0 + mx and qx0 + mx + 4 <= 40
                        and qsy0 <= qy0 + my and qy0 + my + 4 <= qsy1):
                    continue
                s = sum(abs(int(P[r, c]) - int(ref2[qy0 + my + r,
                                                     qx0 + mx + c]))
                        for r in range(4) for c in range(4))
                key = (s, my, mx)
                if best is None or key < best:
                    best = key
        assert mm.pyramid_seed(P, ref2, qx0, qy0, 40, qsy0, qsy1) == \
            (best[2], best[1])
    # flat reference: every position ties, the smallest (my, mx) wins
    flat = np.full((16, 40), 7, np.int64)
    assert mm.pyramid_seed(flat[:4, :4], flat, 20, 8, 40, 0, 16) == (-12, -8)
    assert mm.pyramid_seed(flat[:4, :4], flat, 4, 8, 40, 4, 16) == (-4, -4)
    # nothing valid: no seed
    assert mm.pyramid_seed(flat[:4, :4], flat, 0, 0, 40, 0, 3) is None


def test_state_words_round_trip():
    for mode, hint, hopeless, mv in [(INTER, (-12, 3), False, (-49, 13)),
                                     (INTRA, (48, -48), True, (0, 0)),
                                     (SKIP, (0, 0), False, (0, 0)),
                                     (INTER, (60, -60), False, (240, -240))]:
        w0, w1 = mm.pack_words(mode, hint, hopeless, mv)
        assert -2 ** 31 <= w1 < 2 ** 31
        assert w0 & 3 == mode and (w0 >> 22) & 1 == int(hopeless)
        pv = mm.previous_vector(w0, w1)
        want = (mv[0] >> 2, mv[1] >> 2) if mode == INTER else hint
        assert pv == tuple(max(-48, min(48, v)) for v in want)
    # zeroed state is not "no hint": it reads as (-48, -48)
    assert mm.previous_vector(0, 0) == (-48, -48)
    assert mm.previous_vector(INTRA, 0) == (-48, -48)


# ---- planted translations ---------------------------------------------------

def assert_planted(m, out, mbs, qmv, winner=None):
    assert mbs, "no interior MB: the case checks nothing"
    for key in mbs:
        d = m.last[key]
        assert out[key] == (INTER, qmv), (key, out[key], qmv)
        x0, y0 = key[0] * 16, key[1] * 16
        assert d["hint"] == (qmv[0] >> 2, qmv[1] >> 2)
        if winner is not None:
            assert d["winner"] in winner, (key, d["winner"])


@pytest.mark.parametrize("dx,dy", [(2, 4), (-2, 4), (2, -4), (-2, -4),
                                   (7, -8), (3, 1)])
def test_planted_pass1(dx, dy):
    """Vectors inside +-8: the zero-centred grid, and for odd components
    the +-1 ring, which alone can reach them."""
    W, H = 96, 64
    src, ref = shifted_pair(W, H, dx, dy)
    m, out = run_p(W, H, 64, src, ref)
    mbs = interior(m, 4 * dx, 4 * dy)
    assert_planted(m, out, mbs, (4 * dx, 4 * dy), winner=(1,))
    for key in mbs:
        x0, y0 = key[0] * 16, key[1] * 16
        assert mm.sad(src[y0:y0 + 16, x0:x0 + 16],
                      ref[y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16]) == 0


def test_planted_scroll_tracks_through_the_hint():
    """12 px per frame to the right over four frames.
    (a) against the previous source, the true vector is (-12, 0) every
        frame: out of the zero grid's reach, so frame 1 acquires it on the
        pyramid and frames 2 and 3 must win it in pass 2, from the hint.
    (b) against a fixed reference the vector grows to (-36, 0) and the
        hint must follow it there."""
    W, H = 160, 64
    big = big_plane()
    frames = [big[96:96 + H, 96 - 12 * k:96 - 12 * k + W] for k in range(4)]
    m = MeMirror(W, H, 64, QP)
    m.encode(frames[0], None, idr=True)
    for k in (1, 2, 3):
        out = m.encode(frames[k], frames[k - 1])
        mbs = interior(m, -48, 0)
        assert_planted(m, out, mbs, (-48, 0),
                       winner=(3,) if k == 1 else (2,))
    assert m.pass_wins[2] >= 2 * len(mbs) and m.pass_wins[3] >= len(mbs)

    m = MeMirror(W, H, 64, QP)
    m.encode(frames[0], None, idr=True)
    for k in (1, 2, 3):
        out = m.encode(frames[k], frames[0])
        assert_planted(m, out, interior(m, -48 * k, 0), (-48 * k, 0))
    mbs = interior(m, -144, 0)
    for mbx, mby in mbs:
        assert mm.previous_vector(int(m.word0[mby, mbx]),
                                  int(m.word1[mby, mbx])) == (-36, 0)
        assert ((int(m.word0[mby, mbx]) >> 8) & 127) - 64 == -36
        assert ((int(m.word0[mby, mbx]) >> 15) & 127) - 64 == 0


@pytest.mark.parametrize("dx,dy", [(-32, 8), (40, -12)])
def test_planted_cold_jump_needs_the_pyramid(dx, dy):
    """A jump out of reach of both fine grids on the first P picture,
    inside a 64-row stripe: only the quarter-resolution search finds it."""
    W, H = 160, 64
    src, ref = shifted_pair(W, H, dx, dy)
    m, out = run_p(W, H, 64, src, ref)
    mbs = interior(m, 4 * dx, 4 * dy)
    assert_planted(m, out, mbs, (4 * dx, 4 * dy), winner=(3,))
    assert m.pass_wins[3] >= len(mbs)


@pytest.mark.parametrize("qx,qy", [(2, 0), (0, -2), (-2, 2),       # half
                                   (1, 0), (0, 3), (-1, -1), (3, 2)])
def test_planted_fractional(qx, qy):
    """The source is the reference interpolated by luma_mc at (qx, qy), so
    that vector has SAD 0 and must come back."""
    W, H = 96, 64
    _, ref = shifted_pair(W, H, 0, 0)
    ref = ref.astype(np.int64)
    src = ref.copy()
    m0 = MeMirror(W, H, 64, QP)
    mbs = interior(m0, qx, qy)
    mbs = [k for k in mbs if mm.window_inside(k[0] * 16, k[1] * 16, 0, 0,
                                              W, 0, H)]
    for mbx, mby in mbs:
        src[mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = \
            luma_mc(ref, mbx * 16, mby * 16, qx, qy)
    m, out = run_p(W, H, 64, src, ref)
    assert_planted(m, out, mbs, (qx, qy), winner=(1,))


# ---- bounds -----------------------------------------------------------------

OUTWARD = [(-6, 0), (6, 0), (0, -6), (0, 6), (-5, -5), (5, 5), (-5, 5),
           (5, -5), (-20, -8), (20, 8), (-1, 0), (0, 1), (12, -12)]


@pytest.mark.parametrize("dx,dy", OUTWARD)
def test_vectors_never_leave_the_stripe(dx, dy):
    """A 3x3-MB stripe in the middle of a taller picture, every MB, a
    planted vector that points out of it for the MBs of one side: the
    block of a whole-sample vector and the interpolation window of a
    fractional one must stay inside the stripe and the padded width."""
    W, H = 48, 144
    src, ref = shifted_pair(W, H, dx, dy)
    m = MeMirror(W, H, 48, QP)
    m.encode(ref, None, idr=True)
    out = m.encode(src, ref)
    assert len(out) == 27
    inter = 0
    for (mbx, mby), (mode, (qx, qy)) in out.items():
        sy0 = (mby // 3) * 48
        x0, y0 = mbx * 16, mby * 16
        if mode != INTER:
            assert (qx, qy) == (0, 0)
            continue
        inter += 1
        assert mm.block_inside(x0, y0, qx >> 2, qy >> 2, W, sy0, sy0 + 48)
        if (qx | qy) & 3:
            # the 22x22 samples luma_mc reads round the block
            ix, iy = qx >> 2, qy >> 2
            assert x0 + ix - 2 >= 0 and x0 + ix + 20 <= W
            assert y0 + iy - 2 >= sy0 and y0 + iy + 20 <= sy0 + 48
            assert mm.window_inside(x0, y0, qx, qy, W, sy0, sy0 + 48)
    assert inter >= 3, "the case reaches no inter MB"
    # the centre MB of each stripe can hold any vector up to +-14
    if max(abs(dx), abs(dy)) <= 12:
        for s in range(3):
            assert out[(1, 3 * s + 1)] == (INTER, (4 * dx, 4 * dy))


# ---- hopeless life-cycle ----------------------------------------------------

def test_hopeless_life_cycle_one_mb():
    rng = np.random.default_rng(2)
    noise = [rng.integers(0, 256, (16, 16), dtype=np.uint8)
             for _ in range(12)]
    m = MeMirror(16, 16, 16, QP)
    m.encode(noise[0], None, idr=True)                     # frame_num 0
    assert m.words()[0, 0, 0] == INTRA
    # frame_num 1: cold state searches, finds nothing: intra, hopeless
    out = m.encode(noise[1], noise[0])
    d = m.last[(0, 0)]
    assert out[(0, 0)] == (INTRA, (0, 0))
    assert d["searched"] and d["hopeless"] and not d["probe"]
    assert d["score"] > mm.HOPELESS_GATE and d["hint"] == (0, 0)
    assert (m.words()[0, 0, 0] >> 22) & 1 == 1
    # frame_num 2..7: no search pass at all, the bit holds
    for fn in range(2, 8):
        out = m.encode(noise[fn], noise[fn - 1])
        d = m.last[(0, 0)]
        assert out[(0, 0)] == (INTRA, (0, 0)), fn
        assert not d["searched"] and d["score"] == mm.NO_SCORE, fn
        assert d["hopeless"] and not d["probe"], fn
    assert m.probes == 0
    # frame_num 8: the probe
    out = m.encode(noise[8], noise[7])
    d = m.last[(0, 0)]
    assert d["searched"] and d["probe"] and d["hopeless"]
    assert d["score"] < mm.NO_SCORE and m.probes == 1
    # content settles: skip at once (sad(0,0) runs every frame), bit cleared
    out = m.encode(noise[8], noise[8])
    d = m.last[(0, 0)]
    assert out[(0, 0)] == (SKIP, (0, 0))
    assert not d["searched"] and not d["hopeless"]
    assert m.words()[0, 0, 0] == SKIP | (64 << 8) | (64 << 15)
    # and the full search is back on the next frame
    out = m.encode(noise[9], noise[8])
    d = m.last[(0, 0)]
    assert d["searched"] and not d["probe"] and d["hopeless"]
    assert m.hopeless_mbs == 9


def test_idr_rows_and_unencoded_stripes_keep_state():
    """Two stripes; the second is masked out for a frame: its words do not
    change and steer the next search; an IDR row rewrites mode only."""
    W, H = 64, 64
    big = big_plane()
    fr = [big[96:96 + H, 96 - 12 * k:96 - 12 * k + W] for k in range(4)]
    m = MeMirror(W, H, 32, QP)
    m.encode(fr[0], None, idr=True)
    m.encode(fr[1], fr[0])
    before = m.words().copy()
    out = m.encode(fr[2], fr[1], mask=[True, False])
    assert sorted({k[1] for k in out}) == [0, 1]
    assert np.array_equal(m.words()[2:], before[2:])
    assert [s["frame_num"] for s in m.stripes] == [3, 2]
    # late first encode of a stripe: IDR, whatever the frame's own flag
    m2 = MeMirror(W, H, 32, QP)
    m2.encode(fr[0], None, idr=True, mask=[True, False])
    out = m2.encode(fr[1], fr[0])
    assert all(out[(x, y)] == (INTRA, (0, 0)) for x in range(4)
               for y in (2, 3))
    assert all(out[(x, 0)][0] != INTRA for x in range(1, 4))
    assert (m2.words()[2:, :, 0] == INTRA).all()


# ---- coverage guard for the GPU content -------------------------------------

@pytest.mark.parametrize("w,h", [(256, 96), (250, 90)])
def test_me_frames_reach_every_pass(w, h):
    """The previous source frame stands in for the reconstructed
    reference. Floors are conditions on the content: passes 1, 2 and 3
    each win >= 4 MBs, >= 4 hopeless MBs, >= 1 probe, >= 1 odd, half- and
    quarter-sample vector, and at the unaligned width >= 2 pyramid wins
    in the last MB column.
    Counts with this generator (pass1/2/3, last-column pass 3, hopeless,
    probes, odd/half/quarter) are printed; see profiles/NOTES.md."""
    n = 10
    lumas = [bgrx_to_planes(f)[0] for f in me_frames(w, h, n)]
    m = MeMirror(w, h, 48, QP)
    m.encode(lumas[0], None, idr=True)
    for k in range(1, n):
        m.encode(lumas[k], mm.padded_source(lumas[k - 1], m.mbw, m.mbh))
    c = m.coverage()
    print(f"me_frames {w}x{h}: {c}")
    for p in ("pass1", "pass2", "pass3", "hopeless"):
        assert c[p] >= 4, (p, c)
    for p in ("probes", "odd", "half", "quarter"):
        assert c[p] >= 1, (p, c)
    if w % 16:
        assert c["pass3_last_col"] >= 2, c


def test_tie_frames_make_the_order_decide():
    """tie_frames at qp 17 against the exact previous source: in frame 1
    every MB of a -14 column ties (-8, 0) with (8, 0) in the zero grid,
    takes the first and, where the ring has room, ends on (-16, 0); every MB of a
    -48 column is seeded by a tied pyramid minimum. Floors: >= 4 MBs of
    each kind (there are 12 of each)."""
    w, h = 256, 96
    lumas = [bgrx_to_planes(f)[0] for f in tie_frames(w, h, 3)]
    assert sorted(np.unique(lumas[0])) == [80, 114, 128]
    m = MeMirror(w, h, 48, 17)
    m.encode(lumas[0], None, idr=True)
    out = m.encode(lumas[1], mm.padded_source(lumas[0], m.mbw, m.mbh))
    for c, off in TIE_COLUMNS:
        for mby in range(m.mbh):
            d = m.last[(c, mby)]
            if off == -14:
                assert d["grid_tie"] and d["winner"] == 1
                assert d["score"] == 128 * 14 * 14 + 32
                # only a stripe's middle MB row has room for the ring's
                # interpolation window; the others stay on (-8, 0), whose
                # SAD is over the inter threshold, and keep it as hint
                if mby % 3 == 1:
                    assert out[(c, mby)] == (INTER, (-64, 0))
                else:
                    assert out[(c, mby)] == (INTRA, (0, 0))
                    assert d["hint"] == (-8, 0)
            else:
                assert d["pyramid_tie"] and d["winner"] == 3
                assert out[(c, mby)][0] == INTER
    c = m.coverage()
    print(f"tie_frames {w}x{h}: {c}")
    assert c["grid_ties"] >= 4 and c["pyramid_ties"] >= 4, c
    assert sum(1 for v in out.values() if v[0] == SKIP) == 6 * 12
