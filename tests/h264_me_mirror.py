"""A plain model of the H.264 GPU motion search and mode decision.

Written from the definition of the decision, not from the kernel's data
flow: SSD is a plain integer sum over the 16x16 block, candidates are
enumerated one by one in the order that decides ties, and fractional
samples come from h264_ref_decoder.luma_mc (the spec interpolation the
decoder uses). tests/test_h264_me_mirror_host.py keeps this file honest
without a GPU; tests/test_gpu_h264_me.py holds the GPU to it exactly.

Definitions
-----------
padded source   src[min(y, h-1)][min(x, w-1)] over the MB-aligned plane.
pyramid         two 2x2 box averages with +2 >> 2 of a plane.
source proxy    the 4x4 quarter-resolution block of an MB, read from the
                pyramid of the padded source with rows clamped to
                max(0, (h >> 2) - 1) and columns to max(0, (w >> 2) - 1):
                the last quarter sample whose 4x4 footprint lies inside
                the picture is repeated outward.
score           SSD + 4 * (|mx| + |my|), integer vectors.
grid            the 9x9 vectors centre + 2 * (i - 4, j - 4), visited with
                my outer and mx inner; a strictly smaller score wins; the
                best carries over from grid to grid. A vector is valid
                only if its block lies in [0, mbw*16) x [sy0, sy1).
state           two 32-bit words per MB, as the GPU keeps them:
                word 0 = mode | (hintx + 64) << 8 | (hinty + 64) << 15
                         | hopeless << 22, word 1 = mvx & 0xFFFF | mvy << 16
                (quarter-pel, zero unless the MB is inter).
                All-zero words (a cold start, or an IDR row: mode aside)
                therefore read as hint (-64, -64), clamped to (-48, -48):
                the first P picture after every IDR scores a grid there.
"""

import numpy as np

from h264_ref_decoder import luma_mc

SKIP, INTER, INTRA = 0, 1, 2
PAT = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1), (-1, 1), (1, -1))
NO_SCORE = 2 ** 31 - 1
PYRAMID_GATE = 256 * 180
HOPELESS_GATE = 256 * 1200
# bits of word 0 that the motion search owns: mode, hint and hopeless
WORD0_MASK = 0x3 | 0x7FFF00


# ---- primitives -------------------------------------------------------------

def padded_source(src, mbw, mbh):
    """Edge-replicated picture over the MB-aligned plane."""
    h, w = src.shape
    return np.pad(np.asarray(src, np.int64),
                  ((0, mbh * 16 - h), (0, mbw * 16 - w)), mode="edge")


def box2(p):
    p = np.asarray(p, np.int64)
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            + 2) >> 2


def pyramid(p):
    """Quarter-resolution plane: two box averages."""
    return box2(box2(p))


def source_proxy(pyr, w, h, mbx, mby):
    """4x4 proxy of MB (mbx, mby) from the padded source's pyramid."""
    rmax, cmax = max(0, (h >> 2) - 1), max(0, (w >> 2) - 1)
    rows = np.minimum(np.arange(mby * 4, mby * 4 + 4), rmax)
    cols = np.minimum(np.arange(mbx * 4, mbx * 4 + 4), cmax)
    return pyr[np.ix_(rows, cols)]


def block(plane, x, y, n=16):
    return plane[y:y + n, x:x + n]


def ssd(a, b):
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return int((d * d).sum())


def sad(a, b):
    return int(np.abs(np.asarray(a, np.int64)
                      - np.asarray(b, np.int64)).sum())


def grid_vectors(cx, cy):
    """The 81 vectors of a step-2 grid in visiting order."""
    return [(cx + 2 * (i - 4), cy + 2 * (j - 4))
            for j in range(9) for i in range(9)]


def block_inside(x0, y0, mx, my, W, sy0, sy1):
    return (x0 + mx >= 0 and x0 + mx + 16 <= W
            and y0 + my >= sy0 and y0 + my + 16 <= sy1)


def window_inside(x0, y0, qx, qy, W, sy0, sy1):
    """The interpolation window of a quarter-pel vector: two samples
    before the block, and four after it (the sixth tap plus the x+1 / y+1
    half sample that quarter positions average with)."""
    ix, iy = qx >> 2, qy >> 2
    return (x0 + ix - 2 >= 0 and x0 + ix + 20 <= W
            and y0 + iy - 2 >= sy0 and y0 + iy + 20 <= sy1)


def score_grid(S, ref, x0, y0, cx, cy, W, sy0, sy1, best, seen=None):
    """Visit one grid. best = (score, mx, my); returns the new best.
    `seen`, if given, collects every valid (score, mx, my) visited."""
    for mx, my in grid_vectors(cx, cy):
        if not block_inside(x0, y0, mx, my, W, sy0, sy1):
            continue
        sc = ssd(S, block(ref, x0 + mx, y0 + my)) + 4 * (abs(mx) + abs(my))
        if seen is not None:
            seen.append((sc, mx, my))
        if sc < best[0]:
            best = (sc, mx, my)
    return best


def pyramid_seed(P, ref2, qx0, qy0, qW, qsy0, qsy1, info=None):
    """Exhaustive +-12 SAD of the 4x4 proxy on the quarter-resolution
    reference; minimum wins, ties to the smallest (my, mx). Returns the
    quarter-resolution vector or None when no position is valid.
    `info`, if given, gets info["tied"] = positions sharing the minimum."""
    bs, seed, tied = None, None, 0
    for my in range(-12, 13):
        for mx in range(-12, 13):
            if (qx0 + mx < 0 or qx0 + mx + 4 > qW
                    or qy0 + my < qsy0 or qy0 + my + 4 > qsy1):
                continue
            s = sad(P, block(ref2, qx0 + mx, qy0 + my, 4))
            if bs is None or s < bs:
                bs, seed, tied = s, (mx, my), 1
            elif s == bs:
                tied += 1
    if info is not None:
        info["tied"] = tied
    return seed


def previous_vector(w0, w1):
    """The tracking vector the state words hold, in whole samples."""
    if (w0 & 3) == INTER:
        mvx = ((w1 & 0xFFFF) ^ 0x8000) - 0x8000
        mvy = w1 >> 16
        pvx, pvy = mvx >> 2, mvy >> 2
    else:
        pvx = ((w0 >> 8) & 127) - 64
        pvy = ((w0 >> 15) & 127) - 64
    return max(-48, min(48, pvx)), max(-48, min(48, pvy))


def pack_words(mode, hint, hopeless, mv):
    hx = max(-48, min(48, hint[0])) + 64
    hy = max(-48, min(48, hint[1])) + 64
    w0 = mode | (hx << 8) | (hy << 15) | (int(hopeless) << 22)
    w1 = (mv[0] & 0xFFFF) | ((mv[1] & 0xFFFF) << 16)
    if w1 >= 2 ** 31:
        w1 -= 2 ** 32
    return w0, w1


# ---- one macroblock ---------------------------------------------------------

def decide_mb(S, P, ref, ref2, x0, y0, W, sy0, sy1, qp, frame_num, w0, w1):
    """S: 16x16 padded-source block; P: its 4x4 proxy; ref / ref2: the
    reference plane and its pyramid; (w0, w1): the MB's previous state.

    Returns dict(mode, mv, hint, hopeless, score, winner, probe) where
    winner is the pass (1, 2, 3) whose grid produced the best integer
    vector (0: no search ran) and mv is in quarter samples."""
    best = (NO_SCORE, 0, 0)
    winner = 0
    prev_hopeless = (w0 >> 22) & 1
    searched = not (prev_hopeless and (frame_num & 7) != 0)
    seen, pinfo = [], {"tied": 0}
    if searched:
        best = score_grid(S, ref, x0, y0, 0, 0, W, sy0, sy1, best, seen)
        winner = 1
        pvx, pvy = previous_vector(w0, w1)
        if (pvx, pvy) != (0, 0) and (abs(pvx) > 2 or abs(pvy) > 2):
            nb = score_grid(S, ref, x0, y0, pvx, pvy, W, sy0, sy1, best,
                            seen)
            if nb != best:
                best, winner = nb, 2
        if best[0] > PYRAMID_GATE:
            seed = pyramid_seed(P, ref2, x0 >> 2, y0 >> 2, W >> 2,
                                sy0 >> 2, sy1 >> 2, pinfo)
            if seed is not None:
                nb = score_grid(S, ref, x0, y0, seed[0] * 4, seed[1] * 4,
                                W, sy0, sy1, best, seen)
                if nb != best:
                    best, winner = nb, 3
    score, bmx, bmy = best
    # another vector with the winner's score: the visiting order decided
    grid_tie = any(sc == score and (mx, my) != (bmx, bmy)
                   for sc, mx, my in seen)
    pyramid_tie = winner == 3 and pinfo["tied"] > 1

    skip_thresh = 48 << (qp // 6)
    inter_thresh = 6 * skip_thresh
    sad0 = sad(S, block(ref, x0, y0))
    mv, hint = (0, 0), (0, 0)
    if sad0 <= skip_thresh:
        mode = SKIP
    else:
        best_sad = sad(S, block(ref, x0 + bmx, y0 + bmy))
        bq = (bmx * 4, bmy * 4)
        if best_sad <= 2 * inter_thresh:
            for _ in range(8):                      # integer +-1 ring
                centre, improved = bq, False
                for dx, dy in PAT:
                    q = (centre[0] + 4 * dx, centre[1] + 4 * dy)
                    if not window_inside(x0, y0, q[0], q[1], W, sy0, sy1):
                        continue
                    s = sad(S, block(ref, x0 + (q[0] >> 2),
                                     y0 + (q[1] >> 2)))
                    if s < best_sad:
                        best_sad, bq, improved = s, q, True
                if not improved:
                    break
            for step in (2, 1):                     # half, then quarter
                centre = bq
                for dx, dy in PAT:
                    q = (centre[0] + step * dx, centre[1] + step * dy)
                    if not window_inside(x0, y0, q[0], q[1], W, sy0, sy1):
                        continue
                    s = sad(S, luma_mc(ref, x0, y0, q[0], q[1]))
                    if s < best_sad:
                        best_sad, bq = s, q
        if best_sad <= inter_thresh:
            mode, mv = INTER, bq
        else:
            mode = INTRA
        hint = (bq[0] >> 2, bq[1] >> 2)
    hopeless = mode == INTRA and score > HOPELESS_GATE
    if hopeless:
        hint = (0, 0)
    return dict(mode=mode, mv=mv, hint=hint, hopeless=hopeless, score=score,
                winner=winner if mode != SKIP else 0, searched=searched,
                grid_tie=grid_tie and mode != SKIP,
                pyramid_tie=pyramid_tie and mode != SKIP,
                probe=bool(prev_hopeless and searched))


# ---- one picture, frame after frame -----------------------------------------

class MeMirror:
    """The motion search of one colour plane of one picture size, carried
    from frame to frame as the pipeline carries it: per-stripe frame_num
    and IDR state, two state words per MB."""

    def __init__(self, w, h, stripe_h, qp):
        self.w, self.h, self.stripe_h, self.qp = w, h, stripe_h, qp
        self.mbw, self.mbh = (w + 15) // 16, (h + 15) // 16
        self.word0 = np.zeros((self.mbh, self.mbw), np.int64)
        self.word1 = np.zeros((self.mbh, self.mbw), np.int64)
        self.stripes = [dict(y0=y, frame_num=0, need_idr=True)
                        for y in range(0, h, stripe_h)]
        # counters
        self.pass_wins = {1: 0, 2: 0, 3: 0}
        self.pass3_last_col = 0
        self.hopeless_mbs = 0
        self.probes = 0
        self.grid_ties = 0           # MBs whose winner the grid order chose
        self.pyramid_ties = 0        # ... the pyramid's (my, mx) order
        self.vectors = []            # every inter MB's quarter-pel vector
        self.last = {}               # (mbx, mby) -> decide_mb's last result

    def encode(self, src, ref, idr=False, mask=None):
        """src: the w x h source plane of this frame; ref: the MB-aligned
        reference plane (None for an all-IDR frame). Returns
        {(mbx, mby): (mode, (mvx, mvy))} for every MB of the encoded
        stripes; IDR rows report INTRA."""
        W = self.mbw * 16
        out = {}
        S_full = P_full = ref2 = None
        for si, st in enumerate(self.stripes):
            if mask is not None and not mask[si]:
                continue
            is_idr = idr or st["need_idr"]
            if is_idr:
                st["frame_num"] = 0
                st["need_idr"] = False
            frame_num = st["frame_num"]
            st["frame_num"] += 1
            y0 = st["y0"]
            row0 = y0 // 16
            rows = (min(y0 + self.stripe_h, self.h) - y0 + 15) // 16
            sy0, sy1 = y0, (row0 + rows) * 16
            for mby in range(row0, row0 + rows):
                for mbx in range(self.mbw):
                    if is_idr:
                        # the row kernels' rewrite of an I slice's MBs
                        self.word0[mby, mbx] = INTRA
                        out[(mbx, mby)] = (INTRA, (0, 0))
                        continue
                    if S_full is None:
                        S_full = padded_source(src, self.mbw, self.mbh)
                        P_full = pyramid(S_full)
                        ref = np.asarray(ref, np.int64)
                        ref2 = pyramid(ref)
                    d = decide_mb(
                        block(S_full, mbx * 16, mby * 16),
                        source_proxy(P_full, self.w, self.h, mbx, mby),
                        ref, ref2, mbx * 16, mby * 16, W, sy0, sy1, self.qp,
                        frame_num, int(self.word0[mby, mbx]),
                        int(self.word1[mby, mbx]))
                    w0, w1 = pack_words(d["mode"], d["hint"], d["hopeless"],
                                        d["mv"])
                    self.word0[mby, mbx], self.word1[mby, mbx] = w0, w1
                    out[(mbx, mby)] = (d["mode"], d["mv"])
                    self.last[(mbx, mby)] = d
                    if d["winner"]:
                        self.pass_wins[d["winner"]] += 1
                        if d["winner"] == 3 and mbx == self.mbw - 1:
                            self.pass3_last_col += 1
                    self.hopeless_mbs += int(d["hopeless"])
                    self.probes += int(d["probe"])
                    self.grid_ties += int(d["grid_tie"])
                    self.pyramid_ties += int(d["pyramid_tie"])
                    if d["mode"] == INTER:
                        self.vectors.append(d["mv"])
        return out

    def recode_intra(self, mbx, mby):
        """A monochrome (fullcolor) plane re-codes an inter MB whose
        quantised residual is not zero as I16x16: the row kernel rewrites
        the mode and keeps hint and hopeless bits."""
        assert (self.word0[mby, mbx] & 3) == INTER
        self.word0[mby, mbx] = (self.word0[mby, mbx] & ~3) | INTRA

    def words(self):
        """(mbh, mbw, 2) state words, as dump["meta"] lays them out."""
        return np.stack([self.word0, self.word1], axis=-1)

    def vector_kinds(self):
        """How many inter vectors are odd whole-sample, half-sample and
        quarter-sample."""
        odd = half = quarter = 0
        for mvx, mvy in self.vectors:
            if (mvx | mvy) & 1:
                quarter += 1
            elif (mvx | mvy) & 2:
                half += 1
            elif ((mvx >> 2) | (mvy >> 2)) & 1:
                odd += 1
        return dict(odd=odd, half=half, quarter=quarter)

    def coverage(self):
        c = dict(pass1=self.pass_wins[1], pass2=self.pass_wins[2],
                 pass3=self.pass_wins[3],
                 pass3_last_col=self.pass3_last_col,
                 hopeless=self.hopeless_mbs, probes=self.probes,
                 grid_ties=self.grid_ties, pyramid_ties=self.pyramid_ties)
        c.update(self.vector_kinds())
        return c


def masked_equal(meta, mirror_words):
    """Compare dumped state words with the mirror's under the mask the
    motion search owns: bits 0..1 and 8..22 of word 0 for every MB, word 1
    for skip and inter MBs (an intra MB's word 1 belongs to the row
    kernel). Returns the list of differing (mby, mbx, which)."""
    meta = np.asarray(meta, np.int64)
    bad = []
    m0 = (meta[..., 0] & WORD0_MASK) != (mirror_words[..., 0] & WORD0_MASK)
    for mby, mbx in np.argwhere(m0):
        bad.append((int(mby), int(mbx), 0))
    not_intra = (mirror_words[..., 0] & 3) != INTRA
    m1 = not_intra & ((meta[..., 1] & 0xFFFFFFFF)
                      != (mirror_words[..., 1] & 0xFFFFFFFF))
    for mby, mbx in np.argwhere(m1):
        bad.append((int(mby), int(mbx), 1))
    return bad
