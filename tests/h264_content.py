"""Shared H.264 test content and an instrumented reference decoder.

mixed_frames() builds content that makes the encoders take every
macroblock mode and every deblocking strength inside P slices:
  * a static flat-gradient quarter (P_Skip, low-activity strong edges),
  * two bands translating at different speeds (P_L0_16x16, MV
    differences between neighbours) plus a slower third band,
  * a fresh noise patch per frame (intra MBs inside P slices).
The three colour channels are independent textures, so chroma carries
real residual. tests/test_h264_content.py keeps that coverage from
rotting; the floors there were measured with exactly this generator.

CountingDecoder counts what a stream actually contained and keeps every
frame's UNCROPPED MB-aligned planes, which is what an encoder's
reconstruction buffers hold (motion search reads the padding).
"""

import numpy as np

import h264_ref_decoder
from h264_ref_decoder import BitReader, Decoder, split_nals


def tex(rng, h, w, passes=2):
    f = rng.integers(0, 256, (h, w, 3)).astype(np.float32)
    for _ in range(passes):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1)
             + np.roll(f, 1, 0) + np.roll(f, -1, 0)) / 5
    f = (f - f.mean()) * 2.0 + 128
    return np.clip(f, 0, 255).astype(np.uint8)


def mixed_frames(w, h, n, seed=7):
    rng = np.random.default_rng(seed)
    t = tex(rng, h, w)
    a, b, c = w // 4, w // 2, 3 * w // 4
    frames = []
    for i in range(n):
        f = np.zeros((h, w, 4), np.uint8); f[:, :, 3] = 255
        f[:, :, :3] = t
        f[:, :a, 0] = np.linspace(40, 90, a, dtype=np.uint8)[None, :]
        f[:, :a, 1] = np.linspace(200, 120, h, dtype=np.uint8)[:, None]
        f[:, :a, 2] = 128
        f[:h // 2, a:b, :3] = np.roll(t, (i, 3 * i), (0, 1))[:h // 2, a:b]
        f[h // 2:, a:b, :3] = np.roll(t, (-2 * i, -5 * i), (0, 1))[h // 2:, a:b]
        f[:, b:c, :3] = np.roll(t, (0, 2 * i), (0, 1))[:, b:c]
        if i:
            px = c + (i * 8) % max(1, w - c - 24); py = (i * 16) % max(1, h - 24)
            f[py:py + 24, px:px + 24, :3] = rng.integers(
                0, 256, (24, 24, 3), dtype=np.uint8)
        frames.append(np.ascontiguousarray(f))
    return frames


def smooth_tex(rng, h, w, passes, std=45.0):
    """tex() blurred `passes` times and rescaled to a fixed contrast: a
    texture smooth enough to be sampled at a fraction of its pitch."""
    f = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    for _ in range(passes):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1)
             + np.roll(f, 1, 0) + np.roll(f, -1, 0)) / 5
    f = (f - f.mean()) * (std / f.std()) + 128
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


# me_frames() bands: (name, first column, end column); the last band
# always runs to the right edge of the picture
ME_BANDS = (("static", 0, 32), ("slow", 32, 64), ("frac", 64, 96),
            ("noise", 96, 128), ("jump", 128, 192), ("scroll", 192, None))
ME_MARGIN = 64
ME_JUMP_FRAME = 3
ME_SETTLE_FRAME = 6


def me_scroll_offset(i):
    """The scroll band moves 12 px per frame to the right, and turns round
    at frame 5 so that the search has to acquire it a second time."""
    return 12 * i if i < 5 else 12 * (8 - i)


def me_frames(w, h, n, seed=11):
    """Content for the motion-search tests, in vertical bands:
      static  never changes (P_Skip);
      slow    moves (2, 1) px per frame: the zero-centred grid plus the
              +-1 ring (odd vectors);
      frac    a 4x oversampled texture stepped by quarter samples: upper
              half (2, 0) quarters per frame, lower half (2, 1);
      noise   fresh noise every frame (intra, hopeless). Its left MB
              column freezes from frame ME_SETTLE_FRAME on; the right one
              never does, so it is still hopeless when frame_num 8 probes;
      jump    still, but for one 32 px jump at frame ME_JUMP_FRAME
              (pyramid acquisition from a zero hint);
      scroll  12 px per frame (pyramid acquisition on the first P frame,
              hint tracking afterwards), reversing at frame 5. It reaches
              the right edge, so at a width that is no multiple of 16 the
              last MB column needs the pyramid too.
    The colour channels are independent textures. w >= 208."""
    assert w >= 208, w
    rng = np.random.default_rng(seed)
    M = ME_MARGIN
    T = {name: tex(rng, h + 2 * M, w + 2 * M)
         for name in ("static", "slow", "jump", "scroll")}
    T4 = smooth_tex(rng, 4 * (h + 8), 4 * (32 + 8), passes=40)
    frozen = None
    frames = []
    for i in range(n):
        f = np.zeros((h, w, 4), np.uint8)
        f[:, :, 3] = 255
        for name, xa, xb in ME_BANDS:
            xb = w if xb is None else xb
            ox = oy = 0
            if name == "slow":
                ox, oy = -2 * i, -i
            elif name == "jump":
                ox = -32 if i >= ME_JUMP_FRAME else 0
            elif name == "scroll":
                ox = -me_scroll_offset(i)
            if name == "frac":
                half = h // 2
                for ya, yb, qx, qy in ((0, half, 2 * i, 0),
                                       (half, h, 2 * i, i)):
                    ys = 4 * np.arange(ya, yb) + qy
                    xs = 4 * np.arange(0, xb - xa) + qx
                    f[ya:yb, xa:xb, :3] = T4[np.ix_(ys, xs)]
            elif name == "noise":
                nz = rng.integers(0, 256, (h, xb - xa, 3), dtype=np.uint8)
                if i == ME_SETTLE_FRAME - 1:
                    frozen = nz[:, :16].copy()
                if i >= ME_SETTLE_FRAME:
                    nz[:, :16] = frozen
                f[:, xa:xb, :3] = nz
            else:
                f[:, xa:xb, :3] = T[name][M + oy:M + oy + h,
                                          M + ox + xa:M + ox + xb]
        frames.append(np.ascontiguousarray(f))
    return frames


# tie_frames(): MB columns that differ from the flat picture, and by how much
TIE_COLUMNS = ((3, -14), (7, -14), (11, -48), (13, -48))


def tie_frames(w, h, n):
    """Content on which the order of the candidates decides. Frame 0 is
    flat grey (128) but for whole MB columns that are flat too (TIE_COLUMNS:
    column, offset); the odd frames are flat 128 all over, the even ones
    repeat frame 0. An I16x16 MB predicted from flat 128 neighbours codes
    no residual, so the reconstruction left and right of such a column is
    exactly 128, and in frame 1 a column's MBs see the same SSD at (-8, 0)
    and (8, 0) (half the block off the column on either side):
      offset -14  the score stays under the pyramid gate, the two vectors
                  tie in the zero-centred grid, the first in visiting
                  order has to win, and the +-1 ring walks on to (-16, 0);
      offset -48  the pyramid pass runs, every quarter-resolution position
                  off the column has SAD 0, and the smallest (my, mx) has
                  to seed the last grid.
    Use a qp whose deblocking threshold alpha is below 14 (qp <= 23), so
    that the column edges stay unfiltered. w >= 240."""
    assert w >= 240, w
    base = np.full((h, w, 4), 128, np.uint8)
    base[:, :, 3] = 255
    cols = base.copy()
    for c, off in TIE_COLUMNS:
        cols[:, c * 16:c * 16 + 16, :3] = 128 + off
    return [np.ascontiguousarray(base if i % 2 else cols) for i in range(n)]


def bgrx_to_planes(frame):
    """(Y, Cb, Cr) full-resolution uint8 planes of a BGRX frame: the
    pipelines' colour conversion (full-range BT.601 in float32, products
    summed left to right without fused multiply-add, round half to even).
    Y is the 4:2:0 luma plane too."""
    b, g, r = (frame[:, :, k].astype(np.float32) for k in range(3))
    c = np.float32

    def q(v):
        return np.rint(np.clip(v, c(0), c(255))).astype(np.uint8)

    y = c(0.299) * r + c(0.587) * g + c(0.114) * b
    cb = c(-0.168736) * r - c(0.331264) * g + c(0.5) * b + c(128)
    cr = c(0.5) * r - c(0.418688) * g - c(0.081312) * b + c(128)
    return q(y), q(cb), q(cr)


class CountingDecoder(Decoder):
    """Decoder that counts MB modes and deblock strengths.

    After decode():
      skip / inter   decode_skip / decode_p16 calls
      intra_in_p     decode_i16 calls inside P slices (all decode_i16
                     calls minus mbw*mbh per IDR picture)
      bs             histogram of h264_ref_decoder._db_bs return values
      y / cb / cr    last frame's uncropped MB-aligned planes (int32)
      uncropped      per frame (y, cb, cr) uncropped uint8 planes
      slices         per slice NAL (nal_type, first_mb, frame_num)
      db_changed     samples (all planes) the in-loop filter altered"""

    def __init__(self):
        super().__init__()
        self.db_changed = 0
        self.skip = self.inter = self.i16 = self.idr_mbs = 0
        self.bs = {k: 0 for k in range(5)}
        self.uncropped = []
        self.slices = []

    @property
    def intra_in_p(self):
        return self.i16 - self.idr_mbs

    def decode_skip(self, mbx, mby):
        self.skip += 1
        return super().decode_skip(mbx, mby)

    def decode_p16(self, br, mbx, mby, ctx, qp):
        self.inter += 1
        return super().decode_p16(br, mbx, mby, ctx, qp)

    def decode_i16(self, br, mbx, mby, i16_type, qp, ctx):
        self.i16 += 1
        return super().decode_i16(br, mbx, mby, i16_type, qp, ctx)

    def decode_slice(self, br, nal_type):
        # peek first_mb / frame_num with a reader of our own (the base
        # class parses and discards frame_num)
        pk = BitReader(br.data)
        first_mb = pk.ue()
        pk.ue()                                  # slice_type
        pk.ue()                                  # pps id
        if self.sps["separate"]:
            pk.u(2)
        frame_num = pk.u(self.sps["log2_max_frame_num"])
        self.slices.append((nal_type, first_mb, frame_num))
        if nal_type == 5 and first_mb == 0:
            self.idr_mbs += self.sps["mbw"] * self.sps["mbh"]
        return super().decode_slice(br, nal_type)

    def finish_frame(self):
        super().finish_frame()
        self.uncropped.append((self.y.astype(np.uint8),
                               self.cb.astype(np.uint8),
                               self.cr.astype(np.uint8)))

    def decode(self, data):
        orig_bs = h264_ref_decoder._db_bs
        orig_seg = h264_ref_decoder.deblock_segment_py

        def counting_bs(*a):
            v = orig_bs(*a)
            self.bs[v] += 1
            return v

        def counting_seg(Y, Cb, Cr, mb_row, *a):
            rows = [(Y, slice(mb_row * 16, mb_row * 16 + 16))]
            if Cb is not None:
                rows += [(C, slice(mb_row * 8, mb_row * 8 + 8))
                         for C in (Cb, Cr)]
            before = [P[r].copy() for P, r in rows]
            orig_seg(Y, Cb, Cr, mb_row, *a)
            for (P, r), b in zip(rows, before):
                self.db_changed += int(np.count_nonzero(P[r] != b))

        h264_ref_decoder._db_bs = counting_bs
        h264_ref_decoder.deblock_segment_py = counting_seg
        try:
            return super().decode(data)
        finally:
            h264_ref_decoder._db_bs = orig_bs
            h264_ref_decoder.deblock_segment_py = orig_seg

    def frame_nums(self):
        """frame_num of each picture (taken from its first slice), after
        asserting every slice of a picture carries the same value."""
        out = []
        for nal_type, first_mb, fn in self.slices:
            if first_mb == 0:
                out.append(fn)
            else:
                assert out and fn == out[-1], \
                    f"slice first_mb={first_mb}: frame_num {fn} != {out[-1:]}"
        return out


class RecordingDecoder(CountingDecoder):
    """CountingDecoder that also records what every MB was coded as.

    After decode():
      mbs   per picture {(plane, mbx, mby): (mode, (mvx, mvy))} with mode
            0 skip / 1 inter / 2 intra, vectors in quarter samples, plane
            0 unless the stream codes separate colour planes;
      mvs   {(mbx, mby): vector} of the skip and inter MBs of plane 0,
            the newest picture winning.
    Separate colour planes: `uncropped` holds the three full-size planes."""

    def __init__(self):
        super().__init__()
        self.mbs = [{}]
        self.mvs = {}
        self.plane = 0

    def _record(self, mbx, mby, mode, mv):
        self.mbs[-1][(self.plane, mbx, mby)] = (mode, mv)
        if self.plane == 0 and mode != 2:
            self.mvs[(mbx, mby)] = mv

    def decode_slice(self, br, nal_type):
        self.plane = 0
        if self.sps["separate"]:
            pk = BitReader(br.data)
            pk.ue(); pk.ue(); pk.ue()
            self.plane = pk.u(2)
        return super().decode_slice(br, nal_type)

    def decode_skip(self, mbx, mby):
        super().decode_skip(mbx, mby)
        self._record(mbx, mby, 0, (0, 0))

    def decode_p16(self, br, mbx, mby, ctx, qp):
        info = super().decode_p16(br, mbx, mby, ctx, qp)
        self._record(mbx, mby, 1, tuple(int(v) for v in ctx["left_mv"]))
        return info

    def decode_i16(self, br, mbx, mby, i16_type, qp, ctx):
        super().decode_i16(br, mbx, mby, i16_type, qp, ctx)
        self._record(mbx, mby, 2, (0, 0))

    def finish_frame(self):
        if self.sps["separate"]:
            Decoder.finish_frame(self)
            self.uncropped.append(tuple(p.astype(np.uint8)
                                        for p in self.planes))
        else:
            super().finish_frame()
        self.mbs.append({})


def count_slice_nals(data):
    """Number of slice NALs (types 1 and 5) in an Annex-B stream."""
    return sum(1 for n in split_nals(bytes(data)) if (n[0] & 0x1F) in (1, 5))
