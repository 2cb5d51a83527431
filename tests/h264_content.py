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


def count_slice_nals(data):
    """Number of slice NALs (types 1 and 5) in an Annex-B stream."""
    return sum(1 for n in split_nals(bytes(data)) if (n[0] & 0x1F) in (1, 5))
