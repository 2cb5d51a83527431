"""From-spec decoder for the encoder's Main 4:4:4 streams (H.265 v2+).

Subclasses tests/hevc_ref_decoder.py (same arithmetic) and overrides
only what chroma_format_idc == 3 changes; a 4:2:0 stream falls through to
the parent at every step. The rules, with their spec anchors:

 * profile_tier_level (§7.3.3, §A.3.7): general_profile_idc 4; for that
   profile the first 9 of the 43 reserved bits are the range-extension
   constraint flags (max_12bit, max_10bit, max_8bit, max_422chroma,
   max_420chroma, max_monochrome, intra, one_picture_only,
   lower_bit_rate), followed by 34 reserved zero bits and one more.
 * SPS (§7.3.2.2): chroma_format_idc == 3 is followed by
   separate_colour_plane_flag; the conformance window counts in units of
   SubWidthC = SubHeightC = 1.
 * Chroma QP (§8.6.1): for ChromaArrayType != 1, QpC = Min(qPi, 51); the
   Table 8-10 mapping is not used.
 * CTU (§7.3.8.8-11): chroma TBs are 16x16, residual_coding with
   cIdx 1/2 at log2TrafoSize 4, in the order Y, Cb, Cr.
 * Intra (§8.4.4.2.3): neighbour smoothing applies when cIdx == 0 or
   ChromaArrayType == 3: filterFlag is 0 for DC, else
   minDistVerHor > intraHorVerDistThres[nTbS] (1 at nTbS 16). The DC edge
   filter and the H/V boundary adjust stay cIdx == 0 only.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hevc_ref_decoder as hrd  # noqa: E402

INTRA_HOR_VER_DIST_THRES = {8: 7, 16: 1, 32: 0}


def filter_flag(mode, n):
    """§8.4.4.2.3 filterFlag (strong smoothing is disabled in the SPS)."""
    if mode == 1 or n == 4:
        return False
    dist = min(abs(mode - 26), abs(mode - 10))
    return dist > INTRA_HOR_VER_DIST_THRES[n]


class Decoder444(hrd.Decoder):
    """hrd.Decoder that also decodes chroma_format_idc == 3.

    `ctus`, `qpc_used` and `qpc_override` are the parent's. Each slice and
    CTU is decoded either here (4:4:4) or by the parent (4:2:0), never
    both, so each is recorded once."""

    def __init__(self, qpc_override=None):
        super().__init__(qpc_override)
        self.ptl = None

    # ---- parameter sets ---------------------------------------------------

    def _parse_ptl(self, br):
        ptl = {"profile_space": br.u(2), "tier": br.u(1),
               "profile_idc": br.u(5), "compat": br.u(32),
               "progressive": br.u(1), "interlaced": br.u(1),
               "non_packed": br.u(1), "frame_only": br.u(1)}
        if ptl["profile_idc"] == 4 or (ptl["compat"] >> (31 - 4)) & 1:
            ptl["rext"] = tuple(br.u(1) for _ in range(9))
            assert br.u(17) == 0 and br.u(17) == 0   # reserved_zero_34bits
        else:
            assert br.u(21) == 0 and br.u(22) == 0   # reserved_zero_43bits
        assert br.u(1) == 0                          # inbld / reserved bit
        ptl["level_idc"] = br.u(8)
        self.ptl = ptl

    def _parse_sps(self, br):
        br.u(4)       # vps id
        br.u(3)       # max_sub_layers
        br.u(1)       # nesting
        self._parse_ptl(br)
        assert br.ue() == 0          # sps id
        cfi = br.ue()
        assert cfi in (1, 3), "decoder subset: 4:2:0 or 4:4:4"
        if cfi == 3:
            assert br.u(1) == 0      # separate_colour_plane_flag
        sub = 1 if cfi == 3 else 2   # SubWidthC == SubHeightC
        cw = br.ue()
        ch = br.ue()
        w, h = cw, ch
        if br.u(1):                  # conformance window
            left = br.ue()
            right = br.ue()
            top = br.ue()
            bottom = br.ue()
            assert left == 0 and top == 0
            w = cw - sub * right
            h = ch - sub * bottom
        assert br.ue() == 0 and br.ue() == 0   # bit depths: 8
        br.ue()                      # log2_max_poc_lsb
        if br.u(1):                  # sub_layer_ordering_info_present
            br.ue(), br.ue(), br.ue()
        min_cb = br.ue() + 3
        ctb = min_cb + br.ue()
        min_tb = br.ue() + 2
        max_tb = min_tb + br.ue()
        assert ctb == 4 and max_tb == 4, "decoder subset: CTU16/TB16"
        br.ue(), br.ue()             # transform hierarchy depths
        assert br.u(1) == 0          # scaling lists
        br.u(1)                      # amp
        assert br.u(1) == 0          # sao
        assert br.u(1) == 0          # pcm
        assert br.ue() == 0          # num_short_term_rps
        assert br.u(1) == 0          # long_term_ref_pics_present
        br.u(1)                      # temporal_mvp
        assert br.u(1) == 0          # strong_intra_smoothing
        assert br.u(1) == 0          # vui
        assert br.u(1) == 0          # sps_extension_present: no range ext
        self.sps = {"cw": cw, "ch": ch, "w": w, "h": h,
                    "ctb_w": cw // 16, "ctb_h": ch // 16,
                    "chroma_format_idc": cfi,
                    "profile_idc": self.ptl["profile_idc"]}

    # ---- pictures ---------------------------------------------------------

    def _is444(self):
        return self.sps["chroma_format_idc"] == 3

    def _emit(self, pic):
        if not self._is444():
            return super()._emit(pic)
        s = self.sps
        self.frames.append(tuple(
            p[:s["h"], :s["w"]].astype(np.uint8) for p in pic))

    def _decode_slice(self, br, pic):
        if not self._is444():
            return super()._decode_slice(br, pic)
        # §7.3.6.1 + §7.3.8.1 for this subset, ChromaArrayType 3: the
        # picture has three coded-size planes
        s = self.sps
        first = br.u(1)
        br.u(1)                      # no_output_of_prior_pics
        assert br.ue() == 0          # pps id
        n_ctb = s["ctb_w"] * s["ctb_h"]
        addr = 0
        if not first:
            addr = br.u(max(1, (n_ctb - 1).bit_length()))
        assert br.ue() == 2          # slice_type I
        qp = 26 + br.se()
        br.byte_align()
        if first:
            if pic is not None:
                self._emit(pic)
            pic = tuple(np.zeros((s["ch"], s["cw"]), np.int32)
                        for _ in range(3))
        cab = hrd.Cabac(br)
        ctxs = hrd.Contexts(qp)
        # §8.6.1, ChromaArrayType != 1: QpC = Min(qPi, 51); pps/slice
        # chroma offsets are 0 so qPi = QpY
        qpc = min(qp, 51)
        if self.qpc_override is not None:
            qpc = self.qpc_override(qp)
        self.qpc_used.append(qpc)
        ctb_w = s["ctb_w"]
        caddr = addr
        left_mode = None
        while True:
            cx, cy = caddr % ctb_w, caddr // ctb_w
            left_mode = self._decode_ctu(cab, ctxs, pic, cx, cy, qp, qpc,
                                         left_mode)
            end = cab.terminate()
            caddr += 1
            if end:
                break
            if caddr % ctb_w == 0:
                left_mode = None
        return pic

    def _decode_ctu(self, cab, ctxs, pic, cx, cy, qp, qpc, left_mode):
        if not self._is444():
            return super()._decode_ctu(cab, ctxs, pic, cx, cy, qp, qpc,
                                       left_mode)
        x0, y0 = cx * 16, cy * 16
        assert cab.decision(ctxs.split_cu[0]) == 0, "subset: no CU split"
        # luma intra mode (§8.4.2 MPM)
        prev = cab.decision(ctxs.prev_intra[0])
        cand_a = left_mode if left_mode is not None else 1
        cand_b = 1  # above PU is in another CTU row -> DC
        if cand_a == cand_b:
            if cand_a < 2:
                lst = [0, 1, 26]
            else:
                lst = [cand_a, 2 + ((cand_a + 29) % 32),
                       2 + ((cand_a - 2 + 1) % 32)]
        else:
            lst = [cand_a, cand_b,
                   0 if cand_a != 0 and cand_b != 0 else
                   1 if cand_a != 1 and cand_b != 1 else 26]
        if prev:
            idx = 0
            if cab.bypass():
                idx = 1 + cab.bypass()
            mode = lst[idx]
        else:
            rem = cab.bypass_bits(5)
            for c in sorted(lst):
                if rem >= c:
                    rem += 1
            mode = rem
        # intra_chroma_pred_mode 4 (one bin 0): chroma mode = luma mode
        assert cab.decision(ctxs.chroma_mode[0]) == 0, "subset: DM chroma"

        # transform_tree at trafoDepth 0: cbf_cb, cbf_cr, then cbf_luma
        cbf_cb = cab.decision(ctxs.cbf_chroma[0])
        cbf_cr = cab.decision(ctxs.cbf_chroma[0])
        cbf_y = cab.decision(ctxs.cbf_luma[1])
        self.ctus.append((mode, cbf_y, cbf_cb, cbf_cr))

        avail = {"left": left_mode is not None, "top": False,
                 "top_right": False, "below_left": False, "corner": False}
        # residuals follow in the order Y, Cb, Cr; each plane's prediction
        # only needs its own earlier CTUs, so decode plane by plane
        for plane, cbf, cidx, q in ((pic[0], cbf_y, 0, qp),
                                    (pic[1], cbf_cb, 1, qpc),
                                    (pic[2], cbf_cr, 2, qpc)):
            corner, top, left = hrd.build_refs(plane, x0, y0, 16, avail)
            # cIdx == 0 || ChromaArrayType == 3: every plane may filter
            if filter_flag(mode, 16):
                corner, top, left = hrd.filter_refs(corner, top, left)
            p = hrd.predict(mode, corner, top, left, 16, cidx)
            if cbf:
                lv = hrd.decode_residual(cab, ctxs, 16, cidx)
                res = hrd.inv_transform(hrd.dequant(lv, q, 16), 16)
                plane[y0:y0 + 16, x0:x0 + 16] = np.clip(p + res, 0, 255)
            else:
                plane[y0:y0 + 16, x0:x0 + 16] = p
        return mode
