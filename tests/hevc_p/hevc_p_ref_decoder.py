"""From-spec decoder for the encoder's HEVC streams with P pictures.

Subclasses tests/hevc_ref_decoder.py (same arithmetic decoder, residual
parser, intra predictors and transforms) and adds what a stream of
IDR, P, P... pictures with one reference needs. Written from the spec text,
not from the encoder; where the stream leaves this subset the decoder
raises NotImplementedError instead of guessing. The rules, with anchors:

 * SPS (§7.3.2.2, §7.3.7): log2_max_pic_order_cnt_lsb, the DPB size and
   the short-term RPS candidates (no inter-RPS prediction for idx 0).
 * PPS (§7.3.2.3): parsed for the fields the slice header depends on
   (cabac_init_present_flag, default ref idx counts, weighted prediction,
   lists modification, ...).
 * Slice header (§7.3.6.1), for I and P slices of IDR and TRAIL_R NALs.
 * POC (§8.3.1): PicOrderCntMsb from prevTid0Pic; an IDR resets to 0.
 * RPS (§8.3.2): PocStCurrBefore from the selected SPS candidate; a
   picture that is not in the DPB raises ("no reference picture").
   RefPicList0 (§8.3.4) is that one picture. The DPB holds one picture.
 * CABAC init (§9.3.2.2, Tables 9-5..9-37): initType 0 for I slices, 1 for
   P slices with cabac_init_flag 0.
 * Neighbour availability (§6.4.1): a neighbouring CTU is available when it
   lies in the picture, was decoded before and belongs to the same slice
   (SliceAddrRs equal); computed per neighbour from the recorded slice
   address of every CTU, never assumed.
 * coding_unit (§7.3.8.5): cu_skip_flag (ctxInc from the left and above
   CUs, §9.3.4.2.2), pred_mode_flag, part_mode, merge_flag; rqt_root_cbf
   is absent for a 2Nx2N merge CU and inferred 1; cbf_luma is absent at
   trafoDepth 0 of an inter CU whose chroma cbfs are both 0 and inferred 1
   (§7.4.9.8).
 * Merge candidates (§8.5.3.2.2-.5): A1, B1, B0, A0, B2 with the spec's
   pruning, then zero candidates, cut to MaxNumMergeCand.
 * Inter prediction (§8.5.3.3): integer motion only; the sample path is
   written out (<< 6, then the default weighted prediction's (+32) >> 6).
 * Intra MPM (§8.4.2): candidate A is DC when the left CU is unavailable
   or not intra; candidate B is DC whenever the above CU lies in another
   CTB row.

Per CTU of every picture `p_ctus` records a dict: poc, addr, kind ("skip",
"merge" or "intra"), mode (intra only), cbf (y, cb, cr), cbf_luma_coded,
skip_ctx (cu_skip_flag ctxInc, P slices) and cand_a (intra only).
`pictures` records (nal_type, poc, poc_lsb, slice_type) per picture.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hevc_ref_decoder as hrd  # noqa: E402

# initValues for initType 1 (Tables 9-5..9-37), keyed like hrd.INIT, plus
# the syntax elements an I slice never codes
INIT1 = {
    "split_cu": [107, 139, 126],
    "cu_skip": [197, 185, 201],
    "pred_mode": [149],
    "part_mode": [154],
    "merge_flag": [110],
    "prev_intra": [154],
    "chroma_mode": [152],
    "cbf_luma": [153, 111],
    "cbf_chroma": [149, 107, 167, 154],
    "last_x": [125, 110, 94, 110, 95, 79, 125, 111, 110,
               78, 110, 111, 111, 95, 94, 108, 123, 108],
    "last_y": [125, 110, 94, 110, 95, 79, 125, 111, 110,
               78, 110, 111, 111, 95, 94, 108, 123, 108],
    "csbf": [121, 140, 61, 154],
    "sig": [155, 154, 139, 153, 139, 123, 123, 63, 153, 166, 183, 140,
            136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140,
            136, 153, 154, 170, 153, 123, 123, 107, 121, 107, 121, 167,
            151, 183, 140, 151, 183, 140],
    "gt1": [154, 196, 196, 167, 154, 152, 167, 182, 182, 134, 149, 136,
            153, 121, 136, 137, 169, 194, 166, 167, 154, 167, 137, 182],
    "gt2": [107, 167, 91, 122, 107, 167],
}

# order of the C++ context bank (native/cpu/hevc/tables.h CtxOffset), for
# the table cross-check in the tests
BANK_ORDER = ("split_cu", "prev_intra", "chroma_mode", "cbf_luma",
              "cbf_chroma", "last_x", "last_y", "csbf", "sig", "gt1", "gt2",
              "cu_skip", "pred_mode", "part_mode", "merge_flag")

MODE_INTRA, MODE_INTER, MODE_SKIP = "intra", "merge", "skip"


class ContextsP:
    def __init__(self, qp, init_type):
        table = INIT1 if init_type == 1 else hrd.INIT
        for name, vals in table.items():
            setattr(self, name, [hrd.init_ctx(v, qp) for v in vals])


class DecoderP(hrd.Decoder):
    """hrd.Decoder for chains of IDR and P pictures (4:2:0, one reference).

    decode(data) takes the concatenated emissions of one stripe and
    returns every decoded picture, cropped, in decoding order."""

    def __init__(self, qpc_override=None):
        super().__init__(qpc_override)
        self.pps = None
        self.dpb = {}            # poc -> (y, cb, cr) reference pictures
        self.prev_tid0_poc = 0
        self.pictures = []
        self.p_ctus = []
        self.nal_types = []

    # ---- parameter sets ---------------------------------------------------

    def _parse_sps(self, br):
        br.u(4)       # vps id
        br.u(3)       # max_sub_layers
        br.u(1)       # nesting
        self._parse_ptl(br)
        assert br.ue() == 0          # sps id
        assert br.ue() == 1          # chroma_format: 4:2:0
        cw = br.ue()
        ch = br.ue()
        w, h = cw, ch
        if br.u(1):                  # conformance window
            left, right, top, bottom = br.ue(), br.ue(), br.ue(), br.ue()
            assert left == 0 and top == 0
            w = cw - 2 * right
            h = ch - 2 * bottom
        assert br.ue() == 0 and br.ue() == 0   # bit depths: 8
        log2_max_poc_lsb = br.ue() + 4
        assert br.u(1) == 1          # sub_layer_ordering_info_present
        max_dec_pic_buffering = br.ue() + 1
        br.ue(), br.ue()             # num_reorder, latency_increase
        min_cb = br.ue() + 3
        ctb = min_cb + br.ue()
        min_tb = br.ue() + 2
        max_tb = min_tb + br.ue()
        assert ctb == 4 and max_tb == 4, "decoder subset: CTU16/TB16"
        depth_inter = br.ue()
        depth_intra = br.ue()
        assert br.u(1) == 0          # scaling lists
        amp = br.u(1)
        assert br.u(1) == 0          # sao
        assert br.u(1) == 0          # pcm
        rps = []
        for idx in range(br.ue()):   # num_short_term_ref_pic_sets
            rps.append(self._parse_st_rps(br, idx))
        assert br.u(1) == 0          # long_term_ref_pics_present
        temporal_mvp = br.u(1)
        assert br.u(1) == 0          # strong_intra_smoothing
        assert br.u(1) == 0          # vui
        assert br.u(1) == 0          # sps_extension_present
        self.sps = {"cw": cw, "ch": ch, "w": w, "h": h,
                    "ctb_w": cw // 16, "ctb_h": ch // 16,
                    "log2_max_poc_lsb": log2_max_poc_lsb,
                    "max_dec_pic_buffering": max_dec_pic_buffering,
                    "min_cb_log2": min_cb, "depth_inter": depth_inter,
                    "depth_intra": depth_intra, "amp": amp, "rps": rps,
                    "temporal_mvp": temporal_mvp}

    def _parse_st_rps(self, br, idx):
        """st_ref_pic_set(idx), §7.3.7 / §7.4.8: returns (DeltaPocS0 with
        used flags, DeltaPocS1 with used flags)."""
        if idx != 0 and br.u(1):     # inter_ref_pic_set_prediction_flag
            raise NotImplementedError("inter RPS prediction")
        n_neg, n_pos = br.ue(), br.ue()
        s0, s1 = [], []
        d = 0
        for _ in range(n_neg):
            d -= br.ue() + 1         # delta_poc_s0_minus1
            s0.append((d, br.u(1)))  # used_by_curr_pic_s0_flag
        d = 0
        for _ in range(n_pos):
            d += br.ue() + 1
            s1.append((d, br.u(1)))
        return s0, s1

    def _parse_pps(self, br):
        p = {}
        assert br.ue() == 0 and br.ue() == 0     # pps id, sps id
        p["dependent_slices"] = br.u(1)
        p["output_flag_present"] = br.u(1)
        p["extra_header_bits"] = br.u(3)
        assert br.u(1) == 0                      # sign_data_hiding
        p["cabac_init_present"] = br.u(1)
        p["num_ref_idx_l0_default"] = br.ue() + 1
        br.ue()                                  # l1 default
        p["init_qp"] = 26 + br.se()
        assert br.u(1) == 0                      # constrained_intra_pred
        assert br.u(1) == 0                      # transform_skip
        assert br.u(1) == 0                      # cu_qp_delta_enabled
        assert br.se() == 0 and br.se() == 0     # cb/cr qp offsets
        p["slice_chroma_qp_offsets"] = br.u(1)
        p["weighted_pred"] = br.u(1)
        br.u(1)                                  # weighted_bipred
        assert br.u(1) == 0                      # transquant_bypass
        assert br.u(1) == 0                      # tiles
        assert br.u(1) == 0                      # entropy_coding_sync
        p["loop_filter_across_slices"] = br.u(1)
        p["deblock_override"] = 0
        p["deblock_disabled"] = 0
        if br.u(1):                              # deblocking control present
            p["deblock_override"] = br.u(1)
            p["deblock_disabled"] = br.u(1)
            if not p["deblock_disabled"]:
                br.se(), br.se()
        assert p["deblock_disabled"] == 1, "subset: deblocking off"
        assert br.u(1) == 0                      # scaling list data
        p["lists_modification"] = br.u(1)
        p["log2_par_mrg_level"] = br.ue() + 2
        p["header_extension"] = br.u(1)
        self.pps = p

    # ---- stream -----------------------------------------------------------

    def decode(self, data):
        self.frames = []
        self._pic = None
        for nal in hrd.split_nals(bytes(data)):
            ntype = (nal[0] >> 1) & 0x3F
            self.nal_types.append(ntype)
            body = nal[2:]
            if ntype == 33:
                self._parse_sps(hrd.BitReader(body))
            elif ntype == 34:
                self._parse_pps(hrd.BitReader(body))
            elif ntype == 32:
                continue
            elif ntype in (1, 19):   # TRAIL_R, IDR_W_RADL
                self._decode_slice_p(hrd.BitReader(body), ntype)
            else:
                raise NotImplementedError(f"NAL type {ntype}")
        self._finish_picture()
        return self.frames

    def _finish_picture(self):
        """End of the current picture: output it and make it the (only)
        reference (one-picture DPB; every picture is a reference)."""
        if self._pic is None:
            return
        self._emit(self._pic["planes"])
        self.dpb = {self._pic["poc"]: tuple(p.copy()
                                            for p in self._pic["planes"])}
        self._pic = None

    def _start_picture(self, ntype, poc_lsb):
        s = self.sps
        idr = ntype == 19
        if idr:
            poc = 0                  # §8.3.1: IDR has msb 0 and lsb 0
            self.dpb = {}            # §8.3.2: all reference pictures removed
        else:
            max_lsb = 1 << s["log2_max_poc_lsb"]
            prev_lsb = self.prev_tid0_poc & (max_lsb - 1)
            prev_msb = self.prev_tid0_poc - prev_lsb
            if poc_lsb < prev_lsb and prev_lsb - poc_lsb >= max_lsb // 2:
                msb = prev_msb + max_lsb
            elif poc_lsb > prev_lsb and poc_lsb - prev_lsb > max_lsb // 2:
                msb = prev_msb - max_lsb
            else:
                msb = prev_msb
            poc = msb + poc_lsb
        # TemporalId 0 and neither RASL, RADL nor a sub-layer non-reference
        self.prev_tid0_poc = poc
        n_ctb = s["ctb_w"] * s["ctb_h"]
        self._pic = {
            "poc": poc, "idr": idr,
            "planes": (np.zeros((s["ch"], s["cw"]), np.int32),
                       np.zeros((s["ch"] // 2, s["cw"] // 2), np.int32),
                       np.zeros((s["ch"] // 2, s["cw"] // 2), np.int32)),
            "slice_of": [None] * n_ctb,    # SliceAddrRs of each decoded CTU
            "pred": [None] * n_ctb,        # MODE_* of each decoded CTU
            "intra_mode": [None] * n_ctb,
            "mv": [None] * n_ctb,          # (mvx, mvy, ref_idx) of inter CUs
        }
        return poc

    def _decode_slice_p(self, br, ntype):
        s, pps = self.sps, self.pps
        first = br.u(1)
        if 16 <= ntype <= 23:
            br.u(1)                      # no_output_of_prior_pics_flag
        assert br.ue() == 0              # pps id
        assert not pps["dependent_slices"]
        n_ctb = s["ctb_w"] * s["ctb_h"]
        addr = 0
        if not first:
            addr = br.u(max(1, (n_ctb - 1).bit_length()))
        br.u(pps["extra_header_bits"])
        slice_type = br.ue()             # 0 B, 1 P, 2 I
        if slice_type == 0:
            raise NotImplementedError("B slice")
        assert not pps["output_flag_present"]
        poc_lsb = 0
        rps = ([], [])
        if ntype not in (19, 20):
            poc_lsb = br.u(s["log2_max_poc_lsb"])
            if not br.u(1):              # short_term_ref_pic_set_sps_flag
                raise NotImplementedError("slice-header RPS")
            n_sets = len(s["rps"])
            assert n_sets > 0
            idx_bits = (n_sets - 1).bit_length()   # Ceil(Log2(n_sets))
            rps = s["rps"][br.u(idx_bits) if idx_bits else 0]
            assert not s["temporal_mvp"]
        if first:
            self._finish_picture()
            poc = self._start_picture(ntype, poc_lsb)
            self.pictures.append((ntype, poc, poc_lsb, slice_type))
        pic = self._pic
        assert pic is not None, "slice without a first slice segment"

        # §8.3.2: the reference picture set of this picture
        poc_st_curr_before = [pic["poc"] + d for d, used in rps[0] if used]
        poc_st_curr_after = [pic["poc"] + d for d, used in rps[1] if used]
        refs = []
        for p in poc_st_curr_before + poc_st_curr_after:
            if p not in self.dpb:
                raise ValueError(f"no reference picture with POC {p} for "
                                 f"picture {pic['poc']}")
            refs.append(self.dpb[p])

        num_ref_idx = 0
        max_merge = 0
        if slice_type == 1:
            num_ref_idx = pps["num_ref_idx_l0_default"]
            if br.u(1):                  # num_ref_idx_active_override_flag
                num_ref_idx = br.ue() + 1
            if pps["lists_modification"] and len(refs) > 1:
                raise NotImplementedError("ref_pic_lists_modification")
            cabac_init_flag = br.u(1) if pps["cabac_init_present"] else 0
            if cabac_init_flag:
                raise NotImplementedError("cabac_init_flag")
            if pps["weighted_pred"]:
                raise NotImplementedError("weighted prediction")
            max_merge = 5 - br.ue()      # five_minus_max_num_merge_cand
            assert 1 <= max_merge <= 5
            assert refs, "P slice with an empty RPS"
            # §8.3.4: RefPicList0[i] = RefPicListTemp0[i % NumRpsCurrTempList0]
            ref_list0 = [refs[i % len(refs)] for i in range(num_ref_idx)]
        else:
            ref_list0 = []
        qp = pps["init_qp"] + br.se()
        assert not pps["slice_chroma_qp_offsets"]
        assert not pps["deblock_override"]
        # pps_loop_filter_across_slices && (sao || !deblock_disabled): absent
        assert not pps["header_extension"]
        br.byte_align()

        cab = hrd.Cabac(br)
        ctxs = ContextsP(qp, 1 if slice_type == 1 else 0)
        qpc = hrd.chroma_qp(qp)
        if self.qpc_override is not None:
            qpc = self.qpc_override(qp)
        self.qpc_used.append(qpc)
        caddr = addr
        while True:
            self._decode_ctu_p(cab, ctxs, pic, caddr, addr, slice_type, qp,
                               qpc, ref_list0, num_ref_idx, max_merge)
            caddr += 1
            if cab.terminate():
                break
            assert caddr < n_ctb

    # ---- CTU --------------------------------------------------------------

    def _available(self, pic, cx, cy, slice_addr):
        """§6.4.1 for the CTU at (cx, cy) seen from the CTU being decoded:
        inside the picture, decoded, and in the same slice."""
        s = self.sps
        if cx < 0 or cy < 0 or cx >= s["ctb_w"] or cy >= s["ctb_h"]:
            return False
        so = pic["slice_of"][cy * s["ctb_w"] + cx]
        return so is not None and so == slice_addr

    def _merge_candidates(self, pic, cx, cy, slice_addr, num_ref_idx,
                          max_merge):
        """§8.5.3.2.2-.5 for a 2Nx2N PU that fills the CTU. Candidates are
        (mvx, mvy, ref_idx) of list 0."""
        ctb_w = self.sps["ctb_w"]

        def cand(nx, ny):
            # §6.4.2: available and not intra
            if not self._available(pic, nx, ny, slice_addr):
                return None
            return pic["mv"][ny * ctb_w + nx]    # None for intra CUs

        # the five neighbouring sample positions, as CTU coordinates
        a1 = cand(cx - 1, cy)          # (xPb - 1, yPb + nPbH - 1)
        b1 = cand(cx, cy - 1)          # (xPb + nPbW - 1, yPb - 1)
        b0 = cand(cx + 1, cy - 1)      # (xPb + nPbW, yPb - 1)
        a0 = cand(cx - 1, cy + 1)      # (xPb - 1, yPb + nPbH): not decoded
        b2 = cand(cx - 1, cy - 1)      # (xPb - 1, yPb - 1)
        if b1 is not None and b1 == a1:
            b1 = None
        if b0 is not None and b0 == b1:
            b0 = None
        if a0 is not None and a0 == a1:
            a0 = None
        if b2 is not None and (b2 == a1 or b2 == b1):
            b2 = None
        n4 = sum(c is not None for c in (a1, b1, b0, a0))
        if n4 == 4:
            b2 = None
        lst = [c for c in (a1, b1, b0, a0, b2) if c is not None]
        # no temporal candidate (slice_temporal_mvp_enabled_flag 0), no
        # combined bi-predictive candidates (P slice); zero candidates
        zero_idx = 0
        while len(lst) < max_merge:
            lst.append((0, 0, zero_idx if zero_idx < num_ref_idx else 0))
            zero_idx += 1
        return lst[:max_merge]

    def _decode_ctu_p(self, cab, ctxs, pic, caddr, slice_addr, slice_type,
                      qp, qpc, ref_list0, num_ref_idx, max_merge):
        s = self.sps
        ctb_w = s["ctb_w"]
        cx, cy = caddr % ctb_w, caddr // ctb_w
        x0, y0 = cx * 16, cy * 16
        ry, rcb, rcr = pic["planes"]
        avail_l = self._available(pic, cx - 1, cy, slice_addr)
        avail_a = self._available(pic, cx, cy - 1, slice_addr)
        left = caddr - 1
        above = caddr - ctb_w
        # the CTU joins the slice before its own syntax is parsed
        pic["slice_of"][caddr] = slice_addr

        # split_cu_flag ctxInc (§9.3.4.2.2): neighbour CtDepth > cqtDepth;
        # every CU of this subset has depth 0
        assert cab.decision(ctxs.split_cu[0]) == 0, "subset: no CU split"

        rec = {"poc": pic["poc"], "addr": caddr, "kind": MODE_INTRA,
               "mode": None, "cbf": (0, 0, 0), "cbf_luma_coded": False,
               "skip_ctx": None, "cand_a": None}
        kind = MODE_INTRA
        if slice_type != 2:
            cond_l = avail_l and pic["pred"][left] == MODE_SKIP
            cond_a = avail_a and pic["pred"][above] == MODE_SKIP
            rec["skip_ctx"] = int(cond_l) + int(cond_a)
            if cab.decision(ctxs.cu_skip[rec["skip_ctx"]]):
                kind = MODE_SKIP
            elif cab.decision(ctxs.pred_mode[0]) == 0:
                kind = MODE_INTER
        rec["kind"] = kind
        pic["pred"][caddr] = kind

        if kind == MODE_INTRA:
            # part_mode only at log2CbSize == MinCbLog2SizeY
            assert s["min_cb_log2"] != 4
            self._intra_cu(cab, ctxs, pic, caddr, avail_l, slice_addr, qp,
                           qpc, rec)
            self.p_ctus.append(rec)
            return

        if kind == MODE_INTER:
            # part_mode, log2CbSize > MinCbLog2SizeY: bin 0 = 1 is 2Nx2N
            if cab.decision(ctxs.part_mode[0]) != 1:
                raise NotImplementedError("part_mode != 2Nx2N")
            if cab.decision(ctxs.merge_flag[0]) != 1:
                raise NotImplementedError("merge_flag = 0 (AMVP)")
        if max_merge > 1:
            raise NotImplementedError("merge_idx (MaxNumMergeCand > 1)")
        merge_idx = 0                     # inferred
        mvx, mvy, ref_idx = self._merge_candidates(
            pic, cx, cy, slice_addr, num_ref_idx, max_merge)[merge_idx]
        if (mvx, mvy) != (0, 0):
            raise NotImplementedError("non-zero motion vector")
        pic["mv"][caddr] = (mvx, mvy, ref_idx)
        ref = ref_list0[ref_idx]

        # §8.5.3.3.3 with xFrac = yFrac = 0: predSamples = ref << shift3
        # (14 - BitDepth); §8.5.3.3.4.2 default weighted prediction:
        # Clip((predSamples + offset1) >> shift1), shift1 = 14 - BitDepth
        def inter_pred(plane, x, y, n):
            blk = plane[y:y + n, x:x + n].astype(np.int64) << 6
            return np.clip((blk + 32) >> 6, 0, 255)

        py = inter_pred(ref[0], x0, y0, 16)
        pcb = inter_pred(ref[1], x0 // 2, y0 // 2, 8)
        pcr = inter_pred(ref[2], x0 // 2, y0 // 2, 8)

        cbf_y = cbf_cb = cbf_cr = 0
        if kind == MODE_INTER:
            # rqt_root_cbf: absent for PART_2Nx2N && merge_flag, inferred 1
            # transform_tree(trafoDepth 0): split_transform_flag is absent
            # only if MaxTrafoDepth (= depth_inter) is 0; interSplitFlag is
            # 0 for 2Nx2N
            if s["depth_inter"] != 0:
                raise NotImplementedError("inter transform split")
            cbf_cb = cab.decision(ctxs.cbf_chroma[0])
            cbf_cr = cab.decision(ctxs.cbf_chroma[0])
            if cbf_cb or cbf_cr:
                cbf_y = cab.decision(ctxs.cbf_luma[1])
                rec["cbf_luma_coded"] = True
            else:
                cbf_y = 1                # §7.4.9.8 inference
        rec["cbf"] = (cbf_y, cbf_cb, cbf_cr)

        for plane, pred, cbf, n, cidx, q, xx, yy in (
                (ry, py, cbf_y, 16, 0, qp, x0, y0),
                (rcb, pcb, cbf_cb, 8, 1, qpc, x0 // 2, y0 // 2),
                (rcr, pcr, cbf_cr, 8, 2, qpc, x0 // 2, y0 // 2)):
            if cbf:
                lv = hrd.decode_residual(cab, ctxs, n, cidx)
                res = hrd.inv_transform(hrd.dequant(lv, q, n), n)
                plane[yy:yy + n, xx:xx + n] = np.clip(pred + res, 0, 255)
            else:
                plane[yy:yy + n, xx:xx + n] = pred
        self.p_ctus.append(rec)

    def _intra_cu(self, cab, ctxs, pic, caddr, avail_l, slice_addr, qp, qpc,
                  rec):
        s = self.sps
        ctb_w = s["ctb_w"]
        cx, cy = caddr % ctb_w, caddr // ctb_w
        x0, y0 = cx * 16, cy * 16
        ry, rcb, rcr = pic["planes"]
        prev = cab.decision(ctxs.prev_intra[0])
        # §8.4.2: candidate A is DC when the left CU is unavailable or not
        # MODE_INTRA; candidate B is DC because the above CU lies in
        # another CTB row (yCb - 1 < ((yCb >> CtbLog2SizeY) << CtbLog2SizeY))
        if avail_l and pic["pred"][caddr - 1] == MODE_INTRA:
            cand_a = pic["intra_mode"][caddr - 1]
        else:
            cand_a = 1
        cand_b = 1
        rec["cand_a"] = cand_a
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
        pic["intra_mode"][caddr] = mode
        assert cab.decision(ctxs.chroma_mode[0]) == 0, "subset: DM chroma"
        if s["depth_intra"] != 0:
            raise NotImplementedError("intra transform split")
        cbf_cb = cab.decision(ctxs.cbf_chroma[0])
        cbf_cr = cab.decision(ctxs.cbf_chroma[0])
        cbf_y = cab.decision(ctxs.cbf_luma[1])
        rec["mode"] = mode
        rec["cbf"] = (cbf_y, cbf_cb, cbf_cr)
        rec["cbf_luma_coded"] = True
        self.ctus.append((mode, cbf_y, cbf_cb, cbf_cr))

        # constrained_intra_pred_flag 0: inter neighbours' samples count
        avail = {"left": avail_l,
                 "top": self._available(pic, cx, cy - 1, slice_addr),
                 "top_right": self._available(pic, cx + 1, cy - 1,
                                              slice_addr),
                 "corner": self._available(pic, cx - 1, cy - 1, slice_addr),
                 "below_left": False}    # the CTU below-left is not decoded
        corner, top, left = hrd.build_refs(ry, x0, y0, 16, avail)
        if mode == 0:
            corner, top, left = hrd.filter_refs(corner, top, left)
        p = hrd.predict(mode, corner, top, left, 16, 0)
        if cbf_y:
            lv = hrd.decode_residual(cab, ctxs, 16, 0)
            res = hrd.inv_transform(hrd.dequant(lv, qp, 16), 16)
            ry[y0:y0 + 16, x0:x0 + 16] = np.clip(p + res, 0, 255)
        else:
            ry[y0:y0 + 16, x0:x0 + 16] = p
        cx0, cy0 = x0 // 2, y0 // 2
        for plane, cbf, cidx in ((rcb, cbf_cb, 1), (rcr, cbf_cr, 2)):
            corner, top, left = hrd.build_refs(plane, cx0, cy0, 8, avail)
            p = hrd.predict(mode, corner, top, left, 8, cidx)
            if cbf:
                lv = hrd.decode_residual(cab, ctxs, 8, cidx)
                res = hrd.inv_transform(hrd.dequant(lv, qpc, 8), 8)
                plane[cy0:cy0 + 8, cx0:cx0 + 8] = np.clip(p + res, 0, 255)
            else:
                plane[cy0:cy0 + 8, cx0:cx0 + 8] = p
