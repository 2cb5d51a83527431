"""HEVC 4:2:0 on the CPU encoder and the CPU pipeline, pinned to the
from-spec decoder (hevc_ref_decoder.Decoder): recon planes equal in Y, Cb
and Cr over the decoded area, for every QP, for odd and minimal sizes, for
mid-row slice segments, and on content that makes the encoder take every
mode and both values of every cbf flag. Every comparison is exact.

These run without a GPU and come first: the HIP pipeline must emit the CPU
pipeline's bytes (tests/test_gpu_hevc_recon.py), so when a GPU test fails
these tell whether the CPU encoder or the kernel left the spec.

The last test states the premise of the HIP pipeline's CABAC output
stride: the largest slice segment the encoder produces, per CTU, is at most
half the bytes the pipeline reserves per CTU."""

import os
import sys

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from hipflux import _native
import pipeline_content as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "hevc444"))
from hevc444_ref_decoder import Decoder444  # noqa: E402

MODE = 2   # output_mode of the HEVC pipelines


def encoder_planes(enc, h):
    y, cb, cr, yp, cp = enc.recon()
    yh = (h + 15) & ~15
    return (np.frombuffer(y, np.uint8).reshape(yh, yp),
            np.frombuffer(cb, np.uint8).reshape(yh // 2, cp),
            np.frombuffer(cr, np.uint8).reshape(yh // 2, cp))


def encode_stripes(img, w, h, qp, stripe_h):
    """Each stripe through its own HevcEncoder, as the CPU pipeline does;
    also asserts the CPU pipeline emits exactly these bytes. Returns
    [(y0, vis_h, data, recon planes)]."""
    out = []
    for y0 in range(0, h, stripe_h):
        vis_h = min(stripe_h, h - y0)
        enc = _native.HevcEncoder(w, vis_h)
        data = enc.encode(np.ascontiguousarray(img[y0:y0 + vis_h]).tobytes(),
                          qp=qp)["data"]
        out.append((y0, vis_h, data, encoder_planes(enc, vis_h)))
    piped = pc.per_frame(_native._pipeline_encode(
        "cpu", [img], w, h, qp, stripe_h, MODE))[0]
    assert piped == [(y0, data) for y0, _, data, _ in out]
    return out


# ---- all 52 QPs --------------------------------------------------------------

@pytest.mark.parametrize("qp", range(52))
def test_every_qp_recon_equals_decoder(qp):
    """48x16 noise. The decoder's own Table 8-10 reproduces all three
    planes; an identity chroma QP reproduces the chroma planes exactly
    when the table is the identity (qp < 30)."""
    w, h = 48, 16
    enc = _native.HevcEncoder(w, h)
    data = enc.encode(pc.uniform_noise(w, h, 3).tobytes(), qp=qp)["data"]
    planes = encoder_planes(enc, h)
    dec, got = pc.decode_stripe(data, w, h)
    assert dec.qpc_used == [pc.spec_chroma_qp(qp)]
    assert len(dec.ctus) == 3
    pc.assert_planes_equal(planes, 0, got, f"qp {qp}")

    wrong, bad = pc.decode_stripe(data, w, h, qpc_override=lambda q: q)
    assert wrong.qpc_used == [qp]
    assert np.array_equal(bad[0], got[0])          # luma does not use qpc
    same = np.array_equal(bad[1], got[1]) and np.array_equal(bad[2], got[2])
    assert same == (qp < 30), \
        f"qp {qp}: identity chroma QP {'reproduces' if same else 'misses'} " \
        f"the chroma planes"


def test_decoder444_records_a_420_stream_once():
    """A 4:2:0 stream falls through Decoder444 to the parent, which keeps
    the record: one entry per CTU and per slice, override honoured."""
    w, h, qp = 48, 16, 36
    enc = _native.HevcEncoder(w, h)
    data = enc.encode(pc.uniform_noise(w, h, 3).tobytes(), qp=qp)["data"]
    base, got = pc.decode_stripe(data, w, h)
    dec = Decoder444()
    frames = dec.decode(data)
    assert dec.sps["chroma_format_idc"] == 1
    assert dec.ctus == base.ctus and len(dec.ctus) == 3
    assert dec.qpc_used == [pc.spec_chroma_qp(qp)] == [34]
    for a, b in zip(frames[0], got):
        assert np.array_equal(a, b)
    wrong = Decoder444(qpc_override=lambda q: q)
    wrong.decode(data)
    assert wrong.qpc_used == [qp] and len(wrong.ctus) == 3


# ---- every mode, both values of every cbf ------------------------------------

@pytest.mark.parametrize("qp", [26, 34])
def test_coverage_content_recon_equals_decoder(qp):
    w, h = 161, 75
    decs = []
    for y0, vis_h, data, planes in encode_stripes(
            pc.frames_for(w, h, 1)[0], w, h, qp, 32):
        dec, got = pc.decode_stripe(data, w, vis_h)
        pc.assert_planes_equal(planes, 0, got, f"qp {qp} stripe y={y0}")
        decs.append(dec)
    assert sum(len(d.ctus) for d in decs) == 11 * 5
    pc.assert_full_coverage(decs, f"161x75 qp {qp}")


# ---- sizes ---------------------------------------------------------------------

# (w, h, stripe_h): one CTU; a second stripe with one visible row; a
# partial last stripe; the minimum picture; stripes of 32, 32 and 11 rows
SIZES = [(16, 16, 16), (17, 17, 16), (15, 33, 32), (1, 1, 16), (161, 75, 32)]


@pytest.mark.parametrize("w,h,stripe_h", SIZES,
                         ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_sizes_recon_equals_decoder(w, h, stripe_h):
    """Noise at QP 22. Each stripe is a stream of its own whose decoded
    size is the visible size rounded up to even (decode_stripe asserts
    it)."""
    stripes = encode_stripes(pc.uniform_noise(w, h, 5), w, h, 22, stripe_h)
    assert [(y0, vh) for y0, vh, _, _ in stripes] == \
        [(y0, min(stripe_h, h - y0)) for y0 in range(0, h, stripe_h)]
    shapes = []
    for y0, vis_h, data, planes in stripes:
        dec, got = pc.decode_stripe(data, w, vis_h)
        pc.assert_planes_equal(planes, 0, got, f"{w}x{h} stripe y={y0}")
        shapes.append(got[0].shape)
    if (w, h) == (17, 17):
        assert shapes == [(16, 18), (2, 18)]


# ---- slice segments per CTU row -------------------------------------------------

# HIPFLUX_HEVC_SPR -> IDR NALs of an 80x32 stripe (5 CTUs x 2 rows): the
# row splits into ceil(5 / ceil(5 / spr)) segments
SPR_NALS = [(None, 2), (2, 4), (3, 6), (5, 10), (7, 10)]


@pytest.mark.parametrize("spr,nals", SPR_NALS,
                         ids=[f"spr{s}" for s, _ in SPR_NALS])
def test_segments_recon_equals_decoder(spr, nals):
    w, h = 80, 32
    img = pc.uniform_noise(w, h, 9)
    with pc.env_vars(HIPFLUX_HEVC_SPR=spr):
        out, dump = _native._pipeline_encode("cpu", [img], w, h, 30, 32,
                                             MODE, True)
    (y0, data), = pc.per_frame(out)[0]
    assert len(pc.idr_nals(data)) == nals
    dec, got = pc.decode_stripe(data, w, h)
    assert len(dec.qpc_used) == nals and len(dec.ctus) == 10
    pc.assert_planes_equal(pc.dump_planes(dump, h), 0, got, f"spr {spr}")


# ---- the CABAC output stride's premise -------------------------------------------

CONTENT = {"noise": lambda w, h: pc.uniform_noise(w, h, 3),
           "colour-checker": pc.colour_checker,
           "checkerboard": pc.checkerboard}


def test_stride_leaves_2x_headroom_at_qp0():
    """QP 0, one slice segment per row of 1, 8 and 20 CTUs: the largest
    IDR NAL (headers included) per CTU is at most half the bytes the HIP
    pipeline reserves per CTU. The CABAC kernel's writer has no bound, so
    this headroom is what keeps a worst-case slice inside its slot."""
    stride = _native.HEVC_BYTES_PER_CTU
    assert stride > 0 and _native.HEVC_FULLCOLOR_BYTES_PER_CTU >= stride
    worst = 0.0
    for name, make in CONTENT.items():
        for w in (16, 128, 320):
            data = _native.HevcEncoder(w, 16).encode(
                make(w, 16).tobytes(), qp=0)["data"]
            nal, = pc.idr_nals(data)
            per_ctu = len(nal) / (w // 16)
            print(f"{name} width {w}: {per_ctu:.0f} bytes per CTU")
            worst = max(worst, per_ctu)
    print(f"worst {worst:.0f} of {stride} bytes per CTU")
    assert worst <= stride / 2
