"""HEVC fullcolor (Main 4:4:4) on the CPU encoder and the CPU pipeline,
checked against the from-spec decoder (hevc444_ref_decoder.Decoder444).

Every recon comparison is exact, for all three planes. The fixture is a
colour gradient with a flat patch, a noise band, 1-pixel alternating-chroma
columns and 2-pixel horizontal stripes; at 321x149 it makes the encoder
choose each of Planar/DC/H/V and leave each cbf flag both set and clear,
which the tests assert from the decoder's own record."""

import functools
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from hipflux import _native
import hevc_ref_decoder as hrd
from hevc444_ref_decoder import Decoder444

WEB = pathlib.Path(__file__).resolve().parents[2] / "selkies_amd" / "web"

QPS = [0, 18, 30, 42, 51]
SIZES = [(16, 16), (48, 32), (321, 149)]


@functools.lru_cache(maxsize=None)
def _fixture(w, h):
    rng = np.random.default_rng(11)
    img = np.zeros((h, w, 4), np.uint8)
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    img[:, :, 0] = (x * 255 // max(1, w - 1)).astype(np.uint8)
    img[:, :, 1] = (y * 255 // max(1, h - 1)).astype(np.uint8)
    img[:, :, 2] = 96
    img[:min(16, h), :min(32, w), :3] = (40, 90, 200)      # flat patch
    b0, band = h // 2, max(1, min(8, h // 4))
    img[b0:b0 + band, :, :3] = rng.integers(0, 256, (band, w, 3),
                                            dtype=np.uint8)
    c0 = w // 2                       # 1-pixel alternating-chroma columns
    n = min(16, w - c0)
    odd = np.arange(n) & 1
    img[:, c0:c0 + n, 0] = np.where(odd, 255, 0)[None, :]
    img[:, c0:c0 + n, 2] = np.where(odd, 0, 255)[None, :]
    img[:, c0:c0 + n, 1] = 128
    if w >= 48:                       # 2-pixel horizontal stripes
        rows = (np.arange(h) // 2) & 1
        img[:, w - 16:, :3] = np.where(rows, 200, 60)[:, None, None]
    img[:, :, 3] = 255
    img.setflags(write=False)
    return img


def fixture(w, h):
    """Built once per size and shared; read-only."""
    return _fixture(w, h)


def bgrx_to_i444(img):
    """Full-range BT.601 (JFIF) chroma, the encoder's colour conversion, in
    float64 and unrounded: the I444 source of the fidelity comparison."""
    b, g, r = (img[:, :, i].astype(np.float64) for i in range(3))
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b + 128
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b + 128
    return cb, cr


def pipeline_cpu(img, w, h, qp, fullcolor, dump=False):
    """One frame through the CPU HEVC pipeline as a single stripe."""
    stripe_h = (h + 15) & ~15
    return _native._pipeline_encode("cpu", [img], w, h, qp, stripe_h, 2,
                                    dump, fullcolor=fullcolor)


def dump_planes(dump, w, h):
    yh = (h + 15) & ~15
    return [np.frombuffer(dump[k], np.uint8).reshape(yh, dump[p])[:h, :w]
            for k, p in (("y", "ypitch"), ("cb", "cpitch"), ("cr", "cpitch"))]


# ---- 1. the flag acts (fails on a build without HEVC fullcolor) ------------

def test_pipeline_fullcolor_is_main444():
    w, h, qp = 64, 64, 30
    out = _native._pipeline_encode("cpu", [fixture(w, h)], w, h, qp, 64, 2,
                                   fullcolor=True)
    data = bytes(out[0][0][0])
    dec = Decoder444()
    frames = dec.decode(data)
    assert dec.sps["chroma_format_idc"] == 3
    assert dec.sps["profile_idc"] == 4
    assert [p.shape for p in frames[0]] == [(h, w)] * 3


# ---- 2. encoder recon == decoder output, all three planes ------------------

@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("w,h", SIZES)
def test_recon_equals_decoder(w, h, qp):
    out, dump = pipeline_cpu(fixture(w, h), w, h, qp, True, dump=True)
    assert dump["cpitch"] == dump["ypitch"]
    dec = Decoder444()
    frames = dec.decode(bytes(out[0][0][0]))
    assert len(frames) == 1 and dec.sps["chroma_format_idc"] == 3
    assert (dec.sps["w"], dec.sps["h"]) == (w, h)   # crop in units of 1
    for name, got, want in zip("y cb cr".split(), dump_planes(dump, w, h),
                               frames[0]):
        assert want.shape == (h, w)
        assert np.array_equal(got, want), f"{w}x{h} qp {qp}: plane {name}"
    if (w, h) == (321, 149):
        modes = {c[0] for c in dec.ctus}
        assert modes == {0, 1, 10, 26}, f"modes chosen: {sorted(modes)}"
        for i, name in ((1, "cbf_luma"), (2, "cbf_cb"), (3, "cbf_cr")):
            assert {c[i] for c in dec.ctus} == {0, 1}, \
                f"qp {qp}: {name} never both set and clear"


def test_encoder_class_recon_equals_decoder():
    """HevcEncoder(fullcolor=True): recon() returns full-size chroma."""
    w, h, qp = 48, 32, 24
    enc = _native.HevcEncoder(w, h, fullcolor=True)
    r = enc.encode(fixture(w, h).tobytes(), qp=qp)
    y, cb, cr, yp, cp = enc.recon()
    assert cp == yp and len(cb) == len(y) == len(cr)
    frames = Decoder444().decode(r["data"])
    for buf, want in zip((y, cb, cr), frames[0]):
        got = np.frombuffer(buf, np.uint8).reshape(-1, yp)[:h, :w]
        assert np.array_equal(got, want)


def test_split_rows_recon_equals_decoder():
    """Two slice segments per CTU row (slices_per_row=2)."""
    w, h, qp = 80, 32, 26
    enc = _native.HevcEncoder(w, h, slices_per_row=2, fullcolor=True)
    r = enc.encode(fixture(w, h).tobytes(), qp=qp)
    y, cb, cr, yp, cp = enc.recon()
    frames = Decoder444().decode(r["data"])
    for buf, want in zip((y, cb, cr), frames[0]):
        got = np.frombuffer(buf, np.uint8).reshape(-1, yp)[:h, :w]
        assert np.array_equal(got, want)


# ---- 3. parameter-set bytes, written out from the rules ---------------------

# profile_tier_level, 12 bytes:
#   0x04                  profile_space 00, tier 0, profile_idc 00100
#   0x08 00 00 00         compatibility flag 4 only
#   0xBE                  progressive 1, interlaced 0, non_packed 1,
#                         frame_only 1, max_12bit 1, max_10bit 1,
#                         max_8bit 1, max_422chroma 0
#   0x08                  max_420chroma 0, max_monochrome 0, intra 0,
#                         one_picture_only 0, lower_bit_rate 1, 3 of the 34
#                         reserved zero bits
#   0x00 00 00 00         31 reserved zero bits, reserved bit
#   0x7B                  level_idc 123 (4.1; 64x64 is far below its limit)
# In a NAL the two runs 00 00 00 get an emulation-prevention 03 each.
PTL_444_EP = bytes.fromhex("04 08 00 00 03 00 BE 08 00 00 03 00 00 7B")

# VPS: start code, NAL header (type 32), 0C 01 (vps id 0, base layer flags
# 1 1, max_layers 0, max_sub_layers 0, nesting 1), FF FF, PTL, then
# 1 | ue(0) ue(0) ue(0) | 000000 | ue(0) | 0 | 0 | stop bit, padded: F0 24
VPS_444 = (bytes.fromhex("00 00 00 01 40 01 0C 01 FF FF") + PTL_444_EP
           + bytes.fromhex("F0 24"))

# SPS for 64x64: start code, NAL header (type 33), 01 (vps id 0,
# max_sub_layers 0, nesting 1), PTL, then the bit string
#   1            sps id ue(0)
#   00100        chroma_format_idc ue(3)
#   0            separate_colour_plane_flag
#   0000001000001 x2   width, height ue(64)
#   0            conformance_window_flag (64 is CTU-aligned)
#   1 1          bit depths ue(0)
#   00101        log2_max_poc_lsb_minus4 ue(4)
#   1 111        sub_layer_ordering_info_present, three ue(0)
#   1 010 1 011  min CB 8, CTU 16, min TB 4, max TB 16
#   1 1          transform hierarchy depths ue(0)
#   0000         scaling list, amp, sao, pcm
#   1            num_short_term_ref_pic_sets ue(0)
#   00000        long_term, temporal_mvp, strong_smoothing, vui, extension
#   1            stop bit, then zero padding
# = 90 04 10 20 B2 FD 5E 10 40
SPS_444_64 = (bytes.fromhex("00 00 00 01 42 01 01") + PTL_444_EP
              + bytes.fromhex("90 04 10 20 B2 FD 5E 10 40"))


def test_parameter_set_bytes_pinned():
    w = h = 64
    enc = _native.HevcEncoder(w, h, fullcolor=True)
    data = enc.encode(fixture(w, h).tobytes(), qp=30)["data"]
    assert data[:len(VPS_444)] == VPS_444
    assert data[len(VPS_444):len(VPS_444) + len(SPS_444_64)] == SPS_444_64
    dec = Decoder444()
    dec.decode(data)
    assert dec.ptl["rext"] == (1, 1, 1, 0, 0, 0, 0, 0, 1)
    assert dec.ptl["compat"] == 0x08000000 and dec.ptl["level_idc"] == 123


def test_odd_size_crop_is_exact():
    """4:4:4 crops in units of one sample: 321x149 is signalled as such
    (4:2:0 can only signal even sizes)."""
    w, h = 321, 149
    dec = Decoder444()
    dec.decode(bytes(pipeline_cpu(fixture(w, h), w, h, 30, True)[0][0][0]))
    assert (dec.sps["cw"], dec.sps["ch"]) == (336, 160)
    assert (dec.sps["w"], dec.sps["h"]) == (321, 149)


# ---- 4. chroma QP -----------------------------------------------------------

def test_chroma_qp_is_min_qpi_51():
    """At qp 40 the 4:2:0 table gives QpC 36; ChromaArrayType 3 uses
    Min(qPi, 51) = 40. Only the latter reproduces the encoder's chroma."""
    w, h, qp = 48, 32, 40
    assert hrd.chroma_qp(qp) == 36
    out, dump = pipeline_cpu(fixture(w, h), w, h, qp, True, dump=True)
    data = bytes(out[0][0][0])
    want = dump_planes(dump, w, h)
    dec = Decoder444()
    got = dec.decode(data)[0]
    assert set(dec.qpc_used) == {40}
    assert 36 not in dec.qpc_used
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    wrong = Decoder444(qpc_override=hrd.chroma_qp)
    bad = wrong.decode(data)[0]
    assert set(wrong.qpc_used) == {36}
    assert np.array_equal(bad[0], want[0])            # luma unaffected
    assert not np.array_equal(bad[1], want[1]) or \
        not np.array_equal(bad[2], want[2])


# ---- 5. fidelity ------------------------------------------------------------

def test_chroma_fidelity_beats_420():
    """1-pixel alternating-chroma columns: decoded 4:4:4 chroma is strictly
    closer to the I444 source than 4:2:0 chroma nearest-upsampled."""
    w, h, qp = 64, 32, 22
    img = np.zeros((h, w, 4), np.uint8)
    odd = np.arange(w) & 1
    img[:, :, 0] = np.where(odd, 255, 0)[None, :]
    img[:, :, 2] = np.where(odd, 0, 255)[None, :]
    img[:, :, 1] = 128
    img[:, :, 3] = 255
    src_cb, src_cr = bgrx_to_i444(img)
    d444 = Decoder444().decode(
        bytes(pipeline_cpu(img, w, h, qp, True)[0][0][0]))[0]
    d420 = Decoder444().decode(
        bytes(pipeline_cpu(img, w, h, qp, False)[0][0][0]))[0]
    assert d420[1].shape == (h // 2, w // 2)
    for i, src in ((1, src_cb), (2, src_cr)):
        up = np.repeat(np.repeat(d420[i], 2, axis=0), 2, axis=1)
        mse444 = ((d444[i].astype(np.float64) - src) ** 2).mean()
        mse420 = ((up.astype(np.float64) - src) ** 2).mean()
        print(f"plane {i}: mse 4:4:4 {mse444:.1f}  4:2:0 {mse420:.1f}")
        assert mse444 < mse420


# ---- 6. 4:2:0 is untouched --------------------------------------------------

def test_fullcolor_false_equals_default():
    w, h, qp = 96, 48, 28
    img = fixture(w, h).tobytes()
    a = _native.HevcEncoder(w, h, 1, fullcolor=False).encode(img, qp=qp)
    b = _native.HevcEncoder(w, h).encode(img, qp=qp)
    assert a["data"] == b["data"]
    dec = Decoder444()
    dec.decode(a["data"])
    assert dec.sps["chroma_format_idc"] == 1 and dec.sps["profile_idc"] == 1
    # and the parent decoder still reads it
    assert len(hrd.Decoder().decode(a["data"])) == 1


# ---- 7. web client codec string ----------------------------------------------

JS_HARNESS = """
const fs = require("fs");
const src = fs.readFileSync(process.argv[2], "utf8");
const m = src.match(/\\/\\* hevcCodecString:begin[\\s\\S]*?hevcCodecString:end \\*\\//);
if (!m) { console.error("marker block not found"); process.exit(2); }
const hevcCodecString = new Function(m[0] + "; return hevcCodecString;")();
const out = process.argv.slice(3).map(
  (hex) => hevcCodecString(Uint8Array.from(Buffer.from(hex, "hex"))));
process.stdout.write(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node not available")
def test_js_codec_string_follows_stream(tmp_path):
    import json
    w, h = 64, 64
    img = fixture(w, h).tobytes()
    s420 = _native.HevcEncoder(w, h).encode(img, qp=30)["data"]
    s444 = _native.HevcEncoder(w, h, fullcolor=True).encode(img, qp=30)["data"]
    assert s420[10] & 0x1F == 1 and s444[10] & 0x1F == 4
    harness = tmp_path / "run.js"
    harness.write_text(JS_HARNESS)
    r = subprocess.run(
        ["node", str(harness), str(WEB / "selkies-client.js"),
         s420[:64].hex(), s444[:64].hex()],
        capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == ["hev1.1.6.L123.B0", "hev1.4.10.L123.BE.8"]
