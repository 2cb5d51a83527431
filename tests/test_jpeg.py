"""CPU JPEG encoder vs an independent decoder (PIL/libjpeg), and vs a
float64 DCT through the from-spec coefficient decoder of jpeg_ref.py."""

import io
import math

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from PIL import Image


def psnr(a, b):
    mse = ((a.astype(np.int32) - b.astype(np.int32)) ** 2).mean()
    return 10 * math.log10(255 * 255 / max(mse, 1e-9))


def make_gradient(w, h):
    img = np.zeros((h, w, 4), np.uint8)
    img[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    img[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    img[:, :, 2] = 128
    img[:, :, 3] = 255
    return img


def decode(jpg):
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))


def bgrx_to_rgb(img):
    return np.stack([img[:, :, 2], img[:, :, 1], img[:, :, 0]], -1)


@pytest.mark.parametrize("fullcolor", [False, True])
def test_gradient_roundtrip(fullcolor):
    w, h = 320, 128
    img = make_gradient(w, h)
    jpg = hipflux.jpeg_encode(img.tobytes(), w, h, 90, fullcolor)
    dec = decode(jpg)
    assert dec.shape == (h, w, 3)
    p = psnr(dec, bgrx_to_rgb(img))
    assert p > 40, f"PSNR too low: {p:.1f} dB"


def test_noise_decodable():
    rng = np.random.default_rng(7)
    w, h = 256, 64
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    jpg = hipflux.jpeg_encode(img.tobytes(), w, h, 80, False)
    dec = decode(jpg)
    assert dec.shape == (h, w, 3)


def test_odd_dimensions():
    # non multiple-of-16 dims must still encode (edge replication)
    img = make_gradient(123, 45)
    jpg = hipflux.jpeg_encode(img.tobytes(), 123, 45, 85, False)
    dec = decode(jpg)
    assert dec.shape == (45, 123, 3)
    assert psnr(dec, bgrx_to_rgb(img)) > 35


def test_quality_monotonic():
    img = make_gradient(256, 64)
    sizes = [len(hipflux.jpeg_encode(img.tobytes(), 256, 64, q, False))
             for q in (30, 60, 90)]
    assert sizes[0] < sizes[1] < sizes[2]


def test_fullcolor_better_chroma():
    # saturated red/blue checkerboard: 4:4:4 should beat 4:2:0 clearly
    w, h = 128, 64
    img = np.zeros((h, w, 4), np.uint8)
    checker = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(bool)
    img[:, :, 2][checker] = 255      # red squares
    img[:, :, 0][~checker] = 255     # blue squares
    j420 = hipflux.jpeg_encode(img.tobytes(), w, h, 95, False)
    j444 = hipflux.jpeg_encode(img.tobytes(), w, h, 95, True)
    ref = bgrx_to_rgb(img)
    assert psnr(decode(j444), ref) > psnr(decode(j420), ref) + 3


def test_restart_interval_stream_decodes():
    """Restart-row framing (DRI + RSTn per MCU row — the GPU entropy
    kernel's structure) must produce streams PIL decodes identically to
    the continuous form."""
    import io
    import numpy as np
    from PIL import Image
    from hipflux import _native

    w, h = 128, 96
    rng = np.random.default_rng(17)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[:, :, 3] = 255
    # run both entropy framings over the same quantized blocks via the
    # native test hook (encode once per mode through the CPU pipeline
    # equivalence: jpeg_encode is continuous; _jpeg_restart is row-reset)
    cont = _native.jpeg_encode(img.tobytes(), w, h, 80, False)
    rst = _native._jpeg_encode_restart(img.tobytes(), w, h, 80, False)
    a = np.asarray(Image.open(io.BytesIO(bytes(cont))).convert("L"),
                   dtype=np.int16)
    b = np.asarray(Image.open(io.BytesIO(bytes(rst))).convert("L"),
                   dtype=np.int16)
    assert b.shape == (h, w)
    # same quantized coefficients -> identical pixels either framing
    assert np.abs(a - b).max() <= 1
    assert b"\xff\xdd" in bytes(rst)      # DRI present
    assert b"\xff\xd0" in bytes(rst)      # first RST marker


# ---- coefficients against a float64 DCT, through a from-spec decoder ---------
#
# jpeg_ref.decode_coeffs recovers every quantised coefficient of a stream,
# pad blocks included; jpeg_ref.reference_coeff_real computes the unrounded
# value each one must be a rounding of. The tests below establish both on
# the CPU encoder and on PIL, and show that the checker rejects the faults
# it exists for; the GPU tests (test_gpu_jpeg.py) lean on that.

import jpeg_ref
from hipflux import _native

REF_SIZES = [(False, 16, 16), (False, 17, 17), (False, 123, 45),
             (False, 328, 72), (True, 9, 9), (True, 324, 36)]
REF_QUALITIES = (1, 35, 80, 100)


def ref_content(kind, w, h):
    return (jpeg_ref.content_noise(w, h, 1000 + w) if kind == "noise"
            else jpeg_ref.content_structures(w, h))


@pytest.mark.parametrize("kind", ["noise", "structures"])
@pytest.mark.parametrize("fullcolor,w,h", REF_SIZES,
                         ids=[f"{'444' if f else '420'}-{w}x{h}"
                              for f, w, h in REF_SIZES])
def test_cpu_coefficients_round_the_float64_reference(fullcolor, w, h, kind):
    """Every coefficient of both CPU framings, at four qualities, is a
    rounding of the float64 reference; the two framings carry identical
    coefficients. This proves the plane emulation and the derived margin
    of check_coeffs against an encoder that is not under test."""
    img = ref_content(kind, w, h)
    mcu = 8 if fullcolor else 16
    for quality in REF_QUALITIES:
        cont = jpeg_ref.decode_coeffs(
            _native.jpeg_encode(img.tobytes(), w, h, quality, fullcolor))
        rst = jpeg_ref.decode_coeffs(
            _native._jpeg_encode_restart(img.tobytes(), w, h, quality,
                                         fullcolor))
        assert cont["dri"] == 0 and rst["dri"] == -(-w // mcu)
        for d in (cont, rst):
            assert (d["width"], d["height"], d["fullcolor"]) == \
                (w, h, fullcolor)
            ref = jpeg_ref.reference_coeff_real(img, w, h, d["qy"], d["qc"],
                                                fullcolor)
            stats = jpeg_ref.check_coeffs(d, ref)
            assert stats["checked"] == d["blocks"].size == \
                -(-w // mcu) * -(-h // mcu) * (3 if fullcolor else 6) * 64
        assert np.array_equal(cont["blocks"], rst["blocks"]), \
            f"quality {quality}: the framings carry different coefficients"


def test_coeff_decoder_agrees_with_pil():
    """Tables, size and pixels of the from-spec decoder against libjpeg,
    on 4:4:4 streams, so that no chroma upsampling is involved. A float64
    dequantise + IDCT of the decoded coefficients gives samples within 1
    of libjpeg's Y, Cb, Cr (the accuracy class of its integer IDCT), and
    after the JFIF colour conversion RGB within 2 levels of PIL's at every
    pixel. 2 holds while at most one of a pixel's three samples is off by
    that 1: 1.772 + two roundings of 0.5 < 3. Where libjpeg's IDCT moved
    two samples of one pixel (dense noise only), 1 + 1.772 + 1 < 4
    allows 3."""
    import PIL
    pil_natural_order = tuple(
        int(v) for v in PIL.__version__.split(".")[:2]) >= (8, 3)
    w, h = 324, 36
    for kind, quality in (("noise", 80), ("structures", 35),
                          ("structures", 100)):
        img = ref_content(kind, w, h)
        jpg = _native.jpeg_encode(img.tobytes(), w, h, quality, True)
        d = jpeg_ref.decode_coeffs(jpg)
        pil = Image.open(io.BytesIO(jpg))
        assert pil.size == (d["width"], d["height"]) == (w, h)
        for tid, tab in ((0, d["qy"]), (1, d["qc"])):
            # Pillow lists tables in natural order since 8.3, before
            # that in the stream's zig-zag order
            want = [int(v) for v in tab] if pil_natural_order \
                else [int(tab[k]) for k in jpeg_ref.ZIGZAG]
            assert list(pil.quantization[tid]) == want
        planes = []
        for slot, q in enumerate((d["qy"], d["qc"], d["qc"])):
            coef = (d["blocks"][:, :, slot] * q).astype(np.float64)
            my, mx = coef.shape[:2]
            pix = jpeg_ref.DCT.T @ coef.reshape(my, mx, 8, 8) @ jpeg_ref.DCT
            pix = pix.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:h, :w]
            # a decoder's IDCT hands 8-bit samples to its colour conversion
            planes.append(np.clip(np.rint(pix + 128.0), 0, 255))
        y, cb, cr = planes
        rgb = np.stack([y + 1.402 * (cr - 128),
                        y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128),
                        y + 1.772 * (cb - 128)], -1)
        rgb = np.clip(np.rint(rgb), 0, 255)
        diff = np.abs(rgb - np.asarray(pil.convert("RGB"), np.float64))
        ycc = Image.open(io.BytesIO(jpg))
        ycc.draft("YCbCr", (w, h))      # libjpeg's samples, unconverted
        assert ycc.mode == "YCbCr"
        off = np.abs(np.stack(planes, -1) - np.asarray(ycc, np.float64))
        assert off.max() <= 1, f"{kind} q{quality}: sample off by {off.max()}"
        allowed = np.where((off > 0).sum(-1) <= 1, 2, 3)[:, :, None]
        assert (diff <= allowed).all(), \
            f"{kind} q{quality}: RGB off by {diff.max()}"
        if kind == "structures":
            assert diff.max() <= 2


@pytest.fixture(scope="module")
def clean_328x72():
    """Decoded CPU stream of the 4:2:0 case with both pads 8 wide, with
    its reference: the base every mutant starts from (copied, never
    changed)."""
    w, h = 328, 72
    img = ref_content("structures", w, h)
    d = jpeg_ref.decode_coeffs(
        _native._jpeg_encode_restart(img.tobytes(), w, h, 80, False))
    ref = jpeg_ref.reference_coeff_real(img, w, h, d["qy"], d["qc"], False)
    jpeg_ref.check_coeffs(d, ref)
    return d, ref


def _mutants(d, ref):
    def mutant(fn):
        m = dict(d, blocks=d["blocks"].copy())
        fn(m["blocks"])
        return m

    def zero_right(b):
        b[:, -1, [1, 3]] = 0

    def zero_bottom(b):
        b[-1, :, [2, 3]] = 0

    # an MCU whose Cb and Cr differ, a luma block that is not symmetric
    cmy, cmx = np.argwhere(
        (d["blocks"][:, :, 4] != d["blocks"][:, :, 5]).any(-1))[0]
    luma = d["blocks"][:, :, :4].reshape(*d["blocks"].shape[:2], 4, 8, 8)
    tmy, tmx, tsl = np.argwhere(
        (luma != luma.transpose(0, 1, 2, 4, 3)).any((-1, -2)))[0]

    def swap_chroma(b):
        b[cmy, cmx, [4, 5]] = b[cmy, cmx, [5, 4]]

    def transpose(b):
        b[tmy, tmx, tsl] = b[tmy, tmx, tsl].reshape(8, 8).T.reshape(64)

    # a coefficient whose reference value is far from a rounding tie
    frac = np.abs(ref - np.floor(ref) - 0.5)
    my, mx, sl, k = np.argwhere((frac > 0.1) & (np.abs(ref) > 2))[0]

    def plus_one(b):
        b[my, mx, sl, k] += 1

    def chroma_quant_on_luma(b):
        # Y0 of the first MCU quantised with the chroma table
        b[0, 0, 0] = np.rint(ref[0, 0, 0] * d["qy"] / d["qc"])

    return {f.__name__: mutant(f) for f in (
        zero_right, zero_bottom, swap_chroma, transpose, plus_one,
        chroma_quant_on_luma)}


@pytest.mark.parametrize("name", [
    "zero_right", "zero_bottom", "swap_chroma", "transpose", "plus_one",
    "chroma_quant_on_luma"])
def test_checker_rejects_mutant(clean_328x72, name):
    """check_coeffs must fail on: pad luma blocks left at zero (right
    column: sub 1,3; bottom row: sub 2,3 — what a DCT launch sized by
    ceil(w/8) x ceil(h/8) leaves unwritten), Cb and Cr swapped, a
    transposed block, one coefficient off by one away from a tie, and a
    luma block quantised with the chroma table."""
    d, ref = clean_328x72
    m = _mutants(d, ref)[name]
    assert not np.array_equal(m["blocks"], d["blocks"]), "mutation is void"
    with pytest.raises(AssertionError, match="no rounding of the float64"):
        jpeg_ref.check_coeffs(m, ref)
    jpeg_ref.check_coeffs(d, ref)       # the base itself stayed clean


def test_coeff_decoder_rejects_damaged_streams():
    """A cleared pad bit, a changed RST number and a dropped last byte
    must each raise, as must leftovers after EOI."""
    w, h = 123, 45
    img = ref_content("noise", w, h)
    jpg = bytes(_native._jpeg_encode_restart(img.tobytes(), w, h, 80, False))
    d = jpeg_ref.decode_coeffs(jpg)
    assert jpg[-2:] == b"\xff\xd9" and len(d["pad_bits"]) == 3
    # an interval that closes with pad bits; its final byte sits before
    # the marker that ends it (behind a stuffed 00 if that byte is FF)
    sos = jpg.index(b"\xff\xda")
    ends = [jpg.index(b"\xff\xd0", sos), jpg.index(b"\xff\xd1", sos),
            len(jpg) - 2]
    at = next(e for e, pad in zip(ends, d["pad_bits"]) if pad) - 1
    if jpg[at] == 0 and jpg[at - 1] == 0xFF:
        at -= 1
    damaged = bytearray(jpg)
    damaged[at] &= 0xFE
    if jpg[at] == 0xFF:
        del damaged[at + 1]             # no longer FF: the stuffing goes too
    with pytest.raises(jpeg_ref.JpegError, match="pad bits"):
        jpeg_ref.decode_coeffs(bytes(damaged))

    first_rst = jpg.index(b"\xff\xd0")
    assert jpg.index(b"\xff\xd1") > first_rst
    damaged = bytearray(jpg)
    damaged[first_rst + 1] = 0xD3
    with pytest.raises(jpeg_ref.JpegError, match="RSTn"):
        jpeg_ref.decode_coeffs(bytes(damaged))

    with pytest.raises(jpeg_ref.JpegError):
        jpeg_ref.decode_coeffs(jpg[:-3] + jpg[-2:])
    with pytest.raises(jpeg_ref.JpegError, match="after EOI"):
        jpeg_ref.decode_coeffs(jpg + b"\x00")
    with pytest.raises(jpeg_ref.JpegError):
        jpeg_ref.decode_coeffs(jpg[:-2])
