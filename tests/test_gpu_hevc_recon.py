"""HEVC 4:2:0 on the HIP pipeline, on a real MI355X, pinned to the
from-spec decoder (hevc_ref_decoder.Decoder).

Every test asserts (a) the GPU's bytes equal the CPU pipeline's per frame
and per stripe, and (b) for every stripe encoded in the last frame that
encoded, the recon planes k_hevc_rows wrote (debug dump: curY at rows
y0.., curCb/curCr at rows y0/2..) equal what the decoder reconstructs from
the GPU's own stream, over the decoder's output shape (the visible size
rounded up to even). Every comparison is exact.

tests/test_hevc_recon_host.py pins the CPU encoder to the same decoder on
the same inputs without a GPU; if a test here fails, run that file first."""

import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
import pipeline_content as pc

MODE = 2   # output_mode of the HEVC pipelines


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


def byte_differences(got, want, what):
    """GPU against CPU stripes per frame: a list of what differs."""
    assert len(got) == len(want)
    diffs = []
    for fi, (fg, fw) in enumerate(zip(got, want)):
        if [y for y, _ in fg] != [y for y, _ in fw]:
            diffs.append(f"{what}: frame {fi} emits stripes "
                         f"{[y for y, _ in fg]}, the CPU "
                         f"{[y for y, _ in fw]}")
            continue
        diffs += [f"{what}: frame {fi} stripe y={y} differs from the CPU "
                  f"({len(a)} vs {len(b)} bytes)"
                  for (y, a), (_, b) in zip(fg, fw) if a != b]
    return diffs


def check(frames, w, h, qp, stripe_h, what, depth=1, mask=None):
    """(a) and (b) of the module docstring; both are evaluated before
    either fails, so a report says whether bytes, recon or both are off.
    Returns (GPU stripes per frame, the decoders of the last encoded
    frame's stripes)."""
    require_gpu()
    frames = list(frames)
    out, dump = _native._pipeline_encode(
        "gpu", frames, w, h, qp, stripe_h, MODE, True, False,
        pipeline_depth=depth, encode_mask=mask)
    gpu = pc.per_frame(out)
    cpu = pc.per_frame(_native._pipeline_encode(
        "cpu", frames, w, h, qp, stripe_h, MODE, False, False,
        encode_mask=mask))
    problems = byte_differences(gpu, cpu, what)
    assert (dump["w"], dump["h"]) == (w, h)
    assert dump["ypitch"] == (w + 15) & ~15
    assert dump["cpitch"] == dump["ypitch"] // 2
    planes = pc.dump_planes(dump, h)
    last = [fr for fr in gpu if fr][-1]
    decs = []
    for y0, data in last:
        try:
            dec, got = pc.decode_stripe(data, w, min(stripe_h, h - y0))
            decs.append(dec)
            pc.assert_planes_equal(planes, y0, got,
                                   f"{what}: stripe y={y0}")
        except Exception as e:   # a wrong stream may not even parse
            problems.append(f"{what}: stripe y={y0} recon: "
                            f"{type(e).__name__}: {e}")
    assert not problems, "\n".join(problems)
    return gpu, decs


# ---- 1. QP sweep ---------------------------------------------------------------

# 0 and 51: clip16d, the lv > 32767 clamp, long escape codes. 29/30 and
# 43/44: where Table 8-10 changes shape. 26 and 34: mode and cbf coverage.
@pytest.mark.parametrize("qp", [0, 17, 26, 29, 30, 34, 36, 43, 44, 51])
def test_qp_sweep(qp):
    w, h = 161, 75
    gpu, decs = check(pc.frames_for(w, h, 2), w, h, qp, 32, f"qp {qp}")
    assert [[y for y, _ in fr] for fr in gpu] == [[0, 32, 64]] * 2
    for dec in decs:
        assert set(dec.qpc_used) == {pc.spec_chroma_qp(qp)}
    if qp in (26, 34):
        pc.assert_full_coverage(decs, f"161x75 qp {qp}")


# ---- 2. sizes --------------------------------------------------------------------

SIZES = [(16, 16, 16), (17, 17, 16), (15, 33, 32), (1, 1, 16), (161, 75, 32)]


@pytest.mark.parametrize("w,h,stripe_h", SIZES,
                         ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_sizes(w, h, stripe_h):
    """Noise at QP 22: one CTU, a stripe with one visible row, a partial
    last stripe, the minimum picture, stripes of 32, 32 and 11 rows. Odd
    sizes clamp the chroma reads at cw = (w + 1) >> 1 and decode one
    sample larger than the visible picture."""
    gpu, decs = check([pc.uniform_noise(w, h, 5)], w, h, 22, stripe_h,
                      f"{w}x{h}")
    assert [y for y, _ in gpu[0]] == list(range(0, h, stripe_h))


# ---- 3. slice segments per CTU row ----------------------------------------------

@pytest.mark.parametrize("spr,nals", [(2, 4), (3, 6), (5, 10), (7, 10)])
def test_segments_noise(spr, nals):
    """80x32 (5 CTUs x 2 rows): a segment that starts in mid-row has no
    left neighbour and no left mode, and carries its slice address."""
    w, h = 80, 32
    with pc.env_vars(HIPFLUX_HEVC_SPR=spr):
        gpu, decs = check([pc.uniform_noise(w, h, 9)], w, h, 30, 32,
                          f"spr {spr}")
    (y0, data), = gpu[0]
    assert len(pc.idr_nals(data)) == nals
    assert len(decs[0].ctus) == 10


def test_segments_coverage_content():
    """161x75 with 3 segments per row: 11 CTUs split 4, 4, 3."""
    w, h = 161, 75
    with pc.env_vars(HIPFLUX_HEVC_SPR=3):
        gpu, decs = check(pc.frames_for(w, h, 2), w, h, 26, 32, "spr 3")
    for (y0, data), rows in zip(gpu[-1], (2, 2, 1)):
        assert len(pc.idr_nals(data)) == 3 * rows
    assert sum(len(d.ctus) for d in decs) == 11 * 5


# ---- 4. extremes -------------------------------------------------------------------

@pytest.mark.parametrize("qp", [0, 51])
@pytest.mark.parametrize("content", ["noise", "colour-checker"])
def test_extremes(content, qp):
    w, h = 128, 16
    img = pc.uniform_noise(w, h, 3) if content == "noise" \
        else pc.colour_checker(w, h)
    check([img], w, h, qp, 16, f"{content} qp {qp}")


# ---- 5. damage mask and depth 2 ------------------------------------------------------

MASK = [[True, True, True], [False, False, False],
        [False, True, False], [True, False, True]]


def test_mask_and_depth():
    """A frame in which nothing encodes, with and without a frame in
    flight; the stripes emitted follow the mask, depth 2 equals depth 1
    (both equal the CPU), and recon holds for the last frame's stripes."""
    w, h = 96, 48
    frames = pc.frames_for(w, h, 4)
    runs = []
    for depth in (1, 2):
        gpu, decs = check(frames, w, h, 30, 16, f"depth {depth}",
                          depth=depth, mask=MASK)
        assert [[y for y, _ in fr] for fr in gpu] == \
            [[0, 16, 32], [], [16], [0, 32]]
        assert len(decs) == 2
        runs.append(gpu)
    assert runs[0] == runs[1]


# ---- 6. read-back growth ---------------------------------------------------------------

def test_readback_growth():
    """Flat, flat, mix, flat, mix at QP 10, where mix has noise in its
    first CTU row only. A flat frame leaves the compacted read-back a cap
    of max(4096, 2 * max_count) = 4096 bytes; the noise row outgrows it
    and is fetched again exactly, while its neighbour is not."""
    w, h, qp = 320, 32, 10
    flat, mix = pc.flat_and_mix(w, h)
    frames = [flat, flat, mix, flat, mix]
    cpu = pc.per_frame(_native._pipeline_encode("cpu", frames, w, h, qp, 32,
                                                MODE))
    sizes = [[len(n) for n in pc.idr_nals(fr[0][1])] for fr in cpu]
    print("IDR NAL bytes per frame:", sizes)
    for fi, (row0, row1) in enumerate(sizes):
        if fi in (2, 4):
            assert row0 > 6000 and row1 < 100
        else:
            assert row0 < 100 and row1 < 100
    for depth in (2, 1):
        check(frames, w, h, qp, 32, f"growth depth {depth}", depth=depth)
