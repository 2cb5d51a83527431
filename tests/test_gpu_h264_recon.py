"""GPU H.264 reconstruction pinned to the from-spec decoder on a real
MI355X: the deblock / recon / reference-refresh chain.

Every comparison is exact (np.array_equal) on all three planes over the
full MB-aligned pitch — including the padding right of / below the
picture, because motion search reads it as reference. The debug dump
holds only the final frame's reference planes, so per-frame equality
comes from encoding every prefix frames[:k].

Content is h264_content.mixed_frames (skip, inter and intra MBs inside
P slices, every deblock strength, real chroma residual); its coverage
is guarded without a GPU by tests/test_h264_content.py."""

import contextlib
import functools
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_content import CountingDecoder, count_slice_nals, mixed_frames

N = 4
STRIPE_H = 48


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


@contextlib.contextmanager
def env_vars(**kv):
    """Set environment knobs around a pipeline construction (they are
    read when the pipeline is built) and restore them afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def frames_for(w, h, n):
    """mixed_frames, built once per size and never modified."""
    return tuple(mixed_frames(w, h, n))


def gpu_encode(w, h, qp, k=N, n=N, dump=True, **kw):
    """Encode the first k of n mixed frames on the GPU pipeline."""
    frames = list(frames_for(w, h, n)[:k])
    return _native._pipeline_encode("gpu", frames, w, h, qp, STRIPE_H, 1,
                                    dump, **kw)


def stripe_chunks(out):
    """frames -> {stripe y0: [bytes of each frame it was encoded in]}"""
    rows = {}
    for frame in out:
        for data, y, hgt, key in frame:
            rows.setdefault(y, []).append(bytes(data))
    return rows


def per_frame_bytes(out):
    return [sorted((y, bytes(d)) for d, y, hgt, key in fr) for fr in out]


def dump_planes(dump):
    yp, cp = dump["ypitch"], dump["cpitch"]
    return (np.frombuffer(dump["y"], np.uint8).reshape(-1, yp),
            np.frombuffer(dump["cb"], np.uint8).reshape(-1, cp),
            np.frombuffer(dump["cr"], np.uint8).reshape(-1, cp))


def stripe_mb_rows(y0, h, stripe_h):
    return (min(y0 + stripe_h, h) - y0 + 15) // 16


def assert_planes_equal(planes, dump, w, h, stripe_h, y0, what="decoder"):
    """planes: one stripe's uncropped (y, cb, cr); compare with the dump
    region luma rows [y0, y0 + rows*16), chroma rows [y0/2, y0/2 +
    rows*8), full pitch width."""
    mbw = (w + 15) // 16
    rows = stripe_mb_rows(y0, h, stripe_h)
    assert dump["ypitch"] == mbw * 16 and dump["cpitch"] == mbw * 8
    for name, dp, gp, r0, nr, width in zip(
            ("y", "cb", "cr"), planes, dump_planes(dump),
            (y0, y0 // 2, y0 // 2), (rows * 16, rows * 8, rows * 8),
            (mbw * 16, mbw * 8, mbw * 8)):
        assert dp.shape == (nr, width), \
            f"stripe y={y0} plane {name}: {what} shape {dp.shape}"
        region = gp[r0:r0 + nr, :width]
        assert region.shape == dp.shape, \
            f"stripe y={y0} plane {name}: dump region {region.shape}"
        if not np.array_equal(dp, region):
            diff = np.argwhere(dp != region)
            r, c = (int(v) for v in diff[0])
            pytest.fail(
                f"stripe y={y0} plane {name}: first difference at "
                f"(row {r}, col {c}): {what} {int(dp[r, c])} != GPU "
                f"{int(region[r, c])}; {len(diff)} samples differ")


def assert_recon_equals_decoder(out, dump, w, h, stripe_h, known=None):
    """Decode every stripe stream of `out` and require the decoder's
    uncropped planes of its last frame to equal the GPU dump region.

    `known` ({y0: (chunks, decoder)} from an earlier call on a longer
    run) saves decode time only: when this run's stream is byte-for-byte
    a prefix of the known one, the known decoder's planes after that
    many frames ARE this stream's decode. Returns {y0: (chunks,
    decoder)}."""
    decoded = {}
    chunks_by_y = stripe_chunks(out)
    assert chunks_by_y, "nothing was encoded"
    for y0, chunks in sorted(chunks_by_y.items()):
        dec = None
        if known and y0 in known and known[y0][0][:len(chunks)] == chunks:
            dec = known[y0][1]
        if dec is None:
            dec = CountingDecoder()
            frames = dec.decode(b"".join(chunks))
            assert len(frames) == len(chunks), (
                f"stripe y={y0}: decoded {len(frames)} frames from "
                f"{len(chunks)} encoded")
        assert_planes_equal(dec.uncropped[len(chunks) - 1], dump, w, h,
                            stripe_h, y0)
        decoded[y0] = (chunks, dec)
    return decoded


def check_all_prefixes(w, h, qp, ks=tuple(range(N, 0, -1)), **kw):
    """Decoder equality of the dump after frames[:k] for every k in ks
    (longest first, so shorter runs reuse its decode when their bytes
    are a prefix). Returns the longest run's (out, dump, decoded)."""
    first = None
    known = None
    for k in ks:
        out, dump = gpu_encode(w, h, qp, k=k, **kw)
        assert len(out) == k
        decoded = assert_recon_equals_decoder(out, dump, w, h, STRIPE_H,
                                              known)
        if first is None:
            first = (out, dump, decoded)
            known = decoded
    return first


def coverage(decoded):
    skip = inter = intra_p = 0
    bs = {k: 0 for k in range(5)}
    for chunks, dec in decoded.values():
        skip += dec.skip
        inter += dec.inter
        intra_p += dec.intra_in_p
        for k in bs:
            bs[k] += dec.bs[k]
    return skip, inter, intra_p, bs


# ---- QP sweep ---------------------------------------------------------------

@pytest.mark.parametrize("qp", [14, 17, 24, 30, 38, 45, 51])
def test_gpu_recon_qp_sweep(qp):
    """256x96 (16x6 MBs, two 3-row stripes), every prefix, three planes.
    qp 14: indexA < 16, alpha = beta = 0, the filter must be a no-op;
    17: the first non-zero table entries; 24..38: around the chroma QP
    knee at 30; 45/51: the steep end of the tc0 table."""
    require_gpu()
    w, h = 256, 96
    out, dump, decoded = check_all_prefixes(w, h, qp)
    assert sorted(decoded) == [0, 48]
    skip, inter, intra_p, bs = coverage(decoded)
    print(f"GPU {w}x{h} qp {qp}: skip={skip} inter={inter} "
          f"intra_in_p={intra_p} bs={bs}")
    if qp == 24:
        # floors far below the CPU pipeline's figures (104 / 73 / 111):
        # the GPU motion search is not the CPU's
        assert skip >= 10, skip
        assert inter >= 10, inter
        assert intra_p >= 10, intra_p
        for k in (1, 2, 3, 4):
            assert bs[k] >= 1, f"bS {k} never occurs: {bs}"
    if qp == 14:
        # alpha(14) = beta(14) = 0: in-loop deblocking must do nothing.
        # The test hook cannot switch video_deblock off, so the no-op is
        # shown through the decoder: its spec filter ran over every
        # edge (the streams signal idc=2) and altered no sample, and the
        # GPU planes equal the decoder's for every frame (above) — so
        # the GPU planes are the unfiltered reconstruction.
        assert sum(bs[k] for k in (1, 2, 3, 4)) > 0
        for y0, (chunks, dec) in decoded.items():
            assert dec.db_changed == 0, f"stripe y={y0}"
    if qp >= 17:
        assert sum(dec.db_changed for _, dec in decoded.values()) > 0


# ---- unaligned size ---------------------------------------------------------

@pytest.mark.parametrize("qp", [24, 38])
def test_gpu_recon_unaligned(qp):
    """250x90: crop 6 right, last stripe 42 rows with crop 6 bottom.
    Clamped source reads, SPS cropping, the partial last stripe and the
    padded recon that ME reads — every prefix, three planes, padding
    included."""
    require_gpu()
    w, h = 250, 90
    out, dump, decoded = check_all_prefixes(w, h, qp)
    assert sorted(decoded) == [0, 48]
    want = {0: ((48, 250), (24, 125)), 48: ((42, 250), (21, 125))}
    for y0, (chunks, dec) in decoded.items():
        assert len(dec.frames) == N
        for fy, fcb, fcr in dec.frames:
            assert (fy.shape, fcb.shape, fcr.shape) == \
                (want[y0][0], want[y0][1], want[y0][1])


# ---- mid-row slices ---------------------------------------------------------

@pytest.mark.parametrize("segs", [3, 16])
@pytest.mark.parametrize("w,h", [(256, 96), (250, 90)])
def test_gpu_recon_midrow_slices(w, h, segs):
    """HIPFLUX_SEGS splits each 16-MB row into slices (3 -> 6, 6, 4 MBs;
    16 -> one MB per slice, so no MB-edge filtering at all): a
    segment's first vertical edge is a slice boundary and must not be
    filtered (idc=2). Only SEGS with (segs-1)*ceil(mbw/segs) < mbw are
    legal here."""
    require_gpu()
    qp = 30
    mbw = (w + 15) // 16
    assert (segs - 1) * -(-mbw // segs) < mbw
    with env_vars(HIPFLUX_SEGS=segs):
        out, dump, decoded = check_all_prefixes(w, h, qp, ks=(N, 2))
        with env_vars(HIPFLUX_CPU_ENTROPY=1):
            cpu_ent = gpu_encode(w, h, qp, dump=False)
    # slice NALs per picture = MB rows x segments
    for y0, (chunks, dec) in decoded.items():
        rows = stripe_mb_rows(y0, h, STRIPE_H)
        assert len(chunks) == N
        for fi, chunk in enumerate(chunks):
            assert count_slice_nals(chunk) == rows * segs, \
                f"stripe y={y0} frame {fi}"
        firsts = sorted({fm for _, fm, _ in dec.slices})
        seg_w = -(-mbw // segs)
        assert firsts == sorted(r * mbw + x for r in range(rows)
                                for x in range(0, mbw, seg_w))
    # GPU CAVLC == CPU packer over the segmented job list
    assert per_frame_bytes(out) == per_frame_bytes(cpu_ent)


# ---- recorded P streams -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def p_stream_fixture():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "golden", "h264_p_streams.json")
    with open(path) as f:
        doc = json.load(f)
    assert (doc["content"], doc["frames"], doc["stripe_height"],
            doc["pipeline_depth"]) == ("mixed_frames", N, STRIPE_H, 1)
    return {(c["w"], c["h"], c["qp"]): c["streams"] for c in doc["cases"]}


@pytest.mark.parametrize("qp", [24, 38])
@pytest.mark.parametrize("w,h", [(256, 96), (250, 90)])
def test_gpu_p_streams_match_fixture(w, h, qp):
    """The only pin on the row kernel's P-frame levels (inter dead zone,
    the 12-coefficient cap): decoder equality shows recon and stream agree
    with each other, IDR byte equality covers intra only. Every (frame,
    stripe) stream must hash to tests/golden/h264_p_streams.json, which
    was recorded from the retired 2-wave row kernel — an implementation
    sharing no structure with the shipped one — and not from the code
    under test."""
    require_gpu()
    want = p_stream_fixture()[(w, h, qp)]
    out, _ = gpu_encode(w, h, qp)
    got = per_frame_bytes(out)
    case = f"{w}x{h} qp {qp}"
    assert len(got) == len(want) == N, case
    for fi in range(N):
        assert [str(y) for y, _ in got[fi]] == sorted(want[fi], key=int), \
            f"{case} frame {fi}: stripes encoded"
        for y0, data in got[fi]:
            rec = want[fi][str(y0)]
            assert (hashlib.sha256(data).hexdigest(), len(data)) == \
                (rec["sha256"], rec["length"]), (
                f"{case} frame {fi} stripe y={y0}: stream of {len(data)} "
                f"bytes differs from the fixture's {rec['length']} bytes, "
                "which was recorded from the retired 2-wave row kernel")


# ---- damage-gated stripes ---------------------------------------------------

DAMAGE_MASKS = [[True, True, True], [True, False, True],
                [False, True, False], [True, True, False],
                [False, False, False], [False, True, True]]


@pytest.mark.parametrize("w,h", [(256, 144), (250, 138)])
def test_gpu_recon_damage_gated(w, h):
    """The production shape: only some stripes are encoded per frame.
    The reference refresh merges contiguous encoded spans and must leave
    every other stripe's reference untouched; a stripe's frame_num
    advances only when it is encoded. Three 48-row stripes (48/48/42 at
    250x138), six frames."""
    require_gpu()
    qp, n = 30, len(DAMAGE_MASKS)
    out, dump = gpu_encode(w, h, qp, k=n, n=n, encode_mask=DAMAGE_MASKS)
    assert len(out) == n
    for fi, fr in enumerate(out):
        assert sorted(y for _, y, _, _ in fr) == \
            [y for y, m in zip((0, 48, 96), DAMAGE_MASKS[fi]) if m]
    # final dump == each stripe's last decoded frame, stripe 0 included
    # (not encoded in the last two frames: its reference must be intact)
    decoded = assert_recon_equals_decoder(out, dump, w, h, STRIPE_H)
    assert sorted(decoded) == [0, 48, 96]
    # each stream decodes to exactly as many frames as its stripe was
    # encoded in: the mask columns sum to 3, 4 and 3
    encoded = [sum(m[si] for m in DAMAGE_MASKS) for si in range(3)]
    assert encoded == [3, 4, 3]
    for (y0, (chunks, dec)), want in zip(sorted(decoded.items()), encoded):
        assert len(chunks) == len(dec.frames) == want, f"stripe y={y0}"
        # P slices carry the stripe's own frame_num, IDR first
        assert dec.frame_nums() == list(range(want)), f"stripe y={y0}"
        assert [t for t, fm, _ in dec.slices if fm == 0] == \
            [5] + [1] * (want - 1)
    # depth-2 pipelining: byte-identical per frame and stripe
    piped = gpu_encode(w, h, qp, k=n, n=n, dump=False,
                       encode_mask=DAMAGE_MASKS, pipeline_depth=2)
    assert per_frame_bytes(piped) == per_frame_bytes(out)
