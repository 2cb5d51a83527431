"""Host side of the three HIP pipelines (JPEG, H.264, HEVC) on a real
MI355X: frame pipelining, re-allocation on a resolution change, frame
upload from buffers whose addresses get reused, and the H.264 segment
plan override. Every comparison is byte equality of emitted stripes."""

import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_ref_decoder import Decoder

STRIPE_H = 64
# (id, output_mode, qp / jpeg quality)
CODECS = [("jpeg", 0, 60), ("h264", 1, 26), ("hevc", 2, 26)]


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


def fresh_frame(w, h, seed):
    """A newly allocated BGRX frame: smooth gradients, a seeded box and a
    seeded noise band. Equal arguments give equal pixels in a new array."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    f[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    f[:, :, 2] = 80
    f[:, :, 3] = 255
    f[h // 2:h // 2 + 16] = rng.integers(0, 256, (16, w, 4), dtype=np.uint8)
    x = int(rng.integers(0, w - 48))
    f[16:48, x:x + 48, 0] = 255
    f[16:48, x:x + 48, 2] = 0
    return np.ascontiguousarray(f)


def per_frame_bytes(out):
    return [sorted((y, bytes(d)) for d, y, hgt, key in fr) for fr in out]


# ---- depth 2 against depth 1 ------------------------------------------------

@pytest.mark.parametrize("mode,qp,fullcolor", [
    (0, 60, False), (0, 60, True), (2, 26, False)],
    ids=["jpeg420", "jpeg444", "hevc"])
def test_depth2_byte_identical_to_depth1(mode, qp, fullcolor):
    """One frame in flight (submit N, emit N-1) must not change a byte
    of any frame's stripes. (H.264: test_pipelined_depth2_byte_identical
    in test_gpu_h264.py.)"""
    require_gpu()
    w, h, n = 160, 128, 4
    frames = [fresh_frame(w, h, 100 + i) for i in range(n)]
    runs = [per_frame_bytes(_native._pipeline_encode(
        "gpu", frames, w, h, qp, STRIPE_H, mode, False, fullcolor,
        pipeline_depth=d)) for d in (1, 2)]
    assert len(runs[0]) == len(runs[1]) == n
    for fi in range(n):
        assert len(runs[0][fi]) == h // STRIPE_H, f"frame {fi}: no stripes"
        assert runs[0][fi] == runs[1][fi], f"frame {fi}: depth 2 differs"


# ---- resolution change --------------------------------------------------------

def first_frame_of_fresh_pipeline(mode, qp, w, h, seed):
    p = _native.BenchPipeline("gpu", w, h, qp=qp, stripe_height=STRIPE_H,
                              output_mode=mode, gpu_id=0, pipeline_depth=2)
    p.keep_stripes = True
    p.encode(fresh_frame(w, h, seed), True)
    p.flush()
    fid, stripes = p.kept_stripes()
    assert fid == 0
    return sorted((y, bytes(d)) for y, d in stripes)


# JPEG once more at sizes whose width and height are 8 past a multiple of
# 16: the last MCU column and row then hold luma blocks wholly outside the
# picture, which only stay equal to a fresh pipeline's if every frame
# writes them (a re-allocation hands back memory with old contents)
RESIZES = [c + ([(160, 128), (256, 192), (160, 128)],) for c in CODECS] + [
    ("jpeg-pad8", 0, 60, [(168, 136), (264, 200), (168, 136)])]


@pytest.mark.parametrize("name,mode,qp,sizes", RESIZES,
                         ids=[c[0] for c in RESIZES])
def test_resolution_change_restarts_like_a_fresh_pipeline(name, mode, qp,
                                                          sizes):
    """Depth 2 across 160x128 -> 256x192 -> 160x128, three frames each.
    The frame in flight at a resize references the old buffers and is
    dropped; every other frame emits, in order, and the first frame
    after each resize is byte-equal to what a fresh pipeline makes of it
    (JPEG and HEVC are all-intra; H.264 restarts with an IDR and fresh
    stripe state). Every frame is a newly allocated array that is
    released after its call, so the allocator may hand a later, larger
    frame an address an earlier one was uploaded from."""
    require_gpu()
    p = _native.BenchPipeline("gpu", *sizes[0], qp=qp,
                              stripe_height=STRIPE_H, output_mode=mode,
                              gpu_id=0, pipeline_depth=2)
    p.keep_stripes = True
    emitted = []            # frame ids in emission order
    first_after = {}        # segment -> kept stripes of its first frame
    fid = 0
    for seg, (w, h) in enumerate(sizes):
        if seg:
            p.resize(w, h)
        for i in range(3):
            nbytes, nstripes = p.encode(fresh_frame(w, h, 10 * seg + i),
                                        i == 0)
            if i == 0:
                # nothing to emit: the pipe was empty or just dropped
                assert (nbytes, nstripes) == (0, 0)
                assert p.last_frame_id == -1
            else:
                assert nbytes > 0 and nstripes == -(-h // STRIPE_H)
                emitted.append(p.last_frame_id)
            if i == 1:
                kept_id, stripes = p.kept_stripes()
                assert kept_id == fid - 1
                first_after[seg] = sorted((y, bytes(d)) for y, d in stripes)
            fid += 1
    nbytes, nstripes = p.flush()
    assert nbytes > 0 and nstripes == -(-sizes[-1][1] // STRIPE_H)
    emitted.append(p.last_frame_id)
    assert emitted == [0, 1, 3, 4, 6, 7, 8]
    for seg, (w, h) in enumerate(sizes):
        want = first_frame_of_fresh_pipeline(mode, qp, w, h, 10 * seg)
        assert [y for y, _ in want] == list(range(0, h, STRIPE_H))
        assert first_after[seg] == want, \
            f"{name}: first frame at {w}x{h} (segment {seg}) differs " \
            f"from a fresh pipeline's"


# ---- H.264 segment plan override ----------------------------------------------

def test_h264_segs_override_without_exact_split_is_normalised():
    """16 MBs do not split into 5 slices of ceil(16/5) = 4: the plan
    normalises to 4 slices of 4, so HIPFLUX_SEGS=5 is HIPFLUX_SEGS=4."""
    require_gpu()
    w, h, n = 256, 96, 2
    frames = [fresh_frame(w, h, 200 + i) for i in range(n)]
    outs = {}
    for segs in (4, 5):
        with env_vars(HIPFLUX_SEGS=segs):
            outs[segs] = per_frame_bytes(_native._pipeline_encode(
                "gpu", frames, w, h, 26, STRIPE_H, 1))
    assert outs[5] == outs[4]
    for y0 in (0, 64):
        stream = b"".join(d for fr in outs[5] for y, d in fr if y == y0)
        decoded = Decoder().decode(stream)
        assert len(decoded) == n
        assert decoded[0][0].shape[1] == w
