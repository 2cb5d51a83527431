"""Guards for the shared H.264 test content (tests/h264_content.py) and
the per-frame stripe mask of the _pipeline_encode test hook. No GPU.

The GPU reconstruction tests rely on mixed_frames() reaching every MB
mode and every deblocking strength inside P slices; this file asserts
that on the CPU pipeline (which shares the mode-decision rules), so the
generator's coverage cannot rot unseen. It also checks the shape of the
recorded P-stream fixture those tests compare against."""

import json
import os
import re

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from hipflux import _native
from h264_content import CountingDecoder, mixed_frames
from h264_ref_decoder import Decoder


def stripe_streams(out):
    rows = {}
    for frame in out:
        for data, y, hgt, key in frame:
            rows[y] = rows.get(y, b"") + bytes(data)
    return rows


@pytest.mark.parametrize("w,h", [(256, 96), (250, 90)])
def test_mixed_frames_cover_all_modes_and_bs(w, h):
    """Measured on the CPU pipeline at qp 24 (skip / inter / intra-in-P,
    bS 0..4): 256x96 -> 104 / 73 / 111, 6106 45 2513 8280 2736;
    250x90 -> 87 / 94 / 107, 5780 111 2993 8120 2676."""
    n = 4
    frames = mixed_frames(w, h, n)
    out = _native._pipeline_encode("cpu", frames, w, h, qp=24, stripe_h=48,
                                   output_mode=1)
    skip = inter = intra_p = 0
    bs = {k: 0 for k in range(5)}
    for y0, stream in sorted(stripe_streams(out).items()):
        d = CountingDecoder()
        assert len(d.decode(stream)) == n
        skip += d.skip
        inter += d.inter
        intra_p += d.intra_in_p
        for k in bs:
            bs[k] += d.bs[k]
    print(f"{w}x{h}: skip={skip} inter={inter} intra_in_p={intra_p} bs={bs}")
    assert skip >= 50, skip
    assert inter >= 50, inter
    assert intra_p >= 50, intra_p
    for k in range(5):
        assert bs[k] >= 10, f"bS {k} occurs {bs[k]} times: {bs}"


def test_counting_decoder_matches_plain_decoder():
    """The instrumentation must not change what is decoded, and the
    uncropped planes contain the cropped frame."""
    w, h, n = 250, 90, 3
    out = _native._pipeline_encode("cpu", mixed_frames(w, h, n), w, h,
                                   qp=24, stripe_h=48, output_mode=1)
    for y0, stream in stripe_streams(out).items():
        plain = Decoder().decode(stream)
        d = CountingDecoder()
        counted = d.decode(stream)
        assert len(plain) == len(counted) == len(d.uncropped) == n
        for fp, fc, fu in zip(plain, counted, d.uncropped):
            for a, b, u in zip(fp, fc, fu):
                assert np.array_equal(a, b)
                assert u.shape[0] % 8 == 0 and u.shape[1] % 8 == 0
                assert np.array_equal(u[:a.shape[0], :a.shape[1]], a)
        assert np.array_equal(d.y.astype(np.uint8), d.uncropped[-1][0])
        assert d.frame_nums() == list(range(n))
        assert d.bs[0] + d.bs[1] + d.bs[2] + d.bs[3] + d.bs[4] > 0
        assert d.db_changed > 0      # the filter does real work at qp 24
    import h264_ref_decoder
    assert h264_ref_decoder._db_bs.__name__ == "_db_bs"
    assert h264_ref_decoder.deblock_segment_py.__name__ == \
        "deblock_segment_py"


def test_encode_mask_gates_stripes():
    """encode_mask[frame][stripe] drives StripeJob.encode: a masked-out
    stripe emits nothing that frame, its stream decodes to exactly the
    frames it was encoded in with consecutive frame_num, and an
    all-false frame is legal."""
    w, h, n = 128, 96, 5
    frames = mixed_frames(w, h, n)
    mask = [[True, True], [True, False], [False, False], [False, True],
            [True, True]]
    out = _native._pipeline_encode("cpu", frames, w, h, 28, 48, 1,
                                   encode_mask=mask)
    assert len(out) == n
    for fi, fr in enumerate(out):
        assert sorted(y for _, y, _, _ in fr) == \
            [y for y, m in zip((0, 48), mask[fi]) if m]
    for si, (y0, stream) in enumerate(sorted(stripe_streams(out).items())):
        d = CountingDecoder()
        want = sum(m[si] for m in mask)
        assert len(d.decode(stream)) == want
        assert d.frame_nums() == list(range(want))
    # None keeps the default: every stripe, every frame
    full = _native._pipeline_encode("cpu", frames, w, h, 28, 48, 1,
                                    encode_mask=None)
    ones = _native._pipeline_encode("cpu", frames, w, h, 28, 48, 1,
                                    encode_mask=[[True, True]] * n)
    plain = _native._pipeline_encode("cpu", frames, w, h, 28, 48, 1)
    for a, b, c in zip(full, ones, plain):
        key = lambda fr: sorted((y, bytes(d)) for d, y, _, _ in fr)
        assert key(a) == key(b) == key(c)


def test_p_stream_fixture_shape():
    """tests/golden/h264_p_streams.json, which pins the GPU row kernel's
    P streams (test_gpu_p_streams_match_fixture): the four cases, four
    frames each, the stripes 0 and 48, a SHA-256 and a length per stream."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "golden", "h264_p_streams.json")
    with open(path) as f:
        doc = json.load(f)
    n = 4
    assert doc["content"] == "mixed_frames" and doc["frames"] == n
    assert doc["stripe_height"] == 48 and doc["pipeline_depth"] == 1
    note = doc["recorded_from"]
    assert "2-wave kernel" in note and "mixed_frames" in note
    assert sorted((c["w"], c["h"], c["qp"]) for c in doc["cases"]) == \
        [(250, 90, 24), (250, 90, 38), (256, 96, 24), (256, 96, 38)]
    for c in doc["cases"]:
        assert len(c["streams"]) == n
        for frame in c["streams"]:
            assert sorted(frame) == ["0", "48"]
            for rec in frame.values():
                assert re.fullmatch(r"[0-9a-f]{64}", rec["sha256"])
                assert isinstance(rec["length"], int) and rec["length"] > 0


@pytest.mark.parametrize("bad", [
    [[True, True]] * 2,                  # one entry per frame required
    [[True]] * 3,                        # one bool per stripe required
    [[True, True, True]] * 3,
    [[True, True], [True, True], None],  # entries must be lists
    "yes",                               # not a list at all
])
def test_encode_mask_rejects_malformed(bad):
    w, h = 128, 96
    frames = mixed_frames(w, h, 3)
    with pytest.raises((ValueError, RuntimeError)):
        _native._pipeline_encode("cpu", frames, w, h, 28, 48, 1,
                                 encode_mask=bad)
