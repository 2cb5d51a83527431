"""H.264 fullcolor (Hi444 separate colour planes) through the persistent
pipeline handle, on the CPU pipeline: BenchPipeline takes a trailing
`fullcolor` keyword, and what it emits decodes as profile 244 with three
full-resolution planes. The SPS-444 bytes themselves are pinned by
tests/test_h264.py."""

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_ref_decoder import Decoder


def test_bench_pipeline_fullcolor_keyword_cpu():
    w, h = 120, 52
    bp = _native.BenchPipeline("cpu", w, h, 26, 64, 1, -1, 1, fullcolor=True)
    assert bp.pipeline == "cpu-h264"
    bp.keep_stripes = True
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    nbytes, stripes = bp.encode(frame, True)
    assert stripes == 1 and nbytes > 0
    frame_id, kept = bp.kept_stripes()
    assert frame_id == 0 and len(kept) == 1
    y0, payload = kept[0]
    assert y0 == 0 and len(payload) == nbytes
    dec = Decoder()
    frames = dec.decode(bytes(payload))
    assert dec.sps["profile_idc"] == 244 and dec.sps["separate"]
    assert len(frames) == 1
    assert [p.shape for p in frames[0]] == [(h, w)] * 3


def test_bench_pipeline_fullcolor_defaults_off():
    """Without the keyword the handle codes 4:2:0 as before."""
    w, h = 64, 32
    bp = _native.BenchPipeline("cpu", w, h, 26, 64, 1, -1, 1)
    bp.keep_stripes = True
    bp.encode(np.full((h, w, 4), 90, np.uint8), True)
    dec = Decoder()
    y, cb, cr = dec.decode(bytes(bp.kept_stripes()[1][0][1]))[0]
    assert dec.sps["profile_idc"] == 66
    assert (y.shape, cb.shape) == ((h, w), (h // 2, w // 2))
