"""Slice plan of the HIP H.264 pipeline (native/cpu/h264/seg_plan.h): how
each MB row is cut into slices. Pure arithmetic, checked without a GPU
through the _h264_seg_plan binding."""

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
from hipflux import _native

K_MAX_SEG_MBW = 128   # h264gpu::kMaxSegMbw


def widths(mbw, mbh, override=0):
    """Slice widths of one MB row, cut the way the pipeline's job loop
    cuts them: `segs` slices of min(widest, what is left)."""
    segs, widest = (int(v) for v in _native._h264_seg_plan(mbw, mbh,
                                                           override))
    out, x = [], 0
    for _ in range(segs):
        out.append(min(widest, mbw - x))
        x += out[-1]
    return out


@pytest.mark.parametrize("mbw,mbh,want", [
    (120, 68, [40] * 3),      # 1080p
    (240, 135, [30] * 8),     # 4K
    (480, 270, [60] * 8),     # 8K
])
def test_default_plan_of_the_measured_resolutions(mbw, mbh, want):
    assert widths(mbw, mbh) == want


def test_overrides_at_16_mbs():
    assert widths(16, 6, 3) == [6, 6, 4]
    assert widths(16, 6, 16) == [1] * 16
    # 5 slices of ceil(16 / 5) = 4 would leave the fifth empty
    assert widths(16, 6, 5) == [4] * 4
    # above mbw: one MB per slice
    assert widths(16, 6, 40) == [1] * 16


def test_every_plan_tiles_the_row():
    """mbw 1..1024 x mbh 1..599 x override {none, 1..40}: widths are all
    >= 1 and <= kMaxSegMbw, sum to mbw, and there are `segs` of them.
    The pipeline cuts segs slices of min(widest, rest), so the widths are
    (widest,) * (segs - 1) + (last,) with last = mbw - (segs-1)*widest:
    they sum to mbw by construction and are all valid iff 1 <= last <=
    widest — anything else is a zero-width (or negative) trailing slice."""
    mbw = np.arange(1, 1025, dtype=np.int32)[:, None]
    mbh = np.arange(1, 600, dtype=np.int32)[None, :]
    for override in range(0, 41):
        segs, widest = _native._h264_seg_plan(mbw, mbh, override)
        assert segs.shape == widest.shape == (1024, 599)
        last = mbw - (segs - 1) * widest
        assert (segs >= 1).all(), override
        assert (widest >= 1).all() and (widest <= K_MAX_SEG_MBW).all(), \
            override
        assert (last >= 1).all() and (last <= widest).all(), override
        assert ((segs - 1) * widest + last == mbw).all(), override
    # the vectorised model above is the job loop's cut: spot-check it
    for args in [(1, 1, 0), (129, 9, 0), (1024, 599, 7), (16, 6, 9),
                 (250, 90, 33)]:
        w = widths(*args)
        segs, widest = (int(v) for v in _native._h264_seg_plan(*args))
        assert len(w) == segs and sum(w) == args[0]
        assert min(w) >= 1 and max(w) == widest <= K_MAX_SEG_MBW
