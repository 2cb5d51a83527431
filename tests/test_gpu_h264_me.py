"""The H.264 GPU motion search and mode decision (k_h264_me_mfma with
the k_downsample2 pyramid) pinned to tests/h264_me_mirror.py on a real
MI355X. Every comparison is integer-exact and no MB is left out.

For each case one GPU run is decoded stripe by stripe; the mirror is then
run frame by frame with the decoder's uncropped planes of frame k-1 as the
reference of frame k (what the GPU holds, by the recon tests), and for
every MB of every frame the coded mode and vector must be the mirror's.
After the last frame the dumped state words must equal the mirror's under
the mask the search owns.

Content is h264_content.me_frames; tests/test_h264_me_mirror_host.py
guards, without a GPU, that it reaches every search pass."""

import contextlib
import functools
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
import h264_me_mirror as mm
from h264_content import (RecordingDecoder, bgrx_to_planes, me_frames, tex,
                          tie_frames)
from h264_me_mirror import INTER, INTRA, MeMirror

STRIPE_H = 48
DAMAGE_MASKS = [[True, True, True], [True, False, True],
                [False, True, False], [True, True, False],
                [False, False, False], [False, True, True]]


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


# ---- content ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def content(kind, w, h, n):
    """Frames built once per (kind, size) and never modified."""
    if kind == "me":
        frames = me_frames(w, h, n)
    elif kind == "tie":
        frames = tie_frames(w, h, n)
    elif kind == "drift":
        # a picture smaller than any band: one texture moving (3, -1) px
        # per frame, so that every MB's search is clipped by the picture
        t = tex(np.random.default_rng(21), h + 32, w + 32)
        frames = []
        for i in range(n):
            f = np.full((h, w, 4), 255, np.uint8)
            f[:, :, :3] = t[16 - i:16 - i + h, 16 + 3 * i:16 + 3 * i + w]
            frames.append(np.ascontiguousarray(f))
    else:
        rng = np.random.default_rng(22)
        frames = []
        for i in range(n):
            f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            f[:, :, 3] = 255
            frames.append(np.ascontiguousarray(f))
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def source_planes(kind, w, h, n):
    return tuple(bgrx_to_planes(f) for f in content(kind, w, h, n))


# ---- one pinned run ---------------------------------------------------------

def gpu_encode(kind, w, h, n, qp, k=None, dump=True, fullcolor=False,
               masks=None, **kw):
    k = n if k is None else k
    frames = list(content(kind, w, h, n)[:k])
    if masks is not None:
        kw["encode_mask"] = [list(m) for m in masks[:k]]
    return _native._pipeline_encode("gpu", frames, w, h, qp, STRIPE_H, 1,
                                    dump, fullcolor=fullcolor, **kw)


def per_frame_bytes(out):
    return [sorted((y, bytes(d)) for d, y, hgt, key in fr) for fr in out]


def dumped_words(dump, w, h, planes):
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    meta = np.frombuffer(dump["meta"], np.int32)
    assert meta.size == planes * mbh * mbw * 2
    return meta.reshape(planes, mbh, mbw, 2)


class Pinned:
    """A GPU run, its decode and the mirror's walk over it."""

    def __init__(self, kind, w, h, n, qp, fullcolor=False, masks=None):
        self.args = (kind, w, h, n, qp)
        self.fullcolor, self.masks = fullcolor, masks
        self.planes = 3 if fullcolor else 1
        t0 = time.time()
        self.out, self.dump = gpu_encode(kind, w, h, n, qp,
                                         fullcolor=fullcolor, masks=masks)
        t1 = time.time()
        assert len(self.out) == n
        self.decode(w, h)
        t2 = time.time()
        self.walk(kind, w, h, n, qp)
        t3 = time.time()
        self.coverage = {}
        for m in self.mirrors:
            for key, v in m.coverage().items():
                self.coverage[key] = self.coverage.get(key, 0) + v
        print(f"{kind} {w}x{h} n={n} qp={qp} fullcolor={fullcolor}: "
              f"gpu {t1 - t0:.2f}s decode {t2 - t1:.2f}s mirror "
              f"{t3 - t2:.2f}s; recoded={self.recoded} {self.coverage}")

    def decode(self, w, h):
        """Per stripe: the decoder, and which frames it was encoded in."""
        chunks, self.encoded_in = {}, {}
        for fi, fr in enumerate(self.out):
            for data, y0, hgt, key in fr:
                chunks.setdefault(y0, []).append(bytes(data))
                self.encoded_in.setdefault(y0, []).append(fi)
        assert chunks, "nothing was encoded"
        self.decs = {}
        for y0, ch in sorted(chunks.items()):
            dec = RecordingDecoder()
            frames = dec.decode(b"".join(ch))
            assert len(frames) == len(ch), f"stripe y={y0}"
            self.decs[y0] = dec

    def walk(self, kind, w, h, n, qp):
        mbw, mbh = (w + 15) // 16, (h + 15) // 16
        src = source_planes(kind, w, h, n)
        self.mirrors = [MeMirror(w, h, STRIPE_H, qp)
                        for _ in range(self.planes)]
        ref = [np.zeros((mbh * 16, mbw * 16), np.int64)
               for _ in range(self.planes)]
        self.snapshots = []      # state words after each frame
        self.recoded = 0
        bad = []
        for fi in range(n):
            mask = None if self.masks is None else self.masks[fi]
            encoded = [y0 for y0 in sorted(self.decs)
                       if fi in self.encoded_in[y0]]
            if mask is not None:
                assert encoded == [y0 for y0, m in
                                   zip(range(0, h, STRIPE_H), mask) if m]
            for pl, m in enumerate(self.mirrors):
                got = m.encode(src[fi][pl], ref[pl], idr=(fi == 0),
                               mask=mask)
                seen = 0
                for y0 in encoded:
                    dec = self.decs[y0]
                    j = self.encoded_in[y0].index(fi)
                    for (p, mbx, mby), coded in dec.mbs[j].items():
                        if p != pl:
                            continue
                        seen += 1
                        key = (mbx, mby + y0 // 16)
                        want = got[key]
                        if (self.fullcolor and want[0] == INTER
                                and coded == (INTRA, (0, 0))):
                            # a monochrome inter MB with a non-zero
                            # residual is re-coded as I16x16; the search
                            # state keeps its hint
                            m.recode_intra(*key)
                            self.recoded += 1
                            continue
                        if coded != want:
                            bad.append((fi, pl, key, coded, want))
                assert seen == len(got), \
                    f"frame {fi} plane {pl}: {seen} MBs coded, " \
                    f"mirror decided {len(got)}"
            for y0 in encoded:
                dec = self.decs[y0]
                j = self.encoded_in[y0].index(fi)
                planes = dec.uncropped[j]
                for pl in range(self.planes):
                    p = planes[pl]
                    ref[pl][y0:y0 + p.shape[0]] = p
            self.snapshots.append(np.stack([m.words()
                                            for m in self.mirrors]))
        self.bad = bad

    def assert_decisions(self):
        assert not self.bad, (
            f"{len(self.bad)} MBs differ from the mirror; first "
            f"(frame, plane, (mbx, mby), coded, mirror): {self.bad[:5]}")

    def assert_state(self, dump=None, after=None):
        """Dumped state words == the mirror's after frame `after`."""
        kind, w, h, n, qp = self.args
        dump = self.dump if dump is None else dump
        after = n - 1 if after is None else after
        got = dumped_words(dump, w, h, self.planes)
        for pl in range(self.planes):
            diff = mm.masked_equal(got[pl], self.snapshots[after][pl])
            assert not diff, (
                f"plane {pl}: {len(diff)} state words differ after frame "
                f"{after}; first (mby, mbx, word): {diff[:5]}; GPU "
                f"{[hex(int(got[pl][a, b, c]) & 0xFFFFFFFF) for a, b, c in diff[:5]]}"
                f" mirror "
                f"{[hex(int(self.snapshots[after][pl][a, b, c]) & 0xFFFFFFFF) for a, b, c in diff[:5]]}")

    def assert_coverage(self, keys):
        for key in keys:
            assert self.coverage[key] >= 1, (key, self.coverage)


@functools.lru_cache(maxsize=None)
def pinned(kind, w, h, n, qp, fullcolor=False, masks=None):
    return Pinned(kind, w, h, n, qp, fullcolor, masks)


EVERYTHING = ("pass1", "pass2", "pass3", "hopeless", "probes", "odd",
              "half", "quarter")


# ---- cases ------------------------------------------------------------------

@pytest.mark.parametrize("qp", [17, 30, 45])
def test_gpu_me_base(qp):
    """256x96, two 48-row stripes, 10 frames so that frame_num 8 (the
    hopeless probe) occurs. qp moves the skip / inter thresholds from
    192 / 1152 (qp 17) to 6144 / 36864 (qp 45). Every pass, hopeless
    MBs, a probe and every vector kind must occur at qp 30 with the real
    reference. At qp 45 nothing can be hopeless: fresh noise against
    noise has a SAD near 256 * 85 (mean |a - b| of independent bytes),
    under the inter threshold, so those MBs go inter."""
    require_gpu()
    run = pinned("me", 256, 96, 10, qp)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage({30: EVERYTHING,
                         17: ("pass1", "pass2", "pass3", "hopeless",
                              "probes"),
                         45: ("pass1", "pass2", "pass3")}[qp])


@pytest.mark.parametrize("k", [2, 9])
def test_gpu_me_hidden_state(k):
    """The state words are hidden behind the last frame's dump, so they
    are checked after 2 and after 9 frames by prefix runs: the prefix
    streams are byte-identical to the full run's, whose decode drove the
    mirror."""
    require_gpu()
    run = pinned("me", 256, 96, 10, 30)
    run.assert_decisions()
    out, dump = gpu_encode("me", 256, 96, 10, 30, k=k)
    assert per_frame_bytes(out) == per_frame_bytes(run.out)[:k]
    run.assert_state(dump, after=k - 1)


def test_gpu_me_unaligned():
    """250x90: the last MB column and row are partly padding. The scroll
    band reaches the right edge, so pyramid acquisitions happen in the
    last MB column, whose proxy must be a function of the picture alone."""
    require_gpu()
    run = pinned("me", 250, 90, 10, 30)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage(EVERYTHING + ("pass3_last_col",))


def test_gpu_me_tie_order():
    """h264_content.tie_frames at qp 17: exact ties between (-8, 0) and
    (8, 0) in the zero grid, and between many quarter-resolution positions
    in the pyramid. The first vector in visiting order, and the smallest
    (my, mx), must win; both kinds of tie must occur with the real
    reference."""
    require_gpu()
    run = pinned("tie", 256, 96, 3, 17)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage(("grid_ties", "pyramid_ties"))


def test_gpu_me_small():
    """36x20, one stripe of 3x2 MBs: every grid is clipped by the picture
    on at least two sides."""
    require_gpu()
    run = pinned("drift", 36, 20, 4, 30)
    run.assert_decisions()
    run.assert_state()


def test_gpu_me_segments():
    """HIPFLUX_SEGS=3: three slices per MB row; the search maps blocks to
    MBs through mbx0 and seg_mbw."""
    require_gpu()
    with env_vars(HIPFLUX_SEGS=3):
        run = Pinned("me", 256, 96, 4, 30)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage(("pass1", "pass2", "pass3", "hopeless"))


def test_gpu_me_wide():
    """2064x16: 129 MBs, two segments per row (128 + 1), seg_max 128."""
    require_gpu()
    run = pinned("me", 2064, 16, 3, 30)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage(("pass1", "pass3"))


def test_gpu_me_damage_mask():
    """256x144, three stripes, six frames, some stripes not encoded: the
    state of a stripe that is not encoded must not change (stripe 0 sits
    out the last two frames and is compared in the final dump) and must
    steer that stripe's next encoded frame (every frame is compared)."""
    require_gpu()
    masks = tuple(tuple(m) for m in DAMAGE_MASKS)
    run = pinned("me", 256, 144, 6, 30, masks=masks)
    run.assert_decisions()
    run.assert_state()
    assert [len(run.encoded_in[y]) for y in (0, 48, 96)] == [3, 4, 3]
    # stripe 0's rows: unchanged since frame 3
    assert np.array_equal(run.snapshots[5][:, :3], run.snapshots[3][:, :3])
    run.assert_coverage(("pass1", "pass3"))


def test_gpu_me_depth2_bytes_equal_depth1():
    """pipeline_depth=2 double-buffers the state words; its streams must
    equal depth 1's, which the mirror has pinned."""
    require_gpu()
    run = pinned("me", 256, 96, 10, 30)
    run.assert_decisions()
    piped = gpu_encode("me", 256, 96, 10, 30, dump=False, pipeline_depth=2)
    assert per_frame_bytes(piped) == per_frame_bytes(run.out)


def test_gpu_me_fullcolor():
    """fullcolor: the same kernel runs once per colour plane, each with
    its own source, reference, pyramids and state (plane-major meta). The
    only decision the mirror cannot make is the row kernel's: an inter MB
    whose quantised residual is non-zero is re-coded intra; its search
    state must still be the mirror's."""
    require_gpu()
    run = pinned("me", 256, 96, 4, 30, fullcolor=True)
    run.assert_decisions()
    run.assert_state()
    run.assert_coverage(("pass1", "pass2", "pass3", "hopeless"))


def test_gpu_me_tiny():
    """20x3 noise: fewer than 4 rows. The pyramid's only row is built
    from clamped reads, and the proxy row clamp has a floor of 0."""
    require_gpu()
    run = pinned("noise", 20, 3, 3, 30)
    run.assert_decisions()
    run.assert_state()
