"""Inputs, runners and checks shared by the HEVC P-picture host and GPU
tests. Every case is built once (lru_cache) and read-only; the CPU
pipeline's output and its decode are computed once per case and shared."""

import functools
import threading
import time

import numpy as np

import hipflux
from hipflux import _native
import pipeline_content as pc
from hevc_p_ref_decoder import DecoderP

PARAMETER_SET_NALS = {32, 33, 34}


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def static_frames(w=80, h=32, n=3):
    return (pc.uniform_noise(w, h, 3),) * n


@functools.lru_cache(maxsize=None)
def patch_frames(variant):
    """Frame 1 is frame 0 with an 8x8 block changed inside the CTU at
    (col 1, row 1) of an 80x32 picture. "grey" adds the same step to B, G
    and R (the block is first limited to 0..200 in both frames, so nothing
    clips): luma moves, chroma does not. "colour" changes B alone."""
    a = pc.uniform_noise(80, 32, 3)
    if variant == "grey":
        a = a.copy()
        a[20:28, 20:28, :3] = np.minimum(a[20:28, 20:28, :3], 200)
        b = a.copy()
        b[20:28, 20:28, :3] += 48
        _ro(a)
    else:
        b = a.copy()
        blue = b[20:28, 20:28, 0]
        b[20:28, 20:28, 0] = np.where(blue < 128, 255, 0)
    return a, _ro(b)


@functools.lru_cache(maxsize=None)
def half_frames():
    """Left 3 CTU columns unchanged, right 2 replaced by new noise."""
    a = pc.uniform_noise(80, 32, 3)
    b = a.copy()
    b[:, 48:] = pc.uniform_noise(80, 32, 9)[:, 48:]
    return a, _ro(b)


MASK = [[True, True, True], [False, True, False], [True, False, True],
        [True, True, True]]


def encode(kind, frames, w, h, qp=26, stripe_h=32, depth=1, mask=None,
           **kw):
    """(out, dump) of an hevc_inter run of the named pipeline."""
    return _native._pipeline_encode(kind, list(frames), w, h, qp, stripe_h,
                                    2, True, pipeline_depth=depth,
                                    encode_mask=mask, hevc_inter=True, **kw)


def stripe_chain(out, y0):
    """The emissions of the stripe at luma row y0, in frame order:
    [(frame index, bytes, height, is_keyframe)]."""
    return [(i, bytes(d), hh, key) for i, fr in enumerate(out)
            for d, y, hh, key in fr if y == y0]


def decode_chain(out, y0):
    """Decode one stripe's whole chain IDR, P, P... Returns (decoder,
    pictures)."""
    dec = DecoderP()
    pics = dec.decode(b"".join(c[1] for c in stripe_chain(out, y0)))
    return dec, pics


def nal_types(data):
    return [(n[0] >> 1) & 0x3F for n in pc.hrd.split_nals(bytes(data))]


def check_recon(out, dump, stripe_h, stripes=None):
    """The dumped recon planes equal the decoder's last picture of every
    listed stripe's chain (default: all stripes the dump covers; the CPU
    pipeline dumps stripe 0 only, the HIP pipeline the whole frame).
    Returns {y0: decoder}."""
    planes = pc.dump_planes(dump, dump["h"])
    if stripes is None:
        stripes = range(0, dump["h"], stripe_h)
    decs = {}
    for y0 in stripes:
        dec, pics = decode_chain(out, y0)
        pc.assert_planes_equal(planes, y0, pics[-1], f"stripe at {y0}")
        decs[y0] = dec
    return decs


def p_kinds(dec, poc=None):
    """CTU kinds of the P pictures (POC > 0), or of one POC, in order."""
    return [c["kind"] for c in dec.p_ctus
            if (c["poc"] > 0 if poc is None else c["poc"] == poc)]


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    """(out, dump, w, h, stripe_h, kwargs) of the CPU pipeline for a named
    case; the GPU tests compare against these bytes."""
    if name == "static":
        fr, w, h, sh, kw = static_frames(), 80, 32, 32, {}
    elif name in ("patch-grey", "patch-colour"):
        fr, w, h, sh, kw = patch_frames(name[6:]), 80, 32, 32, {}
    elif name in ("half", "half-spr3"):
        fr, w, h, sh, kw = half_frames(), 80, 32, 32, {}
    elif name.startswith("qp"):
        fr, w, h, sh = pc.frames_for(161, 75, 3), 161, 75, 32
        kw = {"qp": int(name[2:])}
    elif name == "mask":
        fr, w, h, sh = pc.frames_for(96, 48, 4), 96, 48, 16
        kw = {"mask": MASK}
    elif name == "idr":
        fr, w, h, sh = pc.frames_for(96, 48, 4), 96, 48, 16
        kw = {"idr_frames": [2]}
    elif name == "wrap":
        fr, w, h, sh, kw = static_frames(16, 16, 260), 16, 16, 16, {}
    else:
        raise KeyError(name)
    with pc.env_vars(HIPFLUX_HEVC_SPR=3 if name == "half-spr3" else None):
        out, dump = encode("cpu", fr, w, h, stripe_h=sh, **kw)
    return out, dump, fr, w, h, sh, kw


def check_recon_per_stripe_cpu(name):
    """Exact recon of every stripe of a CPU case, not stripe 0 alone. The
    CPU pipeline's debug dump holds its first stripe only, and stripes are
    independent streams, so each stripe is encoded again as a picture of
    its own: the case's frames cropped to the stripe's rows (stripe starts
    are even, so 4:2:0 subsampling is the same), and only the frames in
    which the mask codes that stripe. That run's bytes must equal the
    stripe's chain in the full run; its dump is then that stripe's recon
    and must equal the decoder's last picture of the chain. Returns
    {y0: decoder}."""
    out, _, fr, w, h, sh, kw = cpu_case(name)
    mask = kw.get("mask")
    rest = {k: v for k, v in kw.items() if k != "mask"}
    decs = {}
    for si, y0 in enumerate(range(0, h, sh)):
        y1 = min(y0 + sh, h)
        coded = [i for i in range(len(fr)) if mask is None or mask[i][si]]
        # idr_frames are frame indices; they carry over only when the
        # stripe is coded in every frame
        assert "idr_frames" not in rest or len(coded) == len(fr)
        sub = [np.ascontiguousarray(fr[i][y0:y1]) for i in coded]
        with pc.env_vars(HIPFLUX_HEVC_SPR=3 if name == "half-spr3"
                         else None):
            sout, sdump = encode("cpu", sub, w, y1 - y0, stripe_h=sh, **rest)
        chain = stripe_chain(out, y0)
        assert [c[0] for c in chain] == coded, (y0, coded)
        assert [bytes(f[0][0]) for f in sout] == [c[1] for c in chain], \
            f"stripe at {y0}: alone it codes other bytes than in the frame"
        assert [f[0][3] for f in sout] == [c[3] for c in chain]
        dec, pics = decode_chain(out, y0)
        pc.assert_planes_equal(pc.dump_planes(sdump, sdump["h"]), 0,
                               pics[-1], f"stripe at {y0}")
        decs[y0] = dec
    return decs


def gpu_run(name, depth=1, **env):
    """The same case through the HIP pipeline: (out, dump, cpu_out, sh)."""
    cpu_out, _, fr, w, h, sh, kw = cpu_case(name)
    if name == "half-spr3":
        env["HIPFLUX_HEVC_SPR"] = 3
    env.setdefault("HIPFLUX_HEVC_SPR", None)
    with pc.env_vars(**env):
        out, dump = encode("gpu", fr, w, h, stripe_h=sh, depth=depth, **kw)
    return out, dump, cpu_out, sh


# ---- engine ------------------------------------------------------------------

class _Collector:
    def __init__(self):
        self.keys = []
        self.lock = threading.Lock()

    def __call__(self, data, frame_id, y, width, height, is_keyframe,
                 capture_ts_ms, encode_done_ms, stripe_type):
        with self.lock:
            self.keys.append((frame_id, bool(is_keyframe), bytes(data)))

    def wait(self, pred, what):
        """Poll until pred(keys) holds; the engine delivers on its own
        thread. Ends as soon as the stripes are there."""
        deadline = time.monotonic() + 10
        while time.monotonic() < deadline:
            with self.lock:
                if pred(self.keys):
                    return
            time.sleep(0.005)
        raise AssertionError(f"timed out waiting for {what}")


def engine_delta_then_key(use_cpu, pipeline):
    """ScreenCapture on the synthetic backend with hevc_inter: non-key
    stripes appear, request_idr_frame() brings key stripes back, and a
    stripe carries parameter sets exactly when it is a key stripe."""
    s = hipflux.CaptureSettings()
    s.capture_width, s.capture_height = 320, 160
    s.target_fps = 60
    s.output_mode = 2
    s.use_cpu = use_cpu
    s.gpu_id = -1 if use_cpu else 0
    s.capture_backend = "synthetic:noise"
    s.stripe_height = 64
    s.video_crf = 30
    s.hevc_inter = True
    col = _Collector()
    cap = hipflux.ScreenCapture()
    cap.start_capture(col, s)
    try:
        col.wait(lambda k: any(not key for _, key, _ in k), "a delta stripe")
        with col.lock:
            n = len(col.keys)
            assert col.keys[0][1]            # the first emission is a key
        cap.request_idr_frame()
        col.wait(lambda k: any(key for _, key, _ in k[n:]),
                 "a key stripe after request_idr_frame")
    finally:
        cap.stop_capture()
    assert cap.pipeline == pipeline
    for _, key, data in col.keys:
        assert data[0] == 0x06 and data[1] == (1 if key else 0)
        has_ps = bool(set(nal_types(data[10:])) & PARAMETER_SET_NALS)
        assert has_ps == key
