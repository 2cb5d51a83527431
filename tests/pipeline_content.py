"""Inputs and helpers shared by the encode-pipeline tests: one copy of each
picture generator, the environment-knob context manager, and the HEVC
4:2:0 stream/recon comparison used by the host and the GPU recon tests.

Every generator is cached per argument tuple and returns read-only arrays,
so tests share one instance and cannot change it."""

import contextlib
import functools
import os

import numpy as np

import hevc_ref_decoder as hrd


@contextlib.contextmanager
def env_vars(**kv):
    """Set environment knobs around a pipeline construction (they are
    read when the pipeline is built) and restore them afterwards. A value
    of None unsets the variable for the duration."""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def frames_for(w, h, n, seed=42):
    """Gradient + noise band + a moving saturated box + 1-pixel
    alternating-chroma columns; built once per shape, never modified."""
    rng = np.random.default_rng(seed)
    base = np.zeros((h, w, 4), np.uint8)
    base[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    base[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    base[:, :, 2] = 80
    base[:, :, 3] = 255
    band = max(1, min(16, h // 4))
    base[h // 2:h // 2 + band, :, :3] = rng.integers(
        0, 256, (band, w, 3), dtype=np.uint8)
    c0 = w // 2
    n_alt = min(24, w - c0)
    odd = np.arange(n_alt) & 1
    base[:, c0:c0 + n_alt, 0] = np.where(odd, 255, 0)[None, :]
    base[:, c0:c0 + n_alt, 2] = np.where(odd, 0, 255)[None, :]
    out = []
    for i in range(n):
        f = base.copy()
        if w > 64 and h > 48:
            x = (16 + i * 24) % (w - 48)
            f[16:48, x:x + 48, 0] = 255
            f[16:48, x:x + 48, 2] = 0
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def uniform_noise(w, h, seed):
    """BGRX uniform noise, alpha included."""
    f = np.random.default_rng(seed).integers(0, 256, (h, w, 4),
                                             dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def checkerboard(w, h):
    """1-pixel 0/255 checkerboard in all three colour channels."""
    on = ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1).astype(bool)
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, :3] = np.where(on, 255, 0)[:, :, None]
    f[:, :, 3] = 255
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def colour_checker(w, h):
    """Saturated blue/yellow checker of 2x2 cells: each cell is one chroma
    sample, so the alternation survives 4:2:0 subsampling."""
    on = (((np.arange(h)[:, None] >> 1) + (np.arange(w)[None, :] >> 1))
          & 1).astype(bool)
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, 0] = np.where(on, 255, 0)      # B
    f[:, :, 1] = np.where(on, 0, 255)      # G
    f[:, :, 2] = np.where(on, 0, 255)      # R
    f[:, :, 3] = 255
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def flat_and_mix(w, h, noise_rows=16, seed=7, level=91):
    """(flat, mix): a frame of one grey level, and the same with its first
    `noise_rows` rows replaced by uniform noise."""
    flat = np.full((h, w, 4), level, np.uint8)
    mix = flat.copy()
    mix[:noise_rows] = np.random.default_rng(seed).integers(
        0, 256, (noise_rows, w, 4), dtype=np.uint8)
    flat.setflags(write=False)
    mix.setflags(write=False)
    return flat, mix


# ---- HEVC 4:2:0 streams ------------------------------------------------------

def per_frame(out):
    """_pipeline_encode output -> [[(y0, bytes) per stripe] per frame]"""
    return [[(y, bytes(d)) for d, y, hh, key in fr] for fr in out]


def idr_nals(data):
    """The IDR slice NALs (type 19) of an Annex-B stream, without start
    codes and emulation prevention."""
    return [n for n in hrd.split_nals(bytes(data))
            if (n[0] >> 1) & 0x3F == 19]


def spec_chroma_qp(qp):
    """Table 8-10 (ChromaArrayType 1, offsets 0), written out entry by
    entry rather than as the decoder's three-branch function."""
    table = {30: 29, 31: 30, 32: 31, 33: 32, 34: 33, 35: 33, 36: 34, 37: 34,
             38: 35, 39: 35, 40: 36, 41: 36, 42: 37, 43: 37}
    if qp < 30:
        return qp
    return table[qp] if qp in table else qp - 6


def decode_stripe(data, w, vis_h, qpc_override=None):
    """Decode one stripe's stream (own parameter sets, one IDR picture)
    with the from-spec decoder. Returns (decoder, (y, cb, cr)); asserts
    the 4:2:0 shape rule: the visible size rounded up to even."""
    dec = hrd.Decoder(qpc_override=qpc_override)
    frames = dec.decode(data)
    assert len(frames) == 1
    ew, eh = (w + 1) & ~1, (vis_h + 1) & ~1
    y, cb, cr = frames[0]
    assert y.shape == (eh, ew), (y.shape, (eh, ew))
    assert cb.shape == cr.shape == (eh // 2, ew // 2)
    return dec, frames[0]


def assert_planes_equal(planes, y0, decoded, what):
    """planes: three 2-D recon arrays (Y full size, chroma half size) that
    hold the stripe at luma row y0; decoded: the decoder's (y, cb, cr).
    Exact equality over the decoder's output shape."""
    for name, plane, want, r0 in zip(("y", "cb", "cr"), planes, decoded,
                                     (y0, y0 // 2, y0 // 2)):
        hh, ww = want.shape
        got = plane[r0:r0 + hh, :ww]
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(
                f"{what}: plane {name} differs from the decoder at "
                f"{len(bad)} samples, first (row, col) = {tuple(bad[0])}: "
                f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def dump_planes(dump, h):
    """The three recon planes of a 4:2:0 debug dump as 2-D arrays."""
    yh = (h + 15) & ~15
    return (np.frombuffer(dump["y"], np.uint8).reshape(yh, dump["ypitch"]),
            np.frombuffer(dump["cb"], np.uint8).reshape(yh // 2,
                                                        dump["cpitch"]),
            np.frombuffer(dump["cr"], np.uint8).reshape(yh // 2,
                                                        dump["cpitch"]))


def coverage(decoders):
    """(modes, [cbf_y values, cbf_cb values, cbf_cr values]) over the CTUs
    the given decoders recorded."""
    modes, cbfs = set(), [set(), set(), set()]
    for dec in decoders:
        modes |= {c[0] for c in dec.ctus}
        for i in range(3):
            cbfs[i] |= {c[1 + i] for c in dec.ctus}
    return modes, cbfs


def assert_full_coverage(decoders, what):
    modes, cbfs = coverage(decoders)
    assert modes == {0, 1, 10, 26}, f"{what}: modes chosen {sorted(modes)}"
    for name, s in zip(("cbf_luma", "cbf_cb", "cbf_cr"), cbfs):
        assert s == {0, 1}, f"{what}: {name} takes only {sorted(s)}"
