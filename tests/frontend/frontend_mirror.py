"""numpy mirrors of the capture front end's documented integer math, and
the small inputs its tests share. Nothing here calls the native module."""

import numpy as np

MARGIN = 16


def padded(frame, pad=12):
    """(h, w, 4) uint8 -> (flat buffer with `pad` extra bytes per row,
    stride). The pad bytes are noise: nothing may read them."""
    h, w, _ = frame.shape
    stride = w * 4 + pad
    rng = np.random.default_rng(w * 1000 + h)
    buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w * 4] = frame.reshape(h, w * 4)
    return np.ascontiguousarray(buf).reshape(-1), stride


def watermark_origin(location, fw, fh, w, h, frame_idx):
    if location == 1:
        return MARGIN, MARGIN
    if location == 2:
        return fw - w - MARGIN, MARGIN
    if location == 3:
        return MARGIN, fh - h - MARGIN
    if location == 4:
        return fw - w - MARGIN, fh - h - MARGIN
    if location == 5:
        # C++ integer division truncates toward zero
        return int((fw - w) / 2), int((fh - h) / 2)
    if location == 6:
        sx, sy = max(1, fw - w), max(1, fh - h)
        x0 = (frame_idx * 3) % (2 * sx)
        y0 = (frame_idx * 2) % (2 * sy)
        if x0 >= sx:
            x0 = 2 * sx - x0 - 1
        if y0 >= sy:
            y0 = 2 * sy - y0 - 1
        return x0, y0
    return None


def _clip(x0, y0, w, h, fw, fh):
    ax, ay = max(0, x0), max(0, y0)
    bx, by = min(fw, x0 + w), min(fh, y0 + h)
    if bx <= ax or by <= ay:
        return None
    return ax, ay, bx, by


def blend_watermark(frame, wm, location, frame_idx):
    """frame (h, w, 4) uint8, wm (wh, ww, 4) straight-alpha BGRA."""
    out = frame.copy()
    fh, fw, _ = frame.shape
    wh, ww, _ = wm.shape
    org = watermark_origin(location, fw, fh, ww, wh, frame_idx)
    if org is None:
        return out
    x0, y0 = org
    r = _clip(x0, y0, ww, wh, fw, fh)
    if r is None:
        return out
    ax, ay, bx, by = r
    s = wm[ay - y0:by - y0, ax - x0:bx - x0].astype(np.int64)
    d = out[ay:by, ax:bx].astype(np.int64)
    a = s[..., 3:4]
    v = (s[..., :3] * a + d[..., :3] * (255 - a) + 127) // 255
    d[..., :3] = np.where(a > 0, v, d[..., :3])
    out[ay:by, ax:bx] = d.astype(np.uint8)
    return out


def blend_cursor(frame, argb, cx, cy):
    """argb (ch, cw) uint32, premultiplied."""
    out = frame.copy()
    fh, fw, _ = frame.shape
    ch, cw = argb.shape
    r = _clip(cx, cy, cw, ch, fw, fh)
    if r is None:
        return out
    ax, ay, bx, by = r
    p = argb[ay - cy:by - cy, ax - cx:bx - cx].astype(np.int64)
    a = (p >> 24)[..., None]
    chans = np.stack([p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF], -1)
    d = out[ay:by, ax:bx].astype(np.int64)
    v = np.clip((chans * 255 + d[..., :3] * (255 - a)) // 255, 0, 255)
    d[..., :3] = np.where(a > 0, v, d[..., :3])
    out[ay:by, ax:bx] = d.astype(np.uint8)
    return out


def bilinear(src, scale):
    """The mirror in tests/test_engine.py, as a function of (h, w, 4)."""
    h, w, _ = src.shape
    ow = max(1, int(np.float32(w) * np.float32(scale) + np.float32(0.5)))
    oh = max(1, int(np.float32(h) * np.float32(scale) + np.float32(0.5)))
    xstep = (w << 16) // ow
    ystep = (h << 16) // oh
    s64 = src.astype(np.int64)
    exp = np.zeros((oh, ow, 4), np.int64)
    xs = ((2 * np.arange(ow) + 1) * xstep - (1 << 16)) // 2
    xs = np.clip(xs, 0, None)
    xi = np.minimum(xs >> 16, w - 2)
    fx = (xs >> 8) & 0xFF
    for y in range(oh):
        sy = ((2 * y + 1) * ystep - (1 << 16)) // 2
        sy = max(sy, 0)
        iy = min(sy >> 16, h - 2)
        fy = (sy >> 8) & 0xFF
        a = s64[iy, xi]
        b = s64[iy, xi + 1]
        c = s64[iy + 1, xi]
        e = s64[iy + 1, xi + 1]
        top = (a << 8) + (b - a) * fx[:, None]
        bot = (c << 8) + (e - c) * fx[:, None]
        exp[y] = ((top << 8) + (bot - top) * fy + (1 << 15)) >> 16
    return exp.astype(np.uint8)


def box(src, div):
    h, w, _ = src.shape
    ow, oh = w // div, h // div
    s = src[:oh * div, :ow * div].astype(np.int64)
    acc = s.reshape(oh, div, ow, div, 4).sum(axis=(1, 3))
    n = div * div
    return ((acc + n // 2) // n).astype(np.uint8)


def block_flags(cur, prev, threshold, block=16):
    """(h, w, 4) frames -> (by, bx) uint8: 1 where any byte of the block
    differs by more than threshold (threshold <= 0: differs at all)."""
    h, w, _ = cur.shape
    bx, by = (w + block - 1) // block, (h + block - 1) // block
    d = np.abs(cur.astype(np.int64) - prev.astype(np.int64)).max(axis=2)
    hit = d > max(threshold, 0)
    flags = np.zeros((by, bx), np.uint8)
    for j in range(by):
        for i in range(bx):
            flags[j, i] = hit[j * block:(j + 1) * block,
                              i * block:(i + 1) * block].any()
    return flags


def make_cursor(rng, cw=12, ch=16):
    """Premultiplied-ARGB cursor whose alphas cycle through the edge
    values and whose colour channels mostly EXCEED alpha, so that the
    blend overflows 255 and clip8u has to clip."""
    alphas = np.array([0, 1, 128, 254, 255], np.uint32)
    a = alphas[np.arange(cw * ch) % 5].reshape(ch, cw)
    bgr = rng.integers(0, 256, (ch, cw, 3)).astype(np.uint32)
    bgr[::2] = np.maximum(bgr[::2], 200)
    return (a << 24) | (bgr[..., 2] << 16) | (bgr[..., 1] << 8) | bgr[..., 0]


def make_watermark(rng, ww, wh):
    wm = rng.integers(0, 256, (wh, ww, 4), dtype=np.uint8)
    alphas = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    wm[..., 3] = alphas[np.arange(ww * wh) % 6].reshape(wh, ww)
    return wm
