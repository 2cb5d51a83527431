"""From-spec (ITU-T T.81) helpers that pin the JPEG encoders' coefficients.

Three independent pieces, none derived from the encoder's sources:

  decode_coeffs          baseline JFIF entropy decoder that stops at the
                         quantised coefficients (no IDCT), strict about
                         framing: padding, restart numbering, leftovers
  reference_coeff_real   float64 DCT of one stripe's pixels, divided by the
                         stream's quantisers, UNROUNDED
  check_coeffs           every decoded coefficient must be a correct
                         rounding of the reference value

Block layout everywhere: blocks[my][mx][slot][k], k in natural (row-major
v*8+u) order; slot = Y0 Y1 Y2 Y3 Cb Cr for 4:2:0 (Y sub-block = by*2+bx)
and Y Cb Cr for 4:4:4.
"""

import numpy as np


class JpegError(ValueError):
    """The stream violates baseline T.81 framing or entropy coding."""


def _zigzag():
    """T.81 Figure A.6: zig-zag index -> natural index."""
    order, x, y, up = [], 0, 0, True
    for _ in range(64):
        order.append(y * 8 + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                x, y = x + 1, y - 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                x, y = x - 1, y + 1
    return order


ZIGZAG = _zigzag()

_lut_cache = {}


def _huff_lut(counts, values):
    """T.81 C.2 canonical codes -> 16-bit-peek lookup (length, symbol);
    length 0 marks a bit pattern that is no code of the table."""
    key = (bytes(counts), bytes(values))
    lut = _lut_cache.get(key)
    if lut is not None:
        return lut
    lens = [0] * 65536
    syms = [0] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >> length:
                raise JpegError("DHT: more codes than the lengths allow")
            lo = code << (16 - length)
            hi = (code + 1) << (16 - length)
            lens[lo:hi] = [length] * (hi - lo)
            syms[lo:hi] = [values[k]] * (hi - lo)
            code += 1
            k += 1
        code <<= 1
    lut = (lens, syms)
    _lut_cache[key] = lut
    return lut


def _decode_interval(data, n_mcu, plan, out, what):
    """Decode exactly n_mcu MCUs from one restart interval's unstuffed
    bytes into out[i][slot]; returns the number of pad bits. plan is a
    list of (slot, pred_index, dc_lut, ac_lut)."""
    total = len(data) * 8
    nbytes = len(data)
    pos = acc = nacc = used = 0
    preds = [0, 0, 0]
    zz = ZIGZAG
    for i in range(n_mcu):
        mcu = out[i]
        for slot, comp, (dlen, dsym), (alen, asym) in plan:
            blk = mcu[slot]
            # ---- DC
            while nacc < 32:
                acc = (acc << 8) | (data[pos] if pos < nbytes else 0)
                pos += 1
                nacc += 8
            peek = (acc >> (nacc - 16)) & 0xFFFF
            ln = dlen[peek]
            if ln == 0:
                raise JpegError(f"{what}: DC code not in table")
            t = dsym[peek]
            if t > 11:
                raise JpegError(f"{what}: DC category {t} > 11")
            nacc -= ln
            used += ln
            diff = 0
            if t:
                nacc -= t
                used += t
                diff = (acc >> nacc) & ((1 << t) - 1)
                if diff < (1 << (t - 1)):
                    diff -= (1 << t) - 1
            acc &= (1 << nacc) - 1
            preds[comp] += diff
            blk[0] = preds[comp]
            # ---- AC
            k = 1
            while k < 64:
                while nacc < 32:
                    acc = (acc << 8) | (data[pos] if pos < nbytes else 0)
                    pos += 1
                    nacc += 8
                peek = (acc >> (nacc - 16)) & 0xFFFF
                ln = alen[peek]
                if ln == 0:
                    raise JpegError(f"{what}: AC code not in table")
                rs = asym[peek]
                nacc -= ln
                used += ln
                r, s = rs >> 4, rs & 15
                if s == 0:
                    acc &= (1 << nacc) - 1
                    if r == 15:
                        k += 16
                        if k > 64:
                            raise JpegError(f"{what}: ZRL runs past 64")
                        continue
                    if r == 0:
                        break
                    raise JpegError(f"{what}: symbol {rs:#x} in baseline")
                if s > 10:
                    raise JpegError(f"{what}: AC category {s} > 10")
                k += r
                if k > 63:
                    raise JpegError(f"{what}: block runs past 64 coefficients")
                nacc -= s
                used += s
                v = (acc >> nacc) & ((1 << s) - 1)
                if v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                acc &= (1 << nacc) - 1
                blk[zz[k]] = v
                k += 1
            if used > total:
                raise JpegError(f"{what}: entropy data ends early")
    pad = (-used) % 8
    if used + pad != total:
        raise JpegError(f"{what}: {(total - used - pad) // 8} bytes remain "
                        "after the last MCU")
    if pad:
        last = data[-1] & ((1 << pad) - 1)
        if last != (1 << pad) - 1:
            raise JpegError(f"{what}: pad bits before the marker are not 1")
    return pad


def decode_coeffs(stream):
    """Baseline JFIF -> dict(width, height, fullcolor, qy, qc, dri, blocks,
    pad_bits). qy/qc are natural-order int arrays from the stream's DQT;
    blocks is int32 [mcuy][mcux][slot][64] holding EVERY block of every
    MCU, pads outside the picture included; pad_bits lists the 1-fill bits
    that closed each restart interval. Raises JpegError on any violation."""
    s = bytes(stream)
    n = len(s)
    if s[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    p = 2
    dqt, dht = {}, {}
    frame = scan = None
    dri = 0
    seen_app0 = False
    while True:
        if p + 4 > n:
            raise JpegError("stream ends inside the headers")
        if s[p] != 0xFF:
            raise JpegError(f"expected a marker at byte {p}")
        m = s[p + 1]
        seglen = (s[p + 2] << 8) | s[p + 3]
        body = s[p + 4:p + 2 + seglen]
        if seglen < 2 or p + 2 + seglen > n:
            raise JpegError(f"marker {m:#x}: segment runs past the stream")
        p += 2 + seglen
        if m == 0xE0:
            if body[:5] != b"JFIF\0":
                raise JpegError("APP0 is not JFIF")
            seen_app0 = True
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq != 0 or q + 65 > len(body):
                    raise JpegError("DQT: baseline needs 8-bit tables")
                tab = np.zeros(64, np.int64)
                for i in range(64):
                    tab[ZIGZAG[i]] = body[q + 1 + i]
                if (tab == 0).any():
                    raise JpegError("DQT: zero quantiser")
                dqt[tq] = tab
                q += 65
        elif m == 0xC0:
            if frame is not None:
                raise JpegError("second SOF0")
            if body[0] != 8:
                raise JpegError("SOF0: precision is not 8")
            height = (body[1] << 8) | body[2]
            width = (body[3] << 8) | body[4]
            nc = body[5]
            if len(body) != 6 + 3 * nc:
                raise JpegError("SOF0: bad length")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4,
                      body[7 + 3 * i] & 15, body[8 + 3 * i])
                     for i in range(nc)]
            frame = (width, height, comps)
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                counts = body[q + 1:q + 17]
                nv = sum(counts)
                if tc > 1 or len(counts) != 16 or q + 17 + nv > len(body):
                    raise JpegError("DHT: bad table")
                dht[(tc, th)] = _huff_lut(counts, body[q + 17:q + 17 + nv])
                q += 17 + nv
        elif m == 0xDD:
            if seglen != 4:
                raise JpegError("DRI: bad length")
            dri = (body[0] << 8) | body[1]
        elif m == 0xDA:
            ns = body[0]
            if len(body) != 1 + 2 * ns + 3:
                raise JpegError("SOS: bad length")
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4,
                    body[2 + 2 * i] & 15) for i in range(ns)]
            if tuple(body[1 + 2 * ns:]) != (0, 63, 0):
                raise JpegError("SOS: not a baseline sequential scan")
            scan = sel
            break
        else:
            raise JpegError(f"unexpected marker {m:#x} in the headers")
    if not seen_app0 or frame is None:
        raise JpegError("APP0 or SOF0 missing before SOS")
    width, height, comps = frame
    if width == 0 or height == 0:
        raise JpegError("empty picture")
    if len(comps) != 3 or [c[0] for c in comps] != [c[0] for c in scan]:
        raise JpegError("expected one interleaved scan of 3 components")
    (_, hy, vy, tqy), (_, hb, vb, tqb), (_, hr, vr, tqr) = comps
    if (hb, vb, hr, vr) != (1, 1, 1, 1) or (hy, vy) not in ((1, 1), (2, 2)) \
            or tqb != tqr:
        raise JpegError("sampling is neither 4:4:4 nor 4:2:0")
    fullcolor = hy == 1
    mcu = 8 if fullcolor else 16
    mcux, mcuy = -(-width // mcu), -(-height // mcu)
    per_mcu = 3 if fullcolor else 6
    try:
        qy, qc = dqt[tqy], dqt[tqb]
        luts = [(dht[(0, td)], dht[(1, ta)]) for _, td, ta in scan]
    except KeyError as e:
        raise JpegError(f"table {e} used but not defined") from None
    plan = [(i, 0) + luts[0] for i in range(per_mcu - 2)]
    plan += [(per_mcu - 2, 1) + luts[1], (per_mcu - 1, 2) + luts[2]]

    # split the entropy-coded segment at its markers, undoing 0xFF00
    intervals, rst_seen = [], []
    cur = bytearray()
    while True:
        q = s.find(b"\xff", p)
        if q < 0 or q + 1 >= n:
            raise JpegError("stream ends before EOI")
        cur += s[p:q]
        m = s[q + 1]
        p = q + 2
        if m == 0x00:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            intervals.append(bytes(cur))
            rst_seen.append(m - 0xD0)
            cur = bytearray()
        elif m == 0xD9:
            intervals.append(bytes(cur))
            break
        else:
            raise JpegError(f"marker {m:#x} inside the entropy-coded data")
    if p != n:
        raise JpegError(f"{n - p} bytes after EOI")
    if rst_seen != [i & 7 for i in range(len(rst_seen))]:
        raise JpegError(f"RSTn numbers {rst_seen} do not run 0..7 cyclically")
    n_mcu = mcux * mcuy
    per_interval = dri if dri else n_mcu
    if len(intervals) * per_interval != n_mcu:
        raise JpegError(f"{len(intervals)} restart intervals of "
                        f"{per_interval} MCUs for {n_mcu} MCUs")
    flat = [[[0] * 64 for _ in range(per_mcu)] for _ in range(n_mcu)]
    pads = []
    for i, data in enumerate(intervals):
        pads.append(_decode_interval(
            data, per_interval, plan,
            flat[i * per_interval:(i + 1) * per_interval], f"interval {i}"))
    blocks = np.array(flat, np.int32).reshape(mcuy, mcux, per_mcu, 64)
    return dict(width=width, height=height, fullcolor=fullcolor, qy=qy,
                qc=qc, dri=dri, blocks=blocks, pad_bits=pads)


# ---- float64 reference --------------------------------------------------------

def _dct_matrix():
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] *= np.sqrt(0.5)
    return m


DCT = _dct_matrix()     # DCT[u][x] = 0.5 c(u) cos((2x+1) u pi / 16)


def reference_planes(bgrx, w, h, fullcolor):
    """8-bit Y, Cb, Cr planes of one stripe at whole-MCU size, as float64.
    Pixel reads clamp to the stripe's last row and column (T.81 A.2.4
    leaves the completion of partial MCUs to the encoder; both encoders
    replicate pixels). float32 arithmetic in the order written in
    rgb_to_ycbcr; 4:2:0 chroma = the 2x2 quad summed in load order x 0.25;
    clamp to 0..255, round half to even."""
    f32 = np.float32
    px = np.asarray(bgrx, np.uint8).reshape(h, w, 4)
    mcu = 8 if fullcolor else 16
    ph, pw = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    px = np.pad(px, ((0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    b, g, r = (px[:, :, i].astype(f32) for i in range(3))
    y = f32(0.299) * r + f32(0.587) * g + f32(0.114) * b
    cb = f32(-0.168736) * r - f32(0.331264) * g + f32(0.5) * b + f32(128)
    cr = f32(0.5) * r - f32(0.418688) * g - f32(0.081312) * b + f32(128)
    assert y.dtype == cb.dtype == cr.dtype == np.float32

    def sample(v):
        return np.rint(np.clip(v, f32(0), f32(255))).astype(np.float64)

    if not fullcolor:
        def quad(c):
            s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            assert s.dtype == np.float32
            return s * f32(0.25)
        cb, cr = quad(cb), quad(cr)
    return sample(y), sample(cb), sample(cr)


def _plane_blocks(plane, q):
    """[H][W] samples -> [H/8][W/8][64] real DCT / q, natural order."""
    hh, ww = plane.shape
    blk = (plane - 128.0).reshape(hh // 8, 8, ww // 8, 8).transpose(0, 2, 1, 3)
    coef = DCT @ blk @ DCT.T            # [v][u] = sum_yx M[v][y] B[y][x] M[u][x]
    return coef.reshape(hh // 8, ww // 8, 64) / np.asarray(q, np.float64)


def reference_coeff_real(bgrx, w, h, qy, qc, fullcolor):
    """Unrounded float64 coefficient / quantiser for every block of the
    stripe: float64 [mcuy][mcux][slot][64], the layout of decode_coeffs."""
    y, cb, cr = reference_planes(bgrx, w, h, fullcolor)
    ry, rcb, rcr = _plane_blocks(y, qy), _plane_blocks(cb, qc), \
        _plane_blocks(cr, qc)
    if fullcolor:
        return np.stack([ry, rcb, rcr], axis=2)
    my, mx = rcb.shape[:2]
    ry = ry.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4)
    return np.concatenate([ry.reshape(my, mx, 4, 64),
                           rcb[:, :, None], rcr[:, :, None]], axis=2)


# ---- checker --------------------------------------------------------------------

def coeff_allowance(decoded, reference):
    """Per-coefficient bound on |c - r|: half a step, plus what float32
    can move the transform before the rounding (1.1e-3 in the unquantised
    sum: 16 multiply-adds on partial sums <= 1024, each within 2^-24 of its
    result), plus 2 ulp relative for multiplying by a rounded reciprocal."""
    n_luma = 1 if decoded["fullcolor"] else 4
    q = np.concatenate([np.tile(decoded["qy"], (n_luma, 1)),
                        np.tile(decoded["qc"], (2, 1))]).astype(np.float64)
    return 0.5 + 1.1e-3 / q + 2.0 ** -22 * np.abs(reference)


def check_coeffs(decoded, reference, stripe=None):
    """Every decoded coefficient c must satisfy
    |c - r| <= 0.5 + 1.1e-3/q + 2^-22 |r| against the reference r.
    Raises AssertionError naming the count and the first violations;
    returns dict(checked, worst_excess, worst_allow): the largest
    |c - r| - 0.5 seen and the allowance beyond 0.5 at that coefficient."""
    c = np.asarray(decoded["blocks"], np.float64)
    r = np.asarray(reference, np.float64)
    assert c.shape == r.shape, f"block grid {c.shape} against {r.shape}"
    err = np.abs(c - r)
    allow = coeff_allowance(decoded, r)
    bad = np.argwhere(err > allow)
    if len(bad):
        first = ", ".join(
            f"(stripe {stripe}, MCU ({my},{mx}), slot {sl}, index {k}: "
            f"c={int(c[my, mx, sl, k])} r={r[my, mx, sl, k]:.6f})"
            for my, mx, sl, k in bad[:6])
        raise AssertionError(
            f"{len(bad)} of {c.size} coefficients are no rounding of the "
            f"float64 reference: {first}")
    worst = np.unravel_index(np.argmax(err), err.shape)
    return dict(checked=int(c.size), worst_excess=float(err[worst] - 0.5),
                worst_allow=float(allow[worst] - 0.5))


# ---- test contents ----------------------------------------------------------------

def content_noise(w, h, seed):
    """Uniform random BGRX, alpha 255."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4),
                                               dtype=np.uint8)
    img[:, :, 3] = 255
    return np.ascontiguousarray(img)


def content_structures(w, h):
    """16x16 tiles cycling through the cases an entropy coder and a
    quantiser get wrong: a 1-pixel checkerboard (a lone (7,7) coefficient
    behind three ZRL codes), saturated red, green and blue (chroma clamp),
    a flat odd grey (DC exactly between two levels at even quantisers),
    alternating black and white 8x8 blocks (DC difference category 11 at
    quality 100). The last two columns and rows are the inverse of their
    inner neighbour, so that a pad block left at zero, or filled from the
    wrong side, cannot equal one that replicates the edge."""
    yy, xx = np.mgrid[0:h, 0:w]
    kind = (xx // 16 + yy // 16) % 6
    img = np.zeros((h, w, 4), np.uint8)
    checker = (((xx + yy) & 1) * 255).astype(np.uint8)
    blocks = (((xx // 8 + yy // 8) & 1) * 255).astype(np.uint8)
    bgr = {0: (checker,) * 3, 1: (0, 0, 255), 2: (0, 255, 0), 3: (255, 0, 0),
           4: (77, 77, 77), 5: (blocks,) * 3}
    for k, chans in bgr.items():
        sel = kind == k
        for c in range(3):
            v = chans[c]
            img[:, :, c][sel] = v[sel] if isinstance(v, np.ndarray) else v
    if w > 2:
        img[:, -2:, :3] = 255 - img[:, -3:-2, :3]
    if h > 2:
        img[-2:, :, :3] = 255 - img[-3:-2, :, :3]
    img[:, :, 3] = 255
    return np.ascontiguousarray(img)
