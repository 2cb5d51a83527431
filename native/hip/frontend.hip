// CDNA4 (gfx950) kernels of the capture front end: watermark / cursor
// overlay, bilinear and box downscale, and the 16x16 block damage diff,
// all on device-resident BGRX frames.
//
// Every kernel is streaming integer work, one uchar4 (or uint4) per lane
// per access, 256-thread blocks of 64x4 pixels so that a wave covers one
// contiguous row segment. The arithmetic is the host's: the blend
// formulas come from cpu/overlay.h and the interpolation from
// cpu/scale.h, and everything that needs 64-bit or clamped position math
// (overlay origin, bilinear sample tables) arrives computed by the host.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../cpu/overlay.h"
#include "../cpu/scale.h"
#include "frontend_kernels.h"

namespace hipflux {

namespace {

constexpr int kTileW = 64, kTileH = 4;   // 256 threads, one wave per row

inline dim3 tile_grid(int w, int h) {
  return dim3((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH);
}

__device__ inline uchar4 load_px(const uint8_t* base, int stride, int x,
                                 int y) {
  return *reinterpret_cast<const uchar4*>(
      base + static_cast<size_t>(y) * stride + static_cast<size_t>(x) * 4);
}

__device__ inline uchar4* px_ptr(uint8_t* base, int stride, int x, int y) {
  return reinterpret_cast<uchar4*>(base + static_cast<size_t>(y) * stride +
                                   static_cast<size_t>(x) * 4);
}

}  // namespace

// ---------------------------------------------------------------------------
// Overlays. (rx0, ry0, rw, rh) is the overlay's rectangle clipped to the
// frame; (x0, y0) its unclipped top-left. Byte 3 of the frame is kept.
__global__ __launch_bounds__(256) void k_overlay_watermark(
    uint8_t* __restrict__ frame, int stride, const uint8_t* __restrict__ wm,
    int ww, int x0, int y0, int rx0, int ry0, int rw, int rh) {
  const int x = blockIdx.x * kTileW + threadIdx.x;
  const int y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= rw || y >= rh) return;
  const int fx = rx0 + x, fy = ry0 + y;
  const uchar4 s = load_px(wm, ww * 4, fx - x0, fy - y0);
  const int a = s.w;
  if (a == 0) return;
  uchar4* dp = px_ptr(frame, stride, fx, fy);
  uchar4 d = *dp;
  d.x = blend_watermark(s.x, d.x, a);
  d.y = blend_watermark(s.y, d.y, a);
  d.z = blend_watermark(s.z, d.z, a);
  *dp = d;
}

__global__ __launch_bounds__(256) void k_overlay_cursor(
    uint8_t* __restrict__ frame, int stride, const uint32_t* __restrict__ argb,
    int cw, int cx, int cy, int rx0, int ry0, int rw, int rh) {
  const int x = blockIdx.x * kTileW + threadIdx.x;
  const int y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= rw || y >= rh) return;
  const int fx = rx0 + x, fy = ry0 + y;
  const uint32_t p = argb[static_cast<size_t>(fy - cy) * cw + (fx - cx)];
  const int a = p >> 24;
  if (a == 0) return;
  uchar4* dp = px_ptr(frame, stride, fx, fy);
  uchar4 d = *dp;
  d.x = blend_cursor(p & 0xFF, d.x, a);
  d.y = blend_cursor((p >> 8) & 0xFF, d.y, a);
  d.z = blend_cursor((p >> 16) & 0xFF, d.z, a);
  *dp = d;
}

// ---------------------------------------------------------------------------
// Bilinear: one output pixel per lane. dx / dy are 0 when the source has a
// single column / row (the second tap is then the first one).
__global__ __launch_bounds__(256) void k_bilinear_downscale(
    const uint8_t* __restrict__ src, int sstride, int dx, int dy,
    const uint32_t* __restrict__ xtab, const uint32_t* __restrict__ ytab,
    uint8_t* __restrict__ dst, int ow, int oh, int ostride) {
  const int x = blockIdx.x * kTileW + threadIdx.x;
  const int y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= ow || y >= oh) return;
  const uint32_t xt = xtab[x], yt = ytab[y];
  const int ix = xt >> 8, fx = xt & 0xFF;
  const int iy = yt >> 8, fy = yt & 0xFF;
  const uchar4 a = load_px(src, sstride, ix, iy);
  const uchar4 b = load_px(src, sstride, ix + dx, iy);
  const uchar4 c = load_px(src, sstride, ix, iy + dy);
  const uchar4 e = load_px(src, sstride, ix + dx, iy + dy);
  uchar4 o;
  o.x = bilinear_sample(a.x, b.x, c.x, e.x, fx, fy);
  o.y = bilinear_sample(a.y, b.y, c.y, e.y, fx, fy);
  o.z = bilinear_sample(a.z, b.z, c.z, e.z, fx, fy);
  o.w = bilinear_sample(a.w, b.w, c.w, e.w, fx, fy);
  *px_ptr(dst, ostride, x, y) = o;
}

// Box: out = (sum of DIV x DIV + n/2) / n per channel.
template <int DIV>
__global__ __launch_bounds__(256) void k_box_downscale(
    const uint8_t* __restrict__ src, int sstride, uint8_t* __restrict__ dst,
    int ow, int oh, int ostride) {
  const int x = blockIdx.x * kTileW + threadIdx.x;
  const int y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= ow || y >= oh) return;
  constexpr int n = DIV * DIV, half = n / 2;
  int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
#pragma unroll
  for (int j = 0; j < DIV; ++j) {
#pragma unroll
    for (int i = 0; i < DIV; ++i) {
      const uchar4 p = load_px(src, sstride, x * DIV + i, y * DIV + j);
      acc0 += p.x;
      acc1 += p.y;
      acc2 += p.z;
      acc3 += p.w;
    }
  }
  uchar4 o;
  o.x = static_cast<uint8_t>((acc0 + half) / n);
  o.y = static_cast<uint8_t>((acc1 + half) / n);
  o.z = static_cast<uint8_t>((acc2 + half) / n);
  o.w = static_cast<uint8_t>((acc3 + half) / n);
  *px_ptr(dst, ostride, x, y) = o;
}

// ---------------------------------------------------------------------------
// Damage: one wave per 16x16 block, four blocks per workgroup. Lane l
// holds four pixels of block row l / 4; rows and pixels past the frame edge
// (the last block column / row) take no part. The flag is reduced with a
// ballot and stored by lane 0 alone.
__device__ inline bool px_dirty(uint32_t c, uint32_t p, int threshold) {
  if (c == p) return false;
  if (threshold <= 0) return true;
  bool dirty = false;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int d = static_cast<int>((c >> k) & 0xFF) -
                  static_cast<int>((p >> k) & 0xFF);
    dirty |= d > threshold || d < -threshold;
  }
  return dirty;
}

__global__ __launch_bounds__(256) void k_damage_flags(
    const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int w,
    int h, int stride, int threshold, uint8_t* __restrict__ flags, int bx,
    int nblocks) {
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nblocks) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  const int x = (blk % bx) * 16 + (lane & 3) * 4;
  const int y = (blk / bx) * 16 + (lane >> 2);
  bool dirty = false;
  if (y < h && x < w) {
    const size_t off = static_cast<size_t>(y) * stride +
                       static_cast<size_t>(x) * 4;
    if ((stride & 15) == 0 && x + 4 <= w) {
      const uint4 c = *reinterpret_cast<const uint4*>(cur + off);
      const uint4 p = *reinterpret_cast<const uint4*>(prev + off);
      dirty = px_dirty(c.x, p.x, threshold);
      dirty |= px_dirty(c.y, p.y, threshold);
      dirty |= px_dirty(c.z, p.z, threshold);
      dirty |= px_dirty(c.w, p.w, threshold);
    } else {
      const int n = min(4, w - x);
      for (int i = 0; i < n; ++i)
        dirty |= px_dirty(
            *reinterpret_cast<const uint32_t*>(cur + off + i * 4),
            *reinterpret_cast<const uint32_t*>(prev + off + i * 4), threshold);
    }
  }
  const bool any = __ballot(dirty) != 0;
  if (lane == 0) flags[blk] = any ? 1 : 0;
}

// ---------------------------------------------------------------------------
namespace {

// Clip the w x h rectangle at (x0, y0) to a fw x fh frame.
inline bool clip_rect(int x0, int y0, int w, int h, int fw, int fh, int& rx0,
                      int& ry0, int& rw, int& rh) {
  rx0 = std::max(0, x0);
  ry0 = std::max(0, y0);
  rw = std::min(fw, x0 + w) - rx0;
  rh = std::min(fh, y0 + h) - ry0;
  return rw > 0 && rh > 0;
}

}  // namespace

void launch_overlay_watermark(uint8_t* frame, int fw, int fh, int stride,
                              const uint8_t* wm, int ww, int wh, int x0,
                              int y0, hipStream_t stream) {
  int rx0, ry0, rw, rh;
  if (!clip_rect(x0, y0, ww, wh, fw, fh, rx0, ry0, rw, rh)) return;
  hipLaunchKernelGGL(k_overlay_watermark, tile_grid(rw, rh),
                     dim3(kTileW, kTileH), 0, stream, frame, stride, wm, ww,
                     x0, y0, rx0, ry0, rw, rh);
}

void launch_overlay_cursor(uint8_t* frame, int fw, int fh, int stride,
                           const uint32_t* argb, int cw, int ch, int cx,
                           int cy, hipStream_t stream) {
  int rx0, ry0, rw, rh;
  if (!clip_rect(cx, cy, cw, ch, fw, fh, rx0, ry0, rw, rh)) return;
  hipLaunchKernelGGL(k_overlay_cursor, tile_grid(rw, rh),
                     dim3(kTileW, kTileH), 0, stream, frame, stride, argb, cw,
                     cx, cy, rx0, ry0, rw, rh);
}

void launch_bilinear_downscale(const uint8_t* src, int sstride, int w, int h,
                               const uint32_t* xtab, const uint32_t* ytab,
                               uint8_t* dst, int ow, int oh, int ostride,
                               hipStream_t stream) {
  if (ow <= 0 || oh <= 0) return;
  hipLaunchKernelGGL(k_bilinear_downscale, tile_grid(ow, oh),
                     dim3(kTileW, kTileH), 0, stream, src, sstride,
                     w > 1 ? 1 : 0, h > 1 ? 1 : 0, xtab, ytab, dst, ow, oh,
                     ostride);
}

void launch_box_downscale(const uint8_t* src, int sstride, int div,
                          uint8_t* dst, int ow, int oh, int ostride,
                          hipStream_t stream) {
  if (ow <= 0 || oh <= 0) return;
  const dim3 grid = tile_grid(ow, oh), block(kTileW, kTileH);
  switch (div) {
    case 2:
      hipLaunchKernelGGL(k_box_downscale<2>, grid, block, 0, stream, src,
                         sstride, dst, ow, oh, ostride);
      break;
    case 3:
      hipLaunchKernelGGL(k_box_downscale<3>, grid, block, 0, stream, src,
                         sstride, dst, ow, oh, ostride);
      break;
    case 4:
      hipLaunchKernelGGL(k_box_downscale<4>, grid, block, 0, stream, src,
                         sstride, dst, ow, oh, ostride);
      break;
    default:
      break;   // the owner never asks for another divisor
  }
}

void launch_damage_flags(const uint8_t* cur, const uint8_t* prev, int w,
                         int h, int stride, int threshold, uint8_t* flags,
                         int bx, int by, hipStream_t stream) {
  const int nblocks = bx * by;
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(k_damage_flags, dim3((nblocks + 3) / 4), dim3(256), 0,
                     stream, cur, prev, w, h, stride, threshold, flags, bx,
                     nblocks);
}

}  // namespace hipflux
