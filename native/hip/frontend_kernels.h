// Launchers of the capture front end kernels (hip/frontend.hip): overlay,
// downscale and block damage on device-resident BGRX frames. Every stride
// is in bytes and a multiple of 4; frames are uchar4-aligned.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hipflux {

// Blend a ww x wh straight-alpha BGRA watermark, top-left at (x0, y0),
// into frame in place. Runs over the clipped rectangle only.
void launch_overlay_watermark(uint8_t* frame, int fw, int fh, int stride,
                              const uint8_t* wm, int ww, int wh, int x0,
                              int y0, hipStream_t stream);

// Blend a cw x ch premultiplied-ARGB cursor, top-left at (cx, cy).
void launch_overlay_cursor(uint8_t* frame, int fw, int fh, int stride,
                           const uint32_t* argb, int cw, int ch, int cx,
                           int cy, hipStream_t stream);

// Fractional bilinear downscale. xtab[ow] / ytab[oh] hold the host's
// bilinear_axis_table() entries packed as (index << 8) | weight.
void launch_bilinear_downscale(const uint8_t* src, int sstride, int w, int h,
                               const uint32_t* xtab, const uint32_t* ytab,
                               uint8_t* dst, int ow, int oh, int ostride,
                               hipStream_t stream);

// Box downscale by div in 2..4 (ow = w / div, oh = h / div, floored).
void launch_box_downscale(const uint8_t* src, int sstride, int div,
                          uint8_t* dst, int ow, int oh, int ostride,
                          hipStream_t stream);

// One byte per 16x16 block of a w x h frame (bx * by bytes, row-major):
// 1 if any byte of the block differs between cur and prev by more than
// threshold (threshold <= 0: differs at all), else 0.
void launch_damage_flags(const uint8_t* cur, const uint8_t* prev, int w,
                         int h, int stride, int threshold, uint8_t* flags,
                         int bx, int by, hipStream_t stream);

}  // namespace hipflux
