// Watermark + cursor overlay on BGRX capture frames.
// The origin math and the two blend formulas live here once: the engine's
// host path loops over them below, and the device front end
// (hip/frontend.hip) calls the same blend_* functions from its kernels
// with an origin computed on the host by watermark_origin().
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#if defined(__HIP__)
#define HIPFLUX_HD __host__ __device__
#else
#define HIPFLUX_HD
#endif

namespace hipflux {

HIPFLUX_HD inline uint8_t clip8u(long v) {
  return static_cast<uint8_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Watermark pixels are straight (non-premultiplied) alpha.
HIPFLUX_HD inline uint8_t blend_watermark(int s, int d, int a) {
  return static_cast<uint8_t>((s * a + d * (255 - a) + 127) / 255);
}

// XFixes cursor pixels are premultiplied ARGB; p is one colour channel.
HIPFLUX_HD inline uint8_t blend_cursor(uint32_t p, int d, int a) {
  return clip8u((p * 255 + d * (255 - a)) / 255);
}

// Top-left corner of a w x h watermark on a fw x fh frame. Locations:
// 1=TL 2=TR 3=BL 4=BR 5=center 6=animated (bounces with frame_idx).
// False for any other location: nothing is drawn.
inline bool watermark_origin(int location, int fw, int fh, int w, int h,
                             uint64_t frame_idx, int& x0, int& y0) {
  const int margin = 16;
  x0 = 0;
  y0 = 0;
  switch (location) {
    case 1: x0 = margin; y0 = margin; break;
    case 2: x0 = fw - w - margin; y0 = margin; break;
    case 3: x0 = margin; y0 = fh - h - margin; break;
    case 4: x0 = fw - w - margin; y0 = fh - h - margin; break;
    case 5: x0 = (fw - w) / 2; y0 = (fh - h) / 2; break;
    case 6: {  // bounce animation
      int sx = std::max(1, fw - w), sy = std::max(1, fh - h);
      x0 = static_cast<int>((frame_idx * 3) % (2 * sx));
      y0 = static_cast<int>((frame_idx * 2) % (2 * sy));
      if (x0 >= sx) x0 = 2 * sx - x0 - 1;
      if (y0 >= sy) y0 = 2 * sy - y0 - 1;
      break;
    }
    default: return false;
  }
  return true;
}

// Watermark: raw ".bgra" file = u32 width, u32 height, then BGRA pixels.
// (The Python layer converts PNG -> .bgra via PIL; keeps libpng out of the
// native build.)
struct Watermark {
  int w = 0, h = 0;
  std::vector<uint8_t> bgra;
  bool load(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint32_t wh[2];
    if (std::fread(wh, 4, 2, f) != 2) {
      std::fclose(f);
      return false;
    }
    w = static_cast<int>(wh[0]);
    h = static_cast<int>(wh[1]);
    if (w <= 0 || h <= 0 || w > 8192 || h > 8192) {
      std::fclose(f);
      return false;
    }
    bgra.resize(static_cast<size_t>(w) * h * 4);
    size_t got = std::fread(bgra.data(), 1, bgra.size(), f);
    std::fclose(f);
    return got == bgra.size();
  }

  void composite(uint8_t* frame, int fw, int fh, int stride, int location,
                 uint64_t frame_idx) const {
    if (w == 0) return;
    int x0, y0;
    if (!watermark_origin(location, fw, fh, w, h, frame_idx, x0, y0)) return;
    for (int y = 0; y < h; ++y) {
      int fy = y0 + y;
      if (fy < 0 || fy >= fh) continue;
      uint8_t* dst = frame + static_cast<size_t>(fy) * stride;
      const uint8_t* src = bgra.data() + static_cast<size_t>(y) * w * 4;
      for (int x = 0; x < w; ++x) {
        int fx = x0 + x;
        if (fx < 0 || fx >= fw) continue;
        int a = src[x * 4 + 3];
        if (a == 0) continue;
        uint8_t* d = dst + fx * 4;
        for (int c = 0; c < 3; ++c)
          d[c] = blend_watermark(src[x * 4 + c], d[c], a);
      }
    }
  }
};

// Blend a cw x ch premultiplied-ARGB cursor with its top-left at (cx, cy).
inline void composite_cursor(uint8_t* frame, int fw, int fh, int stride,
                             const uint32_t* argb, int cw, int ch, int cx,
                             int cy) {
  for (int y = 0; y < ch; ++y) {
    int fy = cy + y;
    if (fy < 0 || fy >= fh) continue;
    uint8_t* dst = frame + static_cast<size_t>(fy) * stride;
    for (int x = 0; x < cw; ++x) {
      int fx = cx + x;
      if (fx < 0 || fx >= fw) continue;
      uint32_t p = argb[static_cast<size_t>(y) * cw + x];
      int a = p >> 24;
      if (a == 0) continue;
      uint8_t* d = dst + fx * 4;
      d[0] = blend_cursor(p & 0xFF, d[0], a);
      d[1] = blend_cursor((p >> 8) & 0xFF, d[1], a);
      d[2] = blend_cursor((p >> 16) & 0xFF, d[2], a);
    }
  }
}

}  // namespace hipflux
