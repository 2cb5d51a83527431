// Exact integer box downscale for BGRX capture frames.
// out(x,y) = round(mean of the div x div source block), per channel.
// Integer semantics are identical everywhere (engine CPU path), so tests
// can compare against an independent numpy implementation bit-exactly.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace hipflux {

inline void box_downscale_bgrx(const uint8_t* src, int sstride, int w,
                               int h, int div, std::vector<uint8_t>& out,
                               int& ow, int& oh, int& ostride) {
  ow = w / div;
  oh = h / div;
  ostride = ow * 4;
  out.resize(static_cast<size_t>(ostride) * oh);
  const int n = div * div, half = n / 2;
  for (int y = 0; y < oh; ++y) {
    uint8_t* d = out.data() + static_cast<size_t>(y) * ostride;
    for (int x = 0; x < ow; ++x) {
      int acc[4] = {0, 0, 0, 0};
      for (int dy = 0; dy < div; ++dy) {
        const uint8_t* s = src + static_cast<size_t>(y * div + dy) * sstride +
                           static_cast<size_t>(x) * div * 4;
        for (int dx = 0; dx < div; ++dx) {
          acc[0] += s[dx * 4 + 0];
          acc[1] += s[dx * 4 + 1];
          acc[2] += s[dx * 4 + 2];
          acc[3] += s[dx * 4 + 3];
        }
      }
      d[x * 4 + 0] = static_cast<uint8_t>((acc[0] + half) / n);
      d[x * 4 + 1] = static_cast<uint8_t>((acc[1] + half) / n);
      d[x * 4 + 2] = static_cast<uint8_t>((acc[2] + half) / n);
      d[x * 4 + 3] = static_cast<uint8_t>((acc[3] + half) / n);
    }
  }
}

// Output size of the fractional bilinear downscale along one axis.
inline int bilinear_out_size(int n, float scale) {
  return std::max(1, static_cast<int>(n * scale + 0.5f));
}

// Per-axis sample table of the fractional bilinear downscale: output
// sample i reads source samples idx[i] and idx[i] + 1 (idx[i] alone when
// n_in == 1) with the 8-bit weight wt[i] on the second. Source position of
// output sample center i: (i + 0.5) / scale - 0.5, in 16.16 fixed point
// computed from the integer output size. The device front end uploads
// these tables, so the 64-bit position math and the clamps exist once.
inline void bilinear_axis_table(int n_in, int n_out, std::vector<int>& idx,
                                std::vector<int>& wt) {
  const int64_t step = (static_cast<int64_t>(n_in) << 16) / n_out;
  idx.resize(n_out);
  wt.resize(n_out);
  for (int i = 0; i < n_out; ++i) {
    int64_t s = ((2 * static_cast<int64_t>(i) + 1) * step - (1 << 16)) / 2;
    if (s < 0) s = 0;
    int ii = static_cast<int>(s >> 16);
    if (ii > n_in - 2) ii = n_in - 2;
    int fr = static_cast<int>((s >> 8) & 0xFF);
    if (n_in == 1) { ii = 0; fr = 0; }
    idx[i] = ii;
    wt[i] = fr;
  }
}

// One channel of one output pixel: a b / c e are the 2x2 source samples,
// fx and fy the 8-bit weights. 8.8 horizontally, 8.16 vertically,
// round-half-up.
#if defined(__HIP__)
__host__ __device__
#endif
inline uint8_t bilinear_sample(int a, int b, int c, int e, int fx, int fy) {
  int top = (a << 8) + (b - a) * fx;       // 8.8
  int bot = (c << 8) + (e - c) * fx;
  int v = (top << 8) + (bot - top) * fy;   // 8.16
  return static_cast<uint8_t>((v + (1 << 15)) >> 16);
}

// Fractional bilinear downscale (0 < scale < 1), fixed-point 16.16
// sample positions with 8-bit interpolation weights. The reference's
// `scale` knob (Wayland logical->pixel ratios like 1.5x) needs
// non-integer ratios the box filter can't express. Integer math only,
// so the engine path and the numpy mirror in tests agree bit-exactly.
inline void bilinear_downscale_bgrx(const uint8_t* src, int sstride, int w,
                                    int h, float scale,
                                    std::vector<uint8_t>& out, int& ow,
                                    int& oh, int& ostride) {
  ow = bilinear_out_size(w, scale);
  oh = bilinear_out_size(h, scale);
  ostride = ow * 4;
  out.resize(static_cast<size_t>(ostride) * oh);
  std::vector<int> xi, xw, yi, yw;
  bilinear_axis_table(w, ow, xi, xw);
  bilinear_axis_table(h, oh, yi, yw);
  for (int y = 0; y < oh; ++y) {
    const int fy = yw[y];
    const uint8_t* r0 = src + static_cast<size_t>(yi[y]) * sstride;
    const uint8_t* r1 = r0 + (h > 1 ? sstride : 0);
    uint8_t* d = out.data() + static_cast<size_t>(y) * ostride;
    for (int x = 0; x < ow; ++x) {
      const uint8_t* a = r0 + static_cast<size_t>(xi[x]) * 4;
      const uint8_t* b = a + (w > 1 ? 4 : 0);
      const uint8_t* c = r1 + static_cast<size_t>(xi[x]) * 4;
      const uint8_t* e = c + (w > 1 ? 4 : 0);
      const int fx = xw[x];
      for (int ch = 0; ch < 4; ++ch)
        d[x * 4 + ch] = bilinear_sample(a[ch], b[ch], c[ch], e[ch], fx, fy);
    }
  }
}

}  // namespace hipflux
