// Sanitizer harness (ASan + UBSan) for the capture front end's host code:
// cpu/overlay.h (origin math, clipped watermark and cursor blends),
// bilinear_axis_table / bilinear_downscale_bgrx / box_downscale_bgrx in
// cpu/scale.h, and DamageTracker::update / apply_dirty. Exact-size
// buffers, so any read or write past a clipped edge or a partial block
// aborts with a nonzero exit; apply_dirty must agree with update.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cpu/damage.h"
#include "../cpu/overlay.h"
#include "../cpu/scale.h"

using namespace hipflux;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<uint32_t>(rng_state);
}

static void fail(const char* what) {
  std::fprintf(stderr, "frontend harness: %s\n", what);
  std::exit(1);
}

int main() {
  const int sizes[][2] = {{250, 90}, {64, 48}, {17, 5}, {1, 1}, {2, 1}};
  for (auto& wh : sizes) {
    const int w = wh[0], h = wh[1], stride = w * 4;
    std::vector<uint8_t> frame(static_cast<size_t>(stride) * h);
    for (auto& b : frame) b = static_cast<uint8_t>(rnd());

    // overlays: every location, marks smaller and larger than the frame,
    // bounce indices up to the uint64 range
    const int marks[][2] = {{40, 20}, {300, 100}, {1, 1}};
    for (auto& m : marks) {
      Watermark wm;
      wm.w = m[0];
      wm.h = m[1];
      wm.bgra.resize(static_cast<size_t>(wm.w) * wm.h * 4);
      for (auto& b : wm.bgra) b = static_cast<uint8_t>(rnd());
      const uint64_t idx[] = {0, 35, 70, 1000003, ~0ull};
      for (int loc = 0; loc <= 7; ++loc)
        for (uint64_t fi : idx) {
          std::vector<uint8_t> f = frame;
          wm.composite(f.data(), w, h, stride, loc, fi);
        }
    }
    std::vector<uint32_t> cursor(12 * 16);
    for (auto& p : cursor) p = rnd();
    const int pos[][2] = {{-5, -7}, {w - 3, h - 4}, {w / 2, h / 2},
                          {-12, -16}, {w, h}, {-100, 3}};
    for (auto& p : pos) {
      std::vector<uint8_t> f = frame;
      composite_cursor(f.data(), w, h, stride, cursor.data(), 12, 16, p[0],
                       p[1]);
    }

    // downscale: the tables must index inside the source
    const float scales[] = {0.25f, 0.3f, 0.5f, 0.67f, 0.9f};
    for (float s : scales) {
      std::vector<uint8_t> out;
      int ow, oh, ostride;
      bilinear_downscale_bgrx(frame.data(), stride, w, h, s, out, ow, oh,
                              ostride);
      std::vector<int> idx, wt;
      bilinear_axis_table(w, ow, idx, wt);
      for (int i = 0; i < ow; ++i)
        if (idx[i] < 0 || idx[i] > std::max(0, w - 2) || wt[i] < 0 ||
            wt[i] > 255)
          fail("bilinear table out of range");
    }
    for (int div = 2; div <= 4; ++div) {
      std::vector<uint8_t> out;
      int ow, oh, ostride;
      box_downscale_bgrx(frame.data(), stride, w, h, div, out, ow, oh,
                         ostride);
    }

    // damage: apply_dirty fed update's own verdicts stays in step with it
    for (int threshold : {0, 15}) {
      DamageTracker a, b;
      a.reset(w, h);
      b.reset(w, h);
      for (int f = 0; f < 6; ++f) {
        if (f % 3) {
          size_t i = rnd() % frame.size();
          frame[i] = static_cast<uint8_t>(frame[i] + 16 + rnd() % 64);
        }
        a.update(frame.data(), stride, threshold, 3);
        if (f == 0) {
          b.apply_dirty(nullptr, 3);
        } else {
          // clean blocks only ever count down, so a block at the full
          // duration is one update() found dirty
          std::vector<uint8_t> flags(a.ages().size());
          for (size_t i = 0; i < flags.size(); ++i)
            flags[i] = a.ages()[i] == 3;
          b.apply_dirty(flags.data(), 3);
        }
        if (a.ages() != b.ages() ||
            a.consecutive_still_frames() != b.consecutive_still_frames())
          fail("apply_dirty diverged from update");
      }
    }
  }
  std::printf("frontend harness OK\n");
  return 0;
}
