// Sanitizer harness for the HEVC CPU encoder in fullcolor (Main 4:4:4):
// odd sizes, QP extremes, split rows, and the host entropy path over the
// GPU level layout (encode_hevc_job_nal). Built with ASan + UBSan; any
// heap error or UB aborts with a nonzero exit.
//
// It also reports the largest slice-segment size per CTU at qp 0 on the
// two worst-case inputs. Those figures size the HIP pipeline's fullcolor
// CABAC output stride (pipeline_hip_hevc.cpp, profiles/NOTES.md).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../cpu/hevc/encoder.h"
#include "../cpu/hevc/gpu_entropy.h"
#include "../hip/hevc_gpu_layout.h"

using namespace hipflux;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<uint32_t>(rng_state);
}

// Sizes of the IDR NALs (type 19) in an Annex-B stream, start code and
// NAL header excluded.
static std::vector<size_t> idr_sizes(const std::vector<uint8_t>& s) {
  std::vector<size_t> starts;
  for (size_t i = 0; i + 4 <= s.size(); ++i)
    if (s[i] == 0 && s[i + 1] == 0 && s[i + 2] == 0 && s[i + 3] == 1)
      starts.push_back(i);
  std::vector<size_t> out;
  for (size_t k = 0; k < starts.size(); ++k) {
    size_t b = starts[k] + 4;
    size_t e = k + 1 < starts.size() ? starts[k + 1] : s.size();
    if (((s[b] >> 1) & 0x3F) == 19) out.push_back(e - b - 2);
  }
  return out;
}

// Largest bytes-per-CTU over the slice segments of one fullcolor frame.
static double max_bytes_per_ctu(int w, int h, int spr, int kind) {
  hevc::StripeEncoder enc(w, h, spr, true);
  std::vector<uint8_t> y(static_cast<size_t>(w) * h), cb(y.size()),
      cr(y.size());
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < w; ++c) {
      size_t i = static_cast<size_t>(r) * w + c;
      if (kind == 0) {   // uniform noise
        y[i] = static_cast<uint8_t>(rnd());
        cb[i] = static_cast<uint8_t>(rnd());
        cr[i] = static_cast<uint8_t>(rnd());
      } else {           // saturated 1-pixel checkerboard, all channels
        y[i] = cb[i] = cr[i] = ((r + c) & 1) ? 255 : 0;
      }
    }
  std::vector<uint8_t> out;
  enc.encode_frame(y.data(), w, cb.data(), cr.data(), w, 0, out);
  const int ctbw = (w + 15) / 16;
  const int per = (ctbw + spr - 1) / spr;
  double worst = 0;
  size_t k = 0;
  const std::vector<size_t> sizes = idr_sizes(out);
  for (int row = 0; row < (h + 15) / 16; ++row)
    for (int s0 = 0; s0 < ctbw; s0 += per, ++k) {
      int n = std::min(per, ctbw - s0);
      if (k < sizes.size())
        worst = std::max(worst, static_cast<double>(sizes[k]) / n);
    }
  return worst;
}

int main() {
  // fullcolor encodes: single CTU, odd sizes, split rows, QP extremes
  const int sizes[][3] = {{16, 16, 1}, {48, 32, 1}, {321, 149, 1},
                          {33, 17, 2}, {1296, 16, 2}};
  for (auto& whs : sizes) {
    int w = whs[0], h = whs[1];
    hevc::StripeEncoder enc(w, h, whs[2], true);
    if (enc.recon_cpitch() != enc.recon_ypitch()) return 1;
    std::vector<uint8_t> y(static_cast<size_t>(w) * h), cb(y.size()),
        cr(y.size());
    for (int f = 0; f < 4; ++f) {
      for (auto& v : y) v = static_cast<uint8_t>(rnd());
      for (auto& v : cb) v = static_cast<uint8_t>(f == 3 ? 77 : rnd());
      for (auto& v : cr) v = static_cast<uint8_t>(rnd());
      std::vector<uint8_t> out;
      int qp = f == 0 ? 0 : f == 1 ? 51 : 10 + (rnd() % 35);
      enc.encode_frame(y.data(), w, cb.data(), cr.data(), w, qp, out);
      if (out.empty()) {
        std::fprintf(stderr, "empty stream at %dx%d f%d\n", w, h, f);
        return 2;
      }
    }
  }
  // host entropy over the 4:4:4 GPU level layout: random levels with
  // random cbf masks kept consistent with their content
  {
    const int ctbw = 5;
    std::vector<int16_t> levels(
        static_cast<size_t>(ctbw) * hevcgpu::kHevcLevelsPerCtu444, 0);
    std::vector<int> meta(static_cast<size_t>(ctbw) * hevcgpu::kHevcMetaPerCtu);
    const int modes[4] = {0, 1, 10, 26};
    for (int t = 0; t < 20; ++t) {
      for (int c = 0; c < ctbw; ++c) {
        int cbf = 0;
        for (int pl = 0; pl < 3; ++pl) {
          int16_t* lv = &levels[(static_cast<size_t>(c) * 3 + pl) * 256];
          bool any = false;
          for (int i = 0; i < 256; ++i) {
            int r = rnd() % (t + 2);
            lv[i] = r ? 0
                      : static_cast<int16_t>(
                            static_cast<int>(rnd() % 65535) - 32767);
            any = any || lv[i];
          }
          if (any) cbf |= 1 << pl;
        }
        meta[c * hevcgpu::kHevcMetaPerCtu] = modes[rnd() & 3];
        meta[c * hevcgpu::kHevcMetaPerCtu + 1] = cbf;
      }
      std::vector<uint8_t> out;
      hevc::write_hevc_stripe_headers(ctbw * 16, 16, ctbw * 16 - 3, 13, out,
                                      true);
      hevc::encode_hevc_job_nal(levels.data(), meta.data(), ctbw, 0, 0, ctbw,
                                rnd() % 52, true, 0, 3, out, true);
      if (out.empty()) return 3;
    }
  }
  // worst-case segment bytes per CTU at qp 0 (fullcolor)
  const char* names[2] = {"noise", "checkerboard"};
  for (int kind = 0; kind < 2; ++kind) {
    double a = max_bytes_per_ctu(1920, 64, 2, kind);    // 60-CTU segments
    double b = max_bytes_per_ctu(3840, 32, 32, kind);   // 8-CTU segments
    double c = max_bytes_per_ctu(512, 32, 32, kind);    // 1-CTU segments
    std::printf("fullcolor qp0 %s: max bytes/CTU %.1f (60-CTU seg) "
                "%.1f (8-CTU seg) %.1f (1-CTU seg)\n",
                names[kind], a, b, c);
  }
  std::puts("hevc444 sanitizer harness ok");
  return 0;
}
