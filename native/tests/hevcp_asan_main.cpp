// Sanitizer harness for HEVC P pictures on host code: the CPU encoder
// with `inter` (IDR, P, P... chains) and the host entropy path over the
// GPU level/meta layout with P jobs (encode_hevc_job_nal), through the
// static, half-and-half and POC-wrap cases. Built with ASan + UBSan; any
// heap error or UB aborts with a nonzero exit.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

struct Yuv {
  int w, h;
  std::vector<uint8_t> y, cb, cr;
  Yuv(int w_, int h_)
      : w(w_), h(h_), y(static_cast<size_t>(w_) * h_),
        cb(static_cast<size_t>((w_ + 1) / 2) * ((h_ + 1) / 2)),
        cr(cb.size()) {}
  void noise(int x0) {   // columns >= x0 (luma) become new noise
    for (int r = 0; r < h; ++r)
      for (int c = x0; c < w; ++c) y[static_cast<size_t>(r) * w + c] = rnd();
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    for (int r = 0; r < ch; ++r)
      for (int c = x0 / 2; c < cw; ++c) {
        cb[static_cast<size_t>(r) * cw + c] = rnd();
        cr[static_cast<size_t>(r) * cw + c] = rnd();
      }
  }
};

// NAL types of an Annex-B stream, in order.
static std::vector<int> nal_types(const std::vector<uint8_t>& s) {
  std::vector<int> t;
  for (size_t i = 0; i + 5 <= s.size(); ++i)
    if (s[i] == 0 && s[i + 1] == 0 && s[i + 2] == 0 && s[i + 3] == 1)
      t.push_back((s[i + 4] >> 1) & 0x3F);
  return t;
}

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "hevcp harness: %s\n", what);
    std::exit(1);
  }
}

static std::vector<uint8_t> encode(hevc::StripeEncoder& e, const Yuv& f,
                                   int qp, bool* idr, bool force = false) {
  std::vector<uint8_t> out;
  hevc::EncodeStats st;
  e.encode_frame(f.y.data(), f.w, f.cb.data(), f.cr.data(), (f.w + 1) / 2, qp,
                 out, &st, force);
  *idr = st.idr;
  return out;
}

int main() {
  bool idr = false;
  // ---- static: IDR then all-skip P pictures, at odd sizes too
  const int sizes[][2] = {{80, 32}, {161, 27}, {16, 16}};
  for (const auto& sz : sizes)
    for (int spr : {1, 3}) {
      Yuv f(sz[0], sz[1]);
      f.noise(0);
      hevc::StripeEncoder enc(sz[0], sz[1], spr, false, true);
      auto a = encode(enc, f, 26, &idr);
      expect(idr && nal_types(a)[0] == 32, "first picture is an IDR");
      for (int i = 0; i < 2; ++i) {
        auto p = encode(enc, f, 26, &idr);
        expect(!idr, "static picture is P");
        for (int t : nal_types(p)) expect(t == 1, "P stripe holds TRAIL_R only");
        expect(p.size() < a.size(), "static P is smaller than the IDR");
      }
      auto k = encode(enc, f, 26, &idr, true);
      expect(idr && k == a, "force_idr reproduces the first IDR");
    }
  // ---- half-and-half: skip / merge then intra CTUs, QP extremes
  for (int qp : {0, 26, 51}) {
    Yuv f(80, 32);
    f.noise(0);
    hevc::StripeEncoder enc(80, 32, 1, false, true);
    encode(enc, f, qp, &idr);
    f.noise(48);
    auto p = encode(enc, f, qp, &idr);
    expect(!idr && !p.empty(), "half-and-half picture is P");
  }
  // ---- POC wrap: one CTU, 260 pictures
  {
    Yuv f(16, 16);
    f.noise(0);
    hevc::StripeEncoder enc(16, 16, 1, false, true);
    size_t total = 0;
    for (int i = 0; i < 260; ++i) {
      auto p = encode(enc, f, 26, &idr);
      expect(idr == (i == 0), "only picture 0 is an IDR");
      total += p.size();
    }
    expect(total > 0, "wrap chain produced bytes");
  }
  // inter with fullcolor stays all-intra
  {
    Yuv f(32, 16);
    f.cb.assign(f.y.size(), 128);
    f.cr.assign(f.y.size(), 128);
    f.noise(0);
    hevc::StripeEncoder enc(32, 16, 1, true, true);
    std::vector<uint8_t> o1, o2;
    hevc::EncodeStats st;
    enc.encode_frame(f.y.data(), 32, f.cb.data(), f.cr.data(), 32, 30, o1, &st);
    enc.encode_frame(f.y.data(), 32, f.cb.data(), f.cr.data(), 32, 30, o2, &st);
    expect(st.idr && o1 == o2, "fullcolor ignores inter");
  }
  // ---- host entropy over the GPU layout with P jobs: every CTU kind,
  // segments of 1, 2 and 5 CTUs, random sparse levels
  {
    const int ctbw = 5;
    std::vector<int16_t> levels(
        static_cast<size_t>(ctbw) * hevcgpu::kHevcLevelsPerCtu, 0);
    std::vector<int> meta(static_cast<size_t>(ctbw) * hevcgpu::kHevcMetaPerCtu);
    const int modes[4] = {0, 1, 10, 26};
    for (int round = 0; round < 200; ++round) {
      for (int c = 0; c < ctbw; ++c) {
        int16_t* lv = &levels[static_cast<size_t>(c) * hevcgpu::kHevcLevelsPerCtu];
        int cbf = 0;
        for (int i = 0; i < hevcgpu::kHevcLevelsPerCtu; ++i) {
          lv[i] = (rnd() % 7 == 0) ? static_cast<int16_t>(rnd() % 65 - 32) : 0;
        }
        const int drop = rnd() & 7;   // clear some planes entirely
        if (drop & 1) std::fill(lv, lv + 256, 0);
        if (drop & 2) std::fill(lv + 256, lv + 320, 0);
        if (drop & 4) std::fill(lv + 320, lv + 384, 0);
        for (int i = 0; i < 256; ++i) cbf |= lv[i] ? 1 : 0;
        for (int i = 256; i < 320; ++i) cbf |= lv[i] ? 2 : 0;
        for (int i = 320; i < 384; ++i) cbf |= lv[i] ? 4 : 0;
        const int pick = rnd() % 3;
        int mode = modes[rnd() % 4];
        if (pick == 1) mode = cbf ? hevcgpu::kHevcMetaMerge : hevcgpu::kHevcMetaSkip;
        if (pick == 2) mode = hevcgpu::kHevcMetaSkip;
        if (mode == hevcgpu::kHevcMetaSkip) cbf = 0;
        meta[c * 2 + 0] = mode;
        meta[c * 2 + 1] = cbf;
      }
      for (int seg : {1, 2, 5}) {
        std::vector<uint8_t> out;
        hevc::encode_hevc_job_nal(levels.data(), meta.data(), ctbw, 0, 0, seg,
                                  static_cast<int>(rnd() % 52), round & 1,
                                  round & 1 ? 0 : 3, 4, out, false, 1,
                                  round & 255);
        expect(out.size() > 6 && ((out[4] >> 1) & 0x3F) == 1,
               "P job assembles a TRAIL_R NAL");
      }
    }
  }
  std::puts("hevcp sanitizer harness ok");
  return 0;
}
