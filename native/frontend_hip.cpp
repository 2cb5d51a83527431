// Host owner of the device capture front end (kernels: hip/frontend.hip).
//
// One stream carries a frame's whole chain: H2D of the native frame ->
// watermark -> cursor -> downscale -> block diff -> flag D2H, then one
// synchronise. Scaled frames ping-pong between two buffers: the one not
// written this frame is the previous frame the diff reads, so nothing is
// copied to keep a "previous" image.
//
// Hand-off invariant: a pipeline given Result::dev copies it into its own
// frame buffer on its upload stream, and every HIP pipeline waits for that
// copy before encode_frame() returns (depth 1 collects the whole frame,
// depth 2 waits on the frame's upload event) — the same wait that lets a
// capture source reuse its host buffer. process() is only called after
// encode_frame() returned, and it writes the OTHER buffer anyway, so a
// scaled buffer is never overwritten under a pending copy.
#include "frontend_hip.h"

#include <algorithm>
#include <cstring>

#include "cpu/overlay.h"
#include "cpu/scale.h"
#include "hip/frontend_kernels.h"
#include "hip_host.h"

namespace hipflux {
namespace {

class HipFrontEnd : public GpuFrontEnd {
 public:
  HipFrontEnd(int w, int h, float scale, int scale_div, int gpu_id,
              bool pin_source)
      : dev_(gpu_id), pin_source_(pin_source) {
    scale_ = std::min(1.0f, std::max(0.25f, scale));
    div_ = std::min(4, std::max(1, scale_div));
    mode_ = scale_ < 0.9999f ? kBilinear : div_ > 1 ? kBox : kNone;
    alloc_for(w, h);
  }

  void set_watermark(const uint8_t* bgra, int w, int h) override {
    stream_.sync();
    wm_arena_.release();
    wm_w_ = wm_h_ = 0;
    if (w <= 0 || h <= 0) return;
    const size_t bytes = static_cast<size_t>(w) * h * 4;
    wm_arena_.dev(d_wm_, bytes);
    HIP_CHECK(hipMemcpy(d_wm_, bgra, bytes, hipMemcpyHostToDevice));
    wm_w_ = w;
    wm_h_ = h;
  }

  Result process(const RawFrame& frame, const Overlay& ov, int threshold,
                 bool want_damage) override {
    if (frame.width <= 0 || frame.height <= 0 || frame.stride % 4 ||
        frame.stride < frame.width * 4)
      throw std::runtime_error("GpuFrontEnd: bad frame geometry");
    if (frame.width != w_ || frame.height != h_)
      alloc_for(frame.width, frame.height);
    cur_ ^= 1;
    uint8_t* scaled = d_scaled_[cur_];
    uint8_t* native = mode_ == kNone ? scaled : d_native_;
    const int nstride = w_ * 4;
    const bool timing = !ev_.empty();
    if (timing) HIP_CHECK(hipEventRecord(ev_[0], stream_));

    // ---- upload, tightly packed whatever the source stride
    const size_t row = static_cast<size_t>(nstride);
    const size_t src_bytes =
        static_cast<size_t>(frame.stride) * (h_ - 1) + row;
    if (pin_source_) {
      const uint8_t* src = uploader_.source(frame.data, src_bytes);
      if (frame.stride == nstride)
        HIP_CHECK(hipMemcpyAsync(native, src, src_bytes,
                                 hipMemcpyHostToDevice, stream_));
      else
        HIP_CHECK(hipMemcpy2DAsync(native, row, src, frame.stride, row, h_,
                                   hipMemcpyHostToDevice, stream_));
    } else {
      // the source may be short-lived memory: never register it
      for (int y = 0; y < h_; ++y)
        std::memcpy(h_stage_ + y * row,
                    frame.data + static_cast<size_t>(y) * frame.stride, row);
      HIP_CHECK(hipMemcpyAsync(native, h_stage_, row * h_,
                               hipMemcpyHostToDevice, stream_));
    }
    if (timing) HIP_CHECK(hipEventRecord(ev_[1], stream_));

    // ---- overlays at native size: watermark first, then cursor
    int x0, y0;
    if (wm_w_ > 0 && watermark_origin(ov.wm_location, w_, h_, wm_w_, wm_h_,
                                      ov.wm_frame, x0, y0))
      launch_overlay_watermark(native, w_, h_, nstride, d_wm_, wm_w_, wm_h_,
                               x0, y0, stream_);
    if (ov.cursor && ov.cursor->width > 0 && ov.cursor->height > 0) {
      const CursorImage& c = *ov.cursor;
      upload_cursor(c);
      launch_overlay_cursor(native, w_, h_, nstride, d_cursor_, c.width,
                            c.height, c.x, c.y, stream_);
    }
    if (timing) HIP_CHECK(hipEventRecord(ev_[2], stream_));

    // ---- downscale
    if (mode_ == kBilinear)
      launch_bilinear_downscale(native, nstride, w_, h_, d_xtab_, d_ytab_,
                                scaled, ow_, oh_, ow_ * 4, stream_);
    else if (mode_ == kBox)
      launch_box_downscale(native, nstride, div_, scaled, ow_, oh_, ow_ * 4,
                           stream_);
    if (timing) HIP_CHECK(hipEventRecord(ev_[3], stream_));

    // ---- block diff against the other buffer, flags to pinned memory
    Result r;
    r.dev = scaled;
    r.width = ow_;
    r.height = oh_;
    r.stride = ow_ * 4;
    r.bx = bx_;
    r.by = by_;
    if (want_damage && have_prev_) {
      launch_damage_flags(scaled, d_scaled_[cur_ ^ 1], ow_, oh_, ow_ * 4,
                          threshold, d_flags_, bx_, by_, stream_);
      HIP_CHECK(hipMemcpyAsync(h_flags_, d_flags_,
                               static_cast<size_t>(bx_) * by_,
                               hipMemcpyDeviceToHost, stream_));
      r.flags = h_flags_;
    }
    if (timing) HIP_CHECK(hipEventRecord(ev_[4], stream_));
    HIP_CHECK(hipGetLastError());
    stream_.sync();
    have_prev_ = true;
    if (timing) {
      float* ms[4] = {&stage_ms_.h2d, &stage_ms_.overlay, &stage_ms_.scale,
                      &stage_ms_.damage};
      for (int i = 0; i < 4; ++i)
        HIP_CHECK(hipEventElapsedTime(ms[i], ev_[i], ev_[i + 1]));
    }
    return r;
  }

  void reset_damage() override { have_prev_ = false; }

  void set_timing(bool on) override {
    stream_.sync();
    ev_.clear();
    if (on)
      for (int i = 0; i < 5; ++i) ev_.emplace_back(hipEventDefault);
  }
  StageMs last_stage_ms() const override { return stage_ms_; }

  void download(std::vector<uint8_t>& out) override {
    out.resize(static_cast<size_t>(ow_) * oh_ * 4);
    stream_.sync();
    HIP_CHECK(hipMemcpy(out.data(), d_scaled_[cur_], out.size(),
                        hipMemcpyDeviceToHost));
  }

 private:
  enum Mode { kNone, kBilinear, kBox };

  void alloc_for(int w, int h) {
    stream_.sync();
    arena_.release();
    w_ = h_ = 0;   // until everything below succeeded: a throw retries
    have_prev_ = false;
    cur_ = 0;
    int ow = w, oh = h;
    if (mode_ == kBilinear) {
      ow = bilinear_out_size(w, scale_);
      oh = bilinear_out_size(h, scale_);
    } else if (mode_ == kBox) {
      ow = w / div_;
      oh = h / div_;
    }
    if (ow <= 0 || oh <= 0)
      throw std::runtime_error("GpuFrontEnd: frame smaller than scale_div");
    const size_t native_bytes = static_cast<size_t>(w) * h * 4;
    const size_t scaled_bytes = static_cast<size_t>(ow) * oh * 4;
    for (int i = 0; i < 2; ++i) arena_.dev(d_scaled_[i], scaled_bytes);
    if (mode_ != kNone) arena_.dev(d_native_, native_bytes);
    if (!pin_source_) arena_.pinned(h_stage_, native_bytes);
    if (mode_ == kBilinear) {
      // the host's own sample tables, packed (index << 8) | weight
      std::vector<int> idx, wt;
      std::vector<uint32_t> tab(ow + oh);
      bilinear_axis_table(w, ow, idx, wt);
      for (int i = 0; i < ow; ++i) tab[i] = (idx[i] << 8) | wt[i];
      bilinear_axis_table(h, oh, idx, wt);
      for (int i = 0; i < oh; ++i) tab[ow + i] = (idx[i] << 8) | wt[i];
      arena_.dev(d_xtab_, tab.size());
      d_ytab_ = d_xtab_ + ow;
      HIP_CHECK(hipMemcpy(d_xtab_, tab.data(), tab.size() * 4,
                          hipMemcpyHostToDevice));
    }
    bx_ = (ow + 15) / 16;
    by_ = (oh + 15) / 16;
    arena_.dev(d_flags_, static_cast<size_t>(bx_) * by_);
    arena_.pinned(h_flags_, static_cast<size_t>(bx_) * by_);
    ow_ = ow;
    oh_ = oh;
    w_ = w;
    h_ = h;
  }

  // Re-upload only when the shape changed. cursor_host_ is the copy's
  // source and stays put until the next change, which comes after a
  // stream sync (process() ends with one).
  void upload_cursor(const CursorImage& c) {
    const size_t n = static_cast<size_t>(c.width) * c.height;
    if (c.argb.size() < n)
      throw std::runtime_error("GpuFrontEnd: cursor image too small");
    if (have_cursor_ && c.serial == cursor_serial_ && c.width == cursor_w_ &&
        c.height == cursor_h_)
      return;
    if (n > cursor_cap_) {
      cursor_arena_.release();
      cursor_cap_ = 0;
      cursor_arena_.dev(d_cursor_, n);
      cursor_cap_ = n;
    }
    cursor_host_.assign(c.argb.begin(), c.argb.begin() + n);
    HIP_CHECK(hipMemcpyAsync(d_cursor_, cursor_host_.data(), n * 4,
                             hipMemcpyHostToDevice, stream_));
    cursor_serial_ = c.serial;
    cursor_w_ = c.width;
    cursor_h_ = c.height;
    have_cursor_ = true;
  }

  UseDevice dev_;
  Arena wm_arena_, cursor_arena_;
  Arena arena_;   // everything sized by the resolution
  FrameUploader uploader_;
  Stream stream_;
  std::vector<Event> ev_;   // stage timing, empty = off
  StageMs stage_ms_;
  bool pin_source_;
  Mode mode_ = kNone;
  float scale_ = 1.0f;
  int div_ = 1;
  int w_ = 0, h_ = 0, ow_ = 0, oh_ = 0, bx_ = 0, by_ = 0;
  int cur_ = 0;
  bool have_prev_ = false;
  uint8_t* d_native_ = nullptr;
  uint8_t* d_scaled_[2] = {nullptr, nullptr};
  uint8_t* h_stage_ = nullptr;
  uint32_t* d_xtab_ = nullptr;
  uint32_t* d_ytab_ = nullptr;   // inside d_xtab_'s allocation
  uint8_t* d_flags_ = nullptr;
  uint8_t* h_flags_ = nullptr;
  uint8_t* d_wm_ = nullptr;
  int wm_w_ = 0, wm_h_ = 0;
  uint32_t* d_cursor_ = nullptr;
  size_t cursor_cap_ = 0;
  std::vector<uint32_t> cursor_host_;
  uint64_t cursor_serial_ = 0;
  int cursor_w_ = 0, cursor_h_ = 0;
  bool have_cursor_ = false;
};

}  // namespace

std::unique_ptr<GpuFrontEnd> make_gpu_frontend(int width, int height,
                                               float scale, int scale_div,
                                               int gpu_id, bool pin_source) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    throw std::runtime_error("GpuFrontEnd: no HIP device");
  if (gpu_id >= n) throw std::runtime_error("GpuFrontEnd: no such HIP device");
  return std::make_unique<HipFrontEnd>(width, height, scale, scale_div,
                                       gpu_id, pin_source);
}

}  // namespace hipflux
