// Device-resident capture front end for the HIP pipelines: uploads the
// native frame, blends watermark and cursor, downscales and diffs 16x16
// blocks against the previous scaled frame, all on one stream, and hands
// back a device frame plus the block flag map. Bit-exact with the host
// path (cpu/overlay.h, cpu/scale.h, DamageTracker::update).
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "capture.h"
#include "include/hipflux/common.h"

namespace hipflux {

class GpuFrontEnd {
 public:
  // What to blend onto one frame. The watermark image itself is set once
  // with set_watermark(); its origin comes from (location, frame index).
  struct Overlay {
    int wm_location = 0;          // 0 = no watermark this frame
    uint64_t wm_frame = 0;
    const CursorImage* cursor = nullptr;
  };

  struct Result {
    const uint8_t* dev = nullptr;   // scaled BGRX frame, device memory
    int width = 0, height = 0, stride = 0;
    int bx = 0, by = 0;             // 16x16 block grid of the scaled frame
    // bx * by bytes in pinned host memory, nonzero = block changed. Null
    // when everything counts as changed: the first frame after a reset,
    // or damage was not asked for.
    const uint8_t* flags = nullptr;
  };

  // Per-stage device time of the last process() call, from HIP events;
  // filled only while set_timing(true).
  struct StageMs {
    float h2d = 0, overlay = 0, scale = 0, damage = 0;
  };

  virtual ~GpuFrontEnd() = default;
  virtual void set_watermark(const uint8_t* bgra, int w, int h) = 0;
  // Runs the whole chain and synchronises: on return the scaled frame is
  // complete and the caller may reuse frame.data. The returned buffer
  // stays untouched until the second process() call after this one.
  virtual Result process(const RawFrame& frame, const Overlay& ov,
                         int threshold, bool want_damage) = 0;
  // Forget the previous frame: the next one is all dirty.
  virtual void reset_damage() = 0;
  virtual void set_timing(bool on) = 0;
  virtual StageMs last_stage_ms() const = 0;
  // Tightly packed copy of the last scaled frame (tests, tools).
  virtual void download(std::vector<uint8_t>& out) = 0;
};

// scale < 1 selects the fractional bilinear (and wins over scale_div, as
// in the engine); else scale_div in 2..4 the box filter; else no scaling.
// pin_source: frame.data is long-lived (a capture buffer) and is
// page-locked in place for the upload; false stages every frame through a
// pinned buffer instead, for callers whose frames are short-lived memory.
// Throws when no usable HIP device exists.
std::unique_ptr<GpuFrontEnd> make_gpu_frontend(int width, int height,
                                               float scale, int scale_div,
                                               int gpu_id,
                                               bool pin_source = true);

}  // namespace hipflux
