// HIP (gfx950) encode pipelines: picks the pipeline for an output mode.
// The pipelines live in pipeline_hip_{jpeg,h264,hevc}.cpp; the owners of
// their streams, events and buffers in hip_host.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <exception>

#include "engine.h"

namespace hipflux {

std::unique_ptr<EncodePipeline> make_hip_jpeg_pipeline(const CaptureSettings&);
std::unique_ptr<EncodePipeline> make_hip_h264_pipeline(const CaptureSettings&);
std::unique_ptr<EncodePipeline> make_hip_hevc_pipeline(const CaptureSettings&);

std::unique_ptr<EncodePipeline> make_hip_pipeline(const CaptureSettings& s) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return nullptr;
  if (s.gpu_id >= n) return nullptr;
  try {
    if (s.output_mode == 0) return make_hip_jpeg_pipeline(s);
    if (s.output_mode == 2) return make_hip_hevc_pipeline(s);
    return make_hip_h264_pipeline(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hipflux: HIP pipeline init failed: %s\n", e.what());
    return nullptr;
  }
}

}  // namespace hipflux
