// Slice plan of the HIP H.264 pipeline: how many slices (row segments)
// each MB row is cut into, and how wide the widest one is. Pure
// arithmetic, no HIP, so it is testable without a GPU.
#pragma once

#include <algorithm>

#include "../../hip/h264_gpu_layout.h"   // kMaxSegMbw

namespace hipflux {
namespace h264 {

struct SegPlan {
  int segs;     // slices per MB row
  int widest;   // MBs in every slice but the last, which holds the rest
};

// Latency shaping: the row kernels are serial in the MB chain of one
// slice, and a frame whose rows alone underfill the 256-CU chip is
// LATENCY-bound — so split each row into more slices until there is
// ~one workgroup per CU, as long as chains keep >=20 MBs (slice
// restarts reset intra/MVP context, so ultra-short chains waste bits
// and pipeline warmup). Each extra slice costs a NAL (host assembly +
// ~0.1% bits at 1080p noise). Two regimes, both measured:
//  * latency (rows alone underfill the chip, job_cap > 1): split
//    toward one workgroup per CU but keep total jobs <= 256 so the
//    CAVLC kernel stays in its wide 1024-thread shape (exceeding it
//    fell back to 512 threads and lost 20-40%), chains >= 30 MBs.
//    1080p -> 3 slices of 40 (864 -> 2127 fps with the rest of v25+).
//  * throughput (4K/8K: enough rows to fill the chip): the tail of
//    each wave-round is still chain-latency-bound, so short chains
//    win regardless of CAVLC width — cap chains at ~30 MBs, at most
//    8 slices/row. 4K 513 -> 711 fps (8 slices of 30), 8K 193 -> 205
//    (8 slices of 60; 12 slices measured slightly worse).
// override_segs >= 1 (HIPFLUX_SEGS) replaces the shaping; rows wider than
// kMaxSegMbw are split regardless. The slice count is then re-derived
// from the widest slice, so no request can leave a zero-width trailing
// slice: 5 slices over 16 MBs plan as 4 of 4, and a request above mbw
// degrades to one MB per slice.
// planes > 1 (Hi444 separate colour planes: every MB row is coded once
// per plane, all in the same launches) shapes for mbh * planes concurrent
// rows; planes == 1 is the 4:2:0 plan.
inline SegPlan seg_plan(int mbw, int mbh, int override_segs = 0,
                        int planes = 1) {
  const int min_segs = (mbw + h264gpu::kMaxSegMbw - 1) / h264gpu::kMaxSegMbw;
  int segs;
  if (override_segs >= 1) {
    segs = std::max(min_segs, override_segs);
  } else {
    const int rows = std::max(1, mbh * planes);
    const int fill = (256 + rows - 1) / rows;
    const int chain_cap = std::max(1, mbw / 30);
    const int job_cap = std::max(1, 256 / rows);
    const int shaped = job_cap > 1 ? std::min(std::min(fill, job_cap),
                                              std::min(chain_cap, 8))
                                   : std::min(chain_cap, 8);
    segs = std::max(min_segs, shaped);
  }
  segs = std::max(1, segs);
  const int widest = (mbw + segs - 1) / segs;
  return {(mbw + widest - 1) / std::max(1, widest), widest};
}

}  // namespace h264
}  // namespace hipflux
