// CDNA4 (gfx950) H.264 P-frame motion search and mode decision.
//
//  * k_h264_me_mfma: one wave per MB of every scheduled P slice, launched
//    before the row kernel (h264_rows4.hip). It scores integer candidates
//    by SSD on the matrix cores, refines the winner to quarter-pel by SAD,
//    and writes the MB's decision (skip / inter + mv / intra) and its
//    tracking state for the next frame into the two meta words
//    (h264_gpu_layout.h). Rows of IDR slices return at once.
//  * k_downsample2: the 2x2 box filter that builds the quarter-resolution
//    luma pyramid (two applications) the search's acquisition pass reads.
//
// Both are pinned, integer-exact and for every MB, to
// tests/h264_me_mirror.py by tests/test_gpu_h264_me.py.
#include <hip/hip_runtime.h>

#include "h264_gpu_layout.h"
#include "h264_kernels.h"
#include "h264_rows_common.h"

namespace hipflux {
namespace h264gpu {

// ---------------------------------------------------------------------------
// MFMA-int8 full-search motion estimation.
//
// Scores ALL candidates of a ±8 even-step grid (9x9 = 81) by SSD using the
// matrix cores:  SSD_n = S2 - 2*X_n + R2_n  with pixels centered to int8
// (p-128; SSD is shift-invariant). Per 16-candidate group:
//   X_n  : 4x mfma_i32_16x16x64_i8, A rows = broadcast src chunk (64 px),
//          B cols = candidate chunks       -> D[0][n] = sum(a*b_n)
//   R2_n : 4x mfma with A = B              -> diag D[n][n] = sum(b_n^2)
// One wave per MB. The final skip/inter decision uses the winner's SAD so
// thresholds stay identical to the CPU reference encoder.
using i32x4 = __attribute__((__vector_size__(16))) int;

__global__ void __launch_bounds__(64) k_h264_me_mfma(
    const uint8_t* __restrict__ srcY, int ypitch, int w, int h,
    const uint8_t* __restrict__ refY, const uint8_t* __restrict__ srcY2,
    const uint8_t* __restrict__ refY2, int ypitch2, int mbw, int seg_max,
    int frame_w_mb16, const RowJob* __restrict__ jobs,
    int* __restrict__ meta) {
  const int job_idx = blockIdx.x / seg_max;
  const RowJob job = jobs[job_idx];
  const int mbx = job.mbx0 + blockIdx.x % seg_max;
  if (blockIdx.x % seg_max >= job.seg_mbw) return;
  if (job.flags & kJobIdr) return;
  const int lane = threadIdx.x;
  const int mby = job.mb_row;
  const int x0 = mbx * 16, y0 = mby * 16;
  const size_t mb_index = (size_t)mby * mbw + mbx;

  // --- src MB into LDS (+ centered copy for fragments)
  __shared__ int8_t s_a[256];
  {
    int r = lane >> 2, cq = (lane & 3) * 4;
    const uint8_t* s = srcY + (size_t)min(y0 + r, h - 1) * ypitch;
    for (int j = 0; j < 4; ++j)
      s_a[r * 16 + cq + j] =
          (int8_t)((int)s[min(x0 + cq + j, w - 1)] - 128);
  }
  __syncthreads();

  // S2 = sum(a^2)
  int s2 = 0;
  {
    int r = lane >> 2, cq = (lane & 3) * 4;
    for (int j = 0; j < 4; ++j) {
      int v = s_a[r * 16 + cq + j];
      s2 += v * v;
    }
    s2 = wave_sum_i(s2);
  }

  // A fragment per k-chunk-group kg = lane>>4: bytes a_q[kg*16 .. +15]
  // (identical for the 16 lanes of a group -> broadcast rows). Chunk q is
  // selected per MFMA call; precompute all 4 chunks' fragments.
  i32x4 afrag[4];
  {
    int kg = lane >> 4;
    for (int q = 0; q < 4; ++q) {
      // chunk q = MB rows 4q..4q+3; k = r*16+c (r<4). bytes kg*16..+15 of
      // the chunk = row kg of the chunk.
      const int8_t* p = &s_a[(4 * q + kg) * 16];
      int words[4];
      for (int t = 0; t < 4; ++t)
        words[t] = (uint8_t)p[4 * t] | ((uint8_t)p[4 * t + 1] << 8) |
                   ((uint8_t)p[4 * t + 2] << 16) |
                   ((uint8_t)p[4 * t + 3] << 24);
      afrag[q] = i32x4{words[0], words[1], words[2], words[3]};
    }
  }

  // candidate grids: 81 candidates (9x9) in 6 groups of up to 16, scored
  // by MFMA SSD around an arbitrary center and step
  const int NC = 81;
  int best_score = INT_MAX, best_mvx = 0, best_mvy = 0;
  const int col = lane & 15, kg = lane >> 4;

  auto score_grid = [&](int cx0, int cy0, int step) {
    for (int g0 = 0; g0 < NC; g0 += 16) {
      int cand = g0 + col;
      int mx = 0, my = 0;
      bool valid = cand < NC;
      if (valid) {
        mx = cx0 + ((cand % 9) - 4) * step;
        my = cy0 + ((cand / 9) - 4) * step;
        if (x0 + mx < 0 || x0 + mx + 16 > frame_w_mb16 ||
            y0 + my < job.stripe_y0 || y0 + my + 16 > job.stripe_y1)
          valid = false;
      }
      i32x4 cross = {0, 0, 0, 0};
      i32x4 norm = {0, 0, 0, 0};
      for (int q = 0; q < 4; ++q) {
        // B fragment: lane holds B[k = kg*16 + j][col] = candidate col's
        // chunk-q byte (row kg of chunk, cols 0..15 -> j)
        int8_t bb[16];
        if (valid) {
          const uint8_t* rp =
              refY + (size_t)(y0 + my + 4 * q + kg) * ypitch + x0 + mx;
          for (int j = 0; j < 16; ++j) bb[j] = (int8_t)((int)rp[j] - 128);
        } else {
          for (int j = 0; j < 16; ++j) bb[j] = 0;
        }
        int words[4];
        for (int t = 0; t < 4; ++t)
          words[t] = (uint8_t)bb[4 * t] | ((uint8_t)bb[4 * t + 1] << 8) |
                     ((uint8_t)bb[4 * t + 2] << 16) |
                     ((uint8_t)bb[4 * t + 3] << 24);
        i32x4 bfrag = i32x4{words[0], words[1], words[2], words[3]};
        cross = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[q], bfrag,
                                                      cross, 0, 0, 0);
        norm = __builtin_amdgcn_mfma_i32_16x16x64_i8(bfrag, bfrag, norm,
                                                     0, 0, 0);
      }
      // D mapping (16x16): X_n in row 0 (lane n, acc 0); R2_n on the
      // diagonal (lane ((n>>2)<<4)|n, acc n&3). Reduce on lane 0.
      for (int n_base = 0; n_base < 16; ++n_base) {
        int xl = __shfl(cross[0], n_base);
        int diag_lane = ((n_base >> 2) << 4) | n_base;
        int rl;
        switch (n_base & 3) {
          case 0: rl = __shfl(norm[0], diag_lane); break;
          case 1: rl = __shfl(norm[1], diag_lane); break;
          case 2: rl = __shfl(norm[2], diag_lane); break;
          default: rl = __shfl(norm[3], diag_lane); break;
        }
        int cand2 = g0 + n_base;
        if (cand2 < NC && lane == 0) {
          int mx2 = cx0 + ((cand2 % 9) - 4) * step;
          int my2 = cy0 + ((cand2 / 9) - 4) * step;
          bool v2 = !(x0 + mx2 < 0 || x0 + mx2 + 16 > frame_w_mb16 ||
                      y0 + my2 < job.stripe_y0 ||
                      y0 + my2 + 16 > job.stripe_y1);
          if (v2) {
            int ssd = s2 - 2 * xl + rl;
            // small center bias keeps MVs compact on flat content
            int score = ssd + (abs(mx2) + abs(my2)) * 4;
            if (score < best_score) {
              best_score = score;
              best_mvx = mx2;
              best_mvy = my2;
            }
          }
        }
      }
    }
  };

  // pass 0: previous-frame tracking state (meta still holds last
  // frame's values). An MB whose LAST frame was hopeless (unmatchable
  // at any candidate — noise) skips every search pass except a
  // 1-in-8-frame probe; the sad(0,0) skip/inter test below still runs
  // every frame, so content that settles becomes P_Skip immediately —
  // and going skip clears the hopeless bit, resuming full search.
  const int pm0 = meta[mb_index * kMetaPerMb + 0];
  const int pm1 = meta[mb_index * kMetaPerMb + 1];
  const bool prev_hopeless = (pm0 >> 22) & 1;
  if (!(prev_hopeless && (job.frame_num & 7) != 0)) {
  // pass 1: fine grid at (0,0)
  score_grid(0, 0, 2);
  // pass 2: fine grid at the previous frame's MV/hint for this MB (meta
  // still holds last frame's values here) — tracks sustained motion
  // beyond +-8 even across intra fallbacks
  {
    int pvx = 0, pvy = 0;
    if ((pm0 & 3) == kInter) {
      pvx = ((int)(short)(pm1 & 0xFFFF)) >> 2;
      pvy = (pm1 >> 16) >> 2;
    } else {
      pvx = ((pm0 >> 8) & 127) - 64;    // intra/skip hint (bits 8..21)
      pvy = ((pm0 >> 15) & 127) - 64;
    }
    pvx = max(-48, min(48, pvx));
    pvy = max(-48, min(48, pvy));
    if ((pvx | pvy) != 0 && (abs(pvx) > 2 || abs(pvy) > 2))
      score_grid(pvx, pvy, 2);
  }
  // pass 3: pyramid acquisition when nothing fits yet — first frame of
  // fast new motion. A +-12 step-1 SAD search on the QUARTER-res luma
  // pyramid covers +-48 at full res with correlation intact at that
  // scale; the winner seeds a fine full-res grid.
  if (__shfl(best_score, 0) > 256 * 180) {
    // this MB at quarter res: 4x4 proxy block
    const int qx0 = x0 >> 2, qy0 = y0 >> 2;
    const int qw = frame_w_mb16 >> 2;
    // proxy rows and columns clamp to the last quarter-res sample whose
    // 4x4 footprint lies inside the picture (sample 0 for a picture under
    // 4 rows or columns; the pyramid itself is built from clamped reads)
    const int qr_max = max(0, (h >> 2) - 1), qc_max = max(0, (w >> 2) - 1);
    const int qs_y0 = job.stripe_y0 >> 2, qs_y1 = job.stripe_y1 >> 2;
    int px[4];
    {
      int rr = lane & 3;
      const uint8_t* sr = srcY2 + (size_t)min(qy0 + rr, qr_max) * ypitch2;
      for (int j = 0; j < 4; ++j)
        px[j] = sr[min(qx0 + j, qc_max)];
    }
    int bs = INT_MAX, bmx2 = 0, bmy2 = 0;
    // 25x25 candidates, distributed over lanes (lane covers cands with
    // index % 16 == lane>>2 pattern via strided loop)
    for (int ci = lane >> 2; ci < 625; ci += 16) {
      int mx = (ci % 25) - 12, my = (ci / 25) - 12;
      if (qx0 + mx < 0 || qx0 + mx + 4 > qw || qy0 + my < qs_y0 ||
          qy0 + my + 4 > qs_y1)
        continue;
      const uint8_t* rp =
          refY2 + (size_t)(qy0 + my + (lane & 3)) * ypitch2 + qx0 + mx;
      int sad = abs(px[0] - rp[0]) + abs(px[1] - rp[1]) +
                abs(px[2] - rp[2]) + abs(px[3] - rp[3]);
      // sum the 4 row-partials within the 4-lane group
      sad += __shfl_xor(sad, 1);
      sad += __shfl_xor(sad, 2);
      if (sad < bs) {
        bs = sad;
        bmx2 = mx;
        bmy2 = my;
      }
    }
    // wave-reduce the best candidate
    for (int d = 4; d < 64; d <<= 1) {
      int os = __shfl_xor(bs, d);
      int ox = __shfl_xor(bmx2, d);
      int oy = __shfl_xor(bmy2, d);
      if (os < bs || (os == bs && (oy < bmy2 || (oy == bmy2 && ox < bmx2)))) {
        bs = os;
        bmx2 = ox;
        bmy2 = oy;
      }
    }
    // fine full-res verification grid at the pyramid seed
    if (bs < INT_MAX) score_grid(bmx2 * 4, bmy2 * 4, 2);
  }
  }  // end non-hopeless search passes

  best_score = __shfl(best_score, 0);
  best_mvx = __shfl(best_mvx, 0);
  best_mvy = __shfl(best_mvy, 0);

  // SAD of (0,0) and of the SSD winner -> same thresholds as CPU encoder
  const int r = lane >> 2, cq = (lane & 3) * 4;
  int sp[4];
  {
    const uint8_t* s = srcY + (size_t)min(y0 + r, h - 1) * ypitch;
    for (int j = 0; j < 4; ++j) sp[j] = s[min(x0 + cq + j, w - 1)];
  }
  auto sad_at = [&](int mx, int my) -> int {
    const uint8_t* rp = refY + (size_t)(y0 + my + r) * ypitch + x0 + mx + cq;
    int s = abs(sp[0] - rp[0]) + abs(sp[1] - rp[1]) + abs(sp[2] - rp[2]) +
            abs(sp[3] - rp[3]);
    return wave_sum_i(s);
  };
  // interpolated SAD at a quarter-pel mv (half-pel grid)
  auto sad_q = [&](int qx, int qy) -> int {
    int ixq = qx >> 2, iyq = qy >> 2, fxq = qx & 3, fyq = qy & 3;
    int s = 0;
    for (int j = 0; j < 4; ++j)
      s += abs(sp[j] - luma_interp(refY, ypitch, x0 + ixq + cq + j,
                                   y0 + iyq + r, fxq, fyq));
    return wave_sum_i(s);
  };
  auto window_ok = [&](int qx, int qy) -> bool {
    int ixq = qx >> 2, iyq = qy >> 2;
    // +20: quarter positions may also read the x+1 / y+1 half sample
    return x0 + ixq - 2 >= 0 && x0 + ixq + 20 <= frame_w_mb16 &&
           y0 + iyq - 2 >= job.stripe_y0 && y0 + iyq + 20 <= job.stripe_y1;
  };

  const int qp = job.qp;
  const int skip_thresh = 48 << (qp / 6);
  const int inter_thresh = 6 * skip_thresh;
  int sad0 = sad_at(0, 0);
  int mode, oqx = 0, oqy = 0;
  int hintx = 0, hinty = 0;
  if (sad0 <= skip_thresh) {
    mode = kSkip;
  } else {
    int best_sad = (best_mvx || best_mvy) ? sad_at(best_mvx, best_mvy)
                                          : sad0;
    // refine the even-grid SSD winner: integer +-1 ring, then half-pel
    // (skipped when the MB is headed to intra regardless)
    int bqx = best_mvx * 4, bqy = best_mvy * 4;
    static const int pat[8][2] = {{-1, 0}, {1, 0},  {0, -1}, {0, 1},
                                  {-1, -1}, {1, 1}, {-1, 1}, {1, -1}};
    if (best_sad <= 2 * inter_thresh) {
      for (int iter = 0; iter < 8; ++iter) {
        int cqx = bqx, cqy = bqy;
        bool improved = false;
        for (int pi = 0; pi < 8; ++pi) {
          int qx = cqx + 4 * pat[pi][0], qy = cqy + 4 * pat[pi][1];
          if (!window_ok(qx, qy)) continue;
          int s = sad_at(qx >> 2, qy >> 2);
          if (s < best_sad) {
            best_sad = s;
            bqx = qx;
            bqy = qy;
            improved = true;
          }
        }
        if (!improved) break;
      }
      for (int step = 2; step >= 1; --step) {
        int cqx2 = bqx, cqy2 = bqy;
        for (int pi = 0; pi < 8; ++pi) {
          int qx = cqx2 + step * pat[pi][0], qy = cqy2 + step * pat[pi][1];
          if (!window_ok(qx, qy)) continue;
          int s = sad_q(qx, qy);
          if (s < best_sad) {
            best_sad = s;
            bqx = qx;
            bqy = qy;
          }
        }
      }
    }
    if (best_sad <= inter_thresh) {
      mode = kInter;   // mv may be (0,0): residuals carry the change
      oqx = bqx;
      oqy = bqy;
    } else {
      mode = kIntra;
    }
    hintx = bqx >> 2;
    hinty = bqy >> 2;
  }
  bool hopeless = mode == kIntra && __shfl(best_score, 0) > 256 * 1200;
  if (hopeless) hintx = hinty = 0;
  if (lane == 0) {
    // best-found integer mv persists as a tracking hint even when the MB
    // goes intra; the luma row wave preserves these bits on its M[0]
    // rewrite
    int hx = max(-48, min(48, hintx)) + 64;
    int hy = max(-48, min(48, hinty)) + 64;
    meta[mb_index * kMetaPerMb + 0] =
        mode | (hx << 8) | (hy << 15) | ((hopeless ? 1 : 0) << 22);
    meta[mb_index * kMetaPerMb + 1] =
        (oqx & 0xFFFF) | (int)((unsigned)oqy << 16);
  }
}

// ---------------------------------------------------------------------------
// host launchers
void launch_h264_me(const uint8_t* srcY, int ypitch, int w, int h,
                    const uint8_t* refY, const uint8_t* srcY2,
                    const uint8_t* refY2, int ypitch2, int mbw, int n_jobs,
                    const RowJob* d_jobs, int* d_meta, hipStream_t stream) {
  if (n_jobs == 0) return;
  const int seg_max = mbw < kMaxSegMbw ? mbw : kMaxSegMbw;
  hipLaunchKernelGGL(k_h264_me_mfma, dim3(n_jobs * seg_max), dim3(64), 0,
                     stream, srcY, ypitch, w, h, refY, srcY2, refY2, ypitch2,
                     mbw, seg_max, mbw * 16, d_jobs, d_meta);
}

// ---------------------------------------------------------------------------
// 2x2 box downsample (luma pyramid for ME acquisition). One thread per
// output pixel. The source holds valid samples only in [0, rw) x [0, rh);
// reads clamp to that extent, so the output over the whole sw x sh plane
// is the box average of the edge-replicated picture and depends on
// nothing else.
__global__ void k_downsample2(const uint8_t* __restrict__ src, int spitch,
                              int sw, int sh, int rw, int rh,
                              uint8_t* __restrict__ dst, int dpitch) {
  int x = blockIdx.x * blockDim.x + threadIdx.x;
  int y = blockIdx.y * blockDim.y + threadIdx.y;
  int dw = sw >> 1, dh = sh >> 1;
  if (x >= dw || y >= dh) return;
  const int xa = max(0, min(2 * x, rw - 1));
  const int xb = max(0, min(2 * x + 1, rw - 1));
  const uint8_t* r0 = src + (size_t)max(0, min(2 * y, rh - 1)) * spitch;
  const uint8_t* r1 = src + (size_t)max(0, min(2 * y + 1, rh - 1)) * spitch;
  dst[(size_t)y * dpitch + x] =
      (uint8_t)((r0[xa] + r0[xb] + r1[xa] + r1[xb] + 2) >> 2);
}

void launch_downsample2(const uint8_t* src, int spitch, int sw, int sh,
                        int rw, int rh, uint8_t* dst, int dpitch,
                        hipStream_t stream) {
  dim3 b(16, 16);
  dim3 g(((sw >> 1) + 15) / 16, ((sh >> 1) + 15) / 16);
  hipLaunchKernelGGL(k_downsample2, g, b, 0, stream, src, spitch, sw, sh,
                     rw, rh, dst, dpitch);
}

}  // namespace h264gpu
}  // namespace hipflux
