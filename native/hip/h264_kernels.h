#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "h264_gpu_layout.h"

namespace hipflux {
namespace h264gpu {

// 2x2 box average of the sw x sh plane; reads clamp to the rw x rh extent
// that holds valid samples
void launch_downsample2(const uint8_t* src, int spitch, int sw, int sh,
                        int rw, int rh, uint8_t* dst, int dpitch,
                        hipStream_t stream);

void launch_h264_me(const uint8_t* srcY, int ypitch, int w, int h,
                    const uint8_t* refY, const uint8_t* srcY2,
                    const uint8_t* refY2, int ypitch2, int mbw, int n_jobs,
                    const RowJob* d_jobs, int* d_meta, hipStream_t stream);

void launch_h264_rows4(const uint8_t* srcY, const uint8_t* srcCb,
                       const uint8_t* srcCr, int ypitch, int cpitch, int w,
                       int h, const uint8_t* refY, const uint8_t* refCb,
                       const uint8_t* refCr, uint8_t* curY, uint8_t* curCb,
                       uint8_t* curCr, int mbw, int n_jobs,
                       const struct RowJob* d_jobs, int16_t* d_levels,
                       int* d_meta, hipStream_t stream);

void launch_h264_deblock(uint8_t* d_curY, uint8_t* d_curCb,
                         uint8_t* d_curCr, int ypitch, int cpitch, int mbw,
                         int n_jobs, const RowJob* d_jobs,
                         const int16_t* d_levels, const int* d_meta,
                         hipStream_t stream);

// Hi444 separate colour planes: every job is a monochrome slice of plane
// job.plane. src/ref/cur point at plane 0 and the planes lie plane_stride
// bytes apart with one pitch; levels/meta hold the planes back to back
// (job.mb_base). One launch covers all three planes' jobs.
void launch_h264_rows4_mono(const uint8_t* src, const uint8_t* ref,
                            uint8_t* cur, size_t plane_stride, int pitch,
                            int w, int h, int mbw, int n_jobs,
                            const RowJob* d_jobs, int16_t* d_levels,
                            int* d_meta, hipStream_t stream);

void launch_h264_deblock_mono(uint8_t* d_cur, size_t plane_stride, int pitch,
                              int mbw, int n_jobs, const RowJob* d_jobs,
                              const int* d_meta, hipStream_t stream);

void launch_h264_cavlc_mono(const int16_t* d_levels, const int* d_meta,
                            int mbw, int n_jobs, const RowJob* d_jobs,
                            uint32_t* d_stage, int* d_nbits, uint32_t* d_out,
                            int out_stride_words, int* d_out_bits,
                            hipStream_t stream);

void launch_h264_cavlc(const int16_t* d_levels, const int* d_meta, int mbw,
                       int n_jobs, const RowJob* d_jobs, uint32_t* d_stage,
                       int* d_nbits, uint32_t* d_out, int out_stride_words,
                       int* d_out_bits, hipStream_t stream);

}  // namespace h264gpu
}  // namespace hipflux
