// HIP (gfx950) H.264 encode pipeline host side.
// CSC + motion search + per-MB-row intra/inter kernels + deblock + CAVLC on
// the GPU, compacted D2H, NAL assembly on the pool. Each stripe is an
// independent bitstream with its own frame_num / recon region (SURVEY.md
// §5.7 seam). HIPFLUX_CPU_ENTROPY=1 swaps the CAVLC kernel for the host
// packer over D2H levels/meta.
//
// video_fullcolor: Hi444 (profile 244) with separate_colour_plane_flag=1,
// the stream shape of the CPU StripeEncoder(fullcolor=true). Y, Cb and Cr
// are three full-resolution planes laid back to back (one allocation each
// for src/ref/cur, plane_stride_ bytes apart, cpitch_ == ypitch_), every
// plane is coded as a monochrome picture by the mono kernels, and
// levels/meta hold the planes back to back. Jobs run stripe -> plane ->
// row -> segment, so one launch each of rows, deblock and CAVLC covers all
// three planes and each stripe's slices come out plane-major. Motion
// search runs per plane with that plane's pyramids.
#include <cstdio>
#include <cstdlib>

#include "cpu/h264/gpu_entropy.h"
#include "cpu/h264/headers.h"
#include "cpu/h264/seg_plan.h"
#include "engine.h"
#include "hip/h264_kernels.h"
#include "hip/jpeg_kernels.h"       // launch_bgrx_to_planes
#include "hip_host.h"
#include "thread_pool.h"

namespace hipflux {
namespace {

class HipH264Pipeline : public EncodePipeline {
 public:
  explicit HipH264Pipeline(const CaptureSettings& s)
      : settings_(s), pool_(encode_pool_threads()), dev_(s.gpu_id) {
    stripe_h_ = std::max(16, s.stripe_height & ~15);
    alloc_for(s.capture_width, s.capture_height);
  }

  // ---- frame pipeline -----------------------------------------------------
  // submit_frame enqueues one frame's full GPU sequence (upload -> CSC ->
  // pyramid -> ME -> rows -> CAVLC -> compacted D2H -> ref refresh) with
  // NO sync; collect_pending waits on the frame's completion event and
  // does the host-side bitstream assembly + emission. Depth 1 runs them
  // back to back (today's latency behavior, bit-identical); depth 2 keeps
  // one frame in flight so host assembly of frame N overlaps the GPU
  // compute of frame N+1 (x264-style frame pipelining; throughput mode).
  struct Out {
    std::vector<uint8_t> header;            // SPS/PPS on IDR
    std::vector<std::vector<uint8_t>> rows;   // slices, plane-major
    int plane_slices = 0;                      // slices per colour plane
    std::vector<uint8_t> bytes;
    h264::GpuStripeParams p{};
    int y0 = 0, h = 0;
    bool idr = false;
  };
  struct Pending {
    bool active = false;
    int par = 0;
    int n_jobs = 0;
    int copy_words = 0;    // the D2H cap this frame was submitted with
    double ts_ms = 0;      // capture timestamp of this frame
    uint32_t frame_id = 0;
    std::vector<Out> outs;
    std::vector<std::pair<int, int>> job_map;
  };

  Pending submit_frame(const RawFrame& frame, const FrameContext& ctx) {
    if (frame.width != w_ || frame.height != h_)
      alloc_for(frame.width, frame.height);
    const int par = parity_;
    const int qp = std::min(51, std::max(0, ctx.crf));

    // the ~8 MB BGRX upload rides its own stream so the SDMA engine
    // overlaps it with the previous frame's kernels (measured ~120 us
    // serialized on the compute stream); the compute stream's CSC waits
    // on the copy via event
    const size_t frame_bytes = static_cast<size_t>(frame.stride) * frame.height;
    if (frame.dev)   // front-end frame: already complete on the device
      HIP_CHECK(hipMemcpyAsync(d_frame_[par], frame.dev, frame_bytes,
                               hipMemcpyDeviceToDevice, up_stream_));
    else
      HIP_CHECK(hipMemcpyAsync(d_frame_[par],
                               uploader_.source(frame.data, frame_bytes),
                               frame_bytes, hipMemcpyHostToDevice,
                               up_stream_));
    // the caller may reuse its frame buffer once this event completes
    HIP_CHECK(hipEventRecord(ev_h2d_[par], up_stream_));
    // the whole produce chain (CSC -> ME -> rows) rides rows_stream_ so
    // it overlaps the PREVIOUS frame's entropy kernel + D2H on stream_
    HIP_CHECK(hipStreamWaitEvent(rows_stream_, ev_h2d_[par], 0));
    launch_bgrx_to_planes(d_frame_[par], w_, h_, frame.stride / 4, d_srcY_,
                          d_srcCb_, d_srcCr_, ypitch_, cpitch_, fc_,
                          rows_stream_);

    // build row jobs for scheduled stripes (stripe stream state — IDR,
    // frame_num, idr_pic_id — resolves here so the GPU entropy kernel gets
    // final slice-header fields)
    struct SJob {
      int idx;       // stripe index
      int y0, y1;    // pixel bounds (logical)
      bool idr;
      uint32_t frame_num, idr_pic_id;
    };
    std::vector<SJob> sjobs;
    int n_jobs = 0;
    for (size_t i = 0; i < ctx.stripes.size(); ++i) {
      const auto& st = ctx.stripes[i];
      if (!st.encode) continue;
      auto& state = stripes_[st.y0 / stripe_h_];
      bool idr = ctx.idr || state.need_idr;
      if (idr) {
        state.frame_num = 0;
        ++state.idr_pic_id;
        state.need_idr = false;
      }
      SJob sj{static_cast<int>(st.y0 / stripe_h_), st.y0, st.y1, idr,
              state.frame_num, state.idr_pic_id};
      ++state.frame_num;
      sjobs.push_back(sj);
      int row0 = st.y0 / 16;
      int rows = (std::min(st.y1, mbh_ * 16) - st.y0 + 15) / 16;
      // stripe's padded pixel bounds for ME clamping
      int sy0 = st.y0, sy1 = (row0 + rows) * 16;
      // planes outermost: a stripe's slices come out plane-major
      for (int pl = 0; pl < planes_; ++pl) {
        for (int r = 0; r < rows; ++r) {
          int x = 0;
          for (int sg = 0; sg < segs_; ++sg) {
            int segw = std::min(seg_w0_, mbw_ - x);
            h_jobs_[par][n_jobs].mb_row = row0 + r;
            h_jobs_[par][n_jobs].qp = qp;
            h_jobs_[par][n_jobs].flags =
                (sj.idr ? h264gpu::kJobIdr : 0) |
                (settings_.video_deblock ? h264gpu::kJobDeblock : 0) |
                (fc_ ? h264gpu::kJobMono : 0);
            h_jobs_[par][n_jobs].plane = pl;
            h_jobs_[par][n_jobs].mb_base = pl * mbw_ * mbh_;
            h_jobs_[par][n_jobs].stripe_y0 = sy0;
            h_jobs_[par][n_jobs].stripe_y1 = sy1;
            h_jobs_[par][n_jobs].first_mb = r * mbw_ + x;
            h_jobs_[par][n_jobs].frame_num = static_cast<int>(sj.frame_num);
            h_jobs_[par][n_jobs].idr_pic_id = static_cast<int>(sj.idr_pic_id);
            h_jobs_[par][n_jobs].mbx0 = x;
            h_jobs_[par][n_jobs].seg_mbw = segw;
            x += segw;
            ++n_jobs;
          }
        }
      }
    }
    if (n_jobs == 0) return Pending{};
    parity_ ^= 1;

    // fullcolor: the motion search runs once per plane, so it gets the
    // same jobs again grouped by plane, behind the first n_jobs
    const int me_jobs = n_jobs / planes_;
    if (fc_) {
      int at[3] = {n_jobs, n_jobs + me_jobs, n_jobs + 2 * me_jobs};
      for (int j = 0; j < n_jobs; ++j)
        h_jobs_[par][at[h_jobs_[par][j].plane]++] = h_jobs_[par][j];
    }
    HIP_CHECK(hipMemcpyAsync(d_jobs_[par], h_jobs_[par],
                             sizeof(h264gpu::RowJob) * n_jobs *
                                 (fc_ ? 2 : 1),
                             hipMemcpyHostToDevice, rows_stream_));
    // meta carries cross-frame tracking state (prev MV hints, hopeless
    // bits); seed this parity's buffer from the previous one so the
    // semantics are identical to the single-buffer design even for
    // damage-skipped stripes
    HIP_CHECK(hipMemcpyAsync(d_meta_[par], d_meta_[par ^ 1], meta_bytes_,
                             hipMemcpyDeviceToDevice, rows_stream_));
    // luma pyramid (quarter res) for ME acquisition; fullcolor: each
    // plane searches on its own, with its own pyramids, as the CPU
    // encoder's three plane encoders do
    for (int pl = 0; pl < planes_; ++pl) {
      const uint8_t* src = d_srcY_ + pl * plane_stride_;
      const uint8_t* ref = d_refY_ + pl * plane_stride_;
      uint8_t* src2 = d_srcY2_ + pl * pyr_stride_;
      uint8_t* ref2 = d_refY2_ + pl * pyr_stride_;
      if (!ctx.idr) {
        // the CSC writes only the w_ x h_ picture: the first source level
        // clamps its reads there (edge replication, the rule the full-
        // resolution source reads follow); every other level reads a
        // fully written MB-aligned plane
        const int pw = ypitch_, ph = mbh_ * 16;
        h264gpu::launch_downsample2(src, ypitch_, pw, ph, w_, h_, d_mip1_,
                                    ypitch_ / 2, rows_stream_);
        h264gpu::launch_downsample2(d_mip1_, ypitch_ / 2, pw / 2, ph / 2,
                                    pw / 2, ph / 2, src2, ypitch_ / 4,
                                    rows_stream_);
        h264gpu::launch_downsample2(ref, ypitch_, pw, ph, pw, ph, d_mip1_,
                                    ypitch_ / 2, rows_stream_);
        h264gpu::launch_downsample2(d_mip1_, ypitch_ / 2, pw / 2, ph / 2,
                                    pw / 2, ph / 2, ref2, ypitch_ / 4,
                                    rows_stream_);
      }
      h264gpu::launch_h264_me(
          src, ypitch_, w_, h_, ref, src2, ref2, ypitch_ / 4, mbw_, me_jobs,
          d_jobs_[par] + (fc_ ? n_jobs + pl * me_jobs : 0),
          d_meta_[par] + pl * n_mb_ * h264gpu::kMetaPerMb, rows_stream_);
    }

    // One launch for all rows: the row kernel's cost is per-row LATENCY
    // (all rows run concurrently), so splitting into sequential batches
    // multiplies GPU time (measured: 4 batches regressed 278->155 fps).
    // Entropy overlap is cross-FRAME instead (depth-2 pipelining).
    if (fc_)
      h264gpu::launch_h264_rows4_mono(
          d_srcY_, d_refY_, d_curY_, plane_stride_, ypitch_, w_, h_, mbw_,
          n_jobs, d_jobs_[par], d_levels_[par], d_meta_[par], rows_stream_);
    else
      h264gpu::launch_h264_rows4(
          d_srcY_, d_srcCb_, d_srcCr_, ypitch_, cpitch_, w_, h_, d_refY_,
          d_refCb_, d_refCr_, d_curY_, d_curCb_, d_curCr_, mbw_, n_jobs,
          d_jobs_[par], d_levels_[par], d_meta_[par], rows_stream_);
    if (cpu_entropy_) {
      // the MB rows the jobs span, for the host packer (the same rows of
      // every plane)
      const int row0 = h_jobs_[par][0].mb_row;
      const int rows = h_jobs_[par][n_jobs - 1].mb_row + 1 - row0;
      const size_t lvl_row = static_cast<size_t>(mbw_) * h264gpu::kLevelsPerMb;
      const size_t meta_row = static_cast<size_t>(mbw_) * h264gpu::kMetaPerMb;
      for (int pl = 0; pl < planes_; ++pl) {
        const size_t lo = (static_cast<size_t>(pl) * mbh_ + row0) * lvl_row;
        const size_t mo = (static_cast<size_t>(pl) * mbh_ + row0) * meta_row;
        HIP_CHECK(hipMemcpyAsync(h_levels_ + lo, d_levels_[par] + lo,
                                 rows * lvl_row * sizeof(int16_t),
                                 hipMemcpyDeviceToHost, rows_stream_));
        HIP_CHECK(hipMemcpyAsync(h_meta_ + mo, d_meta_[par] + mo,
                                 rows * meta_row * sizeof(int),
                                 hipMemcpyDeviceToHost, rows_stream_));
      }
    }
    HIP_CHECK(hipEventRecord(ev_rows_[par], rows_stream_));
    // in-loop deblock of the current recon (within-slice edges only;
    // idc=2 is signaled in the slice headers) before it becomes the
    // reference frame. Deblock (reads recon+levels) and CAVLC (reads
    // levels) are independent, so deblock runs on its own stream
    // concurrently with entropy + bitstream D2H; the cur->ref copies
    // below join both streams before the recon becomes the reference.
    if (settings_.video_deblock) {
      HIP_CHECK(hipStreamWaitEvent(db_stream_, ev_rows_[par], 0));
      if (fc_)
        h264gpu::launch_h264_deblock_mono(d_curY_, plane_stride_, ypitch_,
                                          mbw_, n_jobs, d_jobs_[par],
                                          d_meta_[par], db_stream_);
      else
        h264gpu::launch_h264_deblock(d_curY_, d_curCb_, d_curCr_, ypitch_,
                                     cpitch_, mbw_, n_jobs, d_jobs_[par],
                                     d_levels_[par], d_meta_[par],
                                     db_stream_);
      HIP_CHECK(hipEventRecord(ev_db_[par], db_stream_));
    }
    int copy_words = 0;
    if (!cpu_entropy_) {
      // entropy rides stream_ so the NEXT frame's produce chain on
      // rows_stream_ overlaps it (levels/meta are parity-buffered)
      HIP_CHECK(hipStreamWaitEvent(stream_, ev_rows_[par], 0));
      (fc_ ? h264gpu::launch_h264_cavlc_mono : h264gpu::launch_h264_cavlc)(
          d_levels_[par], d_meta_[par], mbw_, n_jobs, d_jobs_[par], d_stage_,
          d_nbits_, d_entout_[par], ent_stride_words_, d_outbits_[par],
          stream_);
      // compaction: copy only ~the used prefix of each row's bitstream
      // (adaptive cap = 2x last frame's max row, full stride first frame;
      // rows that overflow the cap are re-copied exactly in collect)
      copy_words =
          readback_.read(h_entout_[par], d_entout_[par], n_jobs, stream_);
      HIP_CHECK(hipMemcpyAsync(h_outbits_[par], d_outbits_[par],
                               sizeof(int) * n_jobs, hipMemcpyDeviceToHost,
                               stream_));
    }
    // refresh ref from cur for encoded stripes (merge contiguous spans
    // so the all-stripes case is 3 copies, not 3 x n_stripes). They ride
    // rows_stream_ (gated on deblock) so the NEXT frame's rows see the
    // filtered reference without waiting on this frame's entropy.
    if (settings_.video_deblock)
      HIP_CHECK(hipStreamWaitEvent(rows_stream_, ev_db_[par], 0));
    {
      int span_y0 = -1, span_y1 = -1;
      auto flush_span = [&] {
        if (span_y0 < 0) return;
        int rows16 = (std::min(span_y1, mbh_ * 16) - span_y0 + 15) / 16;
        copy_region(d_refY_, d_curY_, ypitch_, span_y0, rows16 * 16);
        if (fc_) {   // three full-size planes
          copy_region(d_refCb_, d_curCb_, ypitch_, span_y0, rows16 * 16);
          copy_region(d_refCr_, d_curCr_, ypitch_, span_y0, rows16 * 16);
        } else {
          copy_region(d_refCb_, d_curCb_, cpitch_, span_y0 / 2, rows16 * 8);
          copy_region(d_refCr_, d_curCr_, cpitch_, span_y0 / 2, rows16 * 8);
        }
        span_y0 = span_y1 = -1;
      };
      for (const auto& sj : sjobs) {
        if (span_y1 == sj.y0) {
          span_y1 = sj.y1;
        } else {
          flush_span();
          span_y0 = sj.y0;
          span_y1 = sj.y1;
        }
      }
      flush_span();
    }
    // the frame is done when its bitstream is on the host; with host
    // entropy, when levels/meta are (rows_stream_ carries those copies)
    HIP_CHECK(hipEventRecord(ev_done_[par],
                             cpu_entropy_ ? rows_stream_ : stream_));

    // host-side output prep (headers, job -> stripe/row mapping)
    Pending pd;
    pd.active = true;
    pd.par = par;
    pd.n_jobs = n_jobs;
    pd.copy_words = copy_words;
    pd.ts_ms = frame.ts_ms;
    pd.frame_id = ctx.frame_id;
    pd.outs.resize(sjobs.size());
    pd.job_map.resize(n_jobs);
    {
      int j = 0;
      for (size_t i = 0; i < sjobs.size(); ++i) {
        const auto& sj = sjobs[i];
        Out& o = pd.outs[i];
        o.y0 = sj.y0;
        o.h = std::min(sj.y1, h_) - sj.y0;
        o.idr = sj.idr;
        h264::GpuStripeParams& p = o.p;
        p.levels = h_levels_;
        p.meta = h_meta_;
        p.mbw = mbw_;
        p.mb_row0 = sj.y0 / 16;
        p.n_mb_rows = (std::min(sj.y1, mbh_ * 16) - sj.y0 + 15) / 16;
        p.width = w_;
        p.height = o.h;
        p.qp = qp;
        p.idr = sj.idr;
        p.deblock = settings_.video_deblock;
        p.frame_num = sj.frame_num;
        p.idr_pic_id = sj.idr_pic_id;
        o.plane_slices = p.n_mb_rows * segs_;
        o.rows.resize(o.plane_slices * planes_);
        if (p.idr) {
          const int smbw = (p.width + 15) / 16;
          if (fc_)
            h264::write_sps_444(o.header, smbw, p.n_mb_rows, p.width,
                                p.height,
                                h264::level_idc_for(smbw, p.n_mb_rows));
          else
            h264::write_sps_nal(o.header, smbw, p.n_mb_rows, p.width,
                                p.height);
          h264::write_pps_nal(o.header);
        }
        for (int r = 0; r < o.plane_slices * planes_; ++r)
          pd.job_map[j++] = {int(i), r};
      }
    }
    return pd;
  }

  void collect_pending(Pending& pd, const Emit& emit) {
    if (!pd.active) return;
    pd.active = false;
    const double c0 = timing_ ? now_us() : 0;
    const int par = pd.par;
    ev_done_[par].sync();
    const double c1 = timing_ ? now_us() : 0;
    if (cpu_entropy_) {
      for (int j = 0; j < pd.n_jobs; ++j) {
        auto [si, sl] = pd.job_map[j];
        auto* dst = &pd.outs[si].rows[sl];
        // the stripe's parameters, pointed at this slice's plane
        h264::GpuStripeParams pp = pd.outs[si].p;
        if (fc_) {
          pp.colour_plane = h_jobs_[par][j].plane;
          pp.mb_base = static_cast<size_t>(h_jobs_[par][j].mb_base);
        }
        const int psl = sl % pd.outs[si].plane_slices;
        int r = psl / segs_;
        int mbx0 = h_jobs_[par][j].mbx0, segw = h_jobs_[par][j].seg_mbw;
        // 4-byte start code on the first slice of each plane
        bool long_sc = psl == 0;
        pool_.submit([pp, r, mbx0, segw, long_sc, dst] {
          h264::encode_seg_nal_from_gpu(pp, r, mbx0, segw, long_sc, *dst);
        });
      }
      pool_.wait_all();
    } else {
      // rare: a row outgrew the adaptive cap; fetch it exactly
      // (d_entout_[par] is parity-preserved until this frame's collect,
      // even with the next frame already submitted)
      readback_.settle(
          h_entout_[par], d_entout_[par], pd.n_jobs, pd.copy_words,
          [&](int j) { return (h_outbits_[par][j] + 31) / 32 + 1; },
          [&](int max_words) {
            return std::min(ent_stride_words_, max_words * 2 + 64);
          });
      // one strided task per worker (not one per NAL: 136 tiny submits
      // per frame serialized on the pool mutex — measured 370 us/frame
      // of wall time for ~40 us of actual assembly work)
      const int nw = std::min(pool_.size(), pd.n_jobs);
      for (int t = 0; t < nw; ++t) {
        pool_.submit([this, &pd, par, t, nw] {
          for (int j = t; j < pd.n_jobs; j += nw) {
            auto [si, sl] = pd.job_map[j];
            h264::assemble_gpu_row_nal(
                h_entout_[par] + (size_t)j * ent_stride_words_,
                h_outbits_[par][j], pd.outs[si].idr,
                sl % pd.outs[si].plane_slices == 0, pd.outs[si].rows[sl]);
          }
        });
      }
      pool_.wait_all();
    }
    const double c2 = timing_ ? now_us() : 0;
    // per-stripe concat on the pool (serial it cost ~90 us/frame)
    if (pd.outs.size() > 1) {
      for (auto& o : pd.outs)
        pool_.submit([&o] {
          o.bytes = std::move(o.header);
          size_t total = o.bytes.size();
          for (auto& r : o.rows) total += r.size();
          o.bytes.reserve(total);
          for (auto& r : o.rows)
            o.bytes.insert(o.bytes.end(), r.begin(), r.end());
        });
      pool_.wait_all();
    } else {
      for (auto& o : pd.outs) {
        o.bytes = std::move(o.header);
        for (auto& r : o.rows)
          o.bytes.insert(o.bytes.end(), r.begin(), r.end());
      }
    }
    for (auto& o : pd.outs) {
      if (o.bytes.empty()) continue;
      EncodedStripe s;
      s.type = StripeType::kH264;
      s.data = o.bytes.data();
      s.size = o.bytes.size();
      s.frame_id = pd.frame_id;
      s.capture_ts_ms = pd.ts_ms;
      s.y = o.y0;
      s.width = w_;
      s.height = o.h;
      s.is_keyframe = o.idr;
      emit(s);
    }
    if (timing_ && !cpu_entropy_) {
      tm_sync_ += c1 - c0;
      tm_asm_ += c2 - c1;
      tm_concat_ += now_us() - c2;
    }
  }

  void encode_frame(const RawFrame& frame, const FrameContext& ctx,
                    const Emit& emit) override {
    const double t0 = timing_ ? now_us() : 0;
    Pending cur = submit_frame(frame, ctx);
    const double t1 = timing_ ? now_us() : 0;
    if (!cur.active) {
      // nothing scheduled this frame; keep the pipe draining
      collect_pending(prev_, emit);
      return;
    }
    if (depth_ < 2 || cpu_entropy_) {
      collect_pending(cur, emit);
      return;
    }
    // depth 2: emit LAST frame's stripes (host assembly overlaps this
    // frame's GPU work), keep this one in flight
    collect_pending(prev_, emit);
    const double t2 = timing_ ? now_us() : 0;
    prev_ = std::move(cur);
    // the caller may reuse its frame buffer after we return
    ev_h2d_[prev_.par].sync();
    if (timing_) {
      tm_submit_ += t1 - t0;
      tm_collect_ += t2 - t1;
      tm_h2d_ += now_us() - t2;
      if (++tm_n_ == 256) {
        std::fprintf(stderr,
                     "[times us/frame] submit=%.0f collect=%.0f (sync=%.0f "
                     "asm=%.0f concat=%.0f) h2dwait=%.0f\n",
                     tm_submit_ / tm_n_, tm_collect_ / tm_n_,
                     tm_sync_ / tm_n_, tm_asm_ / tm_n_, tm_concat_ / tm_n_,
                     tm_h2d_ / tm_n_);
        tm_submit_ = tm_collect_ = tm_h2d_ = tm_sync_ = tm_asm_ =
            tm_concat_ = 0;
        tm_n_ = 0;
      }
    }
  }

  void flush(const Emit& emit) override { collect_pending(prev_, emit); }

  void set_pipeline_depth(int d) override {
    depth_ = std::max(1, std::min(2, d));
  }

  const char* name() const override { return "hip-h264"; }

  bool recon_dev(void** y, int* ypitch, int* height) override {
    *y = d_refY_;
    *ypitch = ypitch_;
    *height = mbh_ * 16;
    return d_refY_ != nullptr;
  }

  bool debug_dump(DebugDump& d) override {
    stream_.sync();
    // the cur -> ref refresh rides rows_stream_ (gated on db_stream_), and
    // the streams are non-blocking, so the blocking copies below do not
    // wait for it on their own
    rows_stream_.sync();
    d.w = w_;
    d.h = h_;
    d.ypitch = ypitch_;
    d.cpitch = cpitch_;
    size_t ysz = static_cast<size_t>(ypitch_) * mbh_ * 16;
    size_t csz = fc_ ? ysz : static_cast<size_t>(cpitch_) * mbh_ * 8;
    d.y.resize(ysz);
    d.cb.resize(csz);
    d.cr.resize(csz);
    // after encode_frame the recon has been copied cur -> ref
    HIP_CHECK(hipMemcpy(d.y.data(), d_refY_, ysz, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.cb.data(), d_refCb_, csz, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.cr.data(), d_refCr_, csz, hipMemcpyDeviceToHost));
    // fullcolor: plane-major (all of Y, then Cb, then Cr)
    size_t nlv = n_mb_ * planes_ * h264gpu::kLevelsPerMb;
    size_t nmt = n_mb_ * planes_ * h264gpu::kMetaPerMb;
    d.levels.resize(nlv);
    d.meta.resize(nmt);
    const int last_par = parity_ ^ 1;
    HIP_CHECK(hipMemcpy(d.levels.data(), d_levels_[last_par],
                        nlv * sizeof(int16_t),
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.meta.data(), d_meta_[last_par],
                        nmt * sizeof(int),
                        hipMemcpyDeviceToHost));
    return true;
  }

 private:
  struct StripeState {
    uint32_t frame_num = 0;
    uint32_t idr_pic_id = 0;
    bool need_idr = true;
  };

  void copy_region(uint8_t* dst, const uint8_t* src, int pitch, int y0,
                   int rows) {
    HIP_CHECK(hipMemcpyAsync(dst + static_cast<size_t>(y0) * pitch,
                             src + static_cast<size_t>(y0) * pitch,
                             static_cast<size_t>(rows) * pitch,
                             hipMemcpyDeviceToDevice, rows_stream_));
  }

  void alloc_for(int w, int h) {
    // resolution change: any pipelined frame still in flight references
    // the old buffers — drop it (streams restart with a fresh IDR anyway)
    prev_.active = false;
    stream_.sync();
    up_stream_.sync();
    db_stream_.sync();
    rows_stream_.sync();
    arena_.release();
    w_ = h_ = 0;   // until everything below succeeded: a throw retries
    mbw_ = (w + 15) / 16;
    mbh_ = (h + 15) / 16;
    ypitch_ = mbw_ * 16;
    cpitch_ = fc_ ? ypitch_ : mbw_ * 8;
    const size_t ysz = static_cast<size_t>(ypitch_) * mbh_ * 16;
    const size_t csz = static_cast<size_t>(cpitch_) * mbh_ * 8;
    for (int i = 0; i < 2; ++i)
      arena_.dev(d_frame_[i], static_cast<size_t>(w) * h * 4);
    plane_stride_ = fc_ ? ysz : 0;
    if (fc_) {
      // three full-size planes back to back: the mono kernels reach
      // plane p at base + p * plane_stride_
      arena_.dev(d_srcY_, 3 * ysz);
      arena_.dev(d_refY_, 3 * ysz);
      arena_.dev(d_curY_, 3 * ysz);
      d_srcCb_ = d_srcY_ + ysz;
      d_srcCr_ = d_srcY_ + 2 * ysz;
      d_refCb_ = d_refY_ + ysz;
      d_refCr_ = d_refY_ + 2 * ysz;
      d_curCb_ = d_curY_ + ysz;
      d_curCr_ = d_curY_ + 2 * ysz;
    } else {
      arena_.dev(d_srcY_, ysz);
      arena_.dev(d_srcCb_, csz);
      arena_.dev(d_srcCr_, csz);
      arena_.dev(d_refY_, ysz);
      arena_.dev(d_refCb_, csz);
      arena_.dev(d_refCr_, csz);
      arena_.dev(d_curY_, ysz);
      arena_.dev(d_curCb_, csz);
      arena_.dev(d_curCr_, csz);
    }
    n_mb_ = static_cast<size_t>(mbw_) * mbh_;
    // levels/meta: one region per coded plane, back to back
    const size_t n_mb = n_mb_ * planes_;
    meta_bytes_ = n_mb * h264gpu::kMetaPerMb * sizeof(int);
    for (int i = 0; i < 2; ++i) {
      arena_.dev(d_levels_[i], n_mb * h264gpu::kLevelsPerMb);
      arena_.dev(d_meta_[i], n_mb * h264gpu::kMetaPerMb);
      // meta seeds from parity^1 every frame; zero both so the first
      // seed copy is well-defined
      HIP_CHECK(hipMemset(d_meta_[i], 0, meta_bytes_));
    }
    arena_.dev(d_mip1_, static_cast<size_t>(ypitch_ / 2) * mbh_ * 8);
    pyr_stride_ = static_cast<size_t>(ypitch_ / 4) * mbh_ * 4;
    arena_.dev(d_srcY2_, pyr_stride_ * planes_);
    arena_.dev(d_refY2_, pyr_stride_ * planes_);
    const char* segs_env = std::getenv("HIPFLUX_SEGS");
    const h264::SegPlan plan = h264::seg_plan(
        mbw_, mbh_, segs_env ? std::atoi(segs_env) : 0, planes_);
    segs_ = plan.segs;
    seg_w0_ = plan.widest;
    const size_t max_jobs = static_cast<size_t>(mbh_) * segs_ * planes_;
    arena_.pinned(h_levels_, n_mb * h264gpu::kLevelsPerMb);
    arena_.pinned(h_meta_, n_mb * h264gpu::kMetaPerMb);
    // GPU entropy buffers (one slot per SLICE = row segment)
    cpu_entropy_ = std::getenv("HIPFLUX_CPU_ENTROPY") != nullptr;
    const size_t nitems = h264gpu::items_per_row(seg_w0_);
    ent_stride_words_ =
        static_cast<int>(nitems * h264gpu::kStageWordsPerItem);
    // first frame after (re)alloc: full copy
    readback_.reset(ent_stride_words_, ent_stride_words_);
    arena_.dev(d_stage_, max_jobs * ent_stride_words_);
    arena_.dev(d_nbits_, max_jobs * nitems);
    for (int i = 0; i < 2; ++i) {
      // fullcolor keeps a second, plane-grouped copy for the motion search
      arena_.dev(d_jobs_[i], max_jobs * (fc_ ? 2 : 1));
      arena_.dev(d_entout_[i], max_jobs * ent_stride_words_);
      arena_.dev(d_outbits_[i], max_jobs);
      arena_.pinned(h_jobs_[i], max_jobs * (fc_ ? 2 : 1));
      arena_.pinned(h_entout_[i], max_jobs * ent_stride_words_);
      arena_.pinned(h_outbits_[i], max_jobs);
    }
    stripes_.assign((h + stripe_h_ - 1) / stripe_h_, StripeState{});
    w_ = w;
    h_ = h;
  }

  CaptureSettings settings_;
  ThreadPool pool_;
  UseDevice dev_;
  Arena arena_;
  FrameUploader uploader_;
  Stream stream_, up_stream_, db_stream_, rows_stream_;
  Event ev_done_[2], ev_h2d_[2], ev_rows_[2], ev_db_[2];
  CompactReadback<uint32_t> readback_;   // bitstream words per slice
  int stripe_h_ = 64;
  // Hi444 separate colour planes: three monochrome pictures per frame
  const bool fc_ = settings_.video_fullcolor;
  const int planes_ = fc_ ? 3 : 1;
  size_t plane_stride_ = 0;   // bytes between the planes of src/ref/cur
  size_t pyr_stride_ = 0;     // ... of the quarter-res pyramids
  size_t n_mb_ = 0;           // MBs per plane
  int w_ = 0, h_ = 0, mbw_ = 0, mbh_ = 0, ypitch_ = 0, cpitch_ = 0;
  int segs_ = 1, seg_w0_ = 0;     // slices per MB row, widest segment
  uint8_t* d_frame_[2] = {nullptr, nullptr};
  uint8_t *d_srcY_ = nullptr, *d_srcCb_ = nullptr,
          *d_srcCr_ = nullptr, *d_refY_ = nullptr, *d_refCb_ = nullptr,
          *d_refCr_ = nullptr, *d_curY_ = nullptr, *d_curCb_ = nullptr,
          *d_curCr_ = nullptr;
  int16_t* d_levels_[2] = {};
  size_t meta_bytes_ = 0;
  uint8_t *d_mip1_ = nullptr, *d_srcY2_ = nullptr, *d_refY2_ = nullptr;
  int* d_meta_[2] = {};
  int16_t* h_levels_ = nullptr;
  int* h_meta_ = nullptr;
  // GPU entropy buffers. Buffers the host writes before (h_jobs_/d_jobs_)
  // or reads after (h_entout_/h_outbits_, d_entout_ for overflow re-copy)
  // a frame's GPU work are parity-double-buffered so depth-2 pipelining
  // can submit frame N+1 while frame N's results are still being read;
  // everything device-only is hazard-free by single-stream ordering.
  bool cpu_entropy_ = false;
  h264gpu::RowJob* d_jobs_[2] = {nullptr, nullptr};
  h264gpu::RowJob* h_jobs_[2] = {nullptr, nullptr};
  uint32_t* d_stage_ = nullptr;
  int* d_nbits_ = nullptr;
  uint32_t* d_entout_[2] = {nullptr, nullptr};
  int* d_outbits_[2] = {nullptr, nullptr};
  uint32_t* h_entout_[2] = {nullptr, nullptr};
  int* h_outbits_[2] = {nullptr, nullptr};
  int depth_ = 1;                  // 1 = sync (latency mode), 2 = pipelined
  int parity_ = 0;
  Pending prev_;                   // the in-flight frame (depth 2)
  // HIPFLUX_TIMES=1 phase accumulators (microseconds)
  const bool timing_ = std::getenv("HIPFLUX_TIMES") != nullptr;
  double tm_submit_ = 0, tm_collect_ = 0, tm_h2d_ = 0, tm_sync_ = 0,
         tm_asm_ = 0, tm_concat_ = 0;
  int tm_n_ = 0;
  int ent_stride_words_ = 0;
  std::vector<StripeState> stripes_;
};

}  // namespace

std::unique_ptr<EncodePipeline> make_hip_h264_pipeline(
    const CaptureSettings& s) {
  return std::make_unique<HipH264Pipeline>(s);
}

}  // namespace hipflux
