// HIP (gfx950) HEVC encode pipeline host side.
// Upload BGRX -> CSC kernel (shared with JPEG/H.264) -> per-slice CTU
// wavefront kernel (intra + transform + quant + recon) -> per-slice CABAC
// kernel -> compacted D2H -> host NAL assembly on the pool.
// Byte-identical to CpuHevcPipeline (asserted by tests/test_gpu_hevc.py);
// HIPFLUX_CPU_HEVC_ENTROPY=1 swaps the CABAC kernel for the host entropy
// coder over D2H levels/meta to isolate rows-kernel vs entropy bugs.
// settings.hevc_inter (4:2:0 only): a stripe's emissions after its first
// are P pictures (zero-motion merge/skip + intra CTUs) against its
// previous coded picture, which is the recon planes themselves, updated
// in place by the rows kernel. Per-stripe {have_ref, poc} live here.
#include <cstdio>
#include <cstdlib>

#include "cpu/hevc/encoder.h"       // default_slices_per_row
#include "cpu/hevc/gpu_entropy.h"
#include "cpu/hevc/tables.h"        // chroma_qp
#include "engine.h"
#include "hip/hevc_kernels.h"
#include "hip/jpeg_kernels.h"       // launch_bgrx_to_planes
#include "hip_host.h"
#include "thread_pool.h"

namespace hipflux {
namespace {

class HipHevcPipeline : public EncodePipeline {
 public:
  // CABAC output bytes reserved per CTU, 4:2:0 and fullcolor (derivation
  // in alloc_for); hip_hevc_bytes_per_ctu() shows both to the tests
  static constexpr int kBytesPerCtu = 2048;
  static constexpr int kFullcolorBytesPerCtu = 4096;

  explicit HipHevcPipeline(const CaptureSettings& s)
      : settings_(s), pool_(encode_pool_threads()), dev_(s.gpu_id),
        fc_(s.video_fullcolor), inter_(s.hevc_inter && !s.video_fullcolor) {
    if (s.hevc_inter && s.video_fullcolor)
      std::fprintf(stderr,
                   "[hip-hevc] hevc_inter is 4:2:0 only; video_fullcolor "
                   "stays all-intra\n");
    cpu_entropy_ = std::getenv("HIPFLUX_CPU_HEVC_ENTROPY") != nullptr;
    timing_ = std::getenv("HIPFLUX_TIMES") != nullptr;
    stripe_h_ = std::max(16, s.stripe_height & ~15);
    alloc_for(s.capture_width, s.capture_height);
  }

  struct StripeRef {
    int y0, vis_h;      // pixels
    int job0, jobn;     // job index range
    bool idr;           // IDR emission (parameter sets, key stripe)
  };
  // Temporal state of one stripe position (index into ctx.stripes).
  struct StripeState {
    bool have_ref = false;   // recon planes hold its previous coded picture
    int poc = 0;             // POC of its next picture (0 after an IDR)
  };
  struct Pending {
    bool active = false;
    int par = 0;
    int n_jobs = 0;
    int cap = 0;        // D2H compaction cap this frame was submitted with
    uint32_t frame_id = 0;
    double ts_ms = 0;
    std::vector<StripeRef> stripes;
  };

  // Queue one frame's full GPU chain (upload, CSC, CTU rows, CABAC,
  // counts + compacted bitstream D2H) on stream_; nothing blocks here
  // beyond pageable-staging copies.
  Pending submit_frame(const RawFrame& frame, const FrameContext& ctx) {
    if (frame.width != w_ || frame.height != h_)
      alloc_for(frame.width, frame.height);
    const int qp = std::min(51, std::max(0, ctx.crf));
    const int par = parity_;

    // ---- upload + CSC
    const size_t frame_bytes = static_cast<size_t>(frame.stride) * frame.height;
    // frame N+1's upload/CSC/rows run on rows_stream_, concurrent with
    // frame N's CABAC on stream_ (levels/meta are parity
    // double-buffered). Without hevc_inter the recon planes have no
    // cross-frame reader. With it, the rows kernel of frame N+1 reads the
    // recon that the rows kernel of frame N wrote: both run on
    // rows_stream_, so at depth 2 frame N+1's rows follow frame N's rows
    // in stream order and no other stream touches the planes.
    if (frame.dev)   // front-end frame: already complete on the device
      HIP_CHECK(hipMemcpyAsync(d_frame_[par], frame.dev, frame_bytes,
                               hipMemcpyDeviceToDevice, rows_stream_));
    else
      HIP_CHECK(hipMemcpyAsync(d_frame_[par],
                               uploader_.source(frame.data, frame_bytes),
                               frame_bytes, hipMemcpyHostToDevice,
                               rows_stream_));
    HIP_CHECK(hipEventRecord(ev_h2d_[par], rows_stream_));
    launch_bgrx_to_planes(d_frame_[par], w_, h_, frame.stride / 4, d_srcY_,
                          d_srcCb_, d_srcCr_, ypitch_, cpitch_, fc_,
                          rows_stream_);

    // ---- job list (must mirror the CPU StripeEncoder's segmentation)
    Pending pd;
    pd.par = par;
    pd.frame_id = ctx.frame_id;
    pd.ts_ms = frame.ts_ms;
    int n_jobs = 0;
    bool any_p = false;
    if (sstate_.size() != ctx.stripes.size())
      sstate_.assign(ctx.stripes.size(), StripeState{});
    const int spr = hevc::default_slices_per_row(w_);
    for (size_t i = 0; i < ctx.stripes.size(); ++i) {
      const auto& st = ctx.stripes[i];
      if (!st.encode) continue;
      const int vis_h = std::min(st.y1, h_) - st.y0;
      const int s_ctb_h = (vis_h + 15) / 16;
      const int n_ctb = ctbw_ * s_ctb_h;
      int addr_bits = 1;
      while ((1 << addr_bits) < n_ctb) ++addr_bits;
      const int per = (ctbw_ + spr - 1) / spr;
      StripeState& ss = sstate_[i];
      const bool p_pic = inter_ && ss.have_ref && !ctx.idr;
      if (!p_pic) ss.poc = 0;
      any_p |= p_pic;
      StripeRef sr{st.y0, vis_h, n_jobs, 0, !p_pic};
      for (int r = 0; r < s_ctb_h; ++r) {
        for (int s0 = 0; s0 < ctbw_; s0 += per) {
          auto& j = h_jobs_[par][n_jobs++];
          j.ctu_row = st.y0 / 16 + r;
          j.ctu_x0 = s0;
          j.seg_w = std::min(per, ctbw_ - s0);
          j.qp = qp;
          j.qpc = hevc::chroma_qp_for(qp, fc_);
          j.first_slice = (r == 0 && s0 == 0) ? 1 : 0;
          j.slice_addr = r * ctbw_ + s0;
          j.addr_bits = addr_bits;
          j.last_in_pic = 0;
          j.slice_type = p_pic ? 1 : 2;
          j.poc_lsb = ss.poc & 255;
        }
      }
      // POC counts this stripe's own coded pictures
      ++ss.poc;
      ss.have_ref = true;
      sr.jobn = n_jobs;
      pd.stripes.push_back(sr);
    }
    if (n_jobs == 0) return pd;
    pd.n_jobs = n_jobs;
    pd.active = true;
    parity_ ^= 1;

    if (timing_) HIP_CHECK(hipEventRecord(ev_t_[0], rows_stream_));
    HIP_CHECK(hipMemcpyAsync(d_jobs_[par], h_jobs_[par],
                             sizeof(hevcgpu::HevcJob) * n_jobs,
                             hipMemcpyHostToDevice, rows_stream_));
    if (fc_)
      hevcgpu::launch_hevc_rows444(d_srcY_, d_srcCb_, d_srcCr_, ypitch_, w_,
                                   h_, d_curY_, d_curCb_, d_curCr_, ctbw_,
                                   n_jobs, d_jobs_[par], d_levels_[par],
                                   d_meta_[par], rows_stream_);
    else if (any_p)
      // I and P jobs of one frame share one launch that branches per job;
      // a frame with no P job keeps the unchanged I kernels
      hevcgpu::launch_hevc_rows_p(d_srcY_, d_srcCb_, d_srcCr_, ypitch_,
                                  cpitch_, w_, h_, d_curY_, d_curCb_,
                                  d_curCr_, ctbw_, n_jobs, d_jobs_[par],
                                  d_levels_[par], d_meta_[par], rows_stream_);
    else
      hevcgpu::launch_hevc_rows(d_srcY_, d_srcCb_, d_srcCr_, ypitch_,
                                cpitch_, w_, h_, d_curY_, d_curCb_, d_curCr_,
                                ctbw_, n_jobs, d_jobs_[par], d_levels_[par],
                                d_meta_[par], rows_stream_);
    HIP_CHECK(hipEventRecord(ev_rows_[par], rows_stream_));
    HIP_CHECK(hipStreamWaitEvent(stream_, ev_rows_[par], 0));
    if (cpu_entropy_) {
      HIP_CHECK(hipMemcpyAsync(h_levels_, d_levels_[par], levels_bytes_,
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipMemcpyAsync(h_meta_, d_meta_[par], meta_bytes_,
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipEventRecord(ev_done_[par], stream_));
      return pd;
    }
    if (timing_) HIP_CHECK(hipEventRecord(ev_t_[1], stream_));
    if (any_p)
      hevcgpu::launch_hevc_cabac_p(d_levels_[par], d_meta_[par], ctbw_,
                                   n_jobs, d_jobs_[par], d_out_[par],
                                   out_stride_, d_counts_[par], stream_);
    else
      hevcgpu::launch_hevc_cabac(d_levels_[par], d_meta_[par], ctbw_, n_jobs,
                                 d_jobs_[par], d_out_[par], out_stride_,
                                 d_counts_[par], stream_, fc_);
    if (timing_) HIP_CHECK(hipEventRecord(ev_t_[2], stream_));
    HIP_CHECK(hipMemcpyAsync(h_counts_[par], d_counts_[par],
                             sizeof(int) * 3 * n_jobs,
                             hipMemcpyDeviceToHost, stream_));
    // adaptive compaction: copy only ~the used prefix of each job's
    // bytes (cap = 2x last frame's max count); overflowing jobs are
    // re-copied exactly at collect time
    pd.cap = readback_.read(h_out_[par], d_out_[par], n_jobs, stream_);
    HIP_CHECK(hipEventRecord(ev_done_[par], stream_));
    return pd;
  }

  // Wait for a submitted frame's D2H, assemble its NALs on the pool and
  // emit.
  void collect_pending(Pending& pd, const Emit& emit) {
    if (!pd.active) return;
    pd.active = false;
    const int par = pd.par;
    ev_done_[par].sync();
    const int n_jobs = pd.n_jobs;
    if (!cpu_entropy_) {
      readback_.settle(
          h_out_[par], d_out_[par], n_jobs, pd.cap,
          [&](int j) {
            const int cnt = h_counts_[par][j * 3];
            if (cnt > out_stride_)
              throw std::runtime_error("hevc cabac overflow");
            return cnt;
          },
          [](int max_count) { return std::max(4096, 2 * max_count); });
      if (timing_) {
        float t_rows = 0, t_cab = 0;
        (void)hipEventElapsedTime(&t_rows, ev_t_[0], ev_t_[1]);
        (void)hipEventElapsedTime(&t_cab, ev_t_[1], ev_t_[2]);
        std::fprintf(stderr, "[hevc-times] rows %.2fms cabac %.2fms\n",
                     t_rows, t_cab);
      }
    }

    // ---- host NAL assembly (parallel over stripes)
    struct SOut {
      std::vector<uint8_t> bytes;
      int y0, vis_h;
      bool idr;
    };
    std::vector<SOut> outs(pd.stripes.size());
    for (size_t si = 0; si < pd.stripes.size(); ++si) {
      pool_.submit([&, si, par] {
        const StripeRef& sr = pd.stripes[si];
        SOut& o = outs[si];
        o.y0 = sr.y0;
        o.vis_h = sr.vis_h;
        const int coded_h = (sr.vis_h + 15) & ~15;
        o.idr = sr.idr;
        if (sr.idr)   // P emissions carry no parameter sets
          hevc::write_hevc_stripe_headers(ctbw_ * 16, coded_h, w_, sr.vis_h,
                                          o.bytes, fc_, inter_);
        for (int j = sr.job0; j < sr.jobn; ++j) {
          const auto& job = h_jobs_[par][j];
          if (cpu_entropy_) {
            hevc::encode_hevc_job_nal(h_levels_, h_meta_, ctbw_,
                                      job.ctu_row, job.ctu_x0, job.seg_w,
                                      job.qp, job.first_slice != 0,
                                      job.slice_addr, job.addr_bits,
                                      o.bytes, fc_, job.slice_type,
                                      job.poc_lsb);
          } else {
            hevc::assemble_hevc_slice_nal(
                h_out_[par] + (size_t)j * out_stride_,
                h_counts_[par][j * 3], h_counts_[par][j * 3 + 1],
                h_counts_[par][j * 3 + 2], job.first_slice != 0,
                job.slice_addr, job.addr_bits, job.qp, o.bytes,
                job.slice_type, job.poc_lsb);
          }
        }
      });
    }
    pool_.wait_all();
    for (auto& o : outs) {
      EncodedStripe s;
      s.type = StripeType::kHevc;
      s.data = o.bytes.data();
      s.size = o.bytes.size();
      s.frame_id = pd.frame_id;
      s.capture_ts_ms = pd.ts_ms;
      s.y = o.y0;
      s.width = w_;
      s.height = o.vis_h;
      s.is_keyframe = o.idr;
      emit(s);
    }
  }

  void encode_frame(const RawFrame& frame, const FrameContext& ctx,
                    const Emit& emit) override {
    Pending cur = submit_frame(frame, ctx);
    if (!cur.active) {
      collect_pending(prev_, emit);
      return;
    }
    if (depth_ < 2 || cpu_entropy_) {
      collect_pending(cur, emit);
      return;
    }
    // depth 2: emit LAST frame's stripes (host assembly overlaps this
    // frame's GPU chain), keep this one in flight
    collect_pending(prev_, emit);
    prev_ = std::move(cur);
    // the caller may reuse its frame buffer once we return
    ev_h2d_[prev_.par].sync();
  }

  void flush(const Emit& emit) override { collect_pending(prev_, emit); }

  void set_pipeline_depth(int d) override {
    depth_ = std::max(1, std::min(2, d));
  }

  const char* name() const override { return "hip-hevc"; }

  bool recon_dev(void** y, int* ypitch, int* height) override {
    *y = d_curY_;
    *ypitch = ypitch_;
    *height = ctbh_ * 16;
    return d_curY_ != nullptr;
  }

  bool debug_dump(DebugDump& d) override {
    d.w = w_;
    d.h = h_;
    d.ypitch = ypitch_;
    d.cpitch = cpitch_;
    const int ch16 = (h_ + 15) & ~15;
    d.y.resize(static_cast<size_t>(ypitch_) * ch16);
    d.cb.resize(static_cast<size_t>(cpitch_) * crows_);
    d.cr.resize(static_cast<size_t>(cpitch_) * crows_);
    HIP_CHECK(hipMemcpy(d.y.data(), d_curY_, d.y.size(),
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.cb.data(), d_curCb_, d.cb.size(),
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.cr.data(), d_curCr_, d.cr.size(),
                        hipMemcpyDeviceToHost));
    d.levels.resize(levels_bytes_ / sizeof(int16_t));
    d.meta.resize(meta_bytes_ / sizeof(int));
    const int last_par = parity_ ^ 1;   // parity of the last submit
    HIP_CHECK(hipMemcpy(d.levels.data(), d_levels_[last_par],
                        levels_bytes_, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(d.meta.data(), d_meta_[last_par], meta_bytes_,
                        hipMemcpyDeviceToHost));
    return true;
  }

 private:
  void alloc_for(int w, int h) {
    prev_ = Pending{};          // in-flight frame is gone with its buffers
    parity_ = 0;
    sstate_.clear();            // new planes hold no reference picture
    stream_.sync();
    rows_stream_.sync();
    arena_.release();
    w_ = h_ = 0;   // until everything below succeeded: a throw retries
    ctbw_ = (w + 15) / 16;
    ctbh_ = (h + 15) / 16;
    ypitch_ = ctbw_ * 16;
    const int ch16 = ctbh_ * 16;
    // fullcolor: full-size chroma source/recon planes
    cpitch_ = fc_ ? ypitch_ : ypitch_ / 2;
    crows_ = fc_ ? ch16 : ch16 / 2;

    for (int i = 0; i < 2; ++i)
      arena_.dev(d_frame_[i], static_cast<size_t>(w + 64) * 4 * (h + 16));
    arena_.dev(d_srcY_, static_cast<size_t>(ypitch_) * ch16);
    arena_.dev(d_srcCb_, static_cast<size_t>(cpitch_) * crows_);
    arena_.dev(d_srcCr_, static_cast<size_t>(cpitch_) * crows_);
    arena_.dev(d_curY_, static_cast<size_t>(ypitch_) * ch16);
    arena_.dev(d_curCb_, static_cast<size_t>(cpitch_) * crows_);
    arena_.dev(d_curCr_, static_cast<size_t>(cpitch_) * crows_);

    const size_t n_ctu = static_cast<size_t>(ctbw_) * ctbh_;
    const size_t n_levels =
        n_ctu * (fc_ ? hevcgpu::kHevcLevelsPerCtu444
                     : hevcgpu::kHevcLevelsPerCtu);
    const size_t n_meta = n_ctu * hevcgpu::kHevcMetaPerCtu;
    levels_bytes_ = n_levels * sizeof(int16_t);
    meta_bytes_ = n_meta * sizeof(int);
    for (int i = 0; i < 2; ++i) {
      arena_.dev(d_levels_[i], n_levels);
      arena_.dev(d_meta_[i], n_meta);
    }

    const int spr = hevc::default_slices_per_row(w);
    const size_t max_jobs = static_cast<size_t>(ctbh_) * spr + 8;
    // DevCabac::put has no bound, so the stride has to hold the largest
    // slice segment. Measured on the CPU encoder at qp 0, largest IDR NAL
    // bytes per CTU over 1-, 8- and 20-CTU segments (profiles/NOTES.md,
    // tests/test_hevc_recon_host.py): uniform noise 500, saturated 2x2
    // colour checker 247, 1-pixel 0/255 checkerboard 169. The stride is
    // at least 2x the largest figure, which the host test asserts.
    // P slices stay inside it. A skip or merge CTU codes the same three
    // TBs with the same level clamp and a smaller rounding offset
    // (85 < 171), so no more levels than an intra CTU, behind a prefix of
    // at most 4 bins (cu_skip, pred_mode, part_mode, merge). An intra CTU
    // of a P slice is the larger case: the whole intra syntax plus
    // cu_skip_flag and pred_mode_flag, under initType-1 contexts; on
    // uniform noise, where every P CTU ends up intra, that measured +0.4
    // to +1.0% bytes over the I slices (profiles/NOTES.md), which the 2x
    // margin over the measured 500 bytes per CTU covers.
    const int per = (ctbw_ + spr - 1) / spr;
    out_stride_ = per * kBytesPerCtu;
    // fullcolor codes 768 coefficients per CTU, so that argument does not
    // carry over. Measured on the CPU encoder at qp 0 (make asan-hevc444),
    // largest slice-segment bytes per CTU over 60-, 8- and 1-CTU segments:
    // uniform noise 1179, saturated 1-pixel checkerboard 500. The stride
    // is 2x the larger figure rounded up to a power of two.
    if (fc_) out_stride_ = per * kFullcolorBytesPerCtu;
    for (int i = 0; i < 2; ++i) {
      arena_.dev(d_jobs_[i], max_jobs);
      arena_.dev(d_out_[i], max_jobs * out_stride_);
      arena_.dev(d_counts_[i], max_jobs * 3);
      arena_.pinned(h_jobs_[i], max_jobs);
      arena_.pinned(h_out_[i], max_jobs * out_stride_);
      arena_.pinned(h_counts_[i], max_jobs * 3);
    }
    arena_.pinned(h_levels_, n_levels);
    arena_.pinned(h_meta_, n_meta);
    readback_.reset(out_stride_, out_stride_);   // first frame: full copy
    w_ = w;
    h_ = h;
  }

  CaptureSettings settings_;
  ThreadPool pool_;
  UseDevice dev_;
  Arena arena_;
  FrameUploader uploader_;
  Stream stream_, rows_stream_;
  Event ev_t_[3] = {Event(hipEventDefault), Event(hipEventDefault),
                    Event(hipEventDefault)};   // HIPFLUX_TIMES marks
  Event ev_h2d_[2], ev_done_[2], ev_rows_[2];
  CompactReadback<uint8_t> readback_;   // CABAC bytes per slice
  bool cpu_entropy_ = false;
  bool timing_ = false;
  const bool fc_;         // video_fullcolor: Main 4:4:4 instead of 4:2:0
  const bool inter_;      // hevc_inter && !fc_: P stripes after each IDR
  std::vector<StripeState> sstate_;   // per ctx.stripes index
  int stripe_h_ = 64;
  int depth_ = 1;         // 1 = sync (latency mode), 2 = pipelined
  int parity_ = 0;
  Pending prev_;
  int w_ = 0, h_ = 0, ctbw_ = 0, ctbh_ = 0, ypitch_ = 0, cpitch_ = 0;
  int crows_ = 0;         // rows of one chroma plane
  int out_stride_ = 0;
  size_t levels_bytes_ = 0, meta_bytes_ = 0;

  uint8_t* d_frame_[2] = {};
  uint8_t *d_srcY_ = nullptr, *d_srcCb_ = nullptr, *d_srcCr_ = nullptr;
  uint8_t *d_curY_ = nullptr, *d_curCb_ = nullptr, *d_curCr_ = nullptr;
  int16_t* d_levels_[2] = {};
  int* d_meta_[2] = {};
  hevcgpu::HevcJob* d_jobs_[2] = {};
  uint8_t* d_out_[2] = {};
  int* d_counts_[2] = {};

  hevcgpu::HevcJob* h_jobs_[2] = {};
  uint8_t* h_out_[2] = {};
  int* h_counts_[2] = {};
  int16_t* h_levels_ = nullptr;
  int* h_meta_ = nullptr;
};

}  // namespace

std::unique_ptr<EncodePipeline> make_hip_hevc_pipeline(
    const CaptureSettings& s) {
  return std::make_unique<HipHevcPipeline>(s);
}

int hip_hevc_bytes_per_ctu(bool fullcolor) {
  return fullcolor ? HipHevcPipeline::kFullcolorBytesPerCtu
                   : HipHevcPipeline::kBytesPerCtu;
}

}  // namespace hipflux
