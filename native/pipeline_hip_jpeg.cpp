// HIP (gfx950) JPEG encode pipeline host side.
// Upload BGRX -> CSC kernel -> wave-per-block DCT/quant kernel -> per-MCU-row
// Huffman kernel -> compacted D2H -> stripe-parallel host framing.
// HIPFLUX_CPU_JPEG_ENTROPY=1 swaps the Huffman kernel for the host packer
// over D2H coefficients.
#include <cstdlib>

#include "cpu/jpeg_enc.h"
#include "engine.h"
#include "hip/jpeg_kernels.h"
#include "hip_host.h"
#include "thread_pool.h"

namespace hipflux {
namespace {

class HipJpegPipeline : public EncodePipeline {
 public:
  explicit HipJpegPipeline(const CaptureSettings& s)
      : settings_(s), pool_(encode_pool_threads()), dev_(s.gpu_id) {
    upload_dct_tables(stream_);
    tables_.dev(d_rqy_, 64);
    tables_.dev(d_rqc_, 64);
    cpu_jpeg_entropy_ = std::getenv("HIPFLUX_CPU_JPEG_ENTROPY") != nullptr;
    {
      uint32_t tabs[12 + 256 + 12 + 256];
      jpeg_export_huff(tabs, tabs + 12, tabs + 268, tabs + 280);
      tables_.dev(d_jtabs_, sizeof(tabs) / sizeof(tabs[0]));
      HIP_CHECK(hipMemcpy(d_jtabs_, tabs, sizeof(tabs),
                          hipMemcpyHostToDevice));
    }
    alloc_for(s.capture_width, s.capture_height);
  }

  struct JOut {
    std::vector<uint8_t> bytes;
    int y0 = 0, h = 0;
    int row0 = 0, rows = 0;     // MCU-row range (GPU entropy path)
    bool encode = false;
  };
  struct JPending {
    bool active = false;
    int par = 0;
    int n_rows = 0;
    int copy_words = 0;
    int quality = 80;
    bool fullcolor = false;
    uint32_t frame_id = 0;
    int mcux = 0;
    std::vector<JOut> outs;
  };

  JPending submit_frame(const RawFrame& frame, const FrameContext& ctx) {
    const bool fullcolor = settings_.video_fullcolor;
    if (frame.width != w_ || frame.height != h_)
      alloc_for(frame.width, frame.height);
    ensure_quality(ctx.jpeg_quality);
    const int par = jparity_;

    // produce chain (upload, CSC, DCT) on its own stream so it overlaps
    // the previous frame's entropy kernel + readback on stream_
    const size_t frame_bytes = static_cast<size_t>(frame.stride) * frame.height;
    if (frame.dev)   // front-end frame: already complete on the device
      HIP_CHECK(hipMemcpyAsync(d_frame2_[par], frame.dev, frame_bytes,
                               hipMemcpyDeviceToDevice, prod_stream_));
    else
      HIP_CHECK(hipMemcpyAsync(d_frame2_[par],
                               uploader_.source(frame.data, frame_bytes),
                               frame_bytes, hipMemcpyHostToDevice,
                               prod_stream_));

    const int stride_px = frame.stride / 4;
    const int stripe_h = std::max(16, settings_.stripe_height & ~15);
    const int mcu = fullcolor ? 8 : 16;
    const int mcux = (w_ + mcu - 1) / mcu;
    const int mcuy = (h_ + mcu - 1) / mcu;
    // 4:2:0 chroma is produced at its MCU-padded size: the pad samples are
    // quads of clamped pixel reads, as in jpeg_encode_bgrx
    const int cwp = mcux * 8, chp = mcuy * 8;
    launch_bgrx_to_planes(d_frame2_[par], w_, h_, stride_px, d_y_, d_cb_,
                          d_cr_, ypitch_, cpitch_, fullcolor, prod_stream_,
                          cwp, chp);

    const int rows_per_stripe = stripe_h / mcu;
    const int stripe_mcu_count = rows_per_stripe * mcux;
    const int per_mcu_real = fullcolor ? 3 : 6;

    int16_t* d_coeff = d_coeff2_[par];
    if (!fullcolor) {
      launch_dct_quant(d_y_, w_, h_, ypitch_, d_rqy_, d_coeff, 0, false,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
      launch_dct_quant(d_cb_, cwp, chp, cpitch_, d_rqc_, d_coeff, 1, false,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
      launch_dct_quant(d_cr_, cwp, chp, cpitch_, d_rqc_, d_coeff, 2, false,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
    } else {
      launch_dct_quant(d_y_, w_, h_, ypitch_, d_rqy_, d_coeff, 0, true,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
      launch_dct_quant(d_cb_, w_, h_, ypitch_, d_rqc_, d_coeff, 1, true,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
      launch_dct_quant(d_cr_, w_, h_, ypitch_, d_rqc_, d_coeff, 2, true,
                       mcux, mcuy, rows_per_stripe, stripe_mcu_count,
                       prod_stream_);
    }
    HIP_CHECK(hipEventRecord(jev_dct_[par], prod_stream_));

    JPending pd;
    pd.par = par;
    pd.quality = ctx.jpeg_quality;
    pd.fullcolor = fullcolor;
    pd.frame_id = ctx.frame_id;
    pd.mcux = mcux;
    pd.outs.resize(ctx.stripes.size());
    for (size_t i = 0; i < ctx.stripes.size(); ++i) {
      const auto& job = ctx.stripes[i];
      pd.outs[i].y0 = job.y0;
      pd.outs[i].h = job.y1 - job.y0;
      pd.outs[i].encode = job.encode;
    }

    if (cpu_jpeg_entropy_) {
      // test/debug path: stays synchronous (depth-1 semantics)
      size_t coeff_count =
          static_cast<size_t>(mcux) * mcuy * per_mcu_real * 64;
      HIP_CHECK(hipMemcpyAsync(h_coeff_, d_coeff,
                               coeff_count * sizeof(int16_t),
                               hipMemcpyDeviceToHost, prod_stream_));
      prod_stream_.sync();
      for (size_t i = 0; i < pd.outs.size(); ++i) {
        if (!pd.outs[i].encode) continue;
        pool_.submit([&, i] {
          const JOut& o = pd.outs[i];
          int stripe_idx = o.y0 / stripe_h;
          int rows = std::min(rows_per_stripe,
                              mcuy - stripe_idx * rows_per_stripe);
          const int16_t* blocks =
              h_coeff_ + static_cast<size_t>(stripe_idx) *
                             stripe_mcu_count * per_mcu_real * 64;
          jpeg_entropy_from_blocks(blocks, mcux, rows, w_, o.h,
                                   pd.quality, fullcolor,
                                   pd.outs[i].bytes, true);
        });
      }
      pool_.wait_all();
      pd.active = true;
      pd.n_rows = 0;              // bytes already assembled
      jparity_ ^= 1;
      return pd;
    }

    // GPU entropy on stream_ behind the DCT event; one kernel row per
    // MCU row of every scheduled stripe
    jpeggpu::JRow* jrows = h_jrows2_[par];
    int n_rows = 0;
    for (size_t i = 0; i < pd.outs.size(); ++i) {
      if (!pd.outs[i].encode) continue;
      int stripe_idx = pd.outs[i].y0 / stripe_h;
      int rows = std::min(rows_per_stripe,
                          mcuy - stripe_idx * rows_per_stripe);
      pd.outs[i].row0 = n_rows;
      pd.outs[i].rows = rows;
      size_t base = static_cast<size_t>(stripe_idx) * stripe_mcu_count *
                    per_mcu_real * 64;
      for (int r = 0; r < rows; ++r)
        jrows[n_rows++].coeff_off = static_cast<int>(
            base + static_cast<size_t>(r) * mcux * per_mcu_real * 64);
    }
    pd.n_rows = n_rows;
    pd.active = true;
    jparity_ ^= 1;
    if (!n_rows) return pd;

    HIP_CHECK(hipStreamWaitEvent(stream_, jev_dct_[par], 0));
    HIP_CHECK(hipMemcpyAsync(d_jrows2_[par], h_jrows2_[par],
                             sizeof(jpeggpu::JRow) * n_rows,
                             hipMemcpyHostToDevice, stream_));
    jpeggpu::launch_jpeg_entropy(d_coeff, d_jrows2_[par], n_rows, mcux,
                                 per_mcu_real, d_jtabs_, d_jstage_,
                                 d_jnbits_, d_jout2_[par], jout_stride_,
                                 d_joutbits2_[par], stream_);
    // adaptive compacted readback (2x last frame's max row)
    pd.copy_words =
        readback_.read(h_jout2_[par], d_jout2_[par], n_rows, stream_);
    HIP_CHECK(hipMemcpyAsync(h_joutbits2_[par], d_joutbits2_[par],
                             4 * n_rows, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(jev_done_[par], stream_));
    return pd;
  }

  void collect_pending(JPending& pd, const Emit& emit) {
    if (!pd.active) return;
    pd.active = false;
    const int par = pd.par;
    if (!cpu_jpeg_entropy_ && pd.n_rows) {
      jev_done_[par].sync();
      const int* outbits = h_joutbits2_[par];
      readback_.settle(
          h_jout2_[par], d_jout2_[par], pd.n_rows, pd.copy_words,
          [&](int r) { return (outbits[r] + 31) / 32 + 1; },
          [&](int max_words) {
            return std::min(jout_stride_, max_words * 2 + 64);
          });
      for (size_t i = 0; i < pd.outs.size(); ++i) {
        if (!pd.outs[i].encode) continue;
        pool_.submit([&, i, par, outbits] {
          JOut& o = pd.outs[i];
          jpeg_write_headers(o.bytes, w_, o.h, pd.quality,
                             pd.fullcolor, pd.mcux);
          int rst = 0;
          for (int r = 0; r < o.rows; ++r) {
            if (r > 0) {
              o.bytes.push_back(0xFF);
              o.bytes.push_back(
                  static_cast<uint8_t>(0xD0 + (rst++ & 7)));
            }
            const uint32_t* words =
                h_jout2_[par] + (size_t)(o.row0 + r) * jout_stride_;
            jpeg_append_row_bits(words, outbits[o.row0 + r], o.bytes);
          }
          o.bytes.push_back(0xFF);
          o.bytes.push_back(0xD9);
        });
      }
      pool_.wait_all();
    }
    for (auto& o : pd.outs) {
      if (!o.encode) continue;
      EncodedStripe s;
      s.type = StripeType::kJpeg;
      s.data = o.bytes.data();
      s.size = o.bytes.size();
      s.frame_id = pd.frame_id;
      s.y = o.y0;
      s.width = w_;
      s.height = o.h;
      s.is_keyframe = true;
      emit(s);
    }
  }

  void encode_frame(const RawFrame& frame, const FrameContext& ctx,
                    const Emit& emit) override {
    JPending cur = submit_frame(frame, ctx);
    if (jdepth_ < 2 || cpu_jpeg_entropy_) {
      collect_pending(cur, emit);
      collect_pending(jprev_, emit);   // drain any leftover from a mode flip
      return;
    }
    collect_pending(jprev_, emit);
    jprev_ = std::move(cur);
    // the caller may reuse its frame buffer once the H2D completes; the
    // DCT event is recorded after CSC+DCT which transitively covers it
    jev_dct_[jprev_.par].sync();
  }

  void flush(const Emit& emit) override { collect_pending(jprev_, emit); }

  void set_pipeline_depth(int d) override {
    jdepth_ = std::max(1, std::min(2, d));
  }

  const char* name() const override { return "hip-jpeg"; }

 private:
  void alloc_for(int w, int h) {
    // an in-flight frame references the old buffers: drop it
    jprev_ = JPending{};
    jparity_ = 0;
    stream_.sync();
    prod_stream_.sync();
    arena_.release();
    w_ = h_ = 0;   // until everything below succeeded: a throw retries
    ypitch_ = (w + 255) & ~255;
    cpitch_ = ((w + 1) / 2 + 255) & ~255;
    for (int i = 0; i < 2; ++i)
      arena_.dev(d_frame2_[i], static_cast<size_t>(w) * h * 4);
    arena_.dev(d_y_, static_cast<size_t>(ypitch_) * h);
    // chroma buffers sized for 4:4:4 (the larger case), and for the
    // MCU-padded 4:2:0 chroma rows, which exceed h when h < 16
    const size_t crows = std::max(h, (h + 15) / 16 * 8);
    arena_.dev(d_cb_, static_cast<size_t>(ypitch_) * crows);
    arena_.dev(d_cr_, static_cast<size_t>(ypitch_) * crows);
    // coefficients: 6 blocks/MCU covers both 420 (6) and 444 (3)
    size_t mcux = (w + 7) / 8, mcuy = (h + 7) / 8;  // worst case 444
    size_t coeff_count = mcux * mcuy * 6 * 64;
    for (int i = 0; i < 2; ++i) arena_.dev(d_coeff2_[i], coeff_count);
    arena_.pinned(h_coeff_, coeff_count);
    // GPU entropy buffers: one slot per MCU row (444 row count is the max)
    size_t max_rows = mcuy;
    size_t max_items = std::max(mcux * 3, ((size_t)(w + 15) / 16) * 6);
    jout_stride_ = (int)(max_items * jpeggpu::kJStageWords);
    arena_.dev(d_jstage_, max_rows * max_items * jpeggpu::kJStageWords);
    arena_.dev(d_jnbits_, max_rows * max_items);
    for (int i = 0; i < 2; ++i) {
      arena_.dev(d_jrows2_[i], max_rows);
      arena_.dev(d_jout2_[i], max_rows * jout_stride_);
      arena_.dev(d_joutbits2_[i], max_rows);
      arena_.pinned(h_jout2_[i], max_rows * jout_stride_);
      arena_.pinned(h_joutbits2_[i], max_rows);
      arena_.pinned(h_jrows2_[i], max_rows);
    }
    readback_.reset(jout_stride_, jout_stride_);   // first frame: full copy
    w_ = w;
    h_ = h;
  }

  void ensure_quality(int q) {
    if (q == cur_quality_) return;
    uint8_t qy[64], qc[64];
    jpeg_quality_tables(q, qy, qc);
    float rqy[64], rqc[64];
    for (int i = 0; i < 64; ++i) {
      rqy[i] = 1.0f / qy[i];
      rqc[i] = 1.0f / qc[i];
    }
    // quality changes are rare: drain BOTH streams so an in-flight
    // frame never sees half-updated tables, then upload on the producer
    stream_.sync();
    prod_stream_.sync();
    HIP_CHECK(hipMemcpyAsync(d_rqy_, rqy, sizeof(rqy), hipMemcpyHostToDevice,
                             prod_stream_));
    HIP_CHECK(hipMemcpyAsync(d_rqc_, rqc, sizeof(rqc), hipMemcpyHostToDevice,
                             prod_stream_));
    prod_stream_.sync();
    cur_quality_ = q;
  }

  CaptureSettings settings_;
  ThreadPool pool_;
  UseDevice dev_;
  Arena tables_;   // quantiser + Huffman tables: live as long as the pipeline
  Arena arena_;    // everything sized by the resolution
  FrameUploader uploader_;
  Stream stream_, prod_stream_;
  Event jev_dct_[2], jev_done_[2];
  CompactReadback<uint32_t> readback_;
  int jparity_ = 0;
  int jdepth_ = 1;
  JPending jprev_;
  uint8_t* d_frame2_[2] = {};
  uint8_t* d_y_ = nullptr;
  uint8_t* d_cb_ = nullptr;
  uint8_t* d_cr_ = nullptr;
  int16_t* d_coeff2_[2] = {};
  uint32_t* d_jtabs_ = nullptr;
  jpeggpu::JRow* d_jrows2_[2] = {};
  uint32_t* d_jstage_ = nullptr;
  int* d_jnbits_ = nullptr;
  uint32_t* d_jout2_[2] = {};
  int* d_joutbits2_[2] = {};
  uint32_t* h_jout2_[2] = {};
  int* h_joutbits2_[2] = {};
  jpeggpu::JRow* h_jrows2_[2] = {};
  int jout_stride_ = 0;
  bool cpu_jpeg_entropy_ = false;
  int16_t* h_coeff_ = nullptr;
  float* d_rqy_ = nullptr;
  float* d_rqc_ = nullptr;
  int w_ = 0, h_ = 0, ypitch_ = 0, cpitch_ = 0;
  int cur_quality_ = -1;
};

}  // namespace

std::unique_ptr<EncodePipeline> make_hip_jpeg_pipeline(
    const CaptureSettings& s) {
  return std::make_unique<HipJpegPipeline>(s);
}

}  // namespace hipflux
