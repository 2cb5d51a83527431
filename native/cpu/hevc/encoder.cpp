// HEVC stripe encoder — CPU reference (see encoder.h for the design).
#include "encoder.h"

#include <algorithm>
#include <climits>
#include <cstring>

#include "cabac.h"
#include "entropy.h"
#include "headers.h"
#include "intra.h"
#include "tables.h"
#include "transform.h"

namespace hipflux {
namespace hevc {

namespace {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

inline uint8_t clip8(int v) {
  return static_cast<uint8_t>(v < 0 ? 0 : v > 255 ? 255 : v);
}

// One transform block's coded data.
template <int N>
struct TbData {
  int16_t level[N * N];
  bool cbf = false;
};

}  // namespace

// ---- encoder impl --------------------------------------------------------

struct StripeEncoder::Impl {
  int w, h;            // visible
  int cw, ch;          // coded (16-aligned)
  int ctb_w, ctb_h;    // CTUs per row / rows
  int slices_per_row;
  bool fullcolor;      // 4:4:4: chroma planes are luma-sized
  int addr_bits;
  std::vector<uint8_t> ry, rcb, rcr;        // recon planes (coded dims)
  std::vector<uint8_t> sy, scb, scr;        // padded source planes
  std::vector<uint8_t> luma_mode;           // per-CTU chosen mode
  std::vector<uint8_t> ps_cache;            // VPS/SPS/PPS bytes
  int ypitch, cpitch;
  bool inter;          // P pictures enabled (4:2:0 only)
  bool have_ref = false;   // recon planes hold the previous coded picture
  int poc = 0;             // POC of the next picture (0 after an IDR)

  Impl(int width, int height, int spr, bool fc, bool inter_on)
      : w(width), h(height), cw((width + 15) & ~15), ch((height + 15) & ~15),
        ctb_w(cw / 16), ctb_h(ch / 16),
        slices_per_row(std::max(1, std::min(spr, cw / 16))), fullcolor(fc),
        inter(inter_on && !fc) {
    int n_ctb = ctb_w * ctb_h;
    addr_bits = 1;
    while ((1 << addr_bits) < n_ctb) ++addr_bits;
    ypitch = cw;
    cpitch = fullcolor ? cw : cw / 2;
    const int crows = fullcolor ? ch : ch / 2;
    ry.resize(static_cast<size_t>(ypitch) * ch);
    rcb.resize(static_cast<size_t>(cpitch) * crows);
    rcr.resize(static_cast<size_t>(cpitch) * crows);
    sy = ry;
    scb = rcb;
    scr = rcr;
    luma_mode.resize(n_ctb);
    write_vps_nal(ps_cache, level_idc_for(cw, ch), fullcolor, inter);
    write_sps_nal(ps_cache, cw, ch, w, h, fullcolor, inter);
    write_pps_nal(ps_cache);
  }

  // pad source into coded-size planes with edge replication
  void load_source(const uint8_t* y, int ypitch_in, const uint8_t* cb,
                   const uint8_t* cr, int cpitch_in) {
    for (int r = 0; r < ch; ++r) {
      int sr = std::min(r, h - 1);
      std::memcpy(&sy[static_cast<size_t>(r) * ypitch],
                  y + static_cast<size_t>(sr) * ypitch_in, w);
      for (int x = w; x < cw; ++x)
        sy[static_cast<size_t>(r) * ypitch + x] = sy[r * ypitch + w - 1];
    }
    int cwh = cw / 2, chh = ch / 2, wh = (w + 1) / 2, hh = (h + 1) / 2;
    if (fullcolor) {
      cwh = cw;
      chh = ch;
      wh = w;
      hh = h;
    }
    for (int r = 0; r < chh; ++r) {
      int sr = std::min(r, hh - 1);
      std::memcpy(&scb[static_cast<size_t>(r) * cpitch],
                  cb + static_cast<size_t>(sr) * cpitch_in, wh);
      std::memcpy(&scr[static_cast<size_t>(r) * cpitch],
                  cr + static_cast<size_t>(sr) * cpitch_in, wh);
      for (int x = wh; x < cwh; ++x) {
        scb[static_cast<size_t>(r) * cpitch + x] = scb[r * cpitch + wh - 1];
        scr[static_cast<size_t>(r) * cpitch + x] = scr[r * cpitch + wh - 1];
      }
    }
  }

  // Encode one 16x16 CTU: choose mode, transform, reconstruct, and emit
  // CABAC bins. left_avail reflects the slice-segment boundary.
  // In a P slice (p_slice) the zero-motion merge candidate competes: the
  // predictor of every sample is the sample it overwrites in the recon
  // planes (the previous coded picture), so recon updates in place.
  // left_mode is the left CTU's luma_mode[] entry (intra mode, or a
  // CtuKind for inter CTUs).
  void encode_ctu(CabacEncoder& cab, ContextBank& bank, int cx, int cy,
                  bool left_avail, int qp, uint8_t left_mode,
                  bool p_slice = false) {
    const int x0 = cx * 16, y0 = cy * 16;
    // --- luma mode decision + transform
    Avail av;  // one slice per CTU row: only left neighbors exist
    av.left = left_avail;
    av.corner = false;
    av.top = av.top_right = av.below_left = false;

    uint8_t ref[65], reff[65];
    build_refs<16>(ry.data(), ypitch, x0, y0, av, ref);
    filter_refs<16>(ref, reff);

    static const int kModes[4] = {kDc, kHor, kVer, kPlanar};
    uint8_t pred[5][256];   // 4 intra candidates + the inter reference
    int best = 0;
    long best_sad = LONG_MAX;
    for (int m = 0; m < 4; ++m) {
      predict<16>(kModes[m], kModes[m] == kPlanar ? reff : ref, 0, pred[m]);
      long sad = 0;
      for (int yy = 0; yy < 16; ++yy)
        for (int xx = 0; xx < 16; ++xx) {
          int d = sy[static_cast<size_t>(y0 + yy) * ypitch + x0 + xx] -
                  pred[m][yy * 16 + xx];
          sad += d < 0 ? -d : d;
        }
      if (sad < best_sad) {
        best_sad = sad;
        best = m;
      }
    }
    const int mode = kModes[best];
    luma_mode[cy * ctb_w + cx] = static_cast<uint8_t>(mode);

    bool is_inter = false;
    if (p_slice) {
      // reference reads are the coded-size recon plane, unclamped
      long sad_inter = 0;
      for (int yy = 0; yy < 16; ++yy)
        for (int xx = 0; xx < 16; ++xx) {
          const size_t o = static_cast<size_t>(y0 + yy) * ypitch + x0 + xx;
          int d = sy[o] - ry[o];
          sad_inter += d < 0 ? -d : d;
          pred[4][yy * 16 + xx] = ry[o];
        }
      is_inter = sad_inter <= best_sad;
      if (is_inter) best = 4;
    }
    // HM rounding: 171/512 intra, 85/512 inter, in all three planes
    const int round = is_inter ? 85 : 171;

    int16_t res[256], coef[256];
    TbData<16> yb;
    for (int yy = 0; yy < 16; ++yy)
      for (int xx = 0; xx < 16; ++xx)
        res[yy * 16 + xx] =
            static_cast<int16_t>(
                sy[static_cast<size_t>(y0 + yy) * ypitch + x0 + xx] -
                pred[best][yy * 16 + xx]);
    fwd_transform<16>(res, 16, coef);
    yb.cbf = quantize<16>(coef, qp, yb.level, round) != 0;
    if (yb.cbf) {
      int16_t deq[256], rres[256];
      dequantize<16>(yb.level, qp, deq);
      inv_transform<16>(deq, rres, 16);
      for (int yy = 0; yy < 16; ++yy)
        for (int xx = 0; xx < 16; ++xx)
          ry[static_cast<size_t>(y0 + yy) * ypitch + x0 + xx] =
              clip8(pred[best][yy * 16 + xx] + rres[yy * 16 + xx]);
    } else {
      for (int yy = 0; yy < 16; ++yy)
        std::memcpy(&ry[static_cast<size_t>(y0 + yy) * ypitch + x0],
                    &pred[best][yy * 16], 16);
    }

    if (fullcolor) {
      encode_ctu_chroma444(cab, bank, x0, y0, av, qp, mode, left_avail,
                           left_mode, yb);
      return;
    }

    // --- chroma (DM mode), 8x8 TBs
    const int qpc = chroma_qp(qp);
    TbData<8> cbb, crb;
    uint8_t cpred[2][64];
    const int cx0 = x0 / 2, cy0 = y0 / 2;
    for (int pl = 0; pl < 2; ++pl) {
      uint8_t* rp = pl ? rcr.data() : rcb.data();
      const uint8_t* sp = pl ? scr.data() : scb.data();
      TbData<8>& tb = pl ? crb : cbb;
      uint8_t cref[33];
      if (is_inter) {
        for (int yy = 0; yy < 8; ++yy)
          std::memcpy(&cpred[pl][yy * 8],
                      &rp[static_cast<size_t>(cy0 + yy) * cpitch + cx0], 8);
      } else {
        build_refs<8>(rp, cpitch, cx0, cy0, av, cref);
        predict<8>(mode, cref, 1, cpred[pl]);
      }
      int16_t cres[64], ccoef[64];
      for (int yy = 0; yy < 8; ++yy)
        for (int xx = 0; xx < 8; ++xx)
          cres[yy * 8 + xx] = static_cast<int16_t>(
              sp[static_cast<size_t>(cy0 + yy) * cpitch + cx0 + xx] -
              cpred[pl][yy * 8 + xx]);
      fwd_transform<8>(cres, 8, ccoef);
      tb.cbf = quantize<8>(ccoef, qpc, tb.level, round) != 0;
      if (tb.cbf) {
        int16_t deq[64], rres[64];
        dequantize<8>(tb.level, qpc, deq);
        inv_transform<8>(deq, rres, 8);
        for (int yy = 0; yy < 8; ++yy)
          for (int xx = 0; xx < 8; ++xx)
            rp[static_cast<size_t>(cy0 + yy) * cpitch + cx0 + xx] =
                clip8(cpred[pl][yy * 8 + xx] + rres[yy * 8 + xx]);
      } else {
        for (int yy = 0; yy < 8; ++yy)
          std::memcpy(&rp[static_cast<size_t>(cy0 + yy) * cpitch + cx0],
                      &cpred[pl][yy * 8], 8);
      }
    }

    // --- CABAC bins for the CTU (shared emission path, entropy.h)
    if (!p_slice) {
      code_ctu_syntax(cab, bank, mode, left_avail ? left_mode : -1, yb.cbf,
                      cbb.cbf, crb.cbf, yb.level, cbb.level, crb.level);
      return;
    }
    // inter with no coded residual is a skip (recon == reference already)
    const int kind = !is_inter                          ? kCtuIntra
                     : (yb.cbf || cbb.cbf || crb.cbf) ? kCtuMerge
                                                      : kCtuSkip;
    if (is_inter) luma_mode[cy * ctb_w + cx] = static_cast<uint8_t>(kind);
    code_ctu_syntax_p(cab, bank, kind, left_avail && left_mode == kCtuSkip,
                      mode, left_avail && left_mode < 35 ? left_mode : -1,
                      yb.cbf, cbb.cbf, crb.cbf, yb.level, cbb.level,
                      crb.level);
  }

  // 4:4:4 chroma (DM mode): Cb and Cr are 16x16 TBs coded like luma with
  // cIdx 1/2, then the CTU's bins are emitted.
  void encode_ctu_chroma444(CabacEncoder& cab, ContextBank& bank, int x0,
                            int y0, const Avail& av, int qp, int mode,
                            bool left_avail, uint8_t left_mode,
                            const TbData<16>& yb) {
    // ChromaArrayType != 1: QpC = Min(qPi, 51), not the Table 8-10 map
    const int qpc = chroma_qp_444(qp);
    TbData<16> tb[2];
    for (int pl = 0; pl < 2; ++pl) {
      uint8_t* rp = pl ? rcr.data() : rcb.data();
      const uint8_t* sp = pl ? scr.data() : scb.data();
      uint8_t cref[65], creff[65], cpred[256];
      build_refs<16>(rp, cpitch, x0, y0, av, cref);
      // §8.4.4.2.3: neighbour smoothing applies when cIdx == 0 or
      // ChromaArrayType == 3. At nTbS 16 the threshold is 1: Planar
      // (distance 10) filters, DC/H/V (exempt / distance 0) do not.
      // The DC edge filter and H/V boundary adjust stay cIdx == 0 only
      // (predict<> with cidx 1).
      const bool filt = mode == kPlanar;
      if (filt) filter_refs<16>(cref, creff);
      predict<16>(mode, filt ? creff : cref, 1, cpred);
      int16_t cres[256], ccoef[256];
      for (int yy = 0; yy < 16; ++yy)
        for (int xx = 0; xx < 16; ++xx)
          cres[yy * 16 + xx] = static_cast<int16_t>(
              sp[static_cast<size_t>(y0 + yy) * cpitch + x0 + xx] -
              cpred[yy * 16 + xx]);
      fwd_transform<16>(cres, 16, ccoef);
      tb[pl].cbf = quantize<16>(ccoef, qpc, tb[pl].level) != 0;
      if (tb[pl].cbf) {
        int16_t deq[256], rres[256];
        dequantize<16>(tb[pl].level, qpc, deq);
        inv_transform<16>(deq, rres, 16);
        for (int yy = 0; yy < 16; ++yy)
          for (int xx = 0; xx < 16; ++xx)
            rp[static_cast<size_t>(y0 + yy) * cpitch + x0 + xx] =
                clip8(cpred[yy * 16 + xx] + rres[yy * 16 + xx]);
      } else {
        for (int yy = 0; yy < 16; ++yy)
          std::memcpy(&rp[static_cast<size_t>(y0 + yy) * cpitch + x0],
                      &cpred[yy * 16], 16);
      }
    }
    code_ctu_syntax(cab, bank, mode, left_avail ? left_mode : -1, yb.cbf,
                    tb[0].cbf, tb[1].cbf, yb.level, tb[0].level, tb[1].level,
                    true);
  }
};

StripeEncoder::StripeEncoder(int width, int height, int slices_per_row,
                             bool fullcolor, bool inter)
    : impl_(new Impl(width, height, slices_per_row, fullcolor, inter)),
      width_(width),
      height_(height) {}

StripeEncoder::~StripeEncoder() = default;

const uint8_t* StripeEncoder::recon_y() const { return impl_->ry.data(); }
const uint8_t* StripeEncoder::recon_cb() const { return impl_->rcb.data(); }
const uint8_t* StripeEncoder::recon_cr() const { return impl_->rcr.data(); }
int StripeEncoder::recon_ypitch() const { return impl_->ypitch; }
int StripeEncoder::recon_cpitch() const { return impl_->cpitch; }

void StripeEncoder::encode_frame(const uint8_t* y, int ypitch,
                                 const uint8_t* cb, const uint8_t* cr,
                                 int cpitch, int qp,
                                 std::vector<uint8_t>& out,
                                 EncodeStats* stats, bool force_idr) {
  Impl& im = *impl_;
  qp = std::clamp(qp, 0, 51);
  im.load_source(y, ypitch, cb, cr, cpitch);
  const bool p_slice = im.inter && im.have_ref && !force_idr;
  if (!p_slice) {
    // IDR: POC 0, parameter sets in front. P emissions carry none.
    im.poc = 0;
    out.insert(out.end(), im.ps_cache.begin(), im.ps_cache.end());
  }
  const int poc_lsb = im.poc & 255;

  // one slice segment per CTU row (split into slices_per_row segments)
  for (int cy = 0; cy < im.ctb_h; ++cy) {
    int per = ceil_div(im.ctb_w, im.slices_per_row);
    for (int s0 = 0; s0 < im.ctb_w; s0 += per) {
      int s1 = std::min(s0 + per, im.ctb_w);
      BitWriter bw;
      bool first = (cy == 0 && s0 == 0);
      if (p_slice)
        write_p_slice_header(bw, first, cy * im.ctb_w + s0, im.addr_bits, qp,
                             poc_lsb);
      else
        write_slice_header(bw, first, cy * im.ctb_w + s0, im.addr_bits, qp);
      std::vector<uint8_t> cabac_bytes;
      CabacEncoder cab(cabac_bytes);
      ContextBank bank;
      bank.init(qp, p_slice ? 1 : 0);
      uint8_t left_mode = kDc;
      for (int cx = s0; cx < s1; ++cx) {
        im.encode_ctu(cab, bank, cx, cy, cx > s0, qp, left_mode, p_slice);
        left_mode = im.luma_mode[cy * im.ctb_w + cx];
        cab.encode_terminate(cx == s1 - 1 ? 1 : 0);
      }
      auto tail = cab.finish();
      for (uint8_t b : cabac_bytes) bw.u(b, 8);
      bw.u(tail.bits, tail.nbits);
      // rbsp_slice_segment_trailing_bits: stop bit + alignment
      bw.rbsp_trailing();
      emit_nal(bw, out, p_slice ? kNalTrailR : kNalIdr);
    }
  }
  // POC advances per coded picture of this stripe (8 lsb bits on the wire)
  ++im.poc;
  im.have_ref = true;
  if (stats) {
    stats->idr = !p_slice;
    stats->frame_qp = qp;
    stats->ctu_count = im.ctb_w * im.ctb_h;
    stats->bytes = out.size();
  }
}

}  // namespace hevc
}  // namespace hipflux
