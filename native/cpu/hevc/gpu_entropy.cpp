// HEVC bitstream assembly from GPU buffers (see gpu_entropy.h).
#include "gpu_entropy.h"

#include "../../hip/hevc_gpu_layout.h"
#include "cabac.h"
#include "entropy.h"
#include "headers.h"

namespace hipflux {
namespace hevc {

void assemble_hevc_slice_nal(const uint8_t* cabac_bytes, int n_bytes,
                             int tail_bits, int tail_nbits, bool first_slice,
                             int slice_addr, int addr_bits, int qp,
                             std::vector<uint8_t>& out, int slice_type,
                             int poc_lsb) {
  BitWriter bw;
  if (slice_type == 1)
    write_p_slice_header(bw, first_slice, slice_addr, addr_bits, qp, poc_lsb);
  else
    write_slice_header(bw, first_slice, slice_addr, addr_bits, qp);
  bw.append_bytes(cabac_bytes, static_cast<size_t>(n_bytes));
  bw.u(static_cast<uint32_t>(tail_bits), tail_nbits);
  bw.rbsp_trailing();
  emit_nal(bw, out, slice_type == 1 ? kNalTrailR : kNalIdr);
}

void encode_hevc_job_nal(const int16_t* levels, const int* meta, int ctbw,
                         int ctu_row, int ctu_x0, int seg_w, int qp,
                         bool first_slice, int slice_addr, int addr_bits,
                         std::vector<uint8_t>& out, bool fullcolor,
                         int slice_type, int poc_lsb) {
  std::vector<uint8_t> cabac_bytes;
  CabacEncoder cab(cabac_bytes);
  ContextBank bank;
  const bool p_slice = slice_type == 1;
  bank.init(qp, p_slice ? 1 : 0);
  int left_mode = -1;
  bool left_skip = false;
  const int stride = fullcolor ? hevcgpu::kHevcLevelsPerCtu444
                               : hevcgpu::kHevcLevelsPerCtu;
  for (int ci = 0; ci < seg_w; ++ci) {
    const size_t mb = static_cast<size_t>(ctu_row) * ctbw + ctu_x0 + ci;
    const int mode = meta[mb * hevcgpu::kHevcMetaPerCtu + 0];
    const int cbf = meta[mb * hevcgpu::kHevcMetaPerCtu + 1];
    const int16_t* lv = levels + mb * stride;
    if (p_slice) {
      // meta +0 is the intra mode, or a CtuKind for inter CTUs
      const int kind = mode < 35 ? kCtuIntra : mode;
      code_ctu_syntax_p(cab, bank, kind, left_skip, mode, left_mode, cbf & 1,
                        cbf & 2, cbf & 4, lv, lv + 256, lv + 320);
      left_skip = kind == kCtuSkip;
      left_mode = kind == kCtuIntra ? mode : -1;
    } else {
      code_ctu_syntax(cab, bank, mode, left_mode, cbf & 1, cbf & 2, cbf & 4,
                      lv, lv + 256, lv + (fullcolor ? 512 : 320), fullcolor);
      left_mode = mode;
    }
    cab.encode_terminate(ci == seg_w - 1 ? 1 : 0);
  }
  auto tail = cab.finish();
  assemble_hevc_slice_nal(cabac_bytes.data(),
                          static_cast<int>(cabac_bytes.size()), tail.bits,
                          tail.nbits, first_slice, slice_addr, addr_bits, qp,
                          out, slice_type, poc_lsb);
}

void write_hevc_stripe_headers(int coded_w, int coded_h, int vis_w,
                               int vis_h, std::vector<uint8_t>& out,
                               bool fullcolor, bool inter) {
  write_vps_nal(out, level_idc_for(coded_w, coded_h), fullcolor, inter);
  write_sps_nal(out, coded_w, coded_h, vis_w, vis_h, fullcolor, inter);
  write_pps_nal(out);
}

}  // namespace hevc
}  // namespace hipflux
