// pfb_ana_stream_rtdada.hip — the streaming analysis kernel of the file-to-file round trip
// (analysis_stream_rt_dada_kernel, pfb_ana_stream.hpp; pfb_roundtrip_execute_dada_to_dada and
// its analysis half): it reads a single-channel DADA section in place, stores the channelised
// product as an NBIT 32 float section and emits the synthesis stage-1 rows in 2-row runs, all in
// one launch.  The four round-trip shapes of the streaming kernel x NBIT 8 / 16 / 32 in: 12
// kernels, in a translation unit of their own so that they compile beside pfb_analysis.hip.
#include "pfb_ana_stream.hpp"

namespace pfb {

namespace {

bool rt_dada_shape(const AnalysisArgs& a) {
  if (a.variant != kBunton || a.N != 256) return false;
  if (a.nu == 8 && a.M == 224) return a.P == 13 || a.P == 12;
  if (a.nu == 4 && a.M == 192) return a.P == 13 || a.P == 12;
  return false;
}

template <int N, int P, int NU, int DE>
hipError_t launch_rt_dada(const AnalysisArgs& a, hipStream_t s) {
  using SH = StreamShape<N, P, NU, DE>;
  void (*kern)(AnalysisArgs) = a.din_nbit == 8    ? analysis_stream_rt_dada_kernel<N, P, NU, DE, InDada8>
                               : a.din_nbit == 16 ? analysis_stream_rt_dada_kernel<N, P, NU, DE, InDada16>
                                                  : analysis_stream_rt_dada_kernel<N, P, NU, DE, InDada32>;
  hipError_t e = set_lds(kern, SH::lds_bytes);
  if (e != hipSuccess) return e;
  // (launch_stream's sizing: the resident workgroup count and the descriptor fit)
  StreamGrid sg;
  e = stream_grid<SH, NU>(a, &sg);
  if (e != hipSuccess) return e;
  if (sg.wgs > INT32_MAX) return hipErrorInvalidValue;
  dim3 grid((unsigned)sg.wgs, (unsigned)a.n_pol);
  return launch_kernel(kern, grid, dim3(NT), SH::lds_bytes, s, a);
}

}  // namespace

bool stream_rt_dada_supported(const AnalysisArgs& a, int in_nbit) {
  if (in_nbit != 8 && in_nbit != 16 && in_nbit != 32) return false;
  if (!rt_dada_shape(a) || knob("PFB_ANALYSIS_NO_STREAM") != nullptr || a.n_pol < 1) return false;
  // one workgroup's rows of the input section fit a descriptor (analysis_reads_dada's limit),
  // and so does one 16-row step of the float product section, both polarisations
  // (launch_stream_dadaout's)
  if ((int64_t)a.n_pol * (in_nbit / 4) * a.N * 512 > kRsrcMaxBytes) return false;
  return (int64_t)16 * a.N * a.n_pol * 8 <= kRsrcMaxBytes;
}

hipError_t launch_stream_rt_dada(const AnalysisArgs& a, hipStream_t s) {
  if (a.K <= a.row0) return hipSuccess;
  if (!stream_rt_dada_supported(a, a.din_nbit)) return hipErrorInvalidValue;
  // a section in, the float section and the 2-row runs out — nothing else: no carry, no read
  // offset, no strided product
  if (!a.din || !a.dout || a.dout_nbit != 32 || !a.z || a.zblk != 2) return hipErrorInvalidValue;
  if (a.pre || a.pad != 0 || a.carry_out || a.out_rs != 0) return hipErrorInvalidValue;
  // every step's 16 rows are whole runs of the stage-1 buffer (analysis_stream_body, ZOUT >= 2)
  if ((a.row0 - a.z_row0) % 16 != 0) return hipErrorInvalidValue;
  if (a.nu == 8) return a.P == 13 ? launch_rt_dada<256, 13, 8, 7>(a, s) : launch_rt_dada<256, 12, 8, 7>(a, s);
  return a.P == 13 ? launch_rt_dada<256, 13, 4, 3>(a, s) : launch_rt_dada<256, 12, 4, 3>(a, s);
}

}  // namespace pfb
