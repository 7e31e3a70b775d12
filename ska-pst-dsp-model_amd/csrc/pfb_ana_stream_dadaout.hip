// pfb_ana_stream_dadaout.hip — the streaming analysis kernel storing its product as a DADA
// data section (analysis_stream_dadaout_kernel, pfb_ana_stream.hpp; pfb_analysis_execute_to_dada
// and its twins).  The five streaming shapes x {cf32 input x NBIT 8 / 16 / 32 out, DADA input
// of NBIT b x the same b out, DADA input of NBIT 8 / 16 x NBIT 32 out — an integer file
// channelised into a float one, harness.channelize}: 40 kernels, in a translation unit of their
// own so that they compile beside pfb_analysis.hip.
#include "pfb_ana_stream.hpp"

namespace pfb {

bool dadaout_reads_dada(int in_nbit, int out_nbit) {
  if (in_nbit != 8 && in_nbit != 16 && in_nbit != 32) return false;
  return in_nbit == out_nbit || out_nbit == 32;
}

namespace {

template <int N, int P, int NU, int DE, bool LCBF>
hipError_t launch_dadaout(const AnalysisArgs& a, hipStream_t s) {
  using SH = StreamShape<N, P, NU, DE>;
  // the plain product only; a section read in place has the output's sample size (another
  // NBIT is unpacked by the caller and comes in as cf32)
  if (!a.dout || a.z || a.out_rs != 0) return hipErrorInvalidValue;
  if (a.din && !dadaout_reads_dada(a.din_nbit, a.dout_nbit)) return hipErrorInvalidValue;
  void (*kern)(AnalysisArgs) = nullptr;
  if (a.din && a.din_nbit != a.dout_nbit) {
    // an integer file channelised into an NBIT 32 one
    kern = a.din_nbit == 8 ? analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InDada8, OutDada32>
                           : analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InDada16, OutDada32>;
  } else
  switch (a.dout_nbit) {
    case 8:
      kern = a.din ? analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InDada8, OutDada8>
                   : analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InCf32, OutDada8>;
      break;
    case 16:
      kern = a.din ? analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InDada16, OutDada16>
                   : analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InCf32, OutDada16>;
      break;
    case 32:
      kern = a.din ? analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InDada32, OutDada32>
                   : analysis_stream_dadaout_kernel<N, P, NU, DE, LCBF, InCf32, OutDada32>;
      break;
    default: return hipErrorInvalidValue;
  }
  // one 16-row step of the section (both polarisations) lies within a descriptor
  if ((int64_t)SH::T * (LCBF ? 216 : N) * a.n_pol * (a.dout_nbit / 4) > kRsrcMaxBytes) return hipErrorInvalidValue;
  // (the carry: launch_stream's bound)
  if (a.pre && (a.pad < 0 || a.pad > (int64_t)SH::WIN * N)) return hipErrorInvalidValue;
  hipError_t e = set_lds(kern, SH::lds_bytes);
  if (e != hipSuccess) return e;
  StreamGrid sg;
  e = stream_grid<SH, NU>(a, &sg);
  if (e != hipSuccess) return e;
  if (sg.wgs > INT32_MAX) return hipErrorInvalidValue;
  dim3 grid((unsigned)sg.wgs, (unsigned)a.n_pol);
  return launch_kernel(kern, grid, dim3(NT), SH::lds_bytes, s, a);
}

}  // namespace

hipError_t launch_stream_dadaout(const AnalysisArgs& a, bool lcbf, hipStream_t s) {
  if (a.K <= a.row0) return hipSuccess;
  if (a.variant != kBunton || a.N != 256) return hipErrorInvalidValue;
  if (lcbf) {
    if (a.M != 192 || a.P != 12 || a.nu != 4) return hipErrorInvalidValue;
    return launch_dadaout<256, 12, 4, 3, true>(a, s);
  }
  if (a.nu == 8 && a.M == 224) {
    if (a.P == 13) return launch_dadaout<256, 13, 8, 7, false>(a, s);
    if (a.P == 12) return launch_dadaout<256, 12, 8, 7, false>(a, s);
  }
  if (a.nu == 4 && a.M == 192) {
    if (a.P == 13) return launch_dadaout<256, 13, 4, 3, false>(a, s);
    if (a.P == 12) return launch_dadaout<256, 12, 4, 3, false>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace pfb
