// pfb_synth_wave_dadaout.hip — the Nf = 256 wave synthesis storing its output as a DADA data
// section (synth_wave_dadaout_kernel, pfb_synth_wave.hpp; pfb_synthesis_execute_to_dada and its
// twins).  The production form only — stored stage-1 rows, pass-1 lanes spread over the
// workgroup, kept-register stores, priority schedule 1 — for W 224 / 192 x spans-Nyquist /
// critical x flat / general window x NBIT 8 / 16 / 32 out: 24 kernels, in a translation unit of
// their own so that they compile beside pfb_synth_wave.hip.  The input side is the channel
// IFFT's launch, so every input form (cf32, strided, a DADA section) combines with these.
#include "pfb_synth_wave.hpp"

namespace pfb {

bool synth_wave_dadaout_supported(const SynthBlockArgs& a, int nbit) {
  if (nbit != 8 && nbit != 16 && nbit != 32) return false;
  // the shapes launch_synth_wave sends to the kept-register kernel on stored rows
  if (a.fir_x || a.zblk == 0 || !synth_wave_supported(a)) return false;
  if (a.Lov != 3 * (a.W / 16) * a.N) return false;
  // every byte offset the store forms lies within one block's L samples of the section
  // (pfb_synth_wave.hpp, store_block), which must fit one descriptor: L >= Lkeep
  return (int64_t)a.L * a.n_pol * (nbit / 4) <= kRsrcMaxBytes;
}

namespace {

template <int RW, bool SPANS, bool WFLAT>
hipError_t launch_dadaout(const SynthBlockArgs& a, hipStream_t s) {
  void (*kern)(SynthBlockArgs) = nullptr;
  switch (a.dout_nbit) {
    case 8: kern = synth_wave_dadaout_kernel<RW, SPANS, WFLAT, OutDada8>; break;
    case 16: kern = synth_wave_dadaout_kernel<RW, SPANS, WFLAT, OutDada16>; break;
    case 32: kern = synth_wave_dadaout_kernel<RW, SPANS, WFLAT, OutDada32>; break;
    default: return hipErrorInvalidValue;
  }
  hipError_t e = set_lds(kern, kLdsB);
  if (e != hipSuccess) return e;
  // launch_wave_t's grid: 3 resident workgroups per CU, contiguous block ranges
  const int groups = a.N / kCols;
  const int per_cu = std::max(1, std::min(3, (160 * 1024) / kLdsB));
  int ranges = std::max(1, cu_count() * per_cu / (groups * a.n_pol));
  ranges = std::min(ranges, a.n_blocks);
  dim3 grid((unsigned)(groups * ranges), (unsigned)a.n_pol);
  return launch_kernel(kern, grid, dim3(kWgThreads), kLdsB, s, a);
}

template <int RW, bool SPANS>
hipError_t launch_dadaout_w(const SynthBlockArgs& a, hipStream_t s) {
  return a.win_flat ? launch_dadaout<RW, SPANS, true>(a, s) : launch_dadaout<RW, SPANS, false>(a, s);
}

}  // namespace

hipError_t launch_synth_wave_dadaout(const SynthBlockArgs& a, hipStream_t s) {
  if (a.n_blocks <= 0) return hipSuccess;
  if (!a.dout || !synth_wave_dadaout_supported(a, a.dout_nbit)) return hipErrorInvalidValue;
  if (a.W == 224) return a.spans ? launch_dadaout_w<14, true>(a, s) : launch_dadaout_w<14, false>(a, s);
  return a.spans ? launch_dadaout_w<12, true>(a, s) : launch_dadaout_w<12, false>(a, s);
}

}  // namespace pfb
