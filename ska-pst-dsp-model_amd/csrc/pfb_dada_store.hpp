// pfb_dada_store.hpp — the store classes of the kernels that write a DADA data section
// themselves: the streaming analysis (analysis_stream_body's OUT, pfb_ana_stream.hpp) and the
// Nf = 256 wave synthesis (synth_wave_body's OUT, pfb_synth_wave.hpp).  One definition, so both
// convert with pfb_dada_pack's to_sample and produce its bytes.
#pragma once
#include "pfb_common.hpp"
#include "pfb_sample.hpp"

namespace pfb {

// OutCf32: the kernel's packed complex float32 product (its own stores).
// OutDada8 / 16 / 32: a TFP DADA section, NDIM 2 — kBytes per complex sample, (re, im)
// converted by to_sample and written by one range-checked buffer store at byte `off` of the
// descriptor.  AUX: the store's cache policy (the analysis: kAuxDadaOut, the default; the
// synthesis: kAuxSynDadaOut).
struct OutCf32 {
  static constexpr bool kDada = false;
};
struct OutDada32 {  // NBIT 32: float (re, im)
  static constexpr bool kDada = true;
  static constexpr int kBytes = 8;
  template <int AUX = kAuxDadaOut>
  static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, float re, float im,
                                               uint32_t soff = 0) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v2f{to_sample<float>(re), to_sample<float>(im)}),
                                          r, off, soff, AUX);
  }
};
struct OutDada16 {  // NBIT 16: int16 (re, im)
  static constexpr bool kDada = true;
  static constexpr int kBytes = 4;
  template <int AUX = kAuxDadaOut>
  static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, float re, float im,
                                               uint32_t soff = 0) {
    const uint32_t w = (uint32_t)(uint16_t)to_sample<int16_t>(re) | ((uint32_t)(uint16_t)to_sample<int16_t>(im) << 16);
    __builtin_amdgcn_raw_buffer_store_b32(w, r, off, soff, AUX);
  }
};
struct OutDada8 {  // NBIT 8: int8 (re, im)
  static constexpr bool kDada = true;
  static constexpr int kBytes = 2;
  template <int AUX = kAuxDadaOut>
  static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, float re, float im,
                                               uint32_t soff = 0) {
    const uint16_t w = (uint16_t)((uint16_t)(uint8_t)to_sample<int8_t>(re) | ((uint16_t)(uint8_t)to_sample<int8_t>(im) << 8));
    __builtin_amdgcn_raw_buffer_store_b16(w, r, off, soff, AUX);
  }
};

}  // namespace pfb
