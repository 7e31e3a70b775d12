// pfb_sample.hpp — the float32 -> DADA sample conversion shared by pfb_dada_pack
// (pfb_layout.hip) and the analysis kernels that store DADA samples themselves
// (pfb_ana_stream.hpp): one definition, so both produce the same bytes.
#pragma once

#include <hip/hip_runtime.h>

#include <limits>
#include <type_traits>

namespace pfb {

// Matlab cast(single -> intN): round half away from zero, saturate, NaN -> 0
template <class T>
__device__ __forceinline__ T to_sample(float v) {
  if constexpr (std::is_same<T, float>::value) {
    return v;
  } else if constexpr (std::is_same<T, double>::value) {
    return (double)v;
  } else {
    constexpr float lo = (float)std::numeric_limits<T>::min();
    constexpr float hi = (float)std::numeric_limits<T>::max();
    if (v != v) return (T)0;
    const float r = roundf(v);
    return (T)fminf(fmaxf(r, lo), hi);
  }
}

}  // namespace pfb
