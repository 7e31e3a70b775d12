// pfb_ana_stream_quant.hip — the quantised FilterBank output (FilterBank.m:106-113,
// pfb_analysis_execute_quantised_to_dada and its twins): the streaming analysis kernel that
// also sums the moments of the product it stores (analysis_stream_moments_kernel,
// pfb_ana_stream.hpp; the five streaming shapes x {cf32, DADA 8 / 16 / 32 input}: 20 kernels),
// the same moments from a stored product (moments_partials_kernel, the STAGED side), the kernel
// that turns the partial sums into the scale (moments_finish_kernel), and the one pass that
// rounds, scales, casts and interleaves the product into the TFP section
// (quantise_pack_kernel).  No floating-point atomics: every partial sum has a slot of its own
// and every sum a fixed order, so the same plan, input and grid give the same scale bits.
#include "pfb_ana_stream.hpp"

namespace pfb {

namespace {

constexpr int QT = kOneShotThreads;

template <int N, int P, int NU, int DE, bool LCBF>
void (*moments_kernel_of(const AnalysisArgs& a))(AnalysisArgs) {
  if (!a.din) return analysis_stream_moments_kernel<N, P, NU, DE, LCBF, InCf32>;
  return a.din_nbit == 8    ? analysis_stream_moments_kernel<N, P, NU, DE, LCBF, InDada8>
         : a.din_nbit == 16 ? analysis_stream_moments_kernel<N, P, NU, DE, LCBF, InDada16>
                            : analysis_stream_moments_kernel<N, P, NU, DE, LCBF, InDada32>;
}

// slots = nullptr: launch; else only the grid's n_pol x nw
template <int N, int P, int NU, int DE, bool LCBF>
hipError_t launch_moments(const AnalysisArgs& a, hipStream_t s, int64_t* slots) {
  using SH = StreamShape<N, P, NU, DE>;
  // the plain cf32 product only
  if (a.dout || a.z || a.out_rs != 0) return hipErrorInvalidValue;
  if (a.din && a.din_nbit != 8 && a.din_nbit != 16 && a.din_nbit != 32) return hipErrorInvalidValue;
  StreamGrid sg;
  hipError_t e = stream_grid<SH, NU>(a, &sg);
  if (e != hipSuccess) return e;
  if (sg.wgs > INT32_MAX) return hipErrorInvalidValue;
  if (slots) {
    *slots = sg.wgs * a.n_pol;
    return hipSuccess;
  }
  if (!a.mom || !a.out) return hipErrorInvalidValue;
  // (the carry: launch_stream's bound)
  if (a.pre && (a.pad < 0 || a.pad > (int64_t)SH::WIN * N)) return hipErrorInvalidValue;
  auto kern = moments_kernel_of<N, P, NU, DE, LCBF>(a);
  e = set_lds(kern, SH::lds_bytes);
  if (e != hipSuccess) return e;
  dim3 grid((unsigned)sg.wgs, (unsigned)a.n_pol);
  return launch_kernel(kern, grid, dim3(NT), SH::lds_bytes, s, a);
}

hipError_t moments_any(const AnalysisArgs& a, bool lcbf, hipStream_t s, int64_t* slots) {
  if (a.variant != kBunton || a.N != 256) return hipErrorInvalidValue;
  if (lcbf) {
    if (a.M != 192 || a.P != 12 || a.nu != 4) return hipErrorInvalidValue;
    return launch_moments<256, 12, 4, 3, true>(a, s, slots);
  }
  if (a.nu == 8 && a.M == 224) {
    if (a.P == 13) return launch_moments<256, 13, 8, 7, false>(a, s, slots);
    if (a.P == 12) return launch_moments<256, 12, 8, 7, false>(a, s, slots);
  }
  if (a.nu == 4 && a.M == 192) {
    if (a.P == 13) return launch_moments<256, 13, 4, 3, false>(a, s, slots);
    if (a.P == 12) return launch_moments<256, 12, 4, 3, false>(a, s, slots);
  }
  return hipErrorInvalidValue;
}

// The moments of a stored product x[pol][0, n) (the STAGED side): workgroup w of polarisation p
// sums the kMomV x QT 16-byte pairs from pair w kMomV QT on and stores its three doubles at
// mom[(p nw + w) 3 ...] — the streaming kernel's slot layout.  One-shot grid; n and the pol
// stride are even and x is 16-B aligned (the launcher checks).
constexpr int kMomV = kMomLoads;
__global__ void __launch_bounds__(QT) moments_partials_kernel(const float2* __restrict__ x, int64_t ps, int64_t n,
                                                              double* __restrict__ mom) {
  __shared__ double red[12];
  const float4* row = reinterpret_cast<const float4*>(x + blockIdx.y * ps);
  const int64_t n2 = n / 2;
  const int64_t i0 = (int64_t)blockIdx.x * (kMomV * QT) + threadIdx.x;
  float4 v[kMomV];
#pragma unroll
  for (int u = 0; u < kMomV; ++u)  // the thread's loads in flight together
    v[u] = i0 + u * QT < n2 ? row[i0 + u * QT] : make_float4(0.f, 0.f, 0.f, 0.f);
  double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < kMomV; ++u) {
    const double a = v[u].x, b = v[u].y, c = v[u].z, d = v[u].w;
    m[0] += a;
    m[1] += b;
    m[2] = fma(a, a, fma(b, b, m[2]));
    m[0] += c;
    m[1] += d;
    m[2] = fma(c, c, fma(d, d, m[2]));
  }
  wg_sum3(m, red);
  if (threadIdx.x == 0) {
    double* slot = mom + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    slot[0] = m[0];
    slot[1] = m[1];
    slot[2] = m[2];
  }
}

// One workgroup: thread t adds slots t, t + QT, ... in index order, the workgroup's sums go
// through wg_sum3's fixed tree, and thread 0 forms the scale (pfb_quantize's expression; a zero
// variance is not special-cased) and writes stats = {sum re, sum im, s2, scale}.  Reads the
// `slots` slots of the launch that just ran and no other.
__global__ void __launch_bounds__(QT) moments_finish_kernel(const double* __restrict__ mom, int64_t slots, double cnt,
                                                            double rms, double* __restrict__ stats) {
  __shared__ double red[12];
  double m[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < slots; i += QT) {
    m[0] += mom[i * 3 + 0];
    m[1] += mom[i * 3 + 1];
    m[2] += mom[i * 3 + 2];
  }
  wg_sum3(m, red);
  if (threadIdx.x == 0) {
    const double m2 = (m[0] * m[0] + m[1] * m[1]) / cnt;
    const double var = (m[2] - m2) / (cnt - 1.0);  // var(x, 0, "all")
    stats[0] = m[0];
    stats[1] = m[1];
    stats[2] = m[2];
    stats[3] = rms / sqrt(var);
  }
}

// The rounding pass: thread i takes elements (k, c) = 4 i .. 4 i + 3 of every polarisation (two
// 16-byte loads each) and writes their 4 x NP complex samples, which are contiguous in the TFP
// section (polarisations interleaved): one run of 8 NP sizeof(T) bytes, as 16-byte stores (8 for
// NBIT 8 single-pol) when `vec` says the section is aligned to them, else one store per
// component.  Per component to_sample(oscale * roundf(sf * x)): pfb_quantize, the caller's
// float32 scale and pfb_dada_pack, in that order.  NP: 1, 2, or 0 for any count (per-component
// stores).  Writes elements [0, n) of the section and no byte beyond; n is a multiple of 4.
template <class T, int NP>
__global__ void __launch_bounds__(QT) quantise_pack_kernel(const float2* __restrict__ x, int64_t ps, int64_t n,
                                                           int n_pol, const double* __restrict__ stats, float oscale,
                                                           T* __restrict__ out, int vec) {
  const int64_t i0 = ((int64_t)blockIdx.x * QT + threadIdx.x) * 4;
  if (i0 >= n) return;
  const float sf = stats ? (float)stats[3] : 1.0f;  // (uniform: one scalar load per wave)
  auto q = [&](float v) { return to_sample<T>(oscale * roundf(sf * v)); };
  if constexpr (NP == 0) {
    for (int p = 0; p < n_pol; ++p) {
      const float4* src = reinterpret_cast<const float4*>(x + p * ps + i0);
      const float4 a = src[0], b = src[1];
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t o = ((i0 + e) * n_pol + p) * 2;
        out[o] = q(v[2 * e]);
        out[o + 1] = q(v[2 * e + 1]);
      }
    }
  } else {
    constexpr int NV = 4 * NP * 2;
    constexpr int BYTES = NV * (int)sizeof(T);
    constexpr int CH = BYTES >= 16 ? 16 : 8;
    T vals[NV];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float4* src = reinterpret_cast<const float4*>(x + p * ps + i0);
      const float4 a = src[0], b = src[1];
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vals[(e * NP + p) * 2] = q(v[2 * e]);
        vals[(e * NP + p) * 2 + 1] = q(v[2 * e + 1]);
      }
    }
    T* dst = out + i0 * NP * 2;
    if (vec) {
#pragma unroll
      for (int k = 0; k < BYTES / CH; ++k) {
        if constexpr (CH == 16) {
          uint4 w;
          __builtin_memcpy(&w, reinterpret_cast<const char*>(vals) + 16 * k, 16);
          reinterpret_cast<uint4*>(dst)[k] = w;
        } else {
          uint2 w;
          __builtin_memcpy(&w, reinterpret_cast<const char*>(vals) + 8 * k, 8);
          reinterpret_cast<uint2*>(dst)[k] = w;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) dst[k] = vals[k];
    }
  }
}

template <class T>
hipError_t launch_pack_t(const float2* x, int64_t ps, int64_t n, int n_pol, const double* stats, float oscale,
                         void* out, hipStream_t s) {
  const int64_t blocks = (n / 4 + QT - 1) / QT;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  const dim3 g((unsigned)blocks);
  T* o = static_cast<T*>(out);
  if (n_pol == 1) {
    const int ch = 8 * (int)sizeof(T) >= 16 ? 16 : 8;
    const int vec = reinterpret_cast<uintptr_t>(out) % (size_t)ch == 0;
    hipLaunchKernelGGL((quantise_pack_kernel<T, 1>), g, dim3(QT), 0, s, x, ps, n, n_pol, stats, oscale, o, vec);
  } else if (n_pol == 2) {
    const int vec = reinterpret_cast<uintptr_t>(out) % 16 == 0;
    hipLaunchKernelGGL((quantise_pack_kernel<T, 2>), g, dim3(QT), 0, s, x, ps, n, n_pol, stats, oscale, o, vec);
  } else {
    hipLaunchKernelGGL((quantise_pack_kernel<T, 0>), g, dim3(QT), 0, s, x, ps, n, n_pol, stats, oscale, o, 0);
  }
  return hipGetLastError();
}

// 16-byte loads of every polarisation's row
bool rows_vec_ok(const float2* x, int64_t ps, int64_t n, int mult) {
  return x && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (ps & 1) == 0 && n % mult == 0 && ps >= n;
}

}  // namespace

int64_t stream_moments_slots(const AnalysisArgs& a, bool lcbf) {
  if (a.K <= a.row0) return 0;
  int64_t slots = -1;
  return moments_any(a, lcbf, nullptr, &slots) == hipSuccess ? slots : -1;
}

hipError_t launch_stream_moments(const AnalysisArgs& a, bool lcbf, hipStream_t s) {
  if (a.K <= a.row0) return hipSuccess;
  return moments_any(a, lcbf, s, nullptr);
}

int64_t moments_partials_slots(int64_t n, int n_pol) {
  return ((n / 2 + kMomV * QT - 1) / (kMomV * QT)) * n_pol;
}

hipError_t launch_moments_partials(const float2* x, int64_t ps, int64_t n, int n_pol, double* mom, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!mom || n_pol <= 0 || n_pol > 65535 || !rows_vec_ok(x, ps, n, 2)) return hipErrorInvalidValue;
  const int64_t nw = moments_partials_slots(n, 1);
  if (nw > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moments_partials_kernel, dim3((unsigned)nw, (unsigned)n_pol), dim3(QT), 0, s, x, ps, n, mom);
  return hipGetLastError();
}

hipError_t launch_moments_finish(const double* mom, int64_t slots, double cnt, double rms, double* stats,
                                 hipStream_t s) {
  if (!mom || !stats || slots <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(QT), 0, s, mom, slots, cnt, rms, stats);
  return hipGetLastError();
}

hipError_t launch_quantise_pack(const float2* x, int64_t ps, int64_t n, int n_pol, const double* stats,
                                float out_scale, void* out, int nbit, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!out || n_pol <= 0 || !rows_vec_ok(x, ps, n, 4)) return hipErrorInvalidValue;
  switch (nbit) {
    case 8: return launch_pack_t<int8_t>(x, ps, n, n_pol, stats, out_scale, out, s);
    case 16: return launch_pack_t<int16_t>(x, ps, n, n_pol, stats, out_scale, out, s);
    case 32: return launch_pack_t<float>(x, ps, n, n_pol, stats, out_scale, out, s);
    case 64: return launch_pack_t<double>(x, ps, n, n_pol, stats, out_scale, out, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pfb
