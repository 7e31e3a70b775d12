// pfb_ana_stream_qin.hip — the quantised FilterBank input (FilterBank.m:75-83,
// pfb_analysis_set_input_quantiser): the moments of a call's new samples read where they lie
// (input_moments_kernel: cf32 rows or a DADA section, one slot per workgroup, finished by
// moments_finish_kernel of pfb_ana_stream_quant.hip), the streaming analysis kernel rounding at
// the load (analysis_stream_qin_kernel and analysis_stream_qin_moments_kernel,
// pfb_ana_stream.hpp; the five streaming shapes x {cf32, DADA 8 / 16 / 32 input}: 40 kernels)
// and the quantising copy of the STAGED side and of the carry tail (quantise_copy_kernel).  No
// floating-point atomics: every partial sum has a slot of its own and every sum a fixed order.
#include "pfb_ana_stream.hpp"

namespace pfb {

namespace {

template <int N, int P, int NU, int DE, bool LCBF, class IN>
void (*qin_kernel_in(bool mom))(AnalysisArgs) {
  return mom ? analysis_stream_qin_moments_kernel<N, P, NU, DE, LCBF, IN> : analysis_stream_qin_kernel<N, P, NU, DE, LCBF, IN>;
}

template <int N, int P, int NU, int DE, bool LCBF>
void (*qin_kernel_of(const AnalysisArgs& a))(AnalysisArgs) {
  const bool mom = a.mom != nullptr;
  if (!a.din) return qin_kernel_in<N, P, NU, DE, LCBF, InCf32>(mom);
  return a.din_nbit == 8    ? qin_kernel_in<N, P, NU, DE, LCBF, InDada8>(mom)
         : a.din_nbit == 16 ? qin_kernel_in<N, P, NU, DE, LCBF, InDada16>(mom)
                            : qin_kernel_in<N, P, NU, DE, LCBF, InDada32>(mom);
}

// (launch_stream_moments' checks and grid: a.mom, when set, has stream_moments_slots(a) slots)
template <int N, int P, int NU, int DE, bool LCBF>
hipError_t launch_qin(const AnalysisArgs& a, hipStream_t s) {
  using SH = StreamShape<N, P, NU, DE>;
  // the plain cf32 product only
  if (a.dout || a.z || a.out_rs != 0 || !a.out) return hipErrorInvalidValue;
  if (a.din && a.din_nbit != 8 && a.din_nbit != 16 && a.din_nbit != 32) return hipErrorInvalidValue;
  StreamGrid sg;
  hipError_t e = stream_grid<SH, NU>(a, &sg);
  if (e != hipSuccess) return e;
  if (sg.wgs > INT32_MAX) return hipErrorInvalidValue;
  // (the carry: launch_stream's bound)
  if (a.pre && (a.pad < 0 || a.pad > (int64_t)SH::WIN * N)) return hipErrorInvalidValue;
  auto kern = qin_kernel_of<N, P, NU, DE, LCBF>(a);
  e = set_lds(kern, SH::lds_bytes);
  if (e != hipSuccess) return e;
  dim3 grid((unsigned)sg.wgs, (unsigned)a.n_pol);
  return launch_kernel(kern, grid, dim3(NT), SH::lds_bytes, s, a);
}

// the samples of one 16-byte load, each added to the thread's sums in the order they lie
template <class IN>
__device__ __forceinline__ void add_sample(double (&m)[3], typename IN::raw_t raw) {
  const v2f v = IN::cvt(raw);
  const double re = v.x, im = v.y;
  m[0] += re;
  m[1] += im;
  m[2] = fma(re, re, fma(im, im, m[2]));
}
template <class IN>
__device__ __forceinline__ void add_vec(double (&m)[3], uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (IN::kBytes == 8) {
    add_sample<IN>(m, __builtin_bit_cast(v2f, v2u{w[0], w[1]}));
    add_sample<IN>(m, __builtin_bit_cast(v2f, v2u{w[2], w[3]}));
  } else if constexpr (IN::kBytes == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) add_sample<IN>(m, w[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      add_sample<IN>(m, (uint16_t)(w[j] & 0xffffu));
      add_sample<IN>(m, (uint16_t)(w[j] >> 16));
    }
  }
}

// The moments of rows of IN samples (cf32: one row per polarisation, row_stride bytes apart; a
// section: its n n_pol samples as one row): row blockIdx.y is the `bytes` bytes from
// base + blockIdx.y row_stride, aligned to one sample.  Workgroup w sums the kMomV x QT 16-byte
// vectors from vector w kMomV QT of the row's 16-byte aligned middle; workgroup 0 also takes the
// samples in front of and behind the middle (fewer than 8 each), one per thread.  Every workgroup
// stores its three doubles at mom[(blockIdx.y nw + w) 3 ...] — zeros when it has no vector.
template <class IN>
__global__ void __launch_bounds__(kOneShotThreads) input_moments_kernel(const char* __restrict__ base, int64_t row_stride,
                                                                        int64_t bytes, double* __restrict__ mom) {
  constexpr int QT = kOneShotThreads;
  __shared__ double red[12];
  const char* row = base + (int64_t)blockIdx.y * row_stride;
  const int64_t head = min(bytes, (int64_t)((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15));
  const int64_t nvec = (bytes - head) / 16;
  const int64_t tail0 = head + nvec * 16;
  const uint4* mid = reinterpret_cast<const uint4*>(row + head);
  const int64_t i0 = (int64_t)blockIdx.x * (kMomLoads * QT) + threadIdx.x;
  uint4 v[kMomLoads];
#pragma unroll
  for (int u = 0; u < kMomLoads; ++u)  // the thread's loads in flight together
    v[u] = i0 + u * QT < nvec ? mid[i0 + u * QT] : make_uint4(0u, 0u, 0u, 0u);
  double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < kMomLoads; ++u) add_vec<IN>(m, v[u]);
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    const int nh = (int)(head / IN::kBytes), nt = (int)((bytes - tail0) / IN::kBytes);
    if (t < nh) add_sample<IN>(m, IN::gload(row + (int64_t)t * IN::kBytes));
    if (t >= 8 && t - 8 < nt) add_sample<IN>(m, IN::gload(row + tail0 + (int64_t)(t - 8) * IN::kBytes));
  }
  wg_sum3(m, red);
  if (threadIdx.x == 0) {
    double* slot = mom + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    slot[0] = m[0];
    slot[1] = m[1];
    slot[2] = m[2];
  }
}

// Samples t = 2 i, 2 i + 1 of polarisation blockIdx.y: sample t at src + pol pol_bytes + t step
// (cf32 rows: step 8; a section: step n_pol kBytes, pol_bytes kBytes), rounded to
// dst[pol dps + t].  vec bit 0: the cf32 pair is one 16-byte load, bit 1: one 16-byte store
// (the launcher checks the alignment of every row).  dst may be the cf32 source (no restrict).
template <class IN>
__global__ void __launch_bounds__(kOneShotThreads) quantise_copy_kernel(const char* src, int64_t step, int64_t pol_bytes,
                                                                        int64_t n, const double* stats, float2* dst,
                                                                        int64_t dps, int vec) {
  const int64_t t = ((int64_t)blockIdx.x * kOneShotThreads + threadIdx.x) * 2;
  if (t >= n) return;
  const float sf = stats ? (float)stats[3] : 1.0f;  // (uniform: one scalar load per wave)
  const char* s0 = src + (int64_t)blockIdx.y * pol_bytes + t * step;
  float2* d = dst + (int64_t)blockIdx.y * dps + t;
  auto q = [&](v2f v) { return make_float2(roundf(sf * v.x), roundf(sf * v.y)); };
  if (t + 1 < n) {
    v2f a, b;
    if constexpr (IN::kBytes == 8) {
      if (vec & 1) {
        const float4 w = *reinterpret_cast<const float4*>(s0);
        a = v2f{w.x, w.y};
        b = v2f{w.z, w.w};
      } else {
        a = IN::cvt(IN::gload(s0));
        b = IN::cvt(IN::gload(s0 + step));
      }
    } else {
      a = IN::cvt(IN::gload(s0));
      b = IN::cvt(IN::gload(s0 + step));
    }
    const float2 qa = q(a), qb = q(b);
    if (vec & 2) {
      *reinterpret_cast<float4*>(d) = make_float4(qa.x, qa.y, qb.x, qb.y);
    } else {
      d[0] = qa;
      d[1] = qb;
    }
  } else {
    d[0] = q(IN::cvt(IN::gload(s0)));
  }
}

bool qin_src_ok(const QinSrc& q) {
  if (!q.base || q.n_pol <= 0 || q.n_pol > 65535) return false;
  if (q.nbit == 0) return q.ps >= q.n && reinterpret_cast<uintptr_t>(q.base) % 8 == 0;
  if (q.nbit != 8 && q.nbit != 16 && q.nbit != 32) return false;
  return reinterpret_cast<uintptr_t>(q.base) % (size_t)(q.nbit / 4) == 0;
}

// the rows input_moments_kernel sees: (rows, bytes per row, bytes from a row to the next)
struct MomRows {
  int64_t rows, bytes, stride;
};
MomRows mom_rows(const QinSrc& q) {
  if (q.nbit == 0) return MomRows{q.n_pol, q.n * 8, q.ps * 8};
  return MomRows{1, q.n * q.n_pol * (q.nbit / 4), 0};
}
// workgroups per row: enough for the aligned middle whatever the row's alignment
int64_t mom_wgs(const MomRows& r) {
  const int64_t per = (int64_t)kMomLoads * kOneShotThreads;
  return std::max<int64_t>(1, (r.bytes / 16 + per - 1) / per);
}

}  // namespace

int64_t input_moments_slots(const QinSrc& q) {
  if (q.n <= 0) return 0;
  const MomRows r = mom_rows(q);
  return mom_wgs(r) * r.rows;
}

hipError_t launch_input_moments(const QinSrc& q, double* mom, hipStream_t s) {
  if (q.n <= 0) return hipSuccess;
  if (!mom || !qin_src_ok(q)) return hipErrorInvalidValue;
  const MomRows r = mom_rows(q);
  const int64_t nw = mom_wgs(r);
  if (nw > INT32_MAX) return hipErrorInvalidValue;
  const dim3 g((unsigned)nw, (unsigned)r.rows), b(kOneShotThreads);
  const char* base = static_cast<const char*>(q.base);
  switch (q.nbit) {
    case 0: hipLaunchKernelGGL(input_moments_kernel<InCf32>, g, b, 0, s, base, r.stride, r.bytes, mom); break;
    case 8: hipLaunchKernelGGL(input_moments_kernel<InDada8>, g, b, 0, s, base, r.stride, r.bytes, mom); break;
    case 16: hipLaunchKernelGGL(input_moments_kernel<InDada16>, g, b, 0, s, base, r.stride, r.bytes, mom); break;
    default: hipLaunchKernelGGL(input_moments_kernel<InDada32>, g, b, 0, s, base, r.stride, r.bytes, mom); break;
  }
  return hipGetLastError();
}

hipError_t launch_quantise_copy(const QinSrc& q, const double* stats, float2* dst, int64_t dps, hipStream_t s) {
  if (q.n <= 0) return hipSuccess;
  if (!dst || dps < q.n || !qin_src_ok(q)) return hipErrorInvalidValue;
  const int64_t blocks = ((q.n + 1) / 2 + kOneShotThreads - 1) / kOneShotThreads;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  const dim3 g((unsigned)blocks, (unsigned)q.n_pol), b(kOneShotThreads);
  const char* base = static_cast<const char*>(q.base);
  int vec = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && dps % 2 == 0) ? 2 : 0;
  const int64_t step = q.nbit == 0 ? 8 : (int64_t)q.n_pol * (q.nbit / 4);
  const int64_t pol_bytes = q.nbit == 0 ? q.ps * 8 : q.nbit / 4;
  switch (q.nbit) {
    case 0:
      if (reinterpret_cast<uintptr_t>(base) % 16 == 0 && q.ps % 2 == 0) vec |= 1;
      hipLaunchKernelGGL(quantise_copy_kernel<InCf32>, g, b, 0, s, base, step, pol_bytes, q.n, stats, dst, dps, vec);
      break;
    case 8:
      hipLaunchKernelGGL(quantise_copy_kernel<InDada8>, g, b, 0, s, base, step, pol_bytes, q.n, stats, dst, dps, vec);
      break;
    case 16:
      hipLaunchKernelGGL(quantise_copy_kernel<InDada16>, g, b, 0, s, base, step, pol_bytes, q.n, stats, dst, dps, vec);
      break;
    default:
      hipLaunchKernelGGL(quantise_copy_kernel<InDada32>, g, b, 0, s, base, step, pol_bytes, q.n, stats, dst, dps, vec);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_stream_qin(const AnalysisArgs& a, bool lcbf, hipStream_t s) {
  if (a.K <= a.row0) return hipSuccess;
  if (a.variant != kBunton || a.N != 256) return hipErrorInvalidValue;
  if (lcbf) {
    if (a.M != 192 || a.P != 12 || a.nu != 4) return hipErrorInvalidValue;
    return launch_qin<256, 12, 4, 3, true>(a, s);
  }
  if (a.nu == 8 && a.M == 224) {
    if (a.P == 13) return launch_qin<256, 13, 8, 7, false>(a, s);
    if (a.P == 12) return launch_qin<256, 12, 8, 7, false>(a, s);
  }
  if (a.nu == 4 && a.M == 192) {
    if (a.P == 13) return launch_qin<256, 13, 4, 3, false>(a, s);
    if (a.P == 12) return launch_qin<256, 12, 4, 3, false>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace pfb
