// pfb_verify.hip — the verification loop of the reference (current_performance.m) on the
// device, and its C ABI (include/pfb_api.h, "verification" section):
//
//   * the two scored test-vector generators, time_domain_impulse.m:13-24 and
//     complex_sinusoid.m:16-31 (double phase, single result), written straight into the
//     rows of a round trip's input batch;
//   * the spurious-power scores of ErrorAnalysis.m:5-52 / DomainPerformance.m:67-100 and the
//     TestImpulse.m:46-73 criterion: first argmax, then max and sum with a window round it
//     zeroed;
//   * the difference score of DomainPerformance.m:7-64.
//
// All of them stream a row once (the spurious score twice: its mask depends on the argmax)
// and do a handful of double operations per sample, so they are HBM-bound one-shot grids:
// 16-byte accesses behind an optional 8-byte head element, four in flight per thread.  Every
// reduction is deterministic: each workgroup writes its partial, a second small kernel
// combines the partials of a vector in a fixed order.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

#include "pfb_api.h"
#include "pfb_host.hpp"

namespace {

pfb_status bad(const char* msg) { return pfb_set_error(PFB_ERR_INVALID_ARG, msg); }

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int U = 4;                    // 16-byte loads in flight per thread (score kernels)
constexpr int64_t TILE = (int64_t)TPB * U;  // slots per workgroup
constexpr int64_t kNoIndex = INT64_MAX;

// ---------------------------------------------------------------- generators
// The parameters of up to GEN_MAX vectors travel as kernel arguments, so the call needs no
// device copy of the host arrays and stays asynchronous.
constexpr int GEN_MAX = 64;
struct GenBatch {
  double w[GEN_MAX];    // sinusoid: (2 pi (frequency + bin_offset)) / n
  double ph[GEN_MAX];   // sinusoid: phase
  int64_t lo[GEN_MAX];  // impulse: ones at [lo, hi), already clipped to [0, n]
  int64_t hi[GEN_MAX];
  int32_t kind[GEN_MAX];
};

__device__ inline float2 testvec_sample(int kind, double w, double ph, int64_t lo, int64_t hi, int64_t t) {
  if (kind == PFB_TESTVEC_IMPULSE) return make_float2(t >= lo && t < hi ? 1.f : 0.f, 0.f);
  // complex_sinusoid.m:24-27: the product and the sum each rounded once (no fused multiply-add)
  const double a = __dadd_rn(__dmul_rn(w, (double)t), ph);
  double s, c;
  sincos(a, &s, &c);
  return make_float2((float)c, (float)s);
}

// grid (slots of the row, vector).  A slot is two samples behind the row's 16-byte boundary;
// the sample in front of it, if any, is stored by slot 0's thread.
__global__ void __launch_bounds__(TPB) testvec_kernel(GenBatch g, int64_t n, float2* __restrict__ out,
                                                      int64_t stride) {
  const int v = blockIdx.y;
  float2* row = out + (int64_t)v * stride;
  const int kind = g.kind[v];
  const double w = g.w[v], ph = g.ph[v];
  const int64_t lo = g.lo[v], hi = g.hi[v];
  const int head = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1);
  const int64_t s = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (s == 0 && head) row[0] = testvec_sample(kind, w, ph, lo, hi, 0);
  const int64_t t = head + 2 * s;
  if (t + 1 < n) {
    const float2 a = testvec_sample(kind, w, ph, lo, hi, t);
    const float2 b = testvec_sample(kind, w, ph, lo, hi, t + 1);
    *reinterpret_cast<float4*>(row + t) = make_float4(a.x, a.y, b.x, b.y);
  } else if (t < n) {
    row[t] = testvec_sample(kind, w, ph, lo, hi, t);
  }
}

// ---------------------------------------------------------------- rows of the scores
// A row of complex float32 (R = float) or complex float64 (R = double), read in slots of 16
// bytes: two cf32 samples behind the row's 16-byte boundary (`head` = 1: sample 0 lies in
// front of it and is read on its own), or one cf64 sample (two 8-byte loads when the row is
// not 16-byte aligned).
template <class R>
struct RowView {
  const R* r;  // re, im interleaved
  int64_t n;
  int head;
  bool vec;
};

template <class R>
__device__ inline RowView<R> row_view(const void* base, int64_t stride, int64_t v, int64_t n) {
  const R* r = static_cast<const R*>(base) + 2 * v * stride;
  const bool mis = (reinterpret_cast<uintptr_t>(r) & 15) != 0;
  if constexpr (sizeof(R) == 4) return RowView<R>{r, n, mis ? 1 : 0, true};
  else return RowView<R>{r, n, 0, !mis};
}

__device__ inline double power_of(double re, double im, double scale) { return scale * (re * re + im * im); }

// the samples of slot s as scale |x|^2: p[0 .. count), the first one sample t
template <class R>
__device__ inline int slot_power(const RowView<R>& w, int64_t s, double scale, double (&p)[2], int64_t& t) {
  if constexpr (sizeof(R) == 4) {
    t = w.head + 2 * s;
    if (t + 1 < w.n) {
      const float4 x = *reinterpret_cast<const float4*>(w.r + 2 * t);
      p[0] = power_of(x.x, x.y, scale);
      p[1] = power_of(x.z, x.w, scale);
      return 2;
    }
    if (t < w.n) {
      const float2 x = *reinterpret_cast<const float2*>(w.r + 2 * t);
      p[0] = power_of(x.x, x.y, scale);
      return 1;
    }
    return 0;
  } else {
    t = s;
    if (t >= w.n) return 0;
    if (w.vec) {
      const double2 x = *reinterpret_cast<const double2*>(w.r + 2 * t);
      p[0] = power_of(x.x, x.y, scale);
    } else {
      p[0] = power_of(w.r[2 * t], w.r[2 * t + 1], scale);
    }
    return 1;
  }
}

// calls f(t, p) for every sample of the workgroup's tile, a thread's loads issued together
template <class R, class F>
__device__ inline void for_tile(const RowView<R>& w, double scale, F&& f) {
  const int64_t s0 = (int64_t)blockIdx.x * TILE + threadIdx.x;
  double p[U][2];
  int64_t t[U];
  int cnt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cnt[u] = slot_power(w, s0 + (int64_t)u * TPB, scale, p[u], t[u]);
  if (w.head && s0 == 0) f((int64_t)0, power_of(w.r[0], w.r[1], scale));
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (cnt[u] > 0) f(t[u], p[u][0]);
    if (cnt[u] > 1) f(t[u] + 1, p[u][1]);
  }
}

// ---------------------------------------------------------------- workgroup reductions
// np.argmax: the larger value, and of equal values the smaller index
__device__ inline void take_first_max(double& bp, int64_t& bt, double p, int64_t t) {
  if (p > bp || (p == bp && t < bt)) {
    bp = p;
    bt = t;
  }
}

__device__ inline int64_t shfl_down_i64(int64_t x, int off) { return (int64_t)__shfl_down((long long)x, off, 64); }

// every thread's (value, index) -> the workgroup's first maximum, in thread 0
__device__ inline void block_first_max(double& bp, int64_t& bt) {
  __shared__ double sp[WAVES];
  __shared__ int64_t st[WAVES];
  for (int off = 32; off > 0; off >>= 1) take_first_max(bp, bt, __shfl_down(bp, off, 64), shfl_down_i64(bt, off));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sp[wv] = bp;
    st[wv] = bt;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < WAVES; ++k) take_first_max(bp, bt, sp[k], st[k]);
  __syncthreads();
}

// every thread's maximum and sum -> the workgroup's, in thread 0 (a fixed tree: the same
// data give the same bits)
__device__ inline void block_max_sum(double& mx, double& sm) {
  __shared__ double smx[WAVES], ssm[WAVES];
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmax(mx, __shfl_down(mx, off, 64));
    sm += __shfl_down(sm, off, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    smx[wv] = mx;
    ssm[wv] = sm;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < WAVES; ++k) {
      mx = fmax(mx, smx[k]);
      sm += ssm[k];
    }
  __syncthreads();
}

// ---------------------------------------------------------------- spurious score
// Per vector v the device keeps fin[6 v ..] (the result row) and nb partials of three words,
// part[3 (v nb + b) ..], reused by the two passes.

// pass 1: the first maximum of p, and p[e] / the maximum outside e +- 1
template <class R>
__global__ void __launch_bounds__(TPB) spur_peak_kernel(const void* a, int64_t stride, int64_t n, double scale,
                                                        const int64_t* __restrict__ expected, int nb,
                                                        double* __restrict__ part, double* __restrict__ fin) {
  const int64_t v = blockIdx.y;
  const RowView<R> w = row_view<R>(a, stride, v, n);
  int64_t e = expected ? expected[v] : -1;
  if (e < 0 || e >= n) e = -1;
  double bp = -1.0, om = 0.0;
  int64_t bt = kNoIndex;
  double* pe = fin + 6 * v + 4;
  for_tile(w, scale, [&](int64_t t, double p) {
    take_first_max(bp, bt, p, t);
    if (e >= 0) {
      if (t == e) *pe = p;
      else if (t < e - 1 || t > e + 1) om = fmax(om, p);
    }
  });
  block_first_max(bp, bt);
  double unused = 0.0;
  block_max_sum(om, unused);
  if (threadIdx.x == 0) {
    double* q = part + 3 * (v * nb + blockIdx.x);
    q[0] = bp;
    q[1] = __longlong_as_double((long long)bt);
    q[2] = om;
  }
}

// one workgroup per vector: partials -> fin[0] = k, [1] = p[k], [5] (and [4], [5] = -1
// without an expected index)
__global__ void __launch_bounds__(TPB) spur_peak_reduce_kernel(const double* __restrict__ part, int nb, int64_t n,
                                                               const int64_t* __restrict__ expected,
                                                               double* __restrict__ fin) {
  const int64_t v = blockIdx.x;
  const double* q = part + 3 * v * nb;
  double bp = -1.0, om = 0.0;
  int64_t bt = kNoIndex;
  for (int b = threadIdx.x; b < nb; b += TPB) {
    take_first_max(bp, bt, q[3 * b], (int64_t)__double_as_longlong(q[3 * b + 1]));
    om = fmax(om, q[3 * b + 2]);
  }
  block_first_max(bp, bt);
  double unused = 0.0;
  block_max_sum(om, unused);
  if (threadIdx.x == 0) {
    const int64_t e = expected ? expected[v] : -1;
    double* f = fin + 6 * v;
    f[0] = bt == kNoIndex ? 0.0 : (double)bt;
    f[1] = bp;
    if (e < 0 || e >= n) {
      f[4] = -1.0;
      f[5] = -1.0;
    } else {
      f[5] = om;
    }
  }
}

// pass 2: maximum and sum of p outside k +- domain, the unmasked terms summed directly
template <class R>
__global__ void __launch_bounds__(TPB) spur_mask_kernel(const void* a, int64_t stride, int64_t n, double scale,
                                                        int64_t domain, int nb, const double* __restrict__ fin,
                                                        double* __restrict__ part) {
  const int64_t v = blockIdx.y;
  const RowView<R> w = row_view<R>(a, stride, v, n);
  const int64_t k = (int64_t)fin[6 * v];
  const int64_t lo = k - domain, hi = k + domain;  // (the clips to [0, n - 1] exclude nothing more)
  double mx = 0.0, sm = 0.0;
  for_tile(w, scale, [&](int64_t t, double p) {
    if (t < lo || t > hi) {
      mx = fmax(mx, p);
      sm += p;
    }
  });
  block_max_sum(mx, sm);
  if (threadIdx.x == 0) {
    double* q = part + 3 * (v * nb + blockIdx.x);
    q[0] = mx;
    q[1] = sm;
  }
}

// one workgroup per vector: (max, sum) partials -> dst[v dst_stride + 0, 1], the sum in a fixed
// order (thread j takes partials j, j + TPB, ..; then the tree of block_max_sum)
__global__ void __launch_bounds__(TPB) max_sum_reduce_kernel(const double* __restrict__ part, int nb,
                                                             double* __restrict__ dst, int dst_stride) {
  const int64_t v = blockIdx.x;
  const double* q = part + 3 * v * nb;
  double mx = 0.0, sm = 0.0;
  for (int b = threadIdx.x; b < nb; b += TPB) {
    mx = fmax(mx, q[3 * b]);
    sm += q[3 * b + 1];
  }
  block_max_sum(mx, sm);
  if (threadIdx.x == 0) {
    dst[v * dst_stride] = mx;
    dst[v * dst_stride + 1] = sm;
  }
}

// ---------------------------------------------------------------- difference score
// d = |a - b|^2 in double.  The slots follow a's 16-byte boundary; b is read with 16-byte
// loads when its row meets the same boundary, else sample by sample.
__global__ void __launch_bounds__(TPB) diff_kernel(const float2* __restrict__ a, int64_t a_stride,
                                                   const float2* __restrict__ b, int64_t b_stride, int64_t n,
                                                   int nb, double* __restrict__ part) {
  const int64_t v = blockIdx.y;
  const float2* ra = a + v * a_stride;
  const float2* rb = b + v * b_stride;
  const int head = (int)((reinterpret_cast<uintptr_t>(ra) >> 3) & 1);
  const bool vecb = (reinterpret_cast<uintptr_t>(rb + head) & 15) == 0;
  auto d2 = [](float ar, float ai, float br, float bi) {
    const double dr = (double)ar - (double)br, di = (double)ai - (double)bi;
    return dr * dr + di * di;
  };
  const int64_t s0 = (int64_t)blockIdx.x * TILE + threadIdx.x;
  double mx = 0.0, sm = 0.0;
  float4 xa[U], xb[U];
  int cnt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t t = head + 2 * (s0 + (int64_t)u * TPB);
    cnt[u] = t + 1 < n ? 2 : t < n ? 1 : 0;
    if (cnt[u] == 2) {
      xa[u] = *reinterpret_cast<const float4*>(ra + t);
      if (vecb) {
        xb[u] = *reinterpret_cast<const float4*>(rb + t);
      } else {
        const float2 b0 = rb[t], b1 = rb[t + 1];
        xb[u] = make_float4(b0.x, b0.y, b1.x, b1.y);
      }
    } else if (cnt[u] == 1) {
      const float2 a0 = ra[t], b0 = rb[t];
      xa[u] = make_float4(a0.x, a0.y, 0.f, 0.f);
      xb[u] = make_float4(b0.x, b0.y, 0.f, 0.f);
    }
  }
  if (head && s0 == 0) {
    const double d = d2(ra[0].x, ra[0].y, rb[0].x, rb[0].y);
    mx = fmax(mx, d);
    sm += d;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (cnt[u] > 0) {
      const double d = d2(xa[u].x, xa[u].y, xb[u].x, xb[u].y);
      mx = fmax(mx, d);
      sm += d;
    }
    if (cnt[u] > 1) {
      const double d = d2(xa[u].z, xa[u].w, xb[u].z, xb[u].w);
      mx = fmax(mx, d);
      sm += d;
    }
  }
  block_max_sum(mx, sm);
  if (threadIdx.x == 0) {
    double* q = part + 3 * (v * nb + blockIdx.x);
    q[0] = mx;
    q[1] = sm;
  }
}

// ---------------------------------------------------------------- host side
// Per-device scratch of the scores (expected indices, result rows, partials), allocated once
// per device and grown when a call needs more.  A score call holds the lock from its first
// launch to its synchronise, so concurrent callers do not share the partials.
struct Scratch {
  std::mutex mu;
  std::vector<pfb::host::DevBuf> per_dev;
};
Scratch g_scratch;

constexpr int64_t kMaxPartials = int64_t(1) << 20;  // partials per launch group (x 24 bytes)

struct Carve {
  int64_t* expected;
  double* fin;
  double* part;
};

hipError_t scratch_for(int64_t vecs, int64_t nb, Carve* c) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if ((int)g_scratch.per_dev.size() <= dev) g_scratch.per_dev.resize(dev + 1);
  pfb::host::DevBuf& b = g_scratch.per_dev[dev];
  const size_t words = (size_t)vecs * (1 + 6 + 3 * (size_t)nb);
  e = b.ensure(words * 8);  // (a regrow frees the old block: hipFree waits for the device)
  if (e != hipSuccess) return e;
  c->expected = b.as<int64_t>();
  c->fin = b.as<double>() + vecs;
  c->part = c->fin + 6 * vecs;
  return hipSuccess;
}

// workgroups per row of `slots` 16-byte slots; 0 when a grid cannot hold them
int64_t tiles_for(int64_t slots) {
  const int64_t nb = std::max<int64_t>((slots + TILE - 1) / TILE, 1);
  return nb > INT32_MAX ? 0 : nb;
}

int64_t vectors_per_group(int64_t n_vec, int64_t nb) {
  return std::min<int64_t>(n_vec, std::max<int64_t>(kMaxPartials / nb, 1));
}

template <class R>
pfb_status spurious_run(const void* a, int64_t stride, int64_t n, int32_t n_vec, double scale, int32_t domain,
                        const int64_t* expected, double* result, hipStream_t s) {
  // (cf32: one more slot than n / 2 covers a head sample and an odd tail)
  const int64_t nb = tiles_for(sizeof(R) == 4 ? n / 2 + 1 : n);
  if (!nb) return pfb_set_error(PFB_ERR_UNSUPPORTED, "pfb_purity_score_spurious: series too long for one grid");
  const int64_t group = vectors_per_group(n_vec, nb);
  std::lock_guard<std::mutex> lk(g_scratch.mu);
  Carve c{};
  HIPCHK(scratch_for(group, nb, &c));
  const int64_t* dexp = expected ? c.expected : nullptr;
  for (int64_t v0 = 0; v0 < n_vec; v0 += group) {
    const int64_t V = std::min<int64_t>(group, n_vec - v0);
    const void* rows = static_cast<const char*>(a) + (size_t)v0 * stride * 2 * sizeof(R);
    if (expected) HIPCHK(hipMemcpyAsync(c.expected, expected + v0, V * sizeof(int64_t), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)nb, (unsigned)V);
    hipLaunchKernelGGL(spur_peak_kernel<R>, grid, TPB, 0, s, rows, stride, n, scale, dexp, (int)nb, c.part, c.fin);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(spur_peak_reduce_kernel, dim3((unsigned)V), TPB, 0, s, c.part, (int)nb, n, dexp, c.fin);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(spur_mask_kernel<R>, grid, TPB, 0, s, rows, stride, n, scale, (int64_t)domain, (int)nb,
                       c.fin, c.part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(max_sum_reduce_kernel, dim3((unsigned)V), TPB, 0, s, c.part, (int)nb, c.fin + 2, 6);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(result + 6 * v0, c.fin, V * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

}  // namespace

extern "C" {

pfb_status pfb_testvec_generate(const int32_t* kind, const double* param, int32_t n_vec, int64_t n,
                                pfb_cf32* out, int64_t out_stride, void* stream) {
  if (n <= 0 || n_vec <= 0) return bad("pfb_testvec_generate: bad sizes");
  if (n_vec > 65535) return bad("pfb_testvec_generate: n_vec > 65535");
  if (out_stride < n) return bad("pfb_testvec_generate: row stride too small");
  if (!kind || !param || !out) return bad("pfb_testvec_generate: null buffer");
  if ((uintptr_t)out & 7) return bad("pfb_testvec_generate: out not aligned to a complex sample");
  for (int32_t v = 0; v < n_vec; ++v) {
    if (kind[v] != PFB_TESTVEC_IMPULSE && kind[v] != PFB_TESTVEC_SINUSOID)
      return bad("pfb_testvec_generate: unknown test-vector kind");
    const int used = kind[v] == PFB_TESTVEC_IMPULSE ? 2 : 3;
    for (int j = 0; j < used; ++j)
      if (!std::isfinite(param[4 * v + j])) return bad("pfb_testvec_generate: non-finite parameter");
  }
  const int64_t gx = (n / 2 + 1 + TPB - 1) / TPB;
  if (gx > INT32_MAX) return pfb_set_error(PFB_ERR_UNSUPPORTED, "pfb_testvec_generate: series too long for one grid");
  hipStream_t s = (hipStream_t)stream;
  const double nd = (double)n;
  for (int32_t v0 = 0; v0 < n_vec; v0 += GEN_MAX) {
    const int V = std::min<int32_t>(GEN_MAX, n_vec - v0);
    GenBatch g{};
    for (int j = 0; j < V; ++j) {
      const double* p = param + 4 * (int64_t)(v0 + j);
      g.kind[j] = kind[v0 + j];
      if (g.kind[j] == PFB_TESTVEC_IMPULSE) {
        const double first = std::floor(p[0]) - 1.0, end = first + std::floor(p[1]);
        g.lo[j] = (int64_t)std::min(std::max(first, 0.0), nd);
        g.hi[j] = (int64_t)std::min(std::max(end, 0.0), nd);
      } else {
        g.w[j] = ((2.0 * M_PI) * (p[0] + p[2])) / nd;
        g.ph[j] = p[1];
      }
    }
    hipLaunchKernelGGL(testvec_kernel, dim3((unsigned)gx, (unsigned)V), TPB, 0, s, g, n,
                       reinterpret_cast<float2*>(out) + (int64_t)v0 * out_stride, out_stride);
    HIPCHK(hipGetLastError());
  }
  return PFB_OK;
}

pfb_status pfb_purity_score_spurious(const void* a, int32_t dtype, int64_t stride, int64_t n, int32_t n_vec,
                                     double scale, int32_t domain, const int64_t* expected, double* result,
                                     void* stream) {
  if (n <= 0 || n_vec <= 0) return bad("pfb_purity_score_spurious: bad sizes");
  if (n_vec > 65535) return bad("pfb_purity_score_spurious: n_vec > 65535");
  if (stride < n) return bad("pfb_purity_score_spurious: row stride too small");
  if (!a || !result) return bad("pfb_purity_score_spurious: null buffer");
  if ((uintptr_t)a & 7) return bad("pfb_purity_score_spurious: series not 8-byte aligned");
  if (domain < 0) return bad("pfb_purity_score_spurious: negative domain");
  if (dtype != 0 && dtype != 1) return bad("pfb_purity_score_spurious: dtype must be 0 (cf32) or 1 (cf64)");
  if (!std::isfinite(scale)) return bad("pfb_purity_score_spurious: non-finite scale");
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? spurious_run<float>(a, stride, n, n_vec, scale, domain, expected, result, s)
                    : spurious_run<double>(a, stride, n, n_vec, scale, domain, expected, result, s);
}

pfb_status pfb_purity_score_difference(const pfb_cf32* a, int64_t a_stride, const pfb_cf32* b, int64_t b_stride,
                                       int64_t n, int32_t n_vec, double* result, void* stream) {
  if (n <= 0 || n_vec <= 0) return bad("pfb_purity_score_difference: bad sizes");
  if (n_vec > 65535) return bad("pfb_purity_score_difference: n_vec > 65535");
  if (a_stride < n || b_stride < n) return bad("pfb_purity_score_difference: row stride too small");
  if (!a || !b || !result) return bad("pfb_purity_score_difference: null buffer");
  if (((uintptr_t)a | (uintptr_t)b) & 7) return bad("pfb_purity_score_difference: series not aligned to a complex sample");
  const int64_t nb = tiles_for(n / 2 + 1);
  if (!nb) return pfb_set_error(PFB_ERR_UNSUPPORTED, "pfb_purity_score_difference: series too long for one grid");
  hipStream_t s = (hipStream_t)stream;
  const int64_t group = vectors_per_group(n_vec, nb);
  std::lock_guard<std::mutex> lk(g_scratch.mu);
  Carve c{};
  HIPCHK(scratch_for(group, nb, &c));
  for (int64_t v0 = 0; v0 < n_vec; v0 += group) {
    const int64_t V = std::min<int64_t>(group, n_vec - v0);
    hipLaunchKernelGGL(diff_kernel, dim3((unsigned)nb, (unsigned)V), TPB, 0, s,
                       reinterpret_cast<const float2*>(a) + v0 * a_stride, a_stride,
                       reinterpret_cast<const float2*>(b) + v0 * b_stride, b_stride, n, (int)nb, c.part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(max_sum_reduce_kernel, dim3((unsigned)V), TPB, 0, s, c.part, (int)nb, c.fin, 2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(result + 2 * v0, c.fin, V * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

}  // extern "C"
