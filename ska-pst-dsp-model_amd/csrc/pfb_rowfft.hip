// pfb_rowfft.hip — N-point row FFT launchers (row_fft_kernel, pfb_common.hpp): the
// analysis FFT for N > 256 and synthesis stage 1 (the N-point inverse DFT across channels
// of every channelised row, polyphase_synthesis.m:282-285 factored).
#include "pfb_common.hpp"
#include "pfb_rowfft4k.hpp"

#include <algorithm>
#include <cstdlib>

namespace pfb {

// Output row rw (row_base + rw, circularly shifted by -sds mod n_total when remap: the padded
// variant's time shift, RowStore's rule) of a [row][N] product -> HBM.
__device__ __forceinline__ void r4k_store_row(const float2 (&v)[16], int tid, const RowFftArgs& a, float2* out,
                                              int64_t rw) {
  int64_t t = a.row_base + rw;
  if (a.remap) {
    t -= a.sds;
    while (t < 0) t += a.n_total;
  }
  // (t is uniform, but the uniformity analysis loses it through the wrap loop: without the
  // read-first-lane every store became a one-trip waterfall loop over the descriptor)
  t = (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)t >> 32)) << 32) |
                __builtin_amdgcn_readfirstlane((uint32_t)t));
  const __amdgpu_buffer_rsrc_t os = make_rsrc(out + t * 4096, (uint32_t)(4096 * 8));
  const uint32_t lane_off = (uint32_t)tid * 8u;
  static_for<0, 16>([&](auto rv) {
    constexpr int r = decltype(rv)::value;
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, cscale(v[r], a.scale)), os, lane_off,
                                          r * 2048, kNtRow ? 2 : 0);
  });
}

template <int DIR>
__device__ __forceinline__ void r4k_row(float2 (&v)[16], float2* row, const float2* t2, const float2* t3,
                                        int tid, const RowFftArgs& a, float2* out, int64_t rw) {
  r4k_fft<DIR>(v, row, t2, t3, tid);
  r4k_store_row(v, tid, a, out, rw);
}

// (buffer loads / stores: one descriptor per row, the lane's byte offset tid * 8 and the
// register's r * 2048 as a scalar offset — no 64-bit address per register: <= 168 VGPRs,
// 3 workgroups per CU)
template <int DIR, bool PERM, bool GAIN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void row_fft4096_kernel(RowFftArgs a) {
  constexpr int N = 4096;
  extern __shared__ __attribute__((aligned(16))) float2 smem[];
  const int pol = blockIdx.y;
  const int wg = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t q0 = a.n_rows * wg / gridDim.x, q1 = a.n_rows * (wg + 1) / gridDim.x;
  if (q0 >= q1) return;  // uniform per workgroup
  const int tid = threadIdx.x;
  float2* row = smem;                        // layouts A / B, kR4kRow slots
  float2* t2 = smem + kR4kRow;               // [p][16]
  float2* t3 = t2 + kR4kTw2;                 // [p][256]
  for (int e = tid; e < kR4kTw3; e += NT) {
    const int pp = e >> 8, k = e & 255;
    t3[e] = a.tw[(k << pp) & (N - 1)];
    if (e < kR4kTw2) t2[e] = a.tw[((e & 15) << ((e >> 4) + 4)) & (N - 1)];
  }
  const float2* in = a.in + pol * a.in_pol_stride;
  float2* out = a.out + pol * a.out_pol_stride;
  [[maybe_unused]] uint32_t col[PERM ? 16 : 1];
  [[maybe_unused]] float g[GAIN ? 16 : 1];
  if constexpr (PERM || GAIN) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = tid + r * 256;
      const int c = PERM ? a.perm[i] : i;
      if constexpr (PERM) col[PERM ? r : 0] = (uint32_t)c * 8u;
      if constexpr (GAIN) g[GAIN ? r : 0] = a.cgain[c];
    }
  }
  const uint32_t lane_off = (uint32_t)tid * 8u;
  // input in 2-row runs (a.in_run, z_index): element e of row rr at ((rr / 2) N + e) 2 + rr % 2
  // — the lane and register strides double; the pair's other row is fetched with the same
  // 128-B lines one row later (L2 / Infinity-Cache hits)
  const int ish = __builtin_amdgcn_readfirstlane(a.in_run ? 1 : 0);  // (scalar: the soffsets use it)
  const uint32_t lane_in = lane_off << ish;
  [[maybe_unused]] uint32_t col_in[PERM ? 16 : 1];
  if constexpr (PERM) {
#pragma unroll
    for (int r = 0; r < 16; ++r) col_in[PERM ? r : 0] = col[PERM ? r : 0] << ish;
  }
  float2 pf[16];
  auto load_row = [&](int64_t rr) {
    const int64_t base = a.in_run ? (((rr >> 1) * N) << 1) + (rr & 1) : rr * N;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc_u(in + base, (uint32_t)((N * 8) << ish));
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      const v2u x = PERM ? __builtin_amdgcn_raw_buffer_load_b64(rs, col_in[PERM ? r : 0], 0, kNtlRow ? 2 : 0)
                         : __builtin_amdgcn_raw_buffer_load_b64(rs, lane_in, (r * 2048) << ish, kNtlRow ? 2 : 0);
      pf[r] = __builtin_bit_cast(float2, x);
    });
  };
  load_row(q0);
  vm_drain();
#pragma unroll 1
  for (int64_t rw = q0; rw < q1; ++rw) {
    float2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = GAIN ? cscale(pf[r], g[GAIN ? r : 0]) : pf[r];
    load_row(min(rw + 1, q1 - 1));  // unconditional: past the end re-reads the last row
    r4k_row<DIR>(v, row, t2, t3, tid, a, out, rw);
  }
}

// Round 6: rows in PAIRS, one pair per workgroup.  RUN (in_run: the SKA-Mid round trip's
// stage-1 rows as the FIR writes them, 2-row runs per column): each lane loads element i of
// both rows with one 16-B buffer load, so the run's 128-B lines cross the memory side once
// (the one-row kernel loaded 8 B of every 16 and re-fetched the partner's lines one row
// later: 913 MB read for 613 MB of rows; 625 MB now, r06 PMC).  !RUN: rows
// [row][N], two 8-B loads per element.  Row 2p is transformed from the first halves while
// row 2p + 1 waits in registers.  REV: the padded variant's index reversal (column (N - i)
// mod N for element i) computed from the lane (element i = tid + 256 r: r >= 1 reads column
// 4096 - 256 r - tid, one lane base (255 - tid) and a scalar offset; r = 0 its own lane
// offset) — 2 registers instead of the 16 column offsets of the generic permutation.  OZS:
// the output in 2-row runs (RowStore::zs = 1, the Nf 512 synthesis' stage-1 layout; row A's
// results held until row B's, one 16-B store per element).  Same passes and tables as the
// one-row kernel: bit-identical.
// SCHED (which pairs a workgroup takes): 0 a contiguous range (XCD-aware order), 1 grid-stride
// from blockIdx.x, 2 one pair per workgroup (grid = pairs) — the default: the dispatcher hands
// out pairs in row order, so the chip's loads in flight stay in one narrow window of the
// rows; 224 vs 262 us per C3 launch (persistent ranges), 243 grid-stride
// (profiles/r06_v3_rowfft_sched_ab.log).  The same holds for a plain float4 copy: one 16-B
// load + store per thread, one-shot grid, 6.6 TB/s; persistent grid-stride or range loops
// 4.7-5.5 TB/s (scripts/copy_probe.hip, profiles/r06_copy_probe.jsonl).
template <int DIR, bool REV, int SCHED, bool RUN = true, bool OZS = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void row_fft4096_pair_kernel(RowFftArgs a) {
  constexpr int N = 4096;
  constexpr uint32_t ES = RUN ? 16u : 8u;  // bytes between elements i and i + 1 of a row
  extern __shared__ __attribute__((aligned(16))) float2 smem[];
  const int pol = blockIdx.y;
  const int64_t np = (a.n_rows + 1) >> 1;
  int64_t p0, p1, pstep = 1;
  if constexpr (SCHED == 0) {
    const int wg = xcd_tile(blockIdx.x, gridDim.x);
    p0 = np * wg / gridDim.x;
    p1 = np * (wg + 1) / gridDim.x;
  } else if constexpr (SCHED == 1) {
    p0 = blockIdx.x;
    p1 = np;
    pstep = gridDim.x;
  } else {
    p0 = blockIdx.x;
    p1 = min(p0 + 1, np);
  }
  if (p0 >= p1) return;  // uniform per workgroup
  const int tid = threadIdx.x;
  float2* row = smem;
  float2* t2 = smem + kR4kRow;
  float2* t3 = t2 + kR4kTw2;
  for (int e = tid; e < kR4kTw3; e += NT) {
    const int pp = e >> 8, k = e & 255;
    t3[e] = a.tw[(k << pp) & (N - 1)];
    if (e < kR4kTw2) t2[e] = a.tw[((e & 15) << ((e >> 4) + 4)) & (N - 1)];
  }
  const float2* in = a.in + pol * a.in_pol_stride;
  float2* out = a.out + pol * a.out_pol_stride;
  const uint32_t lane_a = REV ? (uint32_t)(255 - tid) * ES : (uint32_t)tid * ES;
  const uint32_t lane_0 = REV ? (tid ? (uint32_t)(N - tid) * ES : 0u) : lane_a;
  v4u pf[16];
  auto load_pair = [&](int64_t pp) {
    // (!RUN: the last pair of an odd row count has no row B.  Row B's displacement rides in
    // the scalar offset, which the descriptor's range check does not cover — it compares the
    // lane offset alone, pfb_synth_wave.hpp — so a one-row descriptor would not drop those
    // loads: they would read the 32 KB after the last row.  They are pointed at row A
    // instead: row_b = 0, a uniform scalar; the values are never transformed.)
    const bool has_b = RUN || 2 * pp + 1 < a.n_rows;
    const uint32_t nrec = RUN ? (uint32_t)(N * 16) : (has_b ? 2u : 1u) * (uint32_t)(N * 8);
    [[maybe_unused]] const int row_b = has_b ? N * 8 : 0;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc_u(in + pp * 2 * N, nrec);
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      constexpr int soff = r == 0 ? 0 : REV ? (3841 - 256 * r) * (int)ES : r * 256 * (int)ES;
      const uint32_t lo = r == 0 ? lane_0 : lane_a;
      if constexpr (RUN) {
        pf[r] = __builtin_amdgcn_raw_buffer_load_b128(rs, lo, soff, kNtlRow ? 2 : 0);
      } else {
        const v2u x0 = __builtin_amdgcn_raw_buffer_load_b64(rs, lo, soff, kNtlRow ? 2 : 0);
        const v2u x1 = __builtin_amdgcn_raw_buffer_load_b64(rs, lo, soff + row_b, kNtlRow ? 2 : 0);
        pf[r] = v4u{x0.x, x0.y, x1.x, x1.y};
      }
    });
  };
  load_pair(p0);
  vm_drain();
#pragma unroll 1
  for (int64_t pp = p0; pp < p1; pp += pstep) {
    float2 v[16], h[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const v4f x = __builtin_bit_cast(v4f, pf[r]);
      v[r] = make_float2(x.x, x.y);
      h[r] = make_float2(x.z, x.w);
    }
    if constexpr (OZS) {
      // both rows transformed, then element i of rows (2p, 2p + 1) as one 16-B store into
      // run p (row_base even, no remap: launch_row_fft_t checks)
      r4k_fft<DIR>(v, row, t2, t3, tid);
      if constexpr (SCHED != 2) load_pair(pp + pstep < p1 ? pp + pstep : pp);
      r4k_fft<DIR>(h, row, t2, t3, tid);
      const int64_t run = (a.row_base >> 1) + pp;
      const __amdgpu_buffer_rsrc_t os = make_rsrc_u(out + run * 2 * N, (uint32_t)(N * 16));
      auto st = [&](auto aux) {
        static_for<0, 16>([&](auto rv) {
          constexpr int r = decltype(rv)::value;
          const float2 x0 = cscale(v[r], a.scale), x1 = cscale(h[r], a.scale);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v4f{x0.x, x0.y, x1.x, x1.y}), os,
                                                 (uint32_t)tid * 16u, r * 4096, decltype(aux)::value);
        });
      };
      // (RowStore::nt: the default policy for rows the synthesis reads right after from the
      // Infinity Cache; uniform)
      if (a.nt && kNtRow) st(std::integral_constant<int, 2>{});
      else st(std::integral_constant<int, 0>{});
    } else {
      r4k_row<DIR>(v, row, t2, t3, tid, a, out, 2 * pp);
      if constexpr (SCHED != 2)
        load_pair(pp + pstep < p1 ? pp + pstep : pp);  // unconditional: past the end re-reads this pair
      if (2 * pp + 1 < a.n_rows) r4k_row<DIR>(h, row, t2, t3, tid, a, out, 2 * pp + 1);  // (uniform)
    }
  }
}

// The pair kernel for a padded plan's strided product (RowFftArgs::out_rs > 0, StridedOut;
// pfb_filterbank_execute_strided): rows paired by OUTPUT row.  The workgroup of pair g
// (g = xcd_tile(blockIdx.x), see below) makes output rows
// t = 2g and 2g + 1 from the FIR rows (t + sds) mod K — consecutive except at the single
// wrap, and each read through its own one-row descriptor (lane offset tid * 8, the
// register's r * 2048 as the scalar offset: inside the row by construction) — so a pair
// never starts odd when sds is odd and never straddles the wrap.  Only t < out_keep is made
// (the nu-trim: rows [T_out, K) are neither transformed nor stored); the last pair of an odd
// out_keep has no row B: its loads re-read row A and are never transformed (the !RUN rule of
// row_fft4096_pair_kernel).  Channel-major output (out_rs = 1, a cascade's stage-1 product)
// holds both rows' results and stores bin c of the pair as one 16-B element at c * out_cs +
// 2g, as OZS does for its runs; that needs the base 16-B aligned and out_cs, out_pol_stride
// even (uniform test, else two 8-B stores).  Any other layout: two 8-B stores per bin,
// coalesced across lanes when out_cs = 1.  Guarded plain stores (StridedOut).  Same passes
// and tables as the other 4096-point kernels: bit-identical values.
template <int DIR>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void row_fft4096_pair_strided_kernel(
    RowFftArgs a) {
  constexpr int N = 4096;
  extern __shared__ __attribute__((aligned(16))) float2 smem[];
  const int pol = blockIdx.y;
  // XCD-aware pair order (xcd_tile): consecutive pairs are consecutive workgroups of ONE XCD,
  // so the eight 16-B pieces of a channel-major 128-B line (16 rows of one channel) meet in
  // that XCD's L2 and leave it as one line.  In blockIdx order they come from eight L2s as
  // partial lines: the SKA-Mid cascade 1.84-1.90 ms against 1.50-1.53 with this order, and
  // nontemporal pair stores 2.8-2.9 (profiles/twostage_strided_padded_ab.jsonl)
  const int64_t t0 = 2 * (int64_t)xcd_tile(blockIdx.x, gridDim.x);
  if (t0 >= a.out_keep) return;  // uniform per workgroup
  const bool has_b = t0 + 1 < a.out_keep;
  const int tid = threadIdx.x;
  float2* row = smem;
  float2* t2 = smem + kR4kRow;
  float2* t3 = t2 + kR4kTw2;
  for (int e = tid; e < kR4kTw3; e += NT) {
    const int pp = e >> 8, k = e & 255;
    t3[e] = a.tw[(k << pp) & (N - 1)];
    if (e < kR4kTw2) t2[e] = a.tw[((e & 15) << ((e >> 4) + 4)) & (N - 1)];
  }
  const float2* in = a.in + pol * a.in_pol_stride;
  float2* out = a.out + pol * a.out_pol_stride;
  // FIR row of output row t: (t + sds) mod K (polyphase_analysis_padded.m:156 read backwards);
  // t < out_keep <= K and sh < K: one wrap
  const int64_t sh = a.sds % a.n_total;
  int64_t ra = t0 + sh, rb = has_b ? t0 + 1 + sh : t0 + sh;
  if (ra >= a.n_total) ra -= a.n_total;
  if (rb >= a.n_total) rb -= a.n_total;
  const __amdgpu_buffer_rsrc_t rsa = make_rsrc_u(in + ra * N, (uint32_t)(N * 8));
  const __amdgpu_buffer_rsrc_t rsb = make_rsrc_u(in + rb * N, (uint32_t)(N * 8));
  const uint32_t lane_off = (uint32_t)tid * 8u;
  float2 v[16], h[16];
  static_for<0, 16>([&](auto rv) {
    constexpr int r = decltype(rv)::value;
    v[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsa, lane_off, r * 2048, kNtlRow ? 2 : 0));
    h[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsb, lane_off, r * 2048, kNtlRow ? 2 : 0));
  });
  r4k_fft<DIR>(v, row, t2, t3, tid);
  if (has_b) r4k_fft<DIR>(h, row, t2, t3, tid);  // (uniform)
  const StridedOut lay{a.out_keep, a.out_rs, a.out_cs, a.sel_split, a.sel_shift, a.sel_n};
  const bool wide = has_b && a.out_rs == 1 && ((a.out_cs | a.out_pol_stride) & 1) == 0 &&
                    (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
  if (wide) {
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      const int64_t i = lay.at(t0, tid + 256 * r);  // rows 2g and 2g + 1 < out_keep: same bins kept
      if (i >= 0) {
        const float2 x0 = cscale(v[r], a.scale), x1 = cscale(h[r], a.scale);
        *reinterpret_cast<v4f*>(out + i) = v4f{x0.x, x0.y, x1.x, x1.y};
      }
    });
  } else {
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      lay.put(out, lay.at(t0, tid + 256 * r), cscale(v[r], a.scale));
      if (has_b) lay.put(out, lay.at(t0 + 1, tid + 256 * r), cscale(h[r], a.scale));
    });
  }
}

template <int DIR, bool PERM, bool GAIN>
static hipError_t launch_row_fft4096(const RowFftArgs& r, int n_pol, hipStream_t s, int per_cu) {
  auto kern = row_fft4096_kernel<DIR, PERM, GAIN>;
  hipError_t e = set_lds(kern, kR4kLds);
  if (e != hipSuccess) return e;
  const int64_t wgs = (int64_t)cu_count() * per_cu;
  dim3 grid((unsigned)std::max<int64_t>(1, wgs / n_pol), (unsigned)n_pol);
  return launch_kernel(kern, grid, dim3(NT), kR4kLds, s, r);
}

template <int DIR, bool REV, int SCHED, bool RUN, bool OZS>
static hipError_t launch_r4k_pair(const RowFftArgs& r, int n_pol, hipStream_t s, int per_cu) {
  auto kern = row_fft4096_pair_kernel<DIR, REV, SCHED, RUN, OZS>;
  hipError_t e = set_lds(kern, kR4kLds);
  if (e != hipSuccess) return e;
  const int64_t wgs = SCHED == 2 ? (r.n_rows + 1) / 2 : (int64_t)cu_count() * per_cu / n_pol;
  if (wgs > INT32_MAX) return hipErrorInvalidValue;
  dim3 grid((unsigned)std::max<int64_t>(1, wgs), (unsigned)n_pol);
  return launch_kernel(kern, grid, dim3(NT), kR4kLds, s, r);
}
template <int DIR, bool REV, bool RUN, bool OZS>
static hipError_t launch_row_fft4096_pair(const RowFftArgs& r, int n_pol, hipStream_t s, int per_cu) {
  // (PFB_ROWFFT_SCHED: 0 ranges, 1 grid-stride, 2 one pair per workgroup — experiments A/B)
  static const int sched = knob("PFB_ROWFFT_SCHED") ? std::atoi(knob("PFB_ROWFFT_SCHED")) : 2;
  if constexpr (kExperiments) {
    if (sched == 0) return launch_r4k_pair<DIR, REV, 0, RUN, OZS>(r, n_pol, s, per_cu);
    if (sched == 1) return launch_r4k_pair<DIR, REV, 1, RUN, OZS>(r, n_pol, s, per_cu);
  }
  return launch_r4k_pair<DIR, REV, 2, RUN, OZS>(r, n_pol, s, per_cu);
}

template <int N, int DIR, bool PERM, bool GAIN>
static hipError_t launch_row_fft_t(const RowFftArgs& r, int n_pol, hipStream_t s) {
  constexpr int ROWS = RowShape<N>::ROWS;
  if (r.dout) {
    // the product as a DADA section (launch_analysis' generic path, analysis_writes_dada): the
    // whole call's rows in one launch, plain [row][N] input and the plain section
    if constexpr (N == 4096 && !PERM && !GAIN) {
      if (r.perm || r.cgain || r.out_rs != 0 || r.row_base != 0 || r.n_rows != r.n_total || r.zs != 0 || r.in_run ||
          r.out_keep <= 0 || r.out_keep > r.n_total || r.n_pol != n_pol || n_pol > 65535)
        return hipErrorInvalidValue;
      return launch_row_fft4096_dadaout<DIR>(r, n_pol, s);
    } else {
      return hipErrorInvalidValue;
    }
  }
  if (r.out_rs > 0) {
    // strided product of a padded plan (launch_analysis' generic path): the whole call's
    // rows in one launch, plain [row][N] input, inverse-direction FFT, no perm / gain
    if constexpr (DIR > 0 && !PERM && !GAIN && (N & (N - 1)) == 0) {
      if (!r.remap || r.row_base != 0 || r.n_rows != r.n_total || r.zs != 0 || r.in_run || r.out_cs <= 0 ||
          r.out_keep <= 0 || r.out_keep > r.n_total)
        return hipErrorInvalidValue;
      if constexpr (N == 4096) {
        auto kern = row_fft4096_pair_strided_kernel<DIR>;
        hipError_t e = set_lds(kern, kR4kLds);
        if (e != hipSuccess) return e;
        const int64_t wgs = (r.out_keep + 1) / 2;  // one pair of output rows per workgroup
        if (wgs > INT32_MAX) return hipErrorInvalidValue;
        return launch_kernel(kern, dim3((unsigned)wgs, (unsigned)n_pol), dim3(NT), kR4kLds, s, r);
      } else {
        const size_t bytes = ((size_t)ROWS * RowShape<N>::RS + tw_slots(N)) * sizeof(float2);
        auto kern = row_fft_kernel<N, DIR, false, false, true>;
        hipError_t e = set_lds(kern, bytes);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)((r.n_rows + ROWS - 1) / ROWS), (unsigned)n_pol);
        return launch_kernel(kern, grid, dim3(NT), bytes, s, r);
      }
    } else {
      return hipErrorInvalidValue;
    }
  }
  if constexpr (N == 4096) {
    // persistent workgroups (row_fft_persist_kernel) once there are several rows per
    // resident workgroup; PFB_ROWFFT_PERSIST=0: one workgroup per row (A/B)
    static const bool off = knob("PFB_ROWFFT_PERSIST") && std::atoi(knob("PFB_ROWFFT_PERSIST")) == 0;
    const size_t bytes = row_fft_persist_lds<N>();
    const int per_cu = (int)std::max<size_t>(1, (160 * 1024) / bytes);
    const int64_t wgs = (int64_t)cu_count() * per_cu;
    // the explicit-pass kernel with per-pass twiddle tables (PFB_ROWFFT_4K=0: the generic
    // persistent kernel; PFB_ROWFFT_WPC: its workgroups per CU, default the 3 LDS allows —
    // experiments A/B)
    static const bool k4 = !(knob("PFB_ROWFFT_4K") && std::atoi(knob("PFB_ROWFFT_4K")) == 0);
    static const int wpc = knob("PFB_ROWFFT_WPC") ? std::atoi(knob("PFB_ROWFFT_WPC")) : 0;
    const int per_cu4 = wpc > 0 ? wpc : (int)std::max<size_t>(1, std::min<size_t>(3, (160 * 1024) / kR4kLds));
    // the pair kernel (no per-channel gain, no permutation but the padded index reversal;
    // output rows [row][N], or 2-row runs from an even first row without the time shift);
    // PFB_ROWFFT_PAIR=0: the one-row kernel (A/B)
    static const bool no_pair = knob("PFB_ROWFFT_PAIR") && std::atoi(knob("PFB_ROWFFT_PAIR")) == 0;
    if constexpr (!GAIN) {
      const bool ozs = r.zs == 1 && !r.remap && (r.row_base & 1) == 0 && (r.n_rows & 1) == 0;
      if (!off && k4 && !no_pair && (!PERM || r.rev) && (r.zs == 0 || ozs) && r.n_rows >= 2) {
        if (r.in_run) return ozs ? launch_row_fft4096_pair<DIR, PERM, true, true>(r, n_pol, s, per_cu4)
                                 : launch_row_fft4096_pair<DIR, PERM, true, false>(r, n_pol, s, per_cu4);
        return ozs ? launch_row_fft4096_pair<DIR, PERM, false, true>(r, n_pol, s, per_cu4)
                   : launch_row_fft4096_pair<DIR, PERM, false, false>(r, n_pol, s, per_cu4);
      }
    }
    if (!off && k4 && r.zs == 0 && r.n_rows >= 4 * (int64_t)cu_count() * per_cu4)
      return launch_row_fft4096<DIR, PERM, GAIN>(r, n_pol, s, per_cu4);
    if (!off && r.n_rows >= 4 * wgs) {
      auto kern = row_fft_persist_kernel<N, DIR, PERM, GAIN>;
      hipError_t e = set_lds(kern, bytes);
      if (e != hipSuccess) return e;
      dim3 grid((unsigned)std::max<int64_t>(1, wgs / n_pol), (unsigned)n_pol);
      return launch_kernel(kern, grid, dim3(NT), bytes, s, r);
    }
  }
  const size_t bytes = ((size_t)ROWS * RowShape<N>::RS + tw_slots(N)) * sizeof(float2);
  auto kern = row_fft_kernel<N, DIR, PERM, GAIN>;
  hipError_t e = set_lds(kern, bytes);
  if (e != hipSuccess) return e;
  dim3 grid((unsigned)((r.n_rows + ROWS - 1) / ROWS), (unsigned)n_pol);
  return launch_kernel(kern, grid, dim3(NT), bytes, s, r);
}

template <int N, int DIR>
static hipError_t launch_row_fft(const RowFftArgs& r, int n_pol, hipStream_t s) {
  if constexpr (DIR > 0) {
    if (r.perm && r.cgain) return launch_row_fft_t<N, DIR, true, true>(r, n_pol, s);
    if (r.perm) return launch_row_fft_t<N, DIR, true, false>(r, n_pol, s);
    if (r.cgain) return launch_row_fft_t<N, DIR, false, true>(r, n_pol, s);
  }
  return launch_row_fft_t<N, DIR, false, false>(r, n_pol, s);
}

template <int DIR>
hipError_t dispatch_row_fft(int N, const RowFftArgs& r, int n_pol, hipStream_t s) {
  switch (N) {
    case 8: return launch_row_fft<8, DIR>(r, n_pol, s);
    case 16: return launch_row_fft<16, DIR>(r, n_pol, s);
    case 32: return launch_row_fft<32, DIR>(r, n_pol, s);
    case 64: return launch_row_fft<64, DIR>(r, n_pol, s);
    case 128: return launch_row_fft<128, DIR>(r, n_pol, s);
    case 256: return launch_row_fft<256, DIR>(r, n_pol, s);
    case 512: return launch_row_fft<512, DIR>(r, n_pol, s);
    case 1024: return launch_row_fft<1024, DIR>(r, n_pol, s);
    case 2048: return launch_row_fft<2048, DIR>(r, n_pol, s);
    case 4096: return launch_row_fft<4096, DIR>(r, n_pol, s);
    default: break;
  }
  if constexpr (DIR > 0) {
    switch (N) {
      case 14: return launch_row_fft<14, DIR>(r, n_pol, s);
      case 28: return launch_row_fft<28, DIR>(r, n_pol, s);
      case 56: return launch_row_fft<56, DIR>(r, n_pol, s);
      case 112: return launch_row_fft<112, DIR>(r, n_pol, s);
      case 216: return launch_row_fft<216, DIR>(r, n_pol, s);
      case 224: return launch_row_fft<224, DIR>(r, n_pol, s);
      case 432: return launch_row_fft<432, DIR>(r, n_pol, s);
      case 448: return launch_row_fft<448, DIR>(r, n_pol, s);
      case 864: return launch_row_fft<864, DIR>(r, n_pol, s);
      case 192: return launch_row_fft<192, DIR>(r, n_pol, s);
      case 384: return launch_row_fft<384, DIR>(r, n_pol, s);
      case 768: return launch_row_fft<768, DIR>(r, n_pol, s);
      case 896: return launch_row_fft<896, DIR>(r, n_pol, s);
      case 1536: return launch_row_fft<1536, DIR>(r, n_pol, s);
      case 1792: return launch_row_fft<1792, DIR>(r, n_pol, s);
      case 3072: return launch_row_fft<3072, DIR>(r, n_pol, s);
      case 3584: return launch_row_fft<3584, DIR>(r, n_pol, s);
      default: break;
    }
  }
  return hipErrorInvalidValue;
}

template hipError_t dispatch_row_fft<-1>(int, const RowFftArgs&, int, hipStream_t);
template hipError_t dispatch_row_fft<+1>(int, const RowFftArgs&, int, hipStream_t);

bool chan_ifft_supported(int N) { return pow2_supported(N) || mixed_chan_supported(N); }

// ----------------------------------------------------------------- DADA row loader
// (N = 4096 keeps its pair / persistent kernels and their buffer-descriptor loads: staged)
bool chan_ifft_dada_supported(int N, int nbit) {
  return chan_ifft_supported(N) && N != 4096 && (nbit == 8 || nbit == 16);
}

template <int N, class T, bool LOWCBF>
static hipError_t launch_row_fft_dada(const RowFftArgs& r, const DadaIn& in, int n_pol, hipStream_t s) {
  constexpr int ROWS = RowShape<N>::ROWS;
  const size_t bytes = ((size_t)ROWS * RowShape<N>::RS + tw_slots(N)) * sizeof(float2);
  auto kern = row_fft_dada_kernel<N, T, LOWCBF, false, false>;
  hipError_t e = set_lds(kern, bytes);
  if (e != hipSuccess) return e;
  const int64_t tiles = (r.n_rows + ROWS - 1) / ROWS;
  // workgroups that share lines (DadaRows): the tile's polarisations, and in LowCBF order
  // the (up to 4) tiles of one heap.  Measured at the C2 shape against blockIdx order
  // (profiles/dada_synthesis_order_ab.jsonl): dual-pol TFP NBIT 16 0.210 vs 0.219 ms, LowCBF
  // 0.101 vs 0.103 (one pol) and 0.246 vs 0.247; dual-pol TFP NBIT 8 was slower grouped
  // (0.209 vs 0.197), so it keeps blockIdx order
  int share = LOWCBF ? n_pol * (ROWS < 32 ? std::min(4, (32 + ROWS - 1) / ROWS) : 1) : sizeof(T) == 2 ? n_pol : 1;
  if constexpr (kExperiments) {  // (PFB_DADA_SHARE=1: blockIdx order, A/B)
    static const int forced = knob("PFB_DADA_SHARE") ? std::atoi(knob("PFB_DADA_SHARE")) : 0;
    if (forced > 0) share = forced;
  }
  const int64_t gs = 8 * (int64_t)share;
  const int64_t wgs = (tiles * n_pol + gs - 1) / gs * gs;
  if (wgs > INT32_MAX) return hipErrorInvalidValue;
  const DadaRows d{in.base, in.t0, tiles, n_pol, share};
  return launch_kernel(kern, dim3((unsigned)wgs), dim3(NT), bytes, s, r, d);
}

template <class T, bool LOWCBF>
static hipError_t dispatch_row_fft_dada(int N, const RowFftArgs& r, const DadaIn& in, int n_pol, hipStream_t s) {
  switch (N) {
#define PFB_DADA_N(n) \
  case n: return launch_row_fft_dada<n, T, LOWCBF>(r, in, n_pol, s);
    PFB_DADA_N(8) PFB_DADA_N(16) PFB_DADA_N(32) PFB_DADA_N(64) PFB_DADA_N(128) PFB_DADA_N(256)
    PFB_DADA_N(512) PFB_DADA_N(1024) PFB_DADA_N(2048)
    PFB_DADA_N(14) PFB_DADA_N(28) PFB_DADA_N(56) PFB_DADA_N(112) PFB_DADA_N(192) PFB_DADA_N(216)
    PFB_DADA_N(224) PFB_DADA_N(384) PFB_DADA_N(432) PFB_DADA_N(448) PFB_DADA_N(768) PFB_DADA_N(864)
    PFB_DADA_N(896) PFB_DADA_N(1536) PFB_DADA_N(1792) PFB_DADA_N(3072) PFB_DADA_N(3584)
#undef PFB_DADA_N
    default: return hipErrorInvalidValue;
  }
}

// ----------------------------------------------------------------- strided row loader
// (N = 4096 keeps its pair / persistent kernels and their buffer-descriptor loads: staged)
bool chan_ifft_strided_supported(int N) { return chan_ifft_supported(N) && N != 4096; }

template <int N, bool PERM>
static hipError_t launch_row_fft_strided_t(const RowFftArgs& r, const StridedIn& in, int n_pol, hipStream_t s) {
  constexpr int ROWS = RowShape<N>::ROWS;
  const size_t bytes = ((size_t)ROWS * RowShape<N>::RS + tw_slots(N)) * sizeof(float2);
  auto kern = row_fft_strided_kernel<N, PERM>;
  hipError_t e = set_lds(kern, bytes);
  if (e != hipSuccess) return e;
  const int64_t tiles = (r.n_rows + ROWS - 1) / ROWS;
  // row_fft_kernel's own grid (blockIdx.y = pol).  Polarisations closer than a 128-B line
  // share lines inside every row (the inverse cascade's 112-B slices); handing 16 of them (16
  // ps elements = a whole number of lines) to one XCD back to back (StridedRows) measured
  // SLOWER at the SKA-Mid inverse cascade, 4096 x 14: 3.72-3.89 ms per call against 3.50-3.62
  // in this order (profiles/twostage_inverse_order_ab.jsonl), so it is an experiments knob only
  int share = 0;
  if constexpr (kExperiments) {  // (PFB_STRIDED_SHARE=n: groups of n polarisations per XCD; A/B)
    static const int forced = knob("PFB_STRIDED_SHARE") ? std::atoi(knob("PFB_STRIDED_SHARE")) : 0;
    if (forced > 0) share = std::min(forced, n_pol);
  }
  if (share > 0) {
    const int64_t gs = 8 * (int64_t)share;
    const int64_t wgs = (tiles * n_pol + gs - 1) / gs * gs;
    if (wgs > INT32_MAX) return hipErrorInvalidValue;
    return launch_kernel(kern, dim3((unsigned)wgs), dim3(NT), bytes, s, r, StridedRows{in, tiles, n_pol, share});
  }
  if (tiles > INT32_MAX || n_pol > 65535) return hipErrorInvalidValue;
  return launch_kernel(kern, dim3((unsigned)tiles, (unsigned)n_pol), dim3(NT), bytes, s, r,
                       StridedRows{in, tiles, n_pol, 0});
}

static hipError_t dispatch_row_fft_strided(int N, const RowFftArgs& r, const StridedIn& in, int n_pol, hipStream_t s) {
  switch (N) {
#define PFB_STRIDED_N(n)                                                          \
  case n:                                                                         \
    return r.perm ? launch_row_fft_strided_t<n, true>(r, in, n_pol, s)            \
                  : launch_row_fft_strided_t<n, false>(r, in, n_pol, s);
    PFB_STRIDED_N(8) PFB_STRIDED_N(16) PFB_STRIDED_N(32) PFB_STRIDED_N(64) PFB_STRIDED_N(128)
    PFB_STRIDED_N(256) PFB_STRIDED_N(512) PFB_STRIDED_N(1024) PFB_STRIDED_N(2048)
    PFB_STRIDED_N(14) PFB_STRIDED_N(28) PFB_STRIDED_N(56) PFB_STRIDED_N(112) PFB_STRIDED_N(192)
    PFB_STRIDED_N(216) PFB_STRIDED_N(224) PFB_STRIDED_N(384) PFB_STRIDED_N(432) PFB_STRIDED_N(448)
    PFB_STRIDED_N(768) PFB_STRIDED_N(864) PFB_STRIDED_N(896) PFB_STRIDED_N(1536) PFB_STRIDED_N(1792)
    PFB_STRIDED_N(3072) PFB_STRIDED_N(3584)
#undef PFB_STRIDED_N
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_chan_ifft(const ChanIfftArgs& c, hipStream_t s) {
  if (c.n_rows <= 0) return hipSuccess;
  // (the stage-1 rows are read by the synthesis right after: default store policy while they
  // fit the 256 MB Infinity Cache with room to spare — the nontemporal rows of the generic
  // policy made the synthesis-only C2 path's block kernel read them from HBM)
  bool fits = (double)c.n_pol * c.n_rows * c.N * 8.0 <= 160.0 * (1 << 20);
  if constexpr (kExperiments) {  // (PFB_CHAN_IFFT_NT=1: nontemporal as before, A/B)
    static const bool force_nt = knob("PFB_CHAN_IFFT_NT") && std::atoi(knob("PFB_CHAN_IFFT_NT")) == 1;
    if (force_nt) fits = false;
  }
  RowFftArgs r{c.in, c.in_pol_stride, c.out, c.out_pol_stride, c.n_rows, c.perm, c.cgain, c.twN,
               1.0f, 0, 0, 0, c.n_rows, c.zblk == 4 ? 2 : c.zblk == 2 ? 1 : 0, fits ? 0 : 1};
  if (c.zblk != 1 && c.zblk != 2 && c.zblk != 4) return hipErrorInvalidValue;
  if (c.dada) {
    const DadaIn& d = *c.dada;
    // the loader has no permutation or gain instantiation, and reads whole complex samples
    // of rows [t0, t0 + n_rows) of the section
    if (c.perm || c.cgain || !chan_ifft_dada_supported(c.N, d.nbit) || d.t0 < 0 || d.t0 + c.n_rows > d.n_dat ||
        (d.lowcbf && d.n_dat % 32) || reinterpret_cast<uintptr_t>(d.base) % (size_t)(d.nbit / 4))
      return hipErrorInvalidValue;
    if (d.nbit == 8)
      return d.lowcbf ? dispatch_row_fft_dada<int8_t, true>(c.N, r, d, c.n_pol, s)
                      : dispatch_row_fft_dada<int8_t, false>(c.N, r, d, c.n_pol, s);
    return d.lowcbf ? dispatch_row_fft_dada<int16_t, true>(c.N, r, d, c.n_pol, s)
                    : dispatch_row_fft_dada<int16_t, false>(c.N, r, d, c.n_pol, s);
  }
  if (c.strided) {
    const StridedIn& d = *c.strided;
    // the loader has no gain instantiation, and reads rows [t0, t0 + n_rows) of the layout
    if (c.cgain || !chan_ifft_strided_supported(c.N) || !d.base || d.ps <= 0 || d.rs <= 0 || d.cs <= 0 ||
        d.t0 < 0 || d.t0 + c.n_rows > d.n_dat)
      return hipErrorInvalidValue;
    return dispatch_row_fft_strided(c.N, r, d, c.n_pol, s);
  }
  return dispatch_row_fft<+1>(c.N, r, c.n_pol, s);
}

}  // namespace pfb
