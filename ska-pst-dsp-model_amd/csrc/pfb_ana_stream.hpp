// pfb_ana_stream.hpp — the streaming Bunton analysis for N = 256 (polyphase_analysis.m:83-121),
// analysis_stream_kernel (instantiated in pfb_analysis.hip).
#pragma once
#include <type_traits>

#include "pfb_common.hpp"
#include "pfb_dada_store.hpp"
#include "pfb_sample.hpp"

namespace pfb {


// Bunton analysis for N = 256 with the FIR in registers and no LDS staging of the
// input.  View the input as rows of N samples, X[r][c] = x[r N + c].  With M = N DE/NU,
// output row k = NU q + s (s < NU) starts at kM = DE N q + sM, and the circular shift
// of polyphase_analysis.m:102-105 moves arm n to position (n + sM) mod N.  The thread
// that owns position c therefore computes, for every s, arm n_s = (c - a_s) mod N with
// a_s = sM mod N, and its samples are one COLUMN of X:
//     v_k[c] = sum_m f[m N + n_s] X[DE q + m + b_s + e_s][c],
//     b_s = floor(sM / N), e_s = [c < a_s].
// Folding e_s into the taps (g_s[m'] = f[(m' - e_s) N + n_s] = F[(m' + 1) N + c - a_s]
// with F = [N zeros, f, zeros], P + 1 taps) makes the row index DE q + m' + b_s a
// compile-time offset into a register window that slides down the column: each input
// sample is loaded once, coalesced (a wave reads 512 contiguous bytes of one row), and
// the circshift costs nothing — v_k[c] is already at its shifted position.  The taps
// are read from LDS (lane-contiguous, conflict-free; each read feeds QS rows);
// T = 16 rows per step go to LDS for the N-point FFT.
template <int N, int P, int NU, int DE>
struct StreamShape {
  static_assert(N == NT, "one thread per column");
  static_assert(16 % NU == 0, "NU must divide 16");
  static constexpr int M = N * DE / NU;
  static_assert(M * NU == N * DE, "M = N de/nu must be integral");
  static constexpr int PE = P + 1;        // taps per chain after folding e_s
  static constexpr int QS = 16 / NU;      // commutator periods per step
  static constexpr int T = QS * NU;       // output rows per step (16)
  static constexpr int NEW = DE * QS;     // input rows consumed per step
  static constexpr int WIN = NEW + PE - 1;  // register window (rows)
  static constexpr int RS = lds_row(N);
  static constexpr int TW_OFF = T * RS;               // float2 offset of the twiddles
  static constexpr int F_OFF = 2 * (TW_OFF + tw_slots(N));  // float offset of the taps F
  static constexpr int F_LEN = (P + 2) * N;
  static constexpr size_t lds_bytes = (size_t)F_OFF * sizeof(float) + F_LEN * sizeof(float);
};

// The input fetch of the analysis kernels that read a series through a buffer descriptor
// (analysis_stream_body, fir_lds_body): kBytes per complex sample, one range-checked buffer
// load each (raw_t: what the prefetch registers hold), converted to (re, im) float when the
// sample enters the FIR.  InCf32: the packed [pol][t] complex float32 series.  InDada8 / 16 /
// 32: a single-channel DADA section in TFP order, NDIM 2 (AnalysisArgs::din), read in place —
// sample t of polarisation p at byte ((t n_pol + p) kBytes); the integer cast is exact and a
// load outside the descriptor returns 0 = 0.0f, so the FIR sees the values pfb_dada_unpack
// would have written.
struct InCf32 {
  static constexpr bool kDada = false;
  static constexpr int kBytes = 8;
  using raw_t = v2f;
  template <int AUX>
  static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, AUX));
  }
  static __device__ __forceinline__ raw_t gload(const void* p) { return *reinterpret_cast<const v2f*>(p); }
  static __device__ __forceinline__ v2f cvt(raw_t v) { return v; }
};
struct InDada32 : InCf32 {  // NBIT 32: float (re, im), pols interleaved
  static constexpr bool kDada = true;
};
struct InDada16 {  // NBIT 16: int16 (re, im)
  static constexpr bool kDada = true;
  static constexpr int kBytes = 4;
  using raw_t = uint32_t;
  template <int AUX>
  static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX);
  }
  static __device__ __forceinline__ raw_t gload(const void* p) { return *reinterpret_cast<const uint32_t*>(p); }
  static __device__ __forceinline__ v2f cvt(raw_t v) {
    return v2f{(float)(int16_t)(v & 0xffffu), (float)(int16_t)(v >> 16)};
  }
};
struct InDada8 {  // NBIT 8: int8 (re, im)
  static constexpr bool kDada = true;
  static constexpr int kBytes = 2;
  using raw_t = uint16_t;
  template <int AUX>
  static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, AUX);
  }
  static __device__ __forceinline__ raw_t gload(const void* p) { return *reinterpret_cast<const uint16_t*>(p); }
  static __device__ __forceinline__ v2f cvt(raw_t v) {
    return v2f{(float)(int8_t)(v & 0xffu), (float)(int8_t)(v >> 8)};
  }
};

// The store side of the same kernel (analysis_stream_body's OUT; pfb_dada_store.hpp).  OutCf32:
// the packed [pol][k][c] complex float32 rows (BufRowStore / LcbfRowStore and the strided
// stores).  OutDada8 / 16 / 32: a TFP DADA section, NDIM 2 (AnalysisArgs::dout), through
// DadaRowStore (cache policy kAuxDadaOut).

// Rows [k0, k0 + T) of a DADA section of C channels and P polarisations, polarisation `pol`
// (BufRowStore's twin; LCBF: LcbfRowStore's bin -> channel map and drop rule, C = 216): FFT bin
// f of row `row` is the complex sample at byte ((row C + c) P + pol) kBytes of the step's
// first row, its value to_sample(oscale * (scale * v)) per component — the float32 products of
// the cf32 store followed by the caller's scale and pfb_dada_pack, in that order.  The
// descriptor covers the step's valid rows (all of both polarisations: a workgroup fills every
// P-th sample); rows below `lo` and dropped bins are sent out of its range, rows at or above
// the extent are dropped by the range check.  No branch around the store.
template <class OUT, int N, bool LCBF>
struct DadaRowStore {
  static constexpr bool kIsLds = false;
  static constexpr int C = LCBF ? 216 : N;
  __amdgpu_buffer_rsrc_t r;
  int lo, P, pol;
  float scale, oscale;
  __device__ __forceinline__ void store(int row, int f, float2 v) const {
    const int c = LCBF ? ((f + 108) & 255) : f;
    const bool ok = (row >= lo) & (c < C);
    const uint32_t off = ok ? (uint32_t)(((row * C + c) * P + pol) * OUT::kBytes) : 0xFFFFFFF0u;
    const float2 x = cscale(v, scale);
    OUT::store(r, off, oscale * x.x, oscale * x.y);
  }
  __device__ __forceinline__ static DadaRowStore rows(void* base, int64_t k0, int T, int64_t k_lo, int64_t k_hi,
                                                       int P, int pol, float scale, float oscale) {
    const int64_t hi = min(max(k_hi - k0, (int64_t)0), (int64_t)T);
    const int lo = (int)min(max(k_lo - k0, (int64_t)0), (int64_t)T);
    const int64_t row_bytes = (int64_t)C * P * OUT::kBytes;
    return DadaRowStore{make_rsrc_u(static_cast<char*>(base) + k0 * row_bytes, (uint32_t)(hi * row_bytes)), lo, P,
                        pol, scale, oscale};
  }
};

// The quantised product's moments (analysis_stream_moments_kernel): a row store (BufRowStore /
// LcbfRowStore) that forwards store() and adds the float32 value that goes to memory — after the
// store's scale * v — into the thread's double sums m = {sum re, sum im, sum re^2 + im^2}.  A
// sample counts only where the store lands: rows [lo, hi) of the step, and for LowCBF the 216
// kept bins; a select, no branch and no memory operation.
template <class ST, bool LCBF>
struct MomentRowStore {
  static constexpr bool kIsLds = false;
  ST st;
  int hi;
  double* m;
  __device__ __forceinline__ void store(int row, int f, float2 v) const {
    st.store(row, f, v);
    bool ok = (row >= st.lo) & (row < hi);
    if constexpr (LCBF) ok = ok & (((f + 108) & 255) < 216);
    const float2 x = cscale(v, st.scale);
    const double re = ok ? (double)x.x : 0.0, im = ok ? (double)x.y : 0.0;
    m[0] += re;
    m[1] += im;
    m[2] = fma(re, re, fma(im, im, m[2]));
  }
};

// ZOUT (round trip): each step's channelised rows are also inverse-transformed across
// channels in LDS and written as synthesis stage-1 rows (AnalysisArgs::z), so the
// synthesis does not re-read them from HBM.
// LCBF: the SKA-Low CBF PST filterbank (polyphase_analysis_lowcbf.m / PSTFilterbank.m,
// N 256, M 192, 12 taps) through the same FIR: its FFT of the UNshifted sums times the
// derotation i^{k (j - 128)} equals the FFT of the Bunton-shifted sums v_k (the shift
// r = 192 k mod 256 is a multiple of 64, e^{-2 pi i f r / 256} = i^{k f}, exact), and
// fftshift + the 216-channel selection is output channel c = (f - 148) mod 256 < 216,
// scaled by 2^12 (LowCbfArgs::scale).  Leading pre-padding zeros via AnalysisArgs::pad.
// The last FFT pass's output staged channel-major in the LDS rows' space (channel c at
// c * (T + 1), odd stride: conflict-light column writes and row-pair reads) for the
// channel-major store of a strided launch (out_rs = 1).
template <int T>
struct ColMajorLds {
  static constexpr bool kIsLds = true;
  float2* b;
  __device__ __forceinline__ void store(int row, int c, float2 v) const { b[c * (T + 1) + row] = v; }
  __device__ __forceinline__ float2 load(int row, int c) const { return b[c * (T + 1) + row]; }
};

// timing variant TV 16: a store functor that only keeps the value live (no instruction)
struct SinkStore {
  static constexpr bool kIsLds = false;
  __device__ __forceinline__ void store(int, int, float2 v) const { asm volatile("" ::"v"(v)); }
};

// ZOUT: 0 no stage-1 rows; 1 rows [row][c] (AnalysisArgs::z); 2 / 4: runs of ZOUT rows per
// column (AnalysisArgs::zblk) for the synthesis wave kernel.
// Streaming analysis of step range w of nw (steps of T rows from row0) for polarisation
// pol.
// TV: compile-time timing variants (experiments build only, results invalid): 1 no FIR (one
// window row per output row instead of the PE-tap sums), 2 no FFT (no channelised rows), 4 no
// window slide (the prefetched rows are not moved into the window), 16 the FFT without its
// channelised-row stores (17 of the kernel's 80 us, r06_v16; written instead as whole 1-KB
// runs from the wave-owned LDS rows they took 2 us MORE, r06_v17 — rejected); 8 (valid, the A/B of
// round 6): workgroup barriers inside the FFT (the pre-round-6 form)
// The step's N-point FFT: thread c's butterfly of both radix-16 passes lies in row c / 16, so
// wave w owns rows 4w .. 4w + 3 for the whole transform (wave_rows_ok) and the two barriers
// inside it are wave barriers (round 6; timing variants r06_v14: the FFT was 30 of the
// kernel's 78 us with four workgroup barriers a step, memory traffic masked or not)
// IN: the input fetch (InCf32, or a DADA section read in place)
// OUT: the product's store (OutCf32, or a DADA section written in place: ZOUT 0, GS 0 — and the
// file-to-file round trip's one combination, a section read in place, the NBIT 32 float product
// section and the 2-row runs: ZOUT 2, IN a DADA class, OutDada32)
// MOM: the plain cf32 product with its moments (MomentRowStore): the workgroup's three sums go
// to a.mom[(pol nw + w) 3 ...] with ordinary stores, zeros from a workgroup without steps
// QIN: the input quantiser at the load (FilterBank.m:75-83; pfb_analysis_set_input_quantiser,
// FUSED): every new sample enters the FIR as roundf(sf * IN::cvt(raw)) per component, sf =
// (float)a.qin[3] (the plan's block, one scalar load; 1 without a block) — the first window and
// the rows converted when the window slides; the prefetch registers keep the file values, the
// carried samples (`pre`) are added as they are, a load outside the descriptor gives
// roundf(sf * 0) = 0, and the carry copy writes the rounded values
template <int N, int P, int NU, int DE, int ZOUT, bool LCBF, int GS, int TV = 0, class IN = InCf32,
          class OUT = OutCf32, bool MOM = false, bool QIN = false>
__device__ __forceinline__ void analysis_stream_body(const AnalysisArgs& a, int pol, int w, int nw) {
  static_assert(!MOM || (!OUT::kDada && ZOUT == 0 && GS == 0 && TV == 0), "moments: the plain cf32 product");
  static_assert(!QIN || (!OUT::kDada && ZOUT == 0 && GS == 0 && TV == 0), "input quantiser: the plain cf32 product");
  static_assert(!OUT::kDada || (GS == 0 && TV == 0 &&
                                (ZOUT == 0 || (ZOUT == 2 && !LCBF && IN::kDada && std::is_same<OUT, OutDada32>::value))),
                "the DADA store: the plain product, or the round trip's float section with 2-row runs");
  using SH = StreamShape<N, P, NU, DE>;
  constexpr int M = SH::M, PE = SH::PE, QS = SH::QS, T = SH::T, NEW = SH::NEW, WIN = SH::WIN;
  constexpr bool kWR = (TV & 8) == 0 && wave_rows_ok<N, T, NT>();
  extern __shared__ __attribute__((aligned(16))) float2 smem[];
  const int c = threadIdx.x;
  [[maybe_unused]] float sf = 1.f;
  if constexpr (QIN) {
    if (a.qin) sf = (float)a.qin[3];
  }
  // a sample as it enters the FIR
  auto cvt = [&](typename IN::raw_t raw) {
    const v2f v = IN::cvt(raw);
    if constexpr (QIN) return v2f{roundf(sf * v.x), roundf(sf * v.y)};
    else return v;
  };
  if constexpr (ZOUT == 0 && !LCBF) {  // (stream objects only: no round-trip / LowCBF kernel)
  if (a.carry_out) {
    // the next call's carry, grid-stride over this polarisation's workgroups (its few
    // thousand samples are a fraction of one row of work per workgroup); before any early
    // return, so every workgroup takes its share
    // (a uniform loop with a per-lane guard — no lane-dependent trip count)
    float2* dst = a.carry_out + pol * a.carry_pol_stride;
    if constexpr (IN::kDada) {
      // (the carry stays packed cf32: converted as it is copied)
      const int64_t step = (int64_t)a.n_pol * IN::kBytes;
      const char* src = static_cast<const char*>(a.din) + pol * IN::kBytes + a.carry_src * step;
      for (int64_t i0 = (int64_t)w * NT; i0 < a.carry_n; i0 += (int64_t)nw * NT) {
        const int64_t i = i0 + c;
        if (i < a.carry_n) {
          const v2f v = cvt(IN::gload(src + i * step));
          dst[i] = make_float2(v.x, v.y);
        }
      }
    } else {
    const float2* src = a.in + pol * a.in_pol_stride + a.carry_src;
    for (int64_t i0 = (int64_t)w * NT; i0 < a.carry_n; i0 += (int64_t)nw * NT) {
      const int64_t i = i0 + c;
      if constexpr (QIN) {
        if (i < a.carry_n) dst[i] = make_float2(roundf(sf * src[i].x), roundf(sf * src[i].y));
      } else {
      if (i < a.carry_n) dst[i] = src[i];
      }
    }
    }
  }
  }
  // this workgroup's steps (XCD-aware order: neighbouring ranges share halo rows in L2)
  const int64_t q_lo = a.row0 / NU;
  const int64_t n_steps = ((a.K + NU - 1) / NU - q_lo + QS - 1) / QS;
  const int64_t st0 = n_steps * w / nw, st1 = n_steps * (w + 1) / nw;
  if constexpr (MOM) {
    if (st0 >= st1 && c == 0) {
      double* slot = a.mom + ((int64_t)pol * nw + w) * 3;
      slot[0] = slot[1] = slot[2] = 0.0;
    }
  }
  if (st0 >= st1) return;
  [[maybe_unused]] double mom[3] = {0.0, 0.0, 0.0};

  // input column c from row DE q_first on; range-checked buffer loads return 0 past n_dat
  const int64_t row_first = (int64_t)DE * (q_lo + st0 * QS);
  // window row r, column c is x[(row_first + r) N + c - pad]: the descriptor starts at the
  // first real sample the range reads; pre-padding rows give negative offsets, which wrap
  // past the range check and read as zeros
  const int64_t g0 = row_first * N - a.pad;
  const int64_t gb = max(g0, (int64_t)0);
  const int shift = (int)(g0 - gb);
  const int64_t avail = a.n_dat - gb;
  // the launcher sizes the ranges so that a workgroup's rows span <= kRsrcMaxBytes
  // (launch_stream); the min() only bounds the series tail beyond the range
  uint32_t nbytes;
  const void* xb;
  // bytes from one sample of this polarisation to its next
  int sstep = 8;
  if constexpr (IN::kDada) {
    // a DADA section: the descriptor starts at this polarisation's sample gb and ends with
    // the last byte of its last sample, and every offset is a multiple of the step — no
    // byte of the partner polarisation, and none outside the section, is loaded
    sstep = a.n_pol * IN::kBytes;
    xb = static_cast<const char*>(a.din) + pol * IN::kBytes + gb * (int64_t)sstep;
    nbytes = avail > 0 ? (uint32_t)min((avail - 1) * (int64_t)sstep + IN::kBytes, kRsrcMaxBytes) : 0u;
  } else {
    xb = a.in + pol * a.in_pol_stride + gb;
    nbytes = (uint32_t)min(max(avail, (int64_t)0) * 8, kRsrcMaxBytes);
  }
  if (tmask(a.timing_mask) & 1) nbytes = 0;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(xb, nbytes);
  // rows past the last window of the range (the unconditional last prefetch) re-read the
  // last row instead: an L2 hit rather than HBM traffic nobody uses
  const int r_last = (int)(st1 - st0 - 1) * NEW + WIN - 1;
  auto ld = [&](int r) {  // window row r (relative to row_first)
    if constexpr (IN::kDada) return IN::template load<kAuxIn>(xr, (uint32_t)((min(r, r_last) * N + c + shift) * sstep));
    else return IN::template load<kAuxIn>(xr, (uint32_t)((min(r, r_last) * N + c + shift) * 8));
  };
  // (re, im) as a packed pair: one v_pk_fma_f32 per complex x real tap MAC
  v2f win[WIN];
  if (a.pre != nullptr && g0 < 0) {
    // a stream object's carried samples in front of the input: window sample (row i, column
    // c) is sample (row_first + i) N + c of the carry-then-input series; below pad it is
    // pre[pol][...], at or above it the input (each range-checked load returns 0 outside
    // its part, so the sum is the one sample)
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(a.pre + pol * a.pre_pol_stride, (uint32_t)(a.pad * 8));
#pragma unroll
    for (int i = 0; i < WIN; ++i) {
      const v2u pv = __builtin_amdgcn_raw_buffer_load_b64(pr, (uint32_t)(((row_first + i) * N + c) * 8), 0, 0);
      win[i] = cvt(ld(i)) + __builtin_bit_cast(v2f, pv);
    }
  } else {
#pragma unroll
    for (int i = 0; i < WIN; ++i) win[i] = cvt(ld(i));
  }

  // LDS: twiddles behind the FFT rows, then F = [N zeros, taps, zeros]
  float* F = reinterpret_cast<float*>(smem) + SH::F_OFF;
  smem[SH::TW_OFF + tw_slot(c)] = a.twN[c];
#pragma unroll
  for (int m = 0; m < P + 2; ++m) F[m * N + c] = (m >= 1 && m <= P) ? a.taps[(m - 1) * N + c] : 0.f;

  float2* opol = a.out + pol * a.out_pol_stride;
  float2* zpol = ZOUT ? a.z + pol * a.z_pol_stride - a.z_row0 * N : nullptr;  // Z row k - z_row0
  LdsRows rows(smem, SH::RS);
  const float2* tw = smem + SH::TW_OFF;
  vm_drain();
#pragma unroll 1
  for (int64_t stp = st0; stp < st1; ++stp) {
    const int rel = (int)(stp - st0) * NEW;  // window row 0 of this step
    // prefetch the next step's new rows (consumed when the window slides)
    // (unconditional: past the range it reads rows nobody uses, or zeros past n_dat —
    // a conditional prefetch makes vmcnt path-dependent and the next step waits for
    // every store as well)
    // (a DADA section: the packed file values, converted when the window slides)
    typename IN::raw_t pf[NEW];
#pragma unroll
    for (int i = 0; i < NEW; ++i) pf[i] = ld(rel + WIN + i);
    __syncthreads();  // previous step's FFT has read its rows (first step: F staged)
    // all NU x QS rows accumulate together (tap-outer order): consecutive FMAs are
    // independent, so the 4-cycle FMA latency never stalls issue
    v2f acc[NU][QS];
    static_for<0, NU>([&](auto sv) {
#pragma unroll
      for (int qq = 0; qq < QS; ++qq) acc[decltype(sv)::value][qq] = v2f{0.f, 0.f};
    });
    if constexpr ((TV & 1) != 0) {
      static_for<0, NU>([&](auto sv) {
        static_for<0, QS>([&](auto qv) {
          acc[decltype(sv)::value][decltype(qv)::value] = win[DE * decltype(qv)::value + decltype(sv)::value];
        });
      });
    } else
    static_for<0, PE>([&](auto mv) {
      constexpr int m = decltype(mv)::value;
      float gm[NU];
      static_for<0, NU>([&](auto sv) {
        constexpr int s = decltype(sv)::value;
        gm[s] = F[(m + 1) * N + c - (s * M) % N];
      });
      static_for<0, NU>([&](auto sv) {
        constexpr int s = decltype(sv)::value;
        constexpr int bs = (s * M) / N;
        static_for<0, QS>([&](auto qv) {
          constexpr int qq = decltype(qv)::value;
          acc[s][qq] = __builtin_elementwise_fma(v2f{gm[s], gm[s]}, win[DE * qq + m + bs], acc[s][qq]);
        });
      });
    });
    const int64_t k0 = (q_lo + stp * QS) * NU;
    // ZOUT: the synthesis stage-1 row of output row k is the N-point inverse DFT across
    // channels of out[k] = N FFT_N(v_k), i.e. N^2 v_k exactly — the FIR output this
    // thread already holds at position c (v_k[c]).  It goes to HBM straight from the
    // registers (no inverse FFT; N^2 is a power of two, so the scaling is exact).
    const BufRowStore zs = BufRowStore::rows(ZOUT ? zpol : opol, k0, T, max(a.row0, a.z_row0), a.K,
                                             N, (float)N * (float)N);
    // ZOUT >= 2: the step's T = 16 rows of column c are 16 / ZOUT runs of this column, row
    // k - z_row0 = ZB g + gi at z[pol][(g N + c) ZB + gi]; rows (2m, 2m+1) go out as one 16-B
    // store once both are summed (the launcher guarantees that k0 - z_row0 is a multiple
    // of 16; rows past K land in the buffer's padding)
    const int64_t kz = k0 - a.z_row0;
    const __amdgpu_buffer_rsrc_t zb =
        make_rsrc(ZOUT >= 2 ? a.z + pol * a.z_pol_stride + max(kz, (int64_t)0) * N : opol,
                  (ZOUT >= 2 && kz >= 0 && !(tmask(a.timing_mask) & 4)) ? (uint32_t)(N * T * 8) : 0u);
    static_for<0, NU>([&](auto sv) {
      constexpr int s = decltype(sv)::value;
      static_for<0, QS>([&](auto qv) {
        constexpr int qq = decltype(qv)::value;
        const float2 v = make_float2(acc[s][qq].x, acc[s][qq].y);
        rows.store(qq * NU + s, c, v);
        if constexpr (ZOUT == 1) zs.store(qq * NU + s, c, v);
        if constexpr (ZOUT >= 2 && (s & 1)) {
          constexpr int r1 = qq * NU + s, r0 = r1 - 1;
          constexpr float n2 = (float)N * (float)N;
          const v2f a0 = acc[s - 1][qq] * n2, a1 = acc[s][qq] * n2;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v4f{a0.x, a0.y, a1.x, a1.y}), zb,
                                                 (uint32_t)((((r0 / ZOUT) * N + c) * ZOUT + r0 % ZOUT) * 8), 0,
                                                 kAuxZst);
        }
      });
    });
    __syncthreads();
    if constexpr ((TV & 2) != 0) {
    } else if constexpr (OUT::kDada) {
      // the quantised product, straight into the caller's section (per-step descriptor, one
      // always-issued store per complex sample, as the cf32 row stores)
      const DadaRowStore<OUT, N, LCBF> st = DadaRowStore<OUT, N, LCBF>::rows(
          a.dout, k0, T, a.row0, a.K, a.n_pol, pol, LCBF ? a.lcbf_scale : (float)N, a.dout_scale);
      block_fft<N, -1, T, NT, kWR>(rows, st, rows, tw, c);
    } else if constexpr (LCBF) {
      const LcbfRowStore st = LcbfRowStore::rows(opol, k0, T, a.row0, a.K, a.lcbf_scale);
      if constexpr (MOM) {
        const int hi = (int)min(max(a.K - k0, (int64_t)0), (int64_t)T);
        block_fft<N, -1, T, NT, kWR>(rows, MomentRowStore<LcbfRowStore, true>{st, hi, mom}, rows, tw, c);
      } else
      block_fft<N, -1, T, NT, kWR>(rows, st, rows, tw, c);
    } else if constexpr (GS == 2) {
      // channel-major (a cascade's stage-2 series, out_rs = 1, no chomp): the last pass
      // lands in LDS by channel, then each 8-lane group writes one channel's T = 16
      // consecutive samples as 8 x 16 B (one 128-B run) instead of 16 scattered 8-B stores.
      // The launch's first and last rows are even (launch_stream checks), so a row pair is
      // valid or not as a whole: one store per pair, always issued, invalid pairs sent out
      // of the descriptor's range.  (Stores under a branch made the count path-dependent,
      // and the loop-end wait for the next step's rows then waited for the stores as well;
      // the strided store (GS 1) is a kernel of its own for the same reason: a different
      // store count per step.)
      static_assert(N * (T + 1) <= T * SH::RS, "channel-major staging exceeds the LDS rows");
      const ColMajorLds<T> cm{smem};
      block_fft<N, -1, T, NT, kWR>(rows, cm, rows, tw, c);
      __syncthreads();
      const int hi = (int)min(max(a.K - k0, (int64_t)0), (int64_t)T);
      const int lo = (int)min(max(a.row0 - k0, (int64_t)0), (int64_t)T);
      const __amdgpu_buffer_rsrc_t r =
          make_rsrc_u(opol + k0, hi > 0 ? (uint32_t)(((int64_t)(N - 1) * a.out_cs + hi) * 8) : 0u);
      static_for<0, (T / 2) * N / NT>([&](auto iv) {
        const int idx = c + decltype(iv)::value * NT;
        const int ch = idx / (T / 2), r0 = 2 * (idx % (T / 2));
        const float2 v0 = cscale(cm.load(r0, ch), (float)N), v1 = cscale(cm.load(r0 + 1, ch), (float)N);
        const uint32_t off = (r0 >= lo && r0 + 1 < hi) ? (uint32_t)((ch * a.out_cs + r0) * 8) : 0xFFFFFFF0u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v4f{v0.x, v0.y, v1.x, v1.y}), r, off, 0,
                                               kAuxColMajor);
      });
    } else if constexpr (GS == 1) {
      const StridedRowStore st = StridedRowStore::rows(opol, k0, T, a.row0, a.K, a.out_rs, a.out_cs,
                                                       a.sel_split, a.sel_shift, a.sel_n, N, (float)N);
      block_fft<N, -1, T, NT, kWR>(rows, st, rows, tw, c);
    } else if constexpr ((TV & 16) != 0) {
      // (timing variant: the FFT computed, its channelised rows not stored — kept live only)
      block_fft<N, -1, T, NT, kWR>(rows, SinkStore{}, rows, tw, c);
    } else {
      // (timing mask bit 1, experiments build: no channelised stores)
      const BufRowStore st = BufRowStore::rows(opol, k0, T, a.row0, (tmask(a.timing_mask) & 2) ? k0 : a.K, N, (float)N);
      if constexpr (MOM) {
        const int hi = (int)min(max(a.K - k0, (int64_t)0), (int64_t)T);
        block_fft<N, -1, T, NT, kWR>(rows, MomentRowStore<BufRowStore, false>{st, hi, mom}, rows, tw, c);
      } else
      block_fft<N, -1, T, NT, kWR>(rows, st, rows, tw, c);
    }
    if constexpr ((TV & 4) != 0) {
      // (keep the prefetched rows live: an empty use)
#pragma unroll
      for (int i = 0; i < NEW; ++i) asm volatile("" ::"v"(pf[i]));
    } else {
#pragma unroll
    for (int i = 0; i < PE - 1; ++i) win[i] = win[i + NEW];
#pragma unroll
    for (int i = 0; i < NEW; ++i) win[PE - 1 + i] = cvt(pf[i]);
    }
  }
  if constexpr (MOM) {
    // the workgroup's sums in a fixed order: wave shuffles, then the four waves' values through
    // LDS (behind a barrier: the last step's FFT rows live there), one lane stores the slot
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mom[0] += __shfl_down(mom[0], off, 64);
      mom[1] += __shfl_down(mom[1], off, 64);
      mom[2] += __shfl_down(mom[2], off, 64);
    }
    static_assert(NT == 256, "four waves");
    double* red = reinterpret_cast<double*>(smem);
    __syncthreads();
    if ((c & 63) == 0) {
      red[(c >> 6) * 3 + 0] = mom[0];
      red[(c >> 6) * 3 + 1] = mom[1];
      red[(c >> 6) * 3 + 2] = mom[2];
    }
    __syncthreads();
    if (c == 0) {
      double* slot = a.mom + ((int64_t)pol * nw + w) * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) slot[j] = (red[j] + red[3 + j]) + (red[6 + j] + red[9 + j]);
    }
  }
}

// WPE: waves per SIMD the register allocation targets (2: 184 VGPRs for the C2 round trip;
// 3: <= 168, three 51-KB workgroups per CU)
template <int N, int P, int NU, int DE, int ZOUT, bool LCBF = false, int GS = 0, int WPE = 2, int TV = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WPE))) void analysis_stream_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, ZOUT, LCBF, GS, TV>(a, blockIdx.y, w, gridDim.x);
}

// The same kernel reading a DADA section in place (IN: InDada8 / 16 / 32; AnalysisArgs::din):
// the plain channelised product ([k][c], or the LowCBF 216 channels), stateless or stream
// calls — the carry comes through the cf32 `pre` descriptor as ever.  A kernel of its own
// name, so the cf32 kernels' symbols — the keys of the recorded profiles — stay as they are.
template <int N, int P, int NU, int DE, bool LCBF, class IN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_dada_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 0, LCBF, 0, 0, IN>(a, blockIdx.y, w, gridDim.x);
}

// The same kernel storing its product as a DADA section (OUT: OutDada8 / 16 / 32;
// AnalysisArgs::dout), from packed cf32 input or from a DADA section of the same NBIT read in
// place.  A kernel of its own name again (pfb_ana_stream_dadaout.hip instantiates them).
template <int N, int P, int NU, int DE, bool LCBF, class IN, class OUT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_dadaout_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 0, LCBF, 0, 0, IN, OUT>(a, blockIdx.y, w, gridDim.x);
}

// The round trip's kernel (ZOUT 2: the stage-1 rows in 2-row runs, stored as ever) reading a
// DADA section in place and storing its product as the NBIT 32 float section of the channelised
// file (AnalysisArgs::din, dout with dout_scale 1: 1.0f * x keeps every bit of x, so the section
// holds the cf32 kernel's product) — pfb_roundtrip_execute_dada_to_dada.  A kernel of its own
// name again (pfb_ana_stream_rtdada.hip instantiates them).
template <int N, int P, int NU, int DE, class IN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_rt_dada_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 2, false, 0, 0, IN, OutDada32>(a, blockIdx.y, w, gridDim.x);
}

// The same kernel storing the plain cf32 product and summing its moments
// (pfb_analysis_execute_quantised_to_dada, FUSED; AnalysisArgs::mom): every workgroup of the grid
// writes its slot.  A kernel of its own name again (pfb_ana_stream_quant.hip instantiates them).
template <int N, int P, int NU, int DE, bool LCBF, class IN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_moments_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 0, LCBF, 0, 0, IN, OutCf32, true>(a, blockIdx.y, w, gridDim.x);
}

// The same kernel with the input quantiser at the load (QIN; AnalysisArgs::qin): the plain cf32
// product, and the product with its moments.  Kernels of their own names again
// (pfb_ana_stream_qin.hip instantiates them).
template <int N, int P, int NU, int DE, bool LCBF, class IN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_qin_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 0, LCBF, 0, 0, IN, OutCf32, false, true>(a, blockIdx.y, w, gridDim.x);
}
template <int N, int P, int NU, int DE, bool LCBF, class IN>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void analysis_stream_qin_moments_kernel(AnalysisArgs a) {
  const int w = a.linear ? (int)blockIdx.x : xcd_tile(blockIdx.x, gridDim.x);
  analysis_stream_body<N, P, NU, DE, 0, LCBF, 0, 0, IN, OutCf32, true, true>(a, blockIdx.y, w, gridDim.x);
}

// The one-shot passes beside the streaming kernel (pfb_ana_stream_quant.hip, pfb_ana_stream_qin.hip):
// their workgroup size, and the 16-byte loads a thread of a moments pass has in flight
constexpr int kOneShotThreads = 256;
constexpr int kMomLoads = 8;

// the workgroup's three sums in a fixed order (wave shuffles, then the waves' values through
// LDS); the result in thread 0
__device__ __forceinline__ void wg_sum3(double (&m)[3], double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m[0] += __shfl_down(m[0], off, 64);
    m[1] += __shfl_down(m[1], off, 64);
    m[2] += __shfl_down(m[2], off, 64);
  }
  static_assert(kOneShotThreads == 256, "four waves");
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    red[(t >> 6) * 3 + 0] = m[0];
    red[(t >> 6) * 3 + 1] = m[1];
    red[(t >> 6) * 3 + 2] = m[2];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] = (red[j] + red[3 + j]) + (red[6 + j] + red[9 + j]);
  }
}

// Workgroups per polarisation of a streaming launch, each a contiguous range of steps
struct StreamGrid {
  int64_t n_steps, fit_steps, wgs;
  int env_wpc;
};
template <class SH, int NU>
inline hipError_t stream_grid(const AnalysisArgs& a, StreamGrid* g) {
  constexpr int N = NT;
  const int64_t q_lo = a.row0 / NU;
  const int64_t n_steps = ((a.K + NU - 1) / NU - q_lo + SH::QS - 1) / SH::QS;
  // LDS-limited resident workgroups per CU, each a contiguous range of steps
  // two persistent workgroups per CU (one below the LDS-resident count of 3): longer step
  // ranges amortise each workgroup's start-up window load; measured 4 % faster than 3
  // (PFB_ANA_WG_PER_CU overrides, A/B knob)
  int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / SH::lds_bytes));
  static const int env_wpc = knob("PFB_ANA_WG_PER_CU") ? std::atoi(knob("PFB_ANA_WG_PER_CU")) : 0;
  if (env_wpc > 0) per_cu = env_wpc;
  const int64_t per_pol = std::max<int64_t>(1, (per_cu * cu_count()) / a.n_pol);
  int64_t wgs = std::min<int64_t>(n_steps, per_pol);
  // a workgroup's rows (its steps' NEW rows each + the WIN-row window) must fit one
  // buffer descriptor: huge single series get more, shorter ranges
  // (bytes from one sample of a series to its next: 8, or a DADA section's n_pol x 2 x NBIT / 8)
  const int64_t sstep = a.din ? (int64_t)a.n_pol * (a.din_nbit / 4) : 8;
  const int64_t fit_steps = (kRsrcMaxBytes / (sstep * N) - SH::WIN) / SH::NEW;
  if (fit_steps <= 0) return hipErrorInvalidValue;
  wgs = std::max(wgs, (n_steps + fit_steps - 1) / fit_steps);
  *g = StreamGrid{n_steps, fit_steps, wgs, env_wpc};
  return hipSuccess;
}

}  // namespace pfb
