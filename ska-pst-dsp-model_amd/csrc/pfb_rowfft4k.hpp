// pfb_rowfft4k.hpp — the 4096-point row FFT's passes, tables and LDS budget, shared by the
// 4096-point kernels of pfb_rowfft.hip and the one that stores a DADA section
// (pfb_rowfft_dadaout.hip): one definition, so every kernel computes the same values.
#pragma once
#include "pfb_common.hpp"

namespace pfb {

// ----------------------------------------------------------------- 4096-point row FFT
// The SKA-Mid row FFT (the analysis FFT of polyphase_analysis_padded.m:147 for C3, and the
// synthesis stage 1 of 4096-channel rows) as three explicit radix-16 Stockham passes per
// row, persistent over a contiguous row range (XCD-aware), next row prefetched into
// registers.  Round 5: the twiddles come from per-pass power tables instead of strided
// reads of one 4096-entry table — pass 3 read table entries r k at lane stride r = 2, 4, 8
// (2-, 4- and 8-way LDS bank conflicts, 24 % of the kernel's LDS cycles) — each lane now
// reads w^{2^p}(k) from T3[p][k], contiguous in k (conflict-free).  The entries are the
// same table values (e^{-2 pi i m / 4096}, rounded once from double on the host) and the
// other powers are the same products, so the output is bit-identical to the generic
// passes.  The tables take 8.7 KB instead of 32 KB of LDS: 3 workgroups per CU.
// The row takes two layouts instead of the 1-in-16 pad (whose pass-2 / pass-3 loads wrapped
// one lane of every 32-lane ds_read_b64 group onto bank 0: 2-way, 22 % of the LDS cycles,
// r05_v4 PMC): pass 1 -> pass 2, element 16 j + r at slot kR4kA r + j (rows of kR4kA slots: the
// 16-lane store groups and the load groups, kR4kA (tid mod 16) + tid / 16, on distinct
// banks); pass 2 -> pass 3 unpadded (element e at slot e).  Every access is one lane base
// plus an immediate offset.
// (257: the pass-2 loads compile to ds_read2_b64 — 16-lane groups on 32 banks — whose
// 16 lanes k2 then sit at dword 2 (257 k2 + j) = 2 k2 + 2 j mod 32, all distinct; 258 gave
// 4 k2 mod 32, 2-way, the 18 % of LDS cycles PMC kept counting)
constexpr int kR4kA = 257;         // layout-A row of 16 j + r: slot kR4kA r + j
constexpr int kR4kRow = 15 * kR4kA + 256 + 2;  // slots of the row buffer (layout A; B needs 4096)
constexpr int kR4kTw2 = 4 * 16;    // T2[p][k] = tw[(2^p 16 k) mod N], k < 16
constexpr int kR4kTw3 = 4 * 256;   // T3[p][k] = tw[2^p k], k < 256
constexpr size_t kR4kLds = ((size_t)kR4kRow + kR4kTw2 + kR4kTw3) * sizeof(float2);

template <int DIR>
__device__ __forceinline__ void r4k_twiddles(const float2* t, int k, int stride, float2 (&w)[16]) {
  static_for<0, 4>([&](auto pv) {
    constexpr int p = decltype(pv)::value;
    float2 v = t[p * stride + k];
    if constexpr (DIR > 0) v.y = -v.y;
    w[1 << p] = v;
  });
  static_for<1, 16>([&](auto rv) {
    constexpr int r = decltype(rv)::value;
    constexpr int h = high_bit(r);
    if constexpr (h != r) w[r] = cmul(w[h], w[r - h]);
  });
}

// One row held as v[r] = element tid + 256 r (pass-1 input order): the three radix-16 passes
// through the LDS row; on return v[r] = output element tid + 256 r.  Opens with the barrier
// that orders it after the previous row's pass 3 (and the tables' staging).
template <int DIR>
__device__ __forceinline__ void r4k_fft(float2 (&v)[16], float2* row, const float2* t2, const float2* t3, int tid) {
  const int k2 = tid & 15;
  const int st2 = (tid >> 4) * 256 + k2;     // pass-2 output base (j / 16) 256 + k
  __syncthreads();  // tables staged / the previous row's pass 3 is done with the LDS row
  // pass 1 (NS 1): no twiddles, outputs tid 16 + r
  sdft<16, DIR>(v);
#pragma unroll
  for (int r = 0; r < 16; ++r) row[kR4kA * r + tid] = v[r];  // layout A
  __syncthreads();
  // pass 2 (NS 16): k = tid mod 16, twiddles w^r, r = 1..15, of m = 16 k
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = row[kR4kA * k2 + (tid >> 4) + 16 * r];  // element tid + 256 r
  {
    float2 w[16];
    r4k_twiddles<DIR>(t2, k2, 16, w);
    static_for<1, 16>([&](auto r) { v[r] = cmul(v[r], w[r]); });
  }
  sdft<16, DIR>(v);
  __syncthreads();  // every pass-2 load done before the in-place stores
#pragma unroll
  for (int r = 0; r < 16; ++r) row[st2 + 16 * r] = v[r];  // layout B
  __syncthreads();
  // pass 3 (NS 256): k = tid, twiddles of m = k; outputs tid + 256 r
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = row[tid + 256 * r];
  {
    float2 w[16];
    r4k_twiddles<DIR>(t3, tid, 256, w);
    static_for<1, 16>([&](auto r) { v[r] = cmul(v[r], w[r]); });
  }
  sdft<16, DIR>(v);
}

// The pair kernel storing its product as a DADA section (pfb_rowfft_dadaout.hip;
// RowFftArgs::dout, dout_nbit 8 / 16 / 32): launch_row_fft_t<4096> takes it when dout is set
template <int DIR>
hipError_t launch_row_fft4096_dadaout(const RowFftArgs& r, int n_pol, hipStream_t s);

}  // namespace pfb
