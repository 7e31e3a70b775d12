// pfb_kernels.hpp — internal (C++) launcher interface between the C ABI and the
// HIP kernels.  Not part of the public boundary (see include/pfb_api.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

namespace pfb {

// Release builds carry no tuning or timing switches: the A/B knobs (PFB_* environment
// variables read through knob()) and the timing masks that drop a kernel's loads or
// stores exist only in the experiments build (make EXPERIMENTS=1 ->
// lib/libpfb_hip_exp.so, compiled with -DPFB_EXPERIMENTS).  In a release build knob()
// returns null and tmask() 0 at compile time, so no environment variable reaches a
// code path that skips work.
#ifdef PFB_EXPERIMENTS
constexpr bool kExperiments = true;
#else
constexpr bool kExperiments = false;
#endif
inline const char* knob(const char* name) { return kExperiments ? std::getenv(name) : nullptr; }
__host__ __device__ constexpr int tmask(int m) { return kExperiments ? m : 0; }

enum Variant { kBunton = 0, kPadded = 1, kLowCbf = 2 };

// Largest byte extent one raw buffer descriptor may cover: the kernels form 32-bit
// signed byte offsets from it.  Launchers size their per-workgroup ranges (and plans
// reject shapes) so that no descriptor needs more; nothing is clamped silently.
constexpr int64_t kRsrcMaxBytes = 0x7ffffff0;

// Polyphase analysis (polyphase_analysis.m / polyphase_analysis_padded.m).
struct AnalysisArgs {
  const float2* in;        // [pol][t]
  int64_t in_pol_stride;
  int64_t n_dat;
  float2* out;             // [pol][k][c]
  int64_t out_pol_stride;
  int64_t row0;            // first output row of this launch (global row index)
  int64_t K;               // end of this launch's rows (exclusive, global)
  int64_t K_total;         // output rows per pol of the whole call (padded circular shift)
  int n_pol;
  int N, M, P, nu, sds;    // channels, step, phases, os numerator, padded delay shift
  int variant;
  const float* taps;       // P*N padded taps (device)
  const float2* twN;       // e^{-2 pi i m / N}, m < N (device)
  float2* scratch;         // generic path: [pol][K - row0][N] (device) or null
  int timing_mask;         // timing experiments only (PFB_ANA_MASK, results invalid): bit0 no
                           // input loads, bit1 no channelised stores, bit2 no Z stores
                           // (streaming kernel)
  // Round trip only (pfb_roundtrip_execute): when z is set, every output row k >= z_row0
  // is also transformed by the synthesis stage-1 channel IFFT (the exact computation
  // row_fft_kernel<N, +1> performs on the stored row) into z[pol][k - z_row0][t0].
  float2* z;
  int64_t z_pol_stride;
  int64_t z_row0;
  // generic path (N > 256) with z: the FIR writes only the Z rows (all K of them,
  // z_row0 = 0) and the row FFT makes the channelised rows from them through this
  // index reversal (padded variant; null for Bunton) — see fir_window_kernel
  const int* zrev;
  // leading zeros in front of `in` (the LowCBF wrapper's one-time pre-padding) — the
  // streaming kernel reads x[r N + c - pad] (zero for negative indices); 0 otherwise
  int64_t pad;
  // with pad > 0: the pad samples in front of `in` are pre[pol][0, pad) (a stream object's
  // carried samples; null: zeros, the LowCBF pre-padding).  Streaming kernel only, read by the
  // first window of every workgroup whose window starts before `in` (launch_stream rejects
  // pad > WIN N)
  const float2* pre;
  int64_t pre_pol_stride;
  float lcbf_scale;  // LowCBF streaming path: output scale (2^12)
  // Strided channelised output (out_rs > 0): bin c of row k goes to
  // out[pol][k * out_rs + j * out_cs] with j = c (sel_n = 0) or the two-stage chomp
  // j = c < sel_split ? c : c - sel_shift, kept when c < sel_split or c >= sel_split +
  // sel_shift, and j < sel_n (TwoStageFilterBank.m:102-105); out_rs = 0: [pol][k][c].
  // Taken by the streaming kernel (Bunton, N = 256; rows [row0, K) through per-step
  // descriptors, StridedRowStore) and by every padded plan: the fused kernel
  // (AnalysisStridedStore) and the generic path's row FFTs (RowStridedStore, the 4096-point
  // pair kernel's OST mode).  Padded: k is the row after the circular -sds shift, the launch
  // covers all K_total rows (row0 = 0, K = K_total), and only shifted rows k < out_keep are
  // stored — guarded plain stores, no scratch rows in `out`
  int out_rs, out_cs;
  int sel_split, sel_shift, sel_n;
  // z in a grouped layout (streaming kernel, round trip into synth_wave_kernel): zblk = ZB
  // in {2, 4, 16} puts row k - z_row0 = ZB g + gi of column c at z[pol][g][c][gi] — ZB
  // consecutive rows of one column are one run; needs (row0 - z_row0) % 16 == 0
  // (launch_analysis checks); 0 or 1: rows [row][c]
  int zblk;
  // generic path (N > 256) with z: 0 both launches; 1 only the FIR (Z rows); 2 only the
  // row FFT (channelised rows from Z) — so the row FFT can run beside the synthesis, which
  // reads the same Z rows
  int z_stage;
  // stream objects (streaming kernel only): also copy in[pol][carry_src, carry_src + carry_n)
  // — the next call's carry, FilterBank.m:119-126 — to carry_out[pol][0, carry_n) (a buffer
  // other than `pre`), spread over the grid before the main loop: no separate copy launch
  float2* carry_out;
  int64_t carry_src, carry_n, carry_pol_stride;
  // workgroup -> step range order: 0 XCD-aware (xcd_tile), 1 linear (blockIdx.x: the
  // dispatcher's order is the rows' order, so the chip's loads in flight stay in one window)
  int linear = 0;
  // padded plans with out_rs > 0: the rows kept of the K_total computed (the stream object's
  // nu-trimmed T_out, FilterBank.m:93-104); shifted rows [out_keep, K_total) are not stored
  int64_t out_keep = 0;
  // The input is a single-channel DADA section read in place instead of `in`
  // (pfb_analysis_execute_dada; analysis_reads_dada): TFP order, NDIM 2, din_nbit 8 / 16
  // (integers) or 32 (float), sample t of polarisation p at byte (t n_pol + p) din_nbit / 4 of
  // din, which is aligned to one complex sample.  n_dat, pad, pre and carry_src count samples
  // as ever; `in` and in_pol_stride are unused.
  const void* din = nullptr;
  int din_nbit = 0;
  // The product goes out as a DADA data section instead of `out`
  // (pfb_analysis_execute_to_dada; analysis_writes_dada): TFP order, NDIM 2, dout_nbit 8 / 16
  // (integers) or 32 (float); element (row k, channel c, pol p) at byte
  // ((k C + c) n_pol + p) dout_nbit / 4 of dout, C = N (216 for the LowCBF instantiation), its
  // value to_sample(dout_scale * x) per component of the x the cf32 kernel stores.  dout is
  // aligned to one complex sample; `out` and out_pol_stride are unused.  A DADA input (din)
  // has the same NBIT, or dout_nbit is 32 (dadaout_reads_dada) — the streaming kernel's rule;
  // on the generic path (N = 4096) the FIR reads din and the row FFT stores dout, any pair of
  // NBITs, and only the output rows below out_keep are made.
  void* dout = nullptr;
  int dout_nbit = 0;
  float dout_scale = 1.f;
  // The moments of the product (analysis_stream_moments_kernel, launch_stream_moments): workgroup
  // w of polarisation p of a grid of nw per polarisation stores (sum re, sum im, sum re^2 + im^2)
  // of the values it stored, in double, at mom[(p nw + w) 3 ...]
  double* mom = nullptr;
  // The input quantiser at the load (analysis_stream_qin_kernel, launch_stream_qin): every new
  // sample enters the FIR as roundf(sf * x) per component, sf = (float)qin[3] of the plan's
  // block {sum re, sum im, s2, scale} (launch_moments_finish), 1 when null.  Read only by the
  // QIN instantiations.
  const double* qin = nullptr;
};
// the plan's kernel has a loader for such a section (the streaming kernel; the LDS-shared FIR
// of the N > 256 path, launches without stage-1 rows)
bool analysis_reads_dada(const AnalysisArgs& a, int nbit);
// the plan's kernel has a DADA store: the streaming kernel, or — N = 4096, the plain product
// of one launch over all the call's rows (row0 0; padded: K = K_total) — the generic path's
// row FFT (row_fft4096_pair_dadaout_kernel, which makes the output rows below a.out_keep)
bool analysis_writes_dada(const AnalysisArgs& a, int nbit);
// the streaming kernel with the DADA store (pfb_ana_stream_dadaout.hip); lcbf: the LowCBF
// instantiation (launch_lowcbf_stream's shape)
hipError_t launch_stream_dadaout(const AnalysisArgs& a, bool lcbf, hipStream_t s);
// those kernels read a DADA section of in_nbit in place when they write out_nbit (the same
// NBIT, or any integer NBIT into NBIT 32); other pairs come in unpacked, as cf32
bool dadaout_reads_dada(int in_nbit, int out_nbit);
// The quantised output (pfb_ana_stream_quant.hip; pfb_analysis_execute_quantised_to_dada).
// The streaming kernel storing its cf32 product and the product's moments (AnalysisArgs::mom);
// lcbf: the LowCBF instantiation.  stream_moments_slots: the n_pol x nw slots of three doubles
// the launch of `a` writes (-1: no such kernel), for the caller to size `mom` and to finish.
int64_t stream_moments_slots(const AnalysisArgs& a, bool lcbf);
hipError_t launch_stream_moments(const AnalysisArgs& a, bool lcbf, hipStream_t s);
// The same slots from a stored product x[pol][0, n) (pol stride ps, both even; 16-B aligned): one
// slot per workgroup of a one-shot grid.  moments_partials_slots: their number.
int64_t moments_partials_slots(int64_t n, int n_pol);
hipError_t launch_moments_partials(const float2* x, int64_t ps, int64_t n, int n_pol, double* mom, hipStream_t s);
// stats = {sum re, sum im, sum re^2 + im^2, scale}: the slots added in index order by one
// workgroup, scale = rms / sqrt(var), var = (s2 - (sum re^2 + sum im^2) / cnt) / (cnt - 1)
hipError_t launch_moments_finish(const double* mom, int64_t slots, double cnt, double rms, double* stats,
                                 hipStream_t s);
// x[pol][0, n) -> the TFP section `out` of n x n_pol complex samples of nbit 8 / 16 / 32 / 64:
// each component to_sample(out_scale * roundf(sf * x)), sf = (float)stats[3] or 1 (stats null)
hipError_t launch_quantise_pack(const float2* x, int64_t ps, int64_t n, int n_pol, const double* stats,
                                float out_scale, void* out, int nbit, hipStream_t s);
// The quantised input (pfb_ana_stream_qin.hip; pfb_analysis_set_input_quantiser).
// The new samples of a call, read where they lie: cf32 rows x[pol][0, n) (pol stride ps), or a
// single-channel TFP section (NDIM 2, nbit 8 / 16 / 32, aligned to one complex sample; nbit 0:
// cf32) of n samples x n_pol polarisations from its sample 0.
struct QinSrc {
  const void* base;
  int nbit;      // 0: cf32 rows
  int64_t ps;    // cf32: pol stride in samples
  int64_t n;     // samples per polarisation
  int n_pol;
};
// Their moments in the slot layout launch_moments_finish adds: one slot of three doubles per
// workgroup of a one-shot grid, ordinary stores, 16-byte loads of the aligned middle of each
// row (a section is one row of n n_pol samples) and single samples at its ragged ends; no byte
// outside the rows is read.  input_moments_slots: their number (0: no samples).
int64_t input_moments_slots(const QinSrc& q);
hipError_t launch_input_moments(const QinSrc& q, double* mom, hipStream_t s);
// dst[pol][0, n) (pol stride dps, packed cf32) = roundf(sf * x) per component, sf = (float)stats[3]
// or 1 (stats null): the quantising copy of the STAGED side and of the carry tail; dst may be
// the cf32 source itself (element for element)
hipError_t launch_quantise_copy(const QinSrc& q, const double* stats, float2* dst, int64_t dps, hipStream_t s);
// The streaming kernel rounding at the load (AnalysisArgs::qin; the plain cf32 product, or with
// a.mom the product's moments as launch_stream_moments); lcbf: the LowCBF instantiation
hipError_t launch_stream_qin(const AnalysisArgs& a, bool lcbf, hipStream_t s);
// The file-to-file round trip's analysis launch (pfb_ana_stream_rtdada.hip): the streaming
// kernel reading the section `din` (in_nbit 8 / 16 / 32) in place, storing the product as the
// NBIT 32 float section `dout` (dout_scale 1) and the stage-1 rows z in 2-row runs (zblk 2) —
// the one launch that takes din or dout together with z.  Bunton, N 256, os 8/7 or 4/3, 12 or 13
// phases; no carry, no read offset.
bool stream_rt_dada_supported(const AnalysisArgs& a, int in_nbit);
hipError_t launch_stream_rt_dada(const AnalysisArgs& a, hipStream_t s);
// pfb_dada_pack with both components multiplied by `scale` in float32 first (pfb_layout.hip)
hipError_t launch_dada_pack_scaled(const float2* in, int64_t in_pol_stride, int64_t n_dat, int C, int P,
                                   void* out, int nbit, float scale, hipStream_t s);
// SKA-Low CBF PST filterbank through the streaming analysis kernel (pfb_analysis.hip)
hipError_t launch_lowcbf_stream(const AnalysisArgs& a, hipStream_t s);
// analysis kernels that can also emit the synthesis stage-1 rows (see AnalysisArgs::z)
bool analysis_can_emit_z(const AnalysisArgs& a);
// analysis kernels that can emit the stage-1 rows in the blocked layout (AnalysisArgs::zblk)
bool analysis_can_emit_zblk(const AnalysisArgs& a);
// analysis shapes whose kernel reads with an input offset (AnalysisArgs::pad)
bool analysis_takes_offset(const AnalysisArgs& a);
// the fused kernel reads a stream carry through `pre` with `pad` (non-streaming shapes)
bool analysis_fused_takes_carry(const AnalysisArgs& a);

// Complex-sample index of element (t, c, p) of a DADA data section of C channels and P
// polarisations (NDIM 2): TFP order (reshape_dada_data.m:23-30) or the LowCBF heaps of 32
// samples, [heap][chan][pol][sample] (reshape_low_cbf_data.m:31-41).  Shared by the unpack
// kernels (pfb_layout.hip) and the channel IFFT's DADA row loader (pfb_common.hpp).
template <bool LOWCBF>
__host__ __device__ __forceinline__ int64_t dada_index(int64_t t, int c, int p, int C, int P) {
  if constexpr (LOWCBF) return (((t >> 5) * C + c) * P + p) * 32 + (t & 31);
  else return (t * C + c) * P + p;
}

// A DADA data section the channel IFFT reads in place (NBIT 8 / 16, NDIM 2; n_dat rows of the
// plan's channels x polarisations): the launch's row 0 is file row t0.
struct DadaIn {
  const void* base;
  int nbit, lowcbf;
  int64_t n_dat, t0;
};
// Rows [t0, t0 + n_rows) of such a section -> out[pol][row][chan] complex float32 (the
// pfb_dada_unpack kernels from a row offset: a LowCBF offset need not be a heap boundary)
hipError_t launch_dada_unpack_rows(const DadaIn& d, int64_t n_rows, int C, int P, float2* out,
                                   int64_t out_pol_stride, hipStream_t s);

// Channelised rows that lie strided in device memory (pfb_synthesis_execute_strided): element
// (pol p, row t, channel c) at base[p * ps + t * rs + c * cs], n_dat rows; the launch's row 0
// is row t0.  Only read; polarisations may interleave inside a row (ps < rs) or overlap.
struct StridedIn {
  const float2* base;
  int64_t ps, rs, cs;
  int64_t n_dat, t0;
};
// Rows [t0, t0 + n_rows) of such a layout -> out[pol][row][chan] packed (the strided-rows copy
// kernel, pfb_layout.hip: the stitched head and the carry of a stream call, and the whole
// input of a plan whose channel IFFT has no strided loader)
hipError_t launch_strided_rows_copy(const StridedIn& d, int64_t n_rows, int C, int P, float2* out,
                                    int64_t out_pol_stride, hipStream_t s);

// Synthesis stage 1: per channelised time row, N-point inverse DFT across channels
// (after the combine permutation and per-channel gain).  See DESIGN.md §synthesis.
struct ChanIfftArgs {
  const float2* in;        // [pol][row][c], rows already offset to the first row
  int64_t in_pol_stride;
  float2* out;             // Z: [pol][row][t0]
  int64_t out_pol_stride;
  int64_t n_rows;
  int n_pol;
  int N;
  const int* perm;         // slot -> input channel (null = identity)
  const float* cgain;      // per-slot gain (null = 1)
  const float2* twN;
  int zblk = 1;            // Z rows in runs of zblk (1, 2, 4) per t0 (SynthBlockArgs::zblk)
  // the rows come from a DADA section instead of `in` (chan_ifft_dada_supported; no perm / gain)
  const DadaIn* dada = nullptr;
  // the rows come through a strided layout instead of `in` (chan_ifft_strided_supported; perm
  // allowed, no gain)
  const StridedIn* strided = nullptr;
};
// the channel IFFT has a loader for DADA sections of this sample size (row_fft_dada_kernel)
bool chan_ifft_dada_supported(int N, int nbit);
// the channel IFFT has a strided row loader for this size (row_fft_strided_kernel)
bool chan_ifft_strided_supported(int N);

// Synthesis stage 2: per block and group of t0, Nf-point FFT over time, kept-bin
// selection with deripple gain and four-step twiddle, W-point inverse FFT,
// overlap-discard and the 1/L * de/nu scale.
struct SynthBlockArgs {
  const float2* Z;         // [pol][row][t0] (chunk-local rows)
  int64_t z_pol_stride;
  float2* out;             // [pol][t]
  int64_t out_pol_stride;
  int64_t block0;          // global index of the chunk's first block
  int n_blocks;            // blocks in this chunk
  int n_pol;
  int N, Nf, W, keep, L, Lov, Lkeep, t1_lo, t1_hi;
  float scale;
  const float* window;     // Nf temporal window (device)
  int win_flat;            // 1: window[t] == 1 exactly for t in [48, 208) at Nf 256 / [128, 384) at
                           // Nf 512 (the wave kernels skip those taper multiplies)
  int spans;               // 1: spans Nyquist (signed-frequency bins), 0: critical
  const float2* tw4;       // [j'][t0] = gain[j'] e^{+2 pi i t0 expo[j'] / L} (W x N)
  const float2* twNf;      // e^{-2 pi i m / Nf}
  const float2* twW;       // e^{-2 pi i m / W}
  const float2* tw4s;      // tw4 x (de/nu) / L, rounded once (synth_wave_kernel)
  int64_t out_limit;       // samples per pol actually written (InverseFilterBank trim)
  int ranges;              // 0: one workgroup per block; -1 persistent auto; >0 persistent ranges
  int no_reuse;            // 1: re-read the 2 Ov overlap rows from HBM (PFB_SYNTH_NO_REUSE, A/B only)
  int xcd;                 // 1: XCD-aware workgroup -> (phase group, range) order (PFB_SYNTH_XCD)
  int timing_mask;         // experiments build only (PFB_TIMING_MASK, results invalid): bit0
                           // drop Z loads, bit1 drop output stores, bit2 drop tw4 loads; wave
                           // kernels: bit3 wave barriers for the block loop's workgroup
                           // barriers, bit4 a uniform twiddle for the LDS twiddle tables
  int zblk;                // Z layout of AnalysisArgs::zblk (0/1 rows, else ZB-row runs)
  // Recomputed stage-1 rows (the Nf = 256 round trip, synth_wave_kernel with fir_x set): the
  // analysis writes no Z; the synthesis evaluates each row it needs as N^2 x the streaming
  // analysis's FIR sums of the input series itself (same taps, same FMA order: bit-identical
  // rows).  fir_g[(s N + c) 16 + m] = N^2 x the folded tap of residue s, lag m < PE, column c
  // (pfb_ana_stream.hpp); Z row j is analysis row NU fir_q0 + j.
  const float2* fir_x;     // [pol][t] input series (null: read Z)
  int64_t fir_x_pol_stride;
  int64_t fir_n_dat;
  const float* fir_g;
  int64_t fir_q0;
  int fir_nu, fir_de, fir_pe;
  // The output goes out as a single-channel DADA data section instead of `out`
  // (pfb_synthesis_execute_to_dada; synth_wave_dadaout_supported): TFP order, NDIM 2,
  // dout_nbit 8 / 16 (integers) or 32 (float); sample t of polarisation p at byte
  // (t n_pol + p) dout_nbit / 4 of dout, its value to_sample(dout_scale * y) per component of
  // the y the cf32 kernel stores.  dout is aligned to one complex sample and is the section of
  // the whole call (block0 counts from its sample 0); `out` and out_pol_stride are unused.
  // (Placed so that `linear` stays the struct's last word: the wave kernels fetch it together
  // with the launch's grid size, which follows the struct in the kernel arguments.)
  int dout_nbit = 0;
  void* dout = nullptr;
  float dout_scale = 1.f;
  // wave kernels: workgroup -> (block range, phase group) order, 0 XCD-aware (xcd_tile), 1
  // linear (blockIdx.x: consecutive workgroups are the phase groups of one block range)
  int linear = 0;
};

// Synthesis with a non-identity spectral taper (pfb_spectral.hip): blocks [b0, b0 + nb)
// of the call, every polarisation, through two scratch buffers of nb N max(Nf, W) values.
struct SpectralArgs {
  const float2* in;        // [pol][row][c] channelised rows of the call (sample offset applied)
  int64_t in_pol_stride;
  float2* out;             // [pol][t]
  int64_t out_pol_stride;
  int64_t out_limit;
  int64_t b0, nb;
  int n_pol;
  int N, Nf, W, keep, L, Lov, Lkeep, t1_lo, t1_hi, spans;
  float scale;             // (de/nu) / L
  const float* window;     // Nf temporal window
  const float* cgain;      // per input channel gain (temporal 'hann' quirk) or null
  const int* perm;         // combine permutation (slot -> input channel) or null
  const float* gainj;      // W deripple gains in Matlab's FN row order
  const float* taper;      // L spectral taper coefficients
  const float2* twNf;      // e^{-2 pi i m / Nf}
  const float2* twN;       // e^{-2 pi i m / N}
  const float2* twW;       // e^{-2 pi i m / W}
  float2* buf0;
  float2* buf1;
};
bool spectral_synth_supported(int Nf, int W, int N);
hipError_t launch_spectral_synth(const SpectralArgs& a, hipStream_t s);

// SKA-Low CBF PST filterbank (polyphase_analysis_lowcbf.m / PSTFilterbank.m):
// 256 arms x 12 taps, step 192, forward FFT, fftshift, pi/2 derotation, 216 channels.
struct LowCbfArgs {
  const float2* in;        // [pol][t]
  int64_t in_pol_stride;
  int64_t n_dat;
  int64_t pad;             // leading zeros (1536 on the first call, else 0)
  float2* out;             // [pol][k][216]
  int64_t out_pol_stride;
  int64_t K;
  int n_pol;
  const float* taps;       // 3072 taps (device)
  const float2* tw;        // e^{-2 pi i m / 256}
  float scale;             // 2^28 / 2^9 / 128 = 2^12
  // a stream object's carried samples in front of `in` (AnalysisArgs::pre, with pad = their
  // count; a DADA stream call — the cf32 one concatenates)
  const float2* pre = nullptr;
  // the input is a DADA section read in place (AnalysisArgs::din; streaming path only)
  const void* din = nullptr;
  int din_nbit = 0;
  // the product goes out as a DADA section (AnalysisArgs::dout; streaming path only)
  void* dout = nullptr;
  int dout_nbit = 0;
  float dout_scale = 1.f;
};
hipError_t launch_lowcbf(const LowCbfArgs& a, hipStream_t s);

// Kernel timing (pfb_profile_*): when the C-ABI profiler arms these events, the next
// single-kernel launch records them in its own dispatch (hipExtLaunchKernelGGL), so the
// measured interval is the kernel alone, as a kernel trace sees it.
struct LaunchEvents {
  hipEvent_t start = nullptr, stop = nullptr;
};
LaunchEvents& armed_launch_events();
// name of the last kernel launched through armed events (pfb_profile_kernel_name)
const char*& launched_kernel_name();

// device-to-device strided copy of n_pol rows (pfb_layout.hip)
hipError_t launch_copy_rows(float2* dst, int64_t dps, const float2* src, int64_t sps, int64_t n, int n_pol,
                            hipStream_t s);

bool analysis_supported(int N, int P, int variant, bool* fused);
hipError_t launch_analysis(const AnalysisArgs& a, hipStream_t s);
bool chan_ifft_supported(int N);
hipError_t launch_chan_ifft(const ChanIfftArgs& a, hipStream_t s);
bool synth_block_supported(int Nf, int W);
// Nf = 256 synthesis with one output phase per 16 lanes and no barrier in the block loop
// (pfb_synth_wave.hip); launch_synth_block takes it where it applies
bool synth_wave_supported(const SynthBlockArgs& a);
// the same kernel with recomputed stage-1 rows (SynthBlockArgs::fir_x)
bool synth_wave_fir_supported(const SynthBlockArgs& a);
hipError_t launch_synth_wave(const SynthBlockArgs& a, hipStream_t s);
// the same kernel (stored stage-1 rows, kept-register stores) writing a DADA section of `nbit`
// (SynthBlockArgs::dout; pfb_synth_wave_dadaout.hip); launch_synth_block takes it when dout is set
bool synth_wave_dadaout_supported(const SynthBlockArgs& a, int nbit);
hipError_t launch_synth_wave_dadaout(const SynthBlockArgs& a, hipStream_t s);
// Nf = 512, W = 448, keep 256 (SKA-Mid): one output phase per 32 lanes (pfb_synth_wave512.hip)
bool synth_wave512_supported(const SynthBlockArgs& a);
hipError_t launch_synth_wave512(const SynthBlockArgs& a, hipStream_t s);
hipError_t launch_synth_block(const SynthBlockArgs& a, hipStream_t s);

}  // namespace pfb
