// pfb_host.hpp — what the host-side units of the C ABI (pfb_api_*.hip, pfb_layout.hip) share:
// the error channel, device buffers, the profiler, the two plan types, the small request and
// view structs that cross a unit, and the few functions the round trip takes from the analysis
// and the synthesis unit.  Host code only; not part of the public boundary (include/pfb_api.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pfb_api.h"
#include "pfb_kernels.hpp"

// fail() with a ready-made message, for units that build theirs (pfb_layout.hip)
pfb_status pfb_set_error(pfb_status s, const char* msg);

namespace pfb::host {

// ------------------------------------------------------------------ error channel
// sets the calling thread's pfb_last_error text and returns `s`
pfb_status fail(pfb_status s, const char* fmt, ...);

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return pfb::host::fail(e_ == hipErrorOutOfMemory ? PFB_ERR_OOM : PFB_ERR_HIP,   \
                             "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ------------------------------------------------------------------ device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t ensure(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n, 256));
    if (e == hipSuccess) bytes = std::max<size_t>(n, 256);
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& v) {
  hipError_t e = b.ensure(v.size() * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// e^{sign 2 pi i m / n}, accurate reduction in double
std::vector<float2> twiddles(int64_t n, int sign);

inline int64_t floordiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// n_pol rows of n complex samples at (dst + q*dps) <- (src + q*sps): one 2-D copy, not
// n_pol calls (the two-stage cascades run thousands of series through one plan)
hipError_t copy_pols(float2* dst, int64_t dps, const float2* src, int64_t sps, int64_t n, int n_pol,
                     hipMemcpyKind kind, hipStream_t s);

// ------------------------------------------------------------------ profiling
struct ProfRec {
  int which;
  hipEvent_t a, b;
  double bytes;
};
struct Profiler {
  bool enabled = false;
  std::vector<ProfRec> pending;
  std::vector<hipEvent_t> pool;
  // 0 analysis, 1 chan IFFT, 2 block, 3 analysis + chan IFFT, 4 / 5 the FIR / row FFT of
  // the generic (N > 256) round trip (launched one by one so each is timed alone)
  static constexpr int kClasses = 6;
  double total_ms[kClasses] = {};
  int64_t launches[kClasses] = {};
  double bytes[kClasses] = {};
  std::string names[kClasses];  // kernel of each class's last single-kernel launch (demangled)
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  void drain();
};
Profiler& profiler();  // the one instance (pfb_profile_*)
std::string demangle(const char* name);

// Times the launch(es) issued while in scope.  single = true: exactly one kernel launch
// goes through pfb::launch_kernel, which records the two events inside its own dispatch
// (hipExtLaunchKernelGGL) — the kernel's own duration, as a kernel trace measures it.
// single = false (multi-kernel paths): events recorded on the stream around the scope.
struct ProfScope {
  Profiler& prof = profiler();
  hipEvent_t a = nullptr, b = nullptr;
  int which;
  double bytes;
  hipStream_t s;
  bool single;
  ProfScope(int w, double by, hipStream_t st, bool one = true) : which(w), bytes(by), s(st), single(one) {
    if (prof.enabled) {
      a = prof.get();
      b = prof.get();
      if (a && b) {
        if (single) {
          pfb::armed_launch_events() = pfb::LaunchEvents{a, b};
          pfb::launched_kernel_name() = nullptr;
        }
        else (void)hipEventRecord(a, s);
      }
    }
  }
  ~ProfScope() {
    if (prof.enabled && a && b) {
      if (single) {
        pfb::LaunchEvents& ev = pfb::armed_launch_events();
        if (ev.start) {  // not consumed (no kernel launched): drop the record
          ev = pfb::LaunchEvents{};
          prof.pool.push_back(a);
          prof.pool.push_back(b);
          return;
        }
        if (pfb::launched_kernel_name()) prof.names[which] = demangle(pfb::launched_kernel_name());
      } else {
        (void)hipEventRecord(b, s);
      }
      prof.pending.push_back({which, a, b, bytes});
    }
  }
};

// The scalar shape of a synthesis: what the descriptor fixes before any table or buffer
// exists.  The host-side tables (SynthHost) and the plan both derive from it.
struct SynthShape {
  int N = 0, nu = 1, de = 1, Nf = 0, Ov = 0, spans = 1, combine = 1;
  int W = 0, keep = 0, L = 0, Lov = 0, Lkeep = 0, t1_lo = 0, t1_hi = 0;
  bool deripple = false;
  bool identity_perm = true;
  bool win_flat = false;  // SynthBlockArgs::win_flat
};

}  // namespace pfb::host

// ====================================================================== the plans
struct pfb_analysis_plan {
  using DevBuf = pfb::host::DevBuf;
  uint64_t serial = 0;  // unique per plan (the split round trip's key: pointers get reused)
  int device = 0;
  int variant = 0, N = 0, nu = 1, de = 1, M = 0, P = 0, n_pol = 1, sds = 0;
  int C = 0;                  // output channels per row (N; 216 for the LowCBF filterbank)
  bool lowcbf_pad = false;    // LowCBF: the next call pre-pads 1536 zeros (persistent do_padding)
  int64_t n_taps = 0;
  bool fused = false;
  DevBuf taps, twN, scratch;
  // streaming shapes: the folded taps x N^2 [s][c][16] of analysis_stream_kernel, for the
  // synthesis that recomputes the stage-1 rows (SynthBlockArgs::fir_g); empty otherwise
  DevBuf gtab;
  DevBuf zrev;  // padded generic round trip: index reversal (N - i) mod N of the row FFT input
  // streaming (FilterBank.m:13-14 input_buffer / buffered_samples)
  DevBuf carry, work, stage_in, stage_out;
  DevBuf carry_next;  // device streams: the streaming kernel writes the next carry here, then swap
  int64_t buffered = 0;
  int last_dada = PFB_DADA_INPUT_NONE;  // pfb_analysis_last_dada_input
  int last_dada_out = PFB_DADA_OUTPUT_NONE;  // pfb_analysis_last_dada_output
  DevBuf dada_stage;  // STAGED DADA output: the cf32 product before its scaled pack launch
  // the quantised output (pfb_analysis_execute_quantised_to_dada): the cf32 product the pack
  // launch reads, the moments' partial sums (three doubles per slot) and the 32-byte stats block
  // {sum re, sum im, s2, scale} — the plan's own, grown with the call's length
  DevBuf quant_prod, quant_mom, quant_stats;
  int quant_mode = PFB_QUANTISER_MOMENTS_AUTO;  // pfb_analysis_set_quantiser_moments
  int last_quant = PFB_QUANTISER_NONE;          // pfb_analysis_last_quantiser
  // the quantised input (pfb_analysis_set_input_quantiser): the partial sums of the new samples'
  // moments and the 32-byte block of their own (the output quantiser's can be live in the same
  // call), grown with the call's length
  DevBuf qin_mom, qin_stats;
  bool qin_on = false;
  double qin_rms = 0.0;
  int qin_mode = PFB_QUANTISER_MOMENTS_AUTO;    // pfb_analysis_set_input_quantiser_mode
  int last_qin = PFB_INPUT_QUANTISER_NONE;      // pfb_analysis_last_input_quantiser
  bool qin_scale_dev = false;  // the last call's scale is qin_stats[3] (else 1: pfb_analysis_last_input_scale)
  // round trip (pfb_roundtrip_execute): the analysis runs on this stream, ahead of the
  // synthesis on the caller's stream; one event per chunk orders them
  hipStream_t aux = nullptr;
  std::vector<hipEvent_t> events;
};

struct pfb_synthesis_plan : pfb::host::SynthShape {
  using DevBuf = pfb::host::DevBuf;
  int device = 0;
  int n_pol = 1;
  int chunk_blocks = 0;
  int stage1 = PFB_STAGE1_AUTO;  // pfb_synthesis_set_stage1_rows
  int last_stage1 = 0;           // pfb_synthesis_last_stage1_rows: where the last launch got its rows
  int last_dada = PFB_DADA_INPUT_NONE;  // pfb_synthesis_last_dada_input
  int last_strided = PFB_STRIDED_INPUT_NONE;  // pfb_synthesis_last_strided_input
  int last_dada_out = PFB_DADA_OUTPUT_NONE;   // pfb_synthesis_last_dada_output
  int rt_chunk_blocks = 64;  // round-trip pipeline chunk (PFB_RT_CHUNK_BLOCKS)
  int timing_mask = 0;  // PFB_TIMING_MASK (timing experiments; results invalid when set)
  int ranges = -1;  // PFB_SYNTH_RANGES: 0 one workgroup per block, -1 persistent auto, >0 persistent
  int no_reuse = 0;  // PFB_SYNTH_NO_REUSE: re-read the overlap rows (A/B measurement only)
  int xcd = 1;       // PFB_SYNTH_XCD=0: plain workgroup order (A/B measurement only)
  bool has_cgain = false;
  bool has_spectral = false;  // non-identity spectral taper: pfb_spectral.hip path
  DevBuf window, tw4, tw4s, twN, twNf, twW, perm, cgain;
  DevBuf taper, gainj, sbuf0, sbuf1;  // spectral taper (L), deripple gains (W), scratch
  DevBuf Z, carry, work, stage_in, stage_out;
  int64_t buffered = 0;
  int64_t ifb_offset = 0;  // InverseFilterBank.sample_offset (0-based; InverseFilterBank.m:12)
  // split round trip: what the analysis half left in Z (analysis plan, n_dat, sample
  // offset, row layout, rows) — the synthesis half must match it; cleared whenever Z is
  // written by anything else
  uint64_t zkey_plan = 0;
  int64_t zkey[5] = {-1, -1, -1, -1, -1};
  // (recomputed rows: the analysis half left no rows, only the input the synthesis reads)
  const void* zkey_x = nullptr;
  int64_t zkey_xps = -1;
};

namespace pfb::host {

// a cf32-output call that went through: pfb_*_last_dada_output reports NONE again
template <class Plan>
pfb_status cf32_output(Plan* p, pfb_status st) {
  if (p && st == PFB_OK) p->last_dada_out = PFB_DADA_OUTPUT_NONE;
  return st;
}
// (an analysis plan: pfb_analysis_last_quantiser reports NONE as well)
inline pfb_status cf32_output(pfb_analysis_plan* p, pfb_status st) {
  if (p && st == PFB_OK) p->last_dada_out = PFB_DADA_OUTPUT_NONE, p->last_quant = PFB_QUANTISER_NONE;
  return st;
}

// ====================================================================== DADA input sections
// A DADA data section (device memory) as the input of a call: n samples (analysis: x 1 channel;
// synthesis: rows x the plan's n_chan) x the plan's n_pol x ndim values of nbit
struct DadaSection {
  const void* base;
  int nbit, ndim, order;
  // analysis only: unpack it even where the kernel could read it in place (a _dada_to_dada call
  // whose NBIT pair the DADA-store kernels do not read in place: pfb::dadaout_reads_dada)
  bool force_staged = false;
};

// the checks every call makes of such a section (`plan`: only that there is one)
pfb_status section_check(const void* plan, const DadaSection& sec, int64_t n);

// ====================================================================== analysis launches
// Strided channelised output (AnalysisArgs::out_rs): pfb_filterbank_execute_strided.
// keep: the rows the call returns (T_out; a padded plan computes K >= T_out rows and stores
// only the shifted rows below it, AnalysisArgs::out_keep)
struct OutLayout {
  int64_t rs, cs;
  int32_t split, shift, nsel;
  int64_t keep;
};

// the next call's carry copied by the streaming kernel itself (AnalysisArgs::carry_out)
struct CarryOut {
  float2* dst;
  int64_t src, n, dst_ps;
};

// A single-channel DADA section (TFP, NDIM 2, NBIT 8 / 16 / 32, aligned to a complex sample)
// the analysis kernel reads in place instead of `in` (pfb_analysis_execute_dada, FUSED)
struct AnaDada {
  const void* base;
  int nbit;
};

// A DADA data section (TFP, NDIM 2, NBIT 8 / 16 / 32, aligned to a complex sample) the analysis
// kernel writes instead of `out`, each component to_sample(scale * x)
// (pfb_analysis_execute_to_dada, FUSED)
struct AnaOut {
  void* base;
  int nbit;
  float scale;
};

// The launch also sums the moments of the product it stores (the streaming kernel's moments
// instantiation, FUSED quantised output): analysis_run sizes the plan's quant_mom for the
// launch's grid and reports the slots it wrote (0: nothing launched)
struct AnaMoments {
  int64_t slots = 0;
};

// The launch replaces every new sample x by roundf(sf * x) as it loads it, sf = (float)stats[3]
// of the plan's input-quantiser block, 1 when stats is null (AnalysisArgs::qin)
struct AnaQin {
  const double* stats = nullptr;
};

// One analysis launch (analysis_run); a call site sets the members it uses.
struct AnaLaunch {
  // input: n_dat samples per pol from `in`, which starts `pad` samples into the series (a read
  // offset: streaming kernel, or the fused kernel with `pre`); pre: those pad samples (the
  // stream carry, pol stride pad); null: zeros
  const float2* in = nullptr;
  int64_t in_ps = 0, n_dat = 0, pad = 0;
  const float2* pre = nullptr;
  // output: the call's base, or behind a strided layout
  float2* out = nullptr;
  int64_t out_ps = 0;
  const OutLayout* lay = nullptr;
  // rows [row0, K_end) of a call whose output has K_total rows per pol (the padded variant's
  // circular shift is modulo K_total)
  int64_t row0 = 0, K_end = 0, K_total = 0;
  // stage-1 rows (round trip only): also emit the synthesis stage-1 rows of rows >= z_row0 into
  // z[pol][k - z_row0][t0] (AnalysisArgs::z), in runs of zblk rows; z_stage 1 / 2: only the FIR /
  // only the row FFT of the generic path
  float2* z = nullptr;
  int64_t z_ps = 0, z_row0 = 0;
  int zblk = 0, z_stage = 0;
  const CarryOut* carry_out = nullptr;
  // the launch reads the section instead of `in` (analysis_dada_fusable plans only)
  const AnaDada* dada_in = nullptr;
  // the launch writes the section instead of `out`, which is ignored
  // (analysis_dada_out_fusable plans only).  dada_keep: the rows of it that exist — a padded
  // stream call computes K_end = K rows for the circular shift and returns Kt; shifted rows
  // [Kt, K) are not made (AnalysisArgs::out_keep); negative: all K_end rows
  const AnaOut* dada_out = nullptr;
  int64_t dada_keep = -1;
  // the launch stores the plain cf32 product and its moments (streaming-kernel plans only)
  AnaMoments* moments = nullptr;
  // the launch rounds its new samples at the load (the input quantiser, FUSED: streaming-kernel
  // plans, the plain cf32 product with or without its moments)
  const AnaQin* qin = nullptr;
};

pfb_status analysis_run(pfb_analysis_plan* p, const AnaLaunch& l, hipStream_t s);
int64_t analysis_K(const pfb_analysis_plan* p, int64_t n_dat);
// the shape fields of pfb::AnalysisArgs (variant, N, M, P, nu, n_pol) the kernels' predicates read
pfb::AnalysisArgs analysis_shape(const pfb_analysis_plan* p);
bool analysis_emits_z(const pfb_analysis_plan* p);
bool analysis_emits_zblk(const pfb_analysis_plan* p);
// STAGED: samples [t0, t0 + n) of the section unpacked to dst[pol][0, n)
pfb_status section_unpack(const pfb_analysis_plan* p, const DadaSection& sec, int64_t t0, int64_t n, float2* dst,
                          int64_t dps, hipStream_t s);

// ====================================================================== synthesis launches
// PFB_STAGE1_AUTO: recomputed stage-1 rows in the Nf = 256 round trip
constexpr bool kSynthFirDefault = false;

// the input series a synthesis recomputes its stage-1 rows from (SynthBlockArgs::fir_*)
struct FirSrc {
  const float2* x;
  int64_t x_ps, n_dat, q0;
  const float* g;
  int nu, de, pe;
};

// Where the block launches of a call store: the cf32 series out[pol][t] (pol stride out_ps), or
// the DADA section `dada` instead (TFP, NDIM 2, NBIT 8 / 16 / 32, aligned to a complex sample,
// each component to_sample(scale * y): SynthBlockArgs::dout; synthesis_dada_out_fusable plans
// only), and `out` stays null.  Either way no sample at or past out_limit is stored.
struct SynthDada {
  void* base = nullptr;
  int nbit = 0;
  float scale = 1.f;
};
struct SynthOut {
  float2* out = nullptr;
  int64_t out_ps = 0, out_limit = 0;
  SynthDada dada;
};

// One block-kernel launch over blocks [b0, b0 + nb); Z row 0 is channelised row b0 * keep, in
// runs of zblk rows; fir: the rows are recomputed from the input series instead
struct SynthLaunch {
  const float2* Z = nullptr;
  int64_t z_ps = 0, b0 = 0, nb = 0;
  SynthOut o;
  int zblk = 0;
  const FirSrc* fir = nullptr;
};

// The channelised rows a synthesis call reads, wherever they lie.  Every row index the two
// operations take is a row of this source; row0 says where the call's rows sit in it.
struct SynthRows {
  enum Kind { PACKED, DADA, STRIDED };
  pfb_synthesis_plan* plan = nullptr;
  Kind kind = PACKED;
  // PACKED: cf32 [pol][row][chan] from `base`, pol stride ps; copy: how a copy out of it goes
  // (HostToDevice for a caller's host buffer)
  const float2* base = nullptr;
  int64_t ps = 0;
  hipMemcpyKind copy = hipMemcpyDeviceToDevice;
  // DADA: a section the channel IFFT reads in place (dada_fusable); STRIDED: rows behind a
  // strided layout it reads through (strided_in_place).  Their t0 is set launch by launch.
  pfb::DadaIn dada{};
  pfb::StridedIn strided{};
  int64_t rows = 0;  // rows available from row 0 of the source
  // The row of the source that is the call's row 0: block b reads from row row0 + b keep on.
  // Positive: the call starts that many rows in (a sample offset).  Negative: the call's first
  // -row0 rows are not in this source (a stream call whose carried rows are not in front of the
  // new ones), and only blocks that start at or after them may be run on it.
  int64_t row0 = 0;

  static SynthRows packed(pfb_synthesis_plan* p, const float2* base, int64_t ps, int64_t rows) {
    SynthRows r;
    r.plan = p;
    r.base = base;
    r.ps = ps;
    r.rows = rows;
    return r;
  }
  // The input side of `c` for rows [r, r + n): the launch reads them in place (a section or a
  // layout must hold them all; the plan's last_dada / last_strided then report FUSED /
  // IN_PLACE).  `c` points into this object.
  pfb_status chan_in(int64_t r, int64_t n, pfb::ChanIfftArgs& c);
  // Rows [r, r + n) -> dst[pol][0, n N), pol stride dps: a copy, the unpack kernel or the
  // strided-rows copy kernel (last_dada / last_strided report STAGED unless a launch of the
  // call has read in place already)
  hipError_t copy_to(int64_t r, int64_t n, float2* dst, int64_t dps, hipStream_t s) const;
};

// blocks [lo, hi) of a call
struct Blocks {
  int64_t lo, hi;
};

pfb::SynthBlockArgs synth_args(const pfb_synthesis_plan* p, const SynthLaunch& l);
pfb_status synthesis_blocks(pfb_synthesis_plan* p, const SynthLaunch& l, hipStream_t s);
pfb_status synthesis_chunk(SynthRows rows, Blocks b, const SynthOut& out, hipStream_t s);
int64_t synth_blocks(const pfb_synthesis_plan* p, int64_t n_dat);
void zkey_clear(pfb_synthesis_plan* p);
bool synthesis_dada_out_fusable(const pfb_synthesis_plan* p, const void* out, int nbit);

}  // namespace pfb::host
