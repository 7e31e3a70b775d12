// pfb_api.hip — C ABI of the MI355X PFB engine (declared in include/pfb_api.h).
//
// Host-side plan management: tap padding, twiddle / deripple / window tables computed
// in double and rounded once to float, device scratch, the FilterBank /
// InverseFilterBank streaming state (carry-over buffers) and kernel dispatch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <string>
#include <vector>

#include "pfb_api.h"
#include "pfb_kernels.hpp"

namespace {

thread_local std::string g_err;

pfb_status fail(pfb_status s, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return s;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(e_ == hipErrorOutOfMemory ? PFB_ERR_OOM : PFB_ERR_HIP, "%s: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                  \
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
std::vector<float2> twiddles(int64_t n, int sign) {
  std::vector<float2> t((size_t)n);
  for (int64_t m = 0; m < n; ++m) {
    int64_t mm = m;
    if (2 * mm > n) mm -= n;
    const double a = 2.0 * M_PI * (double)mm / (double)n;
    t[(size_t)m] = make_float2((float)std::cos(a), (float)(sign * std::sin(a)));
  }
  return t;
}

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
  void drain() {
    for (auto& r : pending) {
      float ms = 0.f;
      if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
        total_ms[r.which] += ms;
        launches[r.which] += 1;
        bytes[r.which] += r.bytes;
      }
      pool.push_back(r.a);
      pool.push_back(r.b);
    }
    pending.clear();
  }
};
Profiler g_prof;
thread_local pfb::LaunchEvents g_armed;
thread_local const char* g_launched = nullptr;

static std::string demangle(const char* name) {
  if (!name) return std::string();
  int st = 0;
  char* d = abi::__cxa_demangle(name, nullptr, nullptr, &st);
  std::string out = (st == 0 && d) ? std::string(d) : std::string(name);
  std::free(d);
  return out;
}

// Times the launch(es) issued while in scope.  single = true: exactly one kernel launch
// goes through pfb::launch_kernel, which records the two events inside its own dispatch
// (hipExtLaunchKernelGGL) — the kernel's own duration, as a kernel trace measures it.
// single = false (multi-kernel paths): events recorded on the stream around the scope.
struct ProfScope {
  hipEvent_t a = nullptr, b = nullptr;
  int which;
  double bytes;
  hipStream_t s;
  bool single;
  ProfScope(int w, double by, hipStream_t st, bool one = true) : which(w), bytes(by), s(st), single(one) {
    if (g_prof.enabled) {
      a = g_prof.get();
      b = g_prof.get();
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
    if (g_prof.enabled && a && b) {
      if (single) {
        pfb::LaunchEvents& ev = pfb::armed_launch_events();
        if (ev.start) {  // not consumed (no kernel launched): drop the record
          ev = pfb::LaunchEvents{};
          g_prof.pool.push_back(a);
          g_prof.pool.push_back(b);
          return;
        }
        if (pfb::launched_kernel_name()) g_prof.names[which] = demangle(pfb::launched_kernel_name());
      } else {
        (void)hipEventRecord(b, s);
      }
      g_prof.pending.push_back({which, a, b, bytes});
    }
  }
};

int64_t floordiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// n_pol rows of n complex samples at (dst + q*dps) <- (src + q*sps): one 2-D copy, not
// n_pol calls (the two-stage cascades run thousands of series through one plan)
hipError_t copy_pols(float2* dst, int64_t dps, const float2* src, int64_t sps, int64_t n, int n_pol,
                     hipMemcpyKind kind, hipStream_t s) {
  if (n <= 0 || n_pol <= 0) return hipSuccess;
  if (n_pol == 1) return hipMemcpyAsync(dst, src, n * sizeof(float2), kind, s);
  if (kind == hipMemcpyDeviceToDevice) return pfb::launch_copy_rows(dst, dps, src, sps, n, n_pol, s);
  hipError_t e = hipMemcpy2DAsync(dst, dps * sizeof(float2), src, sps * sizeof(float2), n * sizeof(float2),
                                  n_pol, kind, s);
  if (e == hipSuccess) return e;
  (void)hipGetLastError();  // large row pitches: one copy per row instead
  for (int q = 0; q < n_pol; ++q) {
    e = hipMemcpyAsync(dst + q * dps, src + q * sps, n * sizeof(float2), kind, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

pfb::LaunchEvents& pfb::armed_launch_events() { return g_armed; }
const char*& pfb::launched_kernel_name() { return g_launched; }

// error channel shared with the other C-ABI translation units (pfb_layout.hip)
pfb_status pfb_set_error(pfb_status s, const char* msg) { return fail(s, "%s", msg); }

// ====================================================================== analysis plan
// LowCBF: a call that passed every argument check consumes the one-time pre-padding
// (polyphase_analysis_lowcbf.m:27-34) when it returns — a successful call without output rows
// too, as the Matlab wrapper does.  A rejected call (null output, capacity, stride) returns
// before `accept()` and leaves the padding pending, so the corrected retry computes the same
// rows a first call would have.  (The launch reads the flag: it is cleared on exit, not here.)
struct PadConsume {
  bool* flag;
  bool accepted = false;
  void accept() { accepted = true; }
  ~PadConsume() {
    if (accepted) *flag = false;
  }
};

struct pfb_analysis_plan {
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
  // round trip (pfb_roundtrip_execute): the analysis runs on this stream, ahead of the
  // synthesis on the caller's stream; one event per chunk orders them
  hipStream_t aux = nullptr;
  std::vector<hipEvent_t> events;
};

// Rows [row0, K_end) of a call whose output has K_total rows per pol (the padded
// variant's circular shift is modulo K_total).  `in`/`out` are the call's bases.
// z (round trip only): also emit the synthesis stage-1 rows of rows >= z_row0 into
// z[pol][k - z_row0][t0] (AnalysisArgs::z).
// Strided channelised output (AnalysisArgs::out_rs): pfb_filterbank_execute_strided.
// keep: the rows the call returns (T_out; a padded plan computes K >= T_out rows and stores
// only the shifted rows below it, AnalysisArgs::out_keep)
struct OutLayout {
  int64_t rs, cs;
  int32_t split, shift, nsel;
  int64_t keep;
};

static pfb::AnalysisArgs analysis_args(const pfb_analysis_plan* p, const float2* in, int64_t in_ps, int64_t n_dat,
                                       float2* out, int64_t out_ps, int64_t row0, int64_t K_end,
                                       int64_t K_total, float2* z, int64_t z_ps, int64_t z_row0, int64_t pad,
                                       const OutLayout* lay, int zblk, const float2* pre = nullptr);

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

// dd: the launch reads the section instead of `in` (analysis_dada_fusable plans only)
// od: the launch writes the section instead of `out` (analysis_dada_out_fusable plans only;
// `out` and out_ps are ignored)
static pfb_status analysis_run(pfb_analysis_plan* p, const float2* in, int64_t in_ps, int64_t n_dat,
                               float2* out, int64_t out_ps, int64_t row0, int64_t K_end,
                               int64_t K_total, hipStream_t s, float2* z = nullptr,
                               int64_t z_ps = 0, int64_t z_row0 = 0, int64_t pad = 0,
                               const OutLayout* lay = nullptr, int zblk = 0, const float2* pre = nullptr,
                               int z_stage = 0, const CarryOut* co = nullptr, const AnaDada* dd = nullptr,
                               const AnaOut* od = nullptr) {
  if (K_end <= row0) return PFB_OK;
  if (dd) p->last_dada = PFB_DADA_INPUT_FUSED;
  if (od) {
    // (with stage-1 rows: only the file-to-file round trip's launch — a section read in place,
    // the float section and 2-row runs, pfb::launch_stream_rt_dada)
    const bool rt = z && dd && od->nbit == 32 && zblk == 2 && z_stage == 0 && !pre && !co;
    if ((z && !rt) || lay || row0 != 0) return fail(PFB_ERR_UNSUPPORTED, "DADA output: the plain product only");
    out = nullptr;
    out_ps = 0;
  }
  const double in_b = dd ? 2.0 * (dd->nbit / 8) : 8.0;  // bytes per input sample
  const double out_b = od ? 2.0 * (od->nbit / 8) : 8.0;  // bytes per output sample
  if (p->variant == pfb::kLowCbf) {
    pfb::LowCbfArgs l{};
    l.in = in;
    l.in_pol_stride = in_ps;
    l.n_dat = n_dat;
    // (a DADA stream call: the carried samples in front of the section, pad = their count)
    l.pad = pre ? pad : p->lowcbf_pad ? 1536 : 0;
    l.pre = pre;
    if (dd) {
      l.din = dd->base;
      l.din_nbit = dd->nbit;
    }
    if (od) {
      l.dout = od->base;
      l.dout_nbit = od->nbit;
      l.dout_scale = od->scale;
    }
    l.out = out;
    l.out_pol_stride = out_ps;
    l.K = K_end;
    l.n_pol = p->n_pol;
    l.taps = p->taps.as<float>();
    l.tw = p->twN.as<float2>();
    l.scale = 4096.0f;  // 2^9 * 2048 * 256 / 2^9 / 128
    ProfScope ps(0, (double)p->n_pol * (in_b * n_dat + out_b * K_end * p->C), s);
    HIPCHK(pfb::launch_lowcbf(l, s));
    return PFB_OK;
  }
  pfb::AnalysisArgs a = analysis_args(p, in, in_ps, n_dat, out, out_ps, row0, K_end, K_total, z, z_ps, z_row0,
                                      pad, lay, zblk, pre);
  a.z_stage = z_stage;
  if (co) {
    a.carry_out = co->dst;
    a.carry_src = co->src;
    a.carry_n = co->n;
    a.carry_pol_stride = co->dst_ps;
  }
  if (dd) {
    a.din = dd->base;
    a.din_nbit = dd->nbit;
  }
  if (od) {
    a.dout = od->base;
    a.dout_nbit = od->nbit;
    a.dout_scale = od->scale;
  }
  a.scratch = nullptr;
  if (!p->fused && !z) {
    HIPCHK(p->scratch.ensure((size_t)p->n_pol * (K_end - row0) * p->N * sizeof(float2)));
    a.scratch = p->scratch.as<float2>();
  }
  // algorithmic bytes: each input sample read once (the rows' new samples, the tail of
  // the series with the last rows), each output sample written once
  const int64_t in_samples = (K_end == K_total && row0 == 0)
                                 ? n_dat
                                 : (K_end - row0) * p->M + (K_end == K_total ? n_dat - K_total * p->M : 0);
  // (with z: the stage-1 rows are a synthesis intermediate, not algorithmic bytes —
  // the synthesis' algorithmic read of its input is counted by the block kernel)
  const double bytes = (double)p->n_pol * (in_b * in_samples + out_b * (K_end - row0) * p->N);
  // generic path = FIR + row FFT launches (z_stage 1 / 2: one of them, timed as its own
  // class; their bytes: the FIR reads the input and writes the stage-1 rows, the row FFT
  // reads them and writes the channelised product)
  const double zrow_bytes = (double)p->n_pol * 8.0 * (K_end - row0) * p->N;
  const int cls = !z ? 0 : z_stage == 1 ? 4 : z_stage == 2 ? 5 : 3;
  const double cls_bytes = z_stage == 1 ? (double)p->n_pol * 8.0 * in_samples + zrow_bytes
                           : z_stage == 2 ? 2.0 * zrow_bytes : bytes;
  ProfScope ps(cls, cls_bytes, s, p->fused || z_stage != 0);
  if (dd && !p->fused) {
    // the FIR of the N > 256 path reads the section: timed alone as class 4, which names it
    ProfScope fir(4, (double)p->n_pol * in_b * in_samples + zrow_bytes, s);
    HIPCHK(pfb::launch_analysis(a, s));
    return PFB_OK;
  }
  HIPCHK(pfb::launch_analysis(a, s));
  return PFB_OK;
}

static pfb::AnalysisArgs analysis_args(const pfb_analysis_plan* p, const float2* in, int64_t in_ps, int64_t n_dat,
                                       float2* out, int64_t out_ps, int64_t row0, int64_t K_end,
                                       int64_t K_total, float2* z, int64_t z_ps, int64_t z_row0, int64_t pad,
                                       const OutLayout* lay, int zblk, const float2* pre) {
  pfb::AnalysisArgs a{};
  a.pre = pre;        // the pad samples in front of `in` (stream carry); null: zeros
  a.pre_pol_stride = pad;
  a.z = z;
  a.z_pol_stride = z_ps;
  a.z_row0 = z_row0;
  a.zblk = zblk;
  a.in = in;
  a.in_pol_stride = in_ps;
  a.n_dat = n_dat;
  a.out = out;
  a.out_pol_stride = out_ps;
  a.row0 = row0;
  a.K = K_end;
  a.K_total = K_total;
  a.n_pol = p->n_pol;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  a.sds = p->sds;
  a.variant = p->variant;
  a.taps = p->taps.as<float>();
  a.twN = p->twN.as<float2>();
  a.zrev = p->zrev.p ? p->zrev.as<int>() : nullptr;
  a.pad = pad;  // `in` starts `pad` samples into the series (streaming kernel only)
  if (lay) {
    a.out_rs = (int)lay->rs;
    a.out_cs = (int)lay->cs;
    a.sel_split = lay->split;
    a.sel_shift = lay->shift;
    a.sel_n = lay->nsel;
    a.out_keep = lay->keep;
  }
  return a;
}

// the plan's analysis runs on the streaming kernel, which takes a read offset (pad)
static bool analysis_offset_ok(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  return pfb::analysis_takes_offset(a);
}

// FUSED (pfb_api.h): the plan's kernel loads such a section itself
static bool analysis_dada_fusable(const pfb_analysis_plan* p, const void* base, int nbit, int ndim, int order) {
  if (ndim != 2 || order != PFB_DADA_TFP || (nbit != 8 && nbit != 16 && nbit != 32)) return false;
  if (reinterpret_cast<uintptr_t>(base) % (size_t)(nbit / 4) != 0) return false;
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  a.n_pol = p->n_pol;
  if (p->variant == pfb::kLowCbf) {
    // (the streaming kernel's LCBF instantiation, unless the experiments build's knob picks
    // the one-shot kernel: pfb_lowcbf.hip)
    if (pfb::knob("PFB_LOWCBF_STREAM") && std::atoi(pfb::knob("PFB_LOWCBF_STREAM")) == 0) return false;
    a.variant = pfb::kBunton;
  }
  return pfb::analysis_reads_dada(a, nbit);
}

// FUSED output (pfb_api.h): the plan's kernel stores such a section itself
static bool analysis_dada_out_fusable(const pfb_analysis_plan* p, const void* base, int nbit) {
  if (nbit != 8 && nbit != 16 && nbit != 32) return false;
  if (reinterpret_cast<uintptr_t>(base) % (size_t)(nbit / 4) != 0) return false;
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  a.n_pol = p->n_pol;
  if (p->variant == pfb::kLowCbf) {
    // (the streaming kernel's LCBF instantiation: analysis_dada_fusable's note)
    if (pfb::knob("PFB_LOWCBF_STREAM") && std::atoi(pfb::knob("PFB_LOWCBF_STREAM")) == 0) return false;
    a.variant = pfb::kBunton;
  }
  return pfb::analysis_writes_dada(a, nbit);
}

static bool analysis_fused_carry_ok(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  return pfb::analysis_fused_takes_carry(a);
}

static bool analysis_emits_z(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  return pfb::analysis_can_emit_z(a);  // streaming kernel (N = 256) or register-window FIR
}

static bool analysis_emits_zblk(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  return pfb::analysis_can_emit_zblk(a);  // streaming kernel (N = 256)
}

static int64_t analysis_K(const pfb_analysis_plan* p, int64_t n_dat) {
  if (p->variant == pfb::kLowCbf) {  // PSTFilterbank.m:14-15
    const int64_t k = floordiv(n_dat + (p->lowcbf_pad ? 1536 : 0) - 3072, 192);
    return std::max<int64_t>(k, 0);
  }
  if (p->variant == pfb::kBunton) {
    const int64_t k = floordiv(n_dat - (int64_t)p->P * p->N, p->M);
    return std::max<int64_t>(k, 0);
  }
  return std::max<int64_t>(n_dat / p->M, 0);
}

extern "C" {

const char* pfb_last_error(void) { return g_err.c_str(); }
int32_t pfb_api_version(void) { return PFB_API_VERSION; }

int32_t pfb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Descriptor checks of pfb_analysis_plan_create (no device needed); fills the plan's
// scalar parameters into `p`
static pfb_status analysis_validate(const pfb_analysis_desc* d, pfb_analysis_plan* p) {
  if (!d) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (d->variant == PFB_ANALYSIS_LOWCBF &&
      (d->n_chan != 256 || d->os_nu != 4 || d->os_de != 3 || d->n_taps != 3072))
    return fail(PFB_ERR_INVALID_ARG,
                "polyphase_analysis_lowcbf is the fixed 256-channel 4/3 PST filterbank with "
                "3072 taps (PSTFilterbank.m:7-15); got n_chan=%d os=%d/%d taps=%lld",
                d->n_chan, d->os_nu, d->os_de, (long long)d->n_taps);
  if (d->variant != PFB_ANALYSIS_BUNTON && d->variant != PFB_ANALYSIS_PADDED &&
      d->variant != PFB_ANALYSIS_LOWCBF)
    return fail(PFB_ERR_INVALID_ARG, "unknown analysis variant %d", d->variant);
  if (d->n_chan <= 0 || d->os_nu <= 0 || d->os_de <= 0 || d->os_de > d->os_nu)
    return fail(PFB_ERR_INVALID_ARG, "invalid n_chan/os_factor (%d, %d/%d)", d->n_chan, d->os_nu,
                d->os_de);
  if (!d->taps || d->n_taps <= 0) return fail(PFB_ERR_INVALID_ARG, "no filter taps");
  if (d->n_pol <= 0) return fail(PFB_ERR_INVALID_ARG, "n_pol must be positive");
  if (d->n_pol > 65535)  // polarisations map to grid.y of every launch
    return fail(PFB_ERR_INVALID_ARG, "n_pol = %d exceeds 65535 series per plan", d->n_pol);
  // (sizes whose products the tables and kernels form in 32-bit ints: far beyond any
  // configuration, rejected before any arithmetic on them)
  if (d->n_chan > (1 << 24) || d->os_nu > (1 << 16) || d->n_taps > ((int64_t)1 << 30))
    return fail(PFB_ERR_UNSUPPORTED, "analysis parameters out of range (n_chan %d, os_nu %d, %lld taps)",
                d->n_chan, d->os_nu, (long long)d->n_taps);
  p->variant = d->variant;
  p->N = d->n_chan;
  p->nu = d->os_nu;
  p->de = d->os_de;
  p->M = (int)(((int64_t)d->n_chan * d->os_de) / d->os_nu);  // floor, polyphase_analysis.m:56
  p->n_taps = d->n_taps;
  p->P = (int)((d->n_taps + d->n_chan - 1) / d->n_chan);    // pad_filter.m:10
  p->n_pol = d->n_pol;
  if (p->M <= 0) return fail(PFB_ERR_INVALID_ARG, "commutator step M = floor(N de/nu) is zero");
  p->sds = (int)std::ceil((double)(d->n_taps - 1) / 2.0 / (double)p->M);  // padded.m:89
  p->C = p->N;
  if (p->variant == pfb::kLowCbf) {
    p->C = 216;
    p->lowcbf_pad = true;
    p->fused = true;
  } else if (!pfb::analysis_supported(p->N, p->P, p->variant, &p->fused)) {
    return fail(PFB_ERR_UNSUPPORTED, "no analysis kernel for n_chan=%d", d->n_chan);
  }
  return PFB_OK;
}

// Host-side tables of an analysis plan
struct AnaHost {
  std::vector<float> taps, g;
  std::vector<int> rev;
};

static void analysis_host_tables(const pfb_analysis_desc* d, const pfb_analysis_plan* p, AnaHost& h) {
  // zero rows up to the fused kernel's PMAX (32) so its tap loads are unconditional
  h.taps.assign((size_t)std::max(p->P, 32) * p->N, 0.f);
  for (int64_t i = 0; i < d->n_taps; ++i) h.taps[(size_t)i] = (float)d->taps[i];  // cast(filt, 'single')
  if (analysis_emits_zblk(p) && p->N == 256) {
    // g_s[m][c] = N^2 F[(m + 1) N + c - (s M mod N)], F = [N zeros, taps, zeros] — the
    // streaming kernel's folded taps (pfb_ana_stream.hpp), scaled by the power of two N^2
    // (exact), lags m < P + 1, zero-padded to 16 per (s, c)
    const int N = p->N, PE = p->P + 1;
    const float n2 = (float)N * (float)N;
    h.g.assign((size_t)p->nu * N * 16, 0.f);
    for (int sr = 0; sr < p->nu; ++sr) {
      const int as = (int)(((int64_t)sr * p->M) % N);
      for (int c = 0; c < N; ++c)
        for (int m = 0; m < PE; ++m) {
          const int j = (m + 1) * N + c - as;
          const float f = (j >= N && j < (p->P + 1) * N) ? h.taps[(size_t)(j - N)] : 0.f;
          h.g[((size_t)sr * N + c) * 16 + m] = n2 * f;
        }
    }
  }
  if (!p->fused && p->variant == pfb::kPadded) {
    h.rev.resize((size_t)p->N);
    for (int i = 0; i < p->N; ++i) h.rev[(size_t)i] = (p->N - i) % p->N;
  }
}

static void analysis_release(pfb_analysis_plan* p) {
  for (DevBuf* b : {&p->taps, &p->twN, &p->zrev, &p->gtab, &p->scratch, &p->carry, &p->carry_next, &p->work, &p->stage_in,
                    &p->stage_out, &p->dada_stage})
    b->release();
}

pfb_status pfb_analysis_plan_validate(const pfb_analysis_desc* d) {
  pfb_analysis_plan p;
  const pfb_status st = analysis_validate(d, &p);
  if (st != PFB_OK) return st;
  AnaHost h;
  analysis_host_tables(d, &p, h);
  return PFB_OK;
}

pfb_status pfb_analysis_plan_create(const pfb_analysis_desc* d, pfb_analysis_plan** out) {
  if (!d || !out) return fail(PFB_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  pfb_analysis_plan tmp;
  const pfb_status vst = analysis_validate(d, &tmp);
  if (vst != PFB_OK) return vst;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PFB_ERR_NO_DEVICE, "no HIP device available");
  if (d->device < 0 || d->device >= ndev)
    return fail(PFB_ERR_INVALID_ARG, "device %d out of range (%d devices)", d->device, ndev);
  if (hipSetDevice(d->device) != hipSuccess) return fail(PFB_ERR_HIP, "hipSetDevice(%d) failed", d->device);
  AnaHost h;
  analysis_host_tables(d, &tmp, h);
  static std::atomic<uint64_t> next_serial{1};
  auto* p = new pfb_analysis_plan(tmp);
  p->serial = next_serial++;
  p->device = d->device;
  hipError_t e = upload(p->taps, h.taps);
  if (e == hipSuccess) e = upload(p->twN, twiddles(p->N, -1));
  if (e == hipSuccess && !h.g.empty()) e = upload(p->gtab, h.g);
  if (e == hipSuccess && !h.rev.empty()) e = upload(p->zrev, h.rev);
  if (e != hipSuccess) {
    analysis_release(p);
    delete p;
    return fail(PFB_ERR_HIP, "analysis plan upload: %s", hipGetErrorString(e));
  }
  *out = p;
  return PFB_OK;
}

pfb_status pfb_analysis_plan_destroy(pfb_analysis_plan* p) {
  if (!p) return PFB_OK;
  (void)hipSetDevice(p->device);
  analysis_release(p);
  for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
  if (p->aux) (void)hipStreamDestroy(p->aux);
  delete p;
  return PFB_OK;
}

int32_t pfb_analysis_output_channels(const pfb_analysis_plan* p) { return p ? p->C : -1; }

int64_t pfb_analysis_output_length(const pfb_analysis_plan* p, int64_t n_dat) {
  if (!p) return -1;
  return analysis_K(p, n_dat);
}

// A DADA data section as the input of an analysis call (pfb_analysis_execute_dada,
// pfb_filterbank_execute_dada): n samples x 1 channel x the plan's n_pol x ndim values of nbit
struct AnaSection {
  const void* base;
  int nbit, ndim, order;
  // unpack it even where the kernel could read it in place (a _dada_to_dada call whose NBIT
  // pair the DADA-store kernels do not read in place: pfb::dadaout_reads_dada)
  bool force_staged = false;
};

static bool ana_section_fusable(const pfb_analysis_plan* p, const AnaSection& sec) {
  return !sec.force_staged && analysis_dada_fusable(p, sec.base, sec.nbit, sec.ndim, sec.order);
}

static pfb_status ana_section_check(const pfb_analysis_plan* p, const AnaSection& sec, int64_t n) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (sec.nbit != 8 && sec.nbit != 16 && sec.nbit != 32 && sec.nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "NBIT must be 8, 16, 32 or 64");
  if (sec.ndim != 1 && sec.ndim != 2) return fail(PFB_ERR_INVALID_ARG, "NDIM must be 1 or 2");
  if (sec.order != PFB_DADA_TFP && sec.order != PFB_DADA_LOWCBF)
    return fail(PFB_ERR_INVALID_ARG, "unknown sample order");
  if (sec.order == PFB_DADA_LOWCBF && n > 0 && n % 32)
    return fail(PFB_ERR_INVALID_ARG, "LowCBF data are heaps of 32 samples");
  return PFB_OK;
}

// STAGED: samples [t0, t0 + n) of the section unpacked to dst[pol][0, n) (pfb_dada_unpack; a
// LowCBF section from a heap boundary only)
static pfb_status ana_section_unpack(const pfb_analysis_plan* p, const AnaSection& sec, int64_t t0, int64_t n,
                                     float2* dst, int64_t dps, hipStream_t s) {
  if (n <= 0) return PFB_OK;
  const char* src = static_cast<const char*>(sec.base) + t0 * p->n_pol * sec.ndim * (sec.nbit / 8);
  return pfb_dada_unpack(src, sec.nbit, sec.ndim, sec.order, n, 1, p->n_pol, reinterpret_cast<pfb_cf32*>(dst), dps,
                         s);
}

// pfb_analysis_execute; sec: the series are a DADA section (device memory) instead of `in`;
// od: the product goes out as a DADA section (device memory, FUSED) instead of `out`, which
// then only has to pass the checks
static pfb_status analysis_exec(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, const AnaSection* sec,
                                int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                                int32_t mem, void* stream, const AnaOut* od = nullptr) {
  if (sec) in = static_cast<const pfb_cf32*>(sec->base);
  if (!p || (!in && n_dat > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n_dat < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_dat");
  HIPCHK(hipSetDevice(p->device));
  p->last_dada = PFB_DADA_INPUT_NONE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t K = analysis_K(p, n_dat);
  PadConsume pad_once{&p->lowcbf_pad};
  if (n_out) *n_out = K;
  if (K == 0) {
    pad_once.accept();
    // (no launch: the path the section's rows would have taken)
    if (sec) p->last_dada = ana_section_fusable(p, *sec) ? PFB_DADA_INPUT_FUSED : PFB_DADA_INPUT_STAGED;
    return PFB_OK;
  }
  if (!out) return fail(PFB_ERR_INVALID_ARG, "null output");
  if (cap < K) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                           (long long)cap, (long long)K);
  if (mem == PFB_MEM_DEVICE && ((!sec && in_ps < n_dat) || out_ps < K * p->C))
    return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  pad_once.accept();
  if (sec) {
    if (ana_section_fusable(p, *sec)) {
      const AnaDada dd{sec->base, sec->nbit};
      return analysis_run(p, nullptr, 0, n_dat, (float2*)out, out_ps, 0, K, K, s, nullptr, 0, 0, 0, nullptr, 0,
                          nullptr, 0, nullptr, &dd, od);
    }
    HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n_dat * sizeof(float2)));
    p->last_dada = PFB_DADA_INPUT_STAGED;
    const pfb_status st = ana_section_unpack(p, *sec, 0, n_dat, p->stage_in.as<float2>(), n_dat, s);
    if (st != PFB_OK) return st;
    return analysis_run(p, p->stage_in.as<float2>(), n_dat, n_dat, (float2*)out, out_ps, 0, K, K, s, nullptr, 0, 0, 0,
                        nullptr, 0, nullptr, 0, nullptr, nullptr, od);
  }
  if (mem == PFB_MEM_DEVICE) {
    return analysis_run(p, (const float2*)in, in_ps, n_dat, (float2*)out, out_ps, 0, K, K, s, nullptr, 0, 0, 0,
                        nullptr, 0, nullptr, 0, nullptr, nullptr, od);
  }
  // host staging (synchronous)
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n_dat * sizeof(float2)));
  HIPCHK(p->stage_out.ensure((size_t)p->n_pol * K * p->C * sizeof(float2)));
  HIPCHK(copy_pols(p->stage_in.as<float2>(), n_dat, (const float2*)in, in_ps, n_dat, p->n_pol,
                   hipMemcpyHostToDevice, s));
  pfb_status st = analysis_run(p, p->stage_in.as<float2>(), n_dat, n_dat,
                               p->stage_out.as<float2>(), K * p->C, 0, K, K, s);
  if (st != PFB_OK) return st;
  HIPCHK(copy_pols((float2*)out, out_ps, p->stage_out.as<float2>(), K * p->C, K * p->C, p->n_pol,
                   hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

// a cf32-output call that went through: pfb_analysis_last_dada_output reports NONE again
static pfb_status cf32_output(pfb_analysis_plan* p, pfb_status st) {
  if (p && st == PFB_OK) p->last_dada_out = PFB_DADA_OUTPUT_NONE;
  return st;
}

pfb_status pfb_analysis_execute(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                int64_t* n_out, int32_t mem, void* stream) {
  return cf32_output(p, analysis_exec(p, in, in_ps, nullptr, n_dat, out, out_ps, cap, n_out, mem, stream));
}

pfb_status pfb_analysis_execute_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                     int32_t order, int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                     int64_t* n_out, void* stream) {
  const AnaSection sec{in, nbit, ndim, order};
  const pfb_status st = ana_section_check(p, sec, n_dat);
  if (st != PFB_OK) return st;
  return cf32_output(p, analysis_exec(p, nullptr, 0, &sec, n_dat, out, out_ps, cap, n_out, PFB_MEM_DEVICE, stream));
}

int32_t pfb_analysis_last_dada_input(const pfb_analysis_plan* p) { return p ? p->last_dada : -1; }

static pfb_status filterbank_exec(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_in,
                                  pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out, int32_t mem,
                                  void* stream, const OutLayout* lay, const AnaSection* sec = nullptr,
                                  const AnaOut* od = nullptr);

pfb_status pfb_filterbank_execute_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                       int32_t order, int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                       int64_t* n_out, void* stream) {
  const AnaSection sec{in, nbit, ndim, order};
  const pfb_status st = ana_section_check(p, sec, n_in);
  if (st != PFB_OK) return st;
  return cf32_output(
      p, filterbank_exec(p, nullptr, 0, n_in, out, out_ps, cap, n_out, PFB_MEM_DEVICE, stream, nullptr, &sec));
}

pfb_status pfb_filterbank_execute(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                  int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                  int64_t* n_out, int32_t mem, void* stream) {
  return cf32_output(p, filterbank_exec(p, in, in_ps, n_in, out, out_ps, cap, n_out, mem, stream, nullptr));
}

int64_t pfb_filterbank_output_rows(const pfb_analysis_plan* p, int64_t n_in) {
  if (!p || n_in < 0) return -1;
  const int64_t K = analysis_K(p, p->buffered + n_in);
  return K - (K % p->nu);
}

pfb_status pfb_filterbank_execute_strided(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                          int64_t n_in, pfb_cf32* out, int64_t out_ps,
                                          int64_t row_stride, int64_t chan_stride, int32_t sel_split,
                                          int32_t sel_shift, int32_t sel_n, int64_t cap,
                                          int64_t* n_out, void* stream) {
  if (!p || (!in && n_in > 0) || !out) return fail(PFB_ERR_INVALID_ARG, "null argument");
  // every padded plan (fused kernel or FIR + row FFT: guarded plain stores, StridedOut), and
  // the Bunton plans of the streaming kernel; nothing is launched and no state changes below
  // until filterbank_exec has made its own checks
  const bool padded = p->variant == pfb::kPadded;
  if (!padded && (p->variant != pfb::kBunton || !analysis_offset_ok(p) || p->lowcbf_pad))
    return fail(PFB_ERR_UNSUPPORTED,
                "strided output needs a padded plan or the streaming Bunton analysis kernel");
  if (row_stride <= 0 || chan_stride <= 0 || sel_n < 0 || sel_split < 0 || sel_shift < 0 ||
      (sel_n > 0 && sel_split + sel_shift > p->C) || sel_n > p->C)
    return fail(PFB_ERR_INVALID_ARG, "bad strided output layout");
  const int64_t jn = sel_n > 0 ? sel_n : p->C;
  if (padded) {
    // the kernels hold the two strides as 32-bit ints and form 64-bit element offsets from
    // them: no descriptor, no extent limit beyond that
    if (row_stride > INT32_MAX || chan_stride > INT32_MAX)
      return fail(PFB_ERR_UNSUPPORTED, "strided output: a stride exceeds 2^31 - 1 elements");
    if (out_ps < 0) return fail(PFB_ERR_INVALID_ARG, "negative polarisation stride");
  } else if ((64 * row_stride + jn * chan_stride + 1) * 8 > pfb::kRsrcMaxBytes) {
    // one 16-row step's extent must fit a 32-bit buffer descriptor (StridedRowStore)
    return fail(PFB_ERR_UNSUPPORTED, "strided output extent exceeds a buffer descriptor");
  }
  // out_capacity counts pfb_cf32 elements from `out`: the furthest element this call writes
  // must lie inside it (a wrong stride is rejected, not written past the buffer)
  const int64_t Kt = pfb_filterbank_output_rows(p, n_in);
  if (n_out) *n_out = Kt;
  if (Kt > 0) {
    const int64_t last = (int64_t)(p->n_pol - 1) * out_ps + (Kt - 1) * row_stride + (jn - 1) * chan_stride;
    if (last >= cap)
      return fail(PFB_ERR_BUFFER_TOO_SMALL,
                  "strided output: element %lld is written but out_capacity is %lld elements",
                  (long long)last, (long long)cap);
  }
  const OutLayout lay{row_stride, chan_stride, sel_split, sel_shift, sel_n, std::max<int64_t>(Kt, 0)};
  return cf32_output(p, filterbank_exec(p, in, in_ps, n_in, out, out_ps, std::max<int64_t>(Kt, 0), n_out,
                                        PFB_MEM_DEVICE, stream, &lay));
}

// The to-DADA calls (pfb_api.h): every check here, before the callee launches or changes the
// stream state; then FUSED — the kernel stores the section (od) — or STAGED — the cf32 path
// into the plan's buffer and the scaled pack launch.
static pfb_status analysis_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, const AnaSection* sec_in,
                                   int64_t n, void* out, int32_t nbit, float scale, int64_t cap_bytes,
                                   int64_t* n_out, void* stream, bool stream_call) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (nbit != 8 && nbit != 16 && nbit != 32 && nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "output NBIT must be 8, 16, 32 or 64");
  if (!std::isfinite(scale)) return fail(PFB_ERR_INVALID_ARG, "output scale is not finite");
  if (reinterpret_cast<uintptr_t>(out) % (size_t)(nbit / 8) != 0)
    return fail(PFB_ERR_INVALID_ARG, "output section not aligned to its NBIT");
  // the input-side conditions of the corresponding cf32-output call
  if (sec_in) {
    const pfb_status st = ana_section_check(p, *sec_in, n);
    if (st != PFB_OK) return st;
  }
  if (!(sec_in ? sec_in->base : (const void*)in) && n > 0) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n < 0) return fail(PFB_ERR_INVALID_ARG, "negative sample count");
  if (!sec_in && in_ps < n) return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  // K: the rows the callee computes (the padded variant's shift spans all of them); rows: the
  // rows it returns (a stream call trims to a multiple of nu, FilterBank.m:93-104)
  const int64_t K = analysis_K(p, stream_call ? p->buffered + n : n);
  const int64_t rows = stream_call ? K - (K % p->nu) : K;
  if (n_out) *n_out = rows;
  if (rows > 0) {
    if (!out) return fail(PFB_ERR_INVALID_ARG, "null output");
    const int64_t need = rows * p->C * p->n_pol * 2 * (nbit / 8);
    if (cap_bytes < need)
      return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld bytes", (long long)cap_bytes,
                  (long long)need);
  }
  HIPCHK(hipSetDevice(p->device));
  const bool fused = analysis_dada_out_fusable(p, out, nbit);
  AnaSection sec{};
  if (sec_in) {
    sec = *sec_in;
    // (the DADA-store kernels read cf32, a section of the output's NBIT, or an integer
    // section when they write NBIT 32)
    if (fused && !pfb::dadaout_reads_dada(sec.nbit, nbit)) sec.force_staged = true;
  }
  const AnaSection* sp = sec_in ? &sec : nullptr;
  pfb_status st;
  if (fused) {
    // (`out` stands in for the cf32 buffer in the callee's null, capacity and stride checks:
    // rows packed rows of capacity; the launch writes through od only)
    const AnaOut od{out, nbit, scale};
    pfb_cf32* o = static_cast<pfb_cf32*>(out);
    st = stream_call ? filterbank_exec(p, in, in_ps, n, o, rows * p->C, rows, n_out, PFB_MEM_DEVICE, stream, nullptr,
                                       sp, &od)
                     : analysis_exec(p, in, in_ps, sp, n, o, rows * p->C, rows, n_out, PFB_MEM_DEVICE, stream, &od);
  } else {
    // all K computed rows have room (a padded stream call then runs straight into the buffer)
    HIPCHK(p->dada_stage.ensure((size_t)p->n_pol * std::max<int64_t>(K, 1) * p->C * sizeof(float2)));
    pfb_cf32* o = p->dada_stage.as<pfb_cf32>();
    st = stream_call
             ? filterbank_exec(p, in, in_ps, n, o, K * p->C, K, n_out, PFB_MEM_DEVICE, stream, nullptr, sp)
             : analysis_exec(p, in, in_ps, sp, n, o, K * p->C, K, n_out, PFB_MEM_DEVICE, stream);
    if (st == PFB_OK)
      HIPCHK(pfb::launch_dada_pack_scaled(p->dada_stage.as<float2>(), K * p->C, rows, p->C, p->n_pol, out, nbit,
                                          scale, (hipStream_t)stream));
  }
  if (st == PFB_OK) p->last_dada_out = fused ? PFB_DADA_OUTPUT_FUSED : PFB_DADA_OUTPUT_STAGED;
  return st;
}

pfb_status pfb_analysis_execute_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_dat,
                                        void* out, int32_t out_nbit, float out_scale, int64_t cap_bytes,
                                        int64_t* n_out, void* stream) {
  return analysis_to_dada(p, in, in_ps, nullptr, n_dat, out, out_nbit, out_scale, cap_bytes, n_out, stream, false);
}

pfb_status pfb_filterbank_execute_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_in,
                                          void* out, int32_t out_nbit, float out_scale, int64_t cap_bytes,
                                          int64_t* n_out, void* stream) {
  return analysis_to_dada(p, in, in_ps, nullptr, n_in, out, out_nbit, out_scale, cap_bytes, n_out, stream, true);
}

pfb_status pfb_analysis_execute_dada_to_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                             int32_t order, int64_t n_dat, void* out, int32_t out_nbit,
                                             float out_scale, int64_t cap_bytes, int64_t* n_out, void* stream) {
  const AnaSection sec{in, nbit, ndim, order};
  return analysis_to_dada(p, nullptr, 0, &sec, n_dat, out, out_nbit, out_scale, cap_bytes, n_out, stream, false);
}

pfb_status pfb_filterbank_execute_dada_to_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                               int32_t order, int64_t n_in, void* out, int32_t out_nbit,
                                               float out_scale, int64_t cap_bytes, int64_t* n_out, void* stream) {
  const AnaSection sec{in, nbit, ndim, order};
  return analysis_to_dada(p, nullptr, 0, &sec, n_in, out, out_nbit, out_scale, cap_bytes, n_out, stream, true);
}

int32_t pfb_analysis_last_dada_output(const pfb_analysis_plan* p) { return p ? p->last_dada_out : -1; }

}  // extern "C"

// sec: the new samples are a DADA section (device memory) instead of `in`.  The carry stays
// packed cf32, so cf32 and DADA calls may alternate on one plan.
// od: the rows go out as a DADA section (device memory, FUSED: a plan on the streaming kernel)
// instead of `out`, which then only has to pass the checks.
static pfb_status filterbank_exec(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_in,
                                  pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out, int32_t mem,
                                  void* stream, const OutLayout* lay, const AnaSection* sec, const AnaOut* od) {
  if (sec) {
    in = static_cast<const pfb_cf32*>(sec->base);
    in_ps = n_in;
  }
  if (!p || (!in && n_in > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n_in < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_in");
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  // FUSED: the kernel reads the section's new samples in place; STAGED: they are unpacked
  // behind the carry in the concatenation buffer and the cf32 path runs
  const bool fus = sec && ana_section_fusable(p, *sec);
  const AnaDada dd_{sec ? sec->base : nullptr, sec ? sec->nbit : 0};
  const AnaDada* dd = fus ? &dd_ : nullptr;
  const int last_dada = !sec ? PFB_DADA_INPUT_NONE : PFB_DADA_INPUT_STAGED;  // (a fused launch sets FUSED)
  const int64_t total = p->buffered + n_in;
  const hipMemcpyKind kin = mem == PFB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (mem == PFB_MEM_DEVICE) {
    // the strides of device buffers are the caller's: checked like pfb_analysis_execute's,
    // before any state changes (`lay`: out_ps belongs to the strided layout, range-checked
    // by pfb_filterbank_execute_strided)
    const int64_t K0 = analysis_K(p, total);
    const int64_t Kt0 = K0 - (K0 % p->nu);
    if (in_ps < n_in || (!lay && out_ps < Kt0 * p->C))
      return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  {
    // Carry without the concatenation copy (streaming analysis kernel, device input): when
    // the new carry starts in the new input (input_idat >= B), ONE launch reads the new
    // input in place with the carried B samples as a read offset (AnalysisArgs::pad), and
    // the carried samples themselves through a second descriptor in its first register
    // window (AnalysisArgs::pre).  The result is the same per row as the concatenated run
    // (same kernel, same samples).
    const int64_t B = p->buffered;
    const int64_t K = analysis_K(p, total);
    const int64_t Kt = K - (K % p->nu);
    const int64_t input_idat = (Kt * p->N * p->de) / p->nu;
    static const bool no_split = pfb::knob("PFB_FB_NO_SPLIT") != nullptr;  // A/B
    // the streaming kernel's register window: DE (16 / NU) new rows per step + P (its first
    // window holds every carried sample a workgroup's rows read when B fits in it —
    // launch_stream checks the same bound).  A stream call leaves at most P N + NU M - 1
    // samples behind (total - Kt M with K - Kt < NU), which is below the window's
    // P N + 16 M for every NU <= 16: every carry this object makes fits
    // (tests/test_stream_model.py enumerates it); a longer one would concatenate below.
    const int64_t win = ((int64_t)p->de * (16 / p->nu) + p->P) * p->N;
    // (a DADA section: fused only, else staged; a fused LowCBF stream call takes this path
    // too — its cf32 call concatenates)
    const bool lcbf_dd = dd && p->variant == pfb::kLowCbf;
    if (!no_split && mem == PFB_MEM_DEVICE && B > 0 && B <= win &&
        ((p->variant == pfb::kBunton && analysis_offset_ok(p)) || lcbf_dd) && input_idat >= B &&
        p->lowcbf_pad == false && (!sec || fus)) {
      if (n_out) *n_out = Kt;
      if (Kt > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                                (long long)cap, (long long)Kt);
      p->last_dada = last_dada;
      // no stitched rows, no copies before the launch; then the new carry (stream order:
      // after the kernel read the old one).
      // (Round 5: the bound was P N; a cascade's stage-2 carry of up to P N + NU M samples
      // per series then took a stitched two-launch path — two copies and a small launch per
      // call.)
      // (round 5) the kernel also copies the next carry into the second carry buffer —
      // no copy launch after it — and the two buffers swap
      const int64_t nb = total - input_idat;
      CarryOut co{nullptr, input_idat - B, nb, nb};
      if (nb > 0) {
        HIPCHK(p->carry_next.ensure((size_t)p->n_pol * nb * sizeof(float2)));
        co.dst = p->carry_next.as<float2>();
      }
      // (the LowCBF instantiation has no carry copy: unpacked by a launch behind it)
      pfb_status st = analysis_run(p, (const float2*)in, in_ps, n_in, (float2*)out, out_ps, 0, Kt, K, s,
                                   nullptr, 0, 0, B, lay, 0, p->carry.as<float2>(), 0,
                                   nb > 0 && !lcbf_dd ? &co : nullptr, dd, od);
      if (st != PFB_OK) return st;
      if (lcbf_dd) {
        st = ana_section_unpack(p, *sec, input_idat - B, nb, co.dst, nb, s);
        if (st != PFB_OK) return st;
      }
      if (nb > 0) std::swap(p->carry, p->carry_next);
      p->buffered = std::max<int64_t>(nb, 0);
      return PFB_OK;
    }
  }
  {
    // Carry without the concatenation copy (fused one-launch kernels: N <= 256 shapes the
    // streaming kernel does not take, e.g. a padded cascade's stage 2): the kernel stages each
    // row's input span from the carry (`pre`, the first B samples of the series) and the input
    // in place (round 6; the SKA-Mid padded cascade copied its 613 MB of stage-2 series here).
    const int64_t B = p->buffered;
    const int64_t K = analysis_K(p, total);
    const int64_t Kt = K - (K % p->nu);
    const int64_t input_idat = (Kt * p->N * p->de) / p->nu;
    // (a layout — pfb_filterbank_execute_strided on a padded plan; the Bunton plans it admits
    // take the streaming kernel above — goes straight to `out`: the launch stores the shifted
    // rows below Kt through the layout and drops rows [Kt, K), so there are no scratch rows
    // and no staging buffer)
    if (!sec && !od && mem == PFB_MEM_DEVICE && B > 0 && !p->lowcbf_pad && p->fused && analysis_fused_carry_ok(p) &&
        input_idat >= B && Kt > 0) {
      p->last_dada = last_dada;
      if (n_out) *n_out = Kt;
      if (Kt > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                                (long long)cap, (long long)Kt);
      const int64_t Krun = p->variant == pfb::kPadded ? K : Kt;
      float2* dst = (float2*)out;
      int64_t dps = out_ps;
      // (the scratch rows [Kt, Krun) need room in the pol's own stride too: pols packed
      // closer than Krun rows would have them land on the next pol's first rows)
      if (!lay && (Krun > cap || out_ps < Krun * p->C)) {
        HIPCHK(p->stage_out.ensure((size_t)p->n_pol * Krun * p->C * sizeof(float2)));
        dst = p->stage_out.as<float2>();
        dps = Krun * p->C;
      }
      pfb_status st = analysis_run(p, (const float2*)in, in_ps, n_in, dst, dps, 0, Krun, K, s, nullptr, 0, 0, B,
                                   lay, 0, p->carry.as<float2>());
      if (st != PFB_OK) return st;
      if (dst != (float2*)out)
        HIPCHK(copy_pols((float2*)out, out_ps, dst, dps, Kt * p->C, p->n_pol, hipMemcpyDeviceToDevice, s));
      // carry = series[input_idat, total): all of it in the new input; into the second carry
      // buffer (the kernel just enqueued still reads the first), then swap
      const int64_t nb = total - input_idat;
      if (nb > 0) {
        HIPCHK(p->carry_next.ensure((size_t)p->n_pol * nb * sizeof(float2)));
        HIPCHK(copy_pols(p->carry_next.as<float2>(), nb, (const float2*)in + (input_idat - B), in_ps, nb, p->n_pol,
                         hipMemcpyDeviceToDevice, s));
        std::swap(p->carry, p->carry_next);
      }
      p->buffered = std::max<int64_t>(nb, 0);
      return PFB_OK;
    }
  }
  // input = cat(3, input_buffer, input)   (FilterBank.m:85-88); with nothing buffered and
  // the input already on the device the kernels read it in place (no copy)
  const float2* w;
  int64_t wps;
  const bool in_place = p->buffered == 0 && mem == PFB_MEM_DEVICE && (!sec || fus);
  if (in_place) {
    w = (const float2*)in;  // (a fused section: read through dd, `w` is not dereferenced)
    wps = in_ps;
  } else {
    dd = nullptr;
    HIPCHK(p->work.ensure((size_t)p->n_pol * std::max<int64_t>(total, 1) * sizeof(float2)));
    float2* wk = p->work.as<float2>();
    HIPCHK(copy_pols(wk, total, p->carry.as<float2>(), p->buffered, p->buffered, p->n_pol,
                     hipMemcpyDeviceToDevice, s));
    if (sec) {
      // (unpacked straight behind the carry: no second copy)
      const pfb_status st = ana_section_unpack(p, *sec, 0, n_in, wk + p->buffered, total, s);
      if (st != PFB_OK) return st;
    } else {
      HIPCHK(copy_pols(wk + p->buffered, total, (const float2*)in, in_ps, n_in, p->n_pol, kin, s));
    }
    w = wk;
    wps = total;
  }
  const int64_t K = analysis_K(p, total);
  PadConsume pad_once{&p->lowcbf_pad};
  const int64_t Kt = K - (K % p->nu);  // trim to a multiple of nu (FilterBank.m:93-104)
  if (n_out) *n_out = Kt;
  if (Kt > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                            (long long)cap, (long long)Kt);
  pad_once.accept();
  p->last_dada = dd ? PFB_DADA_INPUT_FUSED : last_dada;
  if (Kt > 0) {
    // rows are independent except for the padded variant's circular shift over all K
    // rows: the others compute just the Kt kept rows, straight into the caller's buffer
    const int64_t Krun = p->variant == pfb::kPadded ? K : Kt;
    float2* dst;
    int64_t dps;
    if (mem == PFB_MEM_HOST) {
      HIPCHK(p->stage_out.ensure((size_t)p->n_pol * Krun * p->C * sizeof(float2)));
      dst = p->stage_out.as<float2>();
      dps = Krun * p->C;
    } else {
      dst = (float2*)out;
      dps = out_ps;
      // padded: K rows computed (the circular shift spans all of them), Kt returned; they go
      // straight into the caller's buffer when it has room for K rows in the capacity and in
      // each pol's stride (rows [Kt, K) are then scratch, pfb_filterbank_execute's contract),
      // else through a staging buffer and a copy
      // (round 6: the SKA-Mid cascade's stage 2 lost a 244-us copy per call)
      // (a layout: `cap` is the Kt rows the strided entry point range-checked and out_ps is
      // the layout's; the launch writes `out` directly — a padded plan's K rows run with the
      // shifted rows [Kt, K) dropped at the store, AnalysisArgs::out_keep)
      if (!lay && (Krun > cap || out_ps < Krun * p->C)) {
        HIPCHK(p->stage_out.ensure((size_t)p->n_pol * Krun * p->C * sizeof(float2)));
        dst = p->stage_out.as<float2>();
        dps = Krun * p->C;
      }
    }
    pfb_status st = analysis_run(p, w, wps, total, dst, dps, 0, Krun, K, s, nullptr, 0, 0, 0, lay, 0, nullptr, 0,
                                 nullptr, dd, od);
    if (st != PFB_OK) return st;
    if (dst != (float2*)out) {
      const hipMemcpyKind ko = mem == PFB_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
      HIPCHK(copy_pols((float2*)out, out_ps, dst, dps, Kt * p->C, p->n_pol, ko, s));
    }
  }
  // carry = input(:,:,input_idat+1:end), input_idat = T_out N de / nu   (FilterBank.m:119-126)
  const int64_t input_idat = (Kt * p->N * p->de) / p->nu;
  const int64_t nb = total - input_idat;
  if (nb > 0) {
    HIPCHK(p->carry.ensure((size_t)p->n_pol * nb * sizeof(float2)));
    // carry may alias nothing in `work` (separate buffer); copy per pol
    if (dd) {
      // (the section's tail, unpacked: the carry stays packed cf32)
      const pfb_status st = ana_section_unpack(p, *sec, input_idat, nb, p->carry.as<float2>(), nb, s);
      if (st != PFB_OK) return st;
    } else {
      HIPCHK(copy_pols(p->carry.as<float2>(), nb, w + input_idat, wps, nb, p->n_pol,
                       hipMemcpyDeviceToDevice, s));
    }
  }
  p->buffered = std::max<int64_t>(nb, 0);
  if (mem == PFB_MEM_HOST) HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

extern "C" {

int64_t pfb_filterbank_buffered(const pfb_analysis_plan* p) { return p ? p->buffered : -1; }

pfb_status pfb_filterbank_reset(pfb_analysis_plan* p) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  p->buffered = 0;
  p->lowcbf_pad = p->variant == pfb::kLowCbf;
  return PFB_OK;
}

}  // extern "C"

// ====================================================================== synthesis plan
struct pfb_synthesis_plan {
  int device = 0;
  int N = 0, nu = 1, de = 1, Nf = 0, Ov = 0, spans = 1, combine = 1, n_pol = 1;
  int W = 0, keep = 0, L = 0, Lov = 0, Lkeep = 0, t1_lo = 0, t1_hi = 0;
  bool deripple = false;
  int chunk_blocks = 0;
  int stage1 = PFB_STAGE1_AUTO;  // pfb_synthesis_set_stage1_rows
  int last_stage1 = 0;           // pfb_synthesis_last_stage1_rows: where the last launch got its rows
  int last_dada = PFB_DADA_INPUT_NONE;  // pfb_synthesis_last_dada_input
  int last_strided = PFB_STRIDED_INPUT_NONE;  // pfb_synthesis_last_strided_input
  int last_dada_out = PFB_DADA_OUTPUT_NONE;   // pfb_synthesis_last_dada_output
  // set for the duration of a FUSED to-DADA call (synthesis_to_dada): every block launch of the
  // call stores into this section instead of its cf32 output (SynthBlockArgs::dout)
  void* dout = nullptr;
  int dout_nbit = 0;
  float dout_scale = 1.f;
  int rt_chunk_blocks = 64;  // round-trip pipeline chunk (PFB_RT_CHUNK_BLOCKS)
  int timing_mask = 0;  // PFB_TIMING_MASK (timing experiments; results invalid when set)
  int ranges = -1;  // PFB_SYNTH_RANGES: 0 one workgroup per block, -1 persistent auto, >0 persistent
  int no_reuse = 0;  // PFB_SYNTH_NO_REUSE: re-read the overlap rows (A/B measurement only)
  int xcd = 1;       // PFB_SYNTH_XCD=0: plain workgroup order (A/B measurement only)
  bool identity_perm = true;
  bool win_flat = false;  // SynthBlockArgs::win_flat
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

// PFB_STAGE1_AUTO: recomputed stage-1 rows in the Nf = 256 round trip
constexpr bool kSynthFirDefault = false;

static void zkey_clear(pfb_synthesis_plan* p) {
  p->zkey_plan = 0;
  std::fill(p->zkey, p->zkey + 5, (int64_t)-1);
  p->zkey_x = nullptr;
  p->zkey_xps = -1;
}

// the input series a synthesis recomputes its stage-1 rows from (SynthBlockArgs::fir_*)
struct FirSrc {
  const float2* x;
  int64_t x_ps, n_dat, q0;
  const float* g;
  int nu, de, pe;
};

static void hann_sym(int L, std::vector<double>& h) {
  h.resize((size_t)L);
  if (L == 1) {
    h[0] = 1.0;
    return;
  }
  for (int n = 0; n < L; ++n) h[(size_t)n] = 0.5 * (1.0 - std::cos(2.0 * M_PI * n / (L - 1)));
}

static int64_t synth_blocks(const pfb_synthesis_plan* p, int64_t n_dat) {
  const int64_t b = floordiv(n_dat - 2 * (int64_t)p->Ov, p->keep);
  return std::max<int64_t>(b, 0);
}

static pfb_status synthesis_blocks(pfb_synthesis_plan* p, const float2* Z, int64_t z_ps, int64_t b0,
                                   int64_t nb, float2* out, int64_t out_ps, int64_t out_limit,
                                   hipStream_t s, int zblk = 0, const FirSrc* fir = nullptr);
static pfb::SynthBlockArgs synth_args(const pfb_synthesis_plan* p, const float2* Z, int64_t z_ps,
                                      int64_t b0, int64_t nb, float2* out, int64_t out_ps,
                                      int64_t out_limit, int zblk = 0, const FirSrc* fir = nullptr);

// Blocks [b0, b0 + nb) with a spectral taper (pfb_spectral.hip): Matlab's order — per
// channel FFT, stitch x taper, then the L-point IFFT as row FFTs — in sub-chunks whose
// scratch stays within 2^26 values per buffer.
static pfb_status synthesis_spectral(pfb_synthesis_plan* p, const float2* in, int64_t in_ps, int64_t b0,
                                     int64_t nb, float2* out, int64_t out_ps, int64_t out_limit,
                                     hipStream_t s) {
  p->last_stage1 = PFB_STAGE1_STORED;  // (the spectral passes read the channelised rows)
  const int64_t per_block = (int64_t)p->N * std::max(p->Nf, p->W);
  const int64_t sub = std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)1 << 26) / per_block));
  const int64_t nsub = std::min(sub, nb);
  HIPCHK(p->sbuf0.ensure((size_t)nsub * per_block * sizeof(float2)));
  HIPCHK(p->sbuf1.ensure((size_t)nsub * per_block * sizeof(float2)));
  for (int64_t c0 = b0; c0 < b0 + nb; c0 += nsub) {
    pfb::SpectralArgs a{};
    a.in = in;
    a.in_pol_stride = in_ps;
    a.out = out;
    a.out_pol_stride = out_ps;
    a.out_limit = out_limit;
    a.b0 = c0;
    a.nb = std::min(nsub, b0 + nb - c0);
    a.n_pol = p->n_pol;
    a.N = p->N;
    a.Nf = p->Nf;
    a.W = p->W;
    a.keep = p->keep;
    a.L = p->L;
    a.Lov = p->Lov;
    a.Lkeep = p->Lkeep;
    a.t1_lo = p->t1_lo;
    a.t1_hi = p->t1_hi;
    a.spans = p->spans;
    a.scale = (float)((double)p->de / (double)p->nu / (double)p->L);
    a.window = p->window.as<float>();
    a.cgain = p->has_cgain ? p->cgain.as<float>() : nullptr;
    a.perm = p->identity_perm ? nullptr : p->perm.as<int>();
    a.gainj = p->gainj.as<float>();
    a.taper = p->taper.as<float>();
    a.twNf = p->twNf.as<float2>();
    a.twN = p->twN.as<float2>();
    a.twW = p->twW.as<float2>();
    a.buf0 = p->sbuf0.as<float2>();
    a.buf1 = p->sbuf1.as<float2>();
    ProfScope ps(2, (double)p->n_pol * a.nb * ((double)p->keep * p->N * 8.0 + p->Lkeep * 8.0), s, false);
    HIPCHK(pfb::launch_spectral_synth(a, s));
  }
  return PFB_OK;
}

// Blocks [b0, b0 + nb) of a call: channel IFFT of their rows into Z, then the block
// kernel.  `in` is the call's first channelised row (sample_offset applied).
// (row_shift: `in` holds the call's channelised rows from row row_shift on — a streaming
// call whose carried rows are not in front of it; blocks b0.. must not read before it.  A
// negative row_shift: block 0 starts -row_shift rows into `in` (InverseFilterBank's
// sample_offset applied to the concatenated rows))
// (dada: the call's rows are a DADA section read in place, `in` is unused — the section's
// row 0 is the call's row row_shift; strided: the same for rows behind a strided layout)
static pfb_status synthesis_chunk(pfb_synthesis_plan* p, const float2* in, int64_t in_ps, int64_t b0,
                                  int64_t nb, float2* out, int64_t out_ps, int64_t out_limit,
                                  hipStream_t s, int64_t row_shift = 0, const pfb::DadaIn* dada = nullptr,
                                  const pfb::StridedIn* strided = nullptr) {
  if (p->has_spectral) {
    if (dada || strided) return fail(PFB_ERR_UNSUPPORTED, "rows read in place with a spectral taper");
    // (a negative row shift: the blocks start -row_shift rows into `in` — a sample offset)
    if (row_shift > 0) return fail(PFB_ERR_UNSUPPORTED, "row shift with a spectral taper");
    return synthesis_spectral(p, in + (-row_shift) * p->N, in_ps, b0, nb, out, out_ps, out_limit, s);
  }
  const int64_t rows = nb * p->keep + 2 * (int64_t)p->Ov;
  zkey_clear(p);
  HIPCHK(p->Z.ensure((size_t)p->n_pol * rows * p->N * sizeof(float2)));
  float2* Z = p->Z.as<float2>();
  pfb::ChanIfftArgs c{};
  pfb::DadaIn dd{};
  pfb::StridedIn sd{};
  if (dada) {
    dd = *dada;
    dd.t0 = b0 * p->keep - row_shift;
    if (dd.t0 < 0 || dd.t0 + rows > dd.n_dat) return fail(PFB_ERR_INVALID_ARG, "rows outside the DADA section");
    c.dada = &dd;
    p->last_dada = PFB_DADA_INPUT_FUSED;
  } else if (strided) {
    sd = *strided;
    sd.t0 = b0 * p->keep - row_shift;
    if (sd.t0 < 0 || sd.t0 + rows > sd.n_dat) return fail(PFB_ERR_INVALID_ARG, "rows outside the strided input");
    c.strided = &sd;
    p->last_strided = PFB_STRIDED_INPUT_IN_PLACE;
  } else {
    c.in = in + (b0 * p->keep - row_shift) * p->N;
  }
  c.in_pol_stride = in_ps;
  c.out = Z;
  c.out_pol_stride = rows * p->N;
  c.n_rows = rows;
  c.n_pol = p->n_pol;
  c.N = p->N;
  c.perm = p->identity_perm ? nullptr : p->perm.as<int>();
  c.cgain = p->has_cgain ? p->cgain.as<float>() : nullptr;
  c.twN = p->twN.as<float2>();
  // the Nf = 256 shapes: Z in the 2-row run layout the wave kernel reads (256-B runs per
  // load instruction, as the fused round trip's analysis writes it); every other shape
  // [row][t0] for the block kernel
  const int zb = pfb::synth_wave_supported(synth_args(p, Z, rows * p->N, b0, nb, out, out_ps, out_limit, 2)) ? 2 : 0;
  c.zblk = zb ? zb : 1;
  {
    const double in_bytes = dada ? 2.0 * (dada->nbit / 8) : 8.0;
    ProfScope ps(1, (double)p->n_pol * rows * p->N * (in_bytes + 8.0), s);
    HIPCHK(pfb::launch_chan_ifft(c, s));
  }
  return synthesis_blocks(p, Z, rows * p->N, b0, nb, out, out_ps, out_limit, s, zb);
}

// Block kernel over blocks [b0, b0 + nb); Z row 0 is channelised row b0 * keep.
static pfb::SynthBlockArgs synth_args(const pfb_synthesis_plan* p, const float2* Z, int64_t z_ps,
                                      int64_t b0, int64_t nb, float2* out, int64_t out_ps,
                                      int64_t out_limit, int zblk, const FirSrc* fir) {
  pfb::SynthBlockArgs a{};
  if (fir) {
    a.fir_x = fir->x;
    a.fir_x_pol_stride = fir->x_ps;
    a.fir_n_dat = fir->n_dat;
    a.fir_g = fir->g;
    a.fir_q0 = fir->q0;
    a.fir_nu = fir->nu;
    a.fir_de = fir->de;
    a.fir_pe = fir->pe;
  }
  a.Z = Z;
  a.z_pol_stride = z_ps;
  a.out = out;
  a.out_pol_stride = out_ps;
  a.block0 = b0;
  a.n_blocks = (int)nb;
  a.n_pol = p->n_pol;
  a.N = p->N;
  a.Nf = p->Nf;
  a.W = p->W;
  a.keep = p->keep;
  a.L = p->L;
  a.Lov = p->Lov;
  a.Lkeep = p->Lkeep;
  a.t1_lo = p->t1_lo;
  a.t1_hi = p->t1_hi;
  a.scale = (float)((double)p->de / (double)p->nu / (double)p->L);
  a.window = p->window.as<float>();
  a.win_flat = p->win_flat ? 1 : 0;
  a.spans = p->spans;
  a.tw4 = p->tw4.as<float2>();
  a.tw4s = p->tw4s.as<float2>();
  a.twNf = p->twNf.as<float2>();
  a.twW = p->twW.as<float2>();
  a.out_limit = out_limit;
  a.ranges = p->ranges;
  a.no_reuse = p->no_reuse;
  a.xcd = p->xcd;
  a.timing_mask = p->timing_mask;
  a.zblk = zblk;
  a.dout = p->dout;
  a.dout_nbit = p->dout_nbit;
  a.dout_scale = p->dout_scale;
  return a;
}

static pfb_status synthesis_blocks(pfb_synthesis_plan* p, const float2* Z, int64_t z_ps, int64_t b0,
                                   int64_t nb, float2* out, int64_t out_ps, int64_t out_limit,
                                   hipStream_t s, int zblk, const FirSrc* fir) {
  const pfb::SynthBlockArgs a = synth_args(p, Z, z_ps, b0, nb, out, out_ps, out_limit, zblk, fir);
  p->last_stage1 = fir ? PFB_STAGE1_RECOMPUTED : PFB_STAGE1_STORED;
  {
    ProfScope ps(2, (double)p->n_pol * (nb * p->keep * p->N * 8.0 + nb * p->Lkeep * 8.0), s);
    HIPCHK(pfb::launch_synth_block(a, s));
  }
  return PFB_OK;
}

static int64_t synthesis_chunk_blocks(const pfb_synthesis_plan* p, int64_t B) {
  int64_t CB = p->chunk_blocks;
  if (CB <= 0) {
    // one chunk up to 2^26 channel-rows x channels (512 MB of Z); fewer, larger
    // launches measured faster than MALL-sized chunks (profiles/r01 sweep)
    const int64_t target = (int64_t)1 << 26;
    CB = std::max<int64_t>(1, target / ((int64_t)p->keep * p->N * p->n_pol));
  }
  return std::min<int64_t>(CB, B);
}

// blocks [b_lo, b_hi) in chunks (see synthesis_chunk for row_shift)
static pfb_status synthesis_range(pfb_synthesis_plan* p, const float2* in, int64_t in_ps, int64_t b_lo,
                                  int64_t b_hi, float2* out, int64_t out_ps, int64_t out_limit,
                                  hipStream_t s, int64_t row_shift = 0, const pfb::DadaIn* dada = nullptr,
                                  const pfb::StridedIn* strided = nullptr) {
  if (b_hi <= b_lo) return PFB_OK;
  const int64_t CB = synthesis_chunk_blocks(p, b_hi - b_lo);
  for (int64_t b0 = b_lo; b0 < b_hi; b0 += CB) {
    pfb_status st = synthesis_chunk(p, in, in_ps, b0, std::min<int64_t>(CB, b_hi - b0), out, out_ps,
                                    out_limit, s, row_shift, dada, strided);
    if (st != PFB_OK) return st;
  }
  return PFB_OK;
}

static pfb_status synthesis_run(pfb_synthesis_plan* p, const float2* in, int64_t in_ps, int64_t n_dat,
                                float2* out, int64_t out_ps, int64_t out_limit, hipStream_t s) {
  return synthesis_range(p, in, in_ps, 0, synth_blocks(p, n_dat), out, out_ps, out_limit, s);
}

extern "C" {

// Descriptor checks of pfb_synthesis_plan_create (no device needed)
static pfb_status synthesis_validate(const pfb_synthesis_desc* d) {
  if (!d) return fail(PFB_ERR_INVALID_ARG, "null argument");
  const int N = d->n_chan, nu = d->os_nu, de = d->os_de, Nf = d->input_fft_length,
            Ov = d->input_overlap;
  if (N <= 0 || nu <= 0 || de <= 0 || Nf <= 0 || Ov < 0 || d->n_pol <= 0)
    return fail(PFB_ERR_INVALID_ARG, "invalid synthesis parameters");
  // (sizes whose products the tables and kernels form in 32-bit ints: far beyond any
  // configuration, rejected before any arithmetic on them)
  if (N > (1 << 24) || Nf > (1 << 24) || de > (1 << 16) || nu > (1 << 16))
    return fail(PFB_ERR_UNSUPPORTED, "synthesis parameters out of range (n_chan %d, Nf %d, Ov %d, os %d/%d)",
                N, Nf, Ov, nu, de);
  if (d->n_pol > 65535)  // polarisations map to grid.y of every launch
    return fail(PFB_ERR_INVALID_ARG, "n_pol = %d exceeds 65535 series per plan", d->n_pol);
  if (((int64_t)Nf * de) % nu != 0)
    return fail(PFB_ERR_INVALID_ARG, "input_fft_length*de/nu = %d*%d/%d is not integral", Nf, de, nu);
  if (((int64_t)Ov * de * N) % nu != 0)
    return fail(PFB_ERR_INVALID_ARG, "output_overlap = Ov*de/nu*n_chan is not integral");
  if ((int64_t)Nf - 2 * (int64_t)Ov <= 0)
    return fail(PFB_ERR_INVALID_ARG, "input_keep = Nf - 2 Ov must be positive");
  const int W = (int)(((int64_t)Nf * de) / nu);
  if (W % 2 != 0) return fail(PFB_ERR_INVALID_ARG, "FN_width %d must be even", W);
  if (d->combine < 1 || N % d->combine != 0)
    return fail(PFB_ERR_INVALID_ARG, "combine=%d must divide n_chan=%d", d->combine, N);
  // spectral tapers act on the stitched L-vector (polyphase_synthesis.m:282): 'hann'
  // (PFBWindow.m:70-100, circshift(hann(L), L/2) on an L-row column) or explicit L
  // coefficients; tukey / top_hat index columns 1..Ov of that L x 1 column and have no
  // defined meaning there
  if (d->spectral_taper != PFB_WINDOW_NONE && d->spectral_taper != PFB_WINDOW_HANN &&
      d->spectral_taper != PFB_WINDOW_CUSTOM)
    return fail(PFB_ERR_INVALID_ARG,
                "spectral taper %d: only identity, hann or custom (L coefficients) act on the "
                "stitched spectrum", d->spectral_taper);
  if (d->spectral_taper == PFB_WINDOW_CUSTOM && !d->spectral_coeffs)
    return fail(PFB_ERR_INVALID_ARG, "CUSTOM spectral taper without coefficients");
  if (d->spectral_taper != PFB_WINDOW_NONE &&
      !pfb::spectral_synth_supported(Nf, (int)(((int64_t)Nf * de) / nu), N))
    return fail(PFB_ERR_UNSUPPORTED, "no spectral-taper synthesis kernels for Nf=%d n_chan=%d", Nf, N);
  if (!pfb::chan_ifft_supported(N))
    return fail(PFB_ERR_UNSUPPORTED, "no channel-IFFT kernel for n_chan=%d", N);
  if (!pfb::synth_block_supported(Nf, W))
    return fail(PFB_ERR_UNSUPPORTED, "no synthesis kernel for Nf=%d W=%d", Nf, W);
  // the block kernel's buffer descriptors span one block's output (L_keep samples), the
  // gain x twiddle table (L values) and one block's stage-1 rows (Nf x N): each must fit
  // one 32-bit descriptor extent (pfb::kRsrcMaxBytes) — rejected here, never clamped
  if ((int64_t)W * N * 8 > pfb::kRsrcMaxBytes || (int64_t)Nf * N * 8 > pfb::kRsrcMaxBytes)
    return fail(PFB_ERR_UNSUPPORTED,
                "output_fft_length %lld or Nf x n_chan %lld exceeds a buffer descriptor "
                "(%lld bytes)", (long long)W * N, (long long)Nf * N, (long long)pfb::kRsrcMaxBytes);
  if (d->temporal_taper == PFB_WINDOW_CUSTOM && !d->temporal_coeffs)
    return fail(PFB_ERR_INVALID_ARG, "CUSTOM temporal taper without coefficients");
  if (d->temporal_taper < PFB_WINDOW_NONE || d->temporal_taper > PFB_WINDOW_CUSTOM)
    return fail(PFB_ERR_INVALID_ARG, "unknown temporal taper %d", d->temporal_taper);
  if (d->apply_deripple && (!d->taps || d->n_taps <= 0))
    return fail(PFB_ERR_INVALID_ARG, "deripple requested without filter taps");
  return PFB_OK;
}

// Host-side tables of a synthesis plan (double maths, rounded once to float)
struct SynthHost {
  int N = 0, nu = 1, de = 1, Nf = 0, Ov = 0, W = 0, keep = 0, L = 0, Lov = 0, Lkeep = 0;
  int t1_lo = 0, t1_hi = 0, spans = 1, combine = 1;
  bool deripple = false, identity_perm = true, win_flat = false;
  std::vector<float> window, cgain, taper, gj;
  std::vector<int> perm;
  std::vector<float2> tw4, tw4s;
};

static void synthesis_host_tables(const pfb_synthesis_desc* d, SynthHost& p) {
  const int N = d->n_chan, nu = d->os_nu, de = d->os_de, Nf = d->input_fft_length, Ov = d->input_overlap;
  const int W = (int)(((int64_t)Nf * de) / nu);
  p.N = N;
  p.nu = nu;
  p.de = de;
  p.Nf = Nf;
  p.Ov = Ov;
  p.spans = d->spans_nyquist ? 1 : 0;
  p.combine = d->combine;
  p.W = W;
  p.keep = Nf - 2 * Ov;
  p.L = W * N;
  p.Lov = (int)(((int64_t)Ov * de * N) / nu);
  p.Lkeep = p.L - 2 * p.Lov;
  // the kernels keep y[t0 + N t1] when L_ov <= t0 + N t1 < L - L_ov (sample-exact: L_ov =
  // Ov de/nu N need not be a multiple of N — normalize(os, Ov) = 40.5 for the reference's
  // 'sps' config); [t1_lo, t1_hi) bounds the t1 that hold any kept sample
  p.t1_lo = p.Lov / N;
  p.t1_hi = W - p.t1_lo;
  p.deripple = d->apply_deripple != 0;

  // temporal taper (PFBWindow.m) -> per-time window + per-channel gain (hann quirk)
  std::vector<float>& window = p.window;
  window.assign((size_t)Nf, 1.f);
  switch (d->temporal_taper) {
    case PFB_WINDOW_NONE: break;
    case PFB_WINDOW_TUKEY: {
      std::vector<double> h;
      hann_sym(2 * Ov, h);
      for (int t = 0; t < Ov; ++t) window[(size_t)t] = (float)h[(size_t)t];
      for (int t = 0; t < Ov; ++t) window[(size_t)(Nf - Ov + t)] = (float)h[(size_t)(Ov + t)];
      break;
    }
    case PFB_WINDOW_TOP_HAT:
      for (int t = 0; t < Ov; ++t) {
        window[(size_t)t] = 0.f;
        window[(size_t)(Nf - 1 - t)] = 0.f;
      }
      break;
    case PFB_WINDOW_HANN: {
      // PFBWindow.m:72-99: hann along dim 1 = channels; circshift when n_chan != Nf
      std::vector<double> h;
      hann_sym(N, h);
      p.cgain.resize((size_t)N);
      for (int c = 0; c < N; ++c) {
        const int src = (N != Nf) ? ((c - N / 2) % N + N) % N : c;
        p.cgain[(size_t)c] = (float)h[(size_t)src];
      }
      break;
    }
    case PFB_WINDOW_CUSTOM:
      for (int t = 0; t < Nf; ++t) window[(size_t)t] = (float)d->temporal_coeffs[t];
      break;
    default: break;  // rejected by synthesis_validate
  }

  // combine permutation (polyphase_synthesis.m:198-239): slot chan <- input jchan
  std::vector<int>& perm = p.perm;
  perm.resize((size_t)N);
  for (int c = 0; c < N; ++c) perm[(size_t)c] = c;
  if (p.combine > 1) {
    const int fcc = N / p.combine, fco = N;
    for (int chan = 0; chan < N; ++chan) {
      int fine = (chan + fcc / 2) % fco;
      int coarse = fine / fcc;
      fine -= coarse * fcc;
      coarse = (coarse + p.combine / 2) % p.combine;
      fine = (fine + fcc / 2) % fcc;
      perm[(size_t)chan] = coarse * fcc + fine;
    }
  }
  for (int c = 0; c < N; ++c)
    if (perm[(size_t)c] != c) p.identity_perm = false;

  // kept-bin tables (see oracle.synthesis_tables and DESIGN.md)
  const int W2 = W / 2, d2 = (Nf - W) / 2;
  std::vector<double> g(W2 + 1, 1.0);
  if (p.deripple) {
    // H0 = freqz(h, 1, n), n = N*W/2; filter_response = 1/|H0(0..W/2)|  (:138-150)
    const int64_t nfz = (int64_t)N * W2;
    const int64_t two_n = 2 * nfz;
    for (int k = 0; k <= W2; ++k) {
      double re = 0.0, im = 0.0;
      for (int64_t i = 0; i < d->n_taps; ++i) {
        const int64_t m = ((int64_t)k * i) % two_n;  // angle = pi k i / n = 2 pi m / (2n)
        const double a = 2.0 * M_PI * (double)m / (double)two_n;
        re += d->taps[i] * std::cos(a);
        im -= d->taps[i] * std::sin(a);
      }
      g[(size_t)k] = 1.0 / std::sqrt(re * re + im * im);
    }
  }
  std::vector<int> src((size_t)W), expo((size_t)W);
  std::vector<double> gain((size_t)W);
  for (int jp = 0; jp < W; ++jp) {
    int j, e;
    if (p.spans) {
      j = (jp + W2) % W;
      e = (jp < W2) ? jp : jp - W;
    } else {
      j = jp;
      e = jp;
    }
    src[(size_t)jp] = (d2 + j + Nf / 2) % Nf;
    expo[(size_t)jp] = e;
    gain[(size_t)jp] = (j < W2) ? g[(size_t)(W2 - j)] : g[(size_t)(j - W2)];
  }
  // the rows the wave synthesis kernels treat as flat: [48, 208) at Nf 256, [128, 384) at 512
  p.win_flat = (Nf == 256 || Nf == 512) &&
               std::all_of(window.begin() + (Nf == 256 ? 48 : 128), window.begin() + (Nf == 256 ? 208 : 384),
                           [](float w) { return w == 1.f; });
  // four-step twiddle x deripple gain, laid out [j'][t0] (coalesced in the block kernel)
  p.tw4.resize((size_t)N * W);
  p.tw4s.resize((size_t)N * W);
  const double oscale = (double)p.de / (double)p.nu / (double)p.L;
  for (int t0 = 0; t0 < N; ++t0) {
    for (int jp = 0; jp < W; ++jp) {
      int64_t m = ((int64_t)t0 * expo[(size_t)jp]) % p.L;
      if (m < 0) m += p.L;
      if (2 * m > p.L) m -= p.L;
      const double ang = 2.0 * M_PI * (double)m / (double)p.L;
      const double gj = gain[(size_t)jp];
      p.tw4[(size_t)jp * N + t0] = make_float2((float)(gj * std::cos(ang)), (float)(gj * std::sin(ang)));
      p.tw4s[(size_t)jp * N + t0] =
          make_float2((float)(oscale * gj * std::cos(ang)), (float)(oscale * gj * std::sin(ang)));
    }
  }
  if (d->spectral_taper != PFB_WINDOW_NONE) {
    p.taper.resize((size_t)p.L);
    if (d->spectral_taper == PFB_WINDOW_HANN) {
      // hann(L) circularly shifted by L/2 (PFBWindow.m:83-95: ndat = L != Nf)
      std::vector<double> h;
      hann_sym(p.L, h);
      for (int i = 0; i < p.L; ++i) p.taper[(size_t)i] = (float)h[(size_t)((i - p.L / 2 + p.L) % p.L)];
    } else {
      for (int i = 0; i < p.L; ++i) p.taper[(size_t)i] = (float)d->spectral_coeffs[i];
    }
    // deripple gains in Matlab's FN row order j (polyphase_synthesis.m:244-250)
    p.gj.resize((size_t)W);
    for (int j = 0; j < W; ++j) p.gj[(size_t)j] = (float)((j < W2) ? g[(size_t)(W2 - j)] : g[(size_t)(j - W2)]);
  }
}

static void synthesis_release(pfb_synthesis_plan* p) {
  for (DevBuf* b : {&p->window, &p->tw4, &p->tw4s, &p->twN, &p->twNf, &p->twW, &p->perm, &p->cgain,
                    &p->taper, &p->gainj, &p->sbuf0, &p->sbuf1, &p->Z, &p->carry, &p->work,
                    &p->stage_in, &p->stage_out})
    b->release();
}

pfb_status pfb_synthesis_plan_validate(const pfb_synthesis_desc* d) {
  const pfb_status st = synthesis_validate(d);
  if (st != PFB_OK) return st;
  SynthHost h;
  synthesis_host_tables(d, h);
  return PFB_OK;
}

pfb_status pfb_synthesis_plan_create(const pfb_synthesis_desc* d, pfb_synthesis_plan** out) {
  if (!d || !out) return fail(PFB_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const pfb_status vst = synthesis_validate(d);
  if (vst != PFB_OK) return vst;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PFB_ERR_NO_DEVICE, "no HIP device available");
  if (d->device < 0 || d->device >= ndev)
    return fail(PFB_ERR_INVALID_ARG, "device %d out of range", d->device);
  HIPCHK(hipSetDevice(d->device));

  SynthHost h;
  synthesis_host_tables(d, h);
  auto* p = new pfb_synthesis_plan();
  p->device = d->device;
  if (const char* v = pfb::knob("PFB_SYNTH_RANGES")) p->ranges = std::max(-1, std::atoi(v));
  if (const char* v = pfb::knob("PFB_TIMING_MASK")) p->timing_mask = std::atoi(v);
  if (const char* v = pfb::knob("PFB_SYNTH_NO_REUSE")) p->no_reuse = std::atoi(v) != 0;
  if (const char* v = pfb::knob("PFB_SYNTH_XCD")) p->xcd = std::atoi(v) != 0;
  if (const char* v = pfb::knob("PFB_RT_CHUNK_BLOCKS")) p->rt_chunk_blocks = std::max(1, std::atoi(v));
  p->N = h.N;
  p->nu = h.nu;
  p->de = h.de;
  p->Nf = h.Nf;
  p->Ov = h.Ov;
  p->spans = h.spans;
  p->combine = h.combine;
  p->n_pol = d->n_pol;
  p->W = h.W;
  p->keep = h.keep;
  p->L = h.L;
  p->Lov = h.Lov;
  p->Lkeep = h.Lkeep;
  p->t1_lo = h.t1_lo;
  p->t1_hi = h.t1_hi;
  p->deripple = h.deripple;
  p->identity_perm = h.identity_perm;
  p->win_flat = h.win_flat;
  hipError_t e = upload(p->window, h.window);
  if (e == hipSuccess) e = upload(p->tw4, h.tw4);
  if (e == hipSuccess) e = upload(p->tw4s, h.tw4s);
  if (e == hipSuccess) e = upload(p->perm, h.perm);
  if (e == hipSuccess && !h.cgain.empty()) {
    e = upload(p->cgain, h.cgain);
    p->has_cgain = true;
  }
  if (e == hipSuccess) e = upload(p->twN, twiddles(h.N, -1));
  if (e == hipSuccess) e = upload(p->twNf, twiddles(h.Nf, -1));
  if (e == hipSuccess) e = upload(p->twW, twiddles(h.W, -1));
  if (e == hipSuccess && d->spectral_taper != PFB_WINDOW_NONE) {
    p->has_spectral = true;
    e = upload(p->taper, h.taper);
    if (e == hipSuccess) e = upload(p->gainj, h.gj);
  }
  if (e != hipSuccess) {
    synthesis_release(p);
    delete p;
    return fail(PFB_ERR_HIP, "synthesis plan upload: %s", hipGetErrorString(e));
  }
  *out = p;
  return PFB_OK;
}

pfb_status pfb_synthesis_plan_destroy(pfb_synthesis_plan* p) {
  if (!p) return PFB_OK;
  (void)hipSetDevice(p->device);
  synthesis_release(p);
  delete p;
  return PFB_OK;
}

int64_t pfb_synthesis_output_length(const pfb_synthesis_plan* p, int64_t n_dat) {
  if (!p) return -1;
  return synth_blocks(p, n_dat) * p->Lkeep;
}

pfb_status pfb_synthesis_set_stage1_rows(pfb_synthesis_plan* p, int32_t mode) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (mode != PFB_STAGE1_AUTO && mode != PFB_STAGE1_STORED && mode != PFB_STAGE1_RECOMPUTED)
    return fail(PFB_ERR_INVALID_ARG, "unknown stage-1 row mode %d", mode);
  p->stage1 = mode;
  zkey_clear(p);  // a split round trip in flight is not continued under another mode
  return PFB_OK;
}

int32_t pfb_synthesis_last_stage1_rows(const pfb_synthesis_plan* p) { return p ? p->last_stage1 : -1; }

pfb_status pfb_synthesis_set_chunk_blocks(pfb_synthesis_plan* p, int32_t blocks) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  p->chunk_blocks = std::max(0, blocks);
  return PFB_OK;
}

// A DADA data section as the input of a synthesis call (pfb_synthesis_execute_dada,
// pfb_inverse_filterbank_execute_dada): rows x the plan's n_chan x n_pol x ndim values of nbit
struct DadaSection {
  const void* base;
  int nbit, ndim, order;
};

static pfb_status dada_section_check(const pfb_synthesis_plan* p, const DadaSection& sec, int64_t rows) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (sec.nbit != 8 && sec.nbit != 16 && sec.nbit != 32 && sec.nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "NBIT must be 8, 16, 32 or 64");
  if (sec.ndim != 1 && sec.ndim != 2) return fail(PFB_ERR_INVALID_ARG, "NDIM must be 1 or 2");
  if (sec.order != PFB_DADA_TFP && sec.order != PFB_DADA_LOWCBF)
    return fail(PFB_ERR_INVALID_ARG, "unknown sample order");
  if (sec.order == PFB_DADA_LOWCBF && rows > 0 && rows % 32)
    return fail(PFB_ERR_INVALID_ARG, "LowCBF data are heaps of 32 samples");
  return PFB_OK;
}

// the channel IFFT can read the section in place (pfb_api.h, FUSED)
static bool dada_fusable(const pfb_synthesis_plan* p, const DadaSection& sec) {
  return sec.ndim == 2 && pfb::chan_ifft_dada_supported(p->N, sec.nbit) && p->identity_perm && !p->has_cgain &&
         !p->has_spectral && reinterpret_cast<uintptr_t>(sec.base) % (size_t)(sec.nbit / 4) == 0;
}

// STAGED: the section's `rows` rows unpacked into the plan's staging buffer ([pol][row][chan],
// pol stride rows N)
static pfb_status dada_stage(pfb_synthesis_plan* p, const DadaSection& sec, int64_t rows, hipStream_t s) {
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * std::max<int64_t>(rows, 1) * p->N * sizeof(float2)));
  p->last_dada = PFB_DADA_INPUT_STAGED;
  return pfb_dada_unpack(sec.base, sec.nbit, sec.ndim, sec.order, rows, p->N, p->n_pol,
                         reinterpret_cast<pfb_cf32*>(p->stage_in.p), rows * p->N, s);
}

// The layout of a strided cf32 input (pfb_synthesis_execute_strided,
// pfb_inverse_filterbank_execute_strided): element (pol, row, chan) at in[pol ps + row rs +
// chan cs], `cap` elements available from `in`
struct StridedView {
  int64_t ps, rs, cs, cap;
};

// every stride positive and the furthest element read inside the capacity (pfb_api.h)
static pfb_status strided_view_check(const pfb_synthesis_plan* p, const StridedView& v, int64_t rows) {
  if (v.ps <= 0 || v.rs <= 0 || v.cs <= 0) return fail(PFB_ERR_INVALID_ARG, "input strides must be positive");
  if (rows <= 0) return PFB_OK;
  const __int128 far = (__int128)(p->n_pol - 1) * v.ps + (__int128)(rows - 1) * v.rs + (__int128)(p->N - 1) * v.cs;
  if (far >= (__int128)v.cap)
    return fail(PFB_ERR_INVALID_ARG, "in_capacity %lld does not cover the furthest element read",
                (long long)v.cap);
  return PFB_OK;
}

// the channel IFFT can read the rows through the layout (pfb_api.h, IN_PLACE)
static bool strided_in_place(const pfb_synthesis_plan* p) {
  return pfb::chan_ifft_strided_supported(p->N) && !p->has_cgain && !p->has_spectral;
}

// STAGED: `rows` rows copied through the layout into the plan's staging buffer
// ([pol][row][chan], pol stride rows N)
static pfb_status strided_stage(pfb_synthesis_plan* p, const pfb::StridedIn& d, int64_t rows, hipStream_t s) {
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * std::max<int64_t>(rows, 1) * p->N * sizeof(float2)));
  p->last_strided = PFB_STRIDED_INPUT_STAGED;
  HIPCHK(pfb::launch_strided_rows_copy(d, rows, p->N, p->n_pol, p->stage_in.as<float2>(), rows * p->N, s));
  return PFB_OK;
}

// pfb_synthesis_execute; sec: the rows are a DADA section (device memory) instead of `in`;
// sv: `in` is read through a strided layout (device memory)
static pfb_status synthesis_exec(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                 const DadaSection* sec, int64_t n_dat, int64_t sample_offset,
                                 pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                                 int32_t mem, void* stream, const StridedView* sv = nullptr) {
  if (sec) in = static_cast<const pfb_cf32*>(sec->base);
  if (!p || (!in && n_dat > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (sample_offset < 1) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 1-based (>= 1)");
  if (n_dat < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_dat");
  if (sv) {
    const pfb_status st = strided_view_check(p, *sv, n_dat);
    if (st != PFB_OK) return st;
  }
  HIPCHK(hipSetDevice(p->device));
  p->last_dada = PFB_DADA_INPUT_NONE;
  p->last_strided = PFB_STRIDED_INPUT_NONE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t off = std::min<int64_t>(sample_offset - 1, std::max<int64_t>(n_dat, 0));
  const int64_t n = n_dat - off;  // in = in(:, :, sample_offset:end)  (:99)
  const int64_t olen = synth_blocks(p, n) * p->Lkeep;
  if (n_out) *n_out = olen;
  if (olen == 0) return PFB_OK;
  if (!out) return fail(PFB_ERR_INVALID_ARG, "null output");
  if (cap < olen) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld",
                              (long long)cap, (long long)olen);
  if (mem == PFB_MEM_DEVICE) {
    if ((!sec && !sv && in_ps < n_dat * p->N) || out_ps < olen)
      return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
    if (sv) {
      const pfb::StridedIn d{(const float2*)in, sv->ps, sv->rs, sv->cs, n_dat, 0};
      if (strided_in_place(p))
        // the blocks start `off` rows into the layout (a negative row shift)
        return synthesis_range(p, nullptr, 0, 0, synth_blocks(p, n), (float2*)out, out_ps, olen, s, -off, nullptr,
                               &d);
      const pfb_status st = strided_stage(p, d, n_dat, s);
      if (st != PFB_OK) return st;
      in = reinterpret_cast<const pfb_cf32*>(p->stage_in.p);
      in_ps = n_dat * p->N;
    }
    if (sec) {
      if (dada_fusable(p, *sec)) {
        // the blocks start `off` rows into the section (a negative row shift)
        const pfb::DadaIn d{sec->base, sec->nbit, sec->order == PFB_DADA_LOWCBF, n_dat, 0};
        return synthesis_range(p, nullptr, 0, 0, synth_blocks(p, n), (float2*)out, out_ps, olen, s, -off, &d);
      }
      const pfb_status st = dada_stage(p, *sec, n_dat, s);
      if (st != PFB_OK) return st;
      in = reinterpret_cast<const pfb_cf32*>(p->stage_in.p);
      in_ps = n_dat * p->N;
    }
    return synthesis_run(p, (const float2*)in + off * p->N, in_ps, n, (float2*)out, out_ps, olen, s);
  }
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n * p->N * sizeof(float2)));
  HIPCHK(p->stage_out.ensure((size_t)p->n_pol * olen * sizeof(float2)));
  HIPCHK(copy_pols(p->stage_in.as<float2>(), n * p->N, (const float2*)in + off * p->N, in_ps,
                   n * p->N, p->n_pol, hipMemcpyHostToDevice, s));
  pfb_status st = synthesis_run(p, p->stage_in.as<float2>(), n * p->N, n, p->stage_out.as<float2>(),
                                olen, olen, s);
  if (st != PFB_OK) return st;
  HIPCHK(copy_pols((float2*)out, out_ps, p->stage_out.as<float2>(), olen, olen, p->n_pol,
                   hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

// a cf32-output call that went through: pfb_synthesis_last_dada_output reports NONE again
static pfb_status cf32_output(pfb_synthesis_plan* p, pfb_status st) {
  if (p && st == PFB_OK) p->last_dada_out = PFB_DADA_OUTPUT_NONE;
  return st;
}

pfb_status pfb_synthesis_execute(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                 int64_t n_dat, int64_t sample_offset, pfb_cf32* out,
                                 int64_t out_ps, int64_t cap, int64_t* n_out, int32_t mem,
                                 void* stream) {
  return cf32_output(
      p, synthesis_exec(p, in, in_ps, nullptr, n_dat, sample_offset, out, out_ps, cap, n_out, mem, stream));
}

pfb_status pfb_synthesis_execute_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                      int32_t order, int64_t n_dat, int64_t sample_offset, pfb_cf32* out,
                                      int64_t out_ps, int64_t cap, int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = dada_section_check(p, sec, n_dat);
  if (st != PFB_OK) return st;
  return cf32_output(p, synthesis_exec(p, nullptr, 0, &sec, n_dat, sample_offset, out, out_ps, cap, n_out,
                                       PFB_MEM_DEVICE, stream));
}

int32_t pfb_synthesis_last_dada_input(const pfb_synthesis_plan* p) { return p ? p->last_dada : -1; }

pfb_status pfb_synthesis_execute_strided(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                         int64_t in_rs, int64_t in_cs, int64_t in_cap, int64_t n_dat,
                                         int64_t sample_offset, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                         int64_t* n_out, void* stream) {
  const StridedView sv{in_ps, in_rs, in_cs, in_cap};
  return cf32_output(p, synthesis_exec(p, in, in_ps, nullptr, n_dat, sample_offset, out, out_ps, cap, n_out,
                                       PFB_MEM_DEVICE, stream, &sv));
}

int32_t pfb_synthesis_last_strided_input(const pfb_synthesis_plan* p) { return p ? p->last_strided : -1; }

pfb_status pfb_inverse_filterbank_set_sample_offset(pfb_synthesis_plan* p, int64_t sample_offset) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (sample_offset < 0) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 0-based (>= 0)");
  p->ifb_offset = sample_offset;
  return PFB_OK;
}

// InverseFilterBank.m:73-135.  Every call runs polyphase_synthesis on the concatenated
// rows (carry + input) from row `so` = sample_offset on (:92-96, `sample_offset+1`), and the
// carry starts at input_idat = (output length) nu / (n_chan de) = B keep of the
// concatenation — not offset by `so`: the next call skips `so` rows of it again, so
// consecutive calls see the blocks of one continuous run.
// (sec: the new rows are a DADA section in device memory instead of `in`.  Fusable: the
// blocks of new rows read it in place, and whatever the cf32 call copies out of `in` — the
// stitched head, the carry — is unpacked from the section's rows instead.  Otherwise the
// section is unpacked whole once every check has passed, and the cf32 path runs.)
// (sv: the new rows lie behind a strided layout in device memory.  The same split: the
// blocks of new rows read through the layout where the channel IFFT can, the stitched head
// and the carry are copied out of it by the strided-rows copy kernel; otherwise the rows are
// copied whole once every check has passed, and the cf32 path runs.)
// The lengths of a stream call of n_in new rows on the plan's current state
struct IfbLens {
  int64_t total, so, B, input_idat, buffered, olen;
};
static IfbLens ifb_lens(const pfb_synthesis_plan* p, int64_t n_in) {
  IfbLens l{};
  l.total = p->buffered + n_in;
  l.so = std::min(p->ifb_offset, l.total);  // in(:, :, sample_offset:end)
  // output length and carry-over rounded up to a multiple of nu (InverseFilterBank.m:104-135)
  l.B = synth_blocks(p, l.total - l.so);
  const int64_t full = l.B * p->Lkeep;
  l.input_idat = l.B * p->keep;
  l.buffered = l.total - l.input_idat;
  l.olen = full;
  const int64_t rem = ((l.buffered % p->nu) + p->nu) % p->nu;
  if (rem != 0) {
    l.buffered += p->nu - rem;
    l.input_idat = l.total - l.buffered;
    // output_ndat = input_idat * (n_chan de)/nu, used as a Matlab colon end (floor)
    l.olen = std::min(std::max<int64_t>(0, floordiv(l.input_idat * p->N * p->de, p->nu)), full);
  }
  return l;
}

static pfb_status ifb_exec(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps, const DadaSection* sec,
                           int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                           int32_t mem, void* stream, const StridedView* sv = nullptr) {
  if (sec) in = static_cast<const pfb_cf32*>(sec->base);
  if (!p || (!in && n_in > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n_in < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_in");
  if (sv) {
    const pfb_status st = strided_view_check(p, *sv, n_in);
    if (st != PFB_OK) return st;
  }
  HIPCHK(hipSetDevice(p->device));
  p->last_dada = PFB_DADA_INPUT_NONE;
  p->last_strided = PFB_STRIDED_INPUT_NONE;
  hipStream_t s = (hipStream_t)stream;
  const int N = p->N;
  const hipMemcpyKind kin = mem == PFB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const IfbLens len = ifb_lens(p, n_in);
  const int64_t total = len.total, so = len.so, B = len.B, input_idat = len.input_idat, buffered = len.buffered,
                olen = len.olen;
  if (input_idat < 0)
    // no complete block and a carry rounded up past the data: InverseFilterBank.m:104-122
    // would index input(:, :, input_idat + 1 : end) before the first sample (its rounding
    // loop never settles); the call is rejected and the object state is left unchanged
    return fail(PFB_ERR_INVALID_ARG,
                "InverseFilterBank: %lld buffered + %lld new rows hold no complete block and "
                "round the carry past the data (InverseFilterBank.m:104-122); pass more rows",
                (long long)p->buffered, (long long)n_in);
  if (n_out) *n_out = olen;
  if (olen > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld",
                              (long long)cap, (long long)olen);
  if (mem == PFB_MEM_DEVICE && ((!sec && !sv && in_ps < n_in * N) || out_ps < olen))
    return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  if (olen > 0 && !out) return fail(PFB_ERR_INVALID_ARG, "null output");
  pfb::DadaIn dd{};
  const pfb::DadaIn* dada = nullptr;
  pfb::StridedIn sd{};
  const pfb::StridedIn* strided = nullptr;
  if (sv) {
    sd = pfb::StridedIn{(const float2*)in, sv->ps, sv->rs, sv->cs, n_in, 0};
    if (strided_in_place(p)) {
      strided = &sd;
      in = nullptr;
    } else {
      const pfb_status st = strided_stage(p, sd, n_in, s);
      if (st != PFB_OK) return st;
      in = reinterpret_cast<const pfb_cf32*>(p->stage_in.p);
      in_ps = n_in * N;
    }
  }
  if (sec) {
    if (dada_fusable(p, *sec)) {
      dd = pfb::DadaIn{sec->base, sec->nbit, sec->order == PFB_DADA_LOWCBF, n_in, 0};
      dada = &dd;
      in = nullptr;
    } else {
      const pfb_status st = dada_stage(p, *sec, n_in, s);
      if (st != PFB_OK) return st;
      in = reinterpret_cast<const pfb_cf32*>(p->stage_in.p);
      in_ps = n_in * N;
    }
  }
  // rows [row0, row0 + n) of the new input -> dst[pol][0, n N)
  auto rows_to = [&](float2* dst, int64_t dps, int64_t row0, int64_t n) -> hipError_t {
    if (dada) {
      pfb::DadaIn d = dd;
      d.t0 = row0;
      if (p->last_dada == PFB_DADA_INPUT_NONE) p->last_dada = PFB_DADA_INPUT_STAGED;
      return pfb::launch_dada_unpack_rows(d, n, N, p->n_pol, dst, dps, s);
    }
    if (strided) {
      pfb::StridedIn d = sd;
      d.t0 = row0;
      if (p->last_strided == PFB_STRIDED_INPUT_NONE) p->last_strided = PFB_STRIDED_INPUT_STAGED;
      return pfb::launch_strided_rows_copy(d, n, N, p->n_pol, dst, dps, s);
    }
    return copy_pols(dst, dps, (const float2*)in + row0 * N, in_ps, n * N, p->n_pol, kin, s);
  };
  {
    // Carry without the concatenation copy: blocks whose rows start at or after the
    // carried Bc rows read the new input in place (row shift Bc - so), the first ones a
    // small stitched buffer; same blocks, same kernels as the concatenated run.
    const int64_t Bc = p->buffered;
    static const bool no_split = pfb::knob("PFB_FB_NO_SPLIT") != nullptr;  // A/B
    if (!no_split && mem == PFB_MEM_DEVICE && Bc > 0 && !p->has_spectral && input_idat >= Bc) {
      if (olen > 0) {
        // first block starting at or after row Bc of the concatenation: so + b keep >= Bc
        const int64_t b_s = std::min(B, std::max<int64_t>(0, (Bc - so + p->keep - 1) / p->keep));
        if (b_s > 0) {
          const int64_t L = std::min(total, so + (b_s - 1) * p->keep + p->Nf);
          HIPCHK(p->work.ensure((size_t)p->n_pol * L * N * sizeof(float2)));
          float2* wk = p->work.as<float2>();
          HIPCHK(copy_pols(wk, L * N, p->carry.as<float2>(), Bc * N, std::min(Bc, L) * N, p->n_pol,
                           hipMemcpyDeviceToDevice, s));
          if (L > Bc) HIPCHK(rows_to(wk + Bc * N, L * N, 0, L - Bc));
          pfb_status st = synthesis_range(p, wk, L * N, 0, b_s, (float2*)out, out_ps, olen, s, -so);
          if (st != PFB_OK) return st;
        }
        pfb_status st = synthesis_range(p, (const float2*)in, in_ps, b_s, B, (float2*)out, out_ps, olen, s,
                                        Bc - so, dada, strided);
        if (st != PFB_OK) return st;
      }
      if (buffered > 0) {
        HIPCHK(p->carry.ensure((size_t)p->n_pol * buffered * N * sizeof(float2)));
        HIPCHK(rows_to(p->carry.as<float2>(), buffered * N, input_idat - Bc, buffered));
      }
      p->buffered = std::max<int64_t>(buffered, 0);
      return PFB_OK;
    }
  }
  // input = cat(3, input_buffer, input); read in place when nothing is buffered
  const float2* w;
  int64_t wps;
  if (p->buffered == 0 && mem == PFB_MEM_DEVICE) {
    w = (const float2*)in;
    wps = in_ps;
    if (dada || strided) {
      // nothing carried: every block reads the section (the layout) in place, the carry is
      // its unpacked (copied) tail
      if (olen > 0) {
        pfb_status st = synthesis_range(p, nullptr, 0, 0, B, (float2*)out, out_ps, olen, s, -so, dada, strided);
        if (st != PFB_OK) return st;
      }
      if (buffered > 0) {
        HIPCHK(p->carry.ensure((size_t)p->n_pol * buffered * N * sizeof(float2)));
        HIPCHK(rows_to(p->carry.as<float2>(), buffered * N, input_idat, buffered));
      }
      p->buffered = std::max<int64_t>(buffered, 0);
      return PFB_OK;
    }
  } else {
    HIPCHK(p->work.ensure((size_t)p->n_pol * std::max<int64_t>(total, 1) * N * sizeof(float2)));
    float2* wk = p->work.as<float2>();
    HIPCHK(copy_pols(wk, total * N, p->carry.as<float2>(), p->buffered * N, p->buffered * N, p->n_pol,
                     hipMemcpyDeviceToDevice, s));
    HIPCHK(rows_to(wk + p->buffered * N, total * N, 0, n_in));
    w = wk;
    wps = total * N;
  }
  if (olen > 0) {
    if (mem == PFB_MEM_HOST) {
      HIPCHK(p->stage_out.ensure((size_t)p->n_pol * olen * sizeof(float2)));
      pfb_status st = synthesis_range(p, w, wps, 0, B, p->stage_out.as<float2>(), olen, olen, s, -so);
      if (st != PFB_OK) return st;
      HIPCHK(copy_pols((float2*)out, out_ps, p->stage_out.as<float2>(), olen, olen, p->n_pol,
                       hipMemcpyDeviceToHost, s));
    } else {
      pfb_status st = synthesis_range(p, w, wps, 0, B, (float2*)out, out_ps, olen, s, -so);
      if (st != PFB_OK) return st;
    }
  }
  if (buffered > 0) {
    HIPCHK(p->carry.ensure((size_t)p->n_pol * buffered * N * sizeof(float2)));
    HIPCHK(copy_pols(p->carry.as<float2>(), buffered * N, w + input_idat * N, wps, buffered * N,
                     p->n_pol, hipMemcpyDeviceToDevice, s));
  }
  p->buffered = std::max<int64_t>(buffered, 0);
  if (mem == PFB_MEM_HOST) HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

pfb_status pfb_inverse_filterbank_execute(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                          int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                          int64_t* n_out, int32_t mem, void* stream) {
  return cf32_output(p, ifb_exec(p, in, in_ps, nullptr, n_in, out, out_ps, cap, n_out, mem, stream));
}

pfb_status pfb_inverse_filterbank_execute_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit,
                                               int32_t ndim, int32_t order, int64_t n_in, pfb_cf32* out,
                                               int64_t out_ps, int64_t cap, int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = dada_section_check(p, sec, n_in);
  if (st != PFB_OK) return st;
  return cf32_output(p, ifb_exec(p, nullptr, 0, &sec, n_in, out, out_ps, cap, n_out, PFB_MEM_DEVICE, stream));
}

pfb_status pfb_inverse_filterbank_execute_strided(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                  int64_t in_rs, int64_t in_cs, int64_t in_cap, int64_t n_in,
                                                  pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                                                  void* stream) {
  const StridedView sv{in_ps, in_rs, in_cs, in_cap};
  return cf32_output(p, ifb_exec(p, in, in_ps, nullptr, n_in, out, out_ps, cap, n_out, PFB_MEM_DEVICE, stream, &sv));
}

// the wave kernel stores such a section itself (pfb_api.h, FUSED).  Every (polarisations, NBIT)
// cell stays FUSED: on the C2 synthesis unit each takes 0.49-0.73 of the time of the pair
// (execute, scale, pfb_dada_pack), the gap 0.085-0.177 ms against a run-to-run spread of the
// pair of at most 0.006 ms — cf32 rows into NBIT 8 / 16 / 32: one polarisation 0.115 / 0.119 /
// 0.129 against 0.211 / 0.220 / 0.227 ms, two 0.229 / 0.253 / 0.320 against 0.406 / 0.420 /
// 0.436 ms (the narrowest cell, 0.73); from an NBIT 16 section 0.099 / 0.099 / 0.100 against
// 0.198 / 0.184 / 0.205 and 0.202 / 0.220 / 0.284 against 0.378 / 0.391 / 0.409 ms
// (profiles/dada_synthesis_output_ab.jsonl)
static bool synthesis_dada_out_fusable(const pfb_synthesis_plan* p, const void* out, int nbit) {
  if (nbit != 8 && nbit != 16 && nbit != 32) return false;
  if (p->has_spectral || reinterpret_cast<uintptr_t>(out) % (size_t)(nbit / 4) != 0) return false;
  // (the stage-1 row layout synthesis_chunk picks for the wave kernel: 2-row runs)
  return pfb::synth_wave_dadaout_supported(synth_args(p, nullptr, 0, 0, 1, nullptr, 0, 0, 2), nbit);
}

// The to-DADA calls (pfb_api.h): every check here — the callee's own, in its order, among
// them — before the callee launches or changes the stream state; then FUSED — the plan's block
// launches store the section (pfb_synthesis_plan::dout) — or STAGED — the cf32 path into the
// plan's buffer and the scaled pack launch.
static pfb_status synthesis_to_dada(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                    const DadaSection* sec, int64_t n, int64_t sample_offset, void* out,
                                    int32_t nbit, float scale, int64_t cap_bytes, int64_t* n_out, void* stream,
                                    bool stream_call) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (nbit != 8 && nbit != 16 && nbit != 32 && nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "output NBIT must be 8, 16, 32 or 64");
  if (!std::isfinite(scale)) return fail(PFB_ERR_INVALID_ARG, "output scale is not finite");
  if (reinterpret_cast<uintptr_t>(out) % (size_t)(nbit / 8) != 0)
    return fail(PFB_ERR_INVALID_ARG, "output section not aligned to its NBIT");
  // the input-side conditions of the corresponding cf32-output call
  if (sec) {
    const pfb_status st = dada_section_check(p, *sec, n);
    if (st != PFB_OK) return st;
  }
  if (!(sec ? sec->base : (const void*)in) && n > 0) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (!stream_call && sample_offset < 1) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 1-based (>= 1)");
  if (n < 0) return fail(PFB_ERR_INVALID_ARG, "negative row count");
  int64_t olen;
  if (stream_call) {
    const IfbLens len = ifb_lens(p, n);
    if (len.input_idat < 0)
      return fail(PFB_ERR_INVALID_ARG,
                  "InverseFilterBank: %lld buffered + %lld new rows hold no complete block and "
                  "round the carry past the data (InverseFilterBank.m:104-122); pass more rows",
                  (long long)p->buffered, (long long)n);
    olen = len.olen;
  } else {
    const int64_t off = std::min<int64_t>(sample_offset - 1, n);
    olen = synth_blocks(p, n - off) * p->Lkeep;
  }
  if (n_out) *n_out = olen;
  const int64_t need = olen * p->n_pol * 2 * (nbit / 8);
  if (stream_call) {  // (pfb_inverse_filterbank_execute's order)
    if (cap_bytes < need)
      return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld bytes", (long long)cap_bytes,
                  (long long)need);
    if (!sec && in_ps < n * p->N) return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
    if (olen > 0 && !out) return fail(PFB_ERR_INVALID_ARG, "null output");
  } else if (olen > 0) {  // (pfb_synthesis_execute's; a call that yields nothing checks no more)
    if (!out) return fail(PFB_ERR_INVALID_ARG, "null output");
    if (cap_bytes < need)
      return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld bytes", (long long)cap_bytes,
                  (long long)need);
    if (!sec && in_ps < n * p->N) return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  HIPCHK(hipSetDevice(p->device));
  const bool fused = synthesis_dada_out_fusable(p, out, nbit);
  pfb_cf32* o;
  if (fused) {
    // (`out` stands in for the cf32 buffer in the callee's null, capacity and stride checks;
    // the block launches write through the plan's dout only)
    o = static_cast<pfb_cf32*>(out);
    p->dout = out;
    p->dout_nbit = nbit;
    p->dout_scale = scale;
  } else {
    HIPCHK(p->stage_out.ensure((size_t)p->n_pol * std::max<int64_t>(olen, 1) * sizeof(float2)));
    o = p->stage_out.as<pfb_cf32>();
  }
  const pfb_status st =
      stream_call ? ifb_exec(p, in, in_ps, sec, n, o, olen, olen, n_out, PFB_MEM_DEVICE, stream)
                  : synthesis_exec(p, in, in_ps, sec, n, sample_offset, o, olen, olen, n_out, PFB_MEM_DEVICE, stream);
  p->dout = nullptr;
  if (st != PFB_OK) return st;
  if (!fused && olen > 0)
    HIPCHK(pfb::launch_dada_pack_scaled(p->stage_out.as<float2>(), olen, olen, 1, p->n_pol, out, nbit, scale,
                                        (hipStream_t)stream));
  p->last_dada_out = fused ? PFB_DADA_OUTPUT_FUSED : PFB_DADA_OUTPUT_STAGED;
  return PFB_OK;
}

pfb_status pfb_synthesis_execute_to_dada(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_dat,
                                         int64_t sample_offset, void* out, int32_t out_nbit, float out_scale,
                                         int64_t cap_bytes, int64_t* n_out, void* stream) {
  return synthesis_to_dada(p, in, in_ps, nullptr, n_dat, sample_offset, out, out_nbit, out_scale, cap_bytes, n_out,
                           stream, false);
}

pfb_status pfb_inverse_filterbank_execute_to_dada(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                  int64_t n_in, void* out, int32_t out_nbit, float out_scale,
                                                  int64_t cap_bytes, int64_t* n_out, void* stream) {
  return synthesis_to_dada(p, in, in_ps, nullptr, n_in, 1, out, out_nbit, out_scale, cap_bytes, n_out, stream, true);
}

pfb_status pfb_synthesis_execute_dada_to_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                              int32_t order, int64_t n_dat, int64_t sample_offset, void* out,
                                              int32_t out_nbit, float out_scale, int64_t cap_bytes, int64_t* n_out,
                                              void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return synthesis_to_dada(p, nullptr, 0, &sec, n_dat, sample_offset, out, out_nbit, out_scale, cap_bytes, n_out,
                           stream, false);
}

pfb_status pfb_inverse_filterbank_execute_dada_to_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit,
                                                       int32_t ndim, int32_t order, int64_t n_in, void* out,
                                                       int32_t out_nbit, float out_scale, int64_t cap_bytes,
                                                       int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return synthesis_to_dada(p, nullptr, 0, &sec, n_in, 1, out, out_nbit, out_scale, cap_bytes, n_out, stream, true);
}

int32_t pfb_synthesis_last_dada_output(const pfb_synthesis_plan* p) { return p ? p->last_dada_out : -1; }

int64_t pfb_inverse_filterbank_buffered(const pfb_synthesis_plan* p) { return p ? p->buffered : -1; }

pfb_status pfb_inverse_filterbank_reset(pfb_synthesis_plan* p) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  p->buffered = 0;
  return PFB_OK;
}

// ------------------------------------------------------------------ round trip
// Analysis -> synthesis of one call, pipelined in chunks of synthesis blocks (the
// reference's test_data_pipeline.m:114,132 runs the two back to back).  Chunk c's
// analysis rows run on the analysis plan's own stream while chunk c-1 is synthesised
// on the caller's stream, so the two kernels share the chip (each alone leaves HBM and
// VALU partly idle), and the synthesis reads each channelised row shortly after it was
// written (Infinity-Cache resident).  The full channelised product is still written to
// `chan`.  On this chunked path every row and block is computed by the same kernels with
// the same inputs as pfb_analysis_execute + pfb_synthesis_execute, so both results are
// bit-identical to the separate calls (the fused path below: see its comment).

// What the file-to-file calls (roundtrip_dada, below) ask of roundtrip_run; the cf32 calls pass
// none of it.
struct RtOpt {
  // FUSED: the analysis launch reads the section dd in place and stores the product as the
  // float section od (`in` and `chan` then only have to pass the checks); the synthesis stores
  // through the plan's dout, which the caller sets.  Only for a call that `wave2` named.
  const AnaDada* dd = nullptr;
  const AnaOut* od = nullptr;
  // the stage-1 rows are stored whatever pfb_synthesis_set_stage1_rows says (no recomputing
  // kernel reads a section, and a plan-owned staging buffer is no input to come back to)
  bool stored = false;
  // every check of the call and the allocation of the rows, then return: no launch, no change
  // of the split round trip's key
  bool dry = false;
  // (dry) set when the call takes the fused path through the streaming analysis and the
  // Nf = 256 wave kernel on stored 2-row runs
  bool* wave2 = nullptr;
};

// phase 0: the whole round trip; 1 / 2: only the analysis / only the synthesis half of the
// fused path (pfb_roundtrip_analysis_execute / pfb_roundtrip_synthesis_execute), which hand
// the stage-1 rows over in the synthesis plan's scratch
static pfb_status roundtrip_run(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const pfb_cf32* in,
                                int64_t in_ps, int64_t n_dat, pfb_cf32* chan, int64_t chan_ps,
                                int64_t chan_cap, int64_t* n_chan_rows, int64_t sample_offset,
                                pfb_cf32* out, int64_t out_ps, int64_t out_cap, int64_t* n_out,
                                void* stream, int phase, const RtOpt& opt = RtOpt{}) {
  if (opt.wave2) *opt.wave2 = false;
  if (!pa || !ps || (!in && n_dat > 0 && phase != 2)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (pa->device != ps->device) return fail(PFB_ERR_INVALID_ARG, "plans on different devices");
  if (pa->variant == pfb::kLowCbf)
    return fail(PFB_ERR_UNSUPPORTED, "round trip of the LowCBF filterbank: use the separate calls");
  if (pa->N != ps->N || pa->n_pol != ps->n_pol)
    return fail(PFB_ERR_INVALID_ARG, "analysis (%d ch, %d pol) and synthesis (%d ch, %d pol) differ",
                pa->N, pa->n_pol, ps->N, ps->n_pol);
  if (sample_offset < 1) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 1-based (>= 1)");
  if (n_dat < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_dat");
  HIPCHK(hipSetDevice(pa->device));
  hipStream_t s = (hipStream_t)stream;
  const int64_t K = analysis_K(pa, n_dat);
  const int64_t off = std::min<int64_t>(sample_offset - 1, K);
  const int64_t B = synth_blocks(ps, K - off);
  const int64_t olen = B * ps->Lkeep;
  if (n_chan_rows) *n_chan_rows = K;
  if (n_out) *n_out = olen;
  if (K == 0) return PFB_OK;
  if (phase != 2) {
    if (!chan) return fail(PFB_ERR_INVALID_ARG, "null output");
    if (chan_cap < K) return fail(PFB_ERR_BUFFER_TOO_SMALL, "channelised capacity %lld < %lld rows",
                                  (long long)chan_cap, (long long)K);
    if (in_ps < n_dat || chan_ps < K * pa->N)
      return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  if (phase != 1) {
    if (olen > 0 && !out) return fail(PFB_ERR_INVALID_ARG, "null output");
    if (out_cap < olen) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld",
                                    (long long)out_cap, (long long)olen);
    if (olen > 0 && out_ps < olen) return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  const float2* x = (const float2*)in;
  float2* y = (float2*)chan;
  if (B == 0) return (phase == 2 || opt.dry) ? PFB_OK : analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s);

  // Fused: the analysis kernel also writes the synthesis stage-1 rows (the channel IFFT
  // of every row it produces, taken as N^2 x its FIR sums before the FFT rather than from
  // the rounded channelised row — equal in exact arithmetic, so the output agrees with
  // the separate calls to ~1e-7, not bit for bit) and the block kernel reads them; the
  // channelised product is still written in full (and IS bit-identical).  Needs an
  // analysis kernel that can emit the rows, no combine permutation / per-channel gain,
  // and device memory for the rows (bounded at 16 GiB; an explicit chunk size, or a
  // larger call, takes the chunked pipeline below).
  static const bool no_fuse = pfb::knob("PFB_RT_NO_FUSE") != nullptr;
  // (generic N > 256 path: Z holds all K rows — the row FFT makes the channelised product
  // from them — and the synthesis starts at row `off`; streaming kernel: K - off rows)
  const int64_t z0 = pa->fused ? off : 0;
  const int64_t zr = K - z0;
  // Nf = 256 synthesis through the wave kernel: the streaming analysis writes the rows in
  // the blocked layout it reads (16-row runs per phase; the series' rows from `off` on,
  // which must start a run; rows rounded up to whole runs)
  // (PFB_SYNTH_WAVE=0: the block kernel on rows; PFB_ZBLK: the run length, experiments build)
  static const bool no_wave = pfb::knob("PFB_SYNTH_WAVE") && std::atoi(pfb::knob("PFB_SYNTH_WAVE")) == 0;
  static const int zb_knob = pfb::knob("PFB_ZBLK") ? std::atoi(pfb::knob("PFB_ZBLK")) : 2;
  int zblk = (!no_wave && analysis_emits_zblk(pa) && z0 == off && off % 16 == 0) ? zb_knob : 0;
  if (zblk && !pfb::synth_wave_supported(synth_args(ps, nullptr, 0, 0, B, nullptr, 0, 0, zblk))) zblk = 0;
  // generic path (N > 256, the SKA-Mid round trip): the FIR writes the rows in 2-row runs
  // per column, so the Nf = 512 wave synthesis loads whole 128-B lines (2 rows x 8 phases)
  // — bit-identical; measured (profiles/r05_v17_c3_zrun_kernel_ab/) synthesis -17 us, FIR
  // +8 us, row FFT +4 us (it reads each row's pair partner from the lines fetched one row
  // earlier): net -5 us per unit (PFB_C3_ZRUN=0: rows, experiments build)
  static const bool zrun_on = !(pfb::knob("PFB_C3_ZRUN") && std::atoi(pfb::knob("PFB_C3_ZRUN")) == 0);
  const bool zrun = zrun_on && !zblk && !pa->fused && analysis_emits_z(pa) && off % 2 == 0 &&
                    pfb::synth_wave512_supported(synth_args(ps, nullptr, 0, 0, B, nullptr, 0, 0, 2));
  if (zrun) zblk = 2;
  const int64_t zrows = zrun ? (zr + 1) / 2 * 2 : zblk ? (zr + 15) / 16 * 16 : zr;
  const size_t zbytes = (size_t)pa->n_pol * zrows * pa->N * sizeof(float2);
  bool fuse = !no_fuse && analysis_emits_z(pa) && ps->identity_perm && !ps->has_cgain &&
              !ps->has_spectral && ps->chunk_blocks <= 0 && zbytes <= ((size_t)16 << 30);
  // Recomputed stage-1 rows (SynthBlockArgs::fir_x): the analysis writes only the
  // channelised product and the synthesis evaluates the rows it needs from the input
  // series — the same FIR sums, bit for bit (555 instead of 727 MB of HBM traffic per C2
  // step).  Where the wave kernel takes the run layout (zblk) and has a FIR variant
  // (pfb_synthesis_set_stage1_rows).
  const bool synth_fir_on =
      !opt.stored && (ps->stage1 == PFB_STAGE1_RECOMPUTED || (ps->stage1 == PFB_STAGE1_AUTO && kSynthFirDefault));
  FirSrc fsrc{(const float2*)in, in_ps, n_dat, off / std::max(pa->nu, 1), pa->gtab.as<float>(), pa->nu, pa->de,
              pa->P + 1};
  bool fir = false;
  if (synth_fir_on && zblk && pa->gtab.p && off % pa->nu == 0 && phase != 2) {
    fir = pfb::synth_wave_fir_supported(synth_args(ps, nullptr, 0, 0, B, nullptr, 0, 0, 0, &fsrc));
  }
  if (phase == 2 && ps->zkey_x != nullptr) {
    // the analysis half chose recomputed rows: the synthesis reads the input it recorded
    fir = true;
    fsrc.x = (const float2*)ps->zkey_x;
    fsrc.x_ps = ps->zkey_xps;
  }
  const int64_t zkey[5] = {n_dat, off, fir ? -1 : zblk, K, zrows};
  if (fir && fuse) {
    if (phase == 2) {
      if (ps->zkey_plan != pa->serial || !std::equal(zkey, zkey + 5, ps->zkey))
        return fail(PFB_ERR_INVALID_ARG,
                    "split round trip: the synthesis plan holds no analysis half of this analysis plan, "
                    "n_dat %lld and sample_offset %lld (run pfb_roundtrip_analysis_execute with the same "
                    "arguments first)",
                    (long long)n_dat, (long long)sample_offset);
      if (opt.dry) return PFB_OK;
      return synthesis_blocks(ps, nullptr, 0, 0, B, (float2*)out, out_ps, olen, s, 0, &fsrc);
    }
    if (opt.dry) return PFB_OK;
    zkey_clear(ps);
    pfb_status st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s);
    if (st != PFB_OK) return st;
    if (phase == 1) {
      // the synthesis half re-reads this input: the caller keeps it unchanged until then
      ps->zkey_plan = pa->serial;
      std::copy(zkey, zkey + 5, ps->zkey);
      ps->zkey_x = in;
      ps->zkey_xps = in_ps;
      return PFB_OK;
    }
    return synthesis_blocks(ps, nullptr, 0, 0, B, (float2*)out, out_ps, olen, s, 0, &fsrc);
  }
  if (fuse && phase == 2) {
    // the synthesis half reads the rows the analysis half left in the plan's scratch: they
    // must come from this analysis plan with the same n_dat, offset and row layout
    if (!ps->Z.p || ps->Z.bytes < zbytes || ps->zkey_plan != pa->serial ||
        !std::equal(zkey, zkey + 5, ps->zkey))
      return fail(PFB_ERR_INVALID_ARG,
                  "split round trip: the synthesis plan holds no stage-1 rows of this analysis plan, "
                  "n_dat %lld and sample_offset %lld (run pfb_roundtrip_analysis_execute with the same "
                  "arguments first)",
                  (long long)n_dat, (long long)sample_offset);
  } else if (fuse) {
    // the rows of the whole call stay resident; a device without room for them takes the
    // chunked pipeline below (its scratch is one chunk's rows) instead of failing
    // (a dry run returns before the key is cleared below: rows that a key vouches for go with
    // the buffer this allocation replaces)
    if (opt.dry && (!ps->Z.p || ps->Z.bytes < zbytes)) zkey_clear(ps);
    const hipError_t ze = ps->Z.ensure(zbytes);
    if (ze == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      fuse = false;
    } else if (ze != hipSuccess) {
      return fail(PFB_ERR_HIP, "round trip stage-1 rows (%zu bytes): %s", zbytes, hipGetErrorString(ze));
    }
  }
  // (the file-to-file calls: FUSED is this path only, and is asked for only where a dry run
  // of the same call named it)
  const bool wave2 = fuse && pa->fused && zblk == 2;
  if ((opt.dd || opt.od) && !(wave2 && opt.dd && opt.od))
    return fail(PFB_ERR_UNSUPPORTED, "round trip: these plans have no kernel that reads and stores sections");
  if (phase != 0) {
    // the split round trip exists for the fused path only (one scratch of rows handed over)
    if (!fuse) return fail(PFB_ERR_UNSUPPORTED, "split round trip: these plans take the chunked pipeline "
                                                "(use pfb_roundtrip_execute)");
    if (opt.wave2) *opt.wave2 = wave2;
    if (opt.dry) return PFB_OK;
    float2* Z = ps->Z.as<float2>();
    if (phase == 1) {
      zkey_clear(ps);
      pfb_status st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s, Z, zrows * pa->N, z0, 0, nullptr,
                                   zblk, nullptr, 0, nullptr, opt.dd, opt.od);
      if (st != PFB_OK) return st;
      ps->zkey_plan = pa->serial;
      std::copy(zkey, zkey + 5, ps->zkey);
      return PFB_OK;
    }
    return synthesis_blocks(ps, Z + (off - z0) * pa->N, zrows * pa->N, 0, B, (float2*)out, out_ps, olen, s, zblk);
  }
  if (opt.wave2) *opt.wave2 = wave2;
  if (opt.dry) return PFB_OK;
  zkey_clear(ps);  // phase 0 reuses Z
  if (fuse) {
    float2* Z = ps->Z.as<float2>();
    // (retired round 5, measured slower twice: the row FFT on a second stream beside the
    // synthesis, Infinity-Cache chunking of the generic path and chunked analysis/synthesis
    // concurrency — profiles/HISTORY.md)
    // (generic N > 256 path: the FIR and the row FFT as two calls on the stream — the same
    // two launches as one call, each then timed alone by the profiler)
    pfb_status st = PFB_OK;
    if (!pa->fused) {
      st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s, Z, zrows * pa->N, z0, 0, nullptr, zblk,
                        nullptr, 1);
      if (st == PFB_OK)
        st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s, Z, zrows * pa->N, z0, 0, nullptr, zblk,
                          nullptr, 2);
    } else {
      st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, 0, K, K, s, Z, zrows * pa->N, z0, 0, nullptr, zblk, nullptr,
                        0, nullptr, opt.dd, opt.od);
    }
    if (st != PFB_OK) return st;
    return synthesis_blocks(ps, Z + (off - z0) * pa->N, zrows * pa->N, 0, B, (float2*)out, out_ps,
                            olen, s, zblk);
  }

  if (!pa->aux) HIPCHK(hipStreamCreateWithFlags(&pa->aux, hipStreamNonBlocking));
  int64_t CB = ps->chunk_blocks > 0 ? ps->chunk_blocks : ps->rt_chunk_blocks;
  CB = std::max<int64_t>(1, std::min<int64_t>(CB, B));
  const int64_t n_chunks = (B + CB - 1) / CB;
  while ((int64_t)pa->events.size() < n_chunks + 2) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    pa->events.push_back(e);
  }
  // fork: the analysis stream starts after everything already queued on the caller's
  HIPCHK(hipEventRecord(pa->events[0], s));
  HIPCHK(hipStreamWaitEvent(pa->aux, pa->events[0], 0));
  const float2* sin_ = y + off * pa->N;  // synthesis input = chan(:, :, sample_offset:end)
  int64_t ra = 0;                        // analysis rows done
  for (int64_t c = 0; c < n_chunks; ++c) {
    const int64_t b0 = c * CB, nb = std::min<int64_t>(CB, B - b0);
    // channelised rows the chunk reads: [off + b0 keep, off + (b0+nb) keep + 2 Ov); the
    // padded variant's output row t comes from analysis row (t + sds) mod K (rows that
    // wrap come from the first rows, produced by chunk 0)
    int64_t need = (c == n_chunks - 1) ? K : off + (b0 + nb) * ps->keep + 2 * (int64_t)ps->Ov;
    if (pa->variant == pfb::kPadded) need += pa->sds;
    const int64_t rb = std::max(ra, std::min(K, need));
    pfb_status st = analysis_run(pa, x, in_ps, n_dat, y, chan_ps, ra, rb, K, pa->aux);
    if (st != PFB_OK) return st;
    ra = rb;
    HIPCHK(hipEventRecord(pa->events[1 + c], pa->aux));
    HIPCHK(hipStreamWaitEvent(s, pa->events[1 + c], 0));
    st = synthesis_chunk(ps, sin_, chan_ps, b0, nb, (float2*)out, out_ps, olen, s);
    if (st != PFB_OK) return st;
  }
  // join (the last chunk already ran the analysis to K)
  HIPCHK(hipEventRecord(pa->events[1 + n_chunks], pa->aux));
  HIPCHK(hipStreamWaitEvent(s, pa->events[1 + n_chunks], 0));
  return PFB_OK;
}

pfb_status pfb_roundtrip_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const pfb_cf32* in,
                                 int64_t in_ps, int64_t n_dat, pfb_cf32* chan, int64_t chan_ps,
                                 int64_t chan_cap, int64_t* n_chan_rows, int64_t sample_offset,
                                 pfb_cf32* out, int64_t out_ps, int64_t out_cap, int64_t* n_out,
                                 void* stream) {
  return roundtrip_run(pa, ps, in, in_ps, n_dat, chan, chan_ps, chan_cap, n_chan_rows, sample_offset,
                       out, out_ps, out_cap, n_out, stream, 0);
}

pfb_status pfb_roundtrip_analysis_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const pfb_cf32* in,
                                          int64_t in_ps, int64_t n_dat, pfb_cf32* chan, int64_t chan_ps,
                                          int64_t chan_cap, int64_t* n_chan_rows, int64_t sample_offset,
                                          void* stream) {
  return roundtrip_run(pa, ps, in, in_ps, n_dat, chan, chan_ps, chan_cap, n_chan_rows, sample_offset,
                       nullptr, 0, 0, nullptr, stream, 1);
}

pfb_status pfb_roundtrip_synthesis_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, int64_t n_dat,
                                           int64_t sample_offset, pfb_cf32* out, int64_t out_ps,
                                           int64_t out_cap, int64_t* n_out, void* stream) {
  return roundtrip_run(pa, ps, nullptr, n_dat, n_dat, nullptr, 0, 0, nullptr, sample_offset, out, out_ps,
                       out_cap, n_out, stream, 2);
}

// ---- the round trip from a DADA section into DADA sections (pfb_api.h)
// The sections of a file-to-file call.  Each cell of the A/B (DESIGN.md §4.9,
// profiles/dada_roundtrip_ab.jsonl) that met the decision rule stays FUSED; one that did not
// is listed in rt_dada_cell_staged and takes the STAGED sequence.
struct RtSections {
  AnaSection in;            // phase != 2
  void* chan;               // phase != 2: the float product section
  int64_t chan_cap_bytes;
  void* out;                // phase != 1
  int32_t out_nbit;
  float out_scale;
  int64_t out_cap_bytes;
};

// (polarisations, input NBIT, output NBIT) cells the A/B sent STAGED: none was measured slower
static bool rt_dada_cell_staged(int /*n_pol*/, int /*in_nbit*/, int /*out_nbit*/) { return false; }

// FUSED, input side: the round trip's kernel loads such a section itself
static bool roundtrip_dada_in_fusable(const pfb_analysis_plan* p, const AnaSection& sec, const void* chan) {
  if (sec.ndim != 2 || sec.order != PFB_DADA_TFP || (sec.nbit != 8 && sec.nbit != 16 && sec.nbit != 32)) return false;
  if (reinterpret_cast<uintptr_t>(sec.base) % (size_t)(sec.nbit / 4) != 0) return false;
  if (reinterpret_cast<uintptr_t>(chan) % 8 != 0) return false;
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  a.n_pol = p->n_pol;
  return pfb::stream_rt_dada_supported(a, sec.nbit);
}

// phase: roundtrip_run's.  Every check — roundtrip_run's own among them, through its dry run —
// comes before the first launch and before the split round trip's key changes; then FUSED (the
// analysis launch reads and stores the sections, the wave synthesis stores the output section)
// or STAGED (unpack, the cf32 round trip on plan-owned buffers, the packs).
static pfb_status roundtrip_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const RtSections& sec, int64_t n_dat,
                                 int64_t* n_chan_rows, int64_t sample_offset, int64_t* n_out, void* stream,
                                 int phase) {
  if (!pa || !ps) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (phase != 2) {
    const pfb_status st = ana_section_check(pa, sec.in, n_dat);
    if (st != PFB_OK) return st;
    if (reinterpret_cast<uintptr_t>(sec.in.base) % (size_t)(sec.in.nbit / 8) != 0)
      return fail(PFB_ERR_INVALID_ARG, "input section not aligned to its NBIT");
    if (reinterpret_cast<uintptr_t>(sec.chan) % 4 != 0)
      return fail(PFB_ERR_INVALID_ARG, "channelised section not aligned to a float");
  }
  if (phase != 1) {
    if (sec.out_nbit != 8 && sec.out_nbit != 16 && sec.out_nbit != 32 && sec.out_nbit != 64)
      return fail(PFB_ERR_INVALID_ARG, "output NBIT must be 8, 16, 32 or 64");
    if (!std::isfinite(sec.out_scale)) return fail(PFB_ERR_INVALID_ARG, "output scale is not finite");
    if (reinterpret_cast<uintptr_t>(sec.out) % (size_t)(sec.out_nbit / 8) != 0)
      return fail(PFB_ERR_INVALID_ARG, "output section not aligned to its NBIT");
  }
  // the cf32 call's checks, in its order, with the capacities in its units: whole rows of the
  // product section, whole samples (all polarisations) of the output section
  const int64_t big = INT64_MAX / 4;  // (a stride that passes: nothing is launched)
  const int64_t chan_cap = phase != 2 ? std::max<int64_t>(sec.chan_cap_bytes, 0) / ((int64_t)pa->N * pa->n_pol * 8) : 0;
  const int64_t out_cap =
      phase != 1 ? std::max<int64_t>(sec.out_cap_bytes, 0) / ((int64_t)ps->n_pol * 2 * (sec.out_nbit / 8)) : 0;
  const pfb_cf32* in_c = static_cast<const pfb_cf32*>(sec.in.base);
  pfb_cf32* chan_c = static_cast<pfb_cf32*>(sec.chan);
  pfb_cf32* out_c = static_cast<pfb_cf32*>(sec.out);
  int64_t K = 0, olen = 0;
  bool wave2 = false;
  RtOpt dry;
  dry.stored = true;
  dry.dry = true;
  dry.wave2 = &wave2;
  pfb_status st = phase == 2 ? roundtrip_run(pa, ps, nullptr, n_dat, n_dat, nullptr, 0, 0, &K, sample_offset, out_c,
                                             big, out_cap, &olen, stream, 2, dry)
                             : roundtrip_run(pa, ps, in_c, big, n_dat, chan_c, big, chan_cap, &K, sample_offset,
                                             out_c, big, phase == 1 ? 0 : out_cap, &olen, stream, phase, dry);
  if (n_chan_rows && phase != 2) *n_chan_rows = K;
  if (n_out && phase != 1) *n_out = olen;
  if (st != PFB_OK || K == 0) return st;
  if (phase == 2 && olen == 0) return PFB_OK;

  hipStream_t s = (hipStream_t)stream;
  const int P = pa->n_pol;
  const bool in_fused = phase != 2 && roundtrip_dada_in_fusable(pa, sec.in, sec.chan);
  const bool out_fused = phase != 1 && synthesis_dada_out_fusable(ps, sec.out, sec.out_nbit);
  const bool cell = phase == 0 && rt_dada_cell_staged(P, sec.in.nbit, sec.out_nbit);
  const bool fused = wave2 && !cell && (phase == 2 || in_fused) && (phase == 1 || out_fused);
  RtOpt run;
  run.stored = true;
  if (fused) {
    // (the sections stand in for the cf32 buffers in the callee's checks; the launches go
    // through dd / od and the synthesis plan's dout only)
    const AnaDada dd{sec.in.base, sec.in.nbit};
    const AnaOut od{sec.chan, 32, 1.0f};
    if (phase != 2) {
      run.dd = &dd;
      run.od = &od;
    }
    if (phase != 1) {
      ps->dout = sec.out;
      ps->dout_nbit = sec.out_nbit;
      ps->dout_scale = sec.out_scale;
    }
    st = phase == 2 ? roundtrip_run(pa, ps, nullptr, n_dat, n_dat, nullptr, 0, 0, nullptr, sample_offset, out_c, olen,
                                    olen, nullptr, stream, 2, run)
                    : roundtrip_run(pa, ps, in_c, n_dat, n_dat, chan_c, K * pa->N, K, nullptr, sample_offset, out_c,
                                    olen, olen, nullptr, stream, phase, run);
    ps->dout = nullptr;
    if (st != PFB_OK) return st;
    if (phase != 2) pa->last_dada_out = PFB_DADA_OUTPUT_FUSED;  // (last_dada: analysis_run, FUSED)
    if (phase != 1) ps->last_dada_out = PFB_DADA_OUTPUT_FUSED;
    return PFB_OK;
  }

  // STAGED: pfb_dada_unpack, the cf32 call, pfb_dada_pack at NBIT 32 of the product, the scaled
  // pack of the output.  One polarisation's float section is the cf32 product itself.
  float2* x = nullptr;
  float2* y = nullptr;
  float2* o = nullptr;
  bool chan_direct = false;
  if (phase != 2) {
    HIPCHK(pa->stage_in.ensure((size_t)P * n_dat * sizeof(float2)));
    x = pa->stage_in.as<float2>();
    chan_direct = P == 1 && reinterpret_cast<uintptr_t>(sec.chan) % 8 == 0;
    if (chan_direct) {
      y = static_cast<float2*>(sec.chan);
    } else {
      HIPCHK(pa->dada_stage.ensure((size_t)P * K * pa->N * sizeof(float2)));
      y = pa->dada_stage.as<float2>();
    }
  }
  if (phase != 1 && olen > 0) {
    HIPCHK(ps->stage_out.ensure((size_t)P * olen * sizeof(float2)));
    o = ps->stage_out.as<float2>();
  }
  if (phase != 2) {
    st = ana_section_unpack(pa, sec.in, 0, n_dat, x, n_dat, s);
    if (st != PFB_OK) return st;
  }
  st = phase == 2 ? roundtrip_run(pa, ps, nullptr, n_dat, n_dat, nullptr, 0, 0, nullptr, sample_offset,
                                  reinterpret_cast<pfb_cf32*>(o), olen, olen, nullptr, stream, 2, run)
                  : roundtrip_run(pa, ps, reinterpret_cast<const pfb_cf32*>(x), n_dat, n_dat,
                                  reinterpret_cast<pfb_cf32*>(y), K * pa->N, K, nullptr, sample_offset,
                                  reinterpret_cast<pfb_cf32*>(o), olen, olen, nullptr, stream, phase, run);
  if (st != PFB_OK) return st;
  if (phase != 2) {
    if (!chan_direct) {
      st = pfb_dada_pack(reinterpret_cast<const pfb_cf32*>(y), K * pa->N, K, pa->N, P, sec.chan, 32, stream);
      if (st != PFB_OK) return st;
    }
    pa->last_dada = PFB_DADA_INPUT_STAGED;
    pa->last_dada_out = PFB_DADA_OUTPUT_STAGED;
  }
  if (phase != 1) {
    if (olen > 0) HIPCHK(pfb::launch_dada_pack_scaled(o, olen, olen, 1, P, sec.out, sec.out_nbit, sec.out_scale, s));
    ps->last_dada_out = PFB_DADA_OUTPUT_STAGED;
  }
  return PFB_OK;
}

pfb_status pfb_roundtrip_execute_dada_to_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const void* in,
                                              int32_t nbit, int32_t ndim, int32_t order, int64_t n_dat, void* chan,
                                              int64_t chan_cap_bytes, int64_t* n_chan_rows, int64_t sample_offset,
                                              void* out, int32_t out_nbit, float out_scale, int64_t out_cap_bytes,
                                              int64_t* n_out, void* stream) {
  const RtSections sec{AnaSection{in, nbit, ndim, order}, chan, chan_cap_bytes, out, out_nbit, out_scale, out_cap_bytes};
  return roundtrip_dada(pa, ps, sec, n_dat, n_chan_rows, sample_offset, n_out, stream, 0);
}

pfb_status pfb_roundtrip_analysis_execute_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const void* in,
                                               int32_t nbit, int32_t ndim, int32_t order, int64_t n_dat, void* chan,
                                               int64_t chan_cap_bytes, int64_t* n_chan_rows, int64_t sample_offset,
                                               void* stream) {
  const RtSections sec{AnaSection{in, nbit, ndim, order}, chan, chan_cap_bytes, nullptr, 0, 1.f, 0};
  return roundtrip_dada(pa, ps, sec, n_dat, n_chan_rows, sample_offset, nullptr, stream, 1);
}

pfb_status pfb_roundtrip_synthesis_execute_to_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, int64_t n_dat,
                                                   int64_t sample_offset, void* out, int32_t out_nbit,
                                                   float out_scale, int64_t out_cap_bytes, int64_t* n_out,
                                                   void* stream) {
  const RtSections sec{AnaSection{nullptr, 0, 0, 0}, nullptr, 0, out, out_nbit, out_scale, out_cap_bytes};
  return roundtrip_dada(pa, ps, sec, n_dat, nullptr, sample_offset, n_out, stream, 2);
}

// ------------------------------------------------------------------ utilities
double pfb_calc_output_nbins(int64_t nbins, int32_t channels, int32_t os_nu, int32_t os_de,
                             int64_t filter_taps, int32_t input_fft_length, int32_t input_overlap) {
  // calc_output_nbins.m:17-27, in Matlab's double arithmetic
  const double nu = os_nu, de = os_de, ch = channels;
  const double step = std::floor(ch * de / nu);
  const double nblocks_pfb = std::floor(((double)nbins - (double)filter_taps) / step);
  const double output_pfb = std::floor(step * nblocks_pfb / ch);
  const double input_keep = (double)input_fft_length - 2.0 * input_overlap;
  const double nblocks_ipfb = std::floor((output_pfb - 2.0 * input_overlap) / input_keep);
  const double output_fft_length = (double)input_fft_length * de / nu * ch;  // normalize.m:17
  const double output_overlap = (double)input_overlap * de / nu * ch;
  return (output_fft_length - 2.0 * output_overlap) * nblocks_ipfb;
}

pfb_status pfb_device_malloc(int32_t device, int64_t bytes, void** ptr) {
  if (!ptr || bytes < 0) return fail(PFB_ERR_INVALID_ARG, "bad arguments");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(ptr, (size_t)std::max<int64_t>(bytes, 1)));
  return PFB_OK;
}
pfb_status pfb_device_free(void* ptr) {
  if (ptr) HIPCHK(hipFree(ptr));
  return PFB_OK;
}
pfb_status pfb_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return PFB_OK;
}
pfb_status pfb_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return PFB_OK;
}
pfb_status pfb_stream_synchronize(void* stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return PFB_OK;
}

pfb_status pfb_profile_enable(int32_t enable) {
  g_prof.drain();
  g_prof.enabled = enable != 0;
  return PFB_OK;
}
pfb_status pfb_profile_read(int32_t which, double* total_ms, int64_t* launches, double* bytes) {
  if (which < 0 || which >= Profiler::kClasses) return fail(PFB_ERR_INVALID_ARG, "which must be 0..5");
  g_prof.drain();
  if (total_ms) *total_ms = g_prof.total_ms[which];
  if (launches) *launches = g_prof.launches[which];
  if (bytes) *bytes = g_prof.bytes[which];
  return PFB_OK;
}
pfb_status pfb_profile_reset(void) {
  g_prof.drain();
  for (int i = 0; i < Profiler::kClasses; ++i) {
    g_prof.total_ms[i] = 0;
    g_prof.launches[i] = 0;
    g_prof.bytes[i] = 0;
    g_prof.names[i].clear();
  }
  return PFB_OK;
}
pfb_status pfb_profile_kernel_name(int32_t which, char* buf, int64_t len) {
  if (which < 0 || which >= Profiler::kClasses) return fail(PFB_ERR_INVALID_ARG, "which must be 0..5");
  if (!buf || len <= 0) return fail(PFB_ERR_INVALID_ARG, "null or empty buffer");
  const std::string& n = g_prof.names[which];
  const size_t k = std::min<size_t>(n.size(), (size_t)len - 1);
  std::memcpy(buf, n.data(), k);
  buf[k] = 0;
  return PFB_OK;
}
int32_t pfb_build_flags(void) { return pfb::kExperiments ? 1 : 0; }

}  // extern "C"
