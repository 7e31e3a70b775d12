// pfb_api_analysis.hip — the analysis half of the C ABI (include/pfb_api.h): the analysis plan
// (tap padding and the tables computed in double, rounded once to float), the launch of one
// analysis (analysis_run), pfb_analysis_execute* and the FilterBank stream object
// (pfb_filterbank_*: carry-over buffers and kernel dispatch), with their to-DADA and quantised
// to-DADA forms (analysis_to_dada, analysis_quantised).
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "pfb_host.hpp"

using namespace pfb::host;

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

pfb::AnalysisArgs pfb::host::analysis_shape(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a{};
  a.variant = p->variant;
  a.N = p->N;
  a.M = p->M;
  a.P = p->P;
  a.nu = p->nu;
  a.n_pol = p->n_pol;
  return a;
}

// The shape of the kernel that reads or stores a DADA section in place of the plan's own: a
// LowCBF plan's is the streaming kernel's LCBF instantiation (a Bunton shape), unless the
// experiments build's knob picks the one-shot kernel (pfb_lowcbf.hip), which has none: false
static bool section_kernel_shape(const pfb_analysis_plan* p, pfb::AnalysisArgs& a) {
  a = analysis_shape(p);
  if (p->variant != pfb::kLowCbf) return true;
  if (pfb::knob("PFB_LOWCBF_STREAM") && std::atoi(pfb::knob("PFB_LOWCBF_STREAM")) == 0) return false;
  a.variant = pfb::kBunton;
  return true;
}

// the plan's analysis runs on the streaming kernel, which takes a read offset (pad)
static bool analysis_offset_ok(const pfb_analysis_plan* p) { return pfb::analysis_takes_offset(analysis_shape(p)); }

// FUSED (pfb_api.h): the plan's kernel loads such a section itself
static bool analysis_dada_fusable(const pfb_analysis_plan* p, const void* base, int nbit, int ndim, int order) {
  if (ndim != 2 || order != PFB_DADA_TFP || (nbit != 8 && nbit != 16 && nbit != 32)) return false;
  if (reinterpret_cast<uintptr_t>(base) % (size_t)(nbit / 4) != 0) return false;
  pfb::AnalysisArgs a;
  return section_kernel_shape(p, a) && pfb::analysis_reads_dada(a, nbit);
}

// FUSED output (pfb_api.h): the plan's kernel stores such a section itself
static bool analysis_dada_out_fusable(const pfb_analysis_plan* p, const void* base, int nbit) {
  if (nbit != 8 && nbit != 16 && nbit != 32) return false;
  if (reinterpret_cast<uintptr_t>(base) % (size_t)(nbit / 4) != 0) return false;
  pfb::AnalysisArgs a;
  return section_kernel_shape(p, a) && pfb::analysis_writes_dada(a, nbit);
}

static bool analysis_fused_carry_ok(const pfb_analysis_plan* p) {
  return pfb::analysis_fused_takes_carry(analysis_shape(p));
}

// streaming kernel (N = 256) or register-window FIR
bool pfb::host::analysis_emits_z(const pfb_analysis_plan* p) { return pfb::analysis_can_emit_z(analysis_shape(p)); }

// streaming kernel (N = 256)
bool pfb::host::analysis_emits_zblk(const pfb_analysis_plan* p) {
  return pfb::analysis_can_emit_zblk(analysis_shape(p));
}

int64_t pfb::host::analysis_K(const pfb_analysis_plan* p, int64_t n_dat) {
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

// ====================================================================== one analysis launch
// the request as the kernels take it (every launch but the one-shot LowCBF kernel's)
static pfb::AnalysisArgs analysis_args(const pfb_analysis_plan* p, const AnaLaunch& l) {
  pfb::AnalysisArgs a = analysis_shape(p);
  a.in = l.in;
  a.in_pol_stride = l.in_ps;
  a.n_dat = l.n_dat;
  a.pad = l.pad;
  a.pre = l.pre;
  a.pre_pol_stride = l.pad;
  a.out = l.dada_out ? nullptr : l.out;
  a.out_pol_stride = l.dada_out ? 0 : l.out_ps;
  if (l.lay) {
    a.out_rs = (int)l.lay->rs;
    a.out_cs = (int)l.lay->cs;
    a.sel_split = l.lay->split;
    a.sel_shift = l.lay->shift;
    a.sel_n = l.lay->nsel;
    a.out_keep = l.lay->keep;
  }
  a.row0 = l.row0;
  a.K = l.K_end;
  a.K_total = l.K_total;
  a.z = l.z;
  a.z_pol_stride = l.z_ps;
  a.z_row0 = l.z_row0;
  a.zblk = l.zblk;
  a.z_stage = l.z_stage;
  if (l.carry_out) {
    a.carry_out = l.carry_out->dst;
    a.carry_src = l.carry_out->src;
    a.carry_n = l.carry_out->n;
    a.carry_pol_stride = l.carry_out->dst_ps;
  }
  if (l.dada_in) {
    a.din = l.dada_in->base;
    a.din_nbit = l.dada_in->nbit;
  }
  if (l.dada_out) {
    a.dout = l.dada_out->base;
    a.dout_nbit = l.dada_out->nbit;
    a.dout_scale = l.dada_out->scale;
    a.out_keep = l.dada_keep >= 0 ? l.dada_keep : l.K_end;
  }
  a.sds = p->sds;
  a.taps = p->taps.as<float>();
  a.twN = p->twN.as<float2>();
  a.zrev = p->zrev.p ? p->zrev.as<int>() : nullptr;
  return a;
}

pfb_status pfb::host::analysis_run(pfb_analysis_plan* p, const AnaLaunch& l, hipStream_t s) {
  const int64_t row0 = l.row0, K_end = l.K_end, K_total = l.K_total, n_dat = l.n_dat;
  const AnaDada* dd = l.dada_in;
  const AnaOut* od = l.dada_out;
  if (K_end <= row0) return PFB_OK;
  if (dd) p->last_dada = PFB_DADA_INPUT_FUSED;
  if (od) {
    // (with stage-1 rows: only the file-to-file round trip's launch — a section read in place,
    // the float section and 2-row runs, pfb::launch_stream_rt_dada)
    const bool rt = l.z && dd && od->nbit == 32 && l.zblk == 2 && l.z_stage == 0 && !l.pre && !l.carry_out;
    if ((l.z && !rt) || l.lay || row0 != 0) return fail(PFB_ERR_UNSUPPORTED, "DADA output: the plain product only");
  }
  const double in_b = dd ? 2.0 * (dd->nbit / 8) : 8.0;  // bytes per input sample
  const double out_b = od ? 2.0 * (od->nbit / 8) : 8.0;  // bytes per output sample
  if (l.moments || l.qin) {
    // the streaming kernel's moments instantiation, its input-quantiser instantiation, or both:
    // the plain product of all the call's rows
    // (a LowCBF plan: its streaming shape, as launch_lowcbf sets it up)
    if (od || l.z || l.lay || row0 != 0)
      return fail(PFB_ERR_UNSUPPORTED, "moments / input quantiser at the load: the plain product only");
    const bool lcbf = p->variant == pfb::kLowCbf;
    pfb::AnalysisArgs a = analysis_args(p, l);
    a.scratch = nullptr;
    if (lcbf) {
      a.variant = pfb::kBunton;
      a.pad = l.pre ? l.pad : p->lowcbf_pad ? 1536 : 0;
      a.pre_pol_stride = a.pad;
      a.lcbf_scale = 4096.0f;
    }
    const int64_t slots = pfb::stream_moments_slots(a, lcbf);
    if (slots <= 0) return fail(PFB_ERR_UNSUPPORTED, "moments: the plan is not on the streaming kernel");
    if (l.moments) {
      HIPCHK(p->quant_mom.ensure((size_t)slots * 3 * sizeof(double)));
      a.mom = p->quant_mom.as<double>();
    }
    ProfScope ps(0, (double)p->n_pol * (in_b * n_dat + 8.0 * K_end * p->C), s);
    if (l.qin) {
      a.qin = l.qin->stats;
      HIPCHK(pfb::launch_stream_qin(a, lcbf, s));
    } else {
      HIPCHK(pfb::launch_stream_moments(a, lcbf, s));
    }
    if (l.moments) l.moments->slots = slots;
    return PFB_OK;
  }
  if (p->variant == pfb::kLowCbf) {
    pfb::LowCbfArgs c{};
    c.in = l.in;
    c.in_pol_stride = l.in_ps;
    c.n_dat = n_dat;
    // (a DADA stream call: the carried samples in front of the section, pad = their count)
    c.pad = l.pre ? l.pad : p->lowcbf_pad ? 1536 : 0;
    c.pre = l.pre;
    if (dd) {
      c.din = dd->base;
      c.din_nbit = dd->nbit;
    }
    if (od) {
      c.dout = od->base;
      c.dout_nbit = od->nbit;
      c.dout_scale = od->scale;
    }
    c.out = od ? nullptr : l.out;
    c.out_pol_stride = od ? 0 : l.out_ps;
    c.K = K_end;
    c.n_pol = p->n_pol;
    c.taps = p->taps.as<float>();
    c.tw = p->twN.as<float2>();
    c.scale = 4096.0f;  // 2^9 * 2048 * 256 / 2^9 / 128
    ProfScope ps(0, (double)p->n_pol * (in_b * n_dat + out_b * K_end * p->C), s);
    HIPCHK(pfb::launch_lowcbf(c, s));
    return PFB_OK;
  }
  pfb::AnalysisArgs a = analysis_args(p, l);
  a.scratch = nullptr;
  if (!p->fused && !l.z) {
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
  const int cls = !l.z ? 0 : l.z_stage == 1 ? 4 : l.z_stage == 2 ? 5 : 3;
  const double cls_bytes = l.z_stage == 1 ? (double)p->n_pol * 8.0 * in_samples + zrow_bytes
                           : l.z_stage == 2 ? 2.0 * zrow_bytes : bytes;
  ProfScope ps(cls, cls_bytes, s, p->fused || l.z_stage != 0);
  if (od && !p->fused) {
    // a section from the generic path (a 4096-channel plan): its two launches apart, each timed
    // alone as the class that names it — the FIR (4; it reads the section dd in place) and the
    // row FFT that stores the section (5: the scratch rows in, the kept rows' samples out)
    a.z_stage = 1;
    {
      ProfScope fir(4, (double)p->n_pol * in_b * in_samples + zrow_bytes, s);
      HIPCHK(pfb::launch_analysis(a, s));
    }
    a.z_stage = 2;
    ProfScope rowfft(5, zrow_bytes + (double)p->n_pol * out_b * a.out_keep * p->N, s);
    HIPCHK(pfb::launch_analysis(a, s));
    return PFB_OK;
  }
  if (dd && !p->fused) {
    // the FIR of the N > 256 path reads the section: timed alone as class 4, which names it
    ProfScope fir(4, (double)p->n_pol * in_b * in_samples + zrow_bytes, s);
    HIPCHK(pfb::launch_analysis(a, s));
    return PFB_OK;
  }
  HIPCHK(pfb::launch_analysis(a, s));
  return PFB_OK;
}

extern "C" {

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
                    &p->stage_out, &p->dada_stage, &p->quant_prod, &p->quant_mom, &p->quant_stats, &p->qin_mom, &p->qin_stats})
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

// The DADA section of an analysis call (pfb_analysis_execute_dada, pfb_filterbank_execute_dada:
// n samples x 1 channel x the plan's n_pol x ndim values of nbit) is read in place by the launch
static bool section_fusable(const pfb_analysis_plan* p, const DadaSection& sec) {
  return !sec.force_staged && analysis_dada_fusable(p, sec.base, sec.nbit, sec.ndim, sec.order);
}

}  // extern "C"

// (pfb_dada_unpack; a LowCBF section from a heap boundary only)
pfb_status pfb::host::section_unpack(const pfb_analysis_plan* p, const DadaSection& sec, int64_t t0, int64_t n,
                                     float2* dst, int64_t dps, hipStream_t s) {
  if (n <= 0) return PFB_OK;
  const char* src = static_cast<const char*>(sec.base) + t0 * p->n_pol * sec.ndim * (sec.nbit / 8);
  return pfb_dada_unpack(src, sec.nbit, sec.ndim, sec.order, n, 1, p->n_pol, reinterpret_cast<pfb_cf32*>(dst), dps,
                         s);
}

// ====================================================================== the input quantiser
// The input quantiser of one call (pfb_api.h, pfb_analysis_set_input_quantiser).  `on`: the
// plan's quantiser applies to this call; `fused`: the launch rounds at the load, else the
// quantising copy (STAGED); stats: the plan's block once qin_moments has enqueued the scale, null
// for a round-only call (scale 1).
struct QinCall {
  bool on = false, fused = false;
  const double* stats = nullptr;
};

// the plan is on the streaming kernel (the FUSED side's kernel; section_kernel_shape's LowCBF rule)
static bool analysis_on_stream_kernel(const pfb_analysis_plan* p) {
  pfb::AnalysisArgs a;
  return section_kernel_shape(p, a) && pfb::analysis_takes_offset(a);
}

// the one-shot passes read such a section where it lies (else it is unpacked first)
static bool section_readable(const DadaSection& sec) {
  return sec.ndim == 2 && sec.order == PFB_DADA_TFP && (sec.nbit == 8 || sec.nbit == 16 || sec.nbit == 32) &&
         reinterpret_cast<uintptr_t>(sec.base) % (size_t)(sec.nbit / 4) == 0;
}

// The quantiser's own checks for a call of n new samples per polarisation, and its path:
// fused_ok says whether this call can round at the load.  No launch, no state change.
static pfb_status qin_check(const pfb_analysis_plan* p, int64_t n, bool fused_ok, QinCall& qc) {
  qc = QinCall{};
  if (!p->qin_on) return PFB_OK;
  if (p->qin_rms > 0 && n > 0 && n * p->n_pol < 2)
    return fail(PFB_ERR_INVALID_ARG, "input quantiser: the variance needs at least two samples");
  if (p->qin_mode == PFB_QUANTISER_MOMENTS_FUSED && !fused_ok)
    return fail(PFB_ERR_UNSUPPORTED, "input quantiser FUSED: this call does not read its new samples in place "
                                     "on the streaming analysis kernel");
  qc.on = true;
  qc.fused = fused_ok && p->qin_mode != PFB_QUANTISER_MOMENTS_STAGED;
  return PFB_OK;
}

// The scale of the new samples `src` into the plan's block: the partial sums and the finish
// launch.  Round only (rms <= 0) and a call without samples take scale 1: nothing is launched.
static pfb_status qin_moments(pfb_analysis_plan* p, QinCall& qc, const pfb::QinSrc& src, hipStream_t s) {
  qc.stats = nullptr;
  p->qin_scale_dev = false;
  if (p->qin_rms <= 0 || src.n <= 0) return PFB_OK;
  const int64_t slots = pfb::input_moments_slots(src);
  HIPCHK(p->qin_mom.ensure((size_t)slots * 3 * sizeof(double)));
  HIPCHK(p->qin_stats.ensure(4 * sizeof(double)));
  HIPCHK(pfb::launch_input_moments(src, p->qin_mom.as<double>(), s));
  HIPCHK(pfb::launch_moments_finish(p->qin_mom.as<double>(), slots, (double)src.n * src.n_pol, p->qin_rms,
                                    p->qin_stats.as<double>(), s));
  qc.stats = p->qin_stats.as<double>();
  p->qin_scale_dev = true;
  return PFB_OK;
}

static pfb::QinSrc qin_cf32(const pfb_analysis_plan* p, const float2* x, int64_t ps, int64_t n) {
  return pfb::QinSrc{x, 0, ps, n, p->n_pol};
}
// samples [t0, t0 + n) of a readable section
static pfb::QinSrc qin_section(const pfb_analysis_plan* p, const DadaSection& sec, int64_t t0, int64_t n) {
  return pfb::QinSrc{static_cast<const char*>(sec.base) + t0 * p->n_pol * (sec.nbit / 4), sec.nbit, 0, n, p->n_pol};
}

// STAGED: the new samples, rounded, as packed cf32 at dst[pol][0, n) (pol stride dps) — the
// moments of the samples where they lie and the quantising copy; a section the passes do not
// read, or host memory (kind HostToDevice), is unpacked or copied there first and rounded in place
static pfb_status qin_stage(pfb_analysis_plan* p, QinCall& qc, const float2* in, int64_t in_ps, const DadaSection* sec,
                            int64_t n, hipMemcpyKind kind, float2* dst, int64_t dps, hipStream_t s) {
  if (n <= 0) return qin_moments(p, qc, qin_cf32(p, dst, dps, 0), s);
  pfb::QinSrc src = qin_cf32(p, in, in_ps, n);
  if (sec && section_readable(*sec)) {
    src = qin_section(p, *sec, 0, n);
  } else if (sec || kind != hipMemcpyDeviceToDevice) {
    if (sec) {
      const pfb_status st = section_unpack(p, *sec, 0, n, dst, dps, s);
      if (st != PFB_OK) return st;
    } else {
      HIPCHK(copy_pols(dst, dps, in, in_ps, n, p->n_pol, kind, s));
    }
    src = qin_cf32(p, dst, dps, n);
  }
  const pfb_status st = qin_moments(p, qc, src, s);
  if (st != PFB_OK) return st;
  HIPCHK(pfb::launch_quantise_copy(src, qc.stats, dst, dps, s));
  return PFB_OK;
}

extern "C" {

// pfb_analysis_execute; sec: the series are a DADA section (device memory) instead of `in`;
// od: the product goes out as a DADA section (device memory, FUSED) instead of `out`, which
// then only has to pass the checks
static pfb_status analysis_exec(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, const DadaSection* sec,
                                int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                                int32_t mem, void* stream, const AnaOut* od = nullptr, AnaMoments* mo = nullptr) {
  if (sec) in = static_cast<const pfb_cf32*>(sec->base);
  if (!p || (!in && n_dat > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n_dat < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_dat");
  HIPCHK(hipSetDevice(p->device));
  p->last_dada = PFB_DADA_INPUT_NONE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t K = analysis_K(p, n_dat);
  PadConsume pad_once{&p->lowcbf_pad};
  if (n_out) *n_out = K;
  // the input quantiser: FUSED where the streaming kernel reads the new samples in place and
  // stores the plain cf32 product (with or without its moments)
  const bool sec_fus = sec && section_fusable(p, *sec);
  QinCall qc;
  {
    const bool fused_ok = analysis_on_stream_kernel(p) && mem == PFB_MEM_DEVICE && (!sec || sec_fus) && !od;
    const pfb_status st = qin_check(p, n_dat, fused_ok, qc);
    if (st != PFB_OK) return st;
  }
  const int qin_path = !qc.on ? PFB_INPUT_QUANTISER_NONE : qc.fused ? PFB_INPUT_QUANTISER_FUSED : PFB_INPUT_QUANTISER_STAGED;
  if (K == 0) {
    pad_once.accept();
    // (no launch: the path the section's rows would have taken)
    if (sec) p->last_dada = sec_fus && (!qc.on || qc.fused) ? PFB_DADA_INPUT_FUSED : PFB_DADA_INPUT_STAGED;
    p->last_qin = qin_path;
    p->qin_scale_dev = false;
    return PFB_OK;
  }
  if (!out) return fail(PFB_ERR_INVALID_ARG, "null output");
  if (cap < K) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                           (long long)cap, (long long)K);
  if (mem == PFB_MEM_DEVICE && ((!sec && in_ps < n_dat) || out_ps < K * p->C))
    return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  pad_once.accept();
  p->last_qin = qin_path;
  // all K rows of the n_dat samples, into the caller's buffer (or the section od)
  AnaLaunch l;
  l.n_dat = n_dat;
  l.out = (float2*)out;
  l.out_ps = out_ps;
  l.K_end = l.K_total = K;
  l.dada_out = od;
  l.moments = mo;
  AnaQin aq;
  if (qc.on && !qc.fused && mem == PFB_MEM_DEVICE) {
    // STAGED: the rounded samples into stage_in, then the plan's cf32 path on them
    HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n_dat * sizeof(float2)));
    if (sec) p->last_dada = PFB_DADA_INPUT_STAGED;
    const pfb_status st = qin_stage(p, qc, (const float2*)in, in_ps, sec, n_dat, hipMemcpyDeviceToDevice,
                                    p->stage_in.as<float2>(), n_dat, s);
    if (st != PFB_OK) return st;
    l.in = p->stage_in.as<float2>();
    l.in_ps = n_dat;
    return analysis_run(p, l, s);
  }
  if (qc.fused) {
    // FUSED: the moments of the samples where they lie; the launch rounds at the load
    const pfb_status st =
        qin_moments(p, qc, sec ? qin_section(p, *sec, 0, n_dat) : qin_cf32(p, (const float2*)in, in_ps, n_dat), s);
    if (st != PFB_OK) return st;
    aq.stats = qc.stats;
    l.qin = &aq;
  }
  if (sec) {
    const AnaDada dd{sec->base, sec->nbit};
    if (sec_fus) {
      l.dada_in = &dd;
      return analysis_run(p, l, s);
    }
    HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n_dat * sizeof(float2)));
    p->last_dada = PFB_DADA_INPUT_STAGED;
    const pfb_status st = section_unpack(p, *sec, 0, n_dat, p->stage_in.as<float2>(), n_dat, s);
    if (st != PFB_OK) return st;
    l.in = p->stage_in.as<float2>();
    l.in_ps = n_dat;
    return analysis_run(p, l, s);
  }
  if (mem == PFB_MEM_DEVICE) {
    l.in = (const float2*)in;
    l.in_ps = in_ps;
    return analysis_run(p, l, s);
  }
  // host staging (synchronous)
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * n_dat * sizeof(float2)));
  HIPCHK(p->stage_out.ensure((size_t)p->n_pol * K * p->C * sizeof(float2)));
  if (qc.on) {
    // (STAGED: copied, then rounded in place)
    const pfb_status st = qin_stage(p, qc, (const float2*)in, in_ps, nullptr, n_dat, hipMemcpyHostToDevice,
                                    p->stage_in.as<float2>(), n_dat, s);
    if (st != PFB_OK) return st;
  } else
  HIPCHK(copy_pols(p->stage_in.as<float2>(), n_dat, (const float2*)in, in_ps, n_dat, p->n_pol,
                   hipMemcpyHostToDevice, s));
  l.in = p->stage_in.as<float2>();
  l.in_ps = n_dat;
  l.out = p->stage_out.as<float2>();
  l.out_ps = K * p->C;
  l.dada_out = nullptr;
  l.moments = nullptr;
  pfb_status st = analysis_run(p, l, s);
  if (st != PFB_OK) return st;
  HIPCHK(copy_pols((float2*)out, out_ps, p->stage_out.as<float2>(), K * p->C, K * p->C, p->n_pol,
                   hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

pfb_status pfb_analysis_execute(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                int64_t* n_out, int32_t mem, void* stream) {
  return cf32_output(p, analysis_exec(p, in, in_ps, nullptr, n_dat, out, out_ps, cap, n_out, mem, stream));
}

pfb_status pfb_analysis_execute_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                     int32_t order, int64_t n_dat, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                     int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = section_check(p, sec, n_dat);
  if (st != PFB_OK) return st;
  return cf32_output(p, analysis_exec(p, nullptr, 0, &sec, n_dat, out, out_ps, cap, n_out, PFB_MEM_DEVICE, stream));
}

int32_t pfb_analysis_last_dada_input(const pfb_analysis_plan* p) { return p ? p->last_dada : -1; }

// ====================================================================== FilterBank stream object
// The lengths of a stream call of n_in new samples on the plan's current state
struct FbLens {
  int64_t total;       // buffered + new samples: the series the call runs on
  int64_t K;           // rows it holds (the padded variant's circular shift spans all of them)
  int64_t Kt;          // rows returned: K trimmed to a multiple of nu (FilterBank.m:93-104)
  int64_t input_idat;  // samples consumed = Kt N de / nu (FilterBank.m:119-126)
  int64_t nb;          // the next carry: series[input_idat, total)
};
static FbLens fb_lens(const pfb_analysis_plan* p, int64_t n_in) {
  FbLens l{};
  l.total = p->buffered + n_in;
  l.K = analysis_K(p, l.total);
  l.Kt = l.K - (l.K % p->nu);
  l.input_idat = (l.Kt * p->N * p->de) / p->nu;
  l.nb = l.total - l.input_idat;
  return l;
}

// Where a launch of Krun rows stores them.  The caller's buffer when it has room for them in
// the capacity and in each pol's stride (a padded plan computes K rows for the circular shift
// and returns Kt: rows [Kt, K) are then scratch, pfb_filterbank_execute's contract; pols packed
// closer than Krun rows would have them land on the next pol's first rows), and always with a
// layout (`cap` is the Kt rows the strided entry point range-checked and out_ps is the
// layout's: the launch stores the shifted rows below Kt through it and drops rows [Kt, K),
// AnalysisArgs::out_keep).  Else — and for a host buffer (`staged`) — the plan's staging
// buffer, from which the call copies Kt rows out.
static pfb_status fb_rows_dst(pfb_analysis_plan* p, AnaLaunch& l, float2* out, int64_t out_ps, int64_t cap,
                              int64_t Krun, bool staged) {
  l.out = out;
  l.out_ps = out_ps;
  if (staged || (!l.lay && (Krun > cap || out_ps < Krun * p->C))) {
    HIPCHK(p->stage_out.ensure((size_t)p->n_pol * Krun * p->C * sizeof(float2)));
    l.out = p->stage_out.as<float2>();
    l.out_ps = Krun * p->C;
  }
  return PFB_OK;
}

// The size of either carry buffer for a carry of nb samples per pol: room for the longest carry
// a stream call leaves, so that the buffer is allocated once.  nb = total - Kt M with
// K - Kt < nu and total < P N + (K + 1) M (fb_lens, analysis_K; the padded and LowCBF counts
// are smaller), so nb < P N + nu M.  Sized by nb alone the two buffers, which swap, regrew
// from call to call, and a regrow frees the old block: hipFree waits for the whole device, so
// a stream call stalled behind every stream of the process (tests/test_gpu_streams.py).
static size_t fb_carry_bytes(const pfb_analysis_plan* p, int64_t nb) {
  const int64_t most = (int64_t)p->P * p->N + (int64_t)p->nu * p->M;
  return (size_t)p->n_pol * std::max(nb, most) * sizeof(float2);
}

// The call's tail: the next carry, nb samples per pol (packed cf32, whatever the input was),
// into `into` — unpacked from the section `sec` at sample t0, else copied from src (pol stride
// sps), else (neither) already written there by the launch — and the new count.  `into` is the
// plan's carry, or carry_next where the launch just enqueued still reads the carry: the two
// then swap.
// qf: a FUSED input-quantiser call — the tail is rounded as it is copied or unpacked.
static pfb_status fb_carry(pfb_analysis_plan* p, pfb_analysis_plan::DevBuf& into, int64_t nb, const DadaSection* sec,
                           int64_t t0, const float2* src, int64_t sps, hipStream_t s, const QinCall* qf = nullptr) {
  if (nb > 0) {
    HIPCHK(into.ensure(fb_carry_bytes(p, nb)));
    if (qf && (sec || src)) {
      HIPCHK(pfb::launch_quantise_copy(sec ? qin_section(p, *sec, t0, nb) : qin_cf32(p, src, sps, nb), qf->stats,
                                       into.as<float2>(), nb, s));
    } else if (sec) {
      const pfb_status st = section_unpack(p, *sec, t0, nb, into.as<float2>(), nb, s);
      if (st != PFB_OK) return st;
    } else if (src) {
      HIPCHK(copy_pols(into.as<float2>(), nb, src, sps, nb, p->n_pol, hipMemcpyDeviceToDevice, s));
    }
    if (&into == &p->carry_next) std::swap(p->carry, p->carry_next);
  }
  p->buffered = std::max<int64_t>(nb, 0);
  return PFB_OK;
}

// sec: the new samples are a DADA section (device memory) instead of `in`.  The carry stays
// packed cf32, so cf32 and DADA calls may alternate on one plan.
// od: the rows go out as a DADA section (device memory, FUSED: a plan on the streaming kernel)
// instead of `out`, which then only has to pass the checks.
static pfb_status filterbank_exec(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_in,
                                  pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out, int32_t mem,
                                  void* stream, const OutLayout* lay, const DadaSection* sec = nullptr,
                                  const AnaOut* od = nullptr, AnaMoments* mo = nullptr) {
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
  // (not const: a STAGED input-quantiser call that rounds its samples into stage_in goes on as
  // the cf32 device call on them)
  bool fus = sec && section_fusable(p, *sec);
  const AnaDada dd_{sec ? sec->base : nullptr, sec ? sec->nbit : 0};
  const AnaDada* dd = fus ? &dd_ : nullptr;
  const int last_dada = !sec ? PFB_DADA_INPUT_NONE : PFB_DADA_INPUT_STAGED;  // (a fused launch sets FUSED)
  const FbLens len = fb_lens(p, n_in);
  const int64_t B = p->buffered, total = len.total, K = len.K, Kt = len.Kt, input_idat = len.input_idat,
                nb = len.nb;
  // rows are independent except for the padded variant's circular shift over all K rows:
  // the others compute just the Kt kept rows
  const int64_t Krun = p->variant == pfb::kPadded ? K : Kt;
  const hipMemcpyKind kin = mem == PFB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  // the strides of device buffers are the caller's: checked like pfb_analysis_execute's,
  // before any state changes (`lay`: out_ps belongs to the strided layout, range-checked
  // by pfb_filterbank_execute_strided)
  if (mem == PFB_MEM_DEVICE && (in_ps < n_in || (!lay && out_ps < Kt * p->C)))
    return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  // what every path's launch shares: Krun of the call's K rows, the layout, the sections
  AnaLaunch l;
  l.lay = lay;
  l.K_end = Krun;
  l.K_total = K;
  l.dada_out = od;
  l.moments = mo;
  // The conditions of the two carry paths below, as functions of the input side: (a section, read
  // in place) — the input quantiser asks them for the call as it is and, STAGED, for the cf32
  // device call on the rounded samples.
  // (split: the streaming kernel's register window holds the carry — the bound is explained below)
  static const bool no_split = pfb::knob("PFB_FB_NO_SPLIT") != nullptr;  // A/B
  const int64_t win = ((int64_t)p->de * (16 / p->nu) + p->P) * p->N;
  auto split_ok = [&](bool has_sec, bool sec_fused) {
    const bool lcbf_sec = has_sec && sec_fused && p->variant == pfb::kLowCbf;
    return !no_split && mem == PFB_MEM_DEVICE && B > 0 && B <= win &&
           ((p->variant == pfb::kBunton && analysis_offset_ok(p)) || lcbf_sec) && input_idat >= B &&
           p->lowcbf_pad == false && (!has_sec || sec_fused);
  };
  auto fused_carry_ok = [&](bool has_sec) {
    return !has_sec && !od && !mo && mem == PFB_MEM_DEVICE && B > 0 && !p->lowcbf_pad && p->fused &&
           analysis_fused_carry_ok(p) && input_idat >= B && Kt > 0;
  };
  // The input quantiser (pfb_api.h).  FUSED: the streaming kernel reads the new samples in place
  // (the split launch, or nothing buffered) and stores the plain cf32 product.
  QinCall qc;
  {
    const bool in_place_now = B == 0 && mem == PFB_MEM_DEVICE && (!sec || fus);
    const bool fused_ok = analysis_on_stream_kernel(p) && !od && !lay && (split_ok(sec != nullptr, fus) || in_place_now);
    const pfb_status st = qin_check(p, n_in, fused_ok, qc);
    if (st != PFB_OK) return st;
  }
  // (a call the capacity check below rejects: nothing is launched for the quantiser either)
  if (Kt > cap) qc.on = qc.fused = false;
  if (qc.on || !p->qin_on) p->last_qin = !qc.on ? PFB_INPUT_QUANTISER_NONE : qc.fused ? PFB_INPUT_QUANTISER_FUSED : PFB_INPUT_QUANTISER_STAGED;
  const QinCall* qfused = qc.fused ? &qc : nullptr;
  AnaQin aq;
  // STAGED, when the call on the rounded samples reads them in place (a carry path, or nothing
  // buffered): rounded into stage_in, and the call goes on as the cf32 device call on them.
  // (A call that concatenates rounds them into the work buffer, behind the carry: below.)
  bool qin_staged_in = false;
  if (qc.on && !qc.fused && mem == PFB_MEM_DEVICE && (B == 0 || split_ok(false, false) || fused_carry_ok(false))) {
    HIPCHK(p->stage_in.ensure((size_t)p->n_pol * std::max<int64_t>(n_in, 1) * sizeof(float2)));
    const pfb_status st = qin_stage(p, qc, (const float2*)in, in_ps, sec, n_in, hipMemcpyDeviceToDevice,
                                    p->stage_in.as<float2>(), std::max<int64_t>(n_in, 1), s);
    if (st != PFB_OK) return st;
    in = p->stage_in.as<pfb_cf32>();
    in_ps = std::max<int64_t>(n_in, 1);
    sec = nullptr;
    fus = false;
    dd = nullptr;
    qin_staged_in = true;
  } else if (qc.fused) {
    const pfb_status st =
        qin_moments(p, qc, sec ? qin_section(p, *sec, 0, n_in) : qin_cf32(p, (const float2*)in, in_ps, n_in), s);
    if (st != PFB_OK) return st;
    aq.stats = qc.stats;
    l.qin = &aq;
  }
  {
    // Carry without the concatenation copy (streaming analysis kernel, device input): when
    // the new carry starts in the new input (input_idat >= B), ONE launch reads the new
    // input in place with the carried B samples as a read offset (AnalysisArgs::pad), and
    // the carried samples themselves through a second descriptor in its first register
    // window (AnalysisArgs::pre).  The result is the same per row as the concatenated run
    // (same kernel, same samples).
    // (split_ok, above)
    // the streaming kernel's register window (win): DE (16 / NU) new rows per step + P (its first
    // window holds every carried sample a workgroup's rows read when B fits in it —
    // launch_stream checks the same bound).  A stream call leaves at most P N + NU M - 1
    // samples behind (total - Kt M with K - Kt < NU), which is below the window's
    // P N + 16 M for every NU <= 16: every carry this object makes fits
    // (tests/test_stream_model.py enumerates it); a longer one would concatenate below.
    // (a DADA section: fused only, else staged; a fused LowCBF stream call takes this path
    // too — its cf32 call concatenates)
    const bool lcbf_dd = dd && p->variant == pfb::kLowCbf;
    if (split_ok(sec != nullptr, fus)) {
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
      CarryOut co{nullptr, input_idat - B, nb, nb};
      if (nb > 0) {
        HIPCHK(p->carry_next.ensure(fb_carry_bytes(p, nb)));
        co.dst = p->carry_next.as<float2>();
      }
      l.in = (const float2*)in;
      l.in_ps = in_ps;
      l.n_dat = n_in;
      l.pad = B;
      l.pre = p->carry.as<float2>();
      l.out = (float2*)out;
      l.out_ps = out_ps;
      l.K_end = Kt;
      // (the LowCBF instantiation has no carry copy: unpacked by a launch behind it)
      l.carry_out = nb > 0 && !lcbf_dd ? &co : nullptr;
      l.dada_in = dd;
      const pfb_status st = analysis_run(p, l, s);
      if (st != PFB_OK) return st;
      // (with the input quantiser FUSED: rounded as it is unpacked)
      return fb_carry(p, p->carry_next, nb, lcbf_dd ? sec : nullptr, input_idat - B, nullptr, 0, s, qfused);
    }
  }
  {
    // Carry without the concatenation copy (fused one-launch kernels: N <= 256 shapes the
    // streaming kernel does not take, e.g. a padded cascade's stage 2): the kernel stages each
    // row's input span from the carry (`pre`, the first B samples of the series) and the input
    // in place (round 6; the SKA-Mid padded cascade copied its 613 MB of stage-2 series here).
    // (a layout — pfb_filterbank_execute_strided on a padded plan; the Bunton plans it admits
    // take the streaming kernel above — goes straight to `out`: no scratch rows and no staging
    // buffer, fb_rows_dst)
    if (fused_carry_ok(sec != nullptr)) {
      p->last_dada = last_dada;
      if (n_out) *n_out = Kt;
      if (Kt > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                                (long long)cap, (long long)Kt);
      pfb_status st = fb_rows_dst(p, l, (float2*)out, out_ps, cap, Krun, false);
      if (st != PFB_OK) return st;
      l.in = (const float2*)in;
      l.in_ps = in_ps;
      l.n_dat = n_in;
      l.pad = B;
      l.pre = p->carry.as<float2>();
      st = analysis_run(p, l, s);
      if (st != PFB_OK) return st;
      if (l.out != (float2*)out)
        HIPCHK(copy_pols((float2*)out, out_ps, l.out, l.out_ps, Kt * p->C, p->n_pol, hipMemcpyDeviceToDevice, s));
      // carry = series[input_idat, total): all of it in the new input; into the second carry
      // buffer (the kernel just enqueued still reads the first)
      return fb_carry(p, p->carry_next, nb, nullptr, 0, (const float2*)in + (input_idat - B), in_ps, s);
    }
  }
  // input = cat(3, input_buffer, input)   (FilterBank.m:85-88); with nothing buffered and
  // the input already on the device the kernels read it in place (no copy)
  const float2* w;
  int64_t wps;
  const bool in_place = B == 0 && mem == PFB_MEM_DEVICE && (!sec || fus);
  if (in_place) {
    w = (const float2*)in;  // (a fused section: read through dd, `w` is not dereferenced)
    wps = in_ps;
  } else {
    dd = nullptr;
    HIPCHK(p->work.ensure((size_t)p->n_pol * std::max<int64_t>(total, 1) * sizeof(float2)));
    float2* wk = p->work.as<float2>();
    HIPCHK(copy_pols(wk, total, p->carry.as<float2>(), B, B, p->n_pol, hipMemcpyDeviceToDevice, s));
    if (qc.on && !qin_staged_in) {
      // (the input quantiser, STAGED: the quantising copy stands where the call copies or
      // unpacks its new samples)
      const pfb_status st = qin_stage(p, qc, (const float2*)in, in_ps, sec, n_in, kin, wk + B, total, s);
      if (st != PFB_OK) return st;
    } else if (sec) {
      // (unpacked straight behind the carry: no second copy)
      const pfb_status st = section_unpack(p, *sec, 0, n_in, wk + B, total, s);
      if (st != PFB_OK) return st;
    } else {
      HIPCHK(copy_pols(wk + B, total, (const float2*)in, in_ps, n_in, p->n_pol, kin, s));
    }
    w = wk;
    wps = total;
  }
  PadConsume pad_once{&p->lowcbf_pad};
  if (n_out) *n_out = Kt;
  if (Kt > cap) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld rows",
                            (long long)cap, (long long)Kt);
  pad_once.accept();
  p->last_dada = dd ? PFB_DADA_INPUT_FUSED : last_dada;
  if (Kt > 0) {
    // straight into the caller's buffer where fb_rows_dst finds room, else through the staging
    // buffer and a copy (round 6: the SKA-Mid cascade's stage 2 lost a 244-us copy per call)
    // (a section: the launch stores the Kt kept rows itself — of a padded call's K computed
    // rows, rows [Kt, K) are not made — so there is no staging buffer and no copy)
    pfb_status st = PFB_OK;
    if (od) {
      l.out = (float2*)out;
      l.out_ps = out_ps;
      l.dada_keep = Kt;
    } else {
      st = fb_rows_dst(p, l, (float2*)out, out_ps, cap, Krun, mem == PFB_MEM_HOST);
    }
    if (st != PFB_OK) return st;
    l.in = w;
    l.in_ps = wps;
    l.n_dat = total;
    l.dada_in = dd;
    st = analysis_run(p, l, s);
    if (st != PFB_OK) return st;
    if (l.out != (float2*)out) {
      const hipMemcpyKind ko = mem == PFB_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
      HIPCHK(copy_pols((float2*)out, out_ps, l.out, l.out_ps, Kt * p->C, p->n_pol, ko, s));
    }
  }
  // carry = input(:,:,input_idat+1:end)   (FilterBank.m:119-126); a separate buffer, it aliases
  // nothing in `work`.  (a fused section: its tail, unpacked)
  // (the input quantiser FUSED — read in place, nothing buffered: rounded as it is copied)
  const pfb_status st = fb_carry(p, p->carry, nb, dd ? sec : nullptr, input_idat, w + input_idat, wps, s, qfused);
  if (st != PFB_OK) return st;
  if (mem == PFB_MEM_HOST) HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

pfb_status pfb_filterbank_execute_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                       int32_t order, int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                       int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = section_check(p, sec, n_in);
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
  return fb_lens(p, n_in).Kt;
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
static pfb_status analysis_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps, const DadaSection* sec_in,
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
    const pfb_status st = section_check(p, *sec_in, n);
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
  DadaSection sec{};
  if (sec_in) {
    sec = *sec_in;
    // (the streaming DADA-store kernels read cf32, a section of the output's NBIT, or an integer
    // section when they write NBIT 32.  A 4096-channel plan's FIR reads the section and its row
    // FFT stores the other one, in launches of their own: any pair of NBITs)
    if (fused && analysis_on_stream_kernel(p) && !pfb::dadaout_reads_dada(sec.nbit, nbit)) sec.force_staged = true;
  }
  const DadaSection* sp = sec_in ? &sec : nullptr;
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
  if (st == PFB_OK) {
    p->last_dada_out = fused ? PFB_DADA_OUTPUT_FUSED : PFB_DADA_OUTPUT_STAGED;
    p->last_quant = PFB_QUANTISER_NONE;
  }
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
  const DadaSection sec{in, nbit, ndim, order};
  return analysis_to_dada(p, nullptr, 0, &sec, n_dat, out, out_nbit, out_scale, cap_bytes, n_out, stream, false);
}

pfb_status pfb_filterbank_execute_dada_to_dada(pfb_analysis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                               int32_t order, int64_t n_in, void* out, int32_t out_nbit,
                                               float out_scale, int64_t cap_bytes, int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return analysis_to_dada(p, nullptr, 0, &sec, n_in, out, out_nbit, out_scale, cap_bytes, n_out, stream, true);
}

int32_t pfb_analysis_last_dada_output(const pfb_analysis_plan* p) { return p ? p->last_dada_out : -1; }

// The quantised to-DADA calls (pfb_api.h): every check here, before the callee launches or
// changes the stream state; the cf32 product into the plan's buffer — FUSED: by the streaming
// kernel's moments instantiation, which leaves the partial sums; STAGED: by the plan's cf32 path,
// then moments_partials_kernel — then the finish and the pack launch, all on the caller's stream.
static pfb_status analysis_quantised(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                     const DadaSection* sec_in, int64_t n, double rms, void* out, int32_t nbit,
                                     float oscale, int64_t cap_bytes, int64_t* n_out, double* scale, void* stream,
                                     bool stream_call) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (nbit != 8 && nbit != 16 && nbit != 32 && nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "output NBIT must be 8, 16, 32 or 64");
  if (!std::isfinite(oscale)) return fail(PFB_ERR_INVALID_ARG, "output scale is not finite");
  if (!std::isfinite(rms)) return fail(PFB_ERR_INVALID_ARG, "quantiser rms is not finite");
  if (reinterpret_cast<uintptr_t>(out) % (size_t)(nbit / 8) != 0)
    return fail(PFB_ERR_INVALID_ARG, "output section not aligned to its NBIT");
  if (sec_in) {
    const pfb_status st = section_check(p, *sec_in, n);
    if (st != PFB_OK) return st;
  }
  if (!(sec_in ? sec_in->base : (const void*)in) && n > 0) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (n < 0) return fail(PFB_ERR_INVALID_ARG, "negative sample count");
  if (!sec_in && in_ps < n) return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  // (K and rows: analysis_to_dada's)
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
  // (the moments instantiation is the streaming kernel's: a 4096-channel plan, whose row FFT
  // stores a plain section itself, has none)
  const bool fusable = analysis_on_stream_kernel(p);
  if (p->quant_mode == PFB_QUANTISER_MOMENTS_FUSED && !fusable)
    return fail(PFB_ERR_UNSUPPORTED, "quantiser moments FUSED: the plan is not on the streaming analysis kernel");
  const bool fused = fusable && p->quant_mode != PFB_QUANTISER_MOMENTS_STAGED;
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  // all K computed rows have room (a padded stream call computes K and returns `rows`)
  HIPCHK(p->quant_prod.ensure((size_t)p->n_pol * std::max<int64_t>(K, 1) * p->C * sizeof(float2)));
  HIPCHK(p->quant_stats.ensure(4 * sizeof(double)));
  AnaMoments mo;
  AnaMoments* mp = fused && rms > 0 ? &mo : nullptr;
  pfb_cf32* o = p->quant_prod.as<pfb_cf32>();
  const pfb_status st =
      stream_call ? filterbank_exec(p, in, in_ps, n, o, K * p->C, K, n_out, PFB_MEM_DEVICE, stream, nullptr, sec_in,
                                    nullptr, mp)
                  : analysis_exec(p, in, in_ps, sec_in, n, o, K * p->C, K, n_out, PFB_MEM_DEVICE, stream, nullptr, mp);
  if (st != PFB_OK) return st;
  if (scale) *scale = 1.0;
  if (rows > 0) {
    const float2* prod = p->quant_prod.as<float2>();
    const int64_t cnt = rows * p->C;  // per polarisation
    const double* stats = nullptr;
    if (rms > 0) {
      int64_t slots = mo.slots;
      if (!mp) {
        slots = pfb::moments_partials_slots(cnt, p->n_pol);
        HIPCHK(p->quant_mom.ensure((size_t)slots * 3 * sizeof(double)));
        HIPCHK(pfb::launch_moments_partials(prod, K * p->C, cnt, p->n_pol, p->quant_mom.as<double>(), s));
      }
      HIPCHK(pfb::launch_moments_finish(p->quant_mom.as<double>(), slots, (double)cnt * p->n_pol, rms,
                                        p->quant_stats.as<double>(), s));
      stats = p->quant_stats.as<double>();
    }
    HIPCHK(pfb::launch_quantise_pack(prod, K * p->C, cnt, p->n_pol, stats, oscale, out, nbit, s));
    if (scale && stats) {
      HIPCHK(hipMemcpyAsync(scale, stats + 3, sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
    }
  }
  p->last_quant = fused ? PFB_QUANTISER_FUSED : PFB_QUANTISER_STAGED;
  p->last_dada_out = PFB_DADA_OUTPUT_NONE;
  return PFB_OK;
}

pfb_status pfb_analysis_execute_quantised_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                  int64_t n_dat, double rms, void* out, int32_t out_nbit,
                                                  float out_scale, int64_t cap_bytes, int64_t* n_out, double* scale,
                                                  void* stream) {
  return analysis_quantised(p, in, in_ps, nullptr, n_dat, rms, out, out_nbit, out_scale, cap_bytes, n_out, scale,
                            stream, false);
}

pfb_status pfb_filterbank_execute_quantised_to_dada(pfb_analysis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                    int64_t n_in, double rms, void* out, int32_t out_nbit,
                                                    float out_scale, int64_t cap_bytes, int64_t* n_out, double* scale,
                                                    void* stream) {
  return analysis_quantised(p, in, in_ps, nullptr, n_in, rms, out, out_nbit, out_scale, cap_bytes, n_out, scale,
                            stream, true);
}

pfb_status pfb_analysis_execute_dada_quantised_to_dada(pfb_analysis_plan* p, const void* in, int32_t nbit,
                                                       int32_t ndim, int32_t order, int64_t n_dat, double rms,
                                                       void* out, int32_t out_nbit, float out_scale,
                                                       int64_t cap_bytes, int64_t* n_out, double* scale,
                                                       void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return analysis_quantised(p, nullptr, 0, &sec, n_dat, rms, out, out_nbit, out_scale, cap_bytes, n_out, scale,
                            stream, false);
}

pfb_status pfb_filterbank_execute_dada_quantised_to_dada(pfb_analysis_plan* p, const void* in, int32_t nbit,
                                                         int32_t ndim, int32_t order, int64_t n_in, double rms,
                                                         void* out, int32_t out_nbit, float out_scale,
                                                         int64_t cap_bytes, int64_t* n_out, double* scale,
                                                         void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return analysis_quantised(p, nullptr, 0, &sec, n_in, rms, out, out_nbit, out_scale, cap_bytes, n_out, scale,
                            stream, true);
}

pfb_status pfb_analysis_set_quantiser_moments(pfb_analysis_plan* p, int32_t mode) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (mode != PFB_QUANTISER_MOMENTS_AUTO && mode != PFB_QUANTISER_MOMENTS_FUSED &&
      mode != PFB_QUANTISER_MOMENTS_STAGED)
    return fail(PFB_ERR_INVALID_ARG, "unknown quantiser moments mode %d", mode);
  p->quant_mode = mode;
  return PFB_OK;
}

int32_t pfb_analysis_last_quantiser(const pfb_analysis_plan* p) { return p ? p->last_quant : -1; }

pfb_status pfb_analysis_set_input_quantiser(pfb_analysis_plan* p, int32_t enable, double rms) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (!std::isfinite(rms)) return fail(PFB_ERR_INVALID_ARG, "input quantiser rms is not finite");
  p->qin_on = enable != 0;
  p->qin_rms = rms;
  return PFB_OK;
}

pfb_status pfb_analysis_set_input_quantiser_mode(pfb_analysis_plan* p, int32_t mode) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (mode != PFB_QUANTISER_MOMENTS_AUTO && mode != PFB_QUANTISER_MOMENTS_FUSED &&
      mode != PFB_QUANTISER_MOMENTS_STAGED)
    return fail(PFB_ERR_INVALID_ARG, "unknown input quantiser mode %d", mode);
  p->qin_mode = mode;
  return PFB_OK;
}

int32_t pfb_analysis_last_input_quantiser(const pfb_analysis_plan* p) { return p ? p->last_qin : -1; }

pfb_status pfb_analysis_last_input_scale(pfb_analysis_plan* p, double* scale, void* stream) {
  if (!p || !scale) return fail(PFB_ERR_INVALID_ARG, "null argument");
  *scale = 1.0;
  if (!p->qin_scale_dev) return PFB_OK;
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(scale, p->qin_stats.as<double>() + 3, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}


int64_t pfb_filterbank_buffered(const pfb_analysis_plan* p) { return p ? p->buffered : -1; }

pfb_status pfb_filterbank_reset(pfb_analysis_plan* p) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  p->buffered = 0;
  p->lowcbf_pad = p->variant == pfb::kLowCbf;
  return PFB_OK;
}

}  // extern "C"
