// pfb_api_synthesis.hip — the synthesis half of the C ABI (include/pfb_api.h): the synthesis
// plan (twiddle / deripple / window tables computed in double and rounded once to float), the
// channel-IFFT + block-kernel launches, pfb_synthesis_execute* and the InverseFilterBank stream
// object (pfb_inverse_filterbank_*: carry-over buffers and kernel dispatch).
#include <cmath>
#include <cstdlib>

#include "pfb_host.hpp"

using namespace pfb::host;

// ====================================================================== synthesis plan
void pfb::host::zkey_clear(pfb_synthesis_plan* p) {
  p->zkey_plan = 0;
  std::fill(p->zkey, p->zkey + 5, (int64_t)-1);
  p->zkey_x = nullptr;
  p->zkey_xps = -1;
}

static void hann_sym(int L, std::vector<double>& h) {
  h.resize((size_t)L);
  if (L == 1) {
    h[0] = 1.0;
    return;
  }
  for (int n = 0; n < L; ++n) h[(size_t)n] = 0.5 * (1.0 - std::cos(2.0 * M_PI * n / (L - 1)));
}

int64_t pfb::host::synth_blocks(const pfb_synthesis_plan* p, int64_t n_dat) {
  const int64_t b = floordiv(n_dat - 2 * (int64_t)p->Ov, p->keep);
  return std::max<int64_t>(b, 0);
}

// the request as the block kernels take it
pfb::SynthBlockArgs pfb::host::synth_args(const pfb_synthesis_plan* p, const SynthLaunch& l) {
  pfb::SynthBlockArgs a{};
  if (l.fir) {
    a.fir_x = l.fir->x;
    a.fir_x_pol_stride = l.fir->x_ps;
    a.fir_n_dat = l.fir->n_dat;
    a.fir_g = l.fir->g;
    a.fir_q0 = l.fir->q0;
    a.fir_nu = l.fir->nu;
    a.fir_de = l.fir->de;
    a.fir_pe = l.fir->pe;
  }
  a.Z = l.Z;
  a.z_pol_stride = l.z_ps;
  a.out = l.o.out;
  a.out_pol_stride = l.o.out_ps;
  a.block0 = l.b0;
  a.n_blocks = (int)l.nb;
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
  a.out_limit = l.o.out_limit;
  a.ranges = p->ranges;
  a.no_reuse = p->no_reuse;
  a.xcd = p->xcd;
  a.timing_mask = p->timing_mask;
  a.zblk = l.zblk;
  a.dout = l.o.dada.base;
  a.dout_nbit = l.o.dada.nbit;
  a.dout_scale = l.o.dada.scale;
  return a;
}

pfb_status pfb::host::synthesis_blocks(pfb_synthesis_plan* p, const SynthLaunch& l, hipStream_t s) {
  const pfb::SynthBlockArgs a = synth_args(p, l);
  p->last_stage1 = l.fir ? PFB_STAGE1_RECOMPUTED : PFB_STAGE1_STORED;
  {
    ProfScope ps(2, (double)p->n_pol * (l.nb * p->keep * p->N * 8.0 + l.nb * p->Lkeep * 8.0), s);
    HIPCHK(pfb::launch_synth_block(a, s));
  }
  return PFB_OK;
}

pfb_status SynthRows::chan_in(int64_t r, int64_t n, pfb::ChanIfftArgs& c) {
  switch (kind) {
    case DADA:
      dada.t0 = r;
      if (r < 0 || r + n > rows) return fail(PFB_ERR_INVALID_ARG, "rows outside the DADA section");
      c.dada = &dada;
      plan->last_dada = PFB_DADA_INPUT_FUSED;
      break;
    case STRIDED:
      strided.t0 = r;
      if (r < 0 || r + n > rows) return fail(PFB_ERR_INVALID_ARG, "rows outside the strided input");
      c.strided = &strided;
      plan->last_strided = PFB_STRIDED_INPUT_IN_PLACE;
      break;
    case PACKED:
      c.in = base + r * plan->N;
      c.in_pol_stride = ps;
      break;
  }
  return PFB_OK;
}

hipError_t SynthRows::copy_to(int64_t r, int64_t n, float2* dst, int64_t dps, hipStream_t s) const {
  pfb_synthesis_plan* p = plan;
  switch (kind) {
    case DADA: {
      pfb::DadaIn d = dada;
      d.t0 = r;
      if (p->last_dada == PFB_DADA_INPUT_NONE) p->last_dada = PFB_DADA_INPUT_STAGED;
      return pfb::launch_dada_unpack_rows(d, n, p->N, p->n_pol, dst, dps, s);
    }
    case STRIDED: {
      pfb::StridedIn d = strided;
      d.t0 = r;
      if (p->last_strided == PFB_STRIDED_INPUT_NONE) p->last_strided = PFB_STRIDED_INPUT_STAGED;
      return pfb::launch_strided_rows_copy(d, n, p->N, p->n_pol, dst, dps, s);
    }
    case PACKED: break;
  }
  return copy_pols(dst, dps, base + r * p->N, ps, n * p->N, p->n_pol, copy, s);
}

// Blocks b with a spectral taper (pfb_spectral.hip): Matlab's order — per channel FFT, stitch
// x taper, then the L-point IFFT as row FFTs — in sub-chunks whose scratch stays within 2^26
// values per buffer.  Packed rows only, none of the call's missing from them.
static pfb_status synthesis_spectral(const SynthRows& rows, Blocks b, const SynthOut& out, hipStream_t s) {
  pfb_synthesis_plan* p = rows.plan;
  p->last_stage1 = PFB_STAGE1_STORED;  // (the spectral passes read the channelised rows)
  const int64_t per_block = (int64_t)p->N * std::max(p->Nf, p->W);
  const int64_t sub = std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)1 << 26) / per_block));
  const int64_t nsub = std::min(sub, b.hi - b.lo);
  HIPCHK(p->sbuf0.ensure((size_t)nsub * per_block * sizeof(float2)));
  HIPCHK(p->sbuf1.ensure((size_t)nsub * per_block * sizeof(float2)));
  for (int64_t c0 = b.lo; c0 < b.hi; c0 += nsub) {
    pfb::SpectralArgs a{};
    a.in = rows.base + rows.row0 * p->N;
    a.in_pol_stride = rows.ps;
    a.out = out.out;
    a.out_pol_stride = out.out_ps;
    a.out_limit = out.out_limit;
    a.b0 = c0;
    a.nb = std::min(nsub, b.hi - c0);
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

// Blocks b of a call: channel IFFT of their rows into Z, then the block kernel.
// (`rows` by value: the channel IFFT's arguments point into it, SynthRows::chan_in)
pfb_status pfb::host::synthesis_chunk(SynthRows rows, Blocks b, const SynthOut& out, hipStream_t s) {
  pfb_synthesis_plan* p = rows.plan;
  if (p->has_spectral) {
    if (rows.kind != SynthRows::PACKED) return fail(PFB_ERR_UNSUPPORTED, "rows read in place with a spectral taper");
    // (a positive row0: the blocks start that many rows into the rows — a sample offset)
    if (rows.row0 < 0) return fail(PFB_ERR_UNSUPPORTED, "row shift with a spectral taper");
    return synthesis_spectral(rows, b, out, s);
  }
  const int64_t n = (b.hi - b.lo) * p->keep + 2 * (int64_t)p->Ov;
  zkey_clear(p);
  HIPCHK(p->Z.ensure((size_t)p->n_pol * n * p->N * sizeof(float2)));
  float2* Z = p->Z.as<float2>();
  pfb::ChanIfftArgs c{};
  const pfb_status st = rows.chan_in(rows.row0 + b.lo * p->keep, n, c);
  if (st != PFB_OK) return st;
  c.out = Z;
  c.out_pol_stride = n * p->N;
  c.n_rows = n;
  c.n_pol = p->n_pol;
  c.N = p->N;
  c.perm = p->identity_perm ? nullptr : p->perm.as<int>();
  c.cgain = p->has_cgain ? p->cgain.as<float>() : nullptr;
  c.twN = p->twN.as<float2>();
  // the Nf = 256 shapes: Z in the 2-row run layout the wave kernel reads (256-B runs per
  // load instruction, as the fused round trip's analysis writes it); every other shape
  // [row][t0] for the block kernel
  SynthLaunch l;
  l.Z = Z;
  l.z_ps = n * p->N;
  l.b0 = b.lo;
  l.nb = b.hi - b.lo;
  l.o = out;
  l.zblk = 2;
  if (!pfb::synth_wave_supported(synth_args(p, l))) l.zblk = 0;
  c.zblk = l.zblk ? l.zblk : 1;
  {
    const double in_bytes = rows.kind == SynthRows::DADA ? 2.0 * (rows.dada.nbit / 8) : 8.0;
    ProfScope ps(1, (double)p->n_pol * n * p->N * (in_bytes + 8.0), s);
    HIPCHK(pfb::launch_chan_ifft(c, s));
  }
  return synthesis_blocks(p, l, s);
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

// blocks b in chunks
static pfb_status synthesis_range(const SynthRows& rows, Blocks b, const SynthOut& out, hipStream_t s) {
  if (b.hi <= b.lo) return PFB_OK;
  const int64_t CB = synthesis_chunk_blocks(rows.plan, b.hi - b.lo);
  for (int64_t b0 = b.lo; b0 < b.hi; b0 += CB) {
    const pfb_status st = synthesis_chunk(rows, Blocks{b0, std::min(b0 + CB, b.hi)}, out, s);
    if (st != PFB_OK) return st;
  }
  return PFB_OK;
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
struct SynthHost : SynthShape {
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
    // H0 = freqz(h, 1, n), n = N*W/2; filter_response = 1/|H0(0..W/2)|  (polyphase_synthesis.m:138-150)
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
  static_cast<SynthShape&>(*p) = h;
  p->n_pol = d->n_pol;
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

// The DADA section of a synthesis call (pfb_synthesis_execute_dada,
// pfb_inverse_filterbank_execute_dada: rows x the plan's n_chan x n_pol x ndim values of nbit):
// the channel IFFT can read it in place (pfb_api.h, FUSED)
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

// ---- one call, as its entry point was given it
// The rows: packed cf32 (`in`, pol stride in_ps, in host or device memory), or one of
// sec: a DADA section (device memory; `in` unused);
// sv: `in` read through a strided layout (device memory).
struct SynthIn {
  const pfb_cf32* in = nullptr;
  int64_t in_ps = 0;
  const DadaSection* sec = nullptr;
  const StridedView* sv = nullptr;
  int32_t mem = PFB_MEM_DEVICE;
  const void* base() const { return sec ? sec->base : in; }
  bool packed() const { return !sec && !sv; }
};

// The output: nbit 0, cf32 out[pol][t] (pol stride out_ps; cap in samples per polarisation, in
// the memory the input is in); else a DADA section of that NBIT (cap in bytes), each component
// to_sample(scale * y)
struct SynthDst {
  void* out = nullptr;
  int64_t out_ps = 0, cap = 0;
  int64_t* n_out = nullptr;
  int nbit = 0;
  float scale = 1.f;
};

// n rows; sample_offset: 1-based, the stateless calls only
struct SynthCall {
  SynthIn in;
  int64_t n = 0, sample_offset = 1;
  SynthDst dst;
  void* stream = nullptr;
};

static pfb_status capacity_check(const pfb_synthesis_plan* p, const SynthDst& d, int64_t olen) {
  if (!d.nbit) {
    if (d.cap < olen)
      return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld", (long long)d.cap, (long long)olen);
    return PFB_OK;
  }
  const int64_t need = olen * p->n_pol * 2 * (d.nbit / 8);
  if (d.cap < need)
    return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld bytes", (long long)d.cap, (long long)need);
  return PFB_OK;
}

// the pol strides of buffers in device memory cover the data (a section has none)
static pfb_status stride_check(const pfb_synthesis_plan* p, const SynthCall& c, int64_t olen) {
  if (c.in.mem == PFB_MEM_DEVICE &&
      ((c.in.packed() && c.in.in_ps < c.n * p->N) || (!c.dst.nbit && c.dst.out_ps < olen)))
    return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  return PFB_OK;
}

// The call is under way: its device current, the input reporters start over.  A cf32-output
// call gets here once its input arguments have passed, before its lengths are known; a to-DADA
// call only after every check.
static pfb_status synthesis_begin(pfb_synthesis_plan* p) {
  HIPCHK(hipSetDevice(p->device));
  p->last_dada = PFB_DADA_INPUT_NONE;
  p->last_strided = PFB_STRIDED_INPUT_NONE;
  return PFB_OK;
}

// the input-side checks both call kinds start with; `what`: the row count's name in the call
static pfb_status input_check(pfb_synthesis_plan* p, const SynthCall& c, bool stateless, const char* what) {
  if (!p || (!c.in.base() && c.n > 0)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (stateless && c.sample_offset < 1) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 1-based (>= 1)");
  if (c.n < 0) return fail(PFB_ERR_INVALID_ARG, "negative %s", c.dst.nbit ? "row count" : what);
  if (c.in.sv) {
    const pfb_status st = strided_view_check(p, *c.in.sv, c.n);
    if (st != PFB_OK) return st;
  }
  return c.dst.nbit ? PFB_OK : synthesis_begin(p);
}

// The lengths of a stateless call: the rows from row `off` on, n of them, olen samples out
struct SynthLens {
  int64_t off, n, olen;
};

// The lengths and the argument checks of a stateless call, with its output counted in the
// unit of c.dst.  A call that yields nothing checks no more than its input.
static pfb_status synthesis_check(pfb_synthesis_plan* p, const SynthCall& c, SynthLens& len) {
  pfb_status st = input_check(p, c, true, "n_dat");
  if (st != PFB_OK) return st;
  len.off = std::min<int64_t>(c.sample_offset - 1, c.n);
  len.n = c.n - len.off;  // in = in(:, :, sample_offset:end)  (polyphase_synthesis.m:99)
  len.olen = synth_blocks(p, len.n) * p->Lkeep;
  if (c.dst.n_out) *c.dst.n_out = len.olen;
  if (len.olen == 0) return PFB_OK;
  if (!c.dst.out) return fail(PFB_ERR_INVALID_ARG, "null output");
  st = capacity_check(p, c.dst, len.olen);
  if (st != PFB_OK) return st;
  return stride_check(p, c, len.olen);
}

// What an entry point was given -> the rows the launches read: a section or a layout in place
// where the plan's channel IFFT can (FUSED / IN_PLACE), otherwise unpacked / copied whole into
// the plan's staging buffer, from where the packed path runs (STAGED).  Row 0 is the input's.
static pfb_status synth_rows(pfb_synthesis_plan* p, const SynthCall& c, hipStream_t s, SynthRows& rows) {
  rows = SynthRows::packed(p, (const float2*)c.in.in, c.in.in_ps, c.n);
  if (c.in.packed()) {
    if (c.in.mem == PFB_MEM_HOST) rows.copy = hipMemcpyHostToDevice;
    return PFB_OK;
  }
  if (c.in.sv) {
    const StridedView& v = *c.in.sv;
    rows.kind = SynthRows::STRIDED;
    rows.strided = pfb::StridedIn{(const float2*)c.in.in, v.ps, v.rs, v.cs, c.n, 0};
    if (strided_in_place(p)) return PFB_OK;
    const pfb_status st = strided_stage(p, rows.strided, c.n, s);
    if (st != PFB_OK) return st;
  } else {
    const DadaSection& sec = *c.in.sec;
    rows.kind = SynthRows::DADA;
    rows.dada = pfb::DadaIn{sec.base, sec.nbit, sec.order == PFB_DADA_LOWCBF, c.n, 0};
    if (dada_fusable(p, sec)) return PFB_OK;
    const pfb_status st = dada_stage(p, sec, c.n, s);
    if (st != PFB_OK) return st;
  }
  rows = SynthRows::packed(p, p->stage_in.as<float2>(), c.n * p->N, c.n);
  return PFB_OK;
}

// pfb_synthesis_execute* once synthesis_check has passed
static pfb_status synthesis_go(pfb_synthesis_plan* p, const SynthCall& c, const SynthLens& len, const SynthOut& out) {
  if (len.olen == 0) return PFB_OK;
  hipStream_t s = (hipStream_t)c.stream;
  const Blocks all{0, synth_blocks(p, len.n)};
  SynthRows rows;
  pfb_status st = synth_rows(p, c, s, rows);
  if (st != PFB_OK) return st;
  if (c.in.mem == PFB_MEM_DEVICE) {
    rows.row0 = len.off;  // the blocks start `off` rows into the buffer, the section, the layout
    return synthesis_range(rows, all, out, s);
  }
  HIPCHK(p->stage_in.ensure((size_t)p->n_pol * len.n * p->N * sizeof(float2)));
  HIPCHK(p->stage_out.ensure((size_t)p->n_pol * len.olen * sizeof(float2)));
  HIPCHK(rows.copy_to(len.off, len.n, p->stage_in.as<float2>(), len.n * p->N, s));
  st = synthesis_range(SynthRows::packed(p, p->stage_in.as<float2>(), len.n * p->N, len.n), all,
                       SynthOut{p->stage_out.as<float2>(), len.olen, len.olen, {}}, s);
  if (st != PFB_OK) return st;
  HIPCHK(copy_pols(out.out, out.out_ps, p->stage_out.as<float2>(), len.olen, len.olen, p->n_pol,
                   hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

// the cf32 output of a call that yields olen samples
static SynthOut cf32_out(const SynthDst& d, int64_t olen) {
  return SynthOut{static_cast<float2*>(d.out), d.out_ps, olen, {}};
}

// a cf32-output stateless call
static pfb_status synthesis_exec(pfb_synthesis_plan* p, const SynthCall& c) {
  SynthLens len{};
  const pfb_status st = synthesis_check(p, c, len);
  if (st != PFB_OK) return st;
  return cf32_output(p, synthesis_go(p, c, len, cf32_out(c.dst, len.olen)));
}

pfb_status pfb_synthesis_execute(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                 int64_t n_dat, int64_t sample_offset, pfb_cf32* out,
                                 int64_t out_ps, int64_t cap, int64_t* n_out, int32_t mem,
                                 void* stream) {
  return synthesis_exec(p, SynthCall{{in, in_ps, nullptr, nullptr, mem}, n_dat, sample_offset,
                                     {out, out_ps, cap, n_out}, stream});
}

pfb_status pfb_synthesis_execute_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                      int32_t order, int64_t n_dat, int64_t sample_offset, pfb_cf32* out,
                                      int64_t out_ps, int64_t cap, int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = section_check(p, sec, n_dat);
  if (st != PFB_OK) return st;
  return synthesis_exec(p, SynthCall{{nullptr, 0, &sec}, n_dat, sample_offset, {out, out_ps, cap, n_out}, stream});
}

int32_t pfb_synthesis_last_dada_input(const pfb_synthesis_plan* p) { return p ? p->last_dada : -1; }

pfb_status pfb_synthesis_execute_strided(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                         int64_t in_rs, int64_t in_cs, int64_t in_cap, int64_t n_dat,
                                         int64_t sample_offset, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                         int64_t* n_out, void* stream) {
  const StridedView sv{in_ps, in_rs, in_cs, in_cap};
  return synthesis_exec(p, SynthCall{{in, in_ps, nullptr, &sv}, n_dat, sample_offset, {out, out_ps, cap, n_out},
                                     stream});
}

int32_t pfb_synthesis_last_strided_input(const pfb_synthesis_plan* p) { return p ? p->last_strided : -1; }

pfb_status pfb_inverse_filterbank_set_sample_offset(pfb_synthesis_plan* p, int64_t sample_offset) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (sample_offset < 0) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 0-based (>= 0)");
  p->ifb_offset = sample_offset;
  return PFB_OK;
}

// InverseFilterBank.m:73-135.  Every call runs polyphase_synthesis on the concatenated
// rows (carry + input) from row `so` = sample_offset on (InverseFilterBank.m:92-96, `sample_offset+1`), and the
// carry starts at input_idat = (output length) nu / (n_chan de) = B keep of the
// concatenation — not offset by `so`: the next call skips `so` rows of it again, so
// consecutive calls see the blocks of one continuous run.
// (The new rows as a DADA section or behind a strided layout, in device memory.  Read in
// place (synth_rows): the blocks of new rows read the section or the layout themselves, and
// whatever the packed call copies out of `in` — the stitched head, the carry — is unpacked
// from the section's rows, or copied out of the layout by the strided-rows copy kernel,
// instead (SynthRows::copy_to).  Otherwise the rows are staged whole once every check has
// passed, and the packed path runs.)
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

// The lengths and the argument checks of a stream call, with its output counted in the unit
// of c.dst (the order differs from synthesis_check's on purpose: it is each call's own)
static pfb_status ifb_check(pfb_synthesis_plan* p, const SynthCall& c, IfbLens& len) {
  pfb_status st = input_check(p, c, false, "n_in");
  if (st != PFB_OK) return st;
  len = ifb_lens(p, c.n);
  if (len.input_idat < 0)
    // no complete block and a carry rounded up past the data: InverseFilterBank.m:104-122
    // would index input(:, :, input_idat + 1 : end) before the first sample (its rounding
    // loop never settles); the call is rejected and the object state is left unchanged
    return fail(PFB_ERR_INVALID_ARG,
                "InverseFilterBank: %lld buffered + %lld new rows hold no complete block and "
                "round the carry past the data (InverseFilterBank.m:104-122); pass more rows",
                (long long)p->buffered, (long long)c.n);
  if (c.dst.n_out) *c.dst.n_out = len.olen;
  st = capacity_check(p, c.dst, len.olen);
  if (st != PFB_OK) return st;
  st = stride_check(p, c, len.olen);
  if (st != PFB_OK) return st;
  if (len.olen > 0 && !c.dst.out) return fail(PFB_ERR_INVALID_ARG, "null output");
  return PFB_OK;
}

// The next call's carry: rows [r, r + n) of `rows` into the plan's carry buffer, n <= 0 none
// (twin of the analysis' fb_carry)
static pfb_status ifb_store_carry(const SynthRows& rows, int64_t r, int64_t n, hipStream_t s) {
  pfb_synthesis_plan* p = rows.plan;
  if (n > 0) {
    HIPCHK(p->carry.ensure((size_t)p->n_pol * n * p->N * sizeof(float2)));
    HIPCHK(rows.copy_to(r, n, p->carry.as<float2>(), n * p->N, s));
  }
  p->buffered = std::max<int64_t>(n, 0);
  return PFB_OK;
}

// pfb_inverse_filterbank_execute* once ifb_check has passed
static pfb_status ifb_go(pfb_synthesis_plan* p, const SynthCall& c, const IfbLens& len, const SynthOut& out) {
  hipStream_t s = (hipStream_t)c.stream;
  const int N = p->N;
  const bool device = c.in.mem == PFB_MEM_DEVICE, to_host = c.in.mem == PFB_MEM_HOST;
  const int64_t Bc = p->buffered;
  SynthRows rows;  // the new rows
  pfb_status st = synth_rows(p, c, s, rows);
  if (st != PFB_OK) return st;
  // Carry without the concatenation copy: blocks whose rows start at or after the carried
  // Bc rows read the new rows in place (call row 0 is their row so - Bc), the first ones a
  // small stitched buffer; same blocks, same kernels as the concatenated run.
  static const bool no_split = pfb::knob("PFB_FB_NO_SPLIT") != nullptr;  // A/B
  if (!no_split && device && Bc > 0 && !p->has_spectral && len.input_idat >= Bc) {
    if (len.olen > 0) {
      // first block starting at or after row Bc of the concatenation: so + b keep >= Bc
      const int64_t b_s = std::min(len.B, std::max<int64_t>(0, (Bc - len.so + p->keep - 1) / p->keep));
      if (b_s > 0) {
        const int64_t L = std::min(len.total, len.so + (b_s - 1) * p->keep + p->Nf);
        HIPCHK(p->work.ensure((size_t)p->n_pol * L * N * sizeof(float2)));
        float2* wk = p->work.as<float2>();
        HIPCHK(copy_pols(wk, L * N, p->carry.as<float2>(), Bc * N, std::min(Bc, L) * N, p->n_pol,
                         hipMemcpyDeviceToDevice, s));
        if (L > Bc) HIPCHK(rows.copy_to(0, L - Bc, wk + Bc * N, L * N, s));
        SynthRows head = SynthRows::packed(p, wk, L * N, L);
        head.row0 = len.so;
        st = synthesis_range(head, Blocks{0, b_s}, out, s);
        if (st != PFB_OK) return st;
      }
      rows.row0 = len.so - Bc;
      st = synthesis_range(rows, Blocks{b_s, len.B}, out, s);
      if (st != PFB_OK) return st;
    }
    return ifb_store_carry(rows, len.input_idat - Bc, len.buffered, s);
  }
  // input = cat(3, input_buffer, input); the new rows themselves when nothing is buffered
  // (every block reads them where they lie, the carry is their copied or unpacked tail)
  SynthRows cat = rows;
  if (Bc != 0 || !device) {
    HIPCHK(p->work.ensure((size_t)p->n_pol * std::max<int64_t>(len.total, 1) * N * sizeof(float2)));
    float2* wk = p->work.as<float2>();
    HIPCHK(copy_pols(wk, len.total * N, p->carry.as<float2>(), Bc * N, Bc * N, p->n_pol, hipMemcpyDeviceToDevice, s));
    HIPCHK(rows.copy_to(0, c.n, wk + Bc * N, len.total * N, s));
    cat = SynthRows::packed(p, wk, len.total * N, len.total);
  }
  cat.row0 = len.so;
  if (len.olen > 0) {
    if (to_host) {
      HIPCHK(p->stage_out.ensure((size_t)p->n_pol * len.olen * sizeof(float2)));
      st = synthesis_range(cat, Blocks{0, len.B}, SynthOut{p->stage_out.as<float2>(), len.olen, len.olen, {}}, s);
      if (st != PFB_OK) return st;
      HIPCHK(copy_pols(out.out, out.out_ps, p->stage_out.as<float2>(), len.olen, len.olen, p->n_pol,
                       hipMemcpyDeviceToHost, s));
    } else {
      st = synthesis_range(cat, Blocks{0, len.B}, out, s);
      if (st != PFB_OK) return st;
    }
  }
  st = ifb_store_carry(cat, len.input_idat, len.buffered, s);
  if (st != PFB_OK) return st;
  if (to_host) HIPCHK(hipStreamSynchronize(s));
  return PFB_OK;
}

// a cf32-output stream call
static pfb_status ifb_exec(pfb_synthesis_plan* p, const SynthCall& c) {
  IfbLens len{};
  const pfb_status st = ifb_check(p, c, len);
  if (st != PFB_OK) return st;
  return cf32_output(p, ifb_go(p, c, len, cf32_out(c.dst, len.olen)));
}

pfb_status pfb_inverse_filterbank_execute(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                          int64_t n_in, pfb_cf32* out, int64_t out_ps, int64_t cap,
                                          int64_t* n_out, int32_t mem, void* stream) {
  return ifb_exec(p, SynthCall{{in, in_ps, nullptr, nullptr, mem}, n_in, 1, {out, out_ps, cap, n_out}, stream});
}

pfb_status pfb_inverse_filterbank_execute_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit,
                                               int32_t ndim, int32_t order, int64_t n_in, pfb_cf32* out,
                                               int64_t out_ps, int64_t cap, int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  const pfb_status st = section_check(p, sec, n_in);
  if (st != PFB_OK) return st;
  return ifb_exec(p, SynthCall{{nullptr, 0, &sec}, n_in, 1, {out, out_ps, cap, n_out}, stream});
}

pfb_status pfb_inverse_filterbank_execute_strided(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                  int64_t in_rs, int64_t in_cs, int64_t in_cap, int64_t n_in,
                                                  pfb_cf32* out, int64_t out_ps, int64_t cap, int64_t* n_out,
                                                  void* stream) {
  const StridedView sv{in_ps, in_rs, in_cs, in_cap};
  return ifb_exec(p, SynthCall{{in, in_ps, nullptr, &sv}, n_in, 1, {out, out_ps, cap, n_out}, stream});
}

}  // extern "C"

// the wave kernel stores such a section itself (pfb_api.h, FUSED).  Every (polarisations, NBIT)
// cell stays FUSED: on the C2 synthesis unit each takes 0.49-0.73 of the time of the pair
// (execute, scale, pfb_dada_pack), the gap 0.085-0.177 ms against a run-to-run spread of the
// pair of at most 0.006 ms — cf32 rows into NBIT 8 / 16 / 32: one polarisation 0.115 / 0.119 /
// 0.129 against 0.211 / 0.220 / 0.227 ms, two 0.229 / 0.253 / 0.320 against 0.406 / 0.420 /
// 0.436 ms (the narrowest cell, 0.73); from an NBIT 16 section 0.099 / 0.099 / 0.100 against
// 0.198 / 0.184 / 0.205 and 0.202 / 0.220 / 0.284 against 0.378 / 0.391 / 0.409 ms
// (profiles/dada_synthesis_output_ab.jsonl)
bool pfb::host::synthesis_dada_out_fusable(const pfb_synthesis_plan* p, const void* out, int nbit) {
  if (nbit != 8 && nbit != 16 && nbit != 32) return false;
  if (p->has_spectral || reinterpret_cast<uintptr_t>(out) % (size_t)(nbit / 4) != 0) return false;
  // (the stage-1 row layout synthesis_chunk picks for the wave kernel: 2-row runs)
  SynthLaunch l;
  l.nb = 1;
  l.zblk = 2;
  return pfb::synth_wave_dadaout_supported(synth_args(p, l), nbit);
}

extern "C" {

// The to-DADA calls (pfb_api.h): every check — the section's own, then the corresponding
// cf32-output call's in its order (synthesis_check / ifb_check, the capacity in bytes) — before
// anything is launched or the stream state changes; then FUSED — the call's block launches
// store the section (SynthOut::dada) — or STAGED — the cf32 path into the plan's buffer and the
// scaled pack launch.
static pfb_status synthesis_to_dada(pfb_synthesis_plan* p, const SynthCall& c, bool stream_call) {
  const SynthDst& d = c.dst;
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (d.nbit != 8 && d.nbit != 16 && d.nbit != 32 && d.nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "output NBIT must be 8, 16, 32 or 64");
  if (!std::isfinite(d.scale)) return fail(PFB_ERR_INVALID_ARG, "output scale is not finite");
  if (reinterpret_cast<uintptr_t>(d.out) % (size_t)(d.nbit / 8) != 0)
    return fail(PFB_ERR_INVALID_ARG, "output section not aligned to its NBIT");
  if (c.in.sec) {
    const pfb_status st = section_check(p, *c.in.sec, c.n);
    if (st != PFB_OK) return st;
  }
  SynthLens len{};
  IfbLens ilen{};
  pfb_status st = stream_call ? ifb_check(p, c, ilen) : synthesis_check(p, c, len);
  if (st != PFB_OK) return st;
  const int64_t olen = stream_call ? ilen.olen : len.olen;
  st = synthesis_begin(p);
  if (st != PFB_OK) return st;
  const bool fused = synthesis_dada_out_fusable(p, d.out, d.nbit);
  SynthOut o{nullptr, olen, olen, SynthDada{d.out, d.nbit, d.scale}};
  if (!fused) {
    HIPCHK(p->stage_out.ensure((size_t)p->n_pol * std::max<int64_t>(olen, 1) * sizeof(float2)));
    o = SynthOut{p->stage_out.as<float2>(), olen, olen, {}};
  }
  st = stream_call ? ifb_go(p, c, ilen, o) : synthesis_go(p, c, len, o);
  if (st != PFB_OK) return st;
  if (!fused && olen > 0)
    HIPCHK(pfb::launch_dada_pack_scaled(p->stage_out.as<float2>(), olen, olen, 1, p->n_pol, d.out, d.nbit, d.scale,
                                        (hipStream_t)c.stream));
  p->last_dada_out = fused ? PFB_DADA_OUTPUT_FUSED : PFB_DADA_OUTPUT_STAGED;
  return PFB_OK;
}

pfb_status pfb_synthesis_execute_to_dada(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps, int64_t n_dat,
                                         int64_t sample_offset, void* out, int32_t out_nbit, float out_scale,
                                         int64_t cap_bytes, int64_t* n_out, void* stream) {
  return synthesis_to_dada(
      p, SynthCall{{in, in_ps}, n_dat, sample_offset, {out, 0, cap_bytes, n_out, out_nbit, out_scale}, stream}, false);
}

pfb_status pfb_inverse_filterbank_execute_to_dada(pfb_synthesis_plan* p, const pfb_cf32* in, int64_t in_ps,
                                                  int64_t n_in, void* out, int32_t out_nbit, float out_scale,
                                                  int64_t cap_bytes, int64_t* n_out, void* stream) {
  return synthesis_to_dada(
      p, SynthCall{{in, in_ps}, n_in, 1, {out, 0, cap_bytes, n_out, out_nbit, out_scale}, stream}, true);
}

pfb_status pfb_synthesis_execute_dada_to_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit, int32_t ndim,
                                              int32_t order, int64_t n_dat, int64_t sample_offset, void* out,
                                              int32_t out_nbit, float out_scale, int64_t cap_bytes, int64_t* n_out,
                                              void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return synthesis_to_dada(
      p, SynthCall{{nullptr, 0, &sec}, n_dat, sample_offset, {out, 0, cap_bytes, n_out, out_nbit, out_scale}, stream},
      false);
}

pfb_status pfb_inverse_filterbank_execute_dada_to_dada(pfb_synthesis_plan* p, const void* in, int32_t nbit,
                                                       int32_t ndim, int32_t order, int64_t n_in, void* out,
                                                       int32_t out_nbit, float out_scale, int64_t cap_bytes,
                                                       int64_t* n_out, void* stream) {
  const DadaSection sec{in, nbit, ndim, order};
  return synthesis_to_dada(
      p, SynthCall{{nullptr, 0, &sec}, n_in, 1, {out, 0, cap_bytes, n_out, out_nbit, out_scale}, stream}, true);
}

int32_t pfb_synthesis_last_dada_output(const pfb_synthesis_plan* p) { return p ? p->last_dada_out : -1; }

int64_t pfb_inverse_filterbank_buffered(const pfb_synthesis_plan* p) { return p ? p->buffered : -1; }

pfb_status pfb_inverse_filterbank_reset(pfb_synthesis_plan* p) {
  if (!p) return fail(PFB_ERR_INVALID_ARG, "null plan");
  p->buffered = 0;
  return PFB_OK;
}

}  // extern "C"
