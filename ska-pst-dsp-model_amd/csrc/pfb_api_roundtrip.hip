// pfb_api_roundtrip.hip — the round trips of the C ABI (include/pfb_api.h): analysis ->
// synthesis of one call (pfb_roundtrip_*), cf32 or from a DADA section into DADA sections.
#include <cmath>
#include <cstdlib>

#include "pfb_host.hpp"

using namespace pfb::host;

extern "C" {

// ====================================================================== round trip
// Analysis -> synthesis of one call, pipelined in chunks of synthesis blocks (the
// reference's test_data_pipeline.m:114,132 runs the two back to back).  Chunk c's
// analysis rows run on the analysis plan's own stream while chunk c-1 is synthesised
// on the caller's stream, so the two kernels share the chip (each alone leaves HBM and
// VALU partly idle), and the synthesis reads each channelised row shortly after it was
// written (Infinity-Cache resident).  The full channelised product is still written to
// `chan`.  On this chunked path every row and block is computed by the same kernels with
// the same inputs as pfb_analysis_execute + pfb_synthesis_execute, so both results are
// bit-identical to the separate calls (the fused path below: see its comment).

// One round-trip call.  phase 0: the whole round trip; 1 / 2: only the analysis / only the
// synthesis half of the fused path (pfb_roundtrip_analysis_execute /
// pfb_roundtrip_synthesis_execute), which hand the stage-1 rows over in the synthesis plan's
// scratch.  A half sets the members of its side only.
struct RtBuf {
  void* p = nullptr;
  int64_t ps = 0, cap = 0;  // pol stride; capacity per polarisation
};
struct RtCall {
  int phase = 0;
  int64_t n_dat = 0, sample_offset = 1;
  // input and channelised product (phase != 2): cf32 [pol][t] and [pol][row][chan], capacity in
  // rows — or, with RtOpt::dd / od, the sections themselves
  const void* in = nullptr;
  int64_t in_ps = 0;
  RtBuf chan;
  // output (phase != 1): cf32 [pol][t], capacity in samples — or, with RtOpt::sd, the section
  RtBuf out;
  int64_t* n_chan_rows = nullptr;
  int64_t* n_out = nullptr;
  void* stream = nullptr;
};

// What the file-to-file calls (roundtrip_dada, below) ask of roundtrip_run; the cf32 calls pass
// none of it.
struct RtOpt {
  // FUSED: the analysis launch reads the section dd in place and stores the product as the
  // float section od, and the block launch stores the section sd.  Only for a call that
  // `wave2` named.
  const AnaDada* dd = nullptr;
  const AnaOut* od = nullptr;
  SynthDada sd;
  // the stage-1 rows are stored whatever pfb_synthesis_set_stage1_rows says (no recomputing
  // kernel reads a section, and a plan-owned staging buffer is no input to come back to)
  bool stored = false;
  // every check of the call but those of the pol strides (sections have none), and the
  // allocation of the rows, then return: no launch, no change of the split round trip's key
  bool dry = false;
  // (dry) set when the call takes the fused path through the streaming analysis and the
  // Nf = 256 wave kernel on stored 2-row runs
  bool* wave2 = nullptr;
};

static pfb_status roundtrip_run(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const RtCall& c, const RtOpt& opt) {
  const int phase = c.phase;
  const int64_t n_dat = c.n_dat, sample_offset = c.sample_offset, in_ps = c.in_ps, chan_ps = c.chan.ps;
  const float2* x = static_cast<const float2*>(c.in);
  float2* y = static_cast<float2*>(c.chan.p);
  if (opt.wave2) *opt.wave2 = false;
  if (!pa || !ps || (!x && n_dat > 0 && phase != 2)) return fail(PFB_ERR_INVALID_ARG, "null argument");
  if (pa->device != ps->device) return fail(PFB_ERR_INVALID_ARG, "plans on different devices");
  if (pa->qin_on)
    return fail(PFB_ERR_UNSUPPORTED, "round trip with the input quantiser on: use the separate calls");
  if (pa->variant == pfb::kLowCbf)
    return fail(PFB_ERR_UNSUPPORTED, "round trip of the LowCBF filterbank: use the separate calls");
  if (pa->N != ps->N || pa->n_pol != ps->n_pol)
    return fail(PFB_ERR_INVALID_ARG, "analysis (%d ch, %d pol) and synthesis (%d ch, %d pol) differ",
                pa->N, pa->n_pol, ps->N, ps->n_pol);
  if (sample_offset < 1) return fail(PFB_ERR_INVALID_ARG, "sample_offset is 1-based (>= 1)");
  if (n_dat < 0) return fail(PFB_ERR_INVALID_ARG, "negative n_dat");
  HIPCHK(hipSetDevice(pa->device));
  hipStream_t s = (hipStream_t)c.stream;
  const int64_t K = analysis_K(pa, n_dat);
  const int64_t off = std::min<int64_t>(sample_offset - 1, K);
  const int64_t B = synth_blocks(ps, K - off);
  const int64_t olen = B * ps->Lkeep;
  if (c.n_chan_rows) *c.n_chan_rows = K;
  if (c.n_out) *c.n_out = olen;
  if (K == 0) return PFB_OK;
  if (phase != 2) {
    if (!y) return fail(PFB_ERR_INVALID_ARG, "null output");
    if (c.chan.cap < K) return fail(PFB_ERR_BUFFER_TOO_SMALL, "channelised capacity %lld < %lld rows",
                                    (long long)c.chan.cap, (long long)K);
    if (!opt.dry && (in_ps < n_dat || chan_ps < K * pa->N))
      return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  if (phase != 1) {
    if (olen > 0 && !c.out.p) return fail(PFB_ERR_INVALID_ARG, "null output");
    if (c.out.cap < olen) return fail(PFB_ERR_BUFFER_TOO_SMALL, "output capacity %lld < %lld",
                                      (long long)c.out.cap, (long long)olen);
    if (!opt.dry && olen > 0 && c.out.ps < olen)
      return fail(PFB_ERR_INVALID_ARG, "polarisation stride smaller than the data");
  }
  // the analysis of the whole call: all K rows into `chan` (the launches below add to it)
  AnaLaunch whole;
  whole.in = x;
  whole.in_ps = in_ps;
  whole.n_dat = n_dat;
  whole.out = y;
  whole.out_ps = chan_ps;
  whole.K_end = whole.K_total = K;
  if (B == 0) return (phase == 2 || opt.dry) ? PFB_OK : analysis_run(pa, whole, s);
  // the block-kernel arguments of all B blocks, no buffers set: what the shape predicates read
  auto blocks_probe = [&](int zb, const FirSrc* f) {
    SynthLaunch l;
    l.nb = B;
    l.zblk = zb;
    l.fir = f;
    return synth_args(ps, l);
  };

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
  if (zblk && !pfb::synth_wave_supported(blocks_probe(zblk, nullptr))) zblk = 0;
  // generic path (N > 256, the SKA-Mid round trip): the FIR writes the rows in 2-row runs
  // per column, so the Nf = 512 wave synthesis loads whole 128-B lines (2 rows x 8 phases)
  // — bit-identical; measured (profiles/r05_v17_c3_zrun_kernel_ab/) synthesis -17 us, FIR
  // +8 us, row FFT +4 us (it reads each row's pair partner from the lines fetched one row
  // earlier): net -5 us per unit (PFB_C3_ZRUN=0: rows, experiments build)
  static const bool zrun_on = !(pfb::knob("PFB_C3_ZRUN") && std::atoi(pfb::knob("PFB_C3_ZRUN")) == 0);
  const bool zrun = zrun_on && !zblk && !pa->fused && analysis_emits_z(pa) && off % 2 == 0 &&
                    pfb::synth_wave512_supported(blocks_probe(2, nullptr));
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
  FirSrc fsrc{x, in_ps, n_dat, off / std::max(pa->nu, 1), pa->gtab.as<float>(), pa->nu, pa->de,
              pa->P + 1};
  bool fir = false;
  if (synth_fir_on && zblk && pa->gtab.p && off % pa->nu == 0 && phase != 2) {
    fir = pfb::synth_wave_fir_supported(blocks_probe(0, &fsrc));
  }
  if (phase == 2 && ps->zkey_x != nullptr) {
    // the analysis half chose recomputed rows: the synthesis reads the input it recorded
    fir = true;
    fsrc.x = (const float2*)ps->zkey_x;
    fsrc.x_ps = ps->zkey_xps;
  }
  const int64_t zkey[5] = {n_dat, off, fir ? -1 : zblk, K, zrows};
  // the synthesis of the whole call: all B blocks into `out`, from recomputed rows (fir) or
  // from the rows in Z (set below, with the analysis launch that writes them)
  SynthLaunch blocks;
  blocks.nb = B;
  blocks.o = opt.sd.base ? SynthOut{nullptr, c.out.ps, olen, opt.sd}
                         : SynthOut{static_cast<float2*>(c.out.p), c.out.ps, olen, {}};
  if (fir && fuse) {
    blocks.fir = &fsrc;
    if (phase == 2) {
      if (ps->zkey_plan != pa->serial || !std::equal(zkey, zkey + 5, ps->zkey))
        return fail(PFB_ERR_INVALID_ARG,
                    "split round trip: the synthesis plan holds no analysis half of this analysis plan, "
                    "n_dat %lld and sample_offset %lld (run pfb_roundtrip_analysis_execute with the same "
                    "arguments first)",
                    (long long)n_dat, (long long)sample_offset);
      if (opt.dry) return PFB_OK;
      return synthesis_blocks(ps, blocks, s);
    }
    if (opt.dry) return PFB_OK;
    zkey_clear(ps);
    pfb_status st = analysis_run(pa, whole, s);
    if (st != PFB_OK) return st;
    if (phase == 1) {
      // the synthesis half re-reads this input: the caller keeps it unchanged until then
      ps->zkey_plan = pa->serial;
      std::copy(zkey, zkey + 5, ps->zkey);
      ps->zkey_x = x;
      ps->zkey_xps = in_ps;
      return PFB_OK;
    }
    return synthesis_blocks(ps, blocks, s);
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
  // the fused path: the analysis also writes the stage-1 rows of rows >= z0 into Z, which the
  // blocks read from row `off` on
  AnaLaunch emit = whole;
  if (fuse) {
    emit.z = ps->Z.as<float2>();
    emit.z_ps = zrows * pa->N;
    emit.z_row0 = z0;
    emit.zblk = zblk;
    blocks.Z = emit.z + (off - z0) * pa->N;
    blocks.z_ps = emit.z_ps;
    blocks.zblk = zblk;
  }
  if (phase != 0) {
    // the split round trip exists for the fused path only (one scratch of rows handed over)
    if (!fuse) return fail(PFB_ERR_UNSUPPORTED, "split round trip: these plans take the chunked pipeline "
                                                "(use pfb_roundtrip_execute)");
    if (opt.wave2) *opt.wave2 = wave2;
    if (opt.dry) return PFB_OK;
    if (phase == 1) {
      zkey_clear(ps);
      emit.dada_in = opt.dd;
      emit.dada_out = opt.od;
      pfb_status st = analysis_run(pa, emit, s);
      if (st != PFB_OK) return st;
      ps->zkey_plan = pa->serial;
      std::copy(zkey, zkey + 5, ps->zkey);
      return PFB_OK;
    }
    return synthesis_blocks(ps, blocks, s);
  }
  if (opt.wave2) *opt.wave2 = wave2;
  if (opt.dry) return PFB_OK;
  zkey_clear(ps);  // phase 0 reuses Z
  if (fuse) {
    // (retired round 5, measured slower twice: the row FFT on a second stream beside the
    // synthesis, Infinity-Cache chunking of the generic path and chunked analysis/synthesis
    // concurrency — profiles/HISTORY.md)
    // (generic N > 256 path: the FIR and the row FFT as two calls on the stream — the same
    // two launches as one call, each then timed alone by the profiler)
    pfb_status st = PFB_OK;
    if (!pa->fused) {
      emit.z_stage = 1;
      st = analysis_run(pa, emit, s);
      emit.z_stage = 2;
      if (st == PFB_OK) st = analysis_run(pa, emit, s);
    } else {
      emit.dada_in = opt.dd;
      emit.dada_out = opt.od;
      st = analysis_run(pa, emit, s);
    }
    if (st != PFB_OK) return st;
    return synthesis_blocks(ps, blocks, s);
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
    AnaLaunch part = whole;
    part.row0 = ra;
    part.K_end = rb;
    pfb_status st = analysis_run(pa, part, pa->aux);
    if (st != PFB_OK) return st;
    ra = rb;
    HIPCHK(hipEventRecord(pa->events[1 + c], pa->aux));
    HIPCHK(hipStreamWaitEvent(s, pa->events[1 + c], 0));
    st = synthesis_chunk(SynthRows::packed(ps, sin_, chan_ps, K - off), Blocks{b0, b0 + nb}, blocks.o, s);
    if (st != PFB_OK) return st;
  }
  // join (the last chunk already ran the analysis to K)
  HIPCHK(hipEventRecord(pa->events[1 + n_chunks], pa->aux));
  HIPCHK(hipStreamWaitEvent(s, pa->events[1 + n_chunks], 0));
  return PFB_OK;
}

// the request of an entry point, without its buffers
static RtCall rt_call(int phase, int64_t n_dat, int64_t sample_offset, void* stream) {
  RtCall c;
  c.phase = phase;
  c.n_dat = n_dat;
  c.sample_offset = sample_offset;
  c.stream = stream;
  return c;
}

pfb_status pfb_roundtrip_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const pfb_cf32* in,
                                 int64_t in_ps, int64_t n_dat, pfb_cf32* chan, int64_t chan_ps,
                                 int64_t chan_cap, int64_t* n_chan_rows, int64_t sample_offset,
                                 pfb_cf32* out, int64_t out_ps, int64_t out_cap, int64_t* n_out,
                                 void* stream) {
  RtCall c = rt_call(0, n_dat, sample_offset, stream);
  c.in = in;
  c.in_ps = in_ps;
  c.chan = RtBuf{chan, chan_ps, chan_cap};
  c.n_chan_rows = n_chan_rows;
  c.out = RtBuf{out, out_ps, out_cap};
  c.n_out = n_out;
  return roundtrip_run(pa, ps, c, RtOpt{});
}

pfb_status pfb_roundtrip_analysis_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const pfb_cf32* in,
                                          int64_t in_ps, int64_t n_dat, pfb_cf32* chan, int64_t chan_ps,
                                          int64_t chan_cap, int64_t* n_chan_rows, int64_t sample_offset,
                                          void* stream) {
  RtCall c = rt_call(1, n_dat, sample_offset, stream);
  c.in = in;
  c.in_ps = in_ps;
  c.chan = RtBuf{chan, chan_ps, chan_cap};
  c.n_chan_rows = n_chan_rows;
  return roundtrip_run(pa, ps, c, RtOpt{});
}

pfb_status pfb_roundtrip_synthesis_execute(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, int64_t n_dat,
                                           int64_t sample_offset, pfb_cf32* out, int64_t out_ps,
                                           int64_t out_cap, int64_t* n_out, void* stream) {
  RtCall c = rt_call(2, n_dat, sample_offset, stream);
  c.out = RtBuf{out, out_ps, out_cap};
  c.n_out = n_out;
  return roundtrip_run(pa, ps, c, RtOpt{});
}

// ---- the round trip from a DADA section into DADA sections (pfb_api.h)
// The sections of a file-to-file call.  Each cell of the A/B (DESIGN.md §4.9,
// profiles/dada_roundtrip_ab.jsonl) that met the decision rule stays FUSED; one that did not
// is listed in rt_dada_cell_staged and takes the STAGED sequence.
struct RtSections {
  DadaSection in;            // phase != 2
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
static bool roundtrip_dada_in_fusable(const pfb_analysis_plan* p, const DadaSection& sec, const void* chan) {
  if (sec.ndim != 2 || sec.order != PFB_DADA_TFP || (sec.nbit != 8 && sec.nbit != 16 && sec.nbit != 32)) return false;
  if (reinterpret_cast<uintptr_t>(sec.base) % (size_t)(sec.nbit / 4) != 0) return false;
  if (reinterpret_cast<uintptr_t>(chan) % 8 != 0) return false;
  return pfb::stream_rt_dada_supported(analysis_shape(p), sec.nbit);
}

// `call`: the request without its buffers (phase, n_dat, sample_offset, the two out-lengths,
// the stream).  Every check — roundtrip_run's own among them, through its dry run — comes
// before the first launch and before the split round trip's key changes; then FUSED (the
// analysis launch reads and stores the sections, the wave synthesis stores the output section)
// or STAGED (unpack, the cf32 round trip on plan-owned buffers, the packs).
static pfb_status roundtrip_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const RtSections& sec,
                                 const RtCall& call) {
  const int phase = call.phase;
  const int64_t n_dat = call.n_dat;
  if (!pa || !ps) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (pa->qin_on)
    return fail(PFB_ERR_UNSUPPORTED, "round trip with the input quantiser on: use the separate calls");
  if (phase != 2) {
    const pfb_status st = section_check(pa, sec.in, n_dat);
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
  // the cf32 call's checks, in its order, on the sections themselves, with the capacities in
  // its units: whole rows of the product section, whole samples (all polarisations) of the
  // output section
  int64_t K = 0, olen = 0;
  bool wave2 = false;
  RtCall c = call;
  c.n_chan_rows = &K;
  c.n_out = &olen;
  if (phase != 2) {
    c.in = sec.in.base;
    c.chan = RtBuf{sec.chan, 0, std::max<int64_t>(sec.chan_cap_bytes, 0) / ((int64_t)pa->N * pa->n_pol * 8)};
  }
  if (phase != 1)
    c.out = RtBuf{sec.out, 0, std::max<int64_t>(sec.out_cap_bytes, 0) / ((int64_t)ps->n_pol * 2 * (sec.out_nbit / 8))};
  RtOpt opt;
  opt.stored = true;
  opt.dry = true;
  opt.wave2 = &wave2;
  pfb_status st = roundtrip_run(pa, ps, c, opt);
  if (call.n_chan_rows && phase != 2) *call.n_chan_rows = K;
  if (call.n_out && phase != 1) *call.n_out = olen;
  if (st != PFB_OK || K == 0) return st;
  if (phase == 2 && olen == 0) return PFB_OK;

  // the call itself: packed strides and exact capacities, nothing left to report
  hipStream_t s = (hipStream_t)call.stream;
  const int P = pa->n_pol;
  opt.dry = false;
  opt.wave2 = nullptr;
  c.n_chan_rows = c.n_out = nullptr;
  c.in_ps = n_dat;
  c.chan = RtBuf{c.chan.p, K * pa->N, K};
  c.out = RtBuf{c.out.p, olen, olen};
  const bool in_fused = phase != 2 && roundtrip_dada_in_fusable(pa, sec.in, sec.chan);
  const bool out_fused = phase != 1 && synthesis_dada_out_fusable(ps, sec.out, sec.out_nbit);
  const bool cell = phase == 0 && rt_dada_cell_staged(P, sec.in.nbit, sec.out_nbit);
  if (wave2 && !cell && (phase == 2 || in_fused) && (phase == 1 || out_fused)) {
    // FUSED: the launches go through dd / od / sd (c.in, c.chan.p and c.out.p stay the sections)
    const AnaDada dd{sec.in.base, sec.in.nbit};
    const AnaOut od{sec.chan, 32, 1.0f};
    if (phase != 2) {
      opt.dd = &dd;
      opt.od = &od;
    }
    if (phase != 1) opt.sd = SynthDada{sec.out, sec.out_nbit, sec.out_scale};
    st = roundtrip_run(pa, ps, c, opt);
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
    st = section_unpack(pa, sec.in, 0, n_dat, x, n_dat, s);
    if (st != PFB_OK) return st;
  }
  c.in = x;
  c.chan.p = y;
  c.out.p = o;
  st = roundtrip_run(pa, ps, c, opt);
  if (st != PFB_OK) return st;
  if (phase != 2) {
    if (!chan_direct) {
      st = pfb_dada_pack(reinterpret_cast<const pfb_cf32*>(y), K * pa->N, K, pa->N, P, sec.chan, 32, call.stream);
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
  const RtSections sec{DadaSection{in, nbit, ndim, order}, chan, chan_cap_bytes, out, out_nbit, out_scale, out_cap_bytes};
  RtCall c = rt_call(0, n_dat, sample_offset, stream);
  c.n_chan_rows = n_chan_rows;
  c.n_out = n_out;
  return roundtrip_dada(pa, ps, sec, c);
}

pfb_status pfb_roundtrip_analysis_execute_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, const void* in,
                                               int32_t nbit, int32_t ndim, int32_t order, int64_t n_dat, void* chan,
                                               int64_t chan_cap_bytes, int64_t* n_chan_rows, int64_t sample_offset,
                                               void* stream) {
  const RtSections sec{DadaSection{in, nbit, ndim, order}, chan, chan_cap_bytes, nullptr, 0, 1.f, 0};
  RtCall c = rt_call(1, n_dat, sample_offset, stream);
  c.n_chan_rows = n_chan_rows;
  return roundtrip_dada(pa, ps, sec, c);
}

pfb_status pfb_roundtrip_synthesis_execute_to_dada(pfb_analysis_plan* pa, pfb_synthesis_plan* ps, int64_t n_dat,
                                                   int64_t sample_offset, void* out, int32_t out_nbit,
                                                   float out_scale, int64_t out_cap_bytes, int64_t* n_out,
                                                   void* stream) {
  const RtSections sec{DadaSection{nullptr, 0, 0, 0}, nullptr, 0, out, out_nbit, out_scale, out_cap_bytes};
  RtCall c = rt_call(2, n_dat, sample_offset, stream);
  c.n_out = n_out;
  return roundtrip_dada(pa, ps, sec, c);
}

}  // extern "C"
