/*
 * pfb_api.h — C ABI of the MI355X-native oversampled polyphase filter bank (PFB).
 *
 * Drop-in boundary for the hot path of ska-telescope/ska-pst-dsp-model:
 *   polyphase_analysis        (matlab/polyphase_analysis.m:1-129, Bunton PFB)
 *   polyphase_analysis_padded (matlab/polyphase_analysis_padded.m:1-161, commutator PFB)
 *   polyphase_synthesis       (matlab/polyphase_synthesis.m:1-325, golden inversion)
 * and the stateful stream objects that call them
 *   FilterBank.execute        (matlab/FilterBank.m:65-128)
 *   InverseFilterBank.execute (matlab/InverseFilterBank.m:63-137)
 * which the reference selects by name (FilterBank.m:36 str2func(analysis_function))
 * or through the Python backend switch data_gen.channelize/synthesize
 * (python/data_gen/channelize.py:19-92, synthesize.py:27-95).
 *
 * Everything crossing this boundary is plain C: integers, doubles, pointers, sizes.
 * No C++ or torch types.  No exception crosses it: every entry point returns a
 * pfb_status and pfb_last_error() returns the thread-local message (mirrors the
 * reference's error(...) checks, e.g. InverseFilterBank.m:83-85).
 *
 * Data layout (complex float32, interleaved re/im = pfb_cf32):
 *   single-channel time series : in[pol * pol_stride + t]
 *   channelised data           : x[pol * pol_stride + t * n_chan + c]
 *                                (per polarisation the Matlab memory order of an
 *                                 (n_chan, n_dat) slice: channel fastest, then time)
 * Buffers are device pointers (PFB_MEM_DEVICE, zero copy on the given stream) or host
 * pointers (PFB_MEM_HOST, staged through the plan's device buffers; synchronous).
 *
 * Threading: a plan is bound to one device and is not thread safe (it carries the
 * streaming state).  Different plans are independent; multi-GPU = one plan per GPU.
 *
 * Streams (pinned by tests/test_gpu_streams.py; the fork and join of the pipelined round
 * trip by tests/test_gpu_roundtrip.py):
 *   - Every device operation of a call — kernels, copies, memsets, the moves of a stream
 *     object's carry — is enqueued on the `stream` the call is given and on no other; the
 *     call returns when they are enqueued (the PFB_MEM_HOST paths, pfb_quantize and the
 *     *_quantised_to_dada calls with a `scale`, and the pfb_purity_score_* functions also
 *     wait for that stream).  Nothing is
 *     ordered against the default stream or any other stream of the process.
 *   - The round trip (pfb_roundtrip_*) in its pipelined form runs its analysis on a
 *     stream of the plan's own, which is forked from the given stream at the start of the
 *     call and joined to it before the call returns; the fused form uses the given stream
 *     alone.  Either way the call is, to the caller, work on the given stream.
 *   - The plan-free utilities (pfb_dada_*, pfb_gather_channels, pfb_corner_turn,
 *     pfb_quantize, pfb_testvec_generate, pfb_purity_score_*) share no device state across
 *     streams: calls on different streams, from one host thread or several, may overlap
 *     (one caveat for a captured pfb_quantize: see there).
 *   - A plan may be called on different streams in turn, but its buffers (carry, scratch,
 *     staging, the quantised calls' product, partial sums and stats block) are reused from call to call and nothing inside the plan orders one call
 *     after the one before: the caller orders consecutive calls of one plan that go to
 *     different streams (an event recorded after the first and waited on before the next).
 */
#ifndef PFB_API_H
#define PFB_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFB_API_VERSION 1

typedef struct pfb_cf32 {
  float re;
  float im;
} pfb_cf32;

typedef enum pfb_status {
  PFB_OK = 0,
  PFB_ERR_INVALID_ARG = 1,      /* e.g. N*de/nu, Ov*de/nu or Nf*de/nu not integral */
  PFB_ERR_UNSUPPORTED = 2,      /* size combination with no compiled kernel */
  PFB_ERR_HIP = 3,              /* HIP runtime error (message has hipGetErrorString) */
  PFB_ERR_OOM = 4,
  PFB_ERR_BUFFER_TOO_SMALL = 5, /* output capacity smaller than the required length */
  PFB_ERR_NO_DEVICE = 6
} pfb_status;

typedef enum pfb_analysis_variant {
  PFB_ANALYSIS_BUNTON = 0, /* polyphase_analysis.m */
  PFB_ANALYSIS_PADDED = 1, /* polyphase_analysis_padded.m */
  PFB_ANALYSIS_LOWCBF = 2  /* polyphase_analysis_lowcbf.m -> PSTFilterbank.m: the SKA-Low CBF
                              PST filterbank (n_chan 256, os 4/3, 3072 taps fixed); 216
                              output channels; 1536 zeros pre-padded on the plan's first call.
                              "First call" = the first pfb_analysis_execute /
                              pfb_filterbank_execute that passes every argument check (it may
                              return no rows, as the Matlab wrapper's first call may); a call
                              rejected with an error status (null output, capacity, stride)
                              leaves the padding pending and the length queries unchanged, so
                              the corrected retry returns the rows a first call returns.
                              pfb_filterbank_reset makes the padding due again. */
} pfb_analysis_variant;

typedef enum pfb_mem {
  PFB_MEM_DEVICE = 0,
  PFB_MEM_HOST = 1
} pfb_mem;

/* PFBWindow.m:10-16 lookup names, plus CUSTOM (explicit coefficients). */
typedef enum pfb_window_kind {
  PFB_WINDOW_NONE = 0,    /* no_window / identity_taper */
  PFB_WINDOW_TUKEY = 1,   /* PFBWindow.m:30-44 */
  PFB_WINDOW_TOP_HAT = 2, /* PFBWindow.m:63-68 */
  PFB_WINDOW_HANN = 3,    /* PFBWindow.m:72-99 (temporal: applied per channel row) */
  PFB_WINDOW_CUSTOM = 4   /* explicit coefficients (temporal: Nf values; spectral: L values) */
} pfb_window_kind;

/* ---------------------------------------------------------------- analysis */
typedef struct pfb_analysis_desc {
  int32_t variant;     /* pfb_analysis_variant */
  int32_t n_chan;      /* "block" = N channels (polyphase_analysis.m:3) */
  int32_t os_nu;       /* os_factor.nu */
  int32_t os_de;       /* os_factor.de */
  const double* taps;  /* prototype FIR taps (host memory, copied at create) */
  int64_t n_taps;
  int32_t n_pol;       /* polarisations processed per call */
  int32_t device;      /* HIP device ordinal */
} pfb_analysis_desc;

typedef struct pfb_analysis_plan pfb_analysis_plan;

/* Replaces: FilterBank constructor (FilterBank.m:26-63) + read_fir_filter_coeff. */
pfb_status pfb_analysis_plan_create(const pfb_analysis_desc* desc, pfb_analysis_plan** plan);
pfb_status pfb_analysis_plan_destroy(pfb_analysis_plan* plan);
/* The checks and host-side tables of pfb_analysis_plan_create without a device (nothing
 * allocated, nothing kept): the status create would return before touching the GPU. */
pfb_status pfb_analysis_plan_validate(const pfb_analysis_desc* desc);

/* Number of output samples per channel for n_dat input samples of a stateless call:
 * Bunton K = floor((n_dat - P*N)/M) (polyphase_analysis.m:62), padded K = floor(n_dat/M)
 * (polyphase_analysis_padded.m:75). */
int64_t pfb_analysis_output_length(const pfb_analysis_plan* plan, int64_t n_dat);

/* Channels per output row: n_chan, or 216 for PFB_ANALYSIS_LOWCBF
 * (polyphase_analysis_lowcbf.m:43, PSTFilterbank.m:44). */
int32_t pfb_analysis_output_channels(const pfb_analysis_plan* plan);

/* Stateless analysis — replaces polyphase_analysis(in, filt, block, os_factor) and
 * polyphase_analysis_padded(...).  in: n_pol series of n_dat samples; out: n_pol x
 * (K x n_chan).  *n_out receives K. */
pfb_status pfb_analysis_execute(pfb_analysis_plan* plan, const pfb_cf32* in,
                                int64_t in_pol_stride, int64_t n_dat, pfb_cf32* out,
                                int64_t out_pol_stride, int64_t out_capacity,
                                int64_t* n_out, int32_t mem, void* stream);

/* Stateful stream — replaces FilterBank.execute (FilterBank.m:65-128): prepends the
 * carried-over input, runs the analysis, trims the output to a multiple of nu and
 * keeps input[T_out*M:] for the next call.  Input rounding hooks (rndInput etc.) are
 * applied by the host mirror before this call.  Device buffers: in_pol_stride >= n_in and
 * out_pol_stride >= T_out * n_chan (the samples returned per pol), else
 * PFB_ERR_INVALID_ARG with the stream state unchanged; nothing outside rows [0, T_out) of
 * each pol is written, with one exception.  Padded variant, device output: when
 * out_capacity covers all K computed rows (not just the *n_out = T_out kept ones) AND
 * out_pol_stride >= K * n_chan, rows [T_out, K) of each pol are used as scratch (the
 * circular shift spans all K rows); K - T_out < os_nu.  With a smaller capacity or pols
 * packed closer than K rows the K rows go through a staging buffer and only rows
 * [0, T_out) are written. */
pfb_status pfb_filterbank_execute(pfb_analysis_plan* plan, const pfb_cf32* in,
                                  int64_t in_pol_stride, int64_t n_in, pfb_cf32* out,
                                  int64_t out_pol_stride, int64_t out_capacity,
                                  int64_t* n_out, int32_t mem, void* stream);
int64_t pfb_filterbank_buffered(const pfb_analysis_plan* plan);
pfb_status pfb_filterbank_reset(pfb_analysis_plan* plan);
/* Rows the next pfb_filterbank_execute of n_in samples returns (the nu-trimmed T_out of
 * FilterBank.m:93-104 over the carried + new samples); -1 on a null plan. */
int64_t pfb_filterbank_output_rows(const pfb_analysis_plan* plan, int64_t n_in);

/* The same stream call writing the channelised product strided (device buffers only):
 * bin c of row k of polarisation p goes to
 * out[p * out_pol_stride + k * row_stride + j * chan_stride], j = c, or with sel_n > 0
 * the cascade's channel chomp j = c < sel_split ? c : c - sel_shift (bins in
 * [sel_split, sel_split + sel_shift) and j >= sel_n dropped).  Serves the two-stage
 * cascade (TwoStageFilterBank.m:92-110): stage 1 written channel-major (row_stride 1,
 * chan_stride = series length) is the per-channel input of stage 2 with no corner turn;
 * stage 2 written with row_stride nch1*nch2, out_pol_stride nch2 and the chomp
 * (sel_split nch2/2-1, sel_shift = dropped bins) is the assembled output of
 * TwoStageFilterBank.m:102-105 with no gather.
 * Plans that take it: PFB_ANALYSIS_BUNTON on the streaming kernel (N = 256), and every
 * PFB_ANALYSIS_PADDED plan pfb_filterbank_execute accepts (the fused kernels, N <= 256 with
 * <= 32 tap phases, and the FIR + row-FFT path: N > 256, or more phases).
 * PFB_ERR_UNSUPPORTED for other Bunton plans and for PFB_ANALYSIS_LOWCBF.
 * Padded plans: the call computes K = floor((carried + n_in) / M) rows, FIR row kg becomes
 * output row k = (kg - sds) mod K (polyphase_analysis_padded.m:156), and the *n_out = T_out
 * = K - K mod os_nu rows k < T_out are stored through the layout.  Rows [T_out, K) are
 * dropped at the store: unlike pfb_filterbank_execute there are no scratch rows in the
 * caller's buffer and no staging copy — exactly the mapped elements are written.  The
 * values are those of pfb_filterbank_execute, bit for bit, and the carry is the same
 * (FilterBank.m:119-126).  Range limiting: a shifted row lands anywhere in [0, T_out) of
 * its pol, so these kernels use guarded plain stores with 64-bit addresses (not a buffer
 * descriptor): each store is predicated on k < T_out and a kept bin, and the only extent
 * limit is that row_stride and chan_stride fit in 31 bits (else PFB_ERR_UNSUPPORTED).  The
 * 4096-point row FFT stores channel-major output as 16-byte row pairs when `out` is 16-byte
 * aligned and out_pol_stride and chan_stride are even, else as 8-byte elements.  (The
 * Bunton streaming kernel range-limits each 16-row step with a buffer descriptor, whose
 * extent must fit 32-bit offsets: (64 row_stride + jn chan_stride + 1) * 8 <= 0x7ffffff0 with
 * jn = sel_n, or n_chan without a chomp, else PFB_ERR_UNSUPPORTED — row_stride 1 admits
 * chan_stride <= 1048575 at 256 bins, chan_stride 1 admits row_stride <= 4194299.)
 * Checks, all before any launch or change of the stream state: a bad layout (a stride
 * <= 0, a negative sel_*, sel_split + sel_shift or sel_n beyond the channels) or
 * in_pol_stride < n_in is PFB_ERR_INVALID_ARG; out_capacity is the number of pfb_cf32
 * elements available from `out`: a call whose furthest written element ((n_pol-1)
 * out_pol_stride + (rows-1) row_stride + (j_max) chan_stride) lies beyond it fails with
 * PFB_ERR_BUFFER_TOO_SMALL and writes nothing.  *n_out: the layout checks (the plan, the
 * strides and sel_*, the stride and extent limits above) come first, and a call they refuse
 * (PFB_ERR_INVALID_ARG, PFB_ERR_UNSUPPORTED) leaves *n_out as it was; every later outcome,
 * PFB_ERR_BUFFER_TOO_SMALL included, has set it to T_out. */
pfb_status pfb_filterbank_execute_strided(pfb_analysis_plan* plan, const pfb_cf32* in,
                                          int64_t in_pol_stride, int64_t n_in, pfb_cf32* out,
                                          int64_t out_pol_stride, int64_t row_stride,
                                          int64_t chan_stride, int32_t sel_split,
                                          int32_t sel_shift, int32_t sel_n,
                                          int64_t out_capacity, int64_t* n_out, void* stream);

/* ---------------------------------------------------------------- synthesis */
typedef struct pfb_synthesis_desc {
  int32_t n_chan;             /* channels in the input */
  int32_t os_nu;
  int32_t os_de;
  int32_t input_fft_length;   /* Nf */
  int32_t input_overlap;      /* Ov */
  int32_t spans_nyquist;      /* input_fully_spans_Nyquist_zone (1 = oversampled Low/Mid) */
  int32_t combine;            /* coarse channels combined (polyphase_synthesis.m:198-239) */
  int32_t apply_deripple;     /* deripple.apply_deripple */
  const double* taps;         /* deripple.filter_coeff (host, copied) */
  int64_t n_taps;
  int32_t temporal_taper;     /* pfb_window_kind */
  const double* temporal_coeffs; /* CUSTOM: Nf coefficients */
  int32_t spectral_taper;     /* pfb_window_kind (NONE = identity_taper) */
  const double* spectral_coeffs; /* CUSTOM: L = Nf*de/nu*n_chan coefficients */
  int32_t n_pol;
  int32_t device;
} pfb_synthesis_desc;

typedef struct pfb_synthesis_plan pfb_synthesis_plan;

/* Replaces: InverseFilterBank constructor (InverseFilterBank.m:33-43) incl. the
 * PFBWindow lookup and the freqz-based deripple response (polyphase_synthesis.m:138-150). */
pfb_status pfb_synthesis_plan_create(const pfb_synthesis_desc* desc, pfb_synthesis_plan** plan);
pfb_status pfb_synthesis_plan_destroy(pfb_synthesis_plan* plan);
/* The checks and host-side tables (window, deripple gains, four-step twiddles) of
 * pfb_synthesis_plan_create without a device: the status create would return before
 * touching the GPU. */
pfb_status pfb_synthesis_plan_validate(const pfb_synthesis_desc* desc);

/* n_blocks * output_keep for n_dat channelised samples (polyphase_synthesis.m:112-131). */
int64_t pfb_synthesis_output_length(const pfb_synthesis_plan* plan, int64_t n_dat);

/* Stateless synthesis — replaces polyphase_synthesis(in, spans, Nf, os, deripple,
 * sample_offset, overlap, t_taper, s_taper, combine).  sample_offset is 1-based like
 * Matlab (:99).  in: n_pol x (n_dat x n_chan); out: n_pol series. */
pfb_status pfb_synthesis_execute(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                 int64_t in_pol_stride, int64_t n_dat, int64_t sample_offset,
                                 pfb_cf32* out, int64_t out_pol_stride, int64_t out_capacity,
                                 int64_t* n_out, int32_t mem, void* stream);

/* Stateful stream — replaces InverseFilterBank.execute (InverseFilterBank.m:63-137):
 * carry-over of n_dat - B*keep samples rounded up to a multiple of nu. */
pfb_status pfb_inverse_filterbank_execute(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                          int64_t in_pol_stride, int64_t n_in, pfb_cf32* out,
                                          int64_t out_pol_stride, int64_t out_capacity,
                                          int64_t* n_out, int32_t mem, void* stream);
int64_t pfb_inverse_filterbank_buffered(const pfb_synthesis_plan* plan);
pfb_status pfb_inverse_filterbank_reset(pfb_synthesis_plan* plan);
/* InverseFilterBank.sample_offset (InverseFilterBank.m:12, 0-based, default 0): every
 * pfb_inverse_filterbank_execute call synthesises the concatenated rows (carry + input)
 * from row sample_offset on — polyphase_synthesis(..., sample_offset+1, ...) at :92-96 —
 * while the carry still starts at the consumed blocks' end (:104-133), so the offset is
 * skipped again at the head of every call's concatenation, as the Matlab object does. */
pfb_status pfb_inverse_filterbank_set_sample_offset(pfb_synthesis_plan* plan, int64_t sample_offset);

/* Blocks processed per channel-IFFT/block-kernel chunk (scratch = chunk * keep rows). */
pfb_status pfb_synthesis_set_chunk_blocks(pfb_synthesis_plan* plan, int32_t blocks);

/* Where the fused round trip's synthesis gets its stage-1 rows (the channel IFFT of each
 * channelised row = N^2 x the analysis FIR sums).  STORED: the analysis kernel writes them
 * to the plan's scratch and the synthesis reads them back.  RECOMPUTED (N = 256 streaming
 * shapes, Nf 256): the analysis writes only the channelised product and the synthesis
 * evaluates the rows it needs from the input series — the same FIR sums in the same order,
 * so the output is bit-identical, with the stage-1 rows never crossing HBM.  AUTO: the
 * measured-faster one for the shape.  Shapes without a recomputing
 * kernel use STORED whatever is set.  Reference: polyphase_analysis.m:88-121 and
 * polyphase_synthesis.m:282-285 (the channel IFFT this factors). */
typedef enum pfb_stage1_rows {
  PFB_STAGE1_AUTO = 0,
  PFB_STAGE1_STORED = 1,
  PFB_STAGE1_RECOMPUTED = 2
} pfb_stage1_rows;
pfb_status pfb_synthesis_set_stage1_rows(pfb_synthesis_plan* plan, int32_t mode);
/* Where the plan's last synthesis launch got its stage-1 rows: PFB_STAGE1_STORED (read
 * from rows a channel IFFT or the analysis wrote), PFB_STAGE1_RECOMPUTED (evaluated from
 * the input series), 0 before any launch, -1 for a null plan.  A diagnostic: a caller that
 * asked for RECOMPUTED can tell whether the shape took it (no reference counterpart). */
int32_t pfb_synthesis_last_stage1_rows(const pfb_synthesis_plan* plan);

/* ---------------------------------------------------------------- round trip */
/* Analysis followed by synthesis of its output — replaces the analysis -> synthesis
 * sequence of test_data_pipeline.m:114,132 (and data_gen/pipeline.py:71-75).
 * Device memory only.  in: n_pol series of n_dat samples; chan: the full channelised
 * product (n_pol x K x n_chan, written as pfb_analysis_execute writes it); out: the
 * synthesis of chan(:, :, sample_offset:end) as pfb_synthesis_execute computes it.
 * When the analysis kernel can emit the synthesis stage-1 rows (N = 256 streaming
 * shapes, the N > 256 register-window FIR) and no chunk size is set, the two run fused:
 * `chan` is bit-identical to pfb_analysis_execute and `out` agrees with
 * pfb_synthesis_execute to ~1e-7 (the stage-1 rows are N^2 x the FIR sums, the exact
 * channel IFFT of the unrounded row).  Otherwise the call is pipelined in chunks of
 * synthesis blocks (pfb_synthesis_set_chunk_blocks, default 64) with the analysis on a
 * second stream, and both results are bit-identical to the separate calls.  Ordered
 * after prior work on `stream`; later work on `stream` sees all of it (graph-capturable). */
pfb_status pfb_roundtrip_execute(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                 const pfb_cf32* in, int64_t in_pol_stride, int64_t n_dat,
                                 pfb_cf32* chan, int64_t chan_pol_stride, int64_t chan_capacity,
                                 int64_t* n_chan_rows, int64_t sample_offset, pfb_cf32* out,
                                 int64_t out_pol_stride, int64_t out_capacity, int64_t* n_out,
                                 void* stream);

/* The fused round trip above in two halves, for a caller that pipelines consecutive
 * blocks over two streams (block i's synthesis beside block i+1's analysis, each block on
 * its own plan pair).  pfb_roundtrip_analysis_execute runs the analysis kernel of the
 * fused path: it writes the channelised product (as pfb_roundtrip_execute does) and the
 * synthesis stage-1 rows into `synthesis`'s scratch.  pfb_roundtrip_synthesis_execute
 * turns those rows into the output; n_dat and sample_offset must be the analysis half's.
 * The halves' results equal pfb_roundtrip_execute's fused path bit for bit.  The caller
 * orders them (synthesis after the analysis, the next analysis on the same pair after
 * the synthesis), e.g. with events.  With recomputed stage-1 rows
 * (pfb_synthesis_set_stage1_rows) the analysis half writes no rows: the synthesis half
 * re-reads `in`, which must stay allocated and unchanged until it has run.
 * PFB_ERR_UNSUPPORTED when the plans take the chunked pipeline (see above);
 * PFB_ERR_INVALID_ARG from the synthesis half when the plan holds no analysis half of this
 * analysis plan with the same n_dat and sample_offset (another shape, another plan, or a
 * whole round trip ran on the pair since).  Reference: the same lines as
 * pfb_roundtrip_execute. */
pfb_status pfb_roundtrip_analysis_execute(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                          const pfb_cf32* in, int64_t in_pol_stride, int64_t n_dat,
                                          pfb_cf32* chan, int64_t chan_pol_stride, int64_t chan_capacity,
                                          int64_t* n_chan_rows, int64_t sample_offset, void* stream);
pfb_status pfb_roundtrip_synthesis_execute(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                           int64_t n_dat, int64_t sample_offset, pfb_cf32* out,
                                           int64_t out_pol_stride, int64_t out_capacity, int64_t* n_out,
                                           void* stream);

/* Round-trip output length estimate — replaces calc_output_nbins(nbins, channels,
 * os_factor, filter_taps, input_fft_length, input_overlap) (calc_output_nbins.m:17-27):
 * Matlab double arithmetic with its floor()s, so a non-integral normalize(os, n) gives the
 * same fractional result Matlab does.  Host-only arithmetic (no device needed). */
double pfb_calc_output_nbins(int64_t nbins, int32_t channels, int32_t os_nu, int32_t os_de,
                             int64_t filter_taps, int32_t input_fft_length, int32_t input_overlap);

/* ---------------------------------------------------------------- data formats */
/* Sample order of a DADA file's data section. */
typedef enum pfb_dada_order {
  PFB_DADA_TFP = 0,   /* time, channel, polarisation, re/im (reshape_dada_data.m:23-30,
                         write_dada_data.m:32-50) */
  PFB_DADA_LOWCBF = 1 /* heaps of 32 samples: [heap][chan][pol][sample], INSTRUMENT LowCBF
                         (reshape_low_cbf_data.m:14-43, DADARead.m:74-78) */
} pfb_dada_order;

/* DADA data section (device memory, NBIT 8/16/32/64 signed integer / float samples,
 * NDIM 1 or 2) -> [pol][t][chan] complex float32.  Replaces read_dada_file.m:36-47 +
 * reshape_dada_data.m (and DADARead.generate, DADARead.m:58-83, incl. its cast of
 * integer samples to floating point).  NBIT 64 is rounded to float32 (the engine's
 * arithmetic type).  Asynchronous on `stream`. */
pfb_status pfb_dada_unpack(const void* in, int32_t nbit, int32_t ndim, int32_t order,
                           int64_t n_dat, int32_t n_chan, int32_t n_pol, pfb_cf32* out,
                           int64_t out_pol_stride, void* stream);

/* Synthesis straight from a DADA data section (DADARead.m:58-83 followed by
 * InverseFilterBank.m:92-96 / polyphase_synthesis).  Device memory only.  `in` holds n_dat
 * (n_in) rows x the plan's n_chan x n_pol x ndim values of nbit, in `order` (pfb_dada_order).
 * The result, *n_out, the status codes, pfb_inverse_filterbank_buffered and the stream state
 * are those of pfb_dada_unpack into a packed buffer followed by pfb_synthesis_execute /
 * pfb_inverse_filterbank_execute, bit for bit.  Every check (NBIT 8/16/32/64, NDIM 1/2, the
 * order, LowCBF rows a multiple of 32, null buffers, and the capacity and stride checks of
 * the cf32 calls) runs before any launch or state change: a rejected stream call leaves the
 * carry untouched.
 * FUSED: the channel IFFT reads the section's own bytes (NBIT 8/16, NDIM 2, a section
 * aligned to a complex sample, channel counts below 4096, a plan without combine
 * permutation, temporal-taper gain or spectral taper) and the unpacked samples never cross
 * HBM.  A stream call reads the blocks made of new rows only in place; the blocks that
 * start in the carry are stitched from the cf32 carry and the unpacked head of the section,
 * and the new carry is the unpacked tail.  STAGED: any other plan or format is unpacked into
 * a plan-owned buffer and runs the cf32 path.  pfb_synthesis_last_dada_input: which of the
 * two the plan's last DADA call took (FUSED when any of its channel IFFTs read the section
 * in place), NONE before one or after a cf32 call, -1 for a null plan. */
typedef enum pfb_dada_input {
  PFB_DADA_INPUT_NONE = 0,
  PFB_DADA_INPUT_FUSED = 1,
  PFB_DADA_INPUT_STAGED = 2
} pfb_dada_input;
pfb_status pfb_synthesis_execute_dada(pfb_synthesis_plan* plan, const void* in, int32_t nbit,
                                      int32_t ndim, int32_t order, int64_t n_dat,
                                      int64_t sample_offset, pfb_cf32* out, int64_t out_pol_stride,
                                      int64_t out_capacity, int64_t* n_out, void* stream);
pfb_status pfb_inverse_filterbank_execute_dada(pfb_synthesis_plan* plan, const void* in,
                                               int32_t nbit, int32_t ndim, int32_t order,
                                               int64_t n_in, pfb_cf32* out, int64_t out_pol_stride,
                                               int64_t out_capacity, int64_t* n_out, void* stream);
int32_t pfb_synthesis_last_dada_input(const pfb_synthesis_plan* plan);

/* Analysis straight from a single-channel DADA data section (DADARead.m:58-83 followed by
 * polyphase_analysis / FilterBank.m:65-128): what a file or a beamformer delivers for one
 * channel, [t][pol][re, im] with the polarisations alternating sample by sample.  Device
 * memory only.  `in` holds n_dat (n_in) samples x 1 channel x the plan's n_pol x ndim values
 * of nbit, in `order` (pfb_dada_order); in TFP order complex sample t of polarisation p is
 * element t * n_pol + p.  The output, *n_out, the status codes, pfb_filterbank_buffered,
 * pfb_filterbank_output_rows and the stream state are those of pfb_dada_unpack into a packed
 * [pol][t] buffer followed by pfb_analysis_execute / pfb_filterbank_execute, bit for bit: the
 * integer-to-float cast is exact and the FIR sums run in the same order.  Every check (NBIT
 * 8/16/32/64, NDIM 1/2, the order, LowCBF rows a multiple of 32, null buffers, and the
 * capacity and stride checks of the cf32 calls) runs before any launch or state change: a
 * rejected stream call leaves the carry untouched, and a rejected call on a
 * PFB_ANALYSIS_LOWCBF plan leaves the first-call pre-padding pending (pfb_analysis_variant).
 * cf32 and DADA stream calls may alternate on one plan: the carry stays packed cf32.
 * FUSED: the analysis kernel loads the section's bytes itself, one range-checked buffer load
 * of 2 / 4 / 8 bytes per complex sample, and no unpacked copy crosses HBM — NBIT 8, 16
 * (integers) and 32 (float), NDIM 2, TFP order, a section aligned to one complex sample, and a
 * plan on the streaming kernel (PFB_ANALYSIS_BUNTON with n_chan 256, os 8/7 or 4/3, 12 or 13
 * tap phases, and PFB_ANALYSIS_LOWCBF; stateless and stream calls — a stream call reads the
 * carry through its cf32 descriptor in the same launch) or on the LDS-shared FIR of the
 * n_chan > 256 path (os 8/7 or 4/3, <= 32 phases; the stateless call, and a stream call with
 * nothing buffered).  Descriptor limit: 512 rows of one workgroup at n_pol * 2 * nbit / 8 bytes
 * per sample must fit 32-bit offsets, n_pol * (nbit / 4) * n_chan * 512 <= 0x7ffffff0 (n_chan
 * 256: n_pol <= 2047 / 4095 / 8191 at NBIT 32 / 16 / 8); more polarisations are STAGED.  No
 * byte outside the section is loaded, and of a two-polarisation section
 * a workgroup loads only its own polarisation's samples.  STAGED: every other format (NBIT
 * 64, NDIM 1, LowCBF order, a misaligned section), plan or stream state is unpacked into a
 * plan-owned buffer — a stream call's samples straight behind the carry in the concatenation
 * buffer — and runs the cf32 path, so these calls accept every plan the cf32 calls accept.
 * pfb_analysis_last_dada_input: which of the two the plan's last DADA call took, NONE before
 * one or after a cf32 call, -1 for a null plan.  (Measured A/B against the unpack-then-execute
 * pair: DESIGN.md §4.6.) */
pfb_status pfb_analysis_execute_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit,
                                     int32_t ndim, int32_t order, int64_t n_dat, pfb_cf32* out,
                                     int64_t out_pol_stride, int64_t out_capacity, int64_t* n_out,
                                     void* stream);
pfb_status pfb_filterbank_execute_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit,
                                       int32_t ndim, int32_t order, int64_t n_in, pfb_cf32* out,
                                       int64_t out_pol_stride, int64_t out_capacity, int64_t* n_out,
                                       void* stream);
int32_t pfb_analysis_last_dada_input(const pfb_analysis_plan* plan);

/* Analysis writing its product straight into a DADA data section (polyphase_analysis /
 * FilterBank.m:65-128 followed by write_dada_data.m:32-50): TFP order, NDIM 2, out_nbit 8 /
 * 16 (integers), 32 (float) or 64 (double).  Device memory only.  Element (row k, channel c,
 * polarisation p) of the section, with C = pfb_analysis_output_channels and P the plan's
 * n_pol, lies at byte ((k * C + c) * P + p) * 2 * out_nbit / 8 of `out`, re then im.  The
 * bytes written, *n_out, the status codes, pfb_filterbank_buffered,
 * pfb_filterbank_output_rows and the stream state are those of the corresponding cf32-output
 * call (pfb_analysis_execute, pfb_filterbank_execute and their _dada twins) into a packed
 * [pol][k][c] buffer, both components multiplied by out_scale in float32, followed by
 * pfb_dada_pack at out_nbit, bit for bit: the same float32 operations in the same order.
 * Exactly rows [0, *n_out) of the section are written and not one byte beyond; the rows a
 * stream call trims to a multiple of the oversampling numerator and the spare rows of the
 * padded variant have no place in `out`.  Every check runs before any launch or state change:
 * a rejected stream call leaves the carry and the buffered count untouched, and a rejected
 * call on a PFB_ANALYSIS_LOWCBF plan leaves the first-call pre-padding pending.
 * PFB_ERR_INVALID_ARG: a null plan, null buffers when samples are given or rows are due,
 * out_nbit not 8/16/32/64, a non-finite out_scale, `out` not aligned to one value of out_nbit,
 * and the input-side conditions of the corresponding call.  PFB_ERR_BUFFER_TOO_SMALL, with
 * nothing written: out_capacity_bytes below rows * C * P * 2 * out_nbit / 8.  cf32 and DADA
 * input, and cf32 and DADA output stream calls may alternate on one plan: the carry stays
 * packed cf32.
 * FUSED: the analysis kernel converts and stores the samples itself, one range-checked buffer
 * store of 2 / 4 / 8 bytes per complex sample, and the cf32 product never crosses HBM —
 * out_nbit 8, 16 or 32, `out` aligned to one complex sample, and a plan on the streaming
 * kernel (PFB_ANALYSIS_BUNTON with n_chan 256, os 8/7 or 4/3, 12 or 13 tap phases, and
 * PFB_ANALYSIS_LOWCBF; stateless and stream calls).  Descriptor limit: the 16 rows of one step
 * must fit 32-bit offsets, 16 * C * P * (out_nbit / 4) <= 0x7ffffff0 (C and P as above), which
 * holds for every plan (P <= 65535).  The _dada_to_dada calls read the input
 * section in place as well when it qualifies for pfb_analysis_execute_dada's FUSED and its
 * nbit equals out_nbit or out_nbit is 32 (an integer file channelised into a float one); any
 * other input section is unpacked into the plan's staging buffer first and the output stays
 * fused (pfb_analysis_last_dada_input then reports STAGED).
 * FUSED as well, under the same conditions on out_nbit and `out`: every plan with n_chan 4096
 * (PFB_ANALYSIS_BUNTON and PFB_ANALYSIS_PADDED; stateless and stream calls).  Their FIR fills the
 * plan's scratch rows as ever and the 4096-point row FFT converts and stores the section itself,
 * one descriptor per row of the section, 4096 * P * (out_nbit / 4) <= 0x7ffffff0, which holds
 * for every plan; with two polarisations one workgroup stores both, 4 / 8 / 16 bytes per bin.  A
 * padded stream call computes the rows its circular shift spans and makes only the *n_out kept
 * ones; no buffer holds the others.  FIR and row FFT are launches of their own, so the
 * _dada_to_dada calls read the input section exactly as pfb_analysis_execute_dada does on the
 * same plan and state, whatever the two NBITs.
 * STAGED: every other plan (the padded variant with its circular row shift and the FIR +
 * row-FFT path at n_chan other than 4096, the other n_chan of the Bunton variant), out_nbit 64
 * and an `out` aligned to a value but not to a
 * complex sample run the cf32 path into a plan-owned buffer, then one scaled pack launch; so
 * these calls accept every plan the cf32 calls accept.
 * pfb_analysis_last_dada_output: which of the two the plan's last such call took, NONE before
 * one or after a cf32-output call, -1 for a null plan.  (Measured A/B against the pair:
 * DESIGN.md §4.7.) */
typedef enum pfb_dada_output {
  PFB_DADA_OUTPUT_NONE = 0,
  PFB_DADA_OUTPUT_FUSED = 1,
  PFB_DADA_OUTPUT_STAGED = 2
} pfb_dada_output;
pfb_status pfb_analysis_execute_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in,
                                        int64_t in_pol_stride, int64_t n_dat, void* out,
                                        int32_t out_nbit, float out_scale, int64_t out_capacity_bytes,
                                        int64_t* n_out, void* stream);
pfb_status pfb_filterbank_execute_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in,
                                          int64_t in_pol_stride, int64_t n_in, void* out,
                                          int32_t out_nbit, float out_scale, int64_t out_capacity_bytes,
                                          int64_t* n_out, void* stream);
pfb_status pfb_analysis_execute_dada_to_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit,
                                             int32_t ndim, int32_t order, int64_t n_dat, void* out,
                                             int32_t out_nbit, float out_scale,
                                             int64_t out_capacity_bytes, int64_t* n_out, void* stream);
pfb_status pfb_filterbank_execute_dada_to_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit,
                                               int32_t ndim, int32_t order, int64_t n_in, void* out,
                                               int32_t out_nbit, float out_scale,
                                               int64_t out_capacity_bytes, int64_t* n_out, void* stream);
int32_t pfb_analysis_last_dada_output(const pfb_analysis_plan* plan);

/* The FilterBank's quantised output as a DADA data section (FilterBank.m:106-113 followed by
 * write_dada_data.m:32-50): the product is rescaled to the target rms, rounded to integers,
 * multiplied by out_scale and stored at out_nbit.  With x the cf32 product of the
 * corresponding *_to_dada call (rows [0, *n_out) of every polarisation, cnt = rows * C * P
 * complex samples):
 *   scale = rms / sqrt(var),  var = (sum |x|^2 - ((sum re)^2 + (sum im)^2) / cnt) / (cnt - 1)
 * (var(x, 0, "all"), summed in double; a zero variance is not special-cased, as in
 * pfb_quantize), and per component
 *   q = roundf((float)scale * x),  y = out_scale * q (float32),  sample = cast(y)
 * with pfb_dada_pack's cast (round half away from zero, saturate): the operations of
 * pfb_quantize, a float32 scale pass and pfb_dada_pack, in that order — given the same float32
 * scale, their bytes.  rms <= 0: round only ((float)scale = 1, no moments are taken).
 * The section layout, *n_out, the status codes, pfb_filterbank_buffered,
 * pfb_filterbank_output_rows, the carry and the LowCBF first-call pre-padding are those of the
 * matching *_to_dada call; exactly rows [0, *n_out) are written and not one byte beyond.  Every
 * check runs before any launch or state change: a rejected call leaves `out`, the carry and the
 * pending pre-padding untouched.  PFB_ERR_INVALID_ARG: the *_to_dada conditions and a
 * non-finite rms.  PFB_ERR_BUFFER_TOO_SMALL, with nothing written: out_capacity_bytes below
 * rows * C * P * 2 * out_nbit / 8.  A call that yields 0 rows writes nothing, sets *scale = 1
 * and advances the stream state as the cf32 call does.
 * FUSED: a plan on the streaming kernel (as for *_to_dada's FUSED, any out_nbit).  Three
 * launches: the analysis kernel, which stores the cf32 product into a buffer of the plan and
 * sums the moments of exactly the values it stores (per-workgroup partial sums, ordinary
 * stores); one workgroup that adds the partial sums in a fixed order and forms the scale; one
 * pass that reads the product once and writes the section.
 * STAGED: every other plan (padded, the one-launch N <= 256 kernel, FIR + row FFT), or
 * pfb_analysis_set_quantiser_moments(plan, PFB_QUANTISER_MOMENTS_STAGED): the plan's cf32 path
 * into the same buffer, one pass over it for the partial sums, then the same two launches.
 * PFB_QUANTISER_MOMENTS_FUSED on a plan that cannot take it: PFB_ERR_UNSUPPORTED from the
 * execute call, nothing launched.  AUTO (the default) takes FUSED where the plan allows it.
 * The _dada calls read the input section in place wherever pfb_analysis_execute_dada does,
 * whatever out_nbit is; any other section is unpacked into the plan's staging buffer first.
 * pfb_analysis_last_quantiser: the path of the plan's last such call (of the product, also
 * when rms <= 0), NONE before one or after a cf32-output or *_to_dada call, -1 for a null plan;
 * pfb_analysis_last_dada_output then reports NONE.
 * Streams: everything is enqueued on the given stream.  The product buffer, the partial sums
 * and the 32-byte block {sum re, sum im, sum |x|^2, scale} belong to the plan — nothing is
 * shared per device or per stream — and grow only with the call's length, like the plan's
 * other call-length buffers: the first call, or a longer one, may allocate and wait for the
 * device.  With scale == NULL the call does not wait for the device and can be captured into a
 * graph (after one call of that length outside the capture); with scale non-null it copies
 * the double back and synchronises the stream.
 * Determinism: no floating-point atomics; the same plan, input and launch grid give the same
 * scale bits and the same bytes.  (Measured A/B against the pair: DESIGN.md §4.11.) */
typedef enum pfb_quantiser_moments {
  PFB_QUANTISER_MOMENTS_AUTO = 0,
  PFB_QUANTISER_MOMENTS_FUSED = 1,
  PFB_QUANTISER_MOMENTS_STAGED = 2
} pfb_quantiser_moments;
typedef enum pfb_quantiser {
  PFB_QUANTISER_NONE = 0,
  PFB_QUANTISER_FUSED = 1,
  PFB_QUANTISER_STAGED = 2
} pfb_quantiser;
pfb_status pfb_analysis_execute_quantised_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in,
                                                  int64_t in_pol_stride, int64_t n_dat, double rms,
                                                  void* out, int32_t out_nbit, float out_scale,
                                                  int64_t out_capacity_bytes, int64_t* n_out,
                                                  double* scale, void* stream);
pfb_status pfb_filterbank_execute_quantised_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in,
                                                    int64_t in_pol_stride, int64_t n_in, double rms,
                                                    void* out, int32_t out_nbit, float out_scale,
                                                    int64_t out_capacity_bytes, int64_t* n_out,
                                                    double* scale, void* stream);
pfb_status pfb_analysis_execute_dada_quantised_to_dada(pfb_analysis_plan* plan, const void* in,
                                                       int32_t nbit, int32_t ndim, int32_t order,
                                                       int64_t n_dat, double rms, void* out,
                                                       int32_t out_nbit, float out_scale,
                                                       int64_t out_capacity_bytes, int64_t* n_out,
                                                       double* scale, void* stream);
pfb_status pfb_filterbank_execute_dada_quantised_to_dada(pfb_analysis_plan* plan, const void* in,
                                                         int32_t nbit, int32_t ndim, int32_t order,
                                                         int64_t n_in, double rms, void* out,
                                                         int32_t out_nbit, float out_scale,
                                                         int64_t out_capacity_bytes, int64_t* n_out,
                                                         double* scale, void* stream);
pfb_status pfb_analysis_set_quantiser_moments(pfb_analysis_plan* plan, int32_t mode);
int32_t pfb_analysis_last_quantiser(const pfb_analysis_plan* plan);

/* The FilterBank's quantised input (FilterBank.m:75-83: scale = rmsInput / sqrt(var(input, 0,
 * "all")), input = round(scale * input), before the carried samples are put in front): a property
 * of the analysis plan, off by default.  pfb_analysis_set_input_quantiser(plan, enable, rms)
 * turns it on (enable != 0) or off; with it on, every execute entry below replaces its own new
 * samples x — the n_dat or n_in samples of every polarisation, cnt = samples * n_pol; for a DADA
 * section the exactly cast integers or floats — by
 *   q = roundf((float)scale * x)   per component (pfb_quantize's operation: half away from zero)
 * before anything else sees them, with
 *   scale = rms / sqrt(var),  var = (sum |x|^2 - ((sum re)^2 + (sum im)^2) / cnt) / (cnt - 1)
 * summed in double.  rms <= 0: round only (the scale is 1, no moments are taken).  Carried
 * samples are not rounded again — they were rounded in the call that brought them — and do not
 * enter the variance, nor do the LowCBF pre-padding zeros.  The carry a call leaves holds rounded
 * values at that call's scale, also when the call completes no row.  rms > 0 with cnt < 2 (one
 * sample): PFB_ERR_INVALID_ARG, as in pfb_quantize; a call with no samples takes scale 1.  A
 * non-finite rms or a null plan: PFB_ERR_INVALID_ARG.  A zero variance is not special-cased and
 * is not compared with anything.  The setters may be called at any time, also with samples
 * buffered; they take effect at the next call and touch no device state.
 * Result: everything else about the call is that of the same call on q with the quantiser off,
 * bit for bit — outputs, *n_out, status codes, pfb_filterbank_buffered, the carry,
 * pfb_analysis_last_dada_output, pfb_analysis_last_quantiser and the LowCBF pending pre-padding;
 * pfb_analysis_last_dada_input reports how the section's bytes were read (STAGED when the
 * quantising copy unpacked them).  Every check still runs before any launch or state change.
 * Entries: pfb_analysis_execute, pfb_filterbank_execute (device and host memory),
 * pfb_filterbank_execute_strided, the _dada, _to_dada and _dada_to_dada calls and the four
 * _quantised_to_dada calls.  pfb_roundtrip_execute* with such a plan: PFB_ERR_UNSUPPORTED,
 * nothing launched.
 * FUSED: a plan on the streaming kernel whose call reads its new samples in place (cf32 device
 * memory, or a section pfb_analysis_execute_dada fuses) and whose product goes out as cf32 or
 * through the moments kernel of the quantised output: one pass over the new samples for
 * per-workgroup partial sums (ordinary stores), one workgroup that adds them in a fixed order and
 * forms the scale, then the analysis launch, which rounds each sample as it loads it.
 * STAGED: everything else — padded plans, the one-launch N <= 256 kernel, FIR + row FFT, host
 * memory, strided and plain _to_dada launches, a stream call that concatenates its carry, a
 * section the kernel does not read in place, and mode STAGED: the same two moments launches,
 * then a quantising copy of the new samples into a buffer of the plan (behind the carry in the
 * concatenation buffer where the call concatenates), and the plan's ordinary path on it.
 * pfb_analysis_set_input_quantiser_mode (pfb_quantiser_moments: AUTO, the default, takes FUSED
 * where the call allows it; FUSED on a call that cannot take it: PFB_ERR_UNSUPPORTED from that
 * call, nothing launched; STAGED).  pfb_analysis_last_input_quantiser: the path of the plan's
 * last call, NONE with the quantiser off or before any call, -1 for a null plan.
 * pfb_analysis_last_input_scale copies the last call's scale back on the given stream and
 * synchronises it (1 for a round-only call or one without samples) — the only thing here that
 * waits for the device.
 * The partial sums and the 32-byte block {sum re, sum im, sum |x|^2, scale} belong to the plan,
 * apart from the output quantiser's (both can be live in one call); they grow only with the
 * call's length, nothing is per device or per stream.  The setters and a call can be captured
 * into a graph after one call of that length.  No floating-point atomics: the same plan, input
 * and grid give the same scale bits and the same bytes.  (Measured: DESIGN.md §4.12.) */
typedef enum pfb_input_quantiser {
  PFB_INPUT_QUANTISER_NONE = 0,
  PFB_INPUT_QUANTISER_FUSED = 1,
  PFB_INPUT_QUANTISER_STAGED = 2
} pfb_input_quantiser;
pfb_status pfb_analysis_set_input_quantiser(pfb_analysis_plan* plan, int32_t enable, double rms);
pfb_status pfb_analysis_set_input_quantiser_mode(pfb_analysis_plan* plan, int32_t mode);
int32_t pfb_analysis_last_input_quantiser(const pfb_analysis_plan* plan);
pfb_status pfb_analysis_last_input_scale(pfb_analysis_plan* plan, double* scale, void* stream);

/* Synthesis writing its output straight into a DADA data section (polyphase_synthesis /
 * InverseFilterBank.m:92-96 followed by write_dada_data.m:32-50): the single-channel TFP
 * section, NDIM 2, out_nbit 8 / 16 (integers), 32 (float) or 64 (double).  Device memory only.
 * Output sample t of polarisation p, with P the plan's n_pol, lies at byte
 * (t * P + p) * 2 * out_nbit / 8 of `out`, re then im — the layout pfb_analysis_execute_dada
 * reads, so a synthesised section can be fed back to the analysis.  The bytes written, *n_out,
 * the status codes, pfb_inverse_filterbank_buffered, the sample-offset behaviour and the stream
 * state are those of the corresponding cf32-output call (pfb_synthesis_execute,
 * pfb_inverse_filterbank_execute and their _dada twins) into a packed [pol][t] buffer, both
 * components multiplied by out_scale in float32, followed by pfb_dada_pack at out_nbit with
 * n_chan = 1, bit for bit.  Exactly samples [0, *n_out) of the section are written and not one
 * byte beyond.  Every check runs before any launch or state change: a rejected stream call
 * leaves the carry and the buffered count untouched.  PFB_ERR_INVALID_ARG: a null plan, null
 * buffers when rows are given or output is due, out_nbit not 8/16/32/64, a non-finite
 * out_scale, `out` not aligned to one value of out_nbit, and the input-side conditions of the
 * corresponding call.  PFB_ERR_BUFFER_TOO_SMALL, with nothing written: out_capacity_bytes below
 * n_out * P * 2 * out_nbit / 8.  Every kind of stream call may alternate on one plan: cf32,
 * DADA or strided input, cf32 or DADA output.
 * FUSED: the Nf = 256 wave kernel converts and stores the samples itself, one range-checked
 * buffer store of 2 / 4 / 8 bytes per complex sample, and the cf32 series never crosses HBM —
 * out_nbit 8, 16 or 32, `out` aligned to one complex sample, and a plan on that kernel
 * (input_fft_length 256, input_overlap 48, os 8/7 or 4/3, n_chan a multiple of 16, no spectral
 * taper).  Descriptor limit: one block's L = 256 * de / nu * n_chan output samples must fit
 * 32-bit offsets, L * n_pol * (out_nbit / 4) <= 0x7ffffff0 (n_chan 256, 8/7: n_pol <= 4681 at
 * NBIT 32, 18724 at NBIT 8); more polarisations are STAGED.  The input side is the channel
 * IFFT's own launch, so the _dada_to_dada calls read
 * their section as pfb_synthesis_execute_dada does (pfb_synthesis_last_dada_input reports it)
 * whatever the output takes.
 * STAGED: every other plan (input_fft_length 512, the block-kernel shapes, spectral tapers),
 * out_nbit 64 and an `out` aligned to a value but not to a complex sample run the cf32 path
 * into a plan-owned buffer, then one scaled pack launch; so these calls accept every plan the
 * cf32 calls accept.  Chunked synthesis (pfb_synthesis_set_chunk_blocks) works in both.
 * pfb_synthesis_last_dada_output (enum pfb_dada_output): which of the two the plan's last such
 * call took, NONE before one or after a cf32-output call, -1 for a null plan.  (Measured A/B
 * against the pair: DESIGN.md §4.8.) */
pfb_status pfb_synthesis_execute_to_dada(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                         int64_t in_pol_stride, int64_t n_dat, int64_t sample_offset,
                                         void* out, int32_t out_nbit, float out_scale,
                                         int64_t out_capacity_bytes, int64_t* n_out, void* stream);
pfb_status pfb_inverse_filterbank_execute_to_dada(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                                  int64_t in_pol_stride, int64_t n_in, void* out,
                                                  int32_t out_nbit, float out_scale,
                                                  int64_t out_capacity_bytes, int64_t* n_out, void* stream);
pfb_status pfb_synthesis_execute_dada_to_dada(pfb_synthesis_plan* plan, const void* in, int32_t nbit,
                                              int32_t ndim, int32_t order, int64_t n_dat,
                                              int64_t sample_offset, void* out, int32_t out_nbit,
                                              float out_scale, int64_t out_capacity_bytes, int64_t* n_out,
                                              void* stream);
pfb_status pfb_inverse_filterbank_execute_dada_to_dada(pfb_synthesis_plan* plan, const void* in,
                                                       int32_t nbit, int32_t ndim, int32_t order,
                                                       int64_t n_in, void* out, int32_t out_nbit,
                                                       float out_scale, int64_t out_capacity_bytes,
                                                       int64_t* n_out, void* stream);
int32_t pfb_synthesis_last_dada_output(const pfb_synthesis_plan* plan);

/* The round trip from file bytes to file bytes (DADARead.m:58-83, then the analysis ->
 * synthesis sequence of test_data_pipeline.m:114,132, each step followed by
 * write_dada_data.m:32-50): pfb_roundtrip_execute and its two halves with a single-channel DADA
 * section in, the channelised file's section and the output file's section out.  Device memory
 * only.  `in` is the section pfb_analysis_execute_dada reads: n_dat samples x 1 channel x the
 * plans' n_pol x ndim values of nbit (8/16/32/64), in `order`; in TFP order complex sample t of
 * polarisation p is element t * n_pol + p.  `chan` is the channelised section as the pipeline
 * saves it: TFP, NDIM 2, NBIT 32 float, no scale — element (row k, channel c, polarisation p),
 * with N the channel count and P = n_pol, at byte ((k * N + c) * P + p) * 8, re then im; for
 * one polarisation these are the bytes of pfb_roundtrip_execute's cf32 `chan`.  It is float on
 * purpose: the reference's synthesis reads the channelised file, and the stage-1 rows are taken
 * before the store, so only an unquantised product makes the fused call compute what the
 * two-file pipeline computes.  `out` is the section pfb_synthesis_execute_to_dada writes:
 * sample t of polarisation p at byte (t * P + p) * 2 * out_nbit / 8, out_nbit 8/16/32/64, each
 * component to_sample(out_scale * y).
 * The bytes written, *n_chan_rows, *n_out and the status codes are those of this sequence, bit
 * for bit, on every path: pfb_dada_unpack of `in` into a packed [pol][t] buffer;
 * pfb_roundtrip_execute on it; pfb_dada_pack(..., 32) of its `chan`; both components of its
 * `out` multiplied by out_scale in float32; pfb_dada_pack at out_nbit with n_chan = 1.  Exactly
 * rows [0, *n_chan_rows) of `chan` and samples [0, *n_out) of `out` are written and not one
 * byte beyond.  pfb_roundtrip_analysis_execute_dada and pfb_roundtrip_synthesis_execute_to_dada
 * are the two halves (see pfb_roundtrip_analysis_execute): together they equal the whole call
 * bit for bit, and the synthesis half works after either analysis half, cf32 or DADA — the
 * stage-1 rows and the plan's key are the same; it is refused with PFB_ERR_INVALID_ARG exactly
 * where pfb_roundtrip_synthesis_execute is.  PFB_ERR_UNSUPPORTED as for the cf32 calls: a
 * PFB_ANALYSIS_LOWCBF plan, and the halves on a plan pair that takes the chunked pipeline.
 * Every check runs before any launch or state change.  PFB_ERR_INVALID_ARG: null plans, null
 * buffers when samples are given or output is due, nbit or out_nbit not 8/16/32/64, ndim not
 * 1/2, an unknown order (LowCBF: n_dat a multiple of 32), `in` not aligned to one value of
 * nbit, `chan` not 4-byte aligned, `out` not aligned to one value of out_nbit, a non-finite
 * out_scale, sample_offset < 1, and the plan-mismatch conditions of pfb_roundtrip_execute.
 * PFB_ERR_BUFFER_TOO_SMALL, with nothing written and *n_chan_rows and *n_out set as the cf32
 * call sets them: chan_capacity_bytes below K * N * P * 8, out_capacity_bytes below
 * n_out * P * 2 * out_nbit / 8.
 * FUSED: one analysis launch (analysis_stream_rt_dada_kernel) loads the section's bytes, stores
 * the float product section and emits the stage-1 rows; the Nf = 256 wave synthesis then stores
 * the output section.  No unpacked series, no cf32 series and no pack launch exist.  All of:
 * nbit 8, 16 or 32, NDIM 2, TFP order, `in` aligned to one complex sample; `chan` aligned to 8
 * bytes; out_nbit 8, 16 or 32 and `out` aligned to one complex sample; a plan pair whose cf32
 * round trip takes the fused path through the streaming analysis and the wave kernel on 2-row
 * runs (PFB_ANALYSIS_BUNTON, n_chan 256, os 8/7 or 4/3, 12 or 13 tap phases; input_fft_length
 * 256, input_overlap 48; no combine permutation, temporal-taper gain or spectral taper; no
 * chunk size set; (sample_offset - 1) a multiple of 16); sections within the descriptor limits
 * of pfb_analysis_execute_dada (P * (nbit / 4) * N * 512 <= 0x7ffffff0, N and P as above) and
 * pfb_analysis_execute_to_dada (16 * C * P * (out_nbit / 4) <= 0x7ffffff0, here with C = N and
 * out_nbit = 32, the float `chan` section).  A half needs its own side's
 * conditions only.  The stage-1 rows are STORED in these calls whatever
 * pfb_synthesis_set_stage1_rows says (no recomputing kernel reads a section);
 * pfb_synthesis_last_stage1_rows reports it.
 * STAGED: everything else (padded or n_chan > 256 pairs, other offsets, NBIT 64, NDIM 1, LowCBF
 * order, a `chan` or `out` aligned to a value only, a call too short for one synthesis block)
 * runs the sequence above inside the call on plan-owned staging buffers, so these calls accept
 * every plan pair pfb_roundtrip_execute accepts, the chunked pipeline included; with one
 * polarisation and an 8-byte aligned `chan` the cf32 round trip writes straight into `chan`.
 * pfb_analysis_last_dada_input reports the path of the input, pfb_analysis_last_dada_output
 * that of the product section and pfb_synthesis_last_dada_output that of the output section
 * (unchanged by a call without rows); FUSED is all three FUSED.  (Measured A/B against the
 * sequence: DESIGN.md §4.9.) */
pfb_status pfb_roundtrip_execute_dada_to_dada(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                              const void* in, int32_t nbit, int32_t ndim, int32_t order,
                                              int64_t n_dat, void* chan, int64_t chan_capacity_bytes,
                                              int64_t* n_chan_rows, int64_t sample_offset, void* out,
                                              int32_t out_nbit, float out_scale, int64_t out_capacity_bytes,
                                              int64_t* n_out, void* stream);
pfb_status pfb_roundtrip_analysis_execute_dada(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                               const void* in, int32_t nbit, int32_t ndim, int32_t order,
                                               int64_t n_dat, void* chan, int64_t chan_capacity_bytes,
                                               int64_t* n_chan_rows, int64_t sample_offset, void* stream);
pfb_status pfb_roundtrip_synthesis_execute_to_dada(pfb_analysis_plan* analysis, pfb_synthesis_plan* synthesis,
                                                   int64_t n_dat, int64_t sample_offset, void* out,
                                                   int32_t out_nbit, float out_scale,
                                                   int64_t out_capacity_bytes, int64_t* n_out, void* stream);

/* The synthesis calls reading their channelised rows strided (device memory only): channel c
 * of row t of polarisation p is in[p * in_pol_stride + t * in_row_stride + c * in_chan_stride]
 * — the input-side mirror of pfb_filterbank_execute_strided.  Polarisations may interleave
 * inside a row: the per-coarse-channel slices of TwoStageInverseFilterBank.m:124-126 are
 * in_pol_stride = nch_in, in_row_stride = nchan, in_chan_stride = 1 over the assembled
 * two-stage product, with no gather.  Rows may be channel-major (in_row_stride = 1,
 * in_chan_stride = series length), or a channel window of a wider product.  The input is only
 * read, so polarisations may overlap.
 * The output, *n_out, the status codes, pfb_inverse_filterbank_buffered and the stream state
 * are those of pfb_synthesis_execute / pfb_inverse_filterbank_execute on a packed
 * [pol][t][chan] copy of the same elements, bit for bit: the channel IFFT sees the same
 * values in the same butterflies.  No element outside the mapped ones is loaded.
 * Checks, all before any launch or change of the stream state (a rejected stream call leaves
 * the carry and the buffered count untouched): a stride <= 0, or in_capacity (the pfb_cf32
 * elements available from `in`) not beyond the furthest element read, (n_pol-1) in_pol_stride
 * + (rows-1) in_row_stride + (n_chan-1) in_chan_stride, is PFB_ERR_INVALID_ARG, as are the
 * null, sample_offset and output-stride conditions of the packed calls; an output capacity
 * below the output length is PFB_ERR_BUFFER_TOO_SMALL.
 * IN_PLACE: the channel IFFT's first pass loads through the layout (64-bit addresses, plain
 * loads) and the packed copy never exists — every channel count below 4096, with or without
 * the combine permutation, of a plan without temporal-taper gain or spectral taper.  A
 * stream call reads the blocks made of new rows only in place; the blocks that start in the
 * carry are stitched from the packed cf32 carry and the head of the new rows, and the new
 * carry is their tail, both copied out of the layout.  STAGED: any other plan (4096
 * channels, a Hann temporal taper, a spectral taper) has the rows copied through the layout
 * into a plan-owned packed buffer by one launch and runs the packed path, so these calls
 * accept every plan the packed ones accept.  pfb_synthesis_last_strided_input: which of the
 * two the plan's last strided call took (IN_PLACE when any of its channel IFFTs read through
 * the layout), NONE before one or after a packed or DADA call, -1 for a null plan. */
typedef enum pfb_strided_input {
  PFB_STRIDED_INPUT_NONE = 0,
  PFB_STRIDED_INPUT_IN_PLACE = 1,
  PFB_STRIDED_INPUT_STAGED = 2
} pfb_strided_input;
pfb_status pfb_synthesis_execute_strided(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                         int64_t in_pol_stride, int64_t in_row_stride,
                                         int64_t in_chan_stride, int64_t in_capacity, int64_t n_dat,
                                         int64_t sample_offset, pfb_cf32* out, int64_t out_pol_stride,
                                         int64_t out_capacity, int64_t* n_out, void* stream);
pfb_status pfb_inverse_filterbank_execute_strided(pfb_synthesis_plan* plan, const pfb_cf32* in,
                                                  int64_t in_pol_stride, int64_t in_row_stride,
                                                  int64_t in_chan_stride, int64_t in_capacity,
                                                  int64_t n_in, pfb_cf32* out, int64_t out_pol_stride,
                                                  int64_t out_capacity, int64_t* n_out, void* stream);
int32_t pfb_synthesis_last_strided_input(const pfb_synthesis_plan* plan);

/* [pol][t][chan] complex float32 -> DADA TFP data section (NDIM 2) of NBIT 8/16/32/64;
 * integer types follow Matlab's cast (round half away from zero, saturate).  Replaces
 * write_dada_data.m:32-50 (data written with the class write_dada_header.m:13-22
 * records as NBIT). */
pfb_status pfb_dada_pack(const pfb_cf32* in, int64_t in_pol_stride, int64_t n_dat, int32_t n_chan,
                         int32_t n_pol, void* out, int32_t nbit, void* stream);

/* Channel gather: out[o][t][j] = in[o][t][src0 + j + (j >= split ? shift : 0)] for
 * o < n_outer (<= 65535), t < n_rows, j < n_sel (strides in complex samples).
 * Replaces the stage-2 output assembly of TwoStageFilterBank.m:102-105 (shift = the
 * oversampled channels dropped in the middle) and the per-coarse-channel input slices
 * of TwoStageInverseFilterBank.m:124-126.  Device memory, asynchronous. */
pfb_status pfb_gather_channels(const pfb_cf32* in, int64_t in_outer_stride, int64_t in_row_stride,
                               pfb_cf32* out, int64_t out_outer_stride, int64_t out_row_stride,
                               int64_t n_outer, int64_t n_rows, int32_t n_sel, int32_t src0,
                               int32_t split, int32_t shift, void* stream);

/* Corner turn: out[o][c][r] = in[o][r][c] (r < n_rows, c < n_cols, o < n_outer).
 * Replaces the out1(1,ich,:) channel slices TwoStageFilterBank.m:94 feeds to stage 2
 * (channelised [t][chan] -> per-channel series).  Device memory, asynchronous. */
pfb_status pfb_corner_turn(const pfb_cf32* in, int64_t in_outer_stride, int64_t in_row_stride,
                           int64_t n_outer, int64_t n_rows, int64_t n_cols, pfb_cf32* out,
                           int64_t out_outer_stride, int64_t out_row_stride, void* stream);

/* Quantisation hook: out = round(single(scale) * in) with scale = rms / sqrt(var(in, 0,
 * "all")) over all n_pol x n samples, or 1 when rms <= 0 (Matlab round: half away from
 * zero).  Replaces FilterBank.m:75-83 (rndInput/rmsInput) and :106-113
 * (rndOutput/rmsOutput).  in == out is allowed.  Device memory; asynchronous unless
 * `scale` is non-null (then it receives the scale and the call synchronises).  The moments
 * are summed in a 32-byte block that belongs to the (device, stream) of the call: the first
 * call on a stream allocates it (make that call before capturing the stream into a graph),
 * none after it allocates, and calls on different streams share nothing.  A call captured
 * into a graph keeps the block of the stream it was captured on wherever the graph is
 * replayed: order such a graph's replays against the other calls made on that stream, as
 * calls on one stream are ordered. */
pfb_status pfb_quantize(const pfb_cf32* in, int64_t in_pol_stride, int64_t n, int32_t n_pol,
                        double rms, pfb_cf32* out, int64_t out_pol_stride, double* scale,
                        void* stream);

/* ---------------------------------------------------------------- verification */
/* The reference's verification loop (current_performance.m) on the device: per test vector
 * generate -> round trip -> score, with nothing but a few doubles per vector crossing to the
 * host.  Device pointers, strides in complex elements, n_vec <= 65535; every argument check
 * runs before any device call: n <= 0, n_vec <= 0, a stride below n, a null buffer, a series
 * not aligned to 8 bytes, domain < 0, an unknown kind or dtype and a non-finite scale or
 * parameter are PFB_ERR_INVALID_ARG.  The scores accumulate in double and are deterministic
 * (per-workgroup partials combined in a fixed order: the same data give the same bits).  They
 * use the current device's scratch, so the caller makes the series' device current. */
typedef enum pfb_testvec_kind { PFB_TESTVEC_IMPULSE = 0, PFB_TESTVEC_SINUSOID = 1 } pfb_testvec_kind;

/* out[v*out_stride + t], t < n, for v < n_vec.  kind[v], param[4*v .. 4*v+3] are HOST arrays.
 * IMPULSE  (time_domain_impulse.m:13-24): param = {offset (1-based), width, -, -}: ones at
 *          offset-1 .. offset-2+width clipped to [0, n), zeros elsewhere.
 * SINUSOID (complex_sinusoid.m:16-31):   param = {frequency, phase, bin_offset, -}:
 *          ph = ((2*pi*(frequency+bin_offset))/n)*t + phase evaluated in double in exactly this
 *          order, out = (float)cos(ph), (float)sin(ph).
 * Asynchronous on stream.  Writes nothing outside [0, n) of each row. */
pfb_status pfb_testvec_generate(const int32_t* kind, const double* param, int32_t n_vec, int64_t n,
                                pfb_cf32* out, int64_t out_stride, void* stream);

/* ErrorAnalysis.m:5-52 + DomainPerformance.m:67-100 + TestImpulse.m:46-73 on n_vec series.
 * p[t] = scale * (re^2 + im^2) in double; dtype 0 = complex float32, 1 = complex float64.
 * result (HOST, n_vec x 6 doubles):
 *  [0] k = first index of max p   [1] p[k]
 *  [2] max and [3] sum of p with indices max(k-domain,0) .. min(k+domain,n-1) zeroed
 *      (the unmasked terms summed directly, not a total minus the window)
 *  [4] p[e] and [5] max of p outside max(e-1,0) .. e+1, where e = expected[v];
 *      both -1 when expected is null, e < 0 or e >= n.
 * expected: HOST array or null.  Synchronises the stream. */
pfb_status pfb_purity_score_spurious(const void* a, int32_t dtype, int64_t stride, int64_t n,
                                     int32_t n_vec, double scale, int32_t domain,
                                     const int64_t* expected, double* result, void* stream);

/* DomainPerformance.m:7-64 (correct_phase 0): d[t] = |a[t]-b[t]|^2 in double;
 * result (HOST, n_vec x 2): max d, sum d.  Synchronises the stream. */
pfb_status pfb_purity_score_difference(const pfb_cf32* a, int64_t a_stride, const pfb_cf32* b,
                                       int64_t b_stride, int64_t n, int32_t n_vec, double* result,
                                       void* stream);

/* ---------------------------------------------------------------- utilities */
const char* pfb_last_error(void);
int32_t pfb_api_version(void);
int32_t pfb_device_count(void);
/* Device memory helpers for callers without their own allocator (ctypes harness). */
pfb_status pfb_device_malloc(int32_t device, int64_t bytes, void** ptr);
pfb_status pfb_device_free(void* ptr);
pfb_status pfb_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream);
pfb_status pfb_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream);
pfb_status pfb_stream_synchronize(void* stream);
/* Bandwidth probe (no reference counterpart; SURVEY §8(d) asks for the achievable
 * copy rate beside the HBM spec): device-to-device float4 copy kernel.  16-B aligned
 * pointers, n_bytes a multiple of 64.  Asynchronous on `stream`. */
pfb_status pfb_device_copy(void* dst, const void* src, int64_t n_bytes, void* stream);

/* Kernel timing: average duration (ms) of the named kernel class over the launches
 * recorded since the last reset, measured with HIP events on the plan's stream.
 * which: 0 = analysis, 1 = synthesis channel-IFFT, 2 = synthesis block kernel,
 *        3 = analysis fused with the synthesis channel IFFT (pfb_roundtrip_execute),
 *        4 / 5 = the FIR / the row FFT of the n_chan > 256 round trip (SKA-Mid), each
 *        launch timed alone; bytes: what each reads + writes once. */
pfb_status pfb_profile_enable(int32_t enable);
pfb_status pfb_profile_read(int32_t which, double* total_ms, int64_t* launches, double* bytes);
pfb_status pfb_profile_reset(void);
/* Name of the kernel whose launches class `which` recorded (the last one, demangled as a
 * kernel trace prints it, e.g. "void pfb::synth_block_kernel<256, 224, ...>(pfb::
 * SynthBlockArgs)"); "" when the class recorded no single-kernel launch.  Writes at most
 * `len` bytes including the terminating NUL. */
pfb_status pfb_profile_kernel_name(int32_t which, char* buf, int64_t len);

/* Build flags of the loaded library: bit 0 = experiments build (A/B knobs and timing
 * masks read from PFB_* environment variables; never a release or benchmark library). */
int32_t pfb_build_flags(void);

#ifdef __cplusplus
}
#endif

#endif /* PFB_API_H */
