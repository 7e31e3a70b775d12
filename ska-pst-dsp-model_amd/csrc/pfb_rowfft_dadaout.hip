// pfb_rowfft_dadaout.hip — the 4096-point pair row FFT storing its product as a DADA data
// section (row_fft4096_pair_dadaout_kernel; pfb_analysis_execute_to_dada and its twins on a
// 4096-channel plan).  Forward and inverse x NBIT 8 / 16 / 32 out: 6 kernels, in a translation
// unit of their own so that they compile beside pfb_rowfft.hip.
#include "pfb_dada_store.hpp"
#include "pfb_rowfft4k.hpp"

namespace pfb {

// Bin c of polarisations 0 and 1 of a two-polarisation DADA section as ONE store of 2 OUT::kBytes
// bytes (4 / 8 / 16): (re0, im0, re1, im1), each converted by to_sample as OUT::store does.
template <class OUT, int AUX>
__device__ __forceinline__ void r4k_dada_store2(__amdgpu_buffer_rsrc_t rs, uint32_t off, int soff, float2 x0,
                                                float2 x1) {
  if constexpr (OUT::kBytes == 8) {
    // (the four floats made opaque before they form one vector: as the root of a 4-wide SLP
    // tree the store had the last pass of the two rows' FFTs vectorised ACROSS the rows, with
    // other multiply-add contractions than the cf32 kernels' (re, im) pairs, and the section was
    // not the pair's bit for bit)
    float a = to_sample<float>(x0.x), b = to_sample<float>(x0.y), c = to_sample<float>(x1.x),
          d = to_sample<float>(x1.y);
    asm("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    const v4f w{a, b, c, d};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, w), rs, off, soff, AUX);
  } else if constexpr (OUT::kBytes == 4) {
    auto w = [](float2 x) {
      return (uint32_t)(uint16_t)to_sample<int16_t>(x.x) | ((uint32_t)(uint16_t)to_sample<int16_t>(x.y) << 16);
    };
    __builtin_amdgcn_raw_buffer_store_b64(v2u{w(x0), w(x1)}, rs, off, soff, AUX);
  } else {
    auto b = [](float c) { return (uint32_t)(uint8_t)to_sample<int8_t>(c); };
    __builtin_amdgcn_raw_buffer_store_b32(b(x0.x) | (b(x0.y) << 8) | (b(x1.x) << 16) | (b(x1.y) << 24), rs, off,
                                          soff, AUX);
  }
}

// The pair kernel storing the product as a DADA section itself (RowFftArgs::dout; OUT: OutDada8 /
// 16 / 32, pfb_dada_store.hpp — pfb_analysis_execute_to_dada on a 4096-channel plan): no cf32
// product in HBM and no pack pass.  Input as in the strided kernel: the plan's cf32 scratch
// [pol][row][4096], each row through its own one-row descriptor (lane offset tid * 8, the
// register's r * 2048 as the scalar offset), output row t from the FIR row (t + sds) mod K
// (remap: the padded variant) or from row t (Bunton); only rows t < out_keep are made.  Each
// component is to_sample(dout_scale * x), x the cscale(v, scale) of the cf32 store: the float32
// products of that store, the caller's scale and pfb_dada_pack, in that order.  Same passes and
// tables as the other 4096-point kernels: the values before the conversion are bit-identical.
// What the workgroup's two rows are (uniform, n_pol is a kernel argument):
//  n_pol == 2: output row t = blockIdx.x of polarisations 0 and 1 (grid: out_keep workgroups in
//    the dispatcher's order, which is the rows' order).  Bin c of both goes out as one 4 / 8 / 16-B
//    store at byte c * 2 * esz of row t: the workgroup writes whole lines (stored like the cf32
//    rows, kNtRow).
//  else: output rows 2g and 2g + 1 of polarisation blockIdx.y, g = xcd_tile(blockIdx.x) (grid:
//    (ceil(out_keep / 2), n_pol)); one sample per store at stride n_pol * esz (n_pol == 1: whole
//    lines, kNtRow; else the lines are shared between workgroups: kAuxDadaOut).  The last pair of
//    an odd out_keep has no row B: its loads re-read row A, it is not transformed, and its stores
//    are dropped by the range check (a descriptor of 0 bytes and the lane offset past every
//    extent; the register's displacement alone rides in the scalar offset, which the check does
//    not cover and which stays inside the row).
// One descriptor per output row (base row t of the section, 4096 * n_pol * esz bytes; at most
// 0x7fff8000), built from read-first-lane values; no store sits under a lane-dependent branch.
template <int DIR, class OUT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void row_fft4096_pair_dadaout_kernel(
    RowFftArgs a) {
  constexpr int N = 4096;
  constexpr uint32_t ESZ = OUT::kBytes;
  constexpr int kAuxLine = kNtRow ? 2 : 0;
  extern __shared__ __attribute__((aligned(16))) float2 smem[];
  const bool dual = a.n_pol == 2;
  int64_t ta, tb;
  int pa, pb;
  if (dual) {
    ta = tb = blockIdx.x;
    pa = 0;
    pb = 1;
  } else {
    ta = 2 * (int64_t)xcd_tile(blockIdx.x, gridDim.x);
    tb = ta + 1;
    pa = pb = blockIdx.y;
  }
  if (ta >= a.out_keep) return;  // uniform per workgroup
  const bool has_b = tb < a.out_keep;
  const int tid = threadIdx.x;
  float2* row = smem;
  float2* t2 = smem + kR4kRow;
  float2* t3 = t2 + kR4kTw2;
  for (int e = tid; e < kR4kTw3; e += NT) {
    const int pp = e >> 8, k = e & 255;
    t3[e] = a.tw[(k << pp) & (N - 1)];
    if (e < kR4kTw2) t2[e] = a.tw[((e & 15) << ((e >> 4) + 4)) & (N - 1)];
  }
  // FIR row of output row t: (t + sds) mod K; t < out_keep <= K and sh < K: one wrap
  const int64_t sh = a.remap ? a.sds % a.n_total : 0;
  int64_t ra = ta + sh, rb = (has_b ? tb : ta) + sh;
  if (ra >= a.n_total) ra -= a.n_total;
  if (rb >= a.n_total) rb -= a.n_total;
  const __amdgpu_buffer_rsrc_t rsa = make_rsrc_u(a.in + pa * a.in_pol_stride + ra * N, (uint32_t)(N * 8));
  const __amdgpu_buffer_rsrc_t rsb = make_rsrc_u(a.in + pb * a.in_pol_stride + rb * N, (uint32_t)(N * 8));
  const uint32_t lane_off = (uint32_t)tid * 8u;
  float2 v[16], h[16];
  static_for<0, 16>([&](auto rv) {
    constexpr int r = decltype(rv)::value;
    v[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsa, lane_off, r * 2048, kNtlRow ? 2 : 0));
    h[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsb, lane_off, r * 2048, kNtlRow ? 2 : 0));
  });
  const float os = a.dout_scale;
  const int64_t row_bytes = (int64_t)N * a.n_pol * ESZ;
  char* sect = static_cast<char*>(a.dout);
  if (dual) {
    r4k_fft<DIR>(v, row, t2, t3, tid);
    r4k_fft<DIR>(h, row, t2, t3, tid);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc_u(sect + ta * row_bytes, (uint32_t)row_bytes);
    const uint32_t lane = (uint32_t)tid * 2u * ESZ;
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      const float2 x0 = cscale(v[r], a.scale), x1 = cscale(h[r], a.scale);
      r4k_dada_store2<OUT, kAuxLine>(rs, lane, r * 256 * 2 * (int)ESZ, make_float2(os * x0.x, os * x0.y),
                                     make_float2(os * x1.x, os * x1.y));
    });
    return;
  }
  // one polarisation's rows 2g and 2g + 1: bin c = tid + 256 r at byte (c P + p) esz of its row,
  // the lane's (tid P + p) esz and the register's 256 r P esz as the scalar offset (uniform)
  const uint32_t lane = ((uint32_t)tid * (uint32_t)a.n_pol + (uint32_t)pa) * ESZ;
  const uint32_t rstep = 256u * (uint32_t)a.n_pol * ESZ;
  auto put = [&](const float2 (&y)[16], __amdgpu_buffer_rsrc_t rs, uint32_t off, auto aux) {
    static_for<0, 16>([&](auto rv) {
      constexpr int r = decltype(rv)::value;
      const float2 x = cscale(y[r], a.scale);
      OUT::template store<decltype(aux)::value>(rs, off, os * x.x, os * x.y, (uint32_t)r * rstep);
    });
  };
  auto put_row = [&](const float2 (&y)[16], __amdgpu_buffer_rsrc_t rs, uint32_t off) {
    if (a.n_pol == 1) put(y, rs, off, std::integral_constant<int, kAuxLine>{});  // (uniform)
    else put(y, rs, off, std::integral_constant<int, kAuxDadaOut>{});
  };
  r4k_fft<DIR>(v, row, t2, t3, tid);
  put_row(v, make_rsrc_u(sect + ta * row_bytes, (uint32_t)row_bytes), lane);
  if (has_b) r4k_fft<DIR>(h, row, t2, t3, tid);  // (uniform)
  // (no row B: nothing of h may land — 0 bytes of extent at row A's base, every lane out of range)
  put_row(h, make_rsrc_u(sect + (has_b ? tb : ta) * row_bytes, has_b ? (uint32_t)row_bytes : 0u),
          has_b ? lane : 0xFFFFFFF0u);
}

template <int DIR>
hipError_t launch_row_fft4096_dadaout(const RowFftArgs& r, int n_pol, hipStream_t s) {
  void (*kern)(RowFftArgs) = nullptr;
  switch (r.dout_nbit) {
    case 8: kern = row_fft4096_pair_dadaout_kernel<DIR, OutDada8>; break;
    case 16: kern = row_fft4096_pair_dadaout_kernel<DIR, OutDada16>; break;
    case 32: kern = row_fft4096_pair_dadaout_kernel<DIR, OutDada32>; break;
    default: return hipErrorInvalidValue;
  }
  // one row of the section (all polarisations) lies within a descriptor
  if ((int64_t)4096 * n_pol * (r.dout_nbit / 4) > kRsrcMaxBytes) return hipErrorInvalidValue;
  hipError_t e = set_lds(kern, kR4kLds);
  if (e != hipSuccess) return e;
  const bool dual = n_pol == 2;
  const int64_t wgs = dual ? r.out_keep : (r.out_keep + 1) / 2;
  if (wgs > INT32_MAX) return hipErrorInvalidValue;
  return launch_kernel(kern, dim3((unsigned)wgs, dual ? 1u : (unsigned)n_pol), dim3(NT), kR4kLds, s, r);
}

template hipError_t launch_row_fft4096_dadaout<-1>(const RowFftArgs&, int, hipStream_t);
template hipError_t launch_row_fft4096_dadaout<+1>(const RowFftArgs&, int, hipStream_t);

}  // namespace pfb
