// pfb_api_core.hip — the part of the C ABI (include/pfb_api.h) that belongs to no plan: the
// error channel, version and device queries, the profiler, device memory and copies, and what
// pfb_host.hpp declares for the other host units.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>

#include "pfb_host.hpp"

using namespace pfb::host;

namespace {
thread_local std::string g_err;
Profiler g_prof;
thread_local pfb::LaunchEvents g_armed;
thread_local const char* g_launched = nullptr;
}  // namespace

pfb_status pfb::host::fail(pfb_status s, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return s;
}

pfb_status pfb_set_error(pfb_status s, const char* msg) { return fail(s, "%s", msg); }

std::vector<float2> pfb::host::twiddles(int64_t n, int sign) {
  std::vector<float2> t((size_t)n);
  for (int64_t m = 0; m < n; ++m) {
    int64_t mm = m;
    if (2 * mm > n) mm -= n;
    const double a = 2.0 * M_PI * (double)mm / (double)n;
    t[(size_t)m] = make_float2((float)std::cos(a), (float)(sign * std::sin(a)));
  }
  return t;
}

Profiler& pfb::host::profiler() { return g_prof; }
pfb::LaunchEvents& pfb::armed_launch_events() { return g_armed; }
const char*& pfb::launched_kernel_name() { return g_launched; }

void pfb::host::Profiler::drain() {
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

std::string pfb::host::demangle(const char* name) {
  if (!name) return std::string();
  int st = 0;
  char* d = abi::__cxa_demangle(name, nullptr, nullptr, &st);
  std::string out = (st == 0 && d) ? std::string(d) : std::string(name);
  std::free(d);
  return out;
}

hipError_t pfb::host::copy_pols(float2* dst, int64_t dps, const float2* src, int64_t sps, int64_t n, int n_pol,
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

pfb_status pfb::host::section_check(const void* plan, const DadaSection& sec, int64_t n) {
  if (!plan) return fail(PFB_ERR_INVALID_ARG, "null plan");
  if (sec.nbit != 8 && sec.nbit != 16 && sec.nbit != 32 && sec.nbit != 64)
    return fail(PFB_ERR_INVALID_ARG, "NBIT must be 8, 16, 32 or 64");
  if (sec.ndim != 1 && sec.ndim != 2) return fail(PFB_ERR_INVALID_ARG, "NDIM must be 1 or 2");
  if (sec.order != PFB_DADA_TFP && sec.order != PFB_DADA_LOWCBF)
    return fail(PFB_ERR_INVALID_ARG, "unknown sample order");
  if (sec.order == PFB_DADA_LOWCBF && n > 0 && n % 32)
    return fail(PFB_ERR_INVALID_ARG, "LowCBF data are heaps of 32 samples");
  return PFB_OK;
}

extern "C" {

const char* pfb_last_error(void) { return g_err.c_str(); }
int32_t pfb_api_version(void) { return PFB_API_VERSION; }

int32_t pfb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
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
