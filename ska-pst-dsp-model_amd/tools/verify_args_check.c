/* verify_args_check.c — the argument checks of the verification entry points
 * (pfb_testvec_generate, pfb_purity_score_spurious, pfb_purity_score_difference) under the
 * host sanitizers.  A stand-alone program: `make SANITIZE=1 check-verify-args` links it, built
 * with AddressSanitizer + UndefinedBehaviorSanitizer, against lib/libpfb_hip_san.so and runs
 * it.  Every call below must be refused with PFB_ERR_INVALID_ARG before any device call, so it
 * needs no GPU; a sanitizer report aborts it, a call that is not refused makes it exit 1. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pfb_api.h"

static int failures = 0;
static int calls = 0;

static void expect_bad(const char* what, pfb_status st) {
  const char* msg = pfb_last_error();
  ++calls;
  if (st != PFB_ERR_INVALID_ARG || !msg || strncmp(msg, "pfb_", 4) != 0) {
    fprintf(stderr, "FAIL %s: status %d, message '%s'\n", what, (int)st, msg ? msg : "(null)");
    ++failures;
  }
}

int main(void) {
  /* stand-ins for device buffers: aligned, non-null, never dereferenced by a refused call */
  static _Alignas(16) pfb_cf32 fake_a[4], fake_b[4];
  int32_t kind[2] = {PFB_TESTVEC_IMPULSE, PFB_TESTVEC_SINUSOID};
  int32_t kind_bad[2] = {PFB_TESTVEC_IMPULSE, 2};
  double param[8] = {5, 1, 0, 0, 3, 0.785398163397448, 0, 0};
  double param_nan[8] = {5, 1, 0, 0, NAN, 0.785398163397448, 0, 0};
  double param_inf[8] = {5, INFINITY, 0, 0, 3, 0.785398163397448, 0, 0};
  int64_t expected[2] = {1, 2};
  double result[12];
  pfb_cf32* odd = (pfb_cf32*)((char*)fake_a + 4);

  expect_bad("generate n = 0", pfb_testvec_generate(kind, param, 2, 0, fake_a, 16, NULL));
  expect_bad("generate n_vec = 0", pfb_testvec_generate(kind, param, 0, 16, fake_a, 16, NULL));
  expect_bad("generate n_vec > 65535", pfb_testvec_generate(kind, param, 65536, 16, fake_a, 16, NULL));
  expect_bad("generate stride < n", pfb_testvec_generate(kind, param, 2, 16, fake_a, 15, NULL));
  expect_bad("generate null kind", pfb_testvec_generate(NULL, param, 2, 16, fake_a, 16, NULL));
  expect_bad("generate null param", pfb_testvec_generate(kind, NULL, 2, 16, fake_a, 16, NULL));
  expect_bad("generate null out", pfb_testvec_generate(kind, param, 2, 16, NULL, 16, NULL));
  expect_bad("generate misaligned out", pfb_testvec_generate(kind, param, 2, 16, odd, 16, NULL));
  expect_bad("generate unknown kind", pfb_testvec_generate(kind_bad, param, 2, 16, fake_a, 16, NULL));
  expect_bad("generate NaN frequency", pfb_testvec_generate(kind, param_nan, 2, 16, fake_a, 16, NULL));
  expect_bad("generate infinite width", pfb_testvec_generate(kind, param_inf, 2, 16, fake_a, 16, NULL));

  expect_bad("spurious n = 0", pfb_purity_score_spurious(fake_a, 0, 16, 0, 2, 1.0, 30, expected, result, NULL));
  expect_bad("spurious n_vec = 0", pfb_purity_score_spurious(fake_a, 0, 16, 16, 0, 1.0, 30, expected, result, NULL));
  expect_bad("spurious n_vec > 65535",
             pfb_purity_score_spurious(fake_a, 0, 16, 16, 65536, 1.0, 30, expected, result, NULL));
  expect_bad("spurious stride < n", pfb_purity_score_spurious(fake_a, 0, 15, 16, 2, 1.0, 30, expected, result, NULL));
  expect_bad("spurious null series", pfb_purity_score_spurious(NULL, 0, 16, 16, 2, 1.0, 30, expected, result, NULL));
  expect_bad("spurious null result", pfb_purity_score_spurious(fake_a, 0, 16, 16, 2, 1.0, 30, expected, NULL, NULL));
  expect_bad("spurious misaligned series",
             pfb_purity_score_spurious(odd, 0, 16, 16, 2, 1.0, 30, expected, result, NULL));
  expect_bad("spurious domain < 0", pfb_purity_score_spurious(fake_a, 0, 16, 16, 2, 1.0, -1, expected, result, NULL));
  expect_bad("spurious dtype 2", pfb_purity_score_spurious(fake_a, 2, 16, 16, 2, 1.0, 30, expected, result, NULL));
  expect_bad("spurious NaN scale", pfb_purity_score_spurious(fake_a, 1, 16, 16, 2, NAN, 0, NULL, result, NULL));
  expect_bad("spurious infinite scale",
             pfb_purity_score_spurious(fake_a, 1, 16, 16, 2, INFINITY, 0, NULL, result, NULL));

  expect_bad("difference n = 0", pfb_purity_score_difference(fake_a, 16, fake_b, 16, 0, 2, result, NULL));
  expect_bad("difference n_vec = 0", pfb_purity_score_difference(fake_a, 16, fake_b, 16, 16, 0, result, NULL));
  expect_bad("difference n_vec > 65535",
             pfb_purity_score_difference(fake_a, 16, fake_b, 16, 16, 65536, result, NULL));
  expect_bad("difference a stride < n", pfb_purity_score_difference(fake_a, 15, fake_b, 16, 16, 2, result, NULL));
  expect_bad("difference b stride < n", pfb_purity_score_difference(fake_a, 16, fake_b, 15, 16, 2, result, NULL));
  expect_bad("difference null a", pfb_purity_score_difference(NULL, 16, fake_b, 16, 16, 2, result, NULL));
  expect_bad("difference null b", pfb_purity_score_difference(fake_a, 16, NULL, 16, 16, 2, result, NULL));
  expect_bad("difference null result", pfb_purity_score_difference(fake_a, 16, fake_b, 16, 16, 2, NULL, NULL));
  expect_bad("difference misaligned b", pfb_purity_score_difference(fake_a, 16, odd, 16, 16, 2, result, NULL));

  printf("verify_args_check: %d calls, %d failures\n", calls, failures);
  return failures ? 1 : 0;
}
