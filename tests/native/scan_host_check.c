/* TEST INFRASTRUCTURE.  The scan rectifier's host-only code (csrc/rd_scan_host.c: whether a spec is legal, the bytes of a page, one pixel's ink and flat value, the
 * limits) under AddressSanitizer + UndefinedBehaviorSanitizer, as a plain process: built and run by tests/test_cpu_scan.py.  Every G0, a grid of (N, T) with the
 * extremes - where a signed overflow in the contract's products would be reported -, k and d at their ends, both polarities, each result written into a buffer with
 * guard bytes around it and compared with the contract's steps restated here in 64 bits.  A sanitizer report ends the process with a non-zero exit code. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) fprintf(stderr, "scan_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main(void) {
  int32_t lim[10];
  for (int k = 0; k < 10; k++) lim[k] = -7;
  rd_scan_limits(lim + 1);
  CHECK(lim[0] == -7 && lim[9] == -7);
  CHECK(lim[1] == 7 && lim[2] == (1 | 2 | 4) && lim[3] == 63 && lim[4] >= 64 && lim[4] % 64 == 0 && lim[5] >= 1 && lim[6] == 0 && lim[7] == 0 && lim[8] == 0);
  CHECK(sizeof(rd_scan_spec) == 32);

  static const int ns[] = { 1, 2, 9, 25, 289, 961, 4096, 16128, 16129 }, kd[] = { 0, 26, 255 }, whites[] = { 1, 230, 255 };
  long pixels = 0;
  for (unsigned ni = 0; ni < sizeof(ns) / sizeof(ns[0]); ni++)
    for (int ti = 0; ti <= 18; ti++)      /* 0, sixteenths of the most a window can hold up to all of it, 1, and one less than the most */
      for (int ki = 0; ki < 3; ki++)
        for (int di = 0; di < 3; di++)
          for (int inv = 0; inv < 2; inv++) {
            const int N = ns[ni];
            const int64_t most = 255 * (int64_t)N, T = ti <= 16 ? most * ti / 16 : (ti == 17 ? 1 : most - 1);
            rd_scan_spec s = { RD_SCAN_BILEVEL, 63, kd[ki], kd[di], whites[(ni + ti) % 3], 1, inv, 0 };
            for (int G0 = 0; G0 < 256; G0++) {
              uint8_t buf[6];
              memset(buf, 0xA5, sizeof(buf));
              CHECK(rd_scan_pixel(&s, G0, N, (int)T, buf + 1, buf + 4) == 1);
              CHECK(buf[0] == 0xA5 && buf[2] == 0xA5 && buf[3] == 0xA5 && buf[5] == 0xA5);
              const int64_t G = inv ? 255 - G0 : G0;
              const int ink = 256 * (int64_t)N * (G + s.d) < (256 - (int64_t)s.k) * T;
              int64_t F = T == 0 ? s.white : (G * N * s.white + (T >> 1)) / T;
              if (F > 255) F = 255;
              CHECK(buf[1] == ink && buf[4] == F);
              pixels++;
            }
          }
  CHECK(pixels > 100000);
  CHECK(256LL * 127 * 127 * 510 == 2105802240LL && 2105802240LL < 2147483648LL);

  /* refused arguments write nothing; a NULL result is skipped */
  rd_scan_spec ok = { RD_SCAN_BITS, 15, 26, 0, 230, 1, 0, 0 }, bad;
  uint8_t a = 0xA5, b = 0xA5;
  CHECK(rd_scan_pixel(NULL, 1, 1, 1, &a, &b) == 0 && rd_scan_pixel(&ok, -1, 1, 1, &a, &b) == 0 && rd_scan_pixel(&ok, 256, 1, 1, &a, &b) == 0);
  CHECK(rd_scan_pixel(&ok, 1, 0, 0, &a, &b) == 0 && rd_scan_pixel(&ok, 1, 16130, 0, &a, &b) == 0 && rd_scan_pixel(&ok, 1, 4, -1, &a, &b) == 0 && rd_scan_pixel(&ok, 1, 4, 1021, &a, &b) == 0);
  bad = ok; bad.k = 256; CHECK(rd_scan_pixel(&bad, 1, 1, 1, &a, &b) == 0);
  bad = ok; bad.d = -1; CHECK(rd_scan_pixel(&bad, 1, 1, 1, &a, &b) == 0);
  bad = ok; bad.white = 0; CHECK(rd_scan_pixel(&bad, 1, 1, 1, &a, &b) == 0);
  bad = ok; bad.invert = 2; CHECK(rd_scan_pixel(&bad, 1, 1, 1, &a, &b) == 0);
  CHECK(a == 0xA5 && b == 0xA5);
  CHECK(rd_scan_pixel(&ok, 10, 4, 400, NULL, &b) == 1 && b == 23 && rd_scan_pixel(&ok, 10, 4, 400, &a, NULL) == 1 && a == 1 && rd_scan_pixel(&ok, 10, 4, 400, NULL, NULL) == 1);

  /* legal and illegal specs, and the bytes */
  CHECK(rd_scan_spec_ok(&ok, 128, 96) == 1 && rd_scan_bytes(&ok, 128, 96) == 16 * 96 && rd_scan_bytes(&ok, 9, 5) == 10 && rd_scan_bytes(&ok, 1, 1) == 1);
  CHECK(rd_scan_spec_ok(NULL, 8, 8) == 0 && rd_scan_bytes(NULL, 8, 8) == 0);
  bad = ok; bad.mode = RD_SCAN_FLAT; CHECK(rd_scan_bytes(&bad, 9, 5) == 45);
  bad.mode = RD_SCAN_BILEVEL; CHECK(rd_scan_bytes(&bad, 16384, 16384) == (size_t)16384 * 16384 && rd_scan_bytes(&bad, 16385, 1) == 0 && rd_scan_bytes(&bad, 1, 16385) == 0 && rd_scan_bytes(&bad, 0, 1) == 0 && rd_scan_bytes(&bad, 1, -1) == 0);
  bad.oversample = 4; CHECK(rd_scan_spec_ok(&bad, 4096, 4096) == 1 && rd_scan_spec_ok(&bad, 4097, 8) == 0 && rd_scan_spec_ok(&bad, 8, 4097) == 0);
  static const int32_t wrong[8][4] = { { -1, 3, 255, 3 }, { 0, 64, -1, 64 }, { -1, 256, -1, 256 }, { -1, 256, -1, 256 }, { 0, 256, -1, 256 }, { 0, 3, 8, -1 }, { -1, 2, 255, 2 }, { 1, -1, 255, 1 } };
  for (int field = 0; field < 8; field++)
    for (int k = 0; k < 4; k++) {
      bad = ok;
      ((int32_t *)&bad)[field] = wrong[field][k];
      CHECK(rd_scan_spec_ok(&bad, 8, 8) == 0 && rd_scan_bytes(&bad, 8, 8) == 0);
    }

  if (failures) { fprintf(stderr, "scan_host_check: %d check(s) failed\n", failures); return 1; }
  printf("scan_host_check: ok (%ld pixels)\n", pixels);
  return 0;
}
