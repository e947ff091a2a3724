/* TEST INFRASTRUCTURE.  The tensor rectifier's host-only code (csrc/rd_tensor_host.c: whether a spec is legal, the bytes of a tensor, one element from its box sum,
 * the limits) under AddressSanitizer + UndefinedBehaviorSanitizer, as a plain process: built and run by tests/test_cpu_tensor.py.  Every dtype, every m, every
 * S in 0 .. 255*m*m with the scale and bias pairs of that test, each element written into a buffer with guard bytes around it and compared with the contract's
 * steps restated here (binary16 by a search for the nearest value, not by the bit manipulation under test).  A sanitizer report ends the process with a non-zero
 * exit code. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) fprintf(stderr, "tensor_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* the value of a non-negative finite binary16 bit pattern, exactly (a double holds every one) */
static double half_value(uint32_t h) {
  const int e = (int)(h >> 10) & 31;
  const double mant = (double)(h & 0x3FF);
  return e == 0 ? ldexp(mant, -24) : ldexp(1024.0 + mant, e - 25);
}

/* round to nearest even of a finite float to binary16, overflow to infinity: by bisection over the 0x7C00 finite magnitudes */
static uint16_t half_nearest(float f) {
  const uint16_t sign = signbit(f) ? 0x8000 : 0;
  const double a = fabs((double)f);
  if (isinf(f)) return (uint16_t)(sign | 0x7C00);
  if (a >= 65520.0) return (uint16_t)(sign | 0x7C00);      /* half way between 65504 and 2^16, the tie goes to the even 2^16: infinity */
  uint32_t lo = 0, hi = 0x7BFF;                            /* the greatest pattern whose value is <= a */
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (half_value(mid) <= a) lo = mid; else hi = mid - 1;
  }
  if (lo == 0x7BFF) return (uint16_t)(sign | lo);
  const double below = a - half_value(lo), above = half_value(lo + 1) - a;      /* exact: differences of doubles with few bits */
  if (above < below || (above == below && (lo & 1))) lo++;
  return (uint16_t)(sign | lo);
}

int main(void) {
  int32_t lim[4];
  rd_tensor_limits(lim);
  CHECK(lim[0] == 15 && lim[1] == 3 && lim[2] == 7 && lim[3] == (1 | 2 | 4));
  CHECK(sizeof(rd_tensor_spec) == 40);

  static const float pairs[][2] = { { 1.0f / 255.0f, -0.5f }, { 0.017124754f, -2.1179039f }, { -0.0171f, 2.0f }, { 1.0f, -0.0f }, { -1.0f, -0.0f }, { 1000.0f, 0.0f },
                                    { 3.0e38f, 1.0f }, { -3.0e38f, 0.0f }, { 1.0f, 2048.0f }, { 1.0f, 256.0f }, { 1.0e-7f, 0.0f }, { 2.3e-10f, 6.0e-8f } };
  static const int ms[3] = { 1, 2, 4 };
  long elements = 0;
  for (int dt = RD_TENSOR_U8; dt <= RD_TENSOR_F32; dt++)
    for (int mi = 0; mi < 3; mi++)
      for (unsigned p = 0; p < sizeof(pairs) / sizeof(pairs[0]); p++)
        for (int ch = RD_TENSOR_BGR; ch <= RD_TENSOR_GRAY; ch += 2) {
          const int m = ms[mi], C = ch == RD_TENSOR_GRAY ? 1 : 3, c = C - 1;
          rd_tensor_spec s;
          memset(&s, 0, sizeof(s));
          s.dtype = dt; s.layout = (int32_t)(p & 1); s.channels = ch; s.oversample = m;
          for (int k = 0; k < 3; k++) { s.scale[k] = NAN; s.bias[k] = NAN; }      /* only channel c's may be read */
          s.scale[c] = pairs[p][0]; s.bias[c] = pairs[p][1];
          const int size = dt == RD_TENSOR_U8 ? 1 : (dt == RD_TENSOR_F32 ? 4 : 2);
          for (int32_t S = 0; S <= 255 * m * m; S++) {
            uint8_t buf[8];
            memset(buf, 0xA5, sizeof(buf));
            CHECK(rd_tensor_element(&s, c, S, buf + 2) == size);
            CHECK(buf[0] == 0xA5 && buf[1] == 0xA5 && buf[2 + size] == 0xA5 && buf[7] == 0xA5);
            elements++;
            if (dt == RD_TENSOR_U8) { CHECK(buf[2] == (uint8_t)((S + m * m / 2) / (m * m))); continue; }
            volatile float v = (float)S / (float)(m * m);
            v = v * pairs[p][0];
            v = v + pairs[p][1];
            const float f = v;
            CHECK(!isnan(f));
            uint32_t u;
            memcpy(&u, &f, 4);
            if (dt == RD_TENSOR_F32) { CHECK(memcmp(buf + 2, &u, 4) == 0); continue; }
            uint16_t got;
            memcpy(&got, buf + 2, 2);
            if (dt == RD_TENSOR_F16) CHECK(got == half_nearest(f));
            else CHECK(got == (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16));
          }
        }
  CHECK(elements > 100000);

  /* refused arguments write nothing */
  rd_tensor_spec ok = { RD_TENSOR_F16, RD_TENSOR_NCHW, RD_TENSOR_RGB, 2, { 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f } };
  uint8_t buf[4] = { 0xA5, 0xA5, 0xA5, 0xA5 };
  rd_tensor_spec bad = ok;
  CHECK(rd_tensor_element(NULL, 0, 0, buf) == 0 && rd_tensor_element(&ok, 0, 0, NULL) == 0 && rd_tensor_element(&ok, 3, 0, buf) == 0 && rd_tensor_element(&ok, -1, 0, buf) == 0);
  bad.dtype = 4; CHECK(rd_tensor_element(&bad, 0, 0, buf) == 0); bad = ok;
  bad.oversample = 3; CHECK(rd_tensor_element(&bad, 0, 0, buf) == 0); bad = ok;
  bad.channels = RD_TENSOR_GRAY; CHECK(rd_tensor_element(&bad, 1, 0, buf) == 0 && rd_tensor_element(&bad, 0, 0, buf) == 2);
  CHECK(buf[2] == 0xA5 && buf[3] == 0xA5);

  /* legal and illegal specs, and the bytes */
  CHECK(rd_tensor_spec_ok(&ok, 128, 128) == 1 && rd_tensor_bytes(&ok, 128, 128) == (size_t)128 * 128 * 3 * 2);
  CHECK(rd_tensor_spec_ok(NULL, 8, 8) == 0 && rd_tensor_bytes(NULL, 8, 8) == 0);
  CHECK(rd_tensor_spec_ok(&ok, 8192, 8192) == 1 && rd_tensor_spec_ok(&ok, 8193, 8) == 0 && rd_tensor_spec_ok(&ok, 8, 8193) == 0 && rd_tensor_spec_ok(&ok, 0, 8) == 0 && rd_tensor_spec_ok(&ok, 8, -1) == 0);
  CHECK(rd_tensor_bytes(&ok, 8192, 8192) == (size_t)8192 * 8192 * 6);
  for (int field = 0; field < 4; field++) {
    static const int32_t wrong[4][3] = { { -1, 4, 255 }, { -1, 2, 3 }, { -1, 3, 4 }, { 0, 3, 8 } };
    for (int k = 0; k < 3; k++) {
      bad = ok;
      if (field == 0) bad.dtype = wrong[0][k]; else if (field == 1) bad.layout = wrong[1][k]; else if (field == 2) bad.channels = wrong[2][k]; else bad.oversample = wrong[3][k];
      CHECK(rd_tensor_spec_ok(&bad, 8, 8) == 0 && rd_tensor_bytes(&bad, 8, 8) == 0);
    }
  }
  bad = ok; bad.scale[2] = INFINITY; CHECK(rd_tensor_spec_ok(&bad, 8, 8) == 0);
  bad.channels = RD_TENSOR_GRAY; CHECK(rd_tensor_spec_ok(&bad, 8, 8) == 1 && rd_tensor_bytes(&bad, 8, 8) == 8 * 8 * 2);      /* (an unused channel's is ignored) */
  bad.bias[0] = NAN; CHECK(rd_tensor_spec_ok(&bad, 8, 8) == 0);
  bad.dtype = RD_TENSOR_U8; CHECK(rd_tensor_spec_ok(&bad, 8, 8) == 1 && rd_tensor_bytes(&bad, 8, 8) == 64);                    /* (U8 ignores them all) */

  if (failures) { fprintf(stderr, "tensor_host_check: %d check(s) failed\n", failures); return 1; }
  printf("tensor_host_check: ok (%ld elements)\n", elements);
  return 0;
}
