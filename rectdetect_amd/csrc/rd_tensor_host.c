/* rectdetect-mi355x: model-ready tensors - the host's part of the contract in include/rectdetect_hip.h ("model-ready tensors"): whether a spec is legal, the bytes
 * of a quad's tensor, step 4 for one element, and the limits.  Binary32 operations one at a time, never contracted (-ffp-contract=off), and the conversions to
 * binary16 and bfloat16 in integers, so that the result does not depend on what the compiler knows about half types.  No HIP in here:
 * tests/native/tensor_host_check.c builds this file alone under the sanitizers. */
#include "rectdetect_hip.h"
#include <math.h>
#include <string.h>

static int channels_of(const rd_tensor_spec *spec) { return spec->channels == RD_TENSOR_GRAY ? 1 : 3; }
static int size_of(int dtype) { return dtype == RD_TENSOR_U8 ? 1 : (dtype == RD_TENSOR_F32 ? 4 : 2); }
static int enums_ok(const rd_tensor_spec *spec) {
  return spec->dtype >= RD_TENSOR_U8 && spec->dtype <= RD_TENSOR_F32 && (spec->layout == RD_TENSOR_NHWC || spec->layout == RD_TENSOR_NCHW) &&
         spec->channels >= RD_TENSOR_BGR && spec->channels <= RD_TENSOR_GRAY && (spec->oversample == 1 || spec->oversample == 2 || spec->oversample == 4);
}

int rd_tensor_spec_ok(const rd_tensor_spec *spec, int pw, int ph) {
  if (!spec || !enums_ok(spec)) return 0;
  if (pw < 1 || ph < 1 || pw > 16384 / spec->oversample || ph > 16384 / spec->oversample) return 0;
  if (spec->dtype != RD_TENSOR_U8)
    for (int c = 0; c < channels_of(spec); c++) if (!isfinite(spec->scale[c]) || !isfinite(spec->bias[c])) return 0;
  return 1;
}

size_t rd_tensor_bytes(const rd_tensor_spec *spec, int pw, int ph) {
  if (!rd_tensor_spec_ok(spec, pw, ph)) return 0;
  return (size_t)pw * (size_t)ph * (size_t)(channels_of(spec) * size_of(spec->dtype));
}

/* binary32 bits -> binary16 bits: round to nearest even, overflow to infinity, subnormals kept (a NaN stays a NaN) */
static uint16_t half_bits(uint32_t u) {
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);      /* 65520 and above, infinity included */
  const int e = (int)(a >> 23);
  const uint32_t mant = a & 0x7FFFFFu;
  if (e >= 113) {                                               /* a normal half: 13 bits go; a carry out of the mantissa moves into the exponent */
    uint32_t h = ((uint32_t)(e - 112) << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
  }
  if (e < 102) return (uint16_t)sign;                           /* below 2^-25: zero */
  const int shift = 126 - e;                                    /* 14 .. 24: multiples of 2^-24 */
  const uint32_t m = mant | 0x800000u, half = 1u << (shift - 1), rem = m & ((1u << shift) - 1u);
  uint32_t h = m >> shift;
  if (rem > half || (rem == half && (h & 1u))) h++;
  return (uint16_t)(sign | h);
}

int rd_tensor_element(const rd_tensor_spec *spec, int c, int32_t S, void *out) {
  if (!spec || !out || !enums_ok(spec) || c < 0 || c >= channels_of(spec)) return 0;
  const int m = spec->oversample, mm = m * m, sh = m == 1 ? 0 : (m == 2 ? 2 : 4);
  if (spec->dtype == RD_TENSOR_U8) {
    const uint8_t b = (uint8_t)((S + mm / 2) >> sh);
    memcpy(out, &b, 1);
    return 1;
  }
  volatile float v = (float)S * (1.0f / (float)mm);      /* (volatile: one rounded binary32 value after every step, whatever the machine's registers hold) */
  v = v * spec->scale[c];
  v = v + spec->bias[c];
  const float f = v;
  uint32_t u;
  memcpy(&u, &f, 4);
  if (spec->dtype == RD_TENSOR_F32) { memcpy(out, &u, 4); return 4; }
  const uint16_t h = spec->dtype == RD_TENSOR_F16 ? half_bits(u) : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  memcpy(out, &h, 2);
  return 2;
}

void rd_tensor_limits(int32_t out[4]) {
  out[0] = 1 << RD_TENSOR_U8 | 1 << RD_TENSOR_F16 | 1 << RD_TENSOR_BF16 | 1 << RD_TENSOR_F32;
  out[1] = 1 << RD_TENSOR_NHWC | 1 << RD_TENSOR_NCHW;
  out[2] = 1 << RD_TENSOR_BGR | 1 << RD_TENSOR_RGB | 1 << RD_TENSOR_GRAY;
  out[3] = 1 | 2 | 4;
}
