/* rectdetect-mi355x: scanned pages - the host's part of the contract in include/rectdetect_hip.h ("scanned pages"): whether a spec is legal, the bytes of a
 * quad's page, steps 3 and 4 for one pixel, and the limits.  Integers only.  No HIP in here: tests/native/scan_host_check.c builds this file alone under the
 * sanitizers. */
#include "rectdetect_hip.h"
#include "rd_scan_tile.h"

/* what rd_scan_pixel needs of a spec */
static int pixel_fields_ok(const rd_scan_spec *spec) {
  return spec->k >= 0 && spec->k <= 255 && spec->d >= 0 && spec->d <= 255 && spec->white >= 1 && spec->white <= 255 && (spec->invert == 0 || spec->invert == 1);
}

int rd_scan_spec_ok(const rd_scan_spec *spec, int pw, int ph) {
  if (!spec || !pixel_fields_ok(spec)) return 0;
  if (spec->mode < RD_SCAN_FLAT || spec->mode > RD_SCAN_BITS || spec->radius < 1 || spec->radius > RD_SCAN_MAX_RADIUS || spec->reserved != 0) return 0;
  if (spec->oversample != 1 && spec->oversample != 2 && spec->oversample != 4) return 0;
  return pw >= 1 && ph >= 1 && pw <= 16384 / spec->oversample && ph <= 16384 / spec->oversample;
}

size_t rd_scan_bytes(const rd_scan_spec *spec, int pw, int ph) {
  if (!rd_scan_spec_ok(spec, pw, ph)) return 0;
  return (size_t)(spec->mode == RD_SCAN_BITS ? (pw + 7) >> 3 : pw) * (size_t)ph;
}

int rd_scan_pixel(const rd_scan_spec *spec, int G0, int N, int T, uint8_t *ink, uint8_t *flat) {
  const int side = 2 * RD_SCAN_MAX_RADIUS + 1;
  if (!spec || !pixel_fields_ok(spec) || G0 < 0 || G0 > 255 || N < 1 || N > side * side || T < 0 || T > 255 * N) return 0;
  const int32_t G = spec->invert ? 255 - G0 : G0;
  if (ink) *ink = (uint8_t)(256 * N * (G + spec->d) < (256 - spec->k) * T);      /* at most 256 * 127^2 * 510 = 2 105 802 240 < 2^31 */
  if (flat) {
    const int32_t F = T == 0 ? spec->white : (G * N * spec->white + (T >> 1)) / T;
    *flat = (uint8_t)(F > 255 ? 255 : F);
  }
  return 1;
}

void rd_scan_limits(int32_t out[8]) {
  out[0] = 1 << RD_SCAN_FLAT | 1 << RD_SCAN_BILEVEL | 1 << RD_SCAN_BITS;
  out[1] = 1 | 2 | 4;
  out[2] = RD_SCAN_MAX_RADIUS;
  out[3] = RD_SCAN_TILE_W;
  out[4] = RD_SCAN_TILE_H;
  out[5] = out[6] = out[7] = 0;
}
