/* rectdetect-mi355x: decoded quads - the host's part of the contract in include/rectdetect_hip.h ("decoded quads"): whether a spec is legal, the cell of a pixel,
 * the rotations of a payload, what distance a dictionary keeps, a greedy dictionary generator, the image of a code and the quad that shows it upright.
 * No HIP in here: tests/native/code_host_check.c builds this file alone under the sanitizers. */
#include "rectdetect_hip.h"
#include "rd_code_tile.h"

static int n_ok(int n) { return n >= RD_CODE_MIN_N && n <= RD_CODE_MAX_N; }
static uint64_t payload_mask(int n) { return n * n == 64 ? ~(uint64_t)0 : (((uint64_t)1 << (n * n)) - 1); }
static int popcount64(uint64_t v) { return __builtin_popcountll(v); }

int rd_code_spec_ok(const rd_code_spec *spec, int pw, int ph) {
  if (!spec) return 0;
  if (!n_ok(spec->n) || spec->border < 1 || spec->border > RD_CODE_MAX_BORDER || spec->inset < 0 || spec->inset > RD_CODE_MAX_INSET) return 0;
  if ((spec->polarity != 0 && spec->polarity != 1) || (spec->oversample != 1 && spec->oversample != 2 && spec->oversample != 4)) return 0;
  const int C = spec->n + 2 * spec->border, least = spec->inset ? 4 * C : C;
  if (spec->contrast < 0 || spec->contrast > 255 || spec->max_border < 0 || spec->max_border > C * C - spec->n * spec->n) return 0;
  if (spec->max_hamming < 0 || spec->max_hamming > spec->n * spec->n) return 0;
  return pw >= least && ph >= least && pw <= RD_CODE_MAX_SIDE && ph <= RD_CODE_MAX_SIDE;
}

size_t rd_code_bytes(const rd_code_spec *spec, int pw, int ph) { return rd_code_spec_ok(spec, pw, ph) ? sizeof(rd_code) : 0; }

int rd_code_cell_of(const rd_code_spec *spec, int pw, int ph, int i, int j, int *counted) {
  if (!rd_code_spec_ok(spec, pw, ph) || i < 0 || i >= pw || j < 0 || j >= ph) return -1;
  const int C = spec->n + 2 * spec->border, in = spec->inset;
  const int ax = (2 * i + 1) * C, ay = (2 * j + 1) * C;      /* at most 2047 * 12 */
  const int cx = ax / (2 * pw), fx = ax % (2 * pw), cy = ay / (2 * ph), fy = ay % (2 * ph);
  if (counted) *counted = in * pw <= 4 * fx && 4 * fx <= (8 - in) * pw && in * ph <= 4 * fy && 4 * fy <= (8 - in) * ph;
  return cy * C + cx;
}

static uint64_t rot1(uint64_t bits, int n) {
  uint64_t out = 0;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) out |= ((bits >> ((n - 1 - c) * n + r)) & 1) << (r * n + c);
  return out;
}

uint64_t rd_code_rotate(uint64_t bits, int n, int k) {
  if (!n_ok(n)) return 0;
  bits &= payload_mask(n);
  for (k = ((k % 4) + 4) % 4; k > 0; k--) bits = rot1(bits, n);
  return bits;
}

void rd_code_limits(int32_t out[8]) {
  out[0] = RD_CODE_MIN_N;
  out[1] = RD_CODE_MAX_N;
  out[2] = RD_CODE_MAX_BORDER;
  out[3] = RD_CODE_MAX_INSET;
  out[4] = 1 | 2 | 4;
  out[5] = RD_CODE_MAX_SIDE;
  out[6] = RD_CODE_MAX_DICT;
  out[7] = (int32_t)sizeof(rd_code);
}

/* the smallest distance of `code` (its rotations in r[0..3]) to itself turned */
static int self_distance(const uint64_t r[4]) {
  int d = RD_CODE_NONE;
  for (int k = 1; k < 4; k++) { const int p = popcount64(r[k] ^ r[0]); if (p < d) d = p; }
  return d;
}

/* the smallest distance of a code in any rotation (r[0..3]) to the first m entries of dict */
static int cross_distance(const uint64_t r[4], const uint64_t *dict, int m) {
  int d = RD_CODE_NONE;
  for (int b = 0; b < m; b++)
    for (int k = 0; k < 4; k++) { const int p = popcount64(r[k] ^ dict[b]); if (p < d) d = p; }
  return d;
}

int rd_code_distance(const uint64_t *dict, int ndict, int n) {
  if (!n_ok(n) || ndict < 0 || ndict > RD_CODE_MAX_DICT || (ndict > 0 && !dict)) return -1;
  for (int a = 0; a < ndict; a++) if (dict[a] & ~payload_mask(n)) return -1;
  int d = RD_CODE_NONE;
  for (int a = 0; a < ndict; a++) {      /* (popcount(rot_k(a) ^ b) over k is the same set as popcount(a ^ rot_k(b)): each pair once) */
    uint64_t r[4] = { dict[a], 0, 0, 0 };
    for (int k = 1; k < 4; k++) r[k] = rot1(r[k - 1], n);
    const int s = self_distance(r), c = cross_distance(r, dict, a);
    if (s < d) d = s;
    if (c < d) d = c;
  }
  return d;
}

int rd_code_dictionary(int n, int count, int min_dist, uint64_t seed, int tries, uint64_t *out) {
  if (!n_ok(n) || count < 0 || count > RD_CODE_MAX_DICT || min_dist < 0 || tries < 0 || (count > 0 && !out)) return -1;
  uint64_t s = seed;
  int found = 0;
  for (int t = 0; t < tries && found < count; t++) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uint64_t r[4] = { z & payload_mask(n), 0, 0, 0 };
    for (int k = 1; k < 4; k++) r[k] = rot1(r[k - 1], n);
    if (self_distance(r) >= min_dist && cross_distance(r, out, found) >= min_dist) out[found++] = r[0];
  }
  return found;
}

size_t rd_code_render(const rd_code_spec *spec, uint64_t bits, int cell_px, uint8_t *out) {
  if (!spec || !out || !n_ok(spec->n) || spec->border < 1 || spec->border > RD_CODE_MAX_BORDER || (spec->polarity != 0 && spec->polarity != 1)) return 0;
  if (cell_px < 1 || cell_px > 64 || (bits & ~payload_mask(spec->n))) return 0;
  const int n = spec->n, b = spec->border, C = n + 2 * b, S = C * cell_px;
  for (int y = 0; y < S; y++) {
    const int r = y / cell_px - b;
    for (int x = 0; x < S; x++) {
      const int c = x / cell_px - b;
      const int v = r >= 0 && r < n && c >= 0 && c < n ? (int)((bits >> (r * n + c)) & 1) : 0;
      out[(size_t)y * S + x] = (v ^ spec->polarity) ? 255 : 0;
    }
  }
  return (size_t)S * S;
}

void rd_code_upright(const double quad[8], int rot, double out[8]) {
  if (!quad || !out) return;
  rot = ((rot % 4) + 4) % 4;
  for (int c = 0; c < 4; c++) {
    const int from = (c + 4 - rot) % 4;
    out[2 * c] = quad[2 * from];
    out[2 * c + 1] = quad[2 * from + 1];
  }
}
