// rectdetect-mi355x: scanned pages for gfx950 - the second launch of a scan job: from the G plane the tensor kernel wrote (rd_k_tensor.hip, { U8, NHWC, GRAY, m }) to
// shading-corrected bytes, bilevel bytes or packed bit rows.  The arithmetic is the contract in include/rectdetect_hip.h ("scanned pages"): integers only, no
// atomics, nothing reordered in a way that could change a result (sums of integers: any order is exact).
//
// Launch shape: grid (tiles in x, tiles in y, quads), a block is 4 waves and makes a tile of 64 x 16 output pixels (rd_scan_tile.h); wave w makes rows 4w .. 4w+3 of
// it, its 64 lanes 64 consecutive pixels of ONE row - one ballot is then eight whole bytes of a bit row, and no two waves ever write the same byte.
// With r = radius, W = 64 + 2r, H = 16 + 2r, in dynamically sized LDS (r is a run-time value; 13 KB at r = 15, 45 KB at r = 63):
//   0. g[H][W] bytes: the tile and its halo, inverted where the spec says so, 0 outside the patch.  Every load of a thread's batch is issued before the first is
//      used: a block waits for memory once at r <= 24 and three times at r = 63.
//   1. vs[16][W] 16-bit: the COLUMN sums of 2r+1 rows (at most 127 * 255) as running sums down the column, a lane per column; at W <= 128 two waves share a column,
//      eight rows each.  The only step whose work grows with r: 2r + 1 + 2 * 7 byte reads per lane (2r + 1 + 2 * 15 above W = 128).
//   2. P[16][W + 1] 32-bit: the exclusive prefix of a row of vs, by the wave that makes that row's pixels: two or three 64-lane scans.  T = P[x + 2r + 1] - P[x].
// N comes from the clamps, not from counting.  In every step the lanes of a wave run along x over consecutive cells - bytes (four lanes read one dword: a broadcast),
// 16-bit (two lanes per dword) or dwords - so no access has a bank conflict, whatever r makes of the row pitch; the layout needs no padding.
// Stores: FLAT and BILEVEL gather four lanes' bytes into a dword where the row's address in this tile is dword-aligned (it is not in every row of an odd pw) and
// store single bytes in the row's tail group and in misaligned rows; BITS reverses the bits of each byte of the ballot (most significant bit first) and stores the
// eight bytes as one word where the row has eight bytes left and the address is 8-aligned, byte by byte otherwise.  Lanes beyond pw vote 0: the pad bits.
// An invalid quad stores zeros through the same store functions, after the staging (its plane is zero; the status then costs no trip to memory of its own).
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include "rd_scan_tile.h"

namespace {

constexpr int TW = RD_SCAN_TILE_W, TH = RD_SCAN_TILE_H, WAVES = 4, ROWS = TH / WAVES;
static_assert(TW == RD_WAVE && TH % (2 * WAVES) == 0, "a wave row is 64 pixels; two waves split a column's rows evenly");

__host__ __device__ constexpr size_t lds_bytes(int r) { return (size_t)TH * (TW + 2 * r + 1) * 4 + (size_t)TH * (TW + 2 * r) * 2 + (size_t)(TH + 2 * r) * (TW + 2 * r); }

// row j of a page, the 64 pixels from column tx0: v is the pixel's byte (FLAT, BILEVEL) or whether it is ink (BITS), 0 in lanes beyond pw.  Called by whole waves.
template <int MODE> __device__ __forceinline__ void store_row(uint8_t *page, int pw, int tx0, int j, int lane, uint32_t v) {
  if (MODE == RD_SCAN_BITS) {
    const unsigned long long rev = __builtin_bswap64(__builtin_bitreverse64(__ballot(v != 0)));      // byte b: pixels 8b .. 8b+7, the first in bit 7
    const int rb = (pw + 7) >> 3, nb = min(8, rb - (tx0 >> 3));
    uint8_t *row = page + (size_t)j * rb + (tx0 >> 3);
    if (nb == 8 && ((uintptr_t)row & 7) == 0) { if (lane == 0) *(unsigned long long *)row = rev; }
    else if (lane < nb) row[lane] = (uint8_t)(rev >> (8 * lane));
  } else {
    const int cnt = min(TW, pw - tx0);
    uint8_t *row = page + (size_t)j * pw + tx0;
    if (((uintptr_t)row & 3) == 0) {
      const uint32_t w = v | (__shfl_down(v, 1, RD_WAVE) << 8) | (__shfl_down(v, 2, RD_WAVE) << 16) | (__shfl_down(v, 3, RD_WAVE) << 24);
      if ((lane | 3) < cnt) { if ((lane & 3) == 0) *(uint32_t *)(row + lane) = w; }
      else if (lane < cnt) row[lane] = (uint8_t)v;      // the row's tail group
    } else if (lane < cnt) row[lane] = (uint8_t)v;
  }
}

template <int MODE> __global__ __launch_bounds__(TW * WAVES) void k_scan(uint8_t *out, const uint8_t *plane, const rdk::RectifyQuad *quads, int pw, int ph, size_t patch_bytes,
                                                                         int r, int k, int d, int white, int invert) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, wave = rd::rd_ty();
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, i = tx0 + lane;
  uint8_t *page = out + (size_t)blockIdx.z * patch_bytes;
  const int status = quads[blockIdx.z].status;      // (asked for here, looked at behind the staging: the two trips to memory overlap; an invalid quad's plane is there, and zero)
  const int W = TW + 2 * r, H = TH + 2 * r, PP = W + 1;
  uint32_t *P = lds;
  uint16_t *vs = (uint16_t *)(P + TH * PP);
  uint8_t *g = (uint8_t *)(vs + TH * W);
  const uint8_t *src = plane + (size_t)blockIdx.z * ((size_t)pw * ph);

  // 0. the tile and its halo
  constexpr int U = 16, CH = 3;      // rows of a wave and column chunks per batch: W <= 190 is at most three chunks
  for (int y0 = wave; y0 < H; y0 += WAVES * U) {
    uint8_t v[U][CH];
    bool ok[U][CH];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int ch = 0; ch < CH; ch++) {
        const int y = y0 + WAVES * u, c = ch * RD_WAVE + lane, gj = ty0 - r + y, gi = tx0 - r + c;
        ok[u][ch] = y < H && c < W && gj >= 0 && gj < ph && gi >= 0 && gi < pw;
        v[u][ch] = 0;
        if (y < H && ch * RD_WAVE < W) v[u][ch] = src[ok[u][ch] ? (size_t)gj * pw + gi : 0];      // (the whole wave or none of it: rows and chunks that do not exist cost no load)
      }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int ch = 0; ch < CH; ch++) {
        const int y = y0 + WAVES * u, c = ch * RD_WAVE + lane;
        if (y < H && c < W) g[y * W + c] = ok[u][ch] ? (uint8_t)(invert ? 255 - v[u][ch] : v[u][ch]) : (uint8_t)0;
      }
  }
  if (!status) {      // (the whole block)
    for (int q = 0; q < ROWS; q++) {
      const int j = ty0 + wave * ROWS + q;
      if (j < ph) store_row<MODE>(page, pw, tx0, j, lane, 0u);
    }
    return;
  }
  __syncthreads();

  // 1. column sums of 2r+1 rows, for the TH rows of the tile
  {
    const bool two = W <= 2 * RD_WAVE;      // two chunks of columns: waves 0, 1 make rows 0 .. 7, waves 2, 3 rows 8 .. 15; three chunks: waves 0 .. 2 make all rows
    const int c = (two ? wave & 1 : wave) * RD_WAVE + lane, j0 = two ? (wave >> 1) * (TH / 2) : 0, j1 = two ? j0 + TH / 2 : TH;
    if (c < W && (two || wave < 3)) {
      const uint8_t *col = g + c;
      uint32_t s = 0;
#pragma unroll 8
      for (int y = j0; y <= j0 + 2 * r; y++) s += col[y * W];      // (unrolled: eight reads in flight, not one)
      vs[j0 * W + c] = (uint16_t)s;
      for (int j = j0 + 1; j < j1; j++) {
        s += col[(j + 2 * r) * W];
        s -= col[(j - 1) * W];
        vs[j * W + c] = (uint16_t)s;
      }
    }
  }
  __syncthreads();

  // 2. the exclusive prefix of this wave's rows
  {
    uint32_t carry[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; q++) carry[q] = 0;
    if (lane < ROWS) P[(wave * ROWS + lane) * PP] = 0;
    for (int c0 = 0; c0 < W; c0 += RD_WAVE) {
      const int c = c0 + lane;
      uint32_t s[ROWS];      // the rows side by side: four independent chains of exchanges
#pragma unroll
      for (int q = 0; q < ROWS; q++) s[q] = c < W ? vs[(wave * ROWS + q) * W + c] : 0u;
#pragma unroll
      for (int o = 1; o < RD_WAVE; o <<= 1)
#pragma unroll
        for (int q = 0; q < ROWS; q++) {
          const uint32_t t = __shfl_up(s[q], o, RD_WAVE);
          if (lane >= o) s[q] += t;
        }
#pragma unroll
      for (int q = 0; q < ROWS; q++) {
        if (c < W) P[(wave * ROWS + q) * PP + c + 1] = carry[q] + s[q];
        carry[q] += __shfl(s[q], RD_WAVE - 1, RD_WAVE);
      }
    }
  }
  __syncthreads();

  // 3. the pixels
#pragma unroll
  for (int q = 0; q < ROWS; q++) {
    const int jl = wave * ROWS + q, j = ty0 + jl;
    if (j >= ph) break;      // (the whole wave)
    const uint32_t T = P[jl * PP + lane + 2 * r + 1] - P[jl * PP + lane], G = g[(jl + r) * W + lane + r];
    const uint32_t N = (uint32_t)((min(pw - 1, i + r) - max(0, i - r) + 1) * (min(ph - 1, j + r) - max(0, j - r) + 1));
    uint32_t v;
    if (MODE == RD_SCAN_FLAT) v = T == 0 ? (uint32_t)white : min(255u, (G * N * (uint32_t)white + (T >> 1)) / T);
    else {
      const bool ink = 256u * N * (G + (uint32_t)d) < (uint32_t)(256 - k) * T;      // at most 256 * 127^2 * 510 < 2^31
      v = MODE == RD_SCAN_BITS ? (uint32_t)ink : (ink ? 0u : 255u);
    }
    store_row<MODE>(page, pw, tx0, j, lane, i < pw ? v : 0u);
  }
}

}  // namespace

namespace rdk {

void scan(hipStream_t s, uint8_t *out, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_scan_spec &spec) {
  if (n <= 0) return;
  const dim3 block(TW, WAVES), grid((pw + TW - 1) / TW, (ph + TH - 1) / TH, n);
  const size_t lds = lds_bytes(spec.radius), patch_bytes = rd_scan_bytes(&spec, pw, ph);
  if (!patch_bytes) { fprintf(stderr, "rdk::scan: not a legal scan spec for %d x %d\n", pw, ph); abort(); }      // (rd_rectifier_create_scan refuses it first)
#define RD_SCAN_LAUNCH(MODE) hipLaunchKernelGGL((k_scan<MODE>), grid, block, lds, s, out, plane, quads, pw, ph, patch_bytes, spec.radius, spec.k, spec.d, spec.white, spec.invert)
  if (spec.mode == RD_SCAN_FLAT) RD_SCAN_LAUNCH(RD_SCAN_FLAT);
  else if (spec.mode == RD_SCAN_BILEVEL) RD_SCAN_LAUNCH(RD_SCAN_BILEVEL);
  else RD_SCAN_LAUNCH(RD_SCAN_BITS);
#undef RD_SCAN_LAUNCH
}

}  // namespace rdk
