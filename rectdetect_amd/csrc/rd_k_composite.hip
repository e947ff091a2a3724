// rectdetect-mi355x: composited quads for gfx950 - a colour or an image pasted into every quad of a job, in any of the six pixel formats.  The arithmetic is the
// contract in include/rectdetect_hip.h ("composited quads"): the inverse of the rectifier's map, evaluated per frame pixel in double exactly as written there;
// nothing here may reorder, contract or step it (-ffp-contract=off, see rd_device.h).
//
// Gather, touched tiles only.  The host knows every item's pixel box before the launch, so the grid is its list of touched tiles (rd_composite_tiles): a tile
// that nothing reaches has no block.
//   * a block is ONE wave on a tile of 32 x 16 pixels; the 8 x 8 lanes own 4 x 2 pixels each - and with them the two chroma samples of NV12 / I420.  No LDS, no
//     barrier: the annotator's measurement ("Annotated frames") put 17 us per job on 1020 blocks of 256 threads passing barriers before they learn that
//     their tile is empty
//   * one pixel has one owner, which asks the items from the HIGHEST index down and keeps the first that covers it: painter's order by construction
//   * binning inside the wave: lane l tests the boxes of items base + l of a chunk of 64 against the tile, a ballot gives the chunk's mask, the wave walks its set
//     bits from the top.  A lane stops asking once all of its pixels are decided, the wave when every lane has.  No per-tile capacity exists
//   * an item's record is read at a wave-uniform index: scalar loads, the nine doubles in scalar registers
//   * stores: covered pixels only, byte by byte (in place nothing else may be written, and a pixel is never read)
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_comp.h"

namespace {

using namespace rdpix;

constexpr int TW = RD_COMP_TILE_W, TH = RD_COMP_TILE_H, PXW = 4, PXH = 2;
static_assert((TW / PXW) * (TH / PXH) == 64 && RD_COMP_CHUNK == 64, "one wave per tile, a lane per item of a chunk");

// the colour b | g << 8 | r << 16 of patch `p` (pw x ph BGR bytes) at (s, t) of the unit square
__device__ __forceinline__ uint32_t paste(const uint8_t *p, int pw, int ph, double s, double t) {
  const double u = s * (double)pw - 0.5, v = t * (double)ph - 0.5;
  const int ui = fix8(u, (double)(pw - 1) * 256.0), vi = fix8(v, (double)(ph - 1) * 256.0);
  const int x0 = ui >> 8, fx = ui & 255, x1 = min(x0 + 1, pw - 1);
  const int y0 = vi >> 8, fy = vi & 255, y1 = min(y0 + 1, ph - 1);
  const uint8_t *r0 = p + (size_t)y0 * pw * 3, *r1 = p + (size_t)y1 * pw * 3;
  uint32_t col = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) col |= (uint32_t)blend8(lerp8(r0[x0 * 3 + c], r0[x1 * 3 + c], fx), lerp8(r1[x0 * 3 + c], r1[x1 * 3 + c], fx), fy) << (8 * c);
  return col;
}

template <int FMT> __global__ __launch_bounds__(64) void k_composite(PixFrame F, const rd_comp_rec *__restrict__ recs, int n, const int2 *__restrict__ tiles,
                                                                      const uint8_t *__restrict__ patches, int pw, int ph) {
  constexpr bool YUV = is_yuv(FMT);
  const int2 tile = tiles[blockIdx.x];
  const int lane = threadIdx.x;
  const int tx0 = tile.x * TW, ty0 = tile.y * TH, tx1 = min(tx0 + TW, F.iw) - 1, ty1 = min(ty0 + TH, F.ih) - 1;      // the tile, inside the frame
  const int x0 = tx0 + (lane & 7) * PXW, y0 = ty0 + (lane >> 3) * PXH;      // this lane's pixels: x0 .. x0 + 3, y0 .. y0 + 1
  // bit j * 4 + i: pixel (x0 + i, y0 + j) lies in the frame and no item has claimed it yet
  uint32_t open = 0;
#pragma unroll
  for (int j = 0; j < PXH; j++)
#pragma unroll
    for (int i = 0; i < PXW; i++) open |= (x0 + i < F.iw && y0 + j < F.ih) ? 1u << (j * PXW + i) : 0u;
  const uint32_t inframe = open;
  uint32_t col[PXH][PXW];
#pragma unroll
  for (int j = 0; j < PXH; j++)
#pragma unroll
    for (int i = 0; i < PXW; i++) col[j][i] = 0;
  double X[PXW], Y[PXH];
#pragma unroll
  for (int i = 0; i < PXW; i++) X[i] = (double)(x0 + i);
#pragma unroll
  for (int j = 0; j < PXH; j++) Y[j] = (double)(y0 + j);

  bool done = __ballot(open != 0) == 0;
  for (int base = ((n - 1) / 64) * 64; base >= 0 && !done; base -= 64) {
    const int idx = base + lane;
    bool hit = false;
    if (idx < n) {
      const rd_comp_rec *r = recs + idx;
      hit = r->status && r->box[0] <= tx1 && r->box[2] >= tx0 && r->box[1] <= ty1 && r->box[3] >= ty0;      // (an empty box is 0, 0, -1, -1: it reaches nothing)
    }
    unsigned long long m = __ballot(hit);
    while (m && !done) {
      const int k = 63 - __clzll((long long)m);
      m &= ~(1ull << k);
      const rd_comp_rec *r = recs + __builtin_amdgcn_readfirstlane(base + k);
      if (open) {
        const double A = r->inv[0], B = r->inv[1], C = r->inv[2], D = r->inv[3], E = r->inv[4], Fc = r->inv[5], G = r->inv[6], H = r->inv[7], I = r->inv[8];
        const int bx0 = r->box[0], by0 = r->box[1], bx1 = r->box[2], by1 = r->box[3], patch = r->patch;
        const uint32_t fill = r->col[0] | (r->col[1] << 8) | ((uint32_t)r->col[2] << 16);
        const uint8_t *pp = patch >= 0 ? patches + (size_t)patch * pw * ph * 3 : patches;
        // the products of a column and of a row are the same two operands for every pixel that shares them: computed once, not stepped
        double AX[PXW], DX[PXW], GX[PXW], BY[PXH], EY[PXH], HY[PXH];
#pragma unroll
        for (int i = 0; i < PXW; i++) { AX[i] = A * X[i]; DX[i] = D * X[i]; GX[i] = G * X[i]; }
#pragma unroll
        for (int j = 0; j < PXH; j++) { BY[j] = B * Y[j]; EY[j] = E * Y[j]; HY[j] = H * Y[j]; }
        // s and t of all eight pixels without a branch between them: sixteen independent divisions that the scheduler interleaves (a division is a chain of some
        // twenty dependent operations; pixel by pixel behind a test each, a wave with one item to ask spent most of its time waiting for them one after the other)
        double S[PXH][PXW], T[PXH][PXW];
#pragma unroll
        for (int j = 0; j < PXH; j++)
#pragma unroll
          for (int i = 0; i < PXW; i++) {
            const double wn = (GX[i] + HY[j]) + I;
            S[j][i] = ((AX[i] + BY[j]) + C) / wn;
            T[j][i] = ((DX[i] + EY[j]) + Fc) / wn;
          }
#pragma unroll
        for (int j = 0; j < PXH; j++)
#pragma unroll
          for (int i = 0; i < PXW; i++) {
            const uint32_t bit = 1u << (j * PXW + i);
            const double s = S[j][i], t = T[j][i];
            if ((open & bit) && x0 + i >= bx0 && x0 + i <= bx1 && y0 + j >= by0 && y0 + j <= by1 && s >= 0.0 && s < 1.0 && t >= 0.0 && t < 1.0) {      // (a NaN or an infinity fails)
              open &= ~bit;
              col[j][i] = patch >= 0 ? paste(pp, pw, ph, s, t) : fill;
            }
          }
      }
      done = __ballot(open != 0) == 0;
    }
  }

  const uint32_t cov = inframe & ~open;
  if (!cov) return;
  if (!YUV) {
    constexpr int BPP = bpp(FMT);
    constexpr bool SWAP = rb_swapped(FMT);
#pragma unroll
    for (int j = 0; j < PXH; j++) {
      uint8_t *row = F.pl[0] + (size_t)(y0 + j) * F.pitch[0] + (size_t)x0 * BPP;
#pragma unroll
      for (int i = 0; i < PXW; i++) {
        if (!(cov & (1u << (j * PXW + i)))) continue;
        const uint32_t c = col[j][i];
        row[i * BPP + (SWAP ? 2 : 0)] = (uint8_t)c;
        row[i * BPP + 1] = (uint8_t)(c >> 8);
        row[i * BPP + (SWAP ? 0 : 2)] = (uint8_t)(c >> 16);
      }
    }
  } else {      // (iw and ih are even and so is a lane's origin: its two 2 x 2 blocks lie inside the frame or outside as a whole)
#pragma unroll
    for (int j = 0; j < PXH; j++) {
      uint8_t *row = F.pl[0] + (size_t)(y0 + j) * F.pitch[0] + x0;
#pragma unroll
      for (int i = 0; i < PXW; i++) {
        if (!(cov & (1u << (j * PXW + i)))) continue;
        const uint32_t c = col[j][i];
        row[i] = (uint8_t)bgr_y(c & 255, (c >> 8) & 255, (c >> 16) & 255);
      }
    }
    const int cy = y0 >> 1;
#pragma unroll
    for (int q = 0; q < PXW / 2; q++) {
      int cnt = 0, sb = 0, sg = 0, sr = 0;
#pragma unroll
      for (int j = 0; j < PXH; j++)
#pragma unroll
        for (int i = 2 * q; i < 2 * q + 2; i++) {
          if (!(cov & (1u << (j * PXW + i)))) continue;
          const uint32_t c = col[j][i];
          cnt++; sb += c & 255; sg += (c >> 8) & 255; sr += (c >> 16) & 255;
        }
      if (!cnt) continue;
      const int h = cnt >> 1, mb = (sb + h) / cnt, mg = (sg + h) / cnt, mr = (sr + h) / cnt;
      const uint8_t U = (uint8_t)bgr_u(mb, mg, mr), V = (uint8_t)bgr_v(mb, mg, mr);
      const int cx = (x0 >> 1) + q;
      if (FMT == RD_PIX_NV12) {
        uint8_t *uv = F.pl[1] + (size_t)cy * F.pitch[1] + (size_t)cx * 2;
        uv[0] = U; uv[1] = V;
      } else {
        F.pl[1][(size_t)cy * F.pitch[1] + cx] = U;
        F.pl[2][(size_t)cy * F.pitch[2] + cx] = V;
      }
    }
  }
}

}  // namespace

namespace rdk {

void composite(hipStream_t s, int fmt, const PixFrame &F, const rd_comp_rec *recs, int n, const int32_t *tiles, int ntiles, const uint8_t *patches, int pw, int ph) {
  if (n <= 0 || ntiles <= 0) return;
  const int2 *t = (const int2 *)tiles;
  const dim3 block(64), grid(ntiles);
  if (!dispatch(fmt, [&](auto f) { hipLaunchKernelGGL(k_composite<f.value>, grid, block, 0, s, F, recs, n, t, patches, pw, ph); })) {
    fprintf(stderr, "rdk::composite: unknown pixel format %d\n", fmt); abort();      // (the entry points refuse it first)
  }
}

}  // namespace rdk
