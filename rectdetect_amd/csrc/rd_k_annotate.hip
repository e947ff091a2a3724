// rectdetect-mi355x: annotated frames for gfx950 - rectangles' outlines and line segments drawn into a frame in any of the six pixel formats.  The arithmetic is
// the contract in include/rectdetect_hip.h ("annotated frames"); the coverage test itself is rd_annot_cover.h, shared with the host.
//
// Bin and gather, in ONE launch.  A scatter - a thread per line step - races wherever two lines cross; here every pixel has one owner, which asks each primitive
// that can reach it "do you cover me" in index order, so the last one that says yes wins: painter's order by construction, the same bytes whatever the schedule.
//   * one block of 256 threads per tile of 64 x 32 pixels; a thread owns 4 x 2 pixels - and with them the two chroma samples of NV12 / I420 that belong to them
//   * binning: the block walks the job's primitives 256 at a time, a thread per primitive, and tests the primitive's band against the tile (rd_annot_line_touches:
//     the band's e at the corners of the tile cut to the line's span - the diagonal of a 1920 x 1080 frame passes in 63 of its 1020 tiles).
//     The survivors are compacted IN ORDER into LDS (ballot + prefix count per wave, wave totals through LDS): that is the tile's list, exact, with no capacity to
//     overflow and no scratch memory - a list in global memory would need a count, a scan and a fill launch in front of this one, for a job whose
//     whole drawing is one short launch ("Annotated frames")
//   * drawing: every thread reads the same LDS record (a broadcast, no bank conflict), evaluates e once for its first pixel and steps it by ex / ey to the other
//     seven; a covered pixel remembers the colour.  Nothing is written until all primitives have been asked
//   * writing, in place: covered pixels only - a tile no primitive touches leaves without a memory access; with RD_ANNOT_CLEAR, or into another frame: every
//     pixel of the tile once (the source's, black, or a colour), 12 or 16 bytes per thread and row as dwords where the pointers allow, so that an out-of-place job
//     reads the source tile and writes the destination tile in the same pass
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_kernels.h"

namespace {

using namespace rdpix;

// a job's two frames, of one size, as one kernel argument
struct AnnotFrame { uint8_t *dst[3]; const uint8_t *src[3]; int dpitch[3], spitch[3]; int iw, ih; };

constexpr int TW = rdk::ANNOT_TILE_W, TH = rdk::ANNOT_TILE_H, PXW = 4, PXH = 2, NT = (TW / PXW) * (TH / PXH);
static_assert(NT == rdk::ANNOT_CHUNK && NT % 64 == 0, "a thread per primitive of a chunk, whole waves");
constexpr uint32_t COVERED = 1u << 24;      // above a colour's three bytes: the pixel has one

// nb <= MAXB bytes at p: dwords when there are MAXB of them and p allows, else byte by byte
template <int MAXB> __device__ __forceinline__ void load_bytes(const uint8_t *p, int nb, uint8_t (&b)[MAXB]) {
  if (MAXB % 4 == 0 && nb == MAXB && ((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < MAXB / 4; k++) {
      const uint32_t w = ((const uint32_t *)p)[k];
      b[4 * k] = (uint8_t)w; b[4 * k + 1] = (uint8_t)(w >> 8); b[4 * k + 2] = (uint8_t)(w >> 16); b[4 * k + 3] = (uint8_t)(w >> 24);
    }
  } else {
#pragma unroll
    for (int k = 0; k < MAXB; k++) b[k] = k < nb ? p[k] : (uint8_t)0;
  }
}

template <int MAXB> __device__ __forceinline__ void store_bytes(uint8_t *p, int nb, const uint8_t (&b)[MAXB]) {
  if (MAXB % 4 == 0 && nb == MAXB && ((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < MAXB / 4; k++) ((uint32_t *)p)[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < MAXB; k++) if (k < nb) p[k] = b[k];
  }
}

// One thread's piece of one row of a plane: nel <= NEL elements of BPP bytes at d (and at s in the source), the first NC bytes of each are colour (BPP 4: byte 3 is
// A, which nothing here changes).  cw[i]: element i's colour word (COVERED set) or 0; its bytes from bit `shift` on are the element's.  black: what clear makes of a
// colour byte.  inplace: d is the source.
template <int BPP, int NC, int NEL> __device__ __forceinline__ void put_row(uint8_t *d, const uint8_t *s, int nel, const uint32_t (&cw)[NEL], int shift, bool inplace, bool clear, uint8_t black) {
  if (nel <= 0) return;
  if (inplace && (!clear || BPP > NC)) {      // covered pixels only - or, clearing a format with an A byte in place, every pixel's colour bytes and no other
#pragma unroll
    for (int i = 0; i < NEL; i++) {
      if (i >= nel || !(clear || (cw[i] & COVERED))) continue;
#pragma unroll
      for (int c = 0; c < NC; c++) d[i * BPP + c] = (cw[i] & COVERED) ? (uint8_t)(cw[i] >> (shift + 8 * c)) : black;
    }
    return;
  }
  uint8_t b[NEL * BPP];
  if (!clear || BPP > NC) load_bytes<NEL * BPP>(s, nel * BPP, b);      // (out of place: A travels with its pixel)
#pragma unroll
  for (int i = 0; i < NEL; i++)
#pragma unroll
    for (int c = 0; c < NC; c++) {
      if (cw[i] & COVERED) b[i * BPP + c] = (uint8_t)(cw[i] >> (shift + 8 * c));
      else if (clear) b[i * BPP + c] = black;
    }
  store_bytes<NEL * BPP>(d, nel * BPP, b);
}

template <int FMT> __global__ __launch_bounds__(NT) void k_annotate(AnnotFrame F, const rdk::AnnotRec *recs, int n, int inplace, int clear) {
  __shared__ rdk::AnnotRec s_list[NT];
  __shared__ int s_cnt[NT / 64];
  constexpr bool YUV = is_yuv(FMT);
  const int tid = threadIdx.y * (TW / PXW) + threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, tx1 = min(tx0 + TW, F.iw) - 1, ty1 = min(ty0 + TH, F.ih) - 1;      // the tile, inside the frame
  const int x0 = tx0 + threadIdx.x * PXW, y0 = ty0 + threadIdx.y * PXH;      // this thread's pixels: x0 .. x0 + 3, y0 .. y0 + 1
  uint32_t pix[PXH][PXW], chroma[PXW / 2];
#pragma unroll
  for (int j = 0; j < PXH; j++)
#pragma unroll
    for (int i = 0; i < PXW; i++) pix[j][i] = 0;
#pragma unroll
  for (int i = 0; i < PXW / 2; i++) chroma[i] = 0;

  for (int base = 0; base < n; base += NT) {
    // binning: a thread per primitive of this chunk, the ones whose band can reach the tile into s_list in index order
    const int idx = base + tid;
    rdk::AnnotRec r;
    bool touches = false;
    if (idx < n) { r = recs[idx]; touches = rd_annot_line_touches(&r.L, tx0, ty0, tx1, ty1); }
    const unsigned long long m = __ballot(touches);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) { const int c = s_cnt[w]; off += w < wave ? c : 0; total += c; }
    if (touches) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
    __syncthreads();
    // drawing: every lane asks the same primitive; a later one overwrites an earlier one
    for (int k = 0; k < total; k++) {
      const rd_annot_line Ln = s_list[k].L;
      const uint32_t cw = s_list[k].col | COVERED;
      int64_t erow = rd_annot_line_e(&Ln, x0, y0);
#pragma unroll
      for (int j = 0; j < PXH; j++) {
        int64_t e = erow;
#pragma unroll
        for (int i = 0; i < PXW; i++) {
          if (rd_annot_line_covers_e(&Ln, x0 + i, y0 + j, e)) { pix[j][i] = cw; if (YUV) chroma[i >> 1] = cw; }
          e += Ln.ex;
        }
        erow += Ln.ey;
      }
    }
    __syncthreads();      // (the next chunk overwrites s_cnt and s_list)
  }

  const int npx = min(PXW, F.iw - x0);      // pixels of a row that lie in the frame (<= 0: none)
  if (npx <= 0) return;
  const bool ip = inplace != 0, cl = clear != 0;
  if (!YUV) {
    constexpr int BPP = bpp(FMT);
#pragma unroll
    for (int j = 0; j < PXH; j++)
      if (y0 + j < F.ih)
        put_row<BPP, 3, PXW>(F.dst[0] + (size_t)(y0 + j) * F.dpitch[0] + (size_t)x0 * BPP, F.src[0] + (size_t)(y0 + j) * F.spitch[0] + (size_t)x0 * BPP, npx, pix[j], 0, ip, cl, 0);
  } else {      // (iw and ih are even: a thread's 2 x 2 blocks lie inside the frame or outside as a whole)
    if (y0 >= F.ih) return;
#pragma unroll
    for (int j = 0; j < PXH; j++)
      put_row<1, 1, PXW>(F.dst[0] + (size_t)(y0 + j) * F.dpitch[0] + x0, F.src[0] + (size_t)(y0 + j) * F.spitch[0] + x0, npx, pix[j], 0, ip, cl, 16);
    const int cy = y0 >> 1, cx = x0 >> 1, nc = npx >> 1;
    if (FMT == RD_PIX_NV12) {
      put_row<2, 2, PXW / 2>(F.dst[1] + (size_t)cy * F.dpitch[1] + (size_t)cx * 2, F.src[1] + (size_t)cy * F.spitch[1] + (size_t)cx * 2, nc, chroma, 8, ip, cl, 128);
    } else {
      put_row<1, 1, PXW / 2>(F.dst[1] + (size_t)cy * F.dpitch[1] + cx, F.src[1] + (size_t)cy * F.spitch[1] + cx, nc, chroma, 8, ip, cl, 128);
      put_row<1, 1, PXW / 2>(F.dst[2] + (size_t)cy * F.dpitch[2] + cx, F.src[2] + (size_t)cy * F.spitch[2] + cx, nc, chroma, 16, ip, cl, 128);
    }
  }
}

}  // namespace

namespace rdk {

void annotate(hipStream_t s, int fmt, const PixFrame &dst, const PixFrame &src, const AnnotRec *recs, int n, int clear) {
  if (dst.iw <= 0 || dst.ih <= 0) return;
  const int inplace = dst.pl[0] == src.pl[0];
  if (inplace && !clear && n <= 0) return;      // nothing to write
  const AnnotFrame F = { { dst.pl[0], dst.pl[1], dst.pl[2] }, { src.pl[0], src.pl[1], src.pl[2] }, { dst.pitch[0], dst.pitch[1], dst.pitch[2] },
                         { src.pitch[0], src.pitch[1], src.pitch[2] }, dst.iw, dst.ih };
  const dim3 block(TW / PXW, TH / PXH), grid((F.iw + TW - 1) / TW, (F.ih + TH - 1) / TH);
  if (!dispatch(fmt, [&](auto f) { hipLaunchKernelGGL(k_annotate<f.value>, grid, block, 0, s, F, recs, n, inplace, clear); })) {
    fprintf(stderr, "rdk::annotate: unknown pixel format %d\n", fmt); abort();      // (the entry points refuse it first)
  }
}

}  // namespace rdk
