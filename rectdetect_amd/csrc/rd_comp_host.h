/* rectdetect-mi355x: composited quads - what the host computes once per item (the contract: include/rectdetect_hip.h, "composited quads").  Plain C, no HIP:
 * rd_comp_host.c is built into the library with the host compiler, and tests/native/comp_host_check.c builds it on its own under the sanitizers. */
#ifndef RD_COMP_HOST_H
#define RD_COMP_HOST_H
#include <stdint.h>
#if defined(__cplusplus)
extern "C" {
#endif

enum { RD_COMP_TILE_W = 32, RD_COMP_TILE_H = 16, RD_COMP_CHUNK = 64 };      /* a wave's tile of pixels; items whose boxes the wave tests per ballot */

/* what a job uploads per item: the adjugate A..I, the pixel box bx0, by0, bx1, by1 (empty, and every box of an invalid item: 0, 0, -1, -1), the item's patch
 * (-1: a fill), its colour b, g, r and its status (1 valid, 0 invalid: covers nothing) */
typedef struct { double inv[9]; int32_t box[4]; int32_t patch; uint8_t col[3]; uint8_t status; } rd_comp_rec;      /* 96 bytes */

/* inv, box and status of one quad in an iw x ih frame; patch and col stay as they are */
void rd_comp_make_rec(const double quad[8], int iw, int ih, rd_comp_rec *r);
/* covered <=> the per-pixel test of the contract; st[0], st[1] = s, t (written whenever the box holds the pixel; else 0) */
int rd_comp_rec_covers(const rd_comp_rec *r, int x, int y, double st[2]);
/* The tiles (RD_COMP_TILE_W x RD_COMP_TILE_H pixels, tile (tx, ty) starts at pixel (tx * W, ty * H)) that the boxes of the valid records reach, each once, in raster
 * order: up to max pairs tx, ty into tiles_xy; returns how many there are.  mark: (iw + W - 1) / W * ((ih + H - 1) / H) bytes, all zero on entry and on return. */
int rd_comp_tiles_of(const rd_comp_rec *recs, int n, int iw, int ih, uint8_t *mark, int32_t *tiles_xy, int max);

#if defined(__cplusplus)
}
#endif
#endif
