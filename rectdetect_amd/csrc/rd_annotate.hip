// rectdetect-mi355x: the annotator - rectangles' outlines and line segments drawn into frames behind the detector's poll (the contract: include/rectdetect_hip.h,
// "annotated frames"; the kernel: rd_k_annotate.hip; the coverage test: rd_annot_cover.h; the jobs in flight, the frame's checks and its ways: rd_jobs.h).
#include "rd_jobs.h"
#include "rd_kernels.h"
#include <math.h>
#include <stdio.h>

#define COORD_MIN (-1048576)
#define COORD_MAX 1048575

using namespace rdjob;

namespace {

bool prim_ok(const rd_annot_prim *p) {
  return p->thickness >= 1 && p->x0 >= COORD_MIN && p->x0 <= COORD_MAX && p->y0 >= COORD_MIN && p->y0 <= COORD_MAX &&
         p->x1 >= COORD_MIN && p->x1 <= COORD_MAX && p->y1 >= COORD_MIN && p->y1 <= COORD_MAX;
}

// a coordinate of a rectangle or a segment as cvPoint takes it: truncated toward zero; at scale 2 the source pixel under the detector's (x * 2 + 0.5, the rectifier's
// map).  false: not finite, or outside the legal range
bool coord(double v, int scale, int32_t *out) {
  const double m = scale == 2 ? v * 2.0 + 0.5 : v;
  if (!(m > (double)COORD_MIN - 1.0 && m < (double)COORD_MAX + 1.0)) return false;      // (a NaN fails both)
  *out = (int32_t)m;
  return true;
}

bool make_prim(rd_annot_prim *p, const double a[2], const double b[2], int scale, uint8_t cb, uint8_t cg, uint8_t cr, int thickness) {
  if (!coord(a[0], scale, &p->x0) || !coord(a[1], scale, &p->y0) || !coord(b[0], scale, &p->x1) || !coord(b[1], scale, &p->y1)) return false;
  p->b = cb; p->g = cg; p->r = cr;
  p->thickness = (uint8_t)(thickness > 255 ? 255 : thickness);
  return true;
}

}  // namespace

struct rd_annotator {
  Ring ring;                                // (first: rd_jobs.h)
  rdk::AnnotRec *d_recs, *h_recs;           // njobs blocks of max_prims records each, a job's at slot * max_prims: pinned staging and their place in the device array
  DevBuf frame, oframe;                     // host and pinned frames travel through `frame`, frames on their way to pinned host memory through `oframe`
};

extern "C" {

void rd_annot_limits(int32_t out[4]) {
  out[0] = rdk::ANNOT_TILE_W; out[1] = rdk::ANNOT_TILE_H; out[2] = rdk::ANNOT_CHUNK; out[3] = 0;
}

void rd_annot_yuv(uint8_t b, uint8_t g, uint8_t r, uint8_t yuv[3]) {
  yuv[0] = (uint8_t)rdpix::bgr_y(b, g, r); yuv[1] = (uint8_t)rdpix::bgr_u(b, g, r); yuv[2] = (uint8_t)rdpix::bgr_v(b, g, r);
}

int rd_annot_covers(const rd_annot_prim *p, int x, int y) {
  rd_annot_line L;
  rd_annot_line_setup(&L, p->x0, p->y0, p->x1, p->y1, p->thickness);
  return rd_annot_line_covers(&L, x, y);
}

int rd_annot_touches(const rd_annot_prim *p, int x0, int y0, int x1, int y1) {
  rd_annot_line L;
  rd_annot_line_setup(&L, p->x0, p->y0, p->x1, p->y1, p->thickness);
  return rd_annot_line_touches(&L, x0, y0, x1, y1);
}

int rd_annot_rects(const void *rects, int n, int scale, const uint8_t style[16], rd_annot_prim *out) {
  static const uint8_t vidrect_style[16] = { 0, 255, 0, 1,  0, 200, 255, 2,  255, 0, 0, 1,  0, 0, 255, 2 };
  if (!style) style = vidrect_style;
  if (scale != 1 && scale != 2) return 0;
  int m = 0;
  for (int k = 0; k < n; k++) {
    const char *rec = (const char *)rects + (size_t)k * 176;      // rect_t: c2[4] (x, y) first, status behind c3[4] and value
    const double *c2 = (const double *)rec;
    uint32_t status;
    memcpy(&status, rec + 168, 4);
    if (status > 3) continue;
    const uint8_t *s = style + 4 * status;
    rd_annot_prim p[6];
    bool ok = true;
    for (int i = 0; i < 4 && ok; i++) ok = make_prim(&p[i], c2 + 2 * i, c2 + 2 * ((i + 1) & 3), scale, s[0], s[1], s[2], s[3] * scale);
    ok = ok && make_prim(&p[4], c2, c2 + 4, scale, s[0], s[1], s[2], scale) && make_prim(&p[5], c2 + 2, c2 + 6, scale, s[0], s[1], s[2], scale);
    if (!ok) continue;
    memcpy(out + m, p, sizeof(p));
    m += 6;
  }
  return m;
}

int rd_annot_segments(const void *lslist, int mode, int scale, rd_annot_prim *out, int max) {
  if ((mode != RD_ANNOT_SEG_ALL && mode != RD_ANNOT_SEG_CHAINS) || (scale != 1 && scale != 2) || !lslist) return 0;
  const char *base = (const char *)lslist;      // linesegment_t, 56 bytes: x0 y0 x1 y1 (float) .. leftPtr @24 rightPtr @28 .. polyid @44; record 0: n
  int32_t n;
  memcpy(&n, base, 4);
  int m = 0;
  auto emit = [&](int j, uint8_t cb, uint8_t cg, uint8_t cr) {
    float f[4];
    memcpy(f, base + (size_t)j * 56, 16);
    const double a[2] = { f[0], f[1] }, b[2] = { f[2], f[3] };
    rd_annot_prim p;
    if (!make_prim(&p, a, b, scale, cb, cg, cr, scale)) return;
    if (m < max && out) out[m] = p;
    m++;
  };
  auto field = [&](int j, int at) { int32_t v; memcpy(&v, base + (size_t)j * 56 + at, 4); return v; };
  for (int i = 1; i <= n; i++) {
    if (mode == RD_ANNOT_SEG_ALL) { emit(i, 255, 255, 255); continue; }
    if (field(i, 44) == 0 || field(i, 24) > 0) continue;
    int cnt = 0;
    for (int j = i; j > 0 && j <= n && cnt < n; j = field(j, 28), cnt++) {
      if (cnt & 1) emit(j, 100, 100, 255); else emit(j, 255, 255, 100);
    }
  }
  return m;
}

rd_annotator *rd_annotator_create(int device, int max_prims, int njobs) {
  if (max_prims < 1 || max_prims > (1 << 20) || !ring_args_ok(device, njobs)) return NULL;
  rd_annotator *a = (rd_annotator *)calloc(1, sizeof(*a));
  ring_create(&a->ring, RD_MAGIC_ANNOTATOR, device, max_prims, njobs);
  const size_t nr = (size_t)njobs * max_prims;
  RD_HIP(hipMalloc((void **)&a->d_recs, nr * sizeof(rdk::AnnotRec)));
  RD_HIP(hipHostMalloc((void **)&a->h_recs, nr * sizeof(rdk::AnnotRec), hipHostMallocDefault));
  return a;
}

void rd_annotator_destroy(rd_annotator *a) {
  if (!a) return;
  ring_destroy(ring_of(a, RD_MAGIC_ANNOTATOR, "rd_annotator_destroy"));
  RD_HIP(hipFree(a->d_recs));
  RD_HIP(hipHostFree(a->h_recs));
  a->frame.release();
  a->oframe.release();
  free(a);
}

long rd_annotator_enqueue(rd_annotator *a, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const rd_annot_prim *prims, int n, int flags, void *const out_planes[3], const int out_pitches[3], int out_kind) {
  static const char who[] = "rd_annotator_enqueue";
  Ring *g = ring_of(a, RD_MAGIC_ANNOTATOR, who);
  // argument errors: -1, nothing enqueued
  PixLayout L;
  if (!frame_ok(format, planes, pitches, iw, ih, on_device, &L) || !dest_ok(L, out_planes, out_pitches, out_kind, on_device)) return -1;
  if (flags & ~RD_ANNOT_CLEAR) return -1;
  if (n < 0 || n > g->per_job || (n > 0 && !prims)) return -1;
  for (int k = 0; k < n; k++) if (!prim_ok(&prims[k])) return -1;
  RD_HIP(hipSetDevice(g->device));
  if (!dest_memory_ok(L, out_planes, out_kind)) return -1;
  const int slot = ring_claim(g, who, n);
  rdk::AnnotRec *h_recs = a->h_recs + (size_t)slot * g->per_job, *d_recs = a->d_recs + (size_t)slot * g->per_job;
  for (int k = 0; k < n; k++) {      // the primitives are taken here: the caller may reuse the array when the call returns
    const rd_annot_prim *p = &prims[k];
    rdk::AnnotRec *r = &h_recs[k];
    rd_annot_line_setup(&r->L, p->x0, p->y0, p->x1, p->y1, p->thickness);
    uint8_t c[3] = { p->b, p->g, p->r };
    if (rdpix::rb_swapped(format)) { c[0] = p->r; c[2] = p->b; }
    else if (rdpix::is_yuv(format)) rd_annot_yuv(p->b, p->g, p->r, c);
    r->col = c[0] | (c[1] << 8) | ((uint32_t)c[2] << 16);
    r->pad = 0;
  }
  const bool inplace = out_planes == NULL, to_pinned = !inplace && out_kind == RD_FRAME_HOST_PINNED;
  if (!(inplace && n == 0 && !(flags & RD_ANNOT_CLEAR))) {      // (that job has nothing to write)
    PixFrame src = planes_at(planes, pitches, L);      // a device frame: read where it lies
    if (on_device != RD_FRAME_DEVICE) {              // through the annotator's own buffer, one plane after the other
      a->frame.grow(g->st, L.bytes);
      src = a->frame.packed(L);
      bring(g->st, who, L, src, planes, pitches, on_device);
    }
    PixFrame dst = src;      // in place
    if (to_pinned) { a->oframe.grow(g->st, L.bytes); dst = a->oframe.packed(L); }
    else if (!inplace) dst = planes_at(out_planes, out_pitches, L);
    if (n > 0) RD_HIP(hipMemcpyAsync(d_recs, h_recs, (size_t)n * sizeof(rdk::AnnotRec), hipMemcpyHostToDevice, g->st));
    rdk::annotate(g->st, format, dst, src, d_recs, n, flags & RD_ANNOT_CLEAR);
    rdrt::check_launch("annotated frame");
    if (to_pinned) send(g->st, L, out_planes, out_pitches, dst);
  }
  return ring_record(g);
}

int rd_annotator_wait(rd_annotator *a) {
  Ring *g = ring_of(a, RD_MAGIC_ANNOTATOR, "rd_annotator_wait");
  const int slot = ring_wait(g);
  return slot < 0 ? -1 : g->n[slot];
}

}  // extern "C"
