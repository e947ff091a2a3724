// rectdetect-mi355x: the annotator - rectangles' outlines and line segments drawn into frames behind the detector's poll (the contract: include/rectdetect_hip.h,
// "annotated frames"; the kernel: rd_k_annotate.hip; the coverage test: rd_annot_cover.h).  Built like the rectifier (rd_rectify.hip): one non-blocking stream of
// its own, one event per job in flight; no graphs, no threads, no environment switches.
#include "rd_internal.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAGIC_ANNOTATOR 0x5244414eu
#define COORD_MIN (-1048576)
#define COORD_MAX 1048575

namespace {

struct Job {
  hipEvent_t done;
  rdk::AnnotRec *h_recs, *d_recs;      // this job's records: pinned staging and their place in the device array (max_prims each)
  int n;
};

// the planes a format uses, their row bytes and rows; a frame in one of the annotator's own buffers is packed with row strides rounded up to 4 bytes
struct Layout { int np, row[3], rows[3], pitch[3]; size_t off[3], bytes; };
Layout layout(int fmt, int iw, int ih) {
  Layout L;
  memset(&L, 0, sizeof(L));
  const int bpp = fmt == RD_PIX_BGR || fmt == RD_PIX_RGB ? 3 : 4;
  if (fmt <= RD_PIX_RGBA) { L.np = 1; L.row[0] = iw * bpp; L.rows[0] = ih; }
  else if (fmt == RD_PIX_NV12) { L.np = 2; L.row[0] = L.row[1] = iw; L.rows[0] = ih; L.rows[1] = ih / 2; }
  else { L.np = 3; L.row[0] = iw; L.rows[0] = ih; L.row[1] = L.row[2] = iw / 2; L.rows[1] = L.rows[2] = ih / 2; }
  for (int k = 0; k < L.np; k++) { L.pitch[k] = (L.row[k] + 3) & ~3; L.off[k] = L.bytes; L.bytes += (size_t)L.pitch[k] * L.rows[k]; }
  return L;
}

hipMemoryType memory_type(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return hipMemoryTypeUnregistered; }
  return at.type;
}

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

void ensure(uint8_t **buf, size_t *have, size_t want, hipStream_t st) {
  if (*have >= want) return;
  RD_HIP(hipStreamSynchronize(st));      // (jobs in flight use the old one)
  if (*buf) RD_HIP(hipFree(*buf));
  RD_HIP(hipMalloc((void **)buf, want));
  *have = want;
}

}  // namespace

struct rd_annotator {
  uint32_t magic;
  int device, max_prims, njobs;
  hipStream_t st;
  Job *jobs;
  rdk::AnnotRec *d_recs, *h_recs;           // njobs * max_prims records each
  long next_enqueue, next_wait;
  // host and pinned frames travel through `frame`, frames on their way to pinned host memory through `oframe` (both grow on demand; jobs follow one another on
  // st, so one buffer of each serves them all)
  uint8_t *frame, *oframe; size_t frame_bytes, oframe_bytes;
};

namespace rdrt {
int annotator_device(const rd_annotator *a) { return a && a->magic == MAGIC_ANNOTATOR ? a->device : -1; }
}

extern "C" {

void rd_annot_limits(int32_t out[4]) {
  out[0] = rdk::ANNOT_TILE_W; out[1] = rdk::ANNOT_TILE_H; out[2] = rdk::ANNOT_CHUNK; out[3] = 0;
}

void rd_annot_yuv(uint8_t b, uint8_t g, uint8_t r, uint8_t yuv[3]) {
  const int B = b, G = g, R = r;
  yuv[0] = (uint8_t)(((66 * R + 129 * G + 25 * B + 128) >> 8) + 16);
  yuv[1] = (uint8_t)(((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128);
  yuv[2] = (uint8_t)(((112 * R - 94 * G - 18 * B + 128) >> 8) + 128);
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
  if (max_prims < 1 || max_prims > (1 << 20) || njobs < 1 || njobs > 1024) return NULL;
  if (device < 0 || device >= rd_device_count()) return NULL;
  RD_HIP(hipSetDevice(device));
  rd_annotator *a = (rd_annotator *)calloc(1, sizeof(*a));
  a->magic = MAGIC_ANNOTATOR;
  a->device = device; a->max_prims = max_prims; a->njobs = njobs;
  RD_HIP(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking));
  const size_t nr = (size_t)njobs * max_prims;
  RD_HIP(hipMalloc((void **)&a->d_recs, nr * sizeof(rdk::AnnotRec)));
  RD_HIP(hipHostMalloc((void **)&a->h_recs, nr * sizeof(rdk::AnnotRec), hipHostMallocDefault));
  a->jobs = (Job *)calloc(njobs, sizeof(Job));
  for (int k = 0; k < njobs; k++) {
    RD_HIP(hipEventCreateWithFlags(&a->jobs[k].done, hipEventDisableTiming));
    a->jobs[k].h_recs = a->h_recs + (size_t)k * max_prims;
    a->jobs[k].d_recs = a->d_recs + (size_t)k * max_prims;
  }
  return a;
}

void rd_annotator_destroy(rd_annotator *a) {
  if (!a) return;
  if (a->magic != MAGIC_ANNOTATOR) exitf(-1, "rd_annotator_destroy: bad handle\n");
  RD_HIP(hipSetDevice(a->device));
  RD_HIP(hipStreamSynchronize(a->st));
  for (int k = 0; k < a->njobs; k++) RD_HIP(hipEventDestroy(a->jobs[k].done));
  RD_HIP(hipStreamDestroy(a->st));
  RD_HIP(hipFree(a->d_recs));
  RD_HIP(hipHostFree(a->h_recs));
  if (a->frame) RD_HIP(hipFree(a->frame));
  if (a->oframe) RD_HIP(hipFree(a->oframe));
  free(a->jobs);
  a->magic = 0;
  free(a);
}

long rd_annotator_enqueue(rd_annotator *a, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const rd_annot_prim *prims, int n, int flags, void *const out_planes[3], const int out_pitches[3], int out_kind) {
  if (!a || a->magic != MAGIC_ANNOTATOR) exitf(-1, "rd_annotator_enqueue: bad handle\n");
  // argument errors: -1, nothing enqueued
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches || iw < 1 || ih < 1 || iw > 65536 || ih > 65536) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  if (flags & ~RD_ANNOT_CLEAR) return -1;
  if (format >= RD_PIX_NV12 && ((iw | ih) & 1)) return -1;
  const Layout L = layout(format, iw, ih);
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  const bool inplace = out_planes == NULL;
  if (inplace) {
    if (on_device != RD_FRAME_DEVICE) return -1;
  } else {
    if ((out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) || !out_pitches) return -1;
    for (int k = 0; k < L.np; k++) if (!out_planes[k] || out_pitches[k] < L.row[k]) return -1;
  }
  if (n < 0 || n > a->max_prims || (n > 0 && !prims)) return -1;
  for (int k = 0; k < n; k++) if (!prim_ok(&prims[k])) return -1;
  RD_HIP(hipSetDevice(a->device));
  if (!inplace)
    for (int k = 0; k < L.np; k++)
      if (memory_type(out_planes[k]) != (out_kind == RD_FRAME_DEVICE ? hipMemoryTypeDevice : hipMemoryTypeHost)) return -1;
  if (a->next_enqueue - a->next_wait >= a->njobs) exitf(-1, "rd_annotator_enqueue: %d jobs already in flight (wait first)\n", a->njobs);
  Job *j = &a->jobs[a->next_enqueue % a->njobs];
  j->n = n;
  for (int k = 0; k < n; k++) {      // the primitives are taken here: the caller may reuse the array when the call returns
    const rd_annot_prim *p = &prims[k];
    rdk::AnnotRec *r = &j->h_recs[k];
    rd_annot_line_setup(&r->L, p->x0, p->y0, p->x1, p->y1, p->thickness);
    uint8_t c[3] = { p->b, p->g, p->r };
    if (format == RD_PIX_RGB || format == RD_PIX_RGBA) { c[0] = p->r; c[2] = p->b; }
    else if (format >= RD_PIX_NV12) rd_annot_yuv(p->b, p->g, p->r, c);
    r->col = c[0] | (c[1] << 8) | ((uint32_t)c[2] << 16);
    r->pad = 0;
  }
  if (!(inplace && n == 0 && !(flags & RD_ANNOT_CLEAR))) {      // (that job has nothing to write)
    const uint8_t *src[3] = { NULL, NULL, NULL };
    uint8_t *dst[3] = { NULL, NULL, NULL };
    int spitch[3] = { 0, 0, 0 }, dpitch[3] = { 0, 0, 0 };
    if (on_device == RD_FRAME_DEVICE) {      // read where they lie
      for (int k = 0; k < L.np; k++) { src[k] = (const uint8_t *)planes[k]; spitch[k] = pitches[k]; }
    } else {      // through the annotator's own buffer, one plane after the other
      if (on_device == RD_FRAME_HOST_PINNED)
        for (int k = 0; k < L.np; k++)
          if (memory_type(planes[k]) != hipMemoryTypeHost)
            exitf(-1, "rd_annotator_enqueue: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", k, planes[k]);
      ensure(&a->frame, &a->frame_bytes, L.bytes, a->st);
      for (int k = 0; k < L.np; k++) {
        RD_HIP(hipMemcpy2DAsync(a->frame + L.off[k], L.pitch[k], planes[k], pitches[k], L.row[k], L.rows[k], hipMemcpyHostToDevice, a->st));
        src[k] = a->frame + L.off[k]; spitch[k] = L.pitch[k];
      }
      if (on_device == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(a->st));      // (pageable memory: the caller may reuse the buffer when this call returns)
    }
    if (inplace) {
      for (int k = 0; k < L.np; k++) { dst[k] = (uint8_t *)planes[k]; dpitch[k] = pitches[k]; }
    } else if (out_kind == RD_FRAME_DEVICE) {
      for (int k = 0; k < L.np; k++) { dst[k] = (uint8_t *)out_planes[k]; dpitch[k] = out_pitches[k]; }
    } else {
      ensure(&a->oframe, &a->oframe_bytes, L.bytes, a->st);
      for (int k = 0; k < L.np; k++) { dst[k] = a->oframe + L.off[k]; dpitch[k] = L.pitch[k]; }
    }
    if (n > 0) RD_HIP(hipMemcpyAsync(j->d_recs, j->h_recs, (size_t)n * sizeof(rdk::AnnotRec), hipMemcpyHostToDevice, a->st));
    rdk::annotate(a->st, format, dst, dpitch, src, spitch, iw, ih, j->d_recs, n, flags & RD_ANNOT_CLEAR);
    rdrt::check_launch("annotated frame");
    if (!inplace && out_kind == RD_FRAME_HOST_PINNED)
      for (int k = 0; k < L.np; k++)      // row bytes only: the caller's pitch padding stays as it is
        RD_HIP(hipMemcpy2DAsync(out_planes[k], out_pitches[k], dst[k], dpitch[k], L.row[k], L.rows[k], hipMemcpyDeviceToHost, a->st));
  }
  RD_HIP(hipEventRecord(j->done, a->st));
  return a->next_enqueue++;
}

int rd_annotator_wait(rd_annotator *a) {
  if (!a || a->magic != MAGIC_ANNOTATOR) exitf(-1, "rd_annotator_wait: bad handle\n");
  if (a->next_wait >= a->next_enqueue) return -1;
  RD_HIP(hipSetDevice(a->device));
  Job *j = &a->jobs[a->next_wait % a->njobs];
  RD_HIP(hipEventSynchronize(j->done));
  a->next_wait++;
  return j->n;
}

}  // extern "C"
