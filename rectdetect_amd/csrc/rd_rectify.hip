// rectdetect-mi355x: the rectifier - rectified patches of quads behind the detector's poll (the contract: include/rectdetect_hip.h, "rectified patches";
// the kernel: rd_k_rectify.hip).  One non-blocking stream of its own, one event per job in flight; no graphs, no threads, no environment switches.
#include "rd_internal.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAGIC_RECTIFIER 0x52445246u

namespace {

struct Job {
  hipEvent_t done;
  rdk::RectifyQuad *h_quads, *d_quads;      // this job's coefficient blocks: pinned staging and their place in the device array (max_quads each)
  uint8_t *d_out;                           // max_quads patches on their way to pinned host memory (allocated on first use)
  int n;
};

// the planes a format uses, their row bytes and rows; a host frame is packed into the rectifier's buffer with row strides rounded up to 4 bytes
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

// what kind of memory the runtime says p is (hipMemoryTypeUnregistered: pageable, or unknown to it); asked per job - a microsecond - because a caller may free a
// buffer and get pageable memory at the same address
hipMemoryType memory_type(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return hipMemoryTypeUnregistered; }
  return at.type;
}

}  // namespace

struct rd_rectifier {
  uint32_t magic;
  int device, pw, ph, max_quads, njobs;
  size_t patch_bytes;
  hipStream_t st;
  Job *jobs;
  rdk::RectifyQuad *d_quads, *h_quads;      // njobs * max_quads blocks each
  long next_enqueue, next_wait;
  uint8_t *frame; size_t frame_bytes;       // host and pinned frames travel through here (grows on demand; jobs follow one another on st, so one buffer serves them all)
};

namespace rdrt {
int rectifier_device(const rd_rectifier *r) { return r && r->magic == MAGIC_RECTIFIER ? r->device : -1; }
int rectifier_max_quads(const rd_rectifier *r) { return r && r->magic == MAGIC_RECTIFIER ? r->max_quads : -1; }
}

extern "C" {

void rd_rect_quads(const void *rects, int n, double *quads_out) {
  static const int order[4] = { 0, 3, 2, 1 };
  for (int k = 0; k < n; k++) {
    const double *c2 = (const double *)((const char *)rects + (size_t)k * 176);      // rect_t: c2[4] (x, y) first
    for (int i = 0; i < 4; i++) { quads_out[8 * k + 2 * i] = c2[2 * order[i]]; quads_out[8 * k + 2 * i + 1] = c2[2 * order[i] + 1]; }
  }
}

double rd_rect_aspect(const void *rect) {
  const double *c3 = (const double *)((const char *)rect + 64);      // rect_t: c3[4] (x, y, z) behind c2[4]
  double len[2];
  for (int k = 0; k < 2; k++) {
    const double dx = c3[3 * k] - c3[3 * k + 3], dy = c3[3 * k + 1] - c3[3 * k + 4], dz = c3[3 * k + 2] - c3[3 * k + 5];
    len[k] = sqrt((dx * dx + dy * dy) + dz * dz);
  }
  return len[0] / len[1];
}

void rd_rectify_coefficients(const double quad[8], double coef[8], int *status) {
  for (int k = 0; k < 8; k++) coef[k] = 0.0;
  if (status) *status = 0;
  double x[4], y[4];
  for (int k = 0; k < 4; k++) { x[k] = quad[2 * k]; y[k] = quad[2 * k + 1]; if (!isfinite(x[k]) || !isfinite(y[k])) return; }
  int pos = 0, neg = 0;
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) & 3, k = (i + 2) & 3;
    const double cr = (x[j] - x[i]) * (y[k] - y[j]) - (y[j] - y[i]) * (x[k] - x[j]);
    pos += cr > 0.0; neg += cr < 0.0;
  }
  if (pos != 4 && neg != 4) return;
  const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], sx = ((x[0] - x[1]) + x[2]) - x[3];
  const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], sy = ((y[0] - y[1]) + y[2]) - y[3];
  const double den = dx1 * dy2 - dx2 * dy1;
  const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
  const double c[8] = { (x[1] - x[0]) + g * x[1], (x[3] - x[0]) + h * x[3], x[0], (y[1] - y[0]) + g * y[1], (y[3] - y[0]) + h * y[3], y[0], g, h };
  for (int k = 0; k < 8; k++) if (!isfinite(c[k])) return;
  for (int k = 0; k < 8; k++) coef[k] = c[k];
  if (status) *status = 1;
}

rd_rectifier *rd_rectifier_create(int device, int pw, int ph, int max_quads, int njobs) {
  if (pw < 1 || ph < 1 || pw > 16384 || ph > 16384 || max_quads < 1 || max_quads > 65535 || njobs < 1 || njobs > 1024) return NULL;
  if (device < 0 || device >= rd_device_count()) return NULL;
  RD_HIP(hipSetDevice(device));
  rd_rectifier *r = (rd_rectifier *)calloc(1, sizeof(*r));
  r->magic = MAGIC_RECTIFIER;
  r->device = device; r->pw = pw; r->ph = ph; r->max_quads = max_quads; r->njobs = njobs;
  r->patch_bytes = (size_t)pw * ph * 3;
  RD_HIP(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
  const size_t nq = (size_t)njobs * max_quads;
  RD_HIP(hipMalloc((void **)&r->d_quads, nq * sizeof(rdk::RectifyQuad)));
  RD_HIP(hipHostMalloc((void **)&r->h_quads, nq * sizeof(rdk::RectifyQuad), hipHostMallocDefault));
  r->jobs = (Job *)calloc(njobs, sizeof(Job));
  for (int k = 0; k < njobs; k++) {
    RD_HIP(hipEventCreateWithFlags(&r->jobs[k].done, hipEventDisableTiming));
    r->jobs[k].h_quads = r->h_quads + (size_t)k * max_quads;
    r->jobs[k].d_quads = r->d_quads + (size_t)k * max_quads;
  }
  return r;
}

void rd_rectifier_destroy(rd_rectifier *r) {
  if (!r) return;
  if (r->magic != MAGIC_RECTIFIER) exitf(-1, "rd_rectifier_destroy: bad handle\n");
  RD_HIP(hipSetDevice(r->device));
  RD_HIP(hipStreamSynchronize(r->st));
  for (int k = 0; k < r->njobs; k++) { RD_HIP(hipEventDestroy(r->jobs[k].done)); if (r->jobs[k].d_out) RD_HIP(hipFree(r->jobs[k].d_out)); }
  RD_HIP(hipStreamDestroy(r->st));
  RD_HIP(hipFree(r->d_quads));
  RD_HIP(hipHostFree(r->h_quads));
  if (r->frame) RD_HIP(hipFree(r->frame));
  free(r->jobs);
  r->magic = 0;
  free(r);
}

long rd_rectifier_enqueue(rd_rectifier *r, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const double *quads, int n, void *out, int out_kind) {
  if (!r || r->magic != MAGIC_RECTIFIER) exitf(-1, "rd_rectifier_enqueue: bad handle\n");
  // argument errors: -1, nothing enqueued
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches || iw < 1 || ih < 1 || iw > 65536 || ih > 65536) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  if (out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) return -1;
  if (format >= RD_PIX_NV12 && ((iw | ih) & 1)) return -1;
  const Layout L = layout(format, iw, ih);
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  if (n < 0 || n > r->max_quads || (n > 0 && (!quads || !out))) return -1;
  RD_HIP(hipSetDevice(r->device));
  if (n > 0 && memory_type(out) != (out_kind == RD_FRAME_DEVICE ? hipMemoryTypeDevice : hipMemoryTypeHost)) return -1;
  if (r->next_enqueue - r->next_wait >= r->njobs) exitf(-1, "rd_rectifier_enqueue: %d jobs already in flight (wait first)\n", r->njobs);
  Job *j = &r->jobs[r->next_enqueue % r->njobs];
  j->n = n;
  for (int k = 0; k < n; k++) {
    rdk::RectifyQuad *q = &j->h_quads[k];
    q->pad = 0;
    rd_rectify_coefficients(quads + 8 * (size_t)k, q->c, &q->status);
  }
  if (n > 0) {
    const uint8_t *pl[3] = { NULL, NULL, NULL };
    int pitch[3] = { 0, 0, 0 };
    if (on_device == RD_FRAME_DEVICE) {      // read where they lie
      for (int k = 0; k < L.np; k++) { pl[k] = (const uint8_t *)planes[k]; pitch[k] = pitches[k]; }
    } else {      // through the rectifier's own buffer, one plane after the other
      if (on_device == RD_FRAME_HOST_PINNED)
        for (int k = 0; k < L.np; k++)
          if (memory_type(planes[k]) != hipMemoryTypeHost)
            exitf(-1, "rd_rectifier_enqueue: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", k, planes[k]);
      if (r->frame_bytes < L.bytes) {
        RD_HIP(hipStreamSynchronize(r->st));      // (jobs in flight read the old one)
        if (r->frame) RD_HIP(hipFree(r->frame));
        RD_HIP(hipMalloc((void **)&r->frame, L.bytes));
        r->frame_bytes = L.bytes;
      }
      for (int k = 0; k < L.np; k++) {
        RD_HIP(hipMemcpy2DAsync(r->frame + L.off[k], L.pitch[k], planes[k], pitches[k], L.row[k], L.rows[k], hipMemcpyHostToDevice, r->st));
        pl[k] = r->frame + L.off[k]; pitch[k] = L.pitch[k];
      }
      if (on_device == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(r->st));      // (pageable memory: the caller may reuse the buffer when this call returns)
    }
    RD_HIP(hipMemcpyAsync(j->d_quads, j->h_quads, (size_t)n * sizeof(rdk::RectifyQuad), hipMemcpyHostToDevice, r->st));
    uint8_t *dst = (uint8_t *)out;
    const size_t bytes = (size_t)n * r->patch_bytes;
    if (out_kind == RD_FRAME_HOST_PINNED) {
      if (!j->d_out) RD_HIP(hipMalloc((void **)&j->d_out, (size_t)r->max_quads * r->patch_bytes));      // (on first use: a rectifier that writes to device memory only has none)
      dst = j->d_out;
    }
    rdk::rectify(r->st, dst, format, pl, pitch, iw, ih, j->d_quads, n, r->pw, r->ph);
    rdrt::check_launch("rectified patches");
    if (out_kind == RD_FRAME_HOST_PINNED) RD_HIP(hipMemcpyAsync(out, j->d_out, bytes, hipMemcpyDeviceToHost, r->st));
  }
  RD_HIP(hipEventRecord(j->done, r->st));
  return r->next_enqueue++;
}

int rd_rectifier_wait(rd_rectifier *r, uint8_t *status_out) {
  if (!r || r->magic != MAGIC_RECTIFIER) exitf(-1, "rd_rectifier_wait: bad handle\n");
  if (r->next_wait >= r->next_enqueue) return -1;
  RD_HIP(hipSetDevice(r->device));
  Job *j = &r->jobs[r->next_wait % r->njobs];
  RD_HIP(hipEventSynchronize(j->done));
  if (status_out) for (int k = 0; k < j->n; k++) status_out[k] = (uint8_t)j->h_quads[k].status;
  r->next_wait++;
  return j->n;
}

}  // extern "C"
