// rectdetect-mi355x: the rectifier - rectified patches of quads behind the detector's poll (the contract: include/rectdetect_hip.h, "rectified patches";
// the jobs in flight, the frame's checks and its way to the device: rd_jobs.h).  A rectifier is of one kind, and the kind decides a job's launches:
//   PATCHES  rd_k_rectify.hip;
//   TENSOR   rd_k_tensor.hip under the job's own spec ("model-ready tensors");
//   SCAN     rd_k_tensor.hip into a G plane of the rectifier's own, rd_k_scan.hip from there ("scanned pages");
//   GRADE    the same G plane, the job's output zeroed, rd_k_grade.hip ("graded quads");
//   CODE     the same G plane, rd_k_code.hip with the rectifier's dictionary ("decoded quads");
//   BLOBS    the same G plane, its ink bits by rd_k_scan.hip or rd_k_blob.hip's level kernel, rd_k_blob.hip's component stage ("page components").
#include "rd_jobs.h"
#include "rd_kernels.h"
#include "rd_code_tile.h"
#include "rd_blob_tile.h"
#include <math.h>
#include <stdio.h>

using namespace rdjob;

enum Kind { PATCHES, TENSOR, SCAN, GRADE, CODE, BLOBS };      // which rd_rectifier_create* made it

static bool has_records(Kind k) { return k == GRADE || k == CODE || k == BLOBS; }      // `out` is 8-byte aligned (the records' 64-bit sums; rd_code::bits)

struct SlotScratch {                        // a job slot's scratch in device memory, every member allocated on first use (scratch())
  uint8_t *out;                             // max_quads outputs on their way to pinned host memory (a rectifier that writes to device memory only has none)
  uint8_t *plane;                           // the G planes of max_quads quads, pw * ph bytes each, RD_CODE_PLANE_PAD more for CODE (kinds with a G plane only)
  int *labels, *areas;                      // the component stage's two int planes of max_quads quads, pw * ph ints each (BLOBS only)
};

struct rd_rectifier {
  Ring ring;                                // (first: rd_jobs.h)
  Kind kind;
  int pw, ph;
  size_t patch_bytes;                       // of one quad's output: pw * ph * 3, or rd_tensor_bytes / rd_scan_bytes / rd_grade_bytes / rd_code_bytes / rd_blob_bytes of the spec
  rd_tensor_spec spec;                      // TENSOR: the job's own; kinds with a G plane: { U8, NHWC, GRAY, m }
  rd_scan_spec sspec;                       // SCAN: the job's own; BLOBS: the ink decision of bspec as RD_SCAN_BITS (radius >= 1)
  rd_grade_spec gspec;                      // GRADE
  rd_code_spec cspec;                       // CODE: a record per quad from the ndict codes at d_dict
  uint64_t *d_dict;                         // (NULL when ndict is 0)
  int ndict;
  rd_blob_spec bspec;                       // BLOBS
  rdk::RectifyQuad *d_quads, *h_quads;      // njobs blocks of max_quads each, a job's at slot * max_quads: pinned staging and their place in the device array
  SlotScratch *slots;                       // one per job slot
  DevBuf frame;                             // host and pinned frames travel through here
};

// a member of a slot's scratch: allocated on first use
template <class T> static T *scratch(T **member, size_t bytes) {
  if (!*member) RD_HIP(hipMalloc((void **)member, bytes));
  return *member;
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

// whether rd_rectifier_create* makes a rectifier of these: decided before anything is allocated
static bool create_args_ok(int device, int pw, int ph, int max_quads, int njobs, Kind kind, const void *spec, const uint64_t *dict, int ndict) {
  if (pw < 1 || ph < 1 || pw > 16384 || ph > 16384 || max_quads < 1 || max_quads > 65535 || !ring_args_ok(device, njobs)) return false;
  if (kind != PATCHES && !spec) return false;
  switch (kind) {
    case PATCHES: return true;
    case TENSOR: return rd_tensor_spec_ok((const rd_tensor_spec *)spec, pw, ph);
    case SCAN: return rd_scan_spec_ok((const rd_scan_spec *)spec, pw, ph);
    case GRADE: return rd_grade_spec_ok((const rd_grade_spec *)spec, pw, ph);
    case BLOBS: return rd_blob_spec_ok((const rd_blob_spec *)spec, pw, ph) && (size_t)max_quads * pw * ph <= RD_BLOB_MAX_SLOT_PIXELS;
    case CODE: {
      const rd_code_spec *c = (const rd_code_spec *)spec;
      if (!rd_code_spec_ok(c, pw, ph) || ndict < 0 || ndict > RD_CODE_MAX_DICT || (ndict > 0 && !dict)) return false;
      const int bits = c->n * c->n;
      for (int k = 0; k < ndict; k++) if (bits < 64 && (dict[k] >> bits)) return false;      // (a bit at or above n * n)
      return true;
    }
  }
  return false;
}

// the G plane's spec: step 1 of SCAN, GRADE, CODE and BLOBS IS this tensor
static void gray_plane(rd_rectifier *r, int oversample) {
  r->spec.dtype = RD_TENSOR_U8; r->spec.layout = RD_TENSOR_NHWC; r->spec.channels = RD_TENSOR_GRAY; r->spec.oversample = oversample;
}

// every kind's constructor: `spec` is the kind's own rd_*_spec (PATCHES: none), dict / ndict CODE's dictionary
static rd_rectifier *rectifier_create(int device, int pw, int ph, int max_quads, int njobs, Kind kind, const void *spec, const uint64_t *dict, int ndict) {
  if (!create_args_ok(device, pw, ph, max_quads, njobs, kind, spec, dict, ndict)) return NULL;
  rd_rectifier *r = (rd_rectifier *)calloc(1, sizeof(*r));
  ring_create(&r->ring, RD_MAGIC_RECTIFIER, device, max_quads, njobs);
  r->kind = kind; r->pw = pw; r->ph = ph;
  switch (kind) {
    case PATCHES: r->patch_bytes = (size_t)pw * ph * 3; break;
    case TENSOR: r->spec = *(const rd_tensor_spec *)spec; r->patch_bytes = rd_tensor_bytes(&r->spec, pw, ph); break;
    case SCAN: r->sspec = *(const rd_scan_spec *)spec; r->patch_bytes = rd_scan_bytes(&r->sspec, pw, ph); gray_plane(r, r->sspec.oversample); break;
    case GRADE: r->gspec = *(const rd_grade_spec *)spec; r->patch_bytes = rd_grade_bytes(&r->gspec, pw, ph); gray_plane(r, r->gspec.oversample); break;
    case CODE:
      r->cspec = *(const rd_code_spec *)spec; r->patch_bytes = rd_code_bytes(&r->cspec, pw, ph); gray_plane(r, r->cspec.oversample);
      r->ndict = ndict;
      if (ndict > 0) {
        RD_HIP(hipMalloc((void **)&r->d_dict, (size_t)ndict * sizeof(uint64_t)));
        RD_HIP(hipMemcpy(r->d_dict, dict, (size_t)ndict * sizeof(uint64_t), hipMemcpyHostToDevice));
      }
      break;
    case BLOBS: {
      r->bspec = *(const rd_blob_spec *)spec; r->patch_bytes = rd_blob_bytes(&r->bspec, pw, ph); gray_plane(r, r->bspec.oversample);
      const rd_scan_spec ink = { RD_SCAN_BITS, r->bspec.radius, r->bspec.k, r->bspec.d, 255, r->bspec.oversample, r->bspec.invert, 0 };      // (white: not read in this mode; radius 0 never reaches rdk::scan)
      r->sspec = ink;
      break;
    }
  }
  const size_t nq = (size_t)njobs * max_quads;
  RD_HIP(hipMalloc((void **)&r->d_quads, nq * sizeof(rdk::RectifyQuad)));
  RD_HIP(hipHostMalloc((void **)&r->h_quads, nq * sizeof(rdk::RectifyQuad), hipHostMallocDefault));
  r->slots = (SlotScratch *)calloc(njobs, sizeof(SlotScratch));
  return r;
}

// the kinds without a dictionary
static rd_rectifier *rectifier_create(int device, int pw, int ph, int max_quads, int njobs, Kind kind, const void *spec) {
  return rectifier_create(device, pw, ph, max_quads, njobs, kind, spec, NULL, 0);
}

rd_rectifier *rd_rectifier_create(int device, int pw, int ph, int max_quads, int njobs) { return rectifier_create(device, pw, ph, max_quads, njobs, PATCHES, NULL); }

rd_rectifier *rd_rectifier_create_tensor(int device, int pw, int ph, int max_quads, int njobs, const rd_tensor_spec *spec) {
  return rectifier_create(device, pw, ph, max_quads, njobs, TENSOR, spec);
}

rd_rectifier *rd_rectifier_create_scan(int device, int pw, int ph, int max_quads, int njobs, const rd_scan_spec *spec) {
  return rectifier_create(device, pw, ph, max_quads, njobs, SCAN, spec);
}

rd_rectifier *rd_rectifier_create_grade(int device, int pw, int ph, int max_quads, int njobs, const rd_grade_spec *spec) {
  return rectifier_create(device, pw, ph, max_quads, njobs, GRADE, spec);
}

rd_rectifier *rd_rectifier_create_code(int device, int pw, int ph, int max_quads, int njobs, const rd_code_spec *spec, const uint64_t *dict, int ndict) {
  return rectifier_create(device, pw, ph, max_quads, njobs, CODE, spec, dict, ndict);
}

rd_rectifier *rd_rectifier_create_blobs(int device, int pw, int ph, int max_quads, int njobs, const rd_blob_spec *spec) {
  return rectifier_create(device, pw, ph, max_quads, njobs, BLOBS, spec);
}

int rd_blobs_pages_device(int device, const uint8_t *bits, int pw, int ph, int n, const rd_blob_spec *spec, void *out, int32_t info[8]) {
  if (!bits || !spec || !out || !info || n < 1 || n > 65535 || !rd_blob_spec_ok(spec, pw, ph) || (size_t)n * pw * ph > RD_BLOB_MAX_SLOT_PIXELS) return -1;
  RD_HIP(hipSetDevice(device));
  const size_t npix = (size_t)n * pw * ph, page_bytes = (size_t)((pw + 7) >> 3) * ph, bytes = (size_t)n * rd_blob_bytes(spec, pw, ph);
  int *d_labels = NULL, *d_areas = NULL;
  uint8_t *d_out = NULL;
  hipStream_t st = NULL;
  RD_HIP(hipMalloc((void **)&d_labels, npix * sizeof(int)));
  RD_HIP(hipMalloc((void **)&d_areas, npix * sizeof(int)));
  RD_HIP(hipMalloc((void **)&d_out, bytes));
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemcpyAsync(d_areas, bits, n * page_bytes, hipMemcpyHostToDevice, st));      // (where a job's ink decision puts them)
  rdk::blobs(st, d_out, d_labels, d_areas, NULL, n, pw, ph, *spec, info);
  rdrt::check_launch("rd_blobs_pages_device");
  RD_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  RD_HIP(hipStreamDestroy(st));
  RD_HIP(hipFree(d_out)); RD_HIP(hipFree(d_areas)); RD_HIP(hipFree(d_labels));
  return 0;
}

size_t rd_rectifier_patch_bytes(const rd_rectifier *r) { return r ? r->patch_bytes : 0; }

void rd_rectifier_destroy(rd_rectifier *r) {
  if (!r) return;
  Ring *g = ring_of(r, RD_MAGIC_RECTIFIER, "rd_rectifier_destroy");
  const int njobs = g->njobs;
  ring_destroy(g);
  for (int k = 0; k < njobs; k++) {
    void *const members[4] = { r->slots[k].out, r->slots[k].plane, r->slots[k].labels, r->slots[k].areas };
    for (void *m : members) if (m) RD_HIP(hipFree(m));
  }
  if (r->d_dict) RD_HIP(hipFree(r->d_dict));
  RD_HIP(hipFree(r->d_quads));
  RD_HIP(hipHostFree(r->h_quads));
  r->frame.release();
  free(r->slots);
  free(r);
}

long rd_rectifier_enqueue(rd_rectifier *r, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const double *quads, int n, void *out, int out_kind) {
  static const char who[] = "rd_rectifier_enqueue";
  Ring *g = ring_of(r, RD_MAGIC_RECTIFIER, who);
  // argument errors: -1, nothing enqueued
  PixLayout L;
  if (!frame_ok(format, planes, pitches, iw, ih, on_device, &L)) return -1;
  if (out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) return -1;
  if (n < 0 || n > g->per_job || (n > 0 && (!quads || !out))) return -1;
  RD_HIP(hipSetDevice(g->device));
  if (n > 0 && !is_kind(out, out_kind)) return -1;
  if (n > 0 && has_records(r->kind) && ((uintptr_t)out & 7)) return -1;
  const int slot = ring_claim(g, who, n);
  rdk::RectifyQuad *h_quads = r->h_quads + (size_t)slot * g->per_job, *d_quads = r->d_quads + (size_t)slot * g->per_job;
  for (int k = 0; k < n; k++) {
    rdk::RectifyQuad *q = &h_quads[k];
    q->pad = 0;
    rd_rectify_coefficients(quads + 8 * (size_t)k, q->c, &q->status);
  }
  if (n > 0) {      // (an empty job touches no frame)
    PixFrame src = planes_at(planes, pitches, L);      // a device frame: read where it lies
    if (on_device != RD_FRAME_DEVICE) {              // through the rectifier's own buffer, one plane after the other
      r->frame.grow(g->st, L.bytes);
      src = r->frame.packed(L);
      bring(g->st, who, L, src, planes, pitches, on_device);
    }
    RD_HIP(hipMemcpyAsync(d_quads, h_quads, (size_t)n * sizeof(rdk::RectifyQuad), hipMemcpyHostToDevice, g->st));
    SlotScratch *s = &r->slots[slot];
    const int pw = r->pw, ph = r->ph;
    const size_t npix = (size_t)g->per_job * pw * ph;
    const size_t plane_bytes = npix + (r->kind == CODE ? RD_CODE_PLANE_PAD : 0);      // (rdk::code reads whole 16-byte words, and is told how far it may)
    uint8_t *dst = out_kind == RD_FRAME_HOST_PINNED ? scratch(&s->out, (size_t)g->per_job * r->patch_bytes) : (uint8_t *)out;
    auto g_plane = [&](const char *what) {      // step 1 of the kinds that have a G plane: the job's quads as { U8, NHWC, GRAY, m } tensors in the slot's own planes
      uint8_t *plane = scratch(&s->plane, plane_bytes);
      rdk::rectify_tensor(g->st, plane, format, src, d_quads, n, pw, ph, r->spec);
      rdrt::check_launch(what);
      return plane;
    };
    switch (r->kind) {
      case PATCHES:
        rdk::rectify(g->st, dst, format, src, d_quads, n, pw, ph);
        break;
      case TENSOR:
        rdk::rectify_tensor(g->st, dst, format, src, d_quads, n, pw, ph, r->spec);
        break;
      case SCAN: {
        const uint8_t *plane = g_plane("scanned pages: the G plane");
        rdk::scan(g->st, dst, plane, d_quads, n, pw, ph, r->sspec);
        break;
      }
      case GRADE: {
        const uint8_t *plane = g_plane("graded quads: the G plane");
        RD_HIP(hipMemsetAsync(dst, 0, (size_t)n * r->patch_bytes, g->st));      // the kernel ADDS to the records; an invalid quad's stay as they are here
        rdk::grade(g->st, dst, plane, d_quads, n, pw, ph, r->gspec);
        break;
      }
      case CODE: {
        const uint8_t *plane = g_plane("decoded quads: the G plane");
        rdk::code(g->st, dst, plane, plane_bytes, d_quads, n, pw, ph, r->cspec, r->d_dict, r->ndict);
        break;
      }
      case BLOBS: {
        const uint8_t *plane = g_plane("page components: the G plane");
        int *labels = scratch(&s->labels, npix * sizeof(int)), *areas = scratch(&s->areas, npix * sizeof(int));
        uint8_t *bits = (uint8_t *)areas;      // (rd_k_blob.hip: the bits lie at the start of the area plane until the tile kernel has read them)
        if (r->bspec.radius > 0) rdk::scan(g->st, bits, plane, d_quads, n, pw, ph, r->sspec);
        else rdk::blob_level(g->st, bits, plane, d_quads, n, pw, ph, r->bspec);
        rdrt::check_launch("page components: the ink bits");
        rdk::blobs(g->st, dst, labels, areas, d_quads, n, pw, ph, r->bspec, NULL);
        break;
      }
    }
    rdrt::check_launch("rectified patches");
    if (out_kind == RD_FRAME_HOST_PINNED) RD_HIP(hipMemcpyAsync(out, dst, (size_t)n * r->patch_bytes, hipMemcpyDeviceToHost, g->st));
  }
  return ring_record(g);
}

int rd_rectifier_wait(rd_rectifier *r, uint8_t *status_out) {
  Ring *g = ring_of(r, RD_MAGIC_RECTIFIER, "rd_rectifier_wait");
  const int slot = ring_wait(g);
  if (slot < 0) return -1;
  const rdk::RectifyQuad *h_quads = r->h_quads + (size_t)slot * g->per_job;
  if (status_out) for (int k = 0; k < g->n[slot]; k++) status_out[k] = (uint8_t)h_quads[k].status;
  return g->n[slot];
}

}  // extern "C"
