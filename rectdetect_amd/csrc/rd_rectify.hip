// rectdetect-mi355x: the rectifier - rectified patches of quads behind the detector's poll (the contract: include/rectdetect_hip.h, "rectified patches";
// the kernels: rd_k_rectify.hip and, for a rectifier made with a tensor spec, rd_k_tensor.hip ("model-ready tensors"); made with a scan spec, rd_k_tensor.hip into a
// G plane of the rectifier's own and rd_k_scan.hip from there ("scanned pages"); made with a grade spec, the same G plane and rd_k_grade.hip ("graded quads"); made with a code spec and a dictionary, the same G plane and rd_k_code.hip ("decoded quads"); made with a blob spec, the same G plane, its ink bits by rd_k_scan.hip or rd_k_blob.hip's level kernel and rd_k_blob.hip's component stage ("page components"); the jobs in flight, the frame's checks and its way to the device: rd_jobs.h).
#include "rd_jobs.h"
#include "rd_kernels.h"
#include "rd_code_tile.h"
#include "rd_blob_tile.h"
#include <math.h>
#include <stdio.h>

using namespace rdjob;

struct rd_rectifier {
  Ring ring;                                // (first: rd_jobs.h)
  int pw, ph;
  size_t patch_bytes;                       // of one quad's output: pw * ph * 3, or rd_tensor_bytes / rd_scan_bytes / rd_grade_bytes / rd_code_bytes / rd_blob_bytes of the spec
  int tensor;                               // made by rd_rectifier_create_tensor: jobs launch rdk::rectify_tensor with `spec`
  rd_tensor_spec spec;
  int scan;                                 // made by rd_rectifier_create_scan: jobs launch rdk::rectify_tensor with `spec` ({ U8, NHWC, GRAY, m }) into d_plane, then rdk::scan with `sspec`
  rd_scan_spec sspec;
  int grade;                                // made by rd_rectifier_create_grade: the same G plane, then the stream zeroes the job's output and rdk::grade adds to it under `gspec`
  rd_grade_spec gspec;
  int code;                                 // made by rd_rectifier_create_code: the same G plane, then rdk::code writes a record per quad under `cspec` from the ndict codes at d_dict
  rd_code_spec cspec;
  uint64_t *d_dict;                         // (NULL when ndict is 0)
  int ndict;
  int blob;                                 // made by rd_rectifier_create_blobs: the same G plane, then the ink bits - rdk::scan with `sspec` (RD_SCAN_BITS; radius >= 1) or rdk::blob_level - into the start of d_areas, then rdk::blobs under `bspec`
  rd_blob_spec bspec;
  int **d_labels, **d_areas;                // per slot: the component stage's two int planes of max_quads quads, pw * ph ints each (allocated on first use; blob rectifiers only)
  uint8_t **d_plane;                        // per slot: the G planes of max_quads quads, pw * ph bytes each (allocated on first use; scan, grade, code and blob rectifiers only)
  rdk::RectifyQuad *d_quads, *h_quads;      // njobs blocks of max_quads each, a job's at slot * max_quads: pinned staging and their place in the device array
  uint8_t **d_out;                          // per slot: max_quads patches on their way to pinned host memory (allocated on first use)
  DevBuf frame;                             // host and pinned frames travel through here
};

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

// the G plane's spec: step 1 of "scanned pages" and of "graded quads" IS this tensor
static void gray_plane(rd_rectifier *r, int njobs, int oversample) {
  r->spec.dtype = RD_TENSOR_U8; r->spec.layout = RD_TENSOR_NHWC; r->spec.channels = RD_TENSOR_GRAY; r->spec.oversample = oversample;
  r->d_plane = (uint8_t **)calloc(njobs, sizeof(uint8_t *));
}

// spec == NULL, sspec == NULL, gspec == NULL, cspec == NULL and bspec == NULL: the classic rectifier
static rd_rectifier *rectifier_create(int device, int pw, int ph, int max_quads, int njobs, const rd_tensor_spec *spec, const rd_scan_spec *sspec = NULL, const rd_grade_spec *gspec = NULL,
                                      const rd_code_spec *cspec = NULL, const uint64_t *dict = NULL, int ndict = 0, const rd_blob_spec *bspec = NULL) {
  if (pw < 1 || ph < 1 || pw > 16384 || ph > 16384 || max_quads < 1 || max_quads > 65535 || !ring_args_ok(device, njobs)) return NULL;
  if (spec && !rd_tensor_spec_ok(spec, pw, ph)) return NULL;
  if (sspec && !rd_scan_spec_ok(sspec, pw, ph)) return NULL;
  if (gspec && !rd_grade_spec_ok(gspec, pw, ph)) return NULL;
  if (bspec && (!rd_blob_spec_ok(bspec, pw, ph) || (size_t)max_quads * pw * ph > RD_BLOB_MAX_SLOT_PIXELS)) return NULL;
  if (cspec) {
    if (!rd_code_spec_ok(cspec, pw, ph) || ndict < 0 || ndict > RD_CODE_MAX_DICT || (ndict > 0 && !dict)) return NULL;
    const int bits = cspec->n * cspec->n;
    for (int k = 0; k < ndict; k++) if (bits < 64 && (dict[k] >> bits)) return NULL;      // (a bit at or above n * n)
  }
  rd_rectifier *r = (rd_rectifier *)calloc(1, sizeof(*r));
  ring_create(&r->ring, RD_MAGIC_RECTIFIER, device, max_quads, njobs);
  r->pw = pw; r->ph = ph;
  r->patch_bytes = spec ? rd_tensor_bytes(spec, pw, ph) : (size_t)pw * ph * 3;
  if (spec) { r->tensor = 1; r->spec = *spec; }
  if (sspec) {
    r->scan = 1; r->sspec = *sspec;
    r->patch_bytes = rd_scan_bytes(sspec, pw, ph);
    gray_plane(r, njobs, sspec->oversample);
  }
  if (gspec) {
    r->grade = 1; r->gspec = *gspec;
    r->patch_bytes = rd_grade_bytes(gspec, pw, ph);
    gray_plane(r, njobs, gspec->oversample);
  }
  if (cspec) {
    r->code = 1; r->cspec = *cspec; r->ndict = ndict;
    r->patch_bytes = rd_code_bytes(cspec, pw, ph);
    gray_plane(r, njobs, cspec->oversample);
    if (ndict > 0) {
      RD_HIP(hipMalloc((void **)&r->d_dict, (size_t)ndict * sizeof(uint64_t)));
      RD_HIP(hipMemcpy(r->d_dict, dict, (size_t)ndict * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
  }
  if (bspec) {
    r->blob = 1; r->bspec = *bspec;
    r->patch_bytes = rd_blob_bytes(bspec, pw, ph);
    gray_plane(r, njobs, bspec->oversample);
    const rd_scan_spec ink = { RD_SCAN_BITS, bspec->radius, bspec->k, bspec->d, 255, bspec->oversample, bspec->invert, 0 };      // (white: not read in this mode; radius 0 never reaches rdk::scan)
    r->sspec = ink;
    r->d_labels = (int **)calloc(njobs, sizeof(int *));
    r->d_areas = (int **)calloc(njobs, sizeof(int *));
  }
  const size_t nq = (size_t)njobs * max_quads;
  RD_HIP(hipMalloc((void **)&r->d_quads, nq * sizeof(rdk::RectifyQuad)));
  RD_HIP(hipHostMalloc((void **)&r->h_quads, nq * sizeof(rdk::RectifyQuad), hipHostMallocDefault));
  r->d_out = (uint8_t **)calloc(njobs, sizeof(uint8_t *));
  return r;
}

rd_rectifier *rd_rectifier_create(int device, int pw, int ph, int max_quads, int njobs) { return rectifier_create(device, pw, ph, max_quads, njobs, NULL); }

rd_rectifier *rd_rectifier_create_tensor(int device, int pw, int ph, int max_quads, int njobs, const rd_tensor_spec *spec) {
  return spec ? rectifier_create(device, pw, ph, max_quads, njobs, spec) : NULL;
}

rd_rectifier *rd_rectifier_create_scan(int device, int pw, int ph, int max_quads, int njobs, const rd_scan_spec *spec) {
  return spec ? rectifier_create(device, pw, ph, max_quads, njobs, NULL, spec) : NULL;
}

rd_rectifier *rd_rectifier_create_grade(int device, int pw, int ph, int max_quads, int njobs, const rd_grade_spec *spec) {
  return spec ? rectifier_create(device, pw, ph, max_quads, njobs, NULL, NULL, spec) : NULL;
}

rd_rectifier *rd_rectifier_create_code(int device, int pw, int ph, int max_quads, int njobs, const rd_code_spec *spec, const uint64_t *dict, int ndict) {
  return spec ? rectifier_create(device, pw, ph, max_quads, njobs, NULL, NULL, NULL, spec, dict, ndict) : NULL;
}

rd_rectifier *rd_rectifier_create_blobs(int device, int pw, int ph, int max_quads, int njobs, const rd_blob_spec *spec) {
  return spec ? rectifier_create(device, pw, ph, max_quads, njobs, NULL, NULL, NULL, NULL, NULL, 0, spec) : NULL;
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
  for (int k = 0; k < njobs; k++) if (r->d_out[k]) RD_HIP(hipFree(r->d_out[k]));
  for (int k = 0; k < njobs; k++) if (r->d_plane && r->d_plane[k]) RD_HIP(hipFree(r->d_plane[k]));
  for (int k = 0; k < njobs; k++) if (r->d_labels && r->d_labels[k]) RD_HIP(hipFree(r->d_labels[k]));
  for (int k = 0; k < njobs; k++) if (r->d_areas && r->d_areas[k]) RD_HIP(hipFree(r->d_areas[k]));
  if (r->d_dict) RD_HIP(hipFree(r->d_dict));
  RD_HIP(hipFree(r->d_quads));
  RD_HIP(hipHostFree(r->h_quads));
  r->frame.release();
  free(r->d_out);
  free(r->d_plane);
  free(r->d_labels);
  free(r->d_areas);
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
  if (n > 0 && (r->grade || r->code || r->blob) && ((uintptr_t)out & 7)) return -1;      // (the records' 64-bit sums; rd_code::bits)
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
    uint8_t *dst = (uint8_t *)out;
    if (out_kind == RD_FRAME_HOST_PINNED) {
      if (!r->d_out[slot]) RD_HIP(hipMalloc((void **)&r->d_out[slot], (size_t)g->per_job * r->patch_bytes));      // (on first use: a rectifier that writes to device memory only has none)
      dst = r->d_out[slot];
    }
    if (r->scan || r->grade || r->code || r->blob) {
      const size_t plane_bytes = (size_t)g->per_job * r->pw * r->ph + (r->code ? RD_CODE_PLANE_PAD : 0);      // (rdk::code reads whole 16-byte words, and is told how far it may)
      if (!r->d_plane[slot]) RD_HIP(hipMalloc((void **)&r->d_plane[slot], plane_bytes));      // (on first use, like d_out)
      rdk::rectify_tensor(g->st, r->d_plane[slot], format, src, d_quads, n, r->pw, r->ph, r->spec);
      rdrt::check_launch(r->scan ? "scanned pages: the G plane" : r->grade ? "graded quads: the G plane" : r->code ? "decoded quads: the G plane" : "page components: the G plane");
      if (r->scan) rdk::scan(g->st, dst, r->d_plane[slot], d_quads, n, r->pw, r->ph, r->sspec);
      else if (r->blob) {
        const size_t ints = (size_t)g->per_job * r->pw * r->ph;
        if (!r->d_labels[slot]) RD_HIP(hipMalloc((void **)&r->d_labels[slot], ints * sizeof(int)));      // (on first use, like d_plane)
        if (!r->d_areas[slot]) RD_HIP(hipMalloc((void **)&r->d_areas[slot], ints * sizeof(int)));
        uint8_t *bits = (uint8_t *)r->d_areas[slot];      // (rd_k_blob.hip: the bits lie at the start of the area plane until the tile kernel has read them)
        if (r->bspec.radius > 0) rdk::scan(g->st, bits, r->d_plane[slot], d_quads, n, r->pw, r->ph, r->sspec);
        else rdk::blob_level(g->st, bits, r->d_plane[slot], d_quads, n, r->pw, r->ph, r->bspec);
        rdrt::check_launch("page components: the ink bits");
        rdk::blobs(g->st, dst, r->d_labels[slot], r->d_areas[slot], d_quads, n, r->pw, r->ph, r->bspec, NULL);
      } else if (r->code) rdk::code(g->st, dst, r->d_plane[slot], plane_bytes, d_quads, n, r->pw, r->ph, r->cspec, r->d_dict, r->ndict);
      else {
        RD_HIP(hipMemsetAsync(dst, 0, (size_t)n * r->patch_bytes, g->st));      // the kernel ADDS to the records; an invalid quad's stay as they are here
        rdk::grade(g->st, dst, r->d_plane[slot], d_quads, n, r->pw, r->ph, r->gspec);
      }
    } else if (r->tensor) rdk::rectify_tensor(g->st, dst, format, src, d_quads, n, r->pw, r->ph, r->spec);
    else rdk::rectify(g->st, dst, format, src, d_quads, n, r->pw, r->ph);
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
