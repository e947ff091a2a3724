// rectdetect-mi355x: the reference's public operator API (oclimgutil.h, oclpolyline.h, oclrect.h) and the rd_detector
// extension on top of the gfx950 kernels.  C ABI, opaque handles, fatal-on-error like the reference.
#include "rd_internal.h"
#include "rd_kernels.h"
#include "rd_comp.h"
#include "rd_jobs.h"
#include "rd_poly_scratch.h"
#include "rectdetect_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <time.h>
#include <sched.h>

extern "C" {
#include "vec234.h"
#include "oclimgutil.h"
#include "oclpolyline.h"
#include "oclrect.h"
#include "rd_post.h"
}

using rdrt::dptr;
using rdrt::stream;

// Environment switches.  A detector reads the ones include/rectdetect_hip.h lists ("Environment") when it is created - its behaviour never changes afterwards, and two
// detectors of one process may differ.  The switches of experiments whose variant was measured and NOT kept (profiles/NOTES_r0*.md) exist in tuning builds only
// (-DRD_TUNING, tools/variants.sh): in the product they are the constants below.
static const char *rd_env(const char *name) { const char *v = getenv(name); return (v && *v) ? v : NULL; }
static int rd_env_int(const char *name, int dflt) { const char *v = rd_env(name); return v ? atoi(v) : dflt; }
#ifdef RD_TUNING
#define RD_LAB_INT(name, dflt) rd_env_int(name, dflt)
#else
#define RD_LAB_INT(name, dflt) (dflt)
#endif

#define MAGIC_IMGUTIL 0xa640d893u
#define MAGIC_POLYLINE 0x808f3801u
#define MAGIC_RECT 0x808f3802u

template <typename T> static T *dnew(size_t n) { void *p = NULL; RD_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(T))); return (T *)p; }
static void dfree(void *p) { if (p) RD_HIP(hipFree(p)); }

// ================================================================================================ oclimgutil
struct ImgutilImpl { int N; size_t ntails; float *s[3]; float *tails; int *flags; };

static void imgutil_scratch(oclimgutil_t *t, int iw, int ih) {
  ImgutilImpl *im = (ImgutilImpl *)t->impl;
  const int N = iw * ih;
  const size_t a = rdk::iir_pass_scratch_floats(1, ih, iw), b = rdk::iir_pass_scratch_floats(1, iw, ih), nt = a > b ? a : b;
  if (im->N >= N && im->ntails >= nt) return;
  for (int k = 0; k < 3; k++) { dfree(im->s[k]); im->s[k] = dnew<float>((size_t)N); }
  dfree(im->tails); dfree(im->flags);
  im->tails = dnew<float>(nt);
  im->flags = dnew<int>(16); RD_HIP(hipMemset(im->flags, 0, 16 * sizeof(int))); RD_HIP(hipStreamSynchronize(0));
  im->N = N; im->ntails = nt;
}

extern "C" {

oclimgutil_t *init_oclimgutil(cl_device_id device, cl_context context) {
  oclimgutil_t *t = (oclimgutil_t *)calloc(1, sizeof(*t));
  t->magic = MAGIC_IMGUTIL; t->device = device; t->context = context;
  t->impl = calloc(1, sizeof(ImgutilImpl));
  if (device) RD_HIP(hipSetDevice(device->ordinal));
  return t;
}

void dispose_oclimgutil(oclimgutil_t *t) {
  if (!t || t->magic != MAGIC_IMGUTIL) exitf(-1, "dispose_oclimgutil: bad handle\n");
  ImgutilImpl *im = (ImgutilImpl *)t->impl;
  for (int k = 0; k < 3; k++) dfree(im->s[k]);
  dfree(im->tails); dfree(im->flags);
  free(im);
  t->magic = 0;
  free(t);
}

#define IU_BEGIN(name)                                                                   \
  if (!thiz || thiz->magic != MAGIC_IMGUTIL) exitf(-1, name ": bad oclimgutil handle\n"); \
  rdrt::wait_list(queue, events);                                                        \
  hipStream_t s = stream(queue)
#define IU_END(name) rdrt::check_launch(name); return rdrt::finish_op(queue, events)

cl_event oclimgutil_clear(oclimgutil_t *thiz, cl_mem out, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_clear");
  rdk::clear_i(s, (int *)dptr(out), (size + 3) / 4);
  IU_END("oclimgutil_clear");
}
cl_event oclimgutil_copy(oclimgutil_t *thiz, cl_mem out, cl_mem in, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_copy");
  rdk::copy_i(s, (int *)dptr(out), (const int *)dptr(in), (size + 3) / 4);
  IU_END("oclimgutil_copy");
}
cl_event oclimgutil_cast_i_f(oclimgutil_t *thiz, cl_mem out, cl_mem in, float scale, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_cast_i_f");
  rdk::cast_i_f(s, (int *)dptr(out), (const float *)dptr(in), scale, size);
  IU_END("oclimgutil_cast_i_f");
}
cl_event oclimgutil_cast_c_i(oclimgutil_t *thiz, cl_mem out, cl_mem in, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_cast_c_i");
  rdk::cast_c_i(s, (int8_t *)dptr(out), (const int *)dptr(in), size);
  IU_END("oclimgutil_cast_c_i");
}
cl_event oclimgutil_threshold_i_i(oclimgutil_t *thiz, cl_mem out, cl_mem in, int vlow, int threshold, int vhigh, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_threshold_i_i");
  rdk::threshold_i(s, (int *)dptr(out), (const int *)dptr(in), vlow, threshold, vhigh, size);
  IU_END("oclimgutil_threshold_i_i");
}
cl_event oclimgutil_threshold_f_f(oclimgutil_t *thiz, cl_mem out, cl_mem in, float vlow, float threshold, float vhigh, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_threshold_f_f");
  rdk::threshold_f(s, (float *)dptr(out), (const float *)dptr(in), vlow, threshold, vhigh, size);
  IU_END("oclimgutil_threshold_f_f");
}
cl_event oclimgutil_rand(oclimgutil_t *thiz, cl_mem out, int size, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_rand");
  rdk::rand_i(s, (int *)dptr(out), 0, (size + 3) / 4);   // the reference's wrapper never sets the seed argument (oclimgutil.c:178-183)
  IU_END("oclimgutil_rand");
}
cl_event oclimgutil_convert_plab_bgr(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, int ws, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_convert_plab_bgr");
  rdk::bgr2plab(s, (uint32_t *)dptr(out), (const uint8_t *)dptr(in), iw, ih, ws);
  IU_END("oclimgutil_convert_plab_bgr");
}
cl_event oclimgutil_unpack_f_f_f_plab(oclimgutil_t *thiz, cl_mem out0, cl_mem out1, cl_mem out2, cl_mem in, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_unpack_f_f_f_plab");
  rdk::unpack_plab(s, (float *)dptr(out0), (float *)dptr(out1), (float *)dptr(out2), (const uint32_t *)dptr(in), iw * ih);
  IU_END("oclimgutil_unpack_f_f_f_plab");
}
cl_event oclimgutil_pack_plab_f_f_f(oclimgutil_t *thiz, cl_mem out, cl_mem in0, cl_mem in1, cl_mem in2, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_pack_plab_f_f_f");
  rdk::pack_plab(s, (uint32_t *)dptr(out), (const float *)dptr(in0), (const float *)dptr(in1), (const float *)dptr(in2), iw * ih);
  IU_END("oclimgutil_pack_plab_f_f_f");
}

// oclimgutil.c:248-273.  obuf = vertical(horizontal(ibuf)); tmp0 / tmp1 are scratch.  r = 2 (sigma 1, the only radius any
// caller in the reference passes) takes the blocked evaluation of the frame path (scratch only written when that fails its
// on-device check); every other radius of the table (0..31, sigma = (r + 1) / 3) the full-length sweeps.
cl_event oclimgutil_iirblur_f_f(oclimgutil_t *thiz, cl_mem obuf, cl_mem ibuf, cl_mem tmp0, cl_mem tmp1, int r, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_iirblur_f_f");
  if (r < 0 || r > RD_IIR_MAX_R) exitf(-1, "oclimgutil_iirblur_f_f: r = %d is outside the coefficient table (0..%d; the reference reads beyond iircoef[] there)\n", r, RD_IIR_MAX_R);
  imgutil_scratch(thiz, iw, ih);
  ImgutilImpl *im = (ImgutilImpl *)thiz->impl;
  float *o = (float *)dptr(obuf), *t0 = (float *)dptr(tmp0), *t1 = (float *)dptr(tmp1);
  const float *in = (const float *)dptr(ibuf);
  float *d1[3] = { im->s[0], NULL, NULL }; const float *s1[3] = { in, NULL, NULL };
  if (r != 2) {
    // (the mirrored run-in of r + 9 samples must stay inside the line: iu:551 reads mirror1(x) unchecked)
    if (iw < r + 11 || ih < r + 11) exitf(-1, "oclimgutil_iirblur_f_f: r = %d needs planes of at least %d x %d (the reference reads outside a smaller one), got %d x %d\n", r, r + 11, r + 11, iw, ih);
    rdk::transpose_f(s, d1, s1, 1, iw, ih);                                 // s0 = in^T (ih wide)
    rdk::iir_blur_lines(s, t0, im->s[0], t0, t1, ih, iw, r);                // along x; t0 = horizontal result, transposed
    float *d2[3] = { im->s[1], NULL, NULL }; const float *s2[3] = { t0, NULL, NULL };
    rdk::transpose_f(s, d2, s2, 1, ih, iw);                                 // s1 = horizontal result, original layout
    rdk::iir_blur_lines(s, o, im->s[1], t0, t1, iw, ih, r);                 // along y
    IU_END("oclimgutil_iirblur_f_f");
  }
  rdk::transpose_f(s, d1, s1, 1, iw, ih);                                   // s0 = in^T (ih wide)
  float *fw[3] = { t0, NULL, NULL }, *bw[3] = { t1, NULL, NULL };
  { float *dst[3] = { im->s[1], NULL, NULL }; const float *src[3] = { im->s[0], NULL, NULL };
    rdk::iir_blur_pass(s, dst, src, fw, bw, 1, ih, iw, 1, im->tails, im->flags); }       // along x; s1 = horizontal result, original layout
  { float *dst[3] = { o, NULL, NULL }; const float *src[3] = { im->s[1], NULL, NULL };
    rdk::iir_blur_pass(s, dst, src, fw, bw, 1, iw, ih, 0, im->tails, im->flags + 1); }   // along y
  IU_END("oclimgutil_iirblur_f_f");
}

cl_event oclimgutil_edgevec_f2_f(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_edgevec_f2_f");
  rdk::edgevec(s, (float *)dptr(out), (const float *)dptr(in), iw, ih);
  IU_END("oclimgutil_edgevec_f2_f");
}
cl_event oclimgutil_edge_f_plab(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_edge_f_plab");
  rdk::edge_plab(s, (float *)dptr(out), (const uint32_t *)dptr(in), iw, ih);
  IU_END("oclimgutil_edge_f_plab");
}
cl_event oclimgutil_thinthres_f_f_f2(oclimgutil_t *thiz, cl_mem out, cl_mem in, cl_mem vec, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_thinthres_f_f_f2");
  rdk::thinthres(s, (float *)dptr(out), (const float *)dptr(in), (const float *)dptr(vec), iw, ih);
  IU_END("oclimgutil_thinthres_f_f_f2");
}
// oclimgutil.c:227-246: converged labelling instead of 1 + 10 propagation passes; `tmp` (the reference's pass flags) is unused
cl_event oclimgutil_label8x_int_int(oclimgutil_t *thiz, cl_mem out, cl_mem in, cl_mem tmp, int bgc, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_label8x_int_int");
  (void)tmp;
  rdk::label8(s, (int *)dptr(out), (const int *)dptr(in), bgc, iw, ih);
  IU_END("oclimgutil_label8x_int_int");
}
cl_event oclimgutil_calcStrength(oclimgutil_t *thiz, cl_mem out, cl_mem edge, cl_mem label, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_calcStrength");
  rdk::calc_strength(s, (int *)dptr(out), (const float *)dptr(edge), (int *)dptr(label), iw, ih);
  IU_END("oclimgutil_calcStrength");
}
cl_event oclimgutil_filterStrength(oclimgutil_t *thiz, cl_mem labelinout, cl_mem str, int thre, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_filterStrength");
  rdk::filter_strength(s, (int *)dptr(labelinout), (const int *)dptr(str), thre, iw, ih);
  IU_END("oclimgutil_filterStrength");
}

// Debug visualisers and operators no application calls (SURVEY.md 8a "dead for the apps", 8f rank 4).
cl_event oclimgutil_convert_bgr_lumaf(oclimgutil_t *thiz, cl_mem out, cl_mem in, float f, int iw, int ih, int ws, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_convert_bgr_lumaf");
  rdk::convert_bgr_lumaf(s, (uint8_t *)dptr(out), (const float *)dptr(in), f, iw, ih, ws);
  IU_END("oclimgutil_convert_bgr_lumaf");
}
cl_event oclimgutil_convert_bgr_labeli(oclimgutil_t *thiz, cl_mem out, cl_mem in, int bgc, int iw, int ih, int ws, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_convert_bgr_labeli");
  rdk::convert_bgr_labeli(s, (uint8_t *)dptr(out), (const int *)dptr(in), bgc, iw, ih, ws);
  IU_END("oclimgutil_convert_bgr_labeli");
}
cl_event oclimgutil_convert_bgr_plab(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, int ws, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_convert_bgr_plab");
  rdk::plab2bgr(s, (uint8_t *)dptr(out), (const uint32_t *)dptr(in), iw, ih, ws);
  IU_END("oclimgutil_convert_bgr_plab");
}
cl_event oclimgutil_edge_f_f(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_edge_f_f");
  rdk::edge_f(s, (float *)dptr(out), (const float *)dptr(in), iw, ih);
  IU_END("oclimgutil_edge_f_f");
}
cl_event oclimgutil_edgevec_f2_plab(oclimgutil_t *thiz, cl_mem out, cl_mem in, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_edgevec_f2_plab");
  rdk::edgevec_plab(s, (float *)dptr(out), (const uint32_t *)dptr(in), iw, ih);
  IU_END("oclimgutil_edgevec_f2_plab");
}
cl_event oclimgutil_thincubic_f_f_f2(oclimgutil_t *thiz, cl_mem out, cl_mem in, cl_mem vec, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  IU_BEGIN("oclimgutil_thincubic_f_f_f2");
  rdk::thincubic(s, (float *)dptr(out), (const float *)dptr(in), (const float *)dptr(vec), iw, ih);
  IU_END("oclimgutil_thincubic_f_f_f2");
}
// The reference sets 5 of the 6 arguments of its convert_bgr_luminancef kernel (oclimgutil.c:187 "MMiii" against
// iu:275: out, in, f, iw, ih, ws), so the call cannot succeed on a conforming OpenCL runtime (CL_INVALID_KERNEL_ARGS ->
// exitf); it fails here in the same way, with the reason spelled out.
cl_event oclimgutil_convert_bgr_luminancef(oclimgutil_t *, cl_mem, cl_mem, int, int, int, cl_command_queue, const cl_event *) {
  exitf(-1, "oclimgutil_convert_bgr_luminancef: the reference passes 5 of this kernel's 6 arguments (oclimgutil.c:187); the call is an error there and here\n");
  return NULL;
}

}  // extern "C"

// ================================================================================================ oclpolyline
struct PolylineImpl { int iw, ih; rdk::PolyScratch *ps; };

extern "C" {

oclpolyline_t *init_oclpolyline(cl_device_id device, cl_context context) {
  oclpolyline_t *t = (oclpolyline_t *)calloc(1, sizeof(*t));
  t->magic = MAGIC_POLYLINE; t->device = device; t->context = context;
  t->impl = calloc(1, sizeof(PolylineImpl));
  if (device) RD_HIP(hipSetDevice(device->ordinal));
  return t;
}

void dispose_oclpolyline(oclpolyline_t *t) {
  if (!t || t->magic != MAGIC_POLYLINE) exitf(-1, "dispose_oclpolyline: bad handle\n");
  PolylineImpl *im = (PolylineImpl *)t->impl;
  rdk::poly_scratch_destroy(im->ps);
  free(im);
  t->magic = 0;
  free(t);
}

// oclpolyline.c:218-309.  The caller's scratch planes are not needed by this implementation (it keeps its own compact
// scratch), except that the ring of tmp3 is read for the stale-ring semantics of the reference (see oclpolyline.h).
cl_event oclpolyline_execute(oclpolyline_t *thiz, cl_mem lsList, int lsListSize, cl_mem lsIdOut, cl_mem in, cl_mem tmp0, cl_mem tmp1, cl_mem tmp2, cl_mem tmp3,
                             cl_mem tmp4, cl_mem tmp5, cl_mem tmp6, float minerror, int sizeThre, int iw, int ih, cl_command_queue queue, const cl_event *events) {
  if (!thiz || thiz->magic != MAGIC_POLYLINE) exitf(-1, "oclpolyline_execute: bad handle\n");
  (void)tmp0; (void)tmp1; (void)tmp2; (void)tmp4; (void)tmp5; (void)tmp6;
  PolylineImpl *im = (PolylineImpl *)thiz->impl;
  if (!im->ps || im->iw != iw || im->ih != ih) {
    rdk::poly_scratch_destroy(im->ps);
    im->ps = rdk::poly_scratch_create(iw, ih);
    im->iw = iw; im->ih = ih;
  }
  rdrt::wait_list(queue, events);
  // the frame descriptor of this call (the kernels of the stage take their pointers from it: rd_poly_scratch.h)
  rdk::PolyFrame fr;
  memset(&fr, 0, sizeof(fr));
  fr.ps = *im->ps; fr.in = (const int *)dptr(in); fr.ring_src = (const int *)dptr(tmp3); fr.lslist = dptr(lsList); fr.ids = (int *)dptr(lsIdOut);
  rdk::polyline(stream(queue), &fr, 1, lsListSize, 0, minerror, sizeThre, iw, ih, 0);
  rdk::polyline_ids(stream(queue), &fr, 1, iw * ih);
  rdrt::check_launch("oclpolyline_execute");
  return rdrt::finish_op(queue, events);
}

}  // extern "C"

// ================================================================================================ detector
#define RD_NBUDGETS 7       // launch budgets of the region merge: 8, 10, .. 20 (kRoundBudgets)
#define RD_NSEQ (1 + 2 * RD_NBUDGETS)      // captured launch sequences of a frame or a group (Slot::graphs)
#define RD_MAXREC 512       // records copied back per frame without a second transfer (the copy runs at PCIe speed: 16 us for 2048)

struct Slot {
  hipStream_t st;
  hipStream_t st2;                        // second stream of the slot: polyline stage, parallel to the region stages
  int pooled_streams;                     // st / st2 come from the process-wide pool of high-priority streams and go back there
  int shares_streams;                     // st / st2 belong to another slot (see rd_detector_create)
  hipEvent_t ev_fork, ev_mm, ev_join;
  hipEvent_t ev_begin, ev_done, ev_strong;   // ev_begin/ev_done carry timestamps: device time of the frame (rd_detector_counter)
  hipEvent_t watch_begin, watch_done;        // the events that bracket the frame in flight: the slot's own, or - a frame of a group launch - the ones of the group's first slot
  hipEvent_t ev_redo;                        // end of a repeated part of the frame (slot_finish_device)
  hipEvent_t ev_upload;                      // one or two frames in flight: the copy engine has read a host frame it took straight from the caller's pinned buffer
  hipStream_t st_redo;                       // created on first use: the slow absorption path (frame_absorb_slow), fetches of long lists
  int *big_probes; int big_probes_cap;       // probes of a frame with more segments than `probes` holds (grows on demand)
  const int8_t *prev_in;                  // the strong mask this slot's frame read (plane of rd_detector::prev_ring)
  uint8_t *bgr;
  const uint8_t *src;                     // where the frame in flight is read from: bgr (uploaded) or the caller's device buffer
  uint32_t *plab0, *plab1, *smooth, *quant;
  float *tr[3], *fw[3], *bw[3], *hz[3], *bl[3], *vxy, *strength, *nms;
  int *i0, *i1, *mask0, *tidy, *label1, *strsum, *region, *rsize, *scratch2, *d2s, *boundarysrc, *boundary, *lsid, *table, *claim, *probes, *region0, *tlist;
  int8_t *e8;
  unsigned long long *mmbits;             // the merge mask (oclrect.c:315-321) as a bit plane
  unsigned long long *strongbits;         // this frame's strong mask as a bit plane (ceil(iw / 64) words per row): what the polyline stage traces
  uint16_t *ext;
  float *tails; int *flags;
  void *lslist;
  rdk::PolyScratch *ps;
  rdk::PolyFrame *frame;                  // this slot's descriptor for the sparse stages (element `slot index` of the detector's array)
  hipEvent_t ev_dense;                    // batched mode: the frame's dense stages are done (the batch's sparse stages wait for it)
  int pending_sparse;                     // batched mode: dense stages enqueued, sparse stages not launched yet
  int pending_dense;                      // group mode (rd_detector::zb > 1): frame handed over, nothing launched yet
  int group_n;                            // frames that ran between this frame's ev_begin and ev_done (1, or the group's size: the interval is shared)
  // rectangles on the device (RD_DEVICE_POST): scratch, result block in pinned host memory, whether this frame's block is valid and for which aperture
  int *post_scratch, *h_post, *h_post_dev;
  int post_mode; double post_tan;
  // host side
  void *h_bgr;            // pinned staging for host frames
  void *h_segs; int *h_probes; int *h_ctr;   // views into h_pack
  int *h_pack, *h_pack_dev;                // everything the host needs from a frame, assembled by the device in pinned host memory (host / device address)
  long seq;
  int ws;
  // the frame's pixel format (RD_PIX_*), its planes and their row strides (hand_over); src = pl[0] and ws = pitch[0]; a host frame's planes are packed into bgr
  int fmt;
  const uint8_t *pl[3]; int pitch[3];
  // rd_detector_enqueue_scaled: 1, or 2 - the planes hold a frame of 2 iw x 2 ih pixels, which the front kernel averages 2x2 as it reads.  A host frame of that size
  // (up to 16 bytes per detector pixel) does not fit bgr / h_bgr: it travels through a pair of staging buffers of its own, which a slot gets with its first such frame
  int scale;
  uint8_t *sc_bgr; void *sc_h; size_t sc_bytes;
  // Captured launch sequences: [0] this slot's frame on its own, [1] the group this slot leads (group mode); by sequence - 0: the dense stages up to the first
  // labelling, 1 + 2 * round budget index + polyline mode: everything after the strong masks (the polyline kind's one sequence: 1 + polyline mode).  None reads the
  // frame (the colour conversion runs in front of them, outside), so a change of format or row stride re-captures nothing.
  hipGraphExec_t graphs[2][RD_NSEQ];
  int poly_mode;                          // polyline mode of the frame in flight (1 = single block, 0 = multi-launch)
  int rounds;                             // region-merge round budget of the frame in flight
  // post-process worker
  pthread_t th; pthread_mutex_t mu; pthread_cond_t cv;
  int state;              // 0 idle, 1 submitted to the GPU, 2 result ready
  int quit;
  void *result; double result_tan; void *res_segs; int res_nsegs;
  struct rd_detector *owner;
};

struct rd_detector {
  uint32_t magic;
  int device, iw, ih, N, nslots, nworkers, maxrec_dev;
  // Sparse stages (polylines, votes, probes) of `batch` consecutive frame slots run as ONE set of launches (frame = blockIdx.z): they
  // are a chain of 20-odd latency-bound launches that keeps a hardware queue busy for ~0.4 ms without filling the chip, per
  // batch instead of per frame.  Slots [g * batch, (g + 1) * batch) form group g; 1 = every frame on its own (shortest latency).
  int batch; unsigned sparse_rot;
  int device_post;                        // candidate funnel + pose estimation on the device (rd_k_post.hip) instead of the host worker threads
  long n_post_device, n_post_host, host_post_ns;
  int defer, deferred_slot;               // batched mode: a complete group's sparse stages are launched only once the NEXT group's dense stages are enqueued (deferred_slot: a slot of the waiting group or -1)
  rdk::PolyFrame *frames;                 // nslots descriptors (host memory; they travel as kernel arguments), slot order
  Slot *slots;
  int nstreams;
  int zb;                 // frames per launch of the DENSE stages as well (groups of zb consecutive slots, frame = blockIdx.z): small frames, whose launches do not fill the device
  char *arena; size_t slot_pitch;      // all slots' planes in one allocation, slot k at arena + k * slot_pitch (kSlotPlanes; rd_detector_counter 31: the pitch)
  // strong-edge masks of the last frames (reference quirk H1: a frame's strength sums start from the mask of the frame before), one byte per
  // pixel: a ring of nslots + 1 planes - frame t reads plane t mod (nslots + 1) and writes the next one, so what a frame read stays intact as
  // long as its slot's planes do (debug plane "strsum")
  int8_t *prev_ring; int nring;
  int t_edge, t_strong;                   // thresholds of the strength sums (500, 2500; RD_TEST_THRESHOLDS)
  int strong_by_frame;                    // tests (RD_STRONG_BY_FRAME): the strong masks of a group frame by frame instead of in one launch
  long n_strong_group, n_strong_by_frame; // groups whose strong masks took one launch / one launch per frame (rd_detector_counter 16 / 17)
  hipEvent_t last_strong; int have_last_strong;
  long next_enqueue, next_poll;
  long done_seq;                          // one more than the highest sequence number whose device work a worker has seen finished
  int last_polled_slot;
  void *last_segs; int last_nsegs;
  int use_graph, poly_mode, force_redo, fork_poly, fixed_rounds, budget_cycle; long n_redo, n_redo_rounds, n_redo_absorb;
  int overflow_streak;
  int poly_overflows;                     // set once two frames in a row overflowed the single-launch polyline kernel: later frames go multi-launch
  int rounds_budget, need_hist[64]; unsigned need_pos; long budget_count[RD_NBUDGETS], need_count[21];
  hipStream_t st_upload;     // group mode, host frames: the stream the frames travel on (created on first use, from the pool of high-priority streams)
  int post_helpers;          // helper threads armed by every poll (rd_post.c), 0 = none
  long host_enqueue_ns;      // wall time the caller spent inside rd_detector_enqueue
  long dev_us, dev_frames;   // sum over polled frames of (last kernel end - first kernel start) on the frame's stream, HIP events
  double tan_aov; int have_tan;    // what the workers use ahead of the poll that asks for the result
  pthread_mutex_t tan_mu; pthread_cond_t tan_cv;
  // Slots share streams (slot i uses the streams of slot i mod 4) and a worker thread may repeat part of its slot's frame on such a
  // stream while the enqueueing thread captures another slot's launch sequence on it: a capture would record the foreign launches, and
  // a stream that is capturing must not be synchronised.  launch_mu serialises captures against the launches of a repeat; repeats wait
  // on an event of their own (ev_redo), never on the stream.
  pthread_mutex_t launch_mu;
  const void *pinned[4][2]; unsigned pinned_next;   // the last 4 ranges of caller memory that were verified to be pinned host memory (RD_FRAME_HOST_PINNED; a frame's planes may lie in allocations of their own)
  const void *probed[2]; int probed_pinned[2];      // RD_FRAME_HOST, one or two frames in flight: the last two frame pointers asked about (a loop alternates between its two pages) and the answer
  long n_frames_pinned, n_frames_copied;     // host frames that travelled straight from the caller's pinned memory / through the detector's own staging pages
  long n_unsettled;          // frames whose region merge was still changing after RD_REGION_MAX_LAUNCHES launches (none on any fixture)
  long n_truncated;          // frames with more segment records than the slots' probe buffers hold (maxrec_dev): probed again into a larger buffer
  // the polyline kind (rd_polyline_detector_create: poly.cpp / vidpoly.cpp per frame); a rectangle detector has kind RD_KIND_RECT and none of this
  int kind;
  int p_thre, p_size; float p_minerror;     // filterStrength threshold, sizeThre, minerror
  int handoff_rec;           // records (header included) each slot's pinned block receives at the end of a frame (RD_POLY_HANDOFF)
  long n_long_lists;         // frames whose list did not fit that block and was fetched by the poll (rd_detector_counter 30)
};
#define RD_KIND_RECT 0
#define RD_KIND_POLY 1
#define RD_POLY_HANDOFF_DEFAULT 2048      // records handed off per frame: 112 KB of pinned memory per slot

// The device planes of a slot: the one list of them, both kinds, in layout order.  Every detector carves its slots out of one allocation (rd_detector::arena): slot k
// at arena + k * slot_pitch, its planes in the order of the rows its kind owns, each rounded up to 256 bytes.  The planes of slot k + z then lie a constant number
// of bytes behind those of slot k - a kernel of a group launch reaches frame z's planes as `pointer + blockIdx.z * pitch` - and a frame that is launched on its own
// runs on the layout the groups use: a kernel that runs past its plane lands in the neighbouring plane in every configuration.
// Offsets, the slot's size and the Slot's pointers all come from one walk of this list (slot_planes); nothing else names the planes.
#define PK_RECT 1
#define PK_POLY 2
#define PK_POLY_UNFUSED 4      // the polyline kind at frame sizes the fused front kernel's tiles do not cover (!front_is_fused): the three operators need their planes
#define PK_BOTH (PK_RECT | PK_POLY)
typedef size_t PlaneCount(const rd_detector *d);      // elements of a plane
static size_t pn_n(const rd_detector *d) { return (size_t)d->N; }
static size_t pn_2n(const rd_detector *d) { return (size_t)d->N * 2; }
static size_t pn_4n(const rd_detector *d) { return (size_t)d->N * 4; }
static size_t pn_16n(const rd_detector *d) { return (size_t)d->N * 16; }
static size_t pn_scratch2(const rd_detector *d) { return (size_t)d->N * 3 + 256; }      // region_merge: the initial forest, flags + allow bytes, the second label plane of the rounds
static size_t pn_d2(const rd_detector *d) { return RD_D2_SCRATCH_INTS(d->N); }
static size_t pn_bits(const rd_detector *d) { return (size_t)((d->iw + 63) / 64) * d->ih + 8; }      // a bit plane: ceil(iw / 64) words per row
static size_t pn_tails(const rd_detector *d) { const size_t a = rdk::iir_pass_scratch_floats(3, d->ih, d->iw), b = rdk::iir_pass_scratch_floats(3, d->iw, d->ih); return a > b ? a : b; }
static size_t pn_flags(const rd_detector *) { return 16; }
static size_t pn_probes(const rd_detector *d) { return (size_t)d->maxrec_dev * 15 * 6; }
#define PLANE(field, count, kinds) { offsetof(Slot, field), sizeof(*((Slot *)0)->field), count, kinds }
#define BLUR_PLANES(k) PLANE(tr[k], pn_n, PK_BOTH), PLANE(fw[k], pn_n, PK_BOTH), PLANE(bw[k], pn_n, PK_BOTH), PLANE(hz[k], pn_n, PK_BOTH), PLANE(bl[k], pn_n, PK_BOTH)
static const struct { size_t field, elem; PlaneCount *count; int kinds; } kSlotPlanes[] = {
  PLANE(bgr, pn_4n, PK_BOTH),
  PLANE(plab0, pn_n, PK_BOTH),            // (polyline kind: the colour conversion's packed output is read by nothing but the debug plane)
  PLANE(plab1, pn_n, PK_RECT), PLANE(smooth, pn_n, PK_RECT), PLANE(quant, pn_n, PK_RECT),
  BLUR_PLANES(0), BLUR_PLANES(1), BLUR_PLANES(2),
  PLANE(plab1, pn_n, PK_POLY_UNFUSED),    // (the polyline kind has it behind the blur's planes: a second row, so that no plane of either kind moves)
  PLANE(vxy, pn_2n, PK_RECT | PK_POLY_UNFUSED), PLANE(strength, pn_n, PK_RECT | PK_POLY_UNFUSED),
  PLANE(nms, pn_n, PK_BOTH),
  PLANE(i0, pn_n, PK_RECT), PLANE(i1, pn_n, PK_RECT), PLANE(mask0, pn_n, PK_BOTH), PLANE(tidy, pn_n, PK_RECT), PLANE(label1, pn_n, PK_BOTH), PLANE(strsum, pn_n, PK_BOTH),
  PLANE(region, pn_n, PK_RECT), PLANE(rsize, pn_n, PK_RECT), PLANE(boundarysrc, pn_n, PK_RECT), PLANE(boundary, pn_n, PK_RECT), PLANE(lsid, pn_n, PK_BOTH), PLANE(region0, pn_n, PK_RECT),
  PLANE(scratch2, pn_scratch2, PK_RECT), PLANE(d2s, pn_d2, PK_RECT),
  PLANE(table, pn_4n, PK_RECT), PLANE(claim, pn_n, PK_RECT), PLANE(tlist, pn_n, PK_RECT),
  PLANE(e8, pn_n, PK_RECT),
  PLANE(strongbits, pn_bits, PK_BOTH),    // (polyline kind: the poly mask, what the polyline stage traces)
  PLANE(mmbits, pn_bits, PK_RECT),
  PLANE(ext, pn_n, PK_RECT),
  PLANE(tails, pn_tails, PK_BOTH), PLANE(flags, pn_flags, PK_BOTH),
  { offsetof(Slot, lslist), 1, pn_16n, PK_BOTH },      // (bytes: the list has the reference's capacity)
  PLANE(probes, pn_probes, PK_RECT),
};
#undef BLUR_PLANES
#undef PLANE

static bool front_is_fused(const rd_detector *d);
// The walk: the size of a slot of d's kind; with s != NULL also s's pointers, into the slot's range at `base`.
static size_t slot_planes(const rd_detector *d, Slot *s, char *base) {
  const int kind = d->kind == RD_KIND_POLY ? PK_POLY | (front_is_fused(d) ? 0 : PK_POLY_UNFUSED) : PK_RECT;
  size_t at = 0;
  for (const auto &r : kSlotPlanes) {
    if (!(r.kinds & kind)) continue;
    if (s) { char *p = base + at; memcpy((char *)s + r.field, &p, sizeof(p)); }
    at += (r.count(d) * r.elem + 255) & ~(size_t)255;
  }
  return at;
}

// Streams of the high-priority pool (see slot_alloc) are kept for the life of the process and handed to the next detector of the same device: a detector
// that is closed and another one opened (bench.py's side configurations after the headline) then runs on the same hardware queues instead of a second set.
static struct { pthread_mutex_t mu; hipStream_t st[64]; int dev[64]; int n; } stream_pool = { PTHREAD_MUTEX_INITIALIZER };
static hipStream_t pooled_stream(int device) {
  hipStream_t st = NULL;
  pthread_mutex_lock(&stream_pool.mu);
  for (int i = 0; i < stream_pool.n; i++) if (stream_pool.dev[i] == device) { st = stream_pool.st[i]; stream_pool.st[i] = stream_pool.st[stream_pool.n - 1]; stream_pool.dev[i] = stream_pool.dev[stream_pool.n - 1]; stream_pool.n--; break; }
  pthread_mutex_unlock(&stream_pool.mu);
  if (st) {      // (handed back idle - its last user synchronised it; one that reports an error instead is not handed out again)
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess || e == hipErrorNotReady) return st;
    (void)hipGetLastError();
    (void)hipStreamDestroy(st);
  }
  int lo = 0, hi = 0;
  RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  RD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
  return st;
}
static void unpool_stream(int device, hipStream_t st) {
  pthread_mutex_lock(&stream_pool.mu);
  const bool room = stream_pool.n < 64;
  if (room) { stream_pool.st[stream_pool.n] = st; stream_pool.dev[stream_pool.n] = device; stream_pool.n++; }
  pthread_mutex_unlock(&stream_pool.mu);
  if (!room) RD_HIP(hipStreamDestroy(st));
}

// the pool's teardown, for a caller that wants the streams gone (they are otherwise kept until the process ends, at most 64 of them): destroys every pooled stream
// of `device` (-1: of every device); streams in use by a live detector are not in the pool and are not touched
extern "C" void rd_release_cached_streams(int device) {
  hipStream_t gone[64]; int dev[64]; int n = 0;
  pthread_mutex_lock(&stream_pool.mu);
  for (int i = 0; i < stream_pool.n;) {
    if (device < 0 || stream_pool.dev[i] == device) {
      gone[n] = stream_pool.st[i]; dev[n] = stream_pool.dev[i]; n++;
      stream_pool.st[i] = stream_pool.st[stream_pool.n - 1]; stream_pool.dev[i] = stream_pool.dev[stream_pool.n - 1]; stream_pool.n--;
    } else i++;
  }
  pthread_mutex_unlock(&stream_pool.mu);
  for (int i = 0; i < n; i++) { RD_HIP(hipSetDevice(dev[i])); RD_HIP(hipStreamSynchronize(gone[i])); RD_HIP(hipStreamDestroy(gone[i])); }
}

// A slot's stream for repeats and fetches (created on first use): from the runtime's high-priority pool of hardware queues.  As ordinary streams they share the
// four queues of the default pool with the four streams that carry the groups, so a repeat - the oldest frame in flight, the one the caller waits for - stood in a queue
// behind whole groups of later frames after all (the reason it has a stream of its own); with queues of their own: 2853 against 2776-2791 frames/s on one box
// (RD_REDO_STREAM_PRIORITY=0: ordinary streams).  The group streams themselves stay in the default pool: moved to the high-priority pool they gain as much at 1920x1080
// but a detector opened after another one was closed in the same process (bench.py's side configurations) then ran 10-16 % slower - not understood, not kept.
static hipStream_t make_redo_stream() {
  static const int prio = RD_LAB_INT("RD_REDO_STREAM_PRIORITY", 1);
  hipStream_t st = NULL;
  if (prio) { int lo = 0, hi = 0; RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi)); RD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi)); }
  else RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  return st;
}

// the events of a slot; ev_begin / ev_done carry timestamps (device time of the frame: rd_detector_counter 1)
static const struct { hipEvent_t Slot::*ev; bool timing; } kSlotEvents[] = {
  { &Slot::ev_fork, false }, { &Slot::ev_join, false }, { &Slot::ev_mm, false }, { &Slot::ev_begin, true }, { &Slot::ev_done, true },
  { &Slot::ev_strong, false }, { &Slot::ev_redo, false }, { &Slot::ev_upload, false }, { &Slot::ev_dense, false },
};

// share: the slot whose streams this one uses as well (NULL: own streams)
static void slot_alloc(rd_detector *d, Slot *s, Slot *share) {
  const size_t N = (size_t)d->N;
  s->shares_streams = share != NULL;
  if (share) { s->st = share->st; s->st2 = share->st2; }
  else {
    // One or two frames in flight: each frame spreads over two streams, and the four streams of two frames need four hardware queues of their own.  The
    // runtime hands its four queues per priority level to the streams in the order they first launch something, and the null stream (set-up copies) and the
    // caller's command queue hold two of them: the second frame's streams then land on the queues of the first frame's - its main chain behind the other's polyline
    // chain (traced: two frames in flight ran 1.18 times as fast as one).  The streams of such a detector therefore come from the pool of another priority
    // level, where nothing else lives.  (Raising the number of queues for everybody - GPU_MAX_HW_QUEUES=8 - does the same for this path, 1420 -> 1590 frames/s, but
    // costs the group path, whose four streams are best served by four queues, 9 %.)
    static const int fork_prio = RD_LAB_INT("RD_FORK_STREAM_PRIORITY", 1);
    const bool from_pool = fork_prio != 0;
    if (d->fork_poly && from_pool) {
      s->st = pooled_stream(d->device);
      s->st2 = pooled_stream(d->device);
      s->pooled_streams = 1;
    } else {
    RD_HIP(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    RD_HIP(hipStreamCreateWithFlags(&s->st2, hipStreamNonBlocking));
    }
  }
  for (const auto &e : kSlotEvents) { if (e.timing) RD_HIP(hipEventCreate(&(s->*e.ev))); else RD_HIP(hipEventCreateWithFlags(&(s->*e.ev), hipEventDisableTiming)); }
  slot_planes(d, s, d->arena + (size_t)(s - d->slots) * d->slot_pitch);
  // what the planes must hold before the first frame: empty vote tables, the blur's flags at zero
  if (d->kind == RD_KIND_RECT) rdk::reduce_ls_init(s->st, s->table, s->claim, s->tlist, (int)(N * 4 / 5));
  RD_HIP(hipMemset(s->flags, 0, 16 * sizeof(int))); RD_HIP(hipStreamSynchronize(0));
  s->ps = rdk::poly_scratch_create(d->iw, d->ih);
  RD_HIP(hipHostMalloc(&s->h_bgr, N * 4, hipHostMallocDefault));
  const size_t pack_ints = d->kind == RD_KIND_POLY ? 64 + (size_t)d->handoff_rec * 14 : 64 + (size_t)RD_MAXREC * (14 + 15 * 6);      // (poly kind: counters + records, no probes)
  RD_HIP(hipHostMalloc((void **)&s->h_pack, pack_ints * sizeof(int), hipHostMallocDefault)); memset(s->h_pack, 0, pack_ints * sizeof(int));
  RD_HIP(hipHostGetDevicePointer((void **)&s->h_pack_dev, s->h_pack, 0));
  s->h_ctr = s->h_pack; s->h_segs = s->h_pack + 64; s->h_probes = s->h_pack + 64 + (size_t)RD_MAXREC * 14;
  s->rounds = 20;
  s->seq = -1;
  if (d->device_post) {
    s->post_scratch = dnew<int>(rdk::post_scratch_ints());
    RD_HIP(hipHostMalloc((void **)&s->h_post, rdk::post_out_ints() * sizeof(int), hipHostMallocDefault)); memset(s->h_post, 0, rdk::post_out_ints() * sizeof(int));
    RD_HIP(hipHostGetDevicePointer((void **)&s->h_post_dev, s->h_post, 0));
  }
  // descriptor of the sparse stages
  s->frame = d->frames + (s - d->slots);
  rdk::PolyFrame &f = *s->frame;
  memset(&f, 0, sizeof(f));
  f.ps = *s->ps; f.in = NULL; f.in_bits = s->strongbits; f.ring_src = NULL; f.lslist = s->lslist; f.ids = s->lsid;
  f.boundary = s->boundary; f.table = s->table; f.claim = s->claim; f.tlist = s->tlist; f.probes = s->probes; f.pack = s->h_pack_dev; f.rflags = s->scratch2 ? s->scratch2 + N : NULL;
  f.post_scratch = s->post_scratch; f.post_out = s->h_post_dev;
}

static void slot_free(Slot *s, int device) {
  RD_HIP(hipStreamSynchronize(s->st));
  // (the planes: part of the detector's arena, freed with it)
  rdk::poly_scratch_destroy(s->ps);
  RD_HIP(hipHostFree(s->h_bgr)); RD_HIP(hipHostFree(s->h_pack));
  if (s->sc_bgr) RD_HIP(hipFree(s->sc_bgr));
  if (s->sc_h) RD_HIP(hipHostFree(s->sc_h));
  dfree(s->post_scratch); if (s->h_post) RD_HIP(hipHostFree(s->h_post));
  for (const auto &e : kSlotEvents) RD_HIP(hipEventDestroy(s->*e.ev));
  if (s->st_redo) RD_HIP(hipStreamDestroy(s->st_redo));
  dfree(s->big_probes);
  if (!s->shares_streams) {
    if (s->pooled_streams) { RD_HIP(hipStreamSynchronize(s->st2)); RD_HIP(hipStreamSynchronize(s->st)); unpool_stream(device, s->st2); unpool_stream(device, s->st); }
    else {
    RD_HIP(hipStreamDestroy(s->st2));
    RD_HIP(hipStreamDestroy(s->st));
    }
  }
}

// The device part of one frame (reference oclrect.c:235-381), enqueued on the slot's stream in three segments: [0] up to
// the first labelling and [2] the rest, each captured into a hipGraph (frame_segment), and between them [1] the hand-over of the
// strong-edge mask to the next frame (quirk H1, needs an event wait before it and an event record after it: rect_frames).
// last part of a frame: polylines of the strong edges, votes, probes, transfers.  mode 1 uses the single-launch polyline
// stage, which reports frames that do not fit its on-chip tables in counter 25; slot_postprocess() then repeats this
// part with mode 0.
static void frame_polyline(rd_detector *d, Slot *s, hipStream_t st, int mode, int nz = 1) {
  // frame ring of the bridging step is "non-zero" on this path (oclrect.c:361, H3); the dense id plane is only produced on request (debug plane)
  rdk::polyline(st, s->frame, nz, d->N * 16, 1, 4.0f, 20, d->iw, d->ih, mode);
}

// segment / boundary votes (oclrect.c:365-367) and the probes the host needs (oclrect.c:1066-1098) for nb consecutive slots.
// The block the host needs - counters + round flags, the first RD_MAXREC segment records, their probes - is assembled by the
// sampling kernel directly in pinned host memory (0.2 MB of posted writes; frames with more records fetch the rest on demand):
// no copy launch at the end of the frame.
// tables_are_clean: frame_regions() ran just before (its last kernel undoes the previous entries of the vote tables)
// with_post: also the rectangles on the device, for the aperture the caller polled with last (the reference hands the aperture over with
// the poll, after the frame: a frame polled with another one, or the first frames of a stream, are post-processed on the host)
static void frames_votes(rd_detector *d, const rdk::PolyFrame *frames, int nb, hipStream_t st, int tables_are_clean, int with_post, double tan_aov = 0.0) {
  const int nentry = d->N * 4 / 5;
  rdk::reduce_ls(st, frames, nb, d->iw, d->ih, nentry, tables_are_clean);
  rdk::sample_segments(st, frames, nb, d->maxrec_dev, d->iw, d->ih, nentry, RD_MAXREC);
  if (with_post) rdk::post_device(st, frames, nb, d->maxrec_dev, d->iw, d->ih, tan_aov);      // (the caller's snapshot of the aperture: what the frames are labelled with)
}
// the aperture the device post-process of frames launched now runs with (set by polls and rd_detector_set_aperture, possibly on another thread)
static int aperture_snapshot(rd_detector *d, double *tan_out) {
  pthread_mutex_lock(&d->tan_mu);
  const int have = d->have_tan; *tan_out = d->tan_aov;
  pthread_mutex_unlock(&d->tan_mu);
  return have;
}

static void frame_tail(rd_detector *d, Slot *s, int mode) {   // both, in order, on the slot's main stream (overflow redo)
  frame_polyline(d, s, s->st, mode);
  frames_votes(d, s->frame, 1, s->st, 0, 0);
}

// regions, their sizes, absorption of small ones, boundaries and boundary components (oclrect.c:325-342) of nz frames.  Reads planes that
// nothing later in the frame modifies (quant, mergemask, label1, junction), so it can be repeated with a larger round budget.
static void frame_regions(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs) {
  const int iw = d->iw, ih = d->ih, N = d->N;
  // regions (oclrect.c:325-336)
  int *d2scratch = s->d2s;
  int marked = 0;
  rdk::region_merge(st, s->region0, s->scratch2, (const int *)s->quant, s->mmbits, s->strongbits, iw, ih, s->rounds,
                    s->rsize, &marked, nz, zs);   // H2: the sizes start from the junction counts (evaluated by the first kernel)
  rdk::region_size(st, s->rsize, s->region0, N, d2scratch + N, marked, nz, zs);      // (also strips the rounds' marks from the labels)
  rdk::despeckle2(st, s->region, s->region0, d2scratch, s->rsize, RD_ABSORB_THRE, iw, ih, 1, s->scratch2 + N + RD_REGION_STATUS_AT, nz, zs);   // (status words: they travel to the host with the round flags)

  // region boundaries and their components (oclrect.c:340-342)
  rdk::label8_boundary(st, s->boundary, s->boundarysrc, s->region, iw, ih, s->table, s->claim, s->tlist, nz, zs, RD_BOUNDARY_FLATTEN);   // (also undoes the previous frame's vote-table entries)
}

// votes and probes of a frame whose regions were computed again (a frame whose rectangles the device computes gets them again as well,
// from the new regions, for the aperture known now)
static void redo_votes(rd_detector *d, Slot *s, hipStream_t st) {
  int with_post = 0;
  if (s->post_mode) {
    pthread_mutex_lock(&d->tan_mu);
    with_post = d->have_tan; s->post_tan = d->tan_aov;
    pthread_mutex_unlock(&d->tan_mu);
  }
  frames_votes(d, s->frame, 1, st, 1, with_post, s->post_tan);
  s->post_mode = with_post;
}

// The absorption of small regions again for a frame the two fast launches could not finish (h_ctr[52] != 0: more undecided pixels than
// the single-block tail holds, or dependency chains that wind through more rows than it sweeps - frames that consist of small
// regions), by rounds over work lists until nothing changes, then everything downstream of it.  Runs on a stream of the slot's own
// that is never captured (the loop synchronises), after the frame's ev_done: nothing else touches the slot's planes.
static void frame_absorb_slow(rd_detector *d, Slot *s) {
  if (!s->st_redo) s->st_redo = make_redo_stream();
  hipStream_t st = s->st_redo;
  rdk::despeckle2_slow(st, s->region, s->region0, s->d2s, s->rsize, RD_ABSORB_THRE, d->iw, d->ih);
  rdk::label8_boundary(st, s->boundary, s->boundarysrc, s->region, d->iw, d->ih, s->table, s->claim, s->tlist, 1, 0, RD_BOUNDARY_FLATTEN);
  redo_votes(d, s, st);
  RD_HIP(hipStreamSynchronize(st));
  s->h_ctr[52] = 0;
}

// The whole frame-to-frame dependency chain in ONE launch (not captured: its planes change from frame to frame): this frame's strong mask
// (what oclrect.c:307-313 derives from the strength sums) from the sums + the strong mask of the frame before (H1, oclrect.c:274-275: the
// reference starts the sums from that mask; here the mask's element is added where a sum is read).  The same pass yields the edge mask at
// 500 of oclrect.c:277-284 and filters the labels at 2500 (filtering once at 2500 equals filtering at 500 and then at 2500, and both
// masks come from the unfiltered labels).
static void frame_strong(rd_detector *d, Slot *s, hipStream_t st) {
  const size_t N = (size_t)d->N;
  const long t = s->seq;
  s->prev_in = d->prev_ring + (size_t)(t % d->nring) * N;
  int8_t *out = d->prev_ring + (size_t)((t + 1) % d->nring) * N;
  rdk::strength_masks(st, NULL, out, NULL, s->e8, s->label1, s->strsum, d->t_edge, d->t_strong, d->iw, d->ih, s->prev_in, s->strongbits);      // (the mask as bytes for the next frame, as bits for this frame's polylines; nobody reads it as ints)
}

// gradient direction, re-packed blurred Lab, strength, non-max suppression (oclrect.c:251-258) of nz frames: one tile kernel that keeps the three
// intermediate planes on the chip (rd_k_front.hip: k_grad_nms); frame sizes its tiles do not cover take the three operators' kernels.
// taps: the intermediate planes are written as well (debug planes "plab1", "vxy", "strength")
static bool front_is_fused(const rd_detector *d) { return rdk::grad_nms_fits(d->iw, d->ih) != 0; }
static void frames_grad_nms(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs, int taps = 0) {
  const int iw = d->iw, ih = d->ih;
  if (front_is_fused(d)) {
    if (taps) rdk::grad_nms(st, s->nms, s->bl, iw, ih, nz, zs, s->plab1, s->vxy, s->strength);
    else rdk::grad_nms(st, s->nms, s->bl, iw, ih, nz, zs);
    return;
  }
  rdk::edgevec(st, s->vxy, s->bl[0], iw, ih, s->plab1, s->bl[1], s->bl[2], nz, zs);
  rdk::edge_plab(st, s->strength, s->plab1, iw, ih, nz, zs);
  rdk::thinthres(st, s->nms, s->strength, s->vxy, iw, ih, nz, zs);
}

// the front both detector kinds share, for nz frames: sigma=1 blur of L, a, b -> blurred planes (oclrect.c:246-251), then gradient direction (+ the packing of the
// blurred Lab, oclrect.c:251, on the way), strength, non-max suppression (oclrect.c:253-258)
static void frames_front(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs) {
  const int iw = d->iw, ih = d->ih;
  { const float *c[3] = { s->tr[0], s->tr[1], s->tr[2] }; rdk::iir_blur_pass(st, s->hz, c, s->fw, s->bw, 3, ih, iw, 1, s->tails, s->flags, 1, nz, zs); }        // along x (source: 16-bit fields)
  { const float *c[3] = { s->hz[0], s->hz[1], s->hz[2] }; rdk::iir_blur_pass(st, s->bl, c, s->fw, s->bw, 3, iw, ih, 0, s->tails, s->flags + 1, 0, nz, zs); }   // along y
  frames_grad_nms(d, s, st, nz, zs);
}

// Segment 0 or 2 of one frame (nz = 1, zs = 0) or of the nz frames of a group, whose first slot is s and whose planes lie zs bytes apart.
static void frame_segment(rd_detector *d, Slot *s, int seg, hipStream_t st, int nz, size_t zs) {
  const int iw = d->iw, ih = d->ih;
  if (seg == 0) {
  // (colour conversion, oclrect.c:245: launched by launch_frames in front of this segment, outside the recorded graph - its source is the
  //  caller's device buffer when the frame is resident in HBM: no copy of the frame)
  frames_front(d, s, st, nz, zs);
  // mask of positive responses and the rect-path tidy (oclrect.c:262-272)
  // components (background included) of the tidied mask; the tidy itself runs inside the labelling's tile kernel (and clears the
  // strength sums for the H1 segment); the walk to the roots happens in the first kernel of the next segment
  rdk::label8_tidy(st, s->label1, NULL, s->tidy, s->nms, s->strsum, iw, ih, 1, nz, zs);      // (the mask of positive responses, oclrect.c:262-264, is not stored: nothing reads it - debug plane "mask0" derives it from the responses)
  // strength sums per component (oclrect.c:274-275) - without the strong mask of the frame before (H1), which frame_strong() adds
  rdk::calc_strength(st, s->strsum, s->nms, s->label1, iw, ih, NULL, 1, nz, zs);
  return;
  }
  // Three chains leave this point and meet again before the region stage / the votes:
  //   main stream: edge-stopped blur x20 -> quantise -> despeckle                              (oclrect.c:286-303)
  //   2nd stream : junction counts of the filtered labels -> merge mask                      (oclrect.c:315-321)
  //                then the polyline stage, which needs nothing but the strong mask          (oclrect.c:361)
  // With one or two frames in flight (fork_poly: never a group) the second chain runs on the slot's second stream; else everything on the main stream, blur chain first.
  const bool fork = d->fork_poly != 0;
  if (fork) {
    RD_HIP(hipEventRecord(s->ev_fork, st));
    RD_HIP(hipStreamWaitEvent(s->st2, s->ev_fork, 0));
    rdk::junction_bits(s->st2, (unsigned long long *)s->scratch2, s->strongbits, iw, ih);
    rdk::merge_mask(s->st2, s->mmbits, (const unsigned long long *)s->scratch2, iw, ih);
    RD_HIP(hipEventRecord(s->ev_mm, s->st2));
  }

  // edge-preserving smoothing x10, quantise, despeckle (oclrect.c:286-303)
  rdk::blblur_extents(st, s->ext, s->e8, iw, ih, nz, zs);
  // (Two pairs per launch - halo of 8 cells, four passes through two LDS planes, with and without running sums - halve the launches and
  //  the HBM traffic of this stage and were measured 6 % SLOWER at full rate: 100 KB of LDS leave one 1024-thread block per CU and the
  //  extra barriers cost more than the saved traffic; the stage is bound by vector instructions, not by memory.  DESIGN.md.)
  { const uint32_t *src = s->plab0;     // ping-pong between i0 and smooth; the 10th pair lands in smooth
    for (int i = 0; i < 10; i++) { uint32_t *dst = (i & 1) ? s->smooth : (uint32_t *)s->i0; rdk::blblur_pair(st, dst, s->ext, src, iw, ih, nz, zs); src = dst; } }
  rdk::despeckle(st, s->quant, s->smooth, s->nms, iw, ih, 1, nz, zs);      // quantisation to 24 levels per field (oclrect.c:298) happens on the fly

  if (fork) RD_HIP(hipStreamWaitEvent(st, s->ev_mm, 0));
  else {
    rdk::junction_bits(st, (unsigned long long *)s->scratch2, s->strongbits, iw, ih, nz, zs);
    rdk::merge_mask(st, s->mmbits, (const unsigned long long *)s->scratch2, iw, ih, nz, zs);
  }

  frame_regions(d, s, st, nz, zs);
  if (fork) { frame_polyline(d, s, s->st2, s->poly_mode); RD_HIP(hipEventRecord(s->ev_join, s->st2)); }      // (the polyline chain's launches follow the region stage's: of the three places tried - first, before that stage, after it - the one kept)

  if (d->batch > 1) return;      // the sparse stages of the batch's frames follow in one set of launches (sparse_launch)
  if (fork) RD_HIP(hipStreamWaitEvent(st, s->ev_join, 0));
  else frame_polyline(d, s, st, s->poly_mode, nz);
  frames_votes(d, s->frame, nz, st, 1, 0);
}

// The polyline kind (rd_polyline_detector_create): poly.cpp:104-123 / vidpoly.cpp:165-183 per frame, for nz frames as above.  The front of the rect kind, the
// components of nms > 0 (no tidy), the strength sums from zero (no H1 carry-over: poly.cpp:118 clears them), filterStrength + `label > 0` as a bit plane, the
// polyline stage with the frame ring at zero (the reference's tmp3 is a fresh, zeroed buffer: poly.cpp:93) and the hand-off of the list's first records into
// pinned host memory.  Nothing depends on the frame before: the whole frame is one captured sequence.
static void poly_segment(rd_detector *d, Slot *s, int nz, size_t zs, hipStream_t st, int mode) {
  const int iw = d->iw, ih = d->ih, N = d->N;
  frames_front(d, s, st, nz, zs);
  rdk::label8_positive(st, s->label1, s->mask0, s->nms, s->strsum, iw, ih, 1, nz, zs);      // (poly.cpp:115-118; the walk to the roots happens in the next kernel)
  rdk::calc_strength(st, s->strsum, s->nms, s->label1, iw, ih, NULL, 1, nz, zs);           // (poly.cpp:119)
  rdk::poly_mask_bits(st, s->strongbits, s->label1, s->strsum, d->p_thre, iw, ih, nz, zs);   // (poly.cpp:120-121)
  rdk::polyline(st, s->frame, nz, N * 16, 0, d->p_minerror, d->p_size, iw, ih, mode);      // (poly.cpp:123)
  rdk::polyline_handoff(st, s->frame, nz, d->handoff_rec);
}

// region-merge round budgets a frame can be launched with; the rounds stop changing anything after ~10 on typical frames
// and every launched round costs two dispatches even when it exits at once, so the budget follows what recent frames
// needed (+ margin).  A frame whose last launched round still changed something is repeated with the full budget
// (slot_postprocess), so the result never depends on the budget.
static const int kRoundBudgets[RD_NBUDGETS] = { 8, 10, 12, 14, 16, 18, 20 };
static int budget_index(int rounds) { for (int k = 0; k < RD_NBUDGETS; k++) if (kRoundBudgets[k] == rounds) return k; return RD_NBUDGETS - 1; }

// how the polyline stage of the next frame is launched: the single-block kernel (1) until two frames in a row overflowed its on-chip tables
// (e.g. 3840x2160), from then on the ~85-launch form (0), which is also what repeats a frame the single-block kernel gave up on.  (One
// cooperative launch of several blocks per frame was built in round 3 and measured slower than the 85 launches: profiles/NOTES_r03.md.)
static int current_poly_mode(const rd_detector *d) {
  if (d->poly_mode == 0) return 0;
  return __atomic_load_n(&d->poly_overflows, __ATOMIC_RELAXED) ? 0 : 1;
}

// Where slot s keeps the captured form of launch sequence `seq` for nz frames (Slot::graphs), or NULL where the sequence runs kernel by kernel: without graphs
// (RD_NO_GRAPH), and with one or two frames in flight - the captured graph of the forked segment starts its second branch 170 us late, and the front segment, a
// straight line of ten kernels, is no faster as a graph either: 1615-1623 against 1636-1652 frames/s two deep (profiles/NOTES_r05.md).
static hipGraphExec_t *slot_graph(rd_detector *d, Slot *s, int nz, int seq) {
  if (!d->use_graph || d->fork_poly) return NULL;
  return &s->graphs[nz > 1 ? 1 : 0][seq];
}

// Enqueues on st what `record` enqueues there: directly (ge == NULL), or as a graph that is captured from it on first use and kept in *ge.
template <typename F> static void launch_captured(rd_detector *d, hipGraphExec_t *ge, hipStream_t st, F record) {
  if (!ge) { record(); return; }
  if (!*ge) {
    hipGraph_t g = NULL;
    pthread_mutex_lock(&d->launch_mu);
    RD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    record();
    RD_HIP(hipStreamEndCapture(st, &g));
    pthread_mutex_unlock(&d->launch_mu);
    RD_HIP(hipGraphInstantiate(ge, g, NULL, NULL, 0));
    RD_HIP(hipGraphDestroy(g));
  }
  RD_HIP(hipGraphLaunch(*ge, st));
}

// What the rect kind launches behind the front kernel of one frame (nz = 1) or of the full group that slot s leads.  What cannot be shared by a group is the short
// middle part - a frame's strength sums start from the strong mask of the frame before it (H1) - which runs between the two captured segments, on the same stream.
static void rect_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  const size_t zs = nz > 1 ? d->slot_pitch : 0;
  launch_captured(d, slot_graph(d, s, nz, 0), st, [&] { frame_segment(d, s, 0, st, nz, zs); });
  // the strong masks: each frame's on top of its predecessor's (H1) - one launch for a group where its planes allow 16-byte accesses (the mask of the frame before
  // only decides sums that stand one below a threshold, and is then evaluated on the spot: k_strength_masks_group), else frame by frame
  if (d->have_last_strong) RD_HIP(hipStreamWaitEvent(st, d->last_strong, 0));      // (only the first frame waits for the group before - another stream - and only the last is waited for)
  bool one_launch = nz > 1 && !d->strong_by_frame && (d->N & 3) == 0 && rdk::strength_masks_group_fits(d->iw, s->label1, d->prev_ring, s->e8, zs);
  for (int i = 1; i < nz; i++) one_launch = one_launch && s[i].seq == s->seq + i;
  if (one_launch) {
    for (int i = 0; i < nz; i++) s[i].prev_in = d->prev_ring + (size_t)(s[i].seq % d->nring) * (size_t)d->N;
    rdk::strength_masks_group(st, d->prev_ring, s->e8, s->label1, s->strsum, d->t_edge, d->t_strong, d->iw, d->ih, s->strongbits, s->seq, d->nring, nz, zs);
    d->n_strong_group++;
  } else {
    for (int i = 0; i < nz; i++) frame_strong(d, &s[i], st);
    if (nz > 1) d->n_strong_by_frame++;
  }
  RD_HIP(hipEventRecord(s[nz - 1].ev_strong, st));
  d->last_strong = s[nz - 1].ev_strong; d->have_last_strong = 1;
  int rounds = d->fixed_rounds ? d->fixed_rounds : __atomic_load_n(&d->rounds_budget, __ATOMIC_RELAXED);
  if (d->budget_cycle) rounds = kRoundBudgets[2 + (int)((s->seq / d->budget_cycle) % (RD_NBUDGETS - 2))];      // (tests: a new graph every few frames)
  const int pm = current_poly_mode(d), bi = budget_index(rounds);
  for (int i = 0; i < nz; i++) { s[i].rounds = rounds; s[i].poly_mode = pm; d->budget_count[bi]++; }
  launch_captured(d, slot_graph(d, s, nz, 1 + 2 * bi + (d->batch == 1 ? pm : 0)), st, [&] { frame_segment(d, s, 2, st, nz, zs); });
  if (d->batch > 1) return;      // (votes, probes and rectangles follow with the batch's sparse stages)
  double tn = 0;
  const int with_post = aperture_snapshot(d, &tn) && d->device_post;
  if (with_post) rdk::post_device(st, s->frame, nz, d->maxrec_dev, d->iw, d->ih, tn);      // (outside the captured graphs: the aperture is a launch argument)
  for (int i = 0; i < nz; i++) { s[i].post_mode = with_post; s[i].post_tan = tn; }
}

// the polyline kind's: its one sequence, captured per polyline mode
static void poly_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  const size_t zs = nz > 1 ? d->slot_pitch : 0;
  const int pm = current_poly_mode(d);
  for (int i = 0; i < nz; i++) s[i].poly_mode = pm;
  launch_captured(d, slot_graph(d, s, nz, 1 + pm), st, [&] { poly_segment(d, s, nz, zs, st, pm); });
}

// the frame is on its way: its worker thread may start waiting for ev_done (which has been recorded by now - an event that was never
// recorded counts as complete)
static void slot_submitted(rd_detector *d, Slot *s) {
  if (d->nworkers > 0) {
    pthread_mutex_lock(&s->mu);
    s->state = 1;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
  }
}

// All launches of one frame (nz = 1, st = its slot's stream) or of the full group that slot s leads, for either detector kind.
// Group mode (rd_detector::zb > 1): the frames of zb consecutive slots in ONE set of launches, dense stages included (frame = blockIdx.z; the
// slots' planes lie slot_pitch bytes apart).  For frames so small that a launch does not fill the device (a 640x480 plane is 75 tiles for
// 256 CUs): the frame rate is then set by the number of launches the four hardware queues get through, and a group needs as many as a
// single frame.
static void launch_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  // (ONE pair of events brackets a group - its frames start and end together -, not one per frame: every record is a release fence in the stream)
  RD_HIP(hipEventRecord(s->ev_begin, st));
  for (int i = 0; i < nz; i++) { s[i].pending_dense = 0; s[i].watch_begin = s->ev_begin; s[i].watch_done = s->ev_done; s[i].group_n = nz; }
  // the colour conversion, outside the captured sequences: its source changes from frame to frame
  if (s->scale == 2) {      // (rd_detector_enqueue_scaled: the frames share format, scale and pitches)
    const uint8_t *planes[RD_ZB_MAX][3];
    for (int i = 0; i < nz; i++) for (int k = 0; k < 3; k++) planes[i][k] = s[i].pl[k];
    rdk::pix2plab_half_transposed(st, s->fmt, s->plab0, s->tr, planes, s->pitch, d->iw, d->ih, nz, nz > 1 ? d->slot_pitch : 0);
  } else if (s->fmt != RD_PIX_BGR) {      // (rd_detector_enqueue_planes: the frames share format and pitches)
    const uint8_t *planes[RD_ZB_MAX][3];
    for (int i = 0; i < nz; i++) for (int k = 0; k < 3; k++) planes[i][k] = s[i].pl[k];
    rdk::pix2plab_transposed(st, s->fmt, s->plab0, s->tr, planes, s->pitch, d->iw, d->ih, nz, nz > 1 ? d->slot_pitch : 0);
  } else if (nz == 1) rdk::bgr2plab_transposed(st, s->plab0, s->tr, s->src, d->iw, d->ih, s->ws);
  else {
    const uint8_t *srcs[RD_ZB_MAX];
    for (int i = 0; i < nz; i++) srcs[i] = s[i].src;
    rdk::bgr2plab_transposed(st, s->plab0, s->tr, srcs, d->iw, d->ih, s->ws, nz, d->slot_pitch);
  }
  if (d->kind == RD_KIND_POLY) poly_frames(d, s, nz, st); else rect_frames(d, s, nz, st);
  if (d->batch > 1) { RD_HIP(hipEventRecord(s->ev_dense, st)); s->pending_sparse = 1; }      // (ev_done: behind the batch's sparse stages, sparse_launch)
  else RD_HIP(hipEventRecord(s->ev_done, st));
  rdrt::check_launch(d->kind == RD_KIND_POLY ? "polyline frames" : "rect frames");
  if (d->batch == 1) for (int i = 0; i < nz; i++) slot_submitted(d, &s[i]);
}

// may two frames of a group share one front launch?  (one format, one scale, one set of row strides)
static bool same_layout(const Slot *a, const Slot *b) {
  if (a->fmt != b->fmt || a->scale != b->scale || a->ws != b->ws) return false;
  return a->fmt == RD_PIX_BGR || (a->pitch[1] == b->pitch[1] && a->pitch[2] == b->pitch[2]);
}

static hipStream_t group_stream(rd_detector *d, int g0) { return d->slots[(g0 / d->zb) % (d->nstreams > 0 ? d->nstreams : 1)].st; }

// the frames waiting in the group that starts at slot g0: all zb of them with one layout -> one set of launches; anything else (a poll
// that wants a result before the group is full, the end of a stream) -> frame by frame, the way a detector without groups launches them
static void group_launch(rd_detector *d, int g0) {
  const int g1 = g0 + d->zb < d->nslots ? g0 + d->zb : d->nslots;
  int cnt = 0;
  bool same = true, travelled = false;
  for (int i = g0; i < g1; i++) {
    const Slot *s = &d->slots[i];
    if (!s->pending_dense) continue;
    cnt++;
    same = same && same_layout(s, &d->slots[g0]);
    travelled = travelled || s->src == s->bgr || (s->sc_bgr && s->src == s->sc_bgr);
  }
  if (cnt == 0) return;
  // Host frames travelled when they were handed over, one after the other on the detector's upload stream (hand_over).  The launching thread waits for that
  // stream here - at most for the transfer just issued, 0.1 ms, on a thread that has nothing else to do until the next group completes - and what the host has seen
  // complete needs no ordering on the device: no event.  Round 6 found the 7-8 % that host frames cost against frames resident in HBM in exactly two places: an event
  // recorded after every upload (a record is a system-scope release, a write-back of the device's caches, 2 900 times a second in the middle of everybody's kernels:
  // 2671-2698 frames/s with it, 2886-2901 without) and - pinned frames, whose hand-over takes microseconds - eight transfers queued on the copy engine at once
  // (2701-2723 against 2849-2884 with one at a time).  profiles/NOTES_r06.md.
  if (travelled) RD_HIP(hipStreamSynchronize(d->st_upload));
  if (cnt == d->zb && same) { launch_frames(d, &d->slots[g0], d->zb, group_stream(d, g0)); return; }
  for (int i = g0; i < g1; i++) if (d->slots[i].pending_dense) launch_frames(d, &d->slots[i], 1, d->slots[i].st);
}

// Batched mode: the sparse stages of slots a..b (consecutive slots of one group, dense stages enqueued) as one set of launches on
// the stream of one of them - a different one each time, so that the extra ~0.4 ms of queue time does not always delay the same
// stream's next frame - behind the dense stages of all of them.
static void sparse_launch(rd_detector *d, int a, int b) {
  const int nb = b - a + 1;
  Slot *host = &d->slots[a + (int)(d->sparse_rot++ % (unsigned)nb)];
  hipStream_t st = host->st;
  for (int i = a; i <= b; i++) if (d->slots[i].st != st) RD_HIP(hipStreamWaitEvent(st, d->slots[i].ev_dense, 0));
  const int pm = current_poly_mode(d);
  const rdk::PolyFrame *frames = d->frames + a;
  rdk::polyline(st, frames, nb, d->N * 16, 1, 4.0f, 20, d->iw, d->ih, pm);
  double tn = 0;
  const int with_post = aperture_snapshot(d, &tn) && d->device_post;
  frames_votes(d, frames, nb, st, 1, with_post, tn);
  for (int i = a; i <= b; i++) {
    Slot *s = &d->slots[i];
    s->post_mode = with_post; s->post_tan = tn;
    s->poly_mode = pm;
    RD_HIP(hipEventRecord(s->ev_done, st));
    s->watch_done = s->ev_done;
    s->pending_sparse = 0;
  }
  rdrt::check_launch("rect frames, sparse stages");
  for (int i = a; i <= b; i++) slot_submitted(d, &d->slots[i]);
}

// launches what is pending in the group of slot si (a poll needs one of its frames, or the detector is drained)
static void sparse_flush(rd_detector *d, int si) {
  const int g0 = si / d->batch * d->batch, g1 = g0 + d->batch - 1 < d->nslots - 1 ? g0 + d->batch - 1 : d->nslots - 1;
  int a = -1, b = -1;
  for (int i = g0; i <= g1; i++) if (d->slots[i].pending_sparse) { if (a < 0) a = i; b = i; }
  if (a >= 0) sparse_launch(d, a, b);
  if (d->deferred_slot >= g0 && d->deferred_slot <= g1) d->deferred_slot = -1;
}

static void wait_event_outside_captures(rd_detector *d, hipEvent_t ev);
static void slot_fetch(Slot *s, void *dst, const void *src, size_t bytes);

// The ladder of a frame whose region merge was still changing in the last launch of its first budget: the region stages again with as many launches as it takes
// (32 first - the frames that exceed a budget of 12-14 need 13-20 as a rule, and every launch after the settling one still costs a dispatch of the whole grid -
// then 64, then the definition's limit of RD_REGION_MAX_LAUNCHES = 128: region_ladder_next).  still_after(budget) runs the stages with that budget and returns the
// flag of the budget's last launch.  The one decision of the frame path (slot_finish_device) and of the stage's test tap (rd_region_planes_device).
struct LadderEnd { int budget, settled; };      // the budget that was final; settled = 0: the frame keeps what RD_REGION_MAX_LAUNCHES launches made of it
template <typename F> static LadderEnd region_ladder(F still_after) {
  LadderEnd e = { 0, 0 };
  for (int budget = rdk::region_ladder_next(RD_REGION_FIRST_BUDGET); budget && !e.settled; budget = rdk::region_ladder_next(budget)) {
    e.budget = budget;
    e.settled = still_after(budget) == 0;
  }
  return e;
}

// What remains to be done on the device for a finished slot, once per frame (on the polling thread or on the slot's worker): the two
// rare repeats and the bookkeeping of the round budget.
static void slot_finish_device(rd_detector *d, Slot *s) {
  if (s->rounds <= RD_REGION_FIRST_BUDGET && s->h_ctr[32 + s->rounds - 1] != 0) {   // the region merge was still changing in its last launch: again with as many launches as it takes (region_ladder)
    // (on a stream of the slot's own: the slot's regular stream is one of the four that carry the groups, and the repeat would wait there behind a whole group of
    //  other frames; nothing but this frame's result depends on it - the frame is finished, ev_done has been waited for)
    static const bool redo_inline = RD_LAB_INT("RD_REDO_ON_MAIN_STREAM", 0) != 0;
    if (!s->st_redo && !redo_inline) s->st_redo = make_redo_stream();
    hipStream_t rst = redo_inline ? s->st : s->st_redo;
    const LadderEnd end = region_ladder([&](int budget) {
      s->rounds = budget;
      pthread_mutex_lock(&d->launch_mu);
      frame_regions(d, s, rst, 1, 0);
      redo_votes(d, s, rst);
      RD_HIP(hipEventRecord(s->ev_redo, rst));
      pthread_mutex_unlock(&d->launch_mu);
      wait_event_outside_captures(d, s->ev_redo);
      int still = 0;
      slot_fetch(s, &still, s->scratch2 + d->N + budget - 1, sizeof(int));      // the flag of the budget's last launch
      return still;
    });
    if (!end.settled) __atomic_add_fetch(&d->n_unsettled, 1, __ATOMIC_RELAXED);      // (the definition's limit: the frame keeps what that many launches made of it - counter 6)
    __atomic_add_fetch(&d->n_redo_rounds, 1, __ATOMIC_RELAXED);
  }
  if (s->h_ctr[52] != 0 || (d->force_redo & 2)) {   // the absorption's fast path gave up on this frame: finish it the long way
    frame_absorb_slow(d, s);
    __atomic_add_fetch(&d->n_redo_absorb, 1, __ATOMIC_RELAXED);
  }
  {   // budget for the frames to come (need = launches up to and including the first one that changed nothing)
    int need = 20;
    for (int r = 0; r < 20; r++) if (s->h_ctr[32 + r] == 0) { need = r + 1; break; }
    pthread_mutex_lock(&d->tan_mu);
    d->need_count[need]++;
    d->need_hist[d->need_pos++ & 63] = need;
    // what all but the three most demanding of the last 64 frames needed (a repeat costs a region stage, ~90 launches; a launch too many
    // costs 5 us in EVERY frame: on the bench stream 97 % of the frames need 9-11 launches, one in 150 needs 17 or more)
    int cnt[22] = { 0 }, seen = 0, mx = 20;
    for (int k = 0; k < 64; k++) cnt[d->need_hist[k] > 20 ? 20 : d->need_hist[k]]++;
    for (int v = 20; v >= 0; v--) { seen += cnt[v]; if (seen > 3) { mx = v; break; } }
    int b = 20;
    for (int k = RD_NBUDGETS - 1; k >= 0; k--) if (d->need_pos >= 8 && kRoundBudgets[k] >= mx + 1) b = kRoundBudgets[k];
    __atomic_store_n(&d->rounds_budget, b, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&d->tan_mu);
  }
  // two overflows among the stream's recent frames (whichever slots they ran in): its frames do not fit the single-launch kernel (e.g. 4K) - stop trying
  if (s->poly_mode == 1 && s->h_ctr[25] != 0 && __atomic_add_fetch(&d->overflow_streak, 1, __ATOMIC_RELAXED) >= 2) __atomic_store_n(&d->poly_overflows, 1, __ATOMIC_RELAXED);
  if (s->poly_mode == 1 && s->h_ctr[25] == 0) __atomic_store_n(&d->overflow_streak, 0, __ATOMIC_RELAXED);
  if ((s->poly_mode && s->h_ctr[25] != 0) || (d->force_redo & 1)) {   // the single-launch polyline stage overflowed: repeat the tail the long way
    s->post_mode = 0;
    pthread_mutex_lock(&d->launch_mu);
    frame_tail(d, s, 0);
    RD_HIP(hipEventRecord(s->ev_redo, s->st));
    pthread_mutex_unlock(&d->launch_mu);
    wait_event_outside_captures(d, s->ev_redo);
    __atomic_add_fetch(&d->n_redo, 1, __ATOMIC_RELAXED);
  }
}

// Waiting for an event from a thread that is not the enqueueing one.  Slots share streams, and the enqueueing thread records a new graph
// on a slot's stream whenever a (slot, launch budget) pair is used for the first time - in the middle of a run, since the budget of the
// region merge follows the stream.  HIP refuses hipEventSynchronize / hipEventQuery on an event whose stream is being captured ("operation
// not permitted on an event last recorded in a capturing stream"), so the wait is a poll whose queries exclude captures (launch_mu: held by
// launch_captured for the duration of a capture, a few hundred microseconds).
static void wait_event_outside_captures(rd_detector *d, hipEvent_t ev) {
  for (;;) {
    pthread_mutex_lock(&d->launch_mu);
    const hipError_t e = hipEventQuery(ev);
    pthread_mutex_unlock(&d->launch_mu);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) { RD_HIP(e); }
    struct timespec ts = { 0, 30000 };
    nanosleep(&ts, NULL);
  }
}

// device -> host copy for a slot whose device work is complete, from any thread: on the slot's private stream (never the legacy stream -
// a plain hipMemcpy would make that depend on a stream another thread may be capturing a graph on)
static void slot_fetch(Slot *s, void *dst, const void *src, size_t bytes) {
  if (!s->st_redo) s->st_redo = make_redo_stream();
  RD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->st_redo));
  RD_HIP(hipStreamSynchronize(s->st_redo));
}

// the list a poll returns from a result block of the device post-process (rd_k_post.hip: PolyFrame::post_out) that did not overflow: the
// valid candidates' records in candidate order, element 0 the header.  (Also what the test tap rd_postprocess_planes_device returns.)
static rect_t *post_block_rectangles(const int *h_post) {
  const int nc = h_post[0];
  const char *recs = (const char *)(h_post + 8 + RD_POST_MAXC);
  int nv = 0;
  for (int c = 0; c < nc; c++) nv += h_post[8 + c] != 0;
  rect_t *ret = (rect_t *)calloc((size_t)nv + 1, sizeof(rect_t));
  int at = 1;
  for (int c = 0; c < nc; c++) if (h_post[8 + c] != 0) memcpy(&ret[at++], recs + (size_t)c * sizeof(rect_t), sizeof(rect_t));
  ret[0].nItems = nv + 1;
  return ret;
}

// host post-process of a slot whose device work is complete: rectangles for the given aperture + a copy of the segment list
// (can run again for another aperture: touches nothing on the device but, for frames with very many segments, two copies)
static void *slot_rectangles(rd_detector *d, Slot *s, double tanAOV, void **segs_out, int *nsegs_out) {
  int n = ((int *)s->h_segs)[0];
  // the rectangles the device computed (rd_k_post.hip), if this frame has them for this aperture and nothing overflowed there:
  // the valid candidates' records in candidate order (= the reference's list order)
  if (s->post_mode && s->post_tan == tanAOV && s->h_post[1] == 0 && n + 1 <= d->maxrec_dev) {
    rect_t *ret = post_block_rectangles(s->h_post);
    // the segment list handed to rd_detector_last_segments: all n records, as on the host path - the pinned block holds the first
    // RD_MAXREC of them, a frame with more fetches the list from the device
    void *copy0 = malloc((size_t)(n + 1) * 56);
    if (n + 1 <= RD_MAXREC) memcpy(copy0, s->h_segs, (size_t)(n + 1) * 56);
    else slot_fetch(s, copy0, s->lslist, (size_t)(n + 1) * 56);
    *segs_out = copy0; *nsegs_out = n;
    __atomic_add_fetch(&d->n_post_device, 1, __ATOMIC_RELAXED);
    return ret;
  }
  __atomic_add_fetch(&d->n_post_host, 1, __ATOMIC_RELAXED);
  const void *segs = s->h_segs; const int *probes = s->h_probes;
  void *big_segs = NULL; int *big_probes = NULL;
  int maxrec = d->maxrec_dev < RD_MAXREC ? d->maxrec_dev : RD_MAXREC;
  if (n + 1 > maxrec) {   // rare: more segments than the fixed-size transfer covers
    const int *dev_probes = s->probes;
    if (n + 1 > d->maxrec_dev) {
      // more records than the slot's probe buffer holds (the list itself has the reference's capacity, 16N / 56 records, pl:456): the
      // probes of all of them are taken again into a buffer that grows on demand - nothing is ever dropped
      if (!s->st_redo) s->st_redo = make_redo_stream();
      if (s->big_probes_cap < n + 1) { dfree(s->big_probes); s->big_probes = dnew<int>((size_t)(n + 1) * 15 * 6); s->big_probes_cap = n + 1; }
      rdk::PolyFrame f = *s->frame;
      f.probes = s->big_probes; f.pack = NULL;
      rdk::sample_segments(s->st_redo, &f, 1, n + 1, d->iw, d->ih, d->N * 4 / 5, 0);
      rdrt::check_launch("probes of a frame with very many segments");
      dev_probes = s->big_probes;
      __atomic_add_fetch(&d->n_truncated, 1, __ATOMIC_RELAXED);      // (counter 10: frames that took this path)
    }
    big_segs = malloc((size_t)(n + 1) * 56); big_probes = (int *)malloc((size_t)(n + 1) * 15 * 6 * sizeof(int));
    slot_fetch(s, big_segs, s->lslist, (size_t)(n + 1) * 56);
    slot_fetch(s, big_probes, dev_probes, (size_t)(n + 1) * 15 * 6 * sizeof(int));
    segs = big_segs; probes = big_probes; maxrec = n + 1;
  }
  // RD_DIAG_NO_POST (diagnostics only): an empty rectangle list instead of the host post-process, to see whether a run is host-bound
  struct timespec tp0, tp1;
  clock_gettime(CLOCK_MONOTONIC, &tp0);
  void *r = rd_post_run(segs, maxrec, probes, d->iw, d->ih, tanAOV);
  clock_gettime(CLOCK_MONOTONIC, &tp1);
  __atomic_add_fetch(&d->host_post_ns, (tp1.tv_sec - tp0.tv_sec) * 1000000000L + (tp1.tv_nsec - tp0.tv_nsec), __ATOMIC_RELAXED);
  const int ns = n < maxrec ? n : maxrec - 1;
  void *copy = malloc((size_t)(ns + 1) * 56);
  memcpy(copy, segs, (size_t)(ns + 1) * 56);
  free(big_segs); free(big_probes);
  *segs_out = copy; *nsegs_out = ns;
  return r;
}

static void *slot_worker(void *arg) {
  Slot *s = (Slot *)arg;
  rd_detector *d = s->owner;
  RD_HIP(hipSetDevice(d->device));
  for (;;) {
    pthread_mutex_lock(&s->mu);
    while (s->state != 1 && !s->quit) pthread_cond_wait(&s->cv, &s->mu);
    if (s->quit) { pthread_mutex_unlock(&s->mu); return NULL; }
    pthread_mutex_unlock(&s->mu);
    // the aperture arrives with the poll (reference API); workers run ahead with the last one seen
    pthread_mutex_lock(&d->tan_mu);
    while (!d->have_tan && !s->quit) pthread_cond_wait(&d->tan_cv, &d->tan_mu);
    const double tan = d->tan_aov;
    pthread_mutex_unlock(&d->tan_mu);
    if (s->quit) return NULL;
    // Frames finish roughly in sequence order, and the caller collects them in that order: only the workers of the frames next in line watch their event
    // closely (a query every 30 us); the others - with 64 frames in flight, most of them, for most of the 25 ms their frame spends on the device - sleep in
    // longer steps until the front of finished frames comes within two groups of theirs.  (All of them polling was two million event queries a second
    // through the runtime's locks, next to the thread that launches.)
    {
      const long window = 2L * (d->zb > 1 ? d->zb : 4);
      while (!s->quit && s->seq >= __atomic_load_n(&d->done_seq, __ATOMIC_RELAXED) + window) { struct timespec ts = { 0, 250000 }; nanosleep(&ts, NULL); }
    }
    wait_event_outside_captures(d, s->watch_done);
    { long cur = __atomic_load_n(&d->done_seq, __ATOMIC_RELAXED); while (cur < s->seq + 1 && !__atomic_compare_exchange_n(&d->done_seq, &cur, s->seq + 1, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { } }
    void *segs = NULL; int ns = 0;
    slot_finish_device(d, s);
    void *r = slot_rectangles(d, s, tan, &segs, &ns);
    pthread_mutex_lock(&s->mu);
    s->result = r; s->result_tan = tan; s->res_segs = segs; s->res_nsegs = ns;
    s->state = 2;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
  }
}

// ---- detector set-up: what rd_detector_create and rd_polyline_detector_create share (the argument checks stay with their entry point)
static rd_detector *detector_new(int kind, int device, int iw, int ih, int nslots, int nworkers) {
  RD_HIP(hipSetDevice(device));
  rd_detector *d = (rd_detector *)calloc(1, sizeof(*d));
  d->magic = MAGIC_RECT; d->kind = kind; d->device = device; d->iw = iw; d->ih = ih; d->N = iw * ih; d->nslots = nslots; d->nworkers = nworkers;
  d->maxrec_dev = d->N * 16 / 56;
  if (d->maxrec_dev > 65536) d->maxrec_dev = 65536;      // the slots' probe buffers; frames with more records are probed again into a buffer that grows (slot_rectangles)
  { const int m = rd_env_int("RD_MAXREC_DEV", 0); if (m >= 16 && m < d->maxrec_dev) d->maxrec_dev = m; }      // (tests: exercise that path)
  d->use_graph = rd_env("RD_NO_GRAPH") ? 0 : 1;
  d->poly_mode = rd_env("RD_POLY_MULTILAUNCH") ? 0 : 1;      // (tests: the ~85-launch form for every frame)
  d->force_redo = (rd_env("RD_POLY_FORCE_REDO") ? 1 : 0) | (rd_env("RD_ABSORB_FORCE_SLOW") ? 2 : 0);   // tests: every frame also takes the polyline / absorption fallback
  // The single-block polyline kernel holds 16 384 live chain pixels; a 1920x1080 frame of the synthetic streams has ~11 000, frames of 3 megapixels and
  // more are beyond it as a rule: their streams start on the multi-launch form instead of overflowing - and being repeated - until the two-overflow rule
  // (slot_finish_device, rd_detector_poll_segments) finds that out (3840x2160: 12 of the first 16 frames).  Smaller frames that overflow anyway are still caught by that rule.
  d->poly_overflows = (long)iw * ih > 3000000L ? 1 : 0;
  d->batch = 1; d->deferred_slot = -1; d->last_polled_slot = -1;
  pthread_mutex_init(&d->tan_mu, NULL); pthread_cond_init(&d->tan_cv, NULL);
  pthread_mutex_init(&d->launch_mu, NULL);
  d->slots = (Slot *)calloc((size_t)nslots, sizeof(Slot));
  d->frames = (rdk::PolyFrame *)calloc((size_t)nslots, sizeof(rdk::PolyFrame));
  return d;
}

// streams, group mode, planes and slots, once the kind's own settings (fork_poly, batch) stand
static void detector_slots(rd_detector *d, int nstreams) {
  const int nslots = d->nslots;
  // One stream per frame: the frames beyond the fourth queue up behind earlier ones on the same four streams (slot i uses the
  // streams of slot i mod 4) - a stream of its own would be time-sliced onto the same four hardware queues and stall frames
  // that have nothing to do with each other, while a queued frame keeps its queue busy as soon as its predecessor is done
  // (the host's turn-around between "frame polled" and "next frame enqueued" otherwise idles a quarter of the device).
  d->nstreams = nstreams < nslots ? nstreams : nslots;
  // Group mode: four frames per launch from twelve frame slots on (three groups: one being filled, two in flight), two from six on, eight from 32 on
  // (640x480: 9100 frames/s with 16 slots in groups of four, 11700 with 32 in groups of eight; 1080p: no difference);
  // RD_ZBATCH=k overrides (k frames per launch, 2..8; 0 / 1: off).
  d->zb = nslots >= 32 ? 8 : (nslots >= 12 ? 4 : (nslots >= 6 ? 2 : 1));      // (always at least three or four groups: one being filled, the others in flight on the four streams)
  if ((long long)d->iw * d->ih > 1920ll * 1088) d->zb = 1;      // (launches of larger frames fill the device on their own: 3840x2160 measured 1 % slower in groups)
  if (rd_env("RD_ZBATCH")) { const int z = rd_env_int("RD_ZBATCH", 1); d->zb = z < 1 ? 1 : (z > RD_ZB_MAX ? RD_ZB_MAX : z); }
  if (d->fork_poly || d->zb > nslots) d->zb = 1;
  if (d->zb > 1) { d->batch = 1; d->defer = 0; }      // (a group's sparse stages follow its dense stages on the same stream)
  d->slot_pitch = slot_planes(d, NULL, NULL);
  d->arena = dnew<char>((size_t)nslots * d->slot_pitch);
  for (int i = 0; i < nslots; i++) {
    Slot *s = &d->slots[i];
    slot_alloc(d, s, (!d->fork_poly && i >= nstreams) ? &d->slots[i % nstreams] : NULL);
    s->owner = d;
    pthread_mutex_init(&s->mu, NULL); pthread_cond_init(&s->cv, NULL);
    if (d->nworkers > 0 && pthread_create(&s->th, NULL, slot_worker, s) != 0) exitf(-1, "rd_detector_create: cannot start worker thread\n");
  }
  if (d->kind == RD_KIND_RECT) rdk::quant_lut_init(d->slots[0].st);
  RD_HIP(hipDeviceSynchronize());
}

static void slot_destroy_graphs(Slot *s) {
  for (int g = 0; g < 2; g++) for (int k = 0; k < RD_NSEQ; k++) if (s->graphs[g][k]) { RD_HIP(hipGraphExecDestroy(s->graphs[g][k])); s->graphs[g][k] = NULL; }
}

extern "C" {

rd_detector *rd_detector_create(int device, int iw, int ih, int nslots, int nworkers) {
  if (rd_device_count() <= 0) exitf(-1, "rd_detector_create: no HIP device available - this library has no CPU path\n");
  if (iw < 16 || ih < 16) exitf(-1, "rd_detector_create: frame %dx%d too small\n", iw, ih);
  if ((long long)iw * ih >= (1ll << 25)) exitf(-1, "rd_detector_create: frame %dx%d too large (pixel indices are kept below 2^25: hash keys and marked label words rely on the spare bits)\n", iw, ih);
  if (nslots < 1) nslots = 1;
  rd_detector *d = detector_new(RD_KIND_RECT, device, iw, ih, nslots, nworkers);
  d->nring = nslots + 1;
  d->prev_ring = dnew<int8_t>((size_t)d->N * d->nring);
  RD_HIP(hipMemset(d->prev_ring, 0, (size_t)d->N * d->nring));
  // candidate funnel + pose estimation on the device (rd_k_post.hip) instead of on one worker thread per frame slot: RD_DEVICE_POST=0|1 decides;
  // otherwise the host path - 0.3 ms of CPU time per 1080p frame, i.e. 0.6 of a core at 2000 frames/s: measured 2050 frames/s on 8 cores
  // as on 256, against 1830 for the device path - unless this process may run on one or two cores only
  if (rd_env("RD_DEVICE_POST")) d->device_post = rd_env_int("RD_DEVICE_POST", 0) != 0;
  else {
    cpu_set_t set;
    const int ncpu = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
    d->device_post = (nworkers > 0 && ncpu > 0 && ncpu <= 2) ? 1 : 0;
  }
  // The device runs four hardware queues side by side (more are time-sliced: measured 2x slower per frame).  With one or two
  // frames in flight a frame spreads over two streams (polyline chain beside the blur chain: shortest latency); from three
  // frames on every frame keeps to one stream, so that four frames occupy the four queues (highest throughput).
  d->fork_poly = nslots <= 2 ? 1 : 0;
  if (RD_LAB_INT("RD_FORK_POLY", 1) == 0) d->fork_poly = 0;      // (measurements: one stream per frame with one or two in flight as well)
  // One or two frames in flight and no worker threads = the reference's call sequence (executeOnce, enqueueTask / pollTask): the caller's thread runs the
  // post-process at the end of every frame's latency; helper threads share its pose estimations (rd_post.c), RD_POST_HELPERS=n overrides their number
  d->post_helpers = 0;
  if (nworkers == 0 && nslots <= 2) {
    cpu_set_t set;
    const int ncpu = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
    d->post_helpers = rd_env_int("RD_POST_HELPERS", ncpu >= 16 ? 4 : (ncpu >= 8 ? 2 : (ncpu >= 4 ? 1 : 0)));      // (1 / 3 / 5 / 7 helpers: 1.19 / 1.14-1.20 / 1.11 / 1.12-1.20 ms per executeOnce against 1.28 without)
    if (d->post_helpers > 0) rd_post_helpers_configure(d->post_helpers);
  }
  // round budget of the region merge: what the last 64 frames needed + margin (8 / 12 / 16 / 20 launched rounds; the rounds after
  // the merge has settled are no-ops, but each still costs two launches of a thousand blocks), frames that turn out to need more
  // are repeated with all 20; RD_REGION_ROUNDS_FIXED=8|12|16|20 pins the budget (20: never repeat anything).
  d->fixed_rounds = 0;
  if (rd_env("RD_REGION_ROUNDS_FIXED")) { const int r = rd_env_int("RD_REGION_ROUNDS_FIXED", 20); d->fixed_rounds = (r >= 8 && r <= 20 && !(r & 1)) ? r : 20; }
  d->rounds_budget = 20;
  d->t_edge = 500; d->t_strong = 2500;      // oclrect.c:277-284, 307-313
  if (rd_env("RD_TEST_THRESHOLDS")) {      // tests only: other thresholds, so that many strength sums stand exactly one below one (where the mask of the frame before decides, H1)
    int a = 0, b = 0;
    if (sscanf(rd_env("RD_TEST_THRESHOLDS"), "%d,%d", &a, &b) == 2 && a > 0 && b >= a) { d->t_edge = a; d->t_strong = b; }
  }
  d->strong_by_frame = rd_env("RD_STRONG_BY_FRAME") ? 1 : 0;
  d->budget_cycle = rd_env_int("RD_BUDGET_CYCLE", 0);      // tests: the launch budget changes every so many frames (12, 14, .. 20, 12, ..)
  // frames per set of sparse-stage launches: 4 from twelve frames in flight on - the deferral by one group below needs a third group of
  // slots to keep the streams fed, and without it a batch is a barrier per group (measured 10 % slower than no batching) - else every
  // frame on its own; RD_BATCH=1..4 overrides (tests: batching with any slot count)
  d->batch = nslots >= 24 ? 8 : (nslots >= 12 ? 4 : 1);      // (these stages are latency-bound chains of gathers: eight frames take a launch as long as four)
  if (rd_env("RD_BATCH")) { const int b = rd_env_int("RD_BATCH", 1); d->batch = b < 1 ? 1 : (b > RD_MAXB ? RD_MAXB : b); }
  if (d->fork_poly || d->batch > nslots) d->batch = d->fork_poly ? 1 : nslots;
  d->defer = (d->batch > 1 && nslots >= 3 * d->batch) ? 1 : 0;       // needs a third group of slots to keep the streams fed meanwhile
  const int nstreams = RD_LAB_INT("RD_NSTREAMS", 4) < 1 ? 1 : (RD_LAB_INT("RD_NSTREAMS", 4) > 8 ? 8 : RD_LAB_INT("RD_NSTREAMS", 4));      // (measurements only - 3 / 5 / 6 streams: 2776-2786 / 2746-2753 / 2827-2847 frames/s against 2881-2889 with four, one box)
  detector_slots(d, nstreams);
  return d;
}

void rd_detector_destroy(rd_detector *d) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_destroy: bad handle\n");
  RD_HIP(hipSetDevice(d->device));
  RD_HIP(hipDeviceSynchronize());
  for (int i = d->nslots - 1; i >= 0; i--) {      // (slots that borrowed streams go before the slots that own them)
    Slot *s = &d->slots[i];
    if (d->nworkers > 0) {
      pthread_mutex_lock(&s->mu); s->quit = 1; pthread_cond_broadcast(&s->cv); pthread_mutex_unlock(&s->mu);
      pthread_mutex_lock(&d->tan_mu); pthread_cond_broadcast(&d->tan_cv); pthread_mutex_unlock(&d->tan_mu);
      pthread_join(s->th, NULL);
    }
    free(s->result); free(s->res_segs);
    slot_destroy_graphs(s);
    slot_free(s, d->device);
  }
  if (d->st_upload) { RD_HIP(hipStreamSynchronize(d->st_upload)); unpool_stream(d->device, d->st_upload); }
  free(d->slots);
  free(d->frames);
  dfree(d->prev_ring);
  dfree(d->arena);
  free(d->last_segs);
  d->magic = 0;
  free(d);
}

// ---- hand-over of a frame (rd_detector_enqueue, rd_detector_enqueue_planes)
// The planes a format uses and the layout of a host frame packed into a slot's buffers: rd_jobs.h.
using rdjob::PixLayout;
using rdjob::pix_layout;
// a BGR frame of rd_detector_enqueue keeps the caller's row stride on its way through the slot's buffers: one plane of ws * ih bytes
static PixLayout bgr_layout(int ws, int ih) {
  PixLayout L;
  memset(&L, 0, sizeof(L));
  L.np = 1; L.row[0] = L.pitch[0] = ws; L.rows[0] = ih; L.bytes = (size_t)ws * ih;
  return L;
}

// a pageable frame's way to the device: pieces (byte ranges of the packed layout) gathered from the caller's planes into pinned memory by the caller and whichever
// helper threads are awake, uploaded in order as they complete
struct UploadJob { PixLayout L; const uint8_t *src[3]; int spitch[3]; char *dst, *dev; size_t piece; hipStream_t st; int n, uploaded; int ready[16]; };
static void pack_range(const UploadJob *j, size_t o, size_t end) {
  for (int k = 0; k < j->L.np; k++) {
    const size_t p0 = j->L.off[k], pp = (size_t)j->L.pitch[k];
    const size_t a = o > p0 ? o : p0, b = end < p0 + pp * j->L.rows[k] ? end : p0 + pp * j->L.rows[k];
    if (a >= b) continue;
    if (j->spitch[k] == j->L.pitch[k] && j->L.row[k] == j->L.pitch[k]) { rd_copy_to_staging(j->dst + a, j->src[k] + (a - p0), b - a); continue; }      // (the caller's plane is laid out as the packed one - a BGR frame always: one copy)
    for (size_t r = (a - p0) / pp, at = a; at < b; r++) {      // rows of plane k that meet [a, b)
      const size_t rs = p0 + r * pp, re = rs + (size_t)j->L.row[k];
      const size_t c0 = at > rs ? at : rs, c1 = b < re ? b : re;
      if (c0 < c1) rd_copy_to_staging(j->dst + c0, j->src[k] + r * j->spitch[k] + (c0 - rs), c1 - c0);
      at = rs + pp;
    }
  }
}
static void pack_copy_piece(void *ctx, int i) {
  UploadJob *u = (UploadJob *)ctx;
  const size_t o = (size_t)i * u->piece, m = u->L.bytes - o < u->piece ? u->L.bytes - o : u->piece;
  pack_range(u, o, o + m);
  __atomic_store_n(&u->ready[i], 1, __ATOMIC_RELEASE);
}
static void upload_progress(void *ctx) {      // (caller's thread only)
  UploadJob *u = (UploadJob *)ctx;
  int e = u->uploaded;
  while (e < u->n && __atomic_load_n(&u->ready[e], __ATOMIC_ACQUIRE)) e++;
  if (e == u->uploaded) return;
  const size_t o = (size_t)u->uploaded * u->piece, end = (size_t)e * u->piece < u->L.bytes ? (size_t)e * u->piece : u->L.bytes;
  RD_HIP(hipMemcpyAsync(u->dev + o, u->dst + o, end - o, hipMemcpyHostToDevice, u->st));
  u->uploaded = e;
}

// is this host buffer page-locked (allocatePinnedMemory of oclhelper.h, rd_host_alloc, hipHostMalloc, hipHostRegister)?  One question to the runtime per buffer, not per frame.
static bool host_buffer_is_pinned(rd_detector *d, const void *frame) {
  for (int k = 0; k < 2; k++) if (d->probed[k] == frame) return d->probed_pinned[k] != 0;
  const bool pinned = rdjob::memory_type(frame) == hipMemoryTypeHost;
  d->probed[1] = d->probed[0]; d->probed_pinned[1] = d->probed_pinned[0];
  d->probed[0] = frame; d->probed_pinned[0] = pinned ? 1 : 0;
  return pinned;
}

// what follows the hand-over of a frame: its launches - now, or with its group - and the caller's wait for the copy engine
static long enqueue_launch(rd_detector *d, Slot *s, Slot *wait_upload, struct timespec ts0) {
  const int si = (int)(s - d->slots);
  if (d->zb > 1) {      // group mode: launched together with the other frames of its group, once that is full (or a poll needs one of them)
    s->pending_dense = 1;
    // (the last group of slots may be short - nslots need not be a multiple of zb - and is launched when ITS last slot is filled: every group
    //  is launched the moment its last frame arrives, so frames reach the device in sequence order and at most one group is ever waiting)
    if (si % d->zb == d->zb - 1 || si == d->nslots - 1) group_launch(d, si / d->zb * d->zb);
  } else {
    launch_frames(d, s, 1, s->st);
    if (d->batch > 1 && (si % d->batch == d->batch - 1 || si == d->nslots - 1)) {      // the batch is complete
      // Launched right away, the sparse stages would sit in their stream between this group's dense stages and the next one's, waiting
      // for the slowest of the group's four streams: a barrier per group (measured: 10 % slower than no batching).  One group later,
      // everything they wait for is long done and the stream they land on has the next group's dense work queued in front of them.
      if (d->defer) {
        const int prev = d->deferred_slot;
        d->deferred_slot = si;
        if (prev >= 0) sparse_flush(d, prev);
      } else sparse_flush(d, si);
    }
  }
  if (wait_upload) RD_HIP(hipEventSynchronize(wait_upload->ev_upload));      // (the caller may touch its buffer again)
  { struct timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1); d->host_enqueue_ns += (ts1.tv_sec - ts0.tv_sec) * 1000000000L + (ts1.tv_nsec - ts0.tv_nsec); }
  return d->next_enqueue++;
}

// The next slot takes a frame - format, planes and row strides as the entry point `who` checked them; L: the layout a host frame is packed into - and launches it.
// The BGR frames of rd_detector_enqueue and the frames of the other formats differ in three places, each a condition on fmt below; none of them has been measured the other way.
// scale 2 (rd_detector_enqueue_scaled): planes, pitches and L describe the source frame of 2 iw x 2 ih pixels; a host frame then travels through the slot's
// scaled-source staging (sc_h / sc_bgr, allocated here with the slot's first such frame - the slot is idle: its last frame has been polled) on the same paths.
static long hand_over(rd_detector *d, const char *who, int fmt, const void *const planes[3], const int pitches[3], const PixLayout &L, int on_device, int scale = 1) {
  if (d->next_enqueue - d->next_poll >= d->nslots) exitf(-1, "%s: %d frames already in flight (poll first)\n", who, d->nslots);
  RD_HIP(hipSetDevice(d->device));
  struct timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
  Slot *s = &d->slots[d->next_enqueue % d->nslots];
  s->seq = d->next_enqueue; s->fmt = fmt; s->scale = scale;
  for (int k = 0; k < 3; k++) { s->pl[k] = NULL; s->pitch[k] = 0; }
  if (scale == 2 && on_device != RD_FRAME_DEVICE && !s->sc_bgr) {
    s->sc_bytes = pix_layout(RD_PIX_BGRA, 2 * d->iw, 2 * d->ih).bytes;      // (16 bytes per detector pixel: the largest of the six layouts)
    RD_HIP(hipMalloc((void **)&s->sc_bgr, s->sc_bytes));
    RD_HIP(hipHostMalloc(&s->sc_h, s->sc_bytes, hipHostMallocDefault));
  }
  uint8_t *const dbuf = scale == 2 ? s->sc_bgr : s->bgr;      // a host frame's way: pinned staging hbuf (pageable frames only), device copy dbuf
  void *const hbuf = scale == 2 ? s->sc_h : s->h_bgr;
  Slot *wait_upload = NULL;
  const bool group = d->zb > 1;
  if (on_device == RD_FRAME_DEVICE) {      // read where they lie (the caller keeps them valid until the frame's poll returned)
    for (int k = 0; k < L.np; k++) { s->pl[k] = (const uint8_t *)planes[k]; s->pitch[k] = pitches[k]; }
  } else {      // host frames: through the slot's buffers, one plane after the other
    for (int k = 0; k < L.np; k++) { s->pl[k] = dbuf + L.off[k]; s->pitch[k] = L.pitch[k]; }
    // Group mode: the frame travels NOW, on a stream of the detector's own (high-priority pool: a hardware queue nobody computes on), not when its group is launched:
    // eight uploads in front of a group's kernels kept that group's stream - a quarter of the device's queues - waiting for the copy engine for 1.6 of its 10.8 ms; and
    // an ordinary stream shares a hardware queue with a group's: 2786-2796 frames/s, the caller waiting 0.35 ms per frame.  No event: group_launch waits for the stream.
    hipStream_t ust = s->st;
    if (group) { if (!d->st_upload) d->st_upload = pooled_stream(d->device); ust = d->st_upload; }
    if (on_device == RD_FRAME_HOST_PINNED) {
      // The caller's planes are page-locked and stay as they are until the frame's poll: the copy engine takes them from there.  (The reference copies every frame into its own
      // pinned page first, oclrect.c:1256 - 6 MB per 1920x1080 frame by the caller's thread, 16 GB/s at full rate on the thread that also launches everything.)
      for (int k = 0; k < L.np; k++) {
        const void *lo = planes[k], *hi = (const char *)planes[k] + (size_t)pitches[k] * (L.rows[k] - 1) + L.row[k];
        bool known = false;      // (one look per range, not per frame: a capture loop reuses its pages)
        for (int e = 0; e < 4 && !known; e++) known = lo >= d->pinned[e][0] && hi <= d->pinned[e][1];
        if (known) continue;
        if (rdjob::memory_type(planes[k]) != hipMemoryTypeHost) { exitf(-1, "%s: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", who, k, planes[k]); }
        const unsigned e = d->pinned_next++ & 3;
        d->pinned[e][0] = lo; d->pinned[e][1] = hi;
      }
      // (The colour conversion reading the pinned buffer over PCIe itself, without the copy engine: 1985-2009 frames/s against 2656-2659 - the kernel then runs at the link's
      //  rate, a millisecond per group, with its blocks resident all the while.  profiles/NOTES_r06.md.)
      if (group) RD_HIP(hipStreamSynchronize(ust));      // (one transfer in the copy engine's queue at a time: the caller waits for the frame before - 0.1 ms where it used to copy for 0.16 - see group_launch)
      for (int k = 0; k < L.np; k++) {
        if (pitches[k] == L.row[k] && L.row[k] == L.pitch[k]) RD_HIP(hipMemcpyAsync(dbuf + L.off[k], planes[k], (size_t)L.row[k] * L.rows[k], hipMemcpyHostToDevice, ust));
        else RD_HIP(hipMemcpy2DAsync(dbuf + L.off[k], L.pitch[k], planes[k], pitches[k], L.row[k], L.rows[k], hipMemcpyHostToDevice, ust));
      }
      d->n_frames_pinned++;
    } else if (!group && fmt == RD_PIX_BGR && scale == 1 && host_buffer_is_pinned(d, planes[0])) {      // (only rd_detector_enqueue's frames ask)
      // The reference's call shape (oclrect_enqueueTask / executeOnce) on a buffer that happens to be page-locked - allocatePinnedMemory of oclhelper.h hands such memory out
      // (oclhelper.c:837-851, poly.cpp:68-69): the copy engine reads it in place, nothing is copied by the caller's thread, and the frame's kernels are launched behind the
      // transfer at once.  The reference's contract - the caller may reuse the buffer as soon as the call returns (oclrect.c:1256 copies it) - is kept by returning only when
      // the engine has read it: waited for at the END of this call (enqueue_launch), after the frame's ~45 launches, by which time it has long happened (6 MB in 0.12 ms).
      RD_HIP(hipMemcpyAsync(s->bgr, planes[0], L.bytes, hipMemcpyHostToDevice, s->st));
      RD_HIP(hipEventRecord(s->ev_upload, s->st));
      wait_upload = s;
      d->n_frames_pinned++;
    } else {
      d->n_frames_copied++;
      UploadJob u;
      u.L = L; u.dst = (char *)hbuf; u.dev = (char *)dbuf; u.st = ust; u.uploaded = 0;
      for (int k = 0; k < 3; k++) { u.src[k] = (const uint8_t *)planes[k]; u.spitch[k] = pitches[k]; }
      if (group) {      // the caller's thread packs, then the frame travels at once
        pack_range(&u, 0, L.bytes);
        if (fmt != RD_PIX_BGR || scale != 1) RD_HIP(hipStreamSynchronize(ust));      // (one transfer queued at a time, as the pinned frames'; a BGR frame's upload is queued behind the one before without this wait)
        RD_HIP(hipMemcpyAsync(dbuf, hbuf, L.bytes, hipMemcpyHostToDevice, ust));
      } else {
        // a single frame: the copy into pinned memory and the upload in pieces, so that a piece travels while the next is being copied (6 MB at 1920x1080:
        // the copy alone takes a fifth of a millisecond of the caller's latency).  With helper threads (armed here: the call that hands a frame over is followed by
        // the poll that waits for one) the pieces are copied side by side and uploaded in order as they complete.
        const bool helpers = d->post_helpers > 0;
        if (helpers) rd_post_helpers_arm();
        const int npieces = helpers ? 16 : 4;
        u.piece = ((L.bytes + npieces - 1) / npieces + 4095) & ~(size_t)4095;
        u.n = (int)((L.bytes + u.piece - 1) / u.piece);      // (<= npieces)
        for (int i = 0; i < u.n; i++) u.ready[i] = 0;
        rd_helpers_run(pack_copy_piece, &u, u.n, upload_progress);
        upload_progress(&u);
        if (u.uploaded != u.n) exitf(-1, "%s: internal error (pieces of the frame left behind)\n", who);
      }
    }
  }
  s->src = s->pl[0]; s->ws = s->pitch[0];
  return enqueue_launch(d, s, wait_upload, ts0);
}

long rd_detector_enqueue(rd_detector *d, const void *frame, int ws, int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue: bad handle\n");
  if ((size_t)ws * d->ih > (size_t)d->N * 4) exitf(-1, "rd_detector_enqueue: row stride %d too large for a %dx%d frame\n", ws, d->iw, d->ih);
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) exitf(-1, "rd_detector_enqueue: on_device = %d (0: host memory, 1: device memory, 2: pinned host memory)\n", on_device);
  const void *const planes[3] = { frame, NULL, NULL };
  const int pitches[3] = { ws, 0, 0 };
  return hand_over(d, "rd_detector_enqueue", RD_PIX_BGR, planes, pitches, bgr_layout(ws, d->ih), on_device);
}

long rd_detector_enqueue_planes(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue_planes: bad handle\n");
  // argument errors: -1, nothing enqueued
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  if (rdpix::is_yuv(format) && ((d->iw | d->ih) & 1)) return -1;
  const PixLayout L = pix_layout(format, d->iw, d->ih);
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  if (format == RD_PIX_BGR) return rd_detector_enqueue(d, planes[0], pitches[0], on_device);
  return hand_over(d, "rd_detector_enqueue_planes", format, planes, pitches, L, on_device);
}

long rd_detector_enqueue_scaled(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int scale, int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue_scaled: bad handle\n");
  if (scale == 1) return rd_detector_enqueue_planes(d, format, planes, pitches, on_device);
  // argument errors: -1, nothing enqueued
  if (scale != 2) return -1;
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  const PixLayout L = pix_layout(format, 2 * d->iw, 2 * d->ih);      // (the source frame: even in both directions, whatever iw and ih are)
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  return hand_over(d, "rd_detector_enqueue_scaled", format, planes, pitches, L, on_device, 2);
}

// device time of a polled frame (counters 1 and 2): the interval its events bracket - a group's is shared by its frames: each counts its part
static void count_device_time(rd_detector *d, const Slot *s) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s->watch_begin, s->watch_done) == hipSuccess) { d->dev_us += (long)(ms * 1000.0f) / (s->group_n > 0 ? s->group_n : 1); d->dev_frames++; }
}

void *rd_detector_poll(rd_detector *d, double tanAOV) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_poll: bad handle\n");
  if (d->kind == RD_KIND_POLY) exitf(-1, "rd_detector_poll: this is a polyline detector (rd_polyline_detector_create) - its results come from rd_detector_poll_segments\n");
  if (d->next_poll >= d->next_enqueue) exitf(-1, "rd_detector_poll: nothing enqueued\n");
  RD_HIP(hipSetDevice(d->device));
  const int si = (int)(d->next_poll % d->nslots);
  Slot *s = &d->slots[si];
  void *r = NULL, *segs = NULL; int ns = 0;
  if (s->pending_sparse) sparse_flush(d, si);       // (an incomplete group: the caller wants a result before handing over more frames)
  if (s->pending_dense) group_launch(d, si / d->zb * d->zb);
  pthread_mutex_lock(&d->tan_mu);
  d->tan_aov = tanAOV; d->have_tan = 1;            // what workers and the device post-process of later frames run ahead with
  pthread_cond_broadcast(&d->tan_cv);
  pthread_mutex_unlock(&d->tan_mu);
  if (d->nworkers > 0) {
    pthread_mutex_lock(&s->mu);
    while (s->state != 2) pthread_cond_wait(&s->cv, &s->mu);
    r = s->result; segs = s->res_segs; ns = s->res_nsegs;
    const double used = s->result_tan;
    s->result = NULL; s->res_segs = NULL; s->state = 0;
    pthread_mutex_unlock(&s->mu);
    if (used != tanAOV) {      // the worker ran ahead with another aperture: redo with the requested one
      free(r); free(segs);
      r = slot_rectangles(d, s, tanAOV, &segs, &ns);
    }
  } else {
    if (d->post_helpers && !(s->post_mode && s->post_tan == tanAOV)) rd_post_helpers_arm();      // (they wake while the device is still busy with the frame: rd_post.c; not for a frame whose rectangles the device computes)
    static const int trace_poll = RD_LAB_INT("RD_TRACE_POLL", 0);      // (1: timings, 2: wait by querying instead of hipEventSynchronize)
    struct timespec t0, t1, t2, t3; clock_gettime(CLOCK_MONOTONIC, &t0);
    if (trace_poll == 2) { while (hipEventQuery(s->watch_done) == hipErrorNotReady) sched_yield(); }
    else RD_HIP(hipEventSynchronize(s->watch_done));
    clock_gettime(CLOCK_MONOTONIC, &t1);
    slot_finish_device(d, s);
    clock_gettime(CLOCK_MONOTONIC, &t2);
    r = slot_rectangles(d, s, tanAOV, &segs, &ns);
    clock_gettime(CLOCK_MONOTONIC, &t3);
    if (trace_poll) {
      static double a, b, c; static int n;
      a += (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3; b += (t2.tv_sec - t1.tv_sec) * 1e6 + (t2.tv_nsec - t1.tv_nsec) * 1e-3; c += (t3.tv_sec - t2.tv_sec) * 1e6 + (t3.tv_nsec - t2.tv_nsec) * 1e-3;
      if (++n % 100 == 0) { fprintf(stderr, "poll: wait %.1f us, finish %.1f us, rectangles %.1f us (average of 100)\n", a / 100, b / 100, c / 100); a = b = c = 0; }
    }
  }
  count_device_time(d, s);
  free(d->last_segs);
  d->last_segs = segs; d->last_nsegs = ns;
  d->last_polled_slot = si;
  d->next_poll++;
  return r;
}

// The frame of the most recently polled slot as a job of a service takes it (rd_rectify.hip, rd_annotate.hip, rd_composite.hip, rd_match.hip): format, planes and row strides as
// hand_over left them - device pointers in every case, which a service's stream may read at once: the poll has waited for the frame's last kernel - at the size it
// came in.  own: a host or pinned frame's copy in the slot's own buffer (bgr, or sc_bgr at scale 2), which the next frame of this slot overwrites and no job may write.
// false: nothing polled yet, or `service` is no live service of this kind on the detector's device; cap: the most items one of its jobs takes.
struct PolledFrame { int fmt, iw, ih, scale, cap; const void *planes[3]; const int *pitch; bool own; };
static bool polled_frame(rd_detector *d, const char *who, const void *service, uint32_t magic, PolledFrame *f) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "%s: bad handle\n", who);
  f->cap = rdjob::service_capacity(service, magic, d->device);
  if (d->last_polled_slot < 0 || f->cap < 0) return false;
  const Slot *s = &d->slots[d->last_polled_slot];
  f->fmt = s->fmt; f->scale = s->scale; f->iw = s->scale * d->iw; f->ih = s->scale * d->ih; f->pitch = s->pitch;
  for (int k = 0; k < 3; k++) f->planes[k] = s->pl[k];
  f->own = s->pl[0] == s->bgr || (s->sc_bgr && s->pl[0] == s->sc_bgr);
  return true;
}
// A frame that came in at scale 2 takes quads in detector coordinates: a copy of the job's n items (`size` bytes each, a quad's 8 doubles first), each corner mapped to
// the source's (pixel centres at integers: detector pixel x covers source pixels 2x and 2x+1, centre 2x + 0.5), to be freed behind the enqueue - which takes what it
// needs before it returns.  NULL: the job takes the caller's items (scale 1, or arguments that the service will refuse)
static_assert(offsetof(rd_comp_item, quad) == 0, "an item begins with its quad");
static void *mapped_to_source(const PolledFrame *f, const char *who, const void *items, int n, size_t size) {
  if (f->scale != 2 || !items || n < 1 || n > f->cap) return NULL;
  char *m = (char *)malloc((size_t)n * size);
  if (!m) exitf(-1, "%s: out of memory\n", who);
  memcpy(m, items, (size_t)n * size);
  for (int k = 0; k < n; k++) {
    double *q = (double *)(m + k * size);
    for (int i = 0; i < 8; i++) q[i] = q[i] * 2.0 + 0.5;
  }
  return m;
}
// Rectified patches from the polled frame; nothing of the slot is written.
long rd_detector_rectify_polled(rd_detector *d, rd_rectifier *r, const double *quads, int n, void *out, int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_rectify_polled", r, RD_MAGIC_RECTIFIER, &f)) return -1;
  void *m = mapped_to_source(&f, "rd_detector_rectify_polled", quads, n, 8 * sizeof(double));
  const long q = rd_rectifier_enqueue(r, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, m ? (const double *)m : quads, n, out, out_kind);
  free(m);
  return q;
}
// Matched quads of the polled frame; nothing of the slot is written.
long rd_detector_match_polled(rd_detector *d, rd_matcher *m, const double *quads, int n, int flags) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_match_polled", m, RD_MAGIC_MATCHER, &f)) return -1;
  void *mq = mapped_to_source(&f, "rd_detector_match_polled", quads, n, 8 * sizeof(double));
  const long q = rd_matcher_enqueue(m, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, mq ? (const double *)mq : quads, n, flags);
  free(mq);
  return q;
}
// Annotated frames: a caller's device frame may be drawn into in place; the slot's own copy needs a destination.
long rd_detector_annotate_polled(rd_detector *d, rd_annotator *a, const rd_annot_prim *prims, int n, int flags, void *const out_planes[3], const int out_pitches[3], int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_annotate_polled", a, RD_MAGIC_ANNOTATOR, &f) || (f.own && !out_planes)) return -1;
  return rd_annotator_enqueue(a, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, prims, n, flags, out_planes, out_pitches, out_kind);
}
// Composited quads: in place or into a destination by the annotator's rule.
long rd_detector_composite_polled(rd_detector *d, rd_compositor *c, const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                                  void *const out_planes[3], const int out_pitches[3], int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_composite_polled", c, RD_MAGIC_COMPOSITOR, &f) || (f.own && !out_planes)) return -1;
  void *m = mapped_to_source(&f, "rd_detector_composite_polled", items, n, sizeof(rd_comp_item));
  const long q = rd_compositor_enqueue(c, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, m ? (const rd_comp_item *)m : items, n, patches, npatches, patches_kind, out_planes, out_pitches, out_kind);
  free(m);
  return q;
}

// The reference hands the aperture over with the poll, i.e. after the frame (oclrect_pollTask); whatever runs ahead of the poll - the
// worker threads' post-process, the rectangles on the device - uses the last one seen.  A caller that knows it beforehand says so here,
// and the first frames of a stream are treated like all later ones.
void rd_detector_set_aperture(rd_detector *d, double tanAOV) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_set_aperture: bad handle\n");
  pthread_mutex_lock(&d->tan_mu);
  d->tan_aov = tanAOV; d->have_tan = 1;
  pthread_cond_broadcast(&d->tan_cv);
  pthread_mutex_unlock(&d->tan_mu);
}

void rd_detector_drain(rd_detector *d) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_drain: bad handle\n");
  RD_HIP(hipSetDevice(d->device));
  if (d->batch > 1) for (int i = 0; i < d->nslots; i += d->batch) sparse_flush(d, i);
  if (d->zb > 1) for (long q = d->next_poll; q < d->next_enqueue; q++) {      // (sequence order)
    const int si = (int)(q % d->nslots);
    if (d->slots[si].pending_dense) group_launch(d, si / d->zb * d->zb);
  }
  for (int i = 0; i < d->nslots; i++) RD_HIP(hipStreamSynchronize(d->slots[i].st));
}

long rd_detector_counter(rd_detector *d, int which) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_counter: bad handle\n");
  if (which == 3) return d->host_enqueue_ns / 1000;
  if (which == 4) return __atomic_load_n(&d->n_redo_rounds, __ATOMIC_RELAXED);
  if (which == 5) return __atomic_load_n(&d->rounds_budget, __ATOMIC_RELAXED);
  if (which >= 20 && which < 20 + RD_NBUDGETS) return d->budget_count[which - 20];   // frames launched with a budget of 8 / 10 / .. / 20 launches of the region merge
  if (which == 10) return __atomic_load_n(&d->n_truncated, __ATOMIC_RELAXED);
  if (which == 11) return __atomic_load_n(&d->n_post_device, __ATOMIC_RELAXED);
  if (which == 12) return __atomic_load_n(&d->n_post_host, __ATOMIC_RELAXED);
  if (which == 13) return __atomic_load_n(&d->host_post_ns, __ATOMIC_RELAXED) / 1000;
  if (which == 14) return __atomic_load_n(&d->n_redo_absorb, __ATOMIC_RELAXED);
  if (which == 15) return d->zb;      // frames per group launch (1: every frame its own launches)
  if (which == 6) return __atomic_load_n(&d->n_unsettled, __ATOMIC_RELAXED);
  if (which == 18) return d->n_frames_pinned;
  if (which == 19) return d->n_frames_copied;
  if (which == 16) return d->n_strong_group;        // groups whose strong masks were ONE launch (k_strength_masks_group)
  if (which == 17) return d->n_strong_by_frame;     // groups whose strong masks were evaluated frame by frame
  if (which >= 40 && which <= 60) return d->need_count[which - 40];      // frames whose region merge needed 0..20 launches (the one that changes nothing included; 20: or more)
  if (which == 1) return d->dev_us;
  if (which == 2) return d->dev_frames;
  if (which == 30) return __atomic_load_n(&d->n_long_lists, __ATOMIC_RELAXED);
  if (which == 31) return (long)d->slot_pitch;      // (device bytes of one slot's planes, the way the slots are carved: every plane rounded up to 256 bytes)
  if (which == 32) return d->kind == RD_KIND_POLY ? d->handoff_rec : RD_MAXREC;
  if (which == 33) { size_t b = 0; for (int i = 0; i < d->nslots; i++) if (d->slots[i].sc_bgr && d->slots[i].sc_bytes > b) b = d->slots[i].sc_bytes; return (long)b; }
  return which == 0 ? __atomic_load_n(&d->n_redo, __ATOMIC_RELAXED) : -1;
}

int rd_detector_last_segments(rd_detector *d, void *dst, int max_records) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_last_segments: bad handle\n");
  if (!d->last_segs) return -1;
  int m = d->last_nsegs + 1 < max_records ? d->last_nsegs + 1 : max_records;
  if (dst && m > 0) memcpy(dst, d->last_segs, (size_t)m * 56);
  return d->last_nsegs;
}

// A plane kept as bits on the device (ceil(iw / 64) words per row), handed out as an int plane.  junction: not the bits but the junction counts
// (oclrect.cl:74-95: on-pixels of the 3x3 block, 1 -> 0, frame border 0) evaluated from them.
static size_t bit_plane_as_ints(rd_detector *d, const void *bits, int junction, void *dst, size_t max_bytes) {
  const size_t n = (size_t)d->N * 4 <= max_bytes ? (size_t)d->N : max_bytes / 4;
  const int wpr = (d->iw + 63) / 64, iw = d->iw, ih = d->ih;
  unsigned long long *tmp = (unsigned long long *)malloc((size_t)wpr * ih * 8 + 8);
  if (!tmp) exitf(-1, "rd_detector_debug_plane: out of memory\n");
  RD_HIP(hipMemcpy(tmp, bits, (size_t)wpr * ih * 8, hipMemcpyDeviceToHost));
  auto bit = [&](int x, int y) { return (int)((tmp[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull); };
  for (size_t k = 0; k < n; k++) {
    const int y = (int)(k / iw), x = (int)(k % iw);
    int v = bit(x, y);
    if (junction) {
      if (v && x > 0 && y > 0 && x < iw - 1 && y < ih - 1) { int c = 0; for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) c += bit(x + dx, y + dy); v = c == 1 ? 0 : c; }
      else v = 0;
    }
    ((int *)dst)[k] = v;
  }
  free(tmp);
  return n * 4;
}
// The debug planes of both kinds: the one table of them (include/rectdetect_hip.h lists the names).  A row: name, kinds, plane + byte offset, `bytes`, how the plane is
// viewed, what has to be launched before it can be looked at.  `bytes` is what the CALLER gets when max_bytes is ample, not what lies at the pointer: the rows of the int
// views say N * 4 where the device holds N bytes (edge500) or a bit plane (strong, junction, mergemask, polymask); a raw row's two sizes are the same.
enum { VIEW_RAW,          // as stored; a shorter buffer gets min(bytes, max_bytes)
       // int views - kept in another shape on the device, handed out as the reference's int planes; a shorter buffer gets max_bytes / 4 elements:
       VIEW_BITS,         // a bit plane (what the polyline stage traces / what the region stage reads; oclrect.c:307-321, poly.cpp:121)
       VIEW_JUNCTION,     // the junction counts evaluated from a bit plane
       VIEW_POSITIVE,     // `> 0` of a float plane (rect kind's mask0, oclrect.c:262-264: not stored on the frame path, derived from the suppressed strength)
       VIEW_INT8,         // bytes (the blur's mask; oclrect.c:277-284)
       VIEW_STRSUM };     // raw + the strong mask the frame read: the reference's plane holds the sums ON TOP of the previous frame's strong mask (H1)
enum { PREP_NONE,
       PREP_IDS,          // polyline_ids: the id plane is not part of the frame path, it is built from the compact state
       PREP_FLATTEN,      // a -DRD_BOUNDARY_FLATTEN=0 build leaves the boundary components as a forest (its few readers walk): flattened here, where the plane is looked at
       PREP_TAPS };       // plab1, vxy, strength never leave the chip where the front is fused: the same kernel again, writing them out (the blurred planes are intact)
size_t rd_detector_debug_plane(rd_detector *d, const char *name, void *dst, size_t max_bytes) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_debug_plane: bad handle\n");
  if (d->last_polled_slot < 0) return 0;
  RD_HIP(hipSetDevice(d->device));
  Slot *s = &d->slots[d->last_polled_slot];
  const size_t N = (size_t)d->N, NI = N * 4;
  const int kind = d->kind == RD_KIND_POLY ? PK_POLY : PK_RECT;
  const struct { const char *n; int kinds; const void *p; size_t off, bytes; int view, prep; } tab[] = {
    { "plab0", PK_BOTH, s->plab0, 0, NI, VIEW_RAW, PREP_NONE }, { "plab1", PK_RECT, s->plab1, 0, NI, VIEW_RAW, PREP_TAPS }, { "lblur", PK_BOTH, s->bl[0], 0, NI, VIEW_RAW, PREP_NONE },
    { "vxy", PK_RECT, s->vxy, 0, N * 8, VIEW_RAW, PREP_TAPS }, { "strength", PK_RECT, s->strength, 0, NI, VIEW_RAW, PREP_TAPS }, { "nms", PK_BOTH, s->nms, 0, NI, VIEW_RAW, PREP_NONE },
    { "mask0", PK_RECT, s->nms, 0, NI, VIEW_POSITIVE, PREP_NONE }, { "mask0", PK_POLY, s->mask0, 0, NI, VIEW_RAW, PREP_NONE }, { "tidy", PK_RECT, s->tidy, 0, NI, VIEW_RAW, PREP_NONE },
    { "label1", PK_BOTH, s->label1, 0, NI, VIEW_RAW, PREP_NONE }, { "strsum", PK_RECT, s->strsum, 0, NI, VIEW_STRSUM, PREP_NONE }, { "strsum", PK_POLY, s->strsum, 0, NI, VIEW_RAW, PREP_NONE },
    { "edge500", PK_RECT, s->e8, 0, NI, VIEW_INT8, PREP_NONE }, { "smooth", PK_RECT, s->smooth, 0, NI, VIEW_RAW, PREP_NONE }, { "quant", PK_RECT, s->quant, 0, NI, VIEW_RAW, PREP_NONE },
    { "strong", PK_RECT, s->strongbits, 0, NI, VIEW_BITS, PREP_NONE }, { "junction", PK_RECT, s->strongbits, 0, NI, VIEW_JUNCTION, PREP_NONE }, { "mergemask", PK_RECT, s->mmbits, 0, NI, VIEW_BITS, PREP_NONE },
    { "polymask", PK_POLY, s->strongbits, 0, NI, VIEW_BITS, PREP_NONE },
    { "region", PK_RECT, s->region, 0, NI, VIEW_RAW, PREP_NONE }, { "region0", PK_RECT, s->region0, 0, NI, VIEW_RAW, PREP_NONE }, { "rsize", PK_RECT, s->rsize, 0, NI, VIEW_RAW, PREP_NONE },
    { "boundarysrc", PK_RECT, s->boundarysrc, 0, NI, VIEW_RAW, PREP_NONE }, { "boundary", PK_RECT, s->boundary, 0, NI, VIEW_RAW, PREP_FLATTEN }, { "lsid", PK_BOTH, s->lsid, 0, NI, VIEW_RAW, PREP_IDS },
    { "table", PK_RECT, s->table, 0, (N * 4 / 5) * 5 * 4, VIEW_RAW, PREP_NONE }, { "lslist", PK_BOTH, s->lslist, 0, N * 16, VIEW_RAW, PREP_NONE },
    { "polyctr", PK_BOTH, rdk::poly_scratch_counters(s->ps), 0, 64 * 4, VIEW_RAW, PREP_NONE }, { "iirflags", PK_RECT, s->flags, 0, 16 * 4, VIEW_RAW, PREP_NONE },
    { "d2work", PK_RECT, s->d2s, NI, 16 * 4, VIEW_RAW, PREP_NONE }, { "absorb", PK_RECT, s->scratch2, (N + RD_REGION_STATUS_AT) * 4, 8 * 4, VIEW_RAW, PREP_NONE },
  };
  for (const auto &r : tab) {
    if (!(r.kinds & kind) || strcmp(r.n, name)) continue;
    const char *p = (const char *)r.p + r.off;
    // (launches of a test tap: under the lock that keeps launches out of another thread's graph capture)
    pthread_mutex_lock(&d->launch_mu);
    if (r.prep == PREP_IDS) rdk::polyline_ids(s->st, s->frame, 1, (int)N);
    if (r.prep == PREP_FLATTEN && !RD_BOUNDARY_FLATTEN) rdk::label8_flatten(s->st, s->boundary, (int)N);
    if (r.prep == PREP_TAPS && front_is_fused(d)) frames_grad_nms(d, s, s->st, 1, 0, 1);
    if (r.prep != PREP_NONE) rdrt::check_launch("debug plane");
    pthread_mutex_unlock(&d->launch_mu);
    RD_HIP(hipStreamSynchronize(s->st));
    if (r.view == VIEW_BITS || r.view == VIEW_JUNCTION) return bit_plane_as_ints(d, p, r.view == VIEW_JUNCTION, dst, max_bytes);
    if (r.view == VIEW_POSITIVE || r.view == VIEW_INT8) {
      const size_t n = NI <= max_bytes ? N : max_bytes / 4, eb = r.view == VIEW_INT8 ? 1 : 4;
      void *tmp = malloc(n ? n * eb : 4);
      if (!tmp) exitf(-1, "rd_detector_debug_plane: out of memory\n");
      RD_HIP(hipMemcpy(tmp, p, n * eb, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < n; k++) ((int *)dst)[k] = r.view == VIEW_INT8 ? ((const int8_t *)tmp)[k] : (((const float *)tmp)[k] > 0.0f ? 1 : 0);
      free(tmp);
      return n * 4;
    }
    const size_t b = r.bytes < max_bytes ? r.bytes : max_bytes;
    RD_HIP(hipMemcpy(dst, p, b, hipMemcpyDeviceToHost));
    if (r.view == VIEW_STRSUM && s->prev_in) {
      const size_t n = b / 4;
      int8_t *tmp = (int8_t *)malloc(n ? n : 1);
      RD_HIP(hipMemcpy(tmp, s->prev_in, n, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < n; k++) ((int *)dst)[k] += tmp[k];
      free(tmp);
    }
    return b;
  }
  return 0;
}

// ---- the polyline kind
rd_detector *rd_polyline_detector_create(int device, int iw, int ih, int nslots, int strength_thre, float minerror, int size_thre) {
  if (iw < 16 || ih < 16 || (long long)iw * ih >= (1ll << 25) || nslots < 1 || device < 0 || strength_thre < 0 || !(minerror > 0.0f) || size_thre < 0) return NULL;
  if (rd_device_count() <= 0) exitf(-1, "rd_polyline_detector_create: no HIP device available - this library has no CPU path\n");
  if (device >= rd_device_count()) return NULL;
  rd_detector *d = detector_new(RD_KIND_POLY, device, iw, ih, nslots, 0);
  d->p_thre = strength_thre; d->p_minerror = minerror; d->p_size = size_thre;
  d->handoff_rec = RD_POLY_HANDOFF_DEFAULT;
  { const int h = rd_env_int("RD_POLY_HANDOFF", 0); if (h >= 2) d->handoff_rec = h; }      // (tests: a small block, so that ordinary frames take the long-list path)
  detector_slots(d, 4);      // (streams and group launches as the rect kind's; no second stream per frame, no batches, no rectangles: fork_poly, defer and device_post stay 0)
  return d;
}

void *rd_detector_poll_segments(rd_detector *d, int32_t *ids_out) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_poll_segments: bad handle\n");
  if (d->kind != RD_KIND_POLY) exitf(-1, "rd_detector_poll_segments: this is a rectangle detector (rd_detector_create) - its results come from rd_detector_poll\n");
  if (d->next_poll >= d->next_enqueue) exitf(-1, "rd_detector_poll_segments: nothing enqueued\n");
  RD_HIP(hipSetDevice(d->device));
  const int si = (int)(d->next_poll % d->nslots);
  Slot *s = &d->slots[si];
  const size_t N = (size_t)d->N;
  if (s->pending_dense) group_launch(d, si / d->zb * d->zb);      // (an incomplete group: the caller wants a result before handing over more frames)
  RD_HIP(hipEventSynchronize(s->watch_done));
  // the single-block polyline kernel gave up on this frame (on-chip tables too small): the stage again in multi-launch form, on the slot's own stream (the
  // frame is finished; its slot is not reused before this poll returns); two such frames in a row send the stream's later frames to the multi-launch form
  const bool over = s->poly_mode == 1 && s->h_pack[25] != 0;
  if (s->poly_mode == 1) { if (over) { if (++d->overflow_streak >= 2) d->poly_overflows = 1; } else d->overflow_streak = 0; }
  if (!s->st_redo) s->st_redo = make_redo_stream();
  if (over || (d->force_redo & 1)) {
    rdk::polyline(s->st_redo, s->frame, 1, d->N * 16, 0, d->p_minerror, d->p_size, d->iw, d->ih, 0);
    rdk::polyline_handoff(s->st_redo, s->frame, 1, d->handoff_rec);
    rdrt::check_launch("polyline frame, multi-launch repeat");
    RD_HIP(hipStreamSynchronize(s->st_redo));
    d->n_redo++;
  }
  const int n = s->h_pack[64];
  void *out = malloc((size_t)(n + 1) * 56);
  if (!out) exitf(-1, "rd_detector_poll_segments: out of memory\n");
  if (n + 1 <= d->handoff_rec) memcpy(out, s->h_pack + 64, (size_t)(n + 1) * 56);
  else { slot_fetch(s, out, s->lslist, (size_t)(n + 1) * 56); d->n_long_lists++; }      // (nothing is dropped: the rest of a long list comes from the device)
  if (ids_out) {      // the dense id plane, only on request: from the slot's compact scratch
    rdk::polyline_ids(s->st_redo, s->frame, 1, (int)N);
    RD_HIP(hipMemcpyAsync(ids_out, s->lsid, N * 4, hipMemcpyDeviceToHost, s->st_redo));
    RD_HIP(hipStreamSynchronize(s->st_redo));
  }
  count_device_time(d, s);
  d->last_polled_slot = si;
  d->next_poll++;
  return out;
}

// ================================================================================================ oclrect (reference API)
struct oclrect_t { uint32_t magic; rd_detector *det; int iw, ih; };

struct oclrect_t *init_oclrect(struct oclimgutil_t *oclimgutil, struct oclpolyline_t *oclpolyline, cl_device_id device, cl_context context, cl_command_queue queue, int iw, int ih) {
  (void)oclimgutil; (void)oclpolyline; (void)context; (void)queue;
  struct oclrect_t *t = (struct oclrect_t *)calloc(1, sizeof(*t));
  t->magic = MAGIC_RECT; t->iw = iw; t->ih = ih;
  t->det = rd_detector_create(device ? device->ordinal : rdrt::current_device(), iw, ih, 2, RD_LAB_INT("RD_API_WORKERS", 0));   // two pages like oclrect.c:54
  return t;
}

void dispose_oclrect(struct oclrect_t *t) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "dispose_oclrect: bad handle\n");
  rd_detector_destroy(t->det);
  t->magic = 0;
  free(t);
}

rect_t *oclrect_executeOnce(struct oclrect_t *t, uint8_t *imgData, int ws, const double tanAOV) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_executeOnce: bad handle\n");
  if (t->det->next_enqueue != t->det->next_poll) exitf(-1, "oclrect_executeOnce: a task is still pending (poll it first)\n");
  rd_detector_enqueue(t->det, imgData, ws, 0);
  return (rect_t *)rd_detector_poll(t->det, tanAOV);
}

void oclrect_enqueueTask(struct oclrect_t *t, uint8_t *imgData, int ws) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_enqueueTask: bad handle\n");
  rd_detector_enqueue(t->det, imgData, ws, 0);
}

rect_t *oclrect_pollTask(struct oclrect_t *t, const double tanAOV) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_pollTask: bad handle\n");
  return (rect_t *)rd_detector_poll(t->det, tanAOV);
}

// ---- test taps of the device post-process (neither is on the frame path)
void rd_post_device_limits(int32_t out[8]) { rdk::post_limits(out); }

// rd_postprocess_planes' device twin: the caller's list, boundary plane and vote table through k_sample_segments and the three launches of
// rdk::post_device, once, on a stream, scratch and result block of its own; the result block is packed by the code a poll uses.
// The caller's plane holds a component id per pixel, as the default build's frame path leaves it.  A -DRD_BOUNDARY_FLATTEN=0 build reads
// the plane as a forest of pixel indices and would follow the caller's ids as links: the tap refuses to run there.
void *rd_postprocess_planes_device(int device, const void *segs, const int32_t *boundary, const int32_t *table, int iw, int ih, double tanAOV, int32_t info[8]) {
  if (!RD_BOUNDARY_FLATTEN) exitf(-1, "rd_postprocess_planes_device: needs a build with RD_BOUNDARY_FLATTEN=1 (the plane holds ids, not links)\n");
  RD_HIP(hipSetDevice(device));
  int n = ((const int *)segs)[0];
  if (n < 0) n = 0;
  const size_t N = (size_t)iw * ih;
  const int nentry = iw * ih * 4 / 5;
  char *d_ls = dnew<char>((size_t)(n + 1) * 56);
  int *d_boundary = dnew<int>(N), *d_table = dnew<int>((size_t)nentry * 5), *d_probes = dnew<int>((size_t)(n + 1) * 15 * 6);
  int *d_scratch = dnew<int>(rdk::post_scratch_ints());
  int *h_post = NULL, *h_post_dev = NULL;
  const size_t out_bytes = rdk::post_out_ints() * sizeof(int);
  RD_HIP(hipHostMalloc((void **)&h_post, out_bytes, hipHostMallocDefault)); memset(h_post, 0, out_bytes);
  RD_HIP(hipHostGetDevicePointer((void **)&h_post_dev, h_post, 0));
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemcpyAsync(d_ls, segs, (size_t)(n + 1) * 56, hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(d_boundary, boundary, N * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(d_table, table, (size_t)nentry * 5 * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemsetAsync(d_probes, 0, (size_t)(n + 1) * 15 * 6 * sizeof(int), st));
  rdk::PolyFrame f;
  memset(&f, 0, sizeof(f));
  f.lslist = d_ls; f.boundary = d_boundary; f.table = d_table; f.probes = d_probes; f.pack = NULL;
  f.post_scratch = d_scratch; f.post_out = h_post_dev;
  rdk::sample_segments(st, &f, 1, n + 1, iw, ih, nentry, 0);
  rdk::post_device(st, &f, 1, n + 1, iw, ih, tanAOV);
  rdrt::check_launch("rd_postprocess_planes_device");
  RD_HIP(hipStreamSynchronize(st));
  if (info) { for (int i = 0; i < 8; i++) info[i] = 0; info[0] = h_post[0]; info[1] = h_post[1]; }
  void *ret = h_post[1] == 0 ? (void *)post_block_rectangles(h_post) : NULL;
  RD_HIP(hipStreamDestroy(st));
  RD_HIP(hipHostFree(h_post));
  dfree(d_scratch); dfree(d_probes); dfree(d_table); dfree(d_boundary); dfree(d_ls);
  return ret;
}

// ---- test taps of the polyline stage (neither is on the frame path)
void rd_polyline_limits(int32_t out[4]) { rdk::poly_limits(out); }

// oclpolyline_execute's twin with the form of the stage chosen by the caller: the caller's 0/1 plane through rdk::polyline and rdk::polyline_ids,
// once, on a stream and scratch of its own.  form 1 is the single-block kernel alone: where it gives up (ctr_out[25]) nothing repeats the stage,
// the caller sees the flag and whatever list the kernel left.
int rd_polyline_planes_device(int device, const int32_t *mask, int iw, int ih, int ring_nonzero, float minerror, int size_thre, int lslist_bytes, int form,
                              void *lslist_out, int32_t *ids_out, int32_t ctr_out[64]) {
  // (the stage's scratch is sized for lists of up to 16 bytes per pixel, what every caller in the reference passes; two records are the least a list holds)
  if (!mask || !lslist_out || !ids_out || !ctr_out || iw < 5 || ih < 5 || iw > 0xffff || ih > 0x7fff || (form != 0 && form != 1) || size_thre < 0 ||
      lslist_bytes < 2 * 56 || (long long)lslist_bytes > (long long)iw * ih * 16) return -1;
  RD_HIP(hipSetDevice(device));
  const size_t N = (size_t)iw * ih;
  int *d_mask = dnew<int>(N), *d_ids = dnew<int>(N);
  char *d_ls = dnew<char>((size_t)lslist_bytes + 56);
  rdk::PolyScratch *ps = rdk::poly_scratch_create(iw, ih);
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemcpyAsync(d_mask, mask, N * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemsetAsync(d_ls, 0, (size_t)lslist_bytes + 56, st));
  rdk::PolyFrame f;
  memset(&f, 0, sizeof(f));
  f.ps = *ps; f.in = d_mask; f.lslist = d_ls; f.ids = d_ids;
  rdk::polyline(st, &f, 1, lslist_bytes, ring_nonzero ? 1 : 0, minerror, size_thre, iw, ih, form);
  rdk::polyline_ids(st, &f, 1, (int)N);
  rdrt::check_launch("rd_polyline_planes_device");
  RD_HIP(hipMemcpyAsync(lslist_out, d_ls, (size_t)lslist_bytes, hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(ids_out, d_ids, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(ctr_out, rdk::poly_scratch_counters(ps), 64 * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  RD_HIP(hipStreamDestroy(st));
  rdk::poly_scratch_destroy(ps);
  dfree(d_ls); dfree(d_ids); dfree(d_mask);
  return 0;
}

// ---- test taps of the region stage (neither is on the frame path)
void rd_region_limits(int iw, int ih, int32_t out[32]) { rdk::region_limits(iw, ih, out); }

// an int plane (non-zero / positive = set) as the bit plane the region kernels read: ceil(iw / 64) words per row, bits beyond the row's end clear
static void pack_bit_plane(unsigned long long *bits, const int32_t *plane, int iw, int ih, int positive_only) {
  const int wpr = (iw + 63) / 64;
  memset(bits, 0, ((size_t)wpr * ih + 8) * sizeof(*bits));
  for (int y = 0; y < ih; y++)
    for (int x = 0; x < iw; x++) {
      const int v = plane[(size_t)y * iw + x];
      if (positive_only ? v > 0 : v != 0) bits[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
    }
}

// frame_regions' twin on planes of the caller: stage 0 = region_merge, region_size, despeckle2, label8_boundary from the merge's inputs, with a budget of the caller's or
// (launches = 0) the frame path's - RD_REGION_FIRST_BUDGET launches, then region_ladder -; stage 1 = despeckle2, label8_boundary from the absorption's inputs.  Either way
// the slow absorption (frame_absorb_slow's two calls) where the status word asks for it or the caller forces it.  Once, on a stream, planes and scratch of its own.
int rd_region_planes_device(int device, int stage, int iw, int ih, const int32_t *pix, const int32_t *mask, const int32_t *edge, int launches,
                            const int32_t *region0_in, const int32_t *rsize_in, int force_slow,
                            int32_t *region0_out, int32_t *rsize_out, int32_t *region_out, int32_t *boundarysrc_out, int32_t *boundary_out, int32_t info[RD_REGION_INFO_INTS]) {
  if (!region0_out || !rsize_out || !region_out || !boundarysrc_out || !boundary_out || !info || (stage != 0 && stage != 1)) return -1;
  if (iw < 16 || ih < 16 || (long long)iw * ih >= (1ll << 25)) return -1;      // (rd_detector_create's limits)
  const size_t N = (size_t)iw * ih;
  if (stage == 0) {
    if (!pix || !mask || !edge || launches < 0 || (launches & 1) || launches == 1 || launches > RD_REGION_MAX_LAUNCHES) return -1;
  } else {
    if (!region0_in || !rsize_in) return -1;
    for (size_t p = 0; p < N; p++)
      if (region0_in[p] < 0 || (size_t)region0_in[p] >= N || rsize_in[p] < 0 || rsize_in[p] >= (1 << 26)) return -1;      // (labels index the size table; the tail's words hold sizes in 26 bits)
  }
  RD_HIP(hipSetDevice(device));
  const int n = (int)N, nentry = n * 4 / 5;
  const size_t nbits = (size_t)((iw + 63) / 64) * ih + 8;
  int *d_pix = dnew<int>(N), *d_region0 = dnew<int>(N), *d_rsize = dnew<int>(N), *d_region = dnew<int>(N), *d_bsrc = dnew<int>(N), *d_boundary = dnew<int>(N);
  int *d_scratch2 = dnew<int>(N * 3 + 256), *d_d2s = dnew<int>(RD_D2_SCRATCH_INTS(N)), *d_table = dnew<int>(N * 4), *d_claim = dnew<int>(N), *d_tlist = dnew<int>(N);
  unsigned long long *d_mm = dnew<unsigned long long>(nbits), *d_sb = dnew<unsigned long long>(nbits);
  int *flags = d_scratch2 + N, *status = flags + RD_REGION_STATUS_AT;
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  rdk::reduce_ls_init(st, d_table, d_claim, d_tlist, nentry);
  RD_HIP(hipMemsetAsync(flags, 0, 256 * sizeof(int), st));
  for (int i = 0; i < RD_REGION_INFO_INTS; i++) info[i] = 0;
  int budget = 0, settled = 1;
  if (stage == 0) {
    unsigned long long *h_bits = (unsigned long long *)malloc(nbits * sizeof(*h_bits));
    if (!h_bits) exitf(-1, "rd_region_planes_device: out of memory\n");
    RD_HIP(hipMemcpyAsync(d_pix, pix, N * sizeof(int), hipMemcpyHostToDevice, st));
    pack_bit_plane(h_bits, mask, iw, ih, 0);
    RD_HIP(hipMemcpyAsync(d_mm, h_bits, nbits * sizeof(*h_bits), hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));      // (the one host buffer packs both planes)
    pack_bit_plane(h_bits, edge, iw, ih, 1);
    RD_HIP(hipMemcpyAsync(d_sb, h_bits, nbits * sizeof(*h_bits), hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));
    free(h_bits);
    auto still_after = [&](int b) {      // frame_regions with b launches of the merge; the flag of the last one
      int marked = 0, still = 0;
      rdk::region_merge(st, d_region0, d_scratch2, d_pix, d_mm, d_sb, iw, ih, b, d_rsize, &marked, 1, 0);
      rdk::region_size(st, d_rsize, d_region0, n, d_d2s + N, marked, 1, 0);
      rdk::despeckle2(st, d_region, d_region0, d_d2s, d_rsize, RD_ABSORB_THRE, iw, ih, 1, status, 1, 0);
      rdk::label8_boundary(st, d_boundary, d_bsrc, d_region, iw, ih, d_table, d_claim, d_tlist, 1, 0, RD_BOUNDARY_FLATTEN);
      rdrt::check_launch("rd_region_planes_device");
      RD_HIP(hipMemcpyAsync(&still, flags + b - 1, sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipStreamSynchronize(st));
      return still;
    };
    budget = launches ? launches : RD_REGION_FIRST_BUDGET;
    settled = still_after(budget) == 0;
    if (!launches && !settled) { const LadderEnd e = region_ladder(still_after); budget = e.budget; settled = e.settled; }
  } else {
    RD_HIP(hipMemcpyAsync(d_region0, region0_in, N * sizeof(int), hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(d_rsize, rsize_in, N * sizeof(int), hipMemcpyHostToDevice, st));
    rdk::despeckle2(st, d_region, d_region0, d_d2s, d_rsize, RD_ABSORB_THRE, iw, ih, 0, status, 1, 0);
    rdk::label8_boundary(st, d_boundary, d_bsrc, d_region, iw, ih, d_table, d_claim, d_tlist, 1, 0, RD_BOUNDARY_FLATTEN);
    rdrt::check_launch("rd_region_planes_device");
  }
  RD_HIP(hipMemcpyAsync(info, flags, (size_t)RD_REGION_MAX_LAUNCHES * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(info + RD_REGION_MAX_LAUNCHES + 2, status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  info[RD_REGION_MAX_LAUNCHES] = budget; info[RD_REGION_MAX_LAUNCHES + 1] = settled;
  if (info[RD_REGION_MAX_LAUNCHES + 2] != 0 || force_slow) {      // as frame_absorb_slow
    info[RD_REGION_MAX_LAUNCHES + 7] = rdk::despeckle2_slow(st, d_region, d_region0, d_d2s, d_rsize, RD_ABSORB_THRE, iw, ih);
    rdk::label8_boundary(st, d_boundary, d_bsrc, d_region, iw, ih, d_table, d_claim, d_tlist, 1, 0, RD_BOUNDARY_FLATTEN);
    rdrt::check_launch("rd_region_planes_device, slow absorption");
    info[RD_REGION_MAX_LAUNCHES + 6] = 1;
  }
  if (!RD_BOUNDARY_FLATTEN) rdk::label8_flatten(st, d_boundary, n);      // (a tuning build leaves the components as a forest, as on the frame path: flattened where the plane is looked at)
  RD_HIP(hipMemcpyAsync(region0_out, d_region0, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(rsize_out, d_rsize, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(region_out, d_region, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(boundarysrc_out, d_bsrc, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(boundary_out, d_boundary, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  RD_HIP(hipStreamDestroy(st));
  dfree(d_sb); dfree(d_mm); dfree(d_tlist); dfree(d_claim); dfree(d_table); dfree(d_d2s); dfree(d_scratch2);
  dfree(d_boundary); dfree(d_bsrc); dfree(d_region); dfree(d_rsize); dfree(d_region0); dfree(d_pix);
  return 0;
}

}  // extern "C"
