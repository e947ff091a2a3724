// rectdetect-mi355x: the reference's operator API (oclimgutil.h, oclpolyline.h) on top of the gfx950 kernels.  C ABI, opaque handles, fatal-on-error like the reference.
// (The rectangle detector's API, oclrect.h, is a shim over rd_detector: rd_detector.hip.)
#include "rd_detector.h"      // (the handle magics, dnew / dfree)

extern "C" {
#include "oclimgutil.h"
#include "oclpolyline.h"
}

using rdrt::dptr;
using rdrt::stream;

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
