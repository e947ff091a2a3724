// rectdetect-mi355x: host-callable launchers of the gfx950 kernels (implemented in rd_k_*.hip).
// All pointers are device pointers; every launcher enqueues on `s` and returns immediately.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "rd_annot_cover.h"
#include "rd_pix.h"
#include "rectdetect_hip.h"

// Group launches (small frames, rd_frames.hip): launchers of the frame path take `nz` frames per launch and `zs`, the byte pitch between the planes
// of consecutive frame slots (rd_device.h: RD_ZSHIFT); the defaults launch one frame.
#define RD_ZB_MAX 8

namespace rdk {

// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised once PER DEVICE (a process may drive
// several GPUs from several threads): `done` holds one bit per device ordinal; a race only repeats an idempotent call.
inline void set_max_lds_once(const void *func, int bytes, std::atomic<unsigned> &done) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned bit = 1u << (dev & 31);
  if (done.load(std::memory_order_acquire) & bit) return;
  (void)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done.fetch_or(bit, std::memory_order_release);
}

// ---- rd_k_front.hip: colour, blur, gradient, non-max suppression, element-wise ops
void bgr2plab(hipStream_t s, uint32_t *out, const uint8_t *bgr, int iw, int ih, int ws);
// colour conversion that also leaves the unpacked L, a, b planes transposed (ih wide, iw tall) for the first blur sweep
void bgr2plab_transposed(hipStream_t s, uint32_t *out, float *const dst[3], const uint8_t *bgr, int iw, int ih, int ws);
void bgr2plab_transposed(hipStream_t s, uint32_t *out, float *const dst[3], const uint8_t *const *bgr, int iw, int ih, int ws, int nz, size_t zs);   // bgr: nz source frames   // dst: the three planes transposed, as 16-bit integer fields (iir_blur_pass src16)
// the same outputs from a frame in one of the other pixel formats (fmt: RD_PIX_RGB .. RD_PIX_I420 of rectdetect_hip.h): planes[z][k] = plane k of frame z,
// pitch[k] its row stride in bytes (one set for the nz frames)
void pix2plab_transposed(hipStream_t s, int fmt, uint32_t *out, float *const dst[3], const uint8_t *const (*planes)[3], const int pitch[3], int iw, int ih, int nz, size_t zs);
// the same outputs from source frames of 2 iw x 2 ih pixels (fmt: RD_PIX_BGR .. RD_PIX_I420; planes and pitch at the source size): every iw x ih pixel the 2x2 box
// average of the contract's (B, G, R), (sum + 2) >> 2 (rd_detector_enqueue_scaled)
void pix2plab_half_transposed(hipStream_t s, int fmt, uint32_t *out, float *const dst[3], const uint8_t *const (*planes)[3], const int pitch[3], int iw, int ih, int nz, size_t zs);
void unpack_plab(hipStream_t s, float *L, float *a, float *b, const uint32_t *in, int n);
void pack_plab(hipStream_t s, uint32_t *out, const float *L, const float *a, const float *b, int n);
// transposes of `np` float planes (src planes W x H row-major -> dst planes H x W); src may be packed Lab (np = 3)
void transpose_f(hipStream_t s, float *const dst[3], const float *const src[3], int np, int W, int H);
// one complete blur pass (causal + anti-causal sweep + combination) in a single launch, see rd_k_front.hip
size_t iir_pass_scratch_floats(int np, int W, int H);
void iir_blur_pass(hipStream_t s, float *const dst[3], const float *const src[3], float *const fwd[3], float *const bwd[3], int np, int W, int H,
                   int transpose_out, float *tails, int *bad, int src16 = 0, int nz = 1, size_t zs = 0);
void iir_blur_lines(hipStream_t s, float *dst, const float *src, float *fw, float *bw, int W, int H, int r);   // any radius 0..31, full-length sweeps along y; dst may be fw or bw
#define RD_IIR_MAX_R 31
void edgevec(hipStream_t s, float *vxy, const float *in, int iw, int ih, uint32_t *pack_out = nullptr, const float *a = nullptr, const float *b = nullptr, int nz = 1, size_t zs = 0);   // pack_out (optional): pack_plab(in, a, b) on the way
// visualisers / operators no application calls (oclimgutil.h:84-98)
void convert_bgr_lumaf(hipStream_t s, uint8_t *out, const float *in, float f, int iw, int ih, int ws);
void convert_bgr_labeli(hipStream_t s, uint8_t *out, const int *in, int bgc, int iw, int ih, int ws);
void plab2bgr(hipStream_t s, uint8_t *out, const uint32_t *in, int iw, int ih, int ws);
void edge_f(hipStream_t s, float *out, const float *in, int iw, int ih);
void edgevec_plab(hipStream_t s, float *vxy, const uint32_t *in, int iw, int ih);
void thincubic(hipStream_t s, float *out, const float *in, const float *vxy, int iw, int ih);
void edge_plab(hipStream_t s, float *out, const uint32_t *in, int iw, int ih, int nz = 1, size_t zs = 0);
void thinthres(hipStream_t s, float *out, const float *in, const float *vxy, int iw, int ih, int nz = 1, size_t zs = 0);
// gradient direction + re-packing + strength + non-max suppression of the frame path in one launch (bl: the three blurred planes); taps (all or none):
// the intermediate planes plab1 / vxy / strength are written as well (tests, debug planes)
int grad_nms_fits(int iw, int ih);
void grad_nms(hipStream_t s, float *nms, float *const bl[3], int iw, int ih, int nz = 1, size_t zs = 0, uint32_t *tap_plab1 = nullptr, float *tap_vxy = nullptr, float *tap_strength = nullptr);
void threshold_f(hipStream_t s, float *out, const float *in, float lo, float thr, float hi, int n);
void threshold_i(hipStream_t s, int *out, const int *in, int lo, int thr, int hi, int n);
void cast_i_f(hipStream_t s, int *out, const float *in, float scale, int n);
void cast_c_i(hipStream_t s, int8_t *out, const int *in, int n);
void clear_i(hipStream_t s, int *out, int n);
void copy_i(hipStream_t s, int *out, const int *in, int n);
void rand_i(hipStream_t s, int *out, uint64_t seed, int n);

// ---- rd_k_label.hip: connected components and per-label reductions
// 8-connected components of equal `pix` value, pixels equal to bgc -> -1, label = smallest pixel index
void label8(hipStream_t s, int *label, const int *pix, int bgc, int iw, int ih, int skip_flatten = 0);   // label = smallest index of the 8-connected component of equal value, -1 for bgc; skip_flatten: the final walk to the roots is left to calc_strength(flatten = 1)
void label8_tidy(hipStream_t s, int *label, int *mask0, int *tidy, const float *nms, int *zero_plane, int iw, int ih, int skip_flatten = 0, int nz = 1, size_t zs = 0);   // rect_tidy + label8(tidy, background -1) in the same tile kernel
// flatten = 0: the component plane is left as the union-find forest of the tile and border kernels and its readers - votes, probes - walk to the roots themselves
// (-DRD_BOUNDARY_FLATTEN=0, tuning builds).  Built in round 6, lists identical, and NOT the default: k_label_flatten 5.6 -> 0.9 us per frame, but the 7x7 windows of
// k_reduce_claim then walk (7.6 -> 14.4 us) - 2883-2899 against 2879-2892 frames/s, nothing.  profiles/NOTES_r06.md.
#ifndef RD_BOUNDARY_FLATTEN
#define RD_BOUNDARY_FLATTEN 1
#endif
void label8_boundary(hipStream_t s, int *label, int *marks, const int *region, int iw, int ih, int *vt_table = nullptr, int *vt_claim = nullptr, int *vt_list = nullptr, int nz = 1, size_t zs = 0, int flatten = 1);
void label8_flatten(hipStream_t s, int *label, int n);      // phase 3 alone, later (debug plane)   // mark_boundary + label8(marks, background -1) with the marking fused into the tile kernel
// add (optional): a plane whose non-zero elements are added to out element by element in the same launch (out = zeros + add + sums)
void calc_strength(hipStream_t s, int *out, const float *edge, int *label, int iw, int ih, const int8_t *add = nullptr, int flatten = 0, int nz = 1, size_t zs = 0);   // add (optional): a 0/1 byte plane added to the sums (H1)
void filter_strength(hipStream_t s, int *label, const int *str, int thre, int iw, int ih);
// poly kind (rd_polyline_detector_create): components of nms > 0 (background -> -1, label = smallest pixel index, no tidy) in the tile kernel, which writes the
// 0/1 mask plane the border kernel reads and clears zero_plane (the strength sums); then filterStrength(thre) + `label > 0` as a bit plane for the polyline stage
void label8_positive(hipStream_t s, int *label, int *mask, const float *nms, int *zero_plane, int iw, int ih, int skip_flatten, int nz = 1, size_t zs = 0);
void poly_mask_bits(hipStream_t s, unsigned long long *bits, const int *label, const int *str, int thre, int iw, int ih, int nz = 1, size_t zs = 0);
// strong mask at t_strong (two copies) + edge mask at t_edge (int, int8), both from the unfiltered labels, + filter_strength at t_strong (label in place), one pass; t_edge <= t_strong
// prev (optional): a 0/1 byte plane added to the sums element by element (sum of label l = str[l] + prev[l]: quirk H1 without a pass of its own); strong2 != prev
// the strong masks of the nz frames of a group launch (frame z = sequence number t0 + z, planes zs bytes apart, masks in ring planes (t0 + z + 1) mod nring) in one launch
int strength_masks_group_fits(int iw, const void *label, const void *ring, const void *edge8, size_t zs);
void strength_masks_group(hipStream_t s, int8_t *ring, int8_t *edge8, int *label, const int *str, int t_edge, int t_strong, int iw, int ih, unsigned long long *bits, long t0, int nring, int nz, size_t zs);
void strength_masks(hipStream_t s, int *strong, int8_t *strong2, int *edge /* may be NULL */, int8_t *edge8, int *label, const int *str, int t_edge, int t_strong, int iw, int ih, const int8_t *prev = nullptr, unsigned long long *bits = nullptr);   // bits (optional): the strong mask as a bit plane too (ceil(iw / 64) words per row); strong may then be null

// ---- rd_k_rect.hip: rect-path stages
// "counted" / "curve end" bit rows of the strong mask's junction counts (oclrect.cl:74-95), 2 words per 64 pixels: what merge_mask() reads
void junction_bits(hipStream_t s, unsigned long long *bits, const unsigned long long *strong, int iw, int ih, int nz = 1, size_t zs = 0);
// run extents of the edge-stopped blur (depend on the edge mask only): ext[p] = nl_h | nr_h<<3 | nl_v<<6 | nr_v<<9
void blblur_extents(hipStream_t s, uint16_t *ext, const int8_t *edge, int iw, int ih, int nz = 1, size_t zs = 0);
// one horizontal + vertical pass pair; out must not alias in
void blblur_pair(hipStream_t s, uint32_t *out, const uint16_t *ext, const uint32_t *in, int iw, int ih, int nz = 1, size_t zs = 0);
void quant_lut_init(hipStream_t s);   // once per device before the first despeckle(quantize24 = 1): builds the 24-level quantisation tables on the device
void despeckle(hipStream_t s, uint32_t *out, const uint32_t *in, const float *edge, int iw, int ih, int quantize24, int nz = 1, size_t zs = 0);   // quantize24: `in` is quantised to 24 levels per field on the fly
void merge_mask(hipStream_t s, unsigned long long *out, const unsigned long long *bits, int iw, int ih, int nz = 1, size_t zs = 0);   // out: bit plane, ceil(iw / 64) words per row
// oclrect.cl:289-334 with the work-items of a launch concurrent (rd_k_rect.hip: k_region_init = the links and launch 0, k_region_round = the others).
// mask / edge: the merge mask and the strong mask as bit planes.
// launches: even, 2..RD_REGION_MAX_LAUNCHES (launches after one that changed nothing return at once; flag r of scratch[N + r] = launch r changed something);
// size_out (optional) <- the junction counts of the strong mask (what the reference's size plane holds when the counting starts: quirk H2), for region_size;
// scratch: 3N + 256 ints; *marked <- 1: `label` is left as label << 3 | mark words, which region_size(…, marked) turns into plain labels
void region_merge(hipStream_t s, int *label, int *scratch, const int *pix, const unsigned long long *mask, const unsigned long long *edge, int iw, int ih, int launches,
                  int *size_out, int *marked, int nz = 1, size_t zs = 0);
void region_size(hipStream_t s, int *out, int *label, int n, int *zero_me, int marked = 0, int nz = 1, size_t zs = 0);   // accumulates into out; zero_me (optional): an int to clear on the way
#define RD_D2_SCRATCH_INTS(N) (5 * (size_t)(N) + 64)
// The region merge is launched until a launch changes nothing - at most RD_REGION_MAX_LAUNCHES times (the definition's limit: DESIGN.md, "Region stages").  Its
// flag words (one per launch) are followed by the status words of the absorption at RD_REGION_STATUS_AT.  (Round 6: 128 - one 3840x2160 frame of the held-out stream needs 86,
// two 1920x1080 frames 49; the limit had been 64.)
#define RD_REGION_MAX_LAUNCHES 128
#define RD_REGION_STATUS_AT 128
// absorption of small regions (oclrect.cl:348-371) exactly as the reference's serial raster order gives it.  out != in; scratch: RD_D2_SCRATCH_INTS(N) ints
// (scratch[N] = 0 already if count_is_zero); status: 3 device ints, [0] != 0 <=> not finished (out holds negative words): run despeckle2_slow()
void despeckle2(hipStream_t s, int *out, const int *in, int *scratch, const int *size, int thre, int iw, int ih, int count_is_zero, int *status, int nz = 1, size_t zs = 0);
int despeckle2_slow(hipStream_t s, int *out, const int *in, int *scratch, const int *size, int thre, int iw, int ih);   // the same result for any input; synchronises s (not for captured streams); returns its launches of the rounds
// launches of the rounds after which despeckle2_slow() calls a frame without a fixed point an internal error (a dependency chain moves at least one pixel right or
// one row down per link: iw + 2 * ih bounds its length, and every launch settles two links)
static inline int despeckle2_slow_bound(int iw, int ih) { return iw + 2 * ih + 16; }
#define RD_REGION_FIRST_BUDGET 20      // the largest budget a frame is launched with (rd_frames.hip: kRoundBudgets); a frame still changing in its last launch climbs the ladder (region_ladder)
// the budget after `budget` on that ladder: 32, then doubled up to the definition's limit; 0: there is none
static inline int region_ladder_next(int budget) { const int b = budget < 32 ? 32 : budget * 2; return b <= RD_REGION_MAX_LAUNCHES ? b : 0; }
#define RD_ABSORB_THRE 16              // regions of at most this many pixels (junction counts included: quirk H2) are absorbed (oclrect.c:337)
// the constants the crafted cases of the region stage are built from (rd_region_limits; the header documents the order)
void region_limits(int iw, int ih, int out[32]);
struct PolyScratch;
struct PolyFrame;      // rd_poly_scratch.h: per-frame descriptor of the sparse stages; launches cover nb <= RD_MAXB frames (frame = blockIdx.z), descriptors in HOST memory
void reduce_ls_init(hipStream_t s, int *table, int *claim, int *tlist, int nentry);   // once per allocation
// votes of the chain pixels left in each frame's scratch by the last polyline() call (their final segment ids) into frames[z].table
void reduce_ls(hipStream_t s, const PolyFrame *frames, int nb, int iw, int ih, int nentry, int tables_are_clean = 0);   // tables_are_clean: label8_boundary(vt_*) has undone the previous use already
// The hand-over block: what the host needs from a frame, written by the frame's last kernel (k_sample_segments; the polyline kind's k_poly_handoff) straight into the
// slot's pinned host memory (PolyFrame::pack) and read there by the poll.  Ints:
#define RD_PACK_POLYCTR 0              // [0, 32): the polyline stage's counters 0..31 (poly_scratch_counters)
#define RD_PACK_POLYCTR_INTS 32
#define RD_PACK_GAVE_UP 25             //   of them: != 0, the single-block polyline kernel gave up on the frame (its on-chip tables are too small)
#define RD_PACK_FLAGS 32               // [32, 52): the region merge's flags of its first RD_REGION_FIRST_BUDGET launches (!= 0: that launch changed something)
#define RD_PACK_STATUS 52              // [52, 60): the absorption's status words ([0] != 0: the fast path gave up)
#define RD_PACK_STATUS_INTS 8
#define RD_PACK_RECORDS 64             // the segment list from its header record on, RD_REC_INTS ints per record (linesegment_t, 56 bytes)
#define RD_REC_INTS 14
#define RD_PROBE_INTS (15 * 6)         // behind the block's records: the probes, this many ints per record (15 probe points of 6 values)
static_assert(RD_PACK_FLAGS == RD_PACK_POLYCTR + RD_PACK_POLYCTR_INTS && RD_PACK_STATUS == RD_PACK_FLAGS + RD_REGION_FIRST_BUDGET && RD_PACK_STATUS + RD_PACK_STATUS_INTS <= RD_PACK_RECORDS,
              "the hand-over block's parts lie back to back in front of the records");
// per segment, 15 probe points: {boundary id, table slot owner, 4 box values} -> out[(seg*15 + k)*6 ..]
// pack (may be null): the hand-over block - counters / flags, pack_records records, then their probes
void sample_segments(hipStream_t s, const PolyFrame *frames, int nb, int max_records, int iw, int ih, int nentry, int pack_records);
// the constants the crafted cases of the vote stage are placed by (rd_votes_limits; the header documents the order)
void votes_limits(int out[24]);

// ---- rd_k_post.hip: segments + probes -> rectangles on the device (candidate funnel + pose estimation, one wave per candidate)
size_t post_scratch_ints();      // ints of PolyFrame::post_scratch
size_t post_out_ints();          // ints of PolyFrame::post_out
void post_limits(int out[8]);    // POST_HT, POST_MAXG, POST_MAXC, POST_MEMBERS, POST_CAP, POST_WAVES, RDP_HULL_DEPTH, RDP_POOL_INTS(POST_CAP)
void post_device(hipStream_t s, const PolyFrame *frames, int nb, int max_records, int iw, int ih, double tanAOV);

// ---- rd_k_poly.hip: polyline stage on compacted chain pixels
PolyScratch *poly_scratch_create(int iw, int ih);
void poly_scratch_destroy(PolyScratch *ps);
const int *poly_scratch_counters(const PolyScratch *ps);   // device pointer: [0] chain pixels, [1] chains, [2+r] split candidates of round r
void poly_limits(int out[4]);    // the single-block kernel's PP_T * PP_PX live pixels, PP_MAXSEG records, PP_MAXCAND candidates per round, bits of a record id
// frames: nb descriptors (host memory); frames[z].ring_src: plane whose 2-px frame ring supplies the stale ring values (null -> ring_const)
void polyline(hipStream_t s, const PolyFrame *frames, int nb, int lslist_bytes, int ring_const, float minerror, int sizeThre, int iw, int ih, int mode);
// poly kind: counters + the first `records` records of each frame's list (header included) into frames[z].pack (pinned host memory)
void polyline_handoff(hipStream_t s, const PolyFrame *frames, int nb, int records);
// materialises the dense id planes frames[z].ids from the compact state
void polyline_ids(hipStream_t s, const PolyFrame *frames, int nb, int n);

// ---- rd_k_rectify.hip: rectified patches (the contract: rectdetect_hip.h, "rectified patches")
// what a job uploads per quad: the coefficients a, b, c, d, e, f, g, h of rd_rectify_coefficients and the quad's status (0: an all-zero patch)
struct RectifyQuad { double c[8]; int status; int pad; };
// n patches of pw x ph BGR pixels, patch k at out + k * pw * ph * 3, from one frame in format fmt (RD_PIX_*), one launch (quad = blockIdx.z)
void rectify(hipStream_t s, uint8_t *out, int fmt, const rdpix::PixFrame &src, const RectifyQuad *quads, int n, int pw, int ph);

// ---- rd_k_tensor.hip: model-ready tensors (the contract: rectdetect_hip.h, "model-ready tensors")
// n tensors of pw x ph elements in the dtype, layout and channels of spec (legal for pw x ph: rd_tensor_spec_ok), quad k's at out + k * rd_tensor_bytes(spec, pw, ph),
// from one frame in format fmt (RD_PIX_*), one launch (quad = blockIdx.z)
void rectify_tensor(hipStream_t s, void *out, int fmt, const rdpix::PixFrame &src, const RectifyQuad *quads, int n, int pw, int ph, const rd_tensor_spec &spec);

// ---- rd_k_scan.hip: scanned pages (the contract: rectdetect_hip.h, "scanned pages")
// n pages of pw x ph pixels in the mode of spec (legal for pw x ph: rd_scan_spec_ok), quad k's at out + k * rd_scan_bytes(spec, pw, ph), from the G plane
// rectify_tensor made of the same quads with { U8, NHWC, GRAY, spec.oversample } (quad k's at plane + k * pw * ph), one launch (quad = blockIdx.z)
void scan(hipStream_t s, uint8_t *out, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_scan_spec &spec);

// ---- rd_k_grade.hip: graded quads (the contract: rectdetect_hip.h, "graded quads")
// the records (and histograms) of n quads of pw x ph pixels under spec (legal for pw x ph: rd_grade_spec_ok) ADDED to quad k's rd_grade_bytes(spec, pw, ph) bytes at
// out + k * that (8-byte aligned; cleared by the caller, on s), from the G plane rectify_tensor made of the same quads with { U8, NHWC, GRAY, spec.oversample }
// (quad k's at plane + k * pw * ph), one launch (quad = blockIdx.z); an invalid quad's bytes are left as they are
void grade(hipStream_t s, uint8_t *out, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_grade_spec &spec);

// ---- rd_k_code.hip: decoded quads (the contract: rectdetect_hip.h, "decoded quads")
// the rd_code records of n quads of pw x ph pixels under spec (legal for pw x ph: rd_code_spec_ok), quad k's WRITTEN whole to out + k * 48 (8-byte aligned; zeros for an
// invalid quad), from the G plane rectify_tensor made of the same quads with { U8, NHWC, GRAY, spec.oversample } (quad k's at plane + k * pw * ph) and ndict <= 4096
// codes in device memory (dict may be null when ndict is 0), one launch (quad = blockIdx.x).  The kernel reads WHOLE 16-byte words: up to 15 bytes in front of a quad's
// plane (its neighbour's) and up to 15 behind the last one - so plane must lie on a 16-byte boundary and plane_bytes, the readable bytes from there, must be at least
// n * pw * ph + RD_CODE_PLANE_PAD; the launcher aborts otherwise
void code(hipStream_t s, uint8_t *out, const uint8_t *plane, size_t plane_bytes, const RectifyQuad *quads, int n, int pw, int ph, const rd_code_spec &spec, const uint64_t *dict, int ndict);

// ---- rd_k_blob.hip: page components (the contract: rectdetect_hip.h, "page components")
// radius == 0: the ink bits of n quads, ink = (inverted) G <= spec.k, quad k's ((pw + 7) >> 3) * ph bytes at bits + k * that in the RD_SCAN_BITS layout, from the G plane
// rectify_tensor made of the same quads; an invalid quad's bits are left as they are (the component stage never reads them), one launch
void blob_level(hipStream_t s, uint8_t *bits, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_blob_spec &spec);
// the component stage: steps 2-7 of n quads under spec (legal for pw x ph: rd_blob_spec_ok), quad k's rd_blob_bytes(spec, pw, ph) bytes at out + k * that (8-byte
// aligned; zeroed here, on s).  labels, areas: n * pw * ph ints each, both overwritten; the quads' ink bits lie at the START of areas, quad k's at
// (uint8_t *)areas + k * ((pw + 7) >> 3) * ph in the RD_SCAN_BITS layout (pad bits ignored).  quads may be null: every quad is valid (the test tap); otherwise an
// invalid quad's bytes stay zero.  Three memsets and four or five launches (quad = blockIdx.z).  info (may be null): what rd_blobs_pages_device reports
void blobs(hipStream_t s, uint8_t *out, int *labels, int *areas, const RectifyQuad *quads, int n, int pw, int ph, const rd_blob_spec &spec, int info[8]);

// ---- rd_k_match.hip: matched quads (the contract: rectdetect_hip.h, "matched quads")
// the signatures of n quads of one frame: quad k's G * G int8 values at sig + k * G * G (zeros for an invalid quad), its sa, saa ADDED to sums[2k], sums[2k+1]
// (cleared by the caller); G in {8, 16, 32, 64}, m in {1, 2, 4}
void match_signatures(hipStream_t s, int8_t *sig, int *sums, int fmt, const rdpix::PixFrame &src, const RectifyQuad *quads, int n, int G, int m);
// dots[q * ld + c] = signature q . column c for q < n rounded up to 16, c < ncols rounded up to 16: sig, lib and dots hold the padding rows and columns
void match_dots(hipStream_t s, int *dots, int ld, const int8_t *sig, int n, const int8_t *lib, int ncols, int D);
// the records of n quads, without their scores; colsums: sb, sbb per column
void match_pick(hipStream_t s, rd_match *recs, const int *dots, int ld, const int *colsums, int ncols, const int *sums, const RectifyQuad *quads, int n, int D);
// the four columns of a template (lib4: 4 * G * G bytes) from its signature
void match_rotations(hipStream_t s, int8_t *lib4, const int8_t *sig, int G);

// ---- rd_k_annotate.hip: annotated frames (the contract: rectdetect_hip.h, "annotated frames")
// what a job uploads per primitive: its line record (rd_annot_cover.h) and its colour - the three bytes a covered pixel gets, in the order the frame's format
// stores them (BGR / BGRA: b, g, r; RGB / RGBA: r, g, b; NV12 / I420: y, u, v of rd_annot_yuv) - as col = c0 | c1 << 8 | c2 << 16
struct AnnotRec { rd_annot_line L; uint32_t col; uint32_t pad; };
enum { ANNOT_TILE_W = 64, ANNOT_TILE_H = 32, ANNOT_CHUNK = 256 };      // a block's tile of pixels; primitives tested per pass = records of the tile's list in LDS at a time
// n primitives drawn into one frame in format fmt (dst and src: the same size), one launch, one block per tile.  dst == src plane by plane: in place (only covered pixels are written,
// with clear every pixel); otherwise every pixel of dst is written once: the source's, black, or a primitive's colour.  clear: RD_ANNOT_CLEAR.
void annotate(hipStream_t s, int fmt, const rdpix::PixFrame &dst, const rdpix::PixFrame &src, const AnnotRec *recs, int n, int clear);

// ---- rd_k_remap.hip: remapped frames (the contract: rectdetect_hip.h, "remapped frames")
// the entries of a row of the table as the kernel reads it: ow rounded up to 4, so that a thread's 4 entries are 32 aligned bytes; the padding entries are (-1, -1)
int remap_table_pitch(int ow);
// an ow x oh BGR frame (rows out_pitch bytes apart, 3 * ow of them written) from one frame in format fmt (RD_PIX_*) through `table`: oh rows of
// remap_table_pitch(ow) entries xi, yi, 256-byte aligned, every inside entry within src; outside entries get fill_bgr (B | G << 8 | R << 16)
void remap(hipStream_t s, uint8_t *out, int out_pitch, int fmt, const rdpix::PixFrame &src, const int32_t *table, int ow, int oh, uint32_t fill_bgr);

}  // namespace rdk
