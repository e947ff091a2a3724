/*
 * rectdetect-mi355x: entry points beyond the reference's own headers.  Plain C ABI (pointers and sizes only).
 *
 * The reference API (oclrect.h) takes HOST frames, so each call pays a PCIe upload.  The rd_* functions below let a
 * caller keep frames resident in HBM, run many frames through a multi-stream pipeline with the host post-process
 * on worker threads, and look at intermediate planes (tests).  Semantics of the detector are unchanged.
 */
#ifndef RECTDETECT_HIP_H
#define RECTDETECT_HIP_H
#include <stddef.h>
#include <stdint.h>
#if defined(__cplusplus)
extern "C" {
#endif

const char *rd_version(void);
int rd_device_count(void);                  /* number of HIP devices visible to this process */
void rd_select_device(int ordinal);         /* device used by simpleGetDevice(0) and new detectors (default 0) */
int rd_device_pci_bus_id(int ordinal, char *buf, int len);   /* "0000:c1:00.0" into buf (len >= 16); 0 on success: for pinning a per-GPU host process to the GPU's NUMA cores */

/* device memory helpers for callers without a HIP binding of their own (tests, bench) */
void *rd_device_alloc(size_t bytes);
void rd_device_free(void *dptr);
void *rd_host_alloc(size_t bytes);           /* pinned (page-locked) host memory: see RD_FRAME_HOST_PINNED */
void rd_host_free(void *p);
void rd_upload(void *dptr, const void *host, size_t bytes);
void rd_download(void *host, const void *dptr, size_t bytes);

/* ---- one detector instance = one stream of frames (state carried between frames) */
typedef struct rd_detector rd_detector;

/* nslots frames in flight (>= 1); nworkers != 0: the host post-process runs on worker threads, ONE PER SLOT (the value itself is
 * not a thread count), 0: on the polling thread.
 * 1-2 frames in flight: a frame spreads over two HIP streams (shortest latency); from 3 on: one stream per frame, and frames
 * beyond the fourth queue up on the same four streams (the device runs four hardware queues side by side).  From 6 slots on the
 * frames of two consecutive slots, from 12 on of four, from 32 on of eight, run as ONE set of launches (group launches: a frame waits until its group is
 * full or a poll asks for it - then it is launched on its own); 64 is what bench.py runs ("Data layout in HBM, execution"). */
rd_detector *rd_detector_create(int device, int iw, int ih, int nslots, int nworkers);
void rd_detector_destroy(rd_detector *d);

/* The second kind of detector: line segments, what poly.cpp / vidpoly.cpp compute per frame (poly.cpp: strength_thre 500, minerror 1, size_thre 20;
 * vidpoly.cpp: 2000, 1, 10), with nslots frames in flight in the same slots, groups, graphs and streams as the rectangle kind.  Every frame starts afresh
 * (no state carried between frames).  NULL on invalid arguments (iw or ih < 16, nslots < 1, minerror <= 0, size_thre < 0, strength_thre < 0, no such device).
 * rd_detector_enqueue (all three frame kinds), rd_detector_drain, rd_detector_destroy, rd_detector_counter and rd_detector_debug_plane work on it as on
 * the rectangle kind; rd_detector_poll on it is fatal, as is rd_detector_poll_segments on a rectangle detector. */
rd_detector *rd_polyline_detector_create(int device, int iw, int ih, int nslots, int strength_thre, float minerror, int size_thre);
/* Result of the oldest frame not yet polled: a malloc'd linesegment_t array (56 bytes each) exactly as oclpolyline_execute leaves lsList - record 0 is the
 * header (its first int = n), records 1..n follow, those with polyid == 0 included - owned by the caller.  Blocks until that frame is done.  ids_out != NULL:
 * also the frame's per-pixel segment ids (iw * ih ints, oclpolyline_execute's lsIdOut), produced only when asked for. */
void *rd_detector_poll_segments(rd_detector *d, int32_t *ids_out);

/* Detectors with one or two frames in flight take their HIP streams from a process-wide cache (hardware queues of their own: DESIGN.md) and hand them back when they
 * are destroyed, so that the next detector runs on the same queues.  This destroys the cached streams of `device` (-1: all devices); live detectors are not affected. */
void rd_release_cached_streams(int device);

/* Enqueue one BGR frame (row stride ws bytes).  Where the frame lies (`on_device`):
 *   RD_FRAME_HOST (0)         host memory of any kind; copied before the call returns (the reference's oclrect_enqueueTask does the same, oclrect.c:1256), the caller may
 *                             reuse the buffer at once
 *   RD_FRAME_DEVICE (1)       a device pointer, read in place: must stay valid and unchanged until the matching rd_detector_poll returned
 *   RD_FRAME_HOST_PINNED (2)  PINNED host memory (rd_host_alloc, allocatePinnedMemory of oclhelper.h, hipHostMalloc, or registered with hipHostRegister): the copy engine
 *                             reads it in place - no copy by the caller's thread (6 MB per 1920x1080 frame) - so it must stay unchanged until the matching poll returned,
 *                             like a device pointer; memory that is not pinned is refused (fatal)
 * Returns the frame's sequence number. */
#define RD_FRAME_HOST 0
#define RD_FRAME_DEVICE 1
#define RD_FRAME_HOST_PINNED 2
long rd_detector_enqueue(rd_detector *d, const void *frame, int ws, int on_device);

/* Enqueue one frame in another pixel format: what video decoders, renderers and image libraries hand out, without a BGR copy of it.
 * planes[k] / pitches[k]: plane k and its row stride in bytes (planes a format does not use are ignored).  on_device, the frame kinds and their contracts as for
 * rd_detector_enqueue (host: copied before the call returns; device and pinned: read in place until the frame's poll; under RD_FRAME_HOST_PINNED every plane
 * the format uses must be pinned - fatal otherwise, as is a call with nslots frames already in flight).  Both detector kinds; the format may change from frame to frame.
 * Returns the frame's sequence number, or -1 for an argument error, in which case nothing was enqueued: an unknown format or on_device, a NULL plane the format
 * uses, a pitch smaller than its plane's row, NV12 / I420 with an odd iw or ih.  RD_PIX_BGR is rd_detector_enqueue(d, planes[0], pitches[0], on_device).
 *
 * Conversion contract.  The packed formats are a permutation of their bytes into (B, G, R).  NV12 and I420 are BT.601 limited range with 2x2 nearest chroma
 * (OpenCV's cvtColor COLOR_YUV2BGR_NV12 / _I420 fixed point): pixel (x, y) takes U and V at chroma (x/2, y/2) and, in int32 with arithmetic shifts,
 *   u = U - 128;  v = V - 128;  yy = max(Y - 16, 0) * 1220542
 *   R = clamp((yy + 1673527*v             + (1 << 19)) >> 20, 0, 255)
 *   G = clamp((yy -  852492*v - 409993*u  + (1 << 19)) >> 20, 0, 255)
 *   B = clamp((yy + 2116026*u             + (1 << 19)) >> 20, 0, 255)
 * The (B, G, R) goes through the detector's sRGB -> Lab arithmetic unchanged: the result for such a frame is bit-identical to the result for the BGR frame
 * this formula gives. */
#define RD_PIX_BGR  0   /* 3 bytes per pixel B,G,R: what rd_detector_enqueue takes */
#define RD_PIX_RGB  1   /* 3 bytes per pixel R,G,B */
#define RD_PIX_BGRA 2   /* 4 bytes per pixel B,G,R,A (A ignored) */
#define RD_PIX_RGBA 3   /* 4 bytes per pixel R,G,B,A (A ignored) */
#define RD_PIX_NV12 4   /* plane 0: Y, iw x ih; plane 1: U,V interleaved, iw bytes x ih/2 rows */
#define RD_PIX_I420 5   /* plane 0: Y, iw x ih; plane 1: U, plane 2: V, each iw/2 x ih/2 */
long rd_detector_enqueue_planes(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int on_device);

/* Enqueue one frame that is LARGER than the detector: detection at half the camera's size, with the 2x2 box downscale done by the front kernel as it reads.
 * scale 1: exactly rd_detector_enqueue_planes(d, format, planes, pitches, on_device).
 * scale 2: the source frame is 2*iw x 2*ih pixels in `format` - all six RD_PIX_* formats, BGR included; planes and pitches laid out as for
 *   rd_detector_enqueue_planes at the SOURCE size.  Such a source is even in both directions, so NV12 and I420 are accepted for odd iw or ih of the detector too.
 *   With p_c(X, Y) the channel c (B, G, R) of source pixel (X, Y) under the conversion contract above, detector pixel (x, y) is, in int32,
 *     out_c(x, y) = (p_c(2x, 2y) + p_c(2x+1, 2y) + p_c(2x, 2y+1) + p_c(2x+1, 2y+1) + 2) >> 2
 *   NV12 and I420: each of the four source pixels is converted first - its own Y, the U and V the four share - and the four (B, G, R) are averaged afterwards (the
 *   order the rectifier uses for its taps).  The result for such a frame - every plane, every list - is bit-identical to the result of rd_detector_enqueue on the
 *   BGR frame this formula gives.  (Believed equal to what OpenCV's cv::resize(..., INTER_AREA) gives at exactly half size; not checked.)
 * Any other scale: -1.
 * Frame kinds, their lifetime rules and both detector kinds as for rd_detector_enqueue_planes; format and scale may change from frame to frame.  A device frame is read
 * in place.  A host or pinned frame at scale 2 needs up to 16 bytes per detector pixel on the device: a slot gets a pair of staging buffers of that size with the
 * first such frame it takes (rd_detector_counter 33); a detector that never takes one allocates nothing more.
 * Returns the frame's sequence number, or -1 for an argument error, in which case nothing was enqueued: an unknown format, on_device or scale, a NULL plane the
 * format uses, a pitch smaller than the SOURCE plane's row.  A bad handle and a call with nslots frames already in flight are fatal.
 *
 * rd_detector_rectify_polled (below) on a slot whose frame came in at scale 2 takes `quads` in DETECTOR coordinates - what rd_rect_quads gives for that frame's
 * rectangles - and cuts the patches out of the full-size SOURCE: each corner is mapped on the host, in double, uncontracted,
 *     X = x * 2.0 + 0.5;   Y = y * 2.0 + 0.5
 * (pixel centres sit at integers, so detector pixel x covers source pixels 2x and 2x+1 and its centre lies at 2x + 0.5), and the job runs on the source planes
 * with the source's width and height: the patch equals what rd_rectifier_enqueue gives for the full-size frame and the mapped quads.  A caller with a rectifier
 * job of their own maps the corners the same way. */
long rd_detector_enqueue_scaled(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int scale, int on_device);

/* Result of the oldest frame not yet polled: malloc'd array of rect_t-compatible records (176 bytes each, element 0
 * holds nItems), owned by the caller.  Blocks until that frame is done. */
void *rd_detector_poll(rd_detector *d, double tanAOV);

/* optional: the aperture (tan of half the horizontal angle of view) the polls to come will pass.  The reference's API hands it over with
 * the poll, after the frame; work that runs ahead of the poll (worker threads, RD_DEVICE_POST=1) uses the last one seen, so without this
 * call the first frames of a stream are post-processed at poll time on the polling thread. */
void rd_detector_set_aperture(rd_detector *d, double tanAOV);

/* device-side work only (no host post-process): waits until every enqueued frame has left the GPU */
void rd_detector_drain(rd_detector *d);

/* copy of the line-segment list of the most recently POLLED frame: returns n (records 1..n), writes up to max records */
int rd_detector_last_segments(rd_detector *d, void *dst, int max_records);

/* Counters since creation (`which`; the numbers are part of the ABI); -1 for a number that is none of them.
 * The polyline kind keeps 0, 1, 2, 3, 15, 18, 19 and 30..33; the region, post-process and strong-mask counters stay 0 there. */
enum rd_counter {
  RD_CTR_POLY_REDONE = 0,            /* frames whose polyline stage did not fit the single-launch kernel's on-chip tables and was repeated with the multi-launch path (same results, slower) */
  RD_CTR_DEVICE_US = 1,              /* device microseconds summed over the polled frames (HIP events on the frame's stream: first kernel start to last copy end, so concurrent frames overlap) */
  RD_CTR_DEVICE_FRAMES = 2,          /* frames in that sum */
  RD_CTR_ENQUEUE_US = 3,             /* host microseconds spent inside rd_detector_enqueue */
  RD_CTR_REGION_REDONE = 4,          /* frames whose region merge had not settled within their launch budget and were repeated with more launches (32, then 64, then 128) */
  RD_CTR_REGION_BUDGET = 5,          /* the current launch budget of the region merge (8, 10, .. 20) */
  RD_CTR_REGION_UNSETTLED = 6,       /* frames still changing after 128 launches (none so far) */
  RD_CTR_PROBES_REGROWN = 10,        /* frames with more line segments than a slot's probe buffer holds (65535), whose probes were taken again into a larger buffer (the list keeps
                                        the reference's capacity of 16N / 56 records; nothing is dropped) */
  RD_CTR_POST_DEVICE = 11,           /* frames whose rectangles came from the device post-process (RD_DEVICE_POST=1: candidate funnel + pose estimation in rd_k_post.hip) */
  RD_CTR_POST_HOST = 12,             /* frames whose rectangles came from the host post-process */
  RD_CTR_POST_HOST_US = 13,          /* microseconds the worker threads spent in the host post-process (sum over frames) */
  RD_CTR_ABSORB_SLOW = 14,           /* frames whose small-region absorption (oclrect.cl:348-371) was finished by the slow path - rounds over work lists until nothing changes -
                                        because they left more undecided pixels than the single-block tail holds (frames made of small regions) */
  RD_CTR_FRAMES_PER_LAUNCH = 15,     /* frames per group launch (1: every frame its own launches) */
  RD_CTR_STRONG_ONE_LAUNCH = 16,     /* groups whose strong masks took one launch */
  RD_CTR_STRONG_BY_FRAME = 17,       /* groups whose strong masks took one launch per frame */
  RD_CTR_FRAMES_PINNED = 18,         /* frames that travelled straight from the caller's pinned memory (RD_FRAME_HOST_PINNED) */
  RD_CTR_FRAMES_COPIED = 19,         /* host frames copied into the detector's own pinned staging first (RD_FRAME_HOST) */
  RD_CTR_BUDGET_FRAMES = 20,         /* 20..26: frames launched with a budget of 8 / 10 / .. / 20 launches of the region merge */
  RD_CTR_LONG_LISTS = 30,            /* polyline kind: frames whose segment list was longer than the block handed to pinned host memory at the end of the frame and was fetched by the poll */
  RD_CTR_SLOT_BYTES = 31,            /* device bytes of one slot's planes (both kinds; the polyline stage's compact scratch, the same for both, not included) */
  RD_CTR_HANDOFF_RECORDS = 32,       /* records of the block handed to pinned host memory at the end of a frame (header included) */
  RD_CTR_SCALED_STAGING_BYTES = 33,  /* device bytes of the scaled-source staging a slot owns once it has taken a host or pinned frame at scale 2 (rd_detector_enqueue_scaled; as many
                                        bytes again of pinned host memory go with it), 0 until a slot has - RD_CTR_SLOT_BYTES does not include them */
  RD_CTR_NEED_FRAMES = 40            /* 40 + k, k = 0..20: frames whose region merge needed k launches (the one that changes nothing included; 20: or more) */
};
long rd_detector_counter(rd_detector *d, int which);

/* ---- Environment.  Everything is read when a detector is created (rd_detector_create / init_oclrect) and never again; an empty value counts as unset.
 *   for users:   RD_DEVICE_POST=0|1      candidate funnel + pose estimation on the device (rd_k_post.hip) instead of the host threads (default: host, unless the process may
 *                                        use no more than two cores).  The device holds fixed tables; a frame beyond any of them is flagged there and post-processed
 *                                        on the host instead (counter 12 instead of 11), which has no such bounds (rd_post.c grows its work space): more than 8192 distinct boundary ids under the probes,
 *                                        2048 components with four or more segments, 1024 candidates (such components + polyline heads), 65536 (segment, component)
 *                                        pairs of those components, 160 segments in one candidate, or a convex hull whose construction goes deeper than 48 nested
 *                                        calls or needs more than 16 * 160 pool entries (rd_post_device_limits; each edge has a test in tests/test_gpu_post_device.py)
 *                RD_POST_HELPERS=n       helper threads that share a frame's pose estimations with the polling thread, reference-API shape only (default by core count, 0 = none)
 *                RD_NO_GRAPH=1           plain launches instead of captured hipGraphs
 *   test hooks:  RD_ZBATCH=k / RD_BATCH=k (frames per group launch / per set of sparse-stage launches), RD_REGION_ROUNDS_FIXED=8..20 and RD_BUDGET_CYCLE=n (launch budget of
 *                the region merge pinned / cycling), RD_POLY_MULTILAUNCH, RD_POLY_FORCE_REDO, RD_ABSORB_FORCE_SLOW (the fallback paths for every frame), RD_MAXREC_DEV=n (small
 *                probe buffers), RD_TEST_THRESHOLDS=a,b (strength thresholds), RD_STRONG_BY_FRAME (a group's strong masks frame by frame), RD_IIR_FORCE_FIX (every blur column
 *                through the full-length path; read per call).  Each is driven by a test in tests/test_gpu_parity.py.
 *                Polyline kind: RD_ZBATCH, RD_NO_GRAPH, RD_POLY_MULTILAUNCH and RD_POLY_FORCE_REDO as above, and RD_POLY_HANDOFF=n (records, header included,
 *                handed to pinned host memory at the end of a frame; default 2048) - driven by tests/test_gpu_polyline_stream.py.
 * Switches of experiments that were measured and not kept exist only in tuning builds (-DRD_TUNING, tools/variants.sh). */

/* Test hook: copy an internal plane of the most recently completed frame to host memory.  Returns bytes written,
 * 0 for an unknown name or a name of the other kind.  Both kinds are served from one table (rd_detector.hip).
 * Rectangle kind: plab0 plab1 lblur vxy strength nms mask0 tidy label1 strsum edge500 smooth quant strong junction mergemask
 * region0 (merged regions) rsize region (after absorbing small ones) boundarysrc boundary lsid table lslist (the segment list, 16 bytes per pixel)
 * polyctr (64 counters of the polyline stage) iirflags (16 ints) d2work (16 ints) absorb (8 status words of the absorption);
 * polyline kind: plab0 lblur nms mask0 (nms > 0) label1 (its components) strsum polymask (the traced mask, poly.cpp:121) lslist lsid polyctr.
 * A shorter buffer gets the first max_bytes bytes; of the planes kept in another shape on the device and handed out as ints (mask0 of the rectangle kind,
 * edge500, strong, junction, mergemask, polymask) the first max_bytes / 4 elements. */
size_t rd_detector_debug_plane(rd_detector *d, const char *name, void *dst, size_t max_bytes);

/* ---- host post-process alone (oclrect.c:1049-1226 restated): segments + samples -> rectangles.  Used by tests to
 * check the post-process against the reference with identical inputs.  `boundary` is the boundary-label plane,
 * `table` the reduceLS table (iw*ih*4/5 entries of 5 ints), `segs` the linesegment_t list with header. */
void *rd_postprocess_planes(const void *segs, const int32_t *boundary, const int32_t *table, int iw, int ih, double tanAOV);
/* test tap: the 15 probe pixels of a segment as the sampling kernel computes them (x, y pairs; (-1, -1): outside the frame) - compared with the oracle's
 * independent restatement of oclrect.c:1066-1083 */
void rd_probe_pixels(float x0, float y0, float x1, float y1, int iw, int ih, int32_t *out);
/* test tap: rd_postprocess_planes' twin on the device post-process (rd_k_post.hip), so that its capacity edges can be tested on crafted inputs.  Uploads the
 * list, the boundary plane and the vote table to `device`, takes the probes there (the frame path's sampling kernel) and runs the device post-process once, on a
 * stream, scratch and result block of its own, then frees everything.  The plane holds a component id per pixel: fatal in a -DRD_BOUNDARY_FLATTEN=0 tuning
 * build, whose sampling kernel follows the plane's values as links.  Returns the list exactly as a poll assembles it from the result block - the valid
 * candidates' records in candidate order, element 0 the header, malloc'd, owned by the caller - or NULL when the device flagged an overflow (the frame path
 * then hands the frame to the host post-process).  Either way info[0] = candidates counted (capped at the candidate capacity), info[1] = the overflow word,
 * info[2..7] = 0.  Needs a GPU (fatal without one); not called by the frame path. */
void *rd_postprocess_planes_device(int device, const void *segs, const int32_t *boundary, const int32_t *table, int iw, int ih, double tanAOV, int32_t info[8]);
/* the fixed capacities of the device post-process (see RD_DEVICE_POST under "Environment"): out[0] hash slots for distinct boundary ids under the probes, [1] components
 * with at least four segments, [2] candidates per frame (such components + polyline heads), [3] (segment, component) pairs of those components, [4] segments
 * per candidate, [5] waves per frame of the solving kernel (a candidate count above it only makes waves take several), [6] depth of the hull's explicit stack, [7] entries of
 * the hull's pool (the index lists of its pending calls).
 * Runs without a GPU. */
void rd_post_device_limits(int32_t out[8]);

/* test tap: the polyline stage alone (oclpolyline_execute's kernels, rd_k_poly.hip) on a caller's mask, in the form the caller names, so that the capacity edges of
 * its single-block kernel and crafted lists can be tested.  Uploads `mask` (iw * ih ints, zero / non-zero) to `device`, runs the stage and the id plane once, on a
 * stream and scratch of its own, then frees everything.  ring_nonzero: the value the 2-px frame ring of the bridging step's output takes (the reference leaves
 * that ring stale).  form 0 = the multi-launch form (what oclpolyline_execute runs), form 1 = the single-block kernel the detectors try first.  Out: lslist_out =
 * lslist_bytes bytes of the list (record 0 = header), ids_out = iw * ih ints, ctr_out = the stage's 64 counters ("polyctr" of rd_detector_debug_plane): [0] chain
 * pixels, [1] chains K, [2 + r] split candidates of round r (form 0), [24] live pixels, [25] != 0: the single-block kernel gave up - nothing repeats the stage
 * here, the list and the id plane are then not meaningful -, [39..45] 100 MHz time stamps of the single-block kernel's phases ([43], [44]: around the end-point join).
 * Returns 0, or -1 without touching the device for a null pointer, a plane smaller than 5 x 5 or larger than 65535 x 32767, a form other than 0 / 1, a negative
 * size_thre, or lslist_bytes outside [112, 16 * iw * ih].  Needs a GPU (fatal without one); not called by the frame path. */
int rd_polyline_planes_device(int device, const int32_t *mask, int iw, int ih, int ring_nonzero, float minerror, int size_thre, int lslist_bytes, int form,
                              void *lslist_out, int32_t *ids_out, int32_t ctr_out[64]);
/* the fixed capacities of the single-block kernel: out[0] live pixels (chain pixels of chains longer than size_thre), [1] records, header included (the largest
 * id is one less; at most [1] - 2 initial chains), [2] split candidates in one round, [3] bits of a record id in the kernel's per-pixel word.  A frame beyond any
 * of them is flagged and repeated in multi-launch form, which has no such bounds.  Runs without a GPU. */
void rd_polyline_limits(int32_t out[4]);

/* test tap: the region stage alone (oclrect.c:325-342: region merge, region sizes, absorption of small regions, region boundaries and their components - rd_k_rect.hip,
 * rd_k_label.hip) on planes of the caller, so that its launch budgets, fixed capacities and fallback paths can be tested on crafted planes.  Runs once on `device`, on a
 * stream, planes and scratch of its own, then frees everything.  All planes are iw * ih ints.
 * stage 0, from the merge's inputs: pix = the quantised colour, mask = the merge mask (zero / non-zero), edge = the strong-edge plane (> 0: strong edge).  Runs exactly what
 *   a frame runs.  launches = an even budget in 2..128 for the merge, or 0 for the frame path's behaviour: 20 launches, and where the last of them still changed something
 *   the ladder of 32, 64, 128 - the frame path's own function.  region0_in / rsize_in are not read.
 * stage 1, from the absorption's inputs: region0_in = a label per pixel, each in [0, iw * ih), rsize_in = the size of every label (indexed by label, each in [0, 2^26)).
 *   Runs the absorption and the boundary stages.  pix / mask / edge / launches are not read.
 * Either stage repeats the absorption on its slow path where the fast path's status word asks for it, as the frame path does; force_slow != 0 does so regardless (as
 * RD_ABSORB_FORCE_SLOW does for a detector).
 * Out: region0_out (labels after the merge), rsize_out (junction counts + region sizes, by label), region_out (labels after the absorption), boundarysrc_out (boundary
 * marks), boundary_out (components of the marks), and info: [0..127] the merge's flag per launch of the final budget (!= 0: that launch changed something), [128] the
 * budget that was final (0 in stage 1), [129] 1 = the merge settled within it, 0 = the planes are what that many launches made of them, [130..133] the absorption's
 * status words of the fast path ([0] != 0: it gave up, [1] undecided pixels the tile kernel left, [2] sweeps and [3] steps of the tail), [134] the slow path ran, [135] its
 * launches of the rounds, [136..143] 0.
 * Returns 0, or -1 without touching the device for a null pointer among the planes the stage reads or writes, a frame rd_detector_create refuses (under 16 x 16, or 2^25
 * pixels and more), an odd or out-of-range `launches`, a stage other than 0 / 1, a label outside [0, iw * ih) or a size outside [0, 2^26).  Needs a GPU (fatal without
 * one); not called by the frame path. */
#define RD_REGION_INFO_INTS 144
int rd_region_planes_device(int device, int stage, int iw, int ih, const int32_t *pix, const int32_t *mask, const int32_t *edge, int launches,
                            const int32_t *region0_in, const int32_t *rsize_in, int force_slow,
                            int32_t *region0_out, int32_t *rsize_out, int32_t *region_out, int32_t *boundarysrc_out, int32_t *boundary_out, int32_t info[RD_REGION_INFO_INTS]);
/* the constants of the region stage that crafted planes are built from: out[0] the largest budget of launches a frame's merge starts with, [1..4] the budgets of the ladder
 * a frame still changing in its last launch climbs (0: no further step), [5] the most launches of the merge (the definition's limit), [6] undecided pixels the absorption's
 * single-block tail holds, [7] its sweeps at most, [8] its threads (pixels per thread: the smallest of [19..25] that covers the count), [9] halo of the absorption's tile
 * kernel, [10] small-region cells a tile can own, [11] x [12] the merge's tile, [13] x [14] the absorption's, [15] the absorption threshold (regions up to this size are
 * absorbed), [16] launches after which the slow absorption calls a missing fixed point an internal error and [17] records of undecided pixels the fast path has room for,
 * both for an iw x ih frame (0 if iw or ih is not positive), [18] rounds of the tile kernel, [19..25] the tail's pixels-per-thread variants, [26] bits of a region size in
 * the tail's words, [27..31] 0.  Runs without a GPU. */
void rd_region_limits(int iw, int ih, int32_t out[32]);

/* test tap: the vote stage (oclrect.cl:427-464, reduceLS: rd_k_rect.hip's k_reduce_clean, k_reduce_claim, k_reduce_box) and the sampling kernel that reads its table and
 * assembles a frame's hand-over block, on masks and boundary planes of the caller, through the frame path's own calls.  nsteps >= 1 steps of 1 <= nb <= 8 frames of iw x ih
 * pixels; frame z keeps its scratch, list, table, claim and touched-slot list from step to step, as a detector's slot does from frame to frame (tables set up once).  Per step
 * ONE set of launches for its nb frames: the polyline stage and its id plane (as rd_polyline_planes_device, lists of 16 bytes per pixel), the votes, the samples.
 * In: masks, boundaries = nsteps * nb planes of iw * ih ints, step-major (mask: zero / non-zero; boundary: a component id per pixel, any int, <= 0 = none); ring_nonzero,
 *   minerror, size_thre, form = nsteps values each (a launch shares them among its frames); clean = how a step undoes the tables' entries of the step before: 0 = the votes'
 *   own first launch, 1 = the boundary labelling (run on a scratch region plane of the tap's), whose last kernel does it on the frame path, and votes that are told so;
 *   max_records, pack_records = what the frame path passes the sampling kernel (records that get probes; records that travel in the block); rflags = nb * 256 ints, frame z's
 *   region flags and status words as the block copies them; guard = the word every int of the probes buffer and the block holds before a step; probes_ints, pack_ints = ints
 *   of a frame's probes buffer and block.
 * Out, per step and frame (step-major): ids_out iw * ih ints, lslist_out 16 * iw * ih bytes, ctr_out 64 ints (rd_polyline_planes_device), table_out nentry * 5 ints (nentry =
 *   iw * ih * 4 / 5), tlist_out nentry + 1 ints ([0] = count), claim_out nentry ints, probes_out probes_ints ints, pack_out pack_ints ints.
 * Returns 0, or -1 without touching the device for a null pointer, a frame rd_detector_create refuses, nsteps < 1, nb outside 1..8, a form or clean other than 0 / 1, a negative
 * size_thre, max_records < 5 (the block's leading 60 words are written by the first of max_records * 15 threads; one record of margin), pack_records < 1 (the header record travels always),
 * probes_ints < max_records * 90 or pack_ints < 64 + pack_records * 104.  Fatal in a -DRD_BOUNDARY_FLATTEN=0 tuning build (the plane holds ids, not links).  Needs a GPU
 * (fatal without one); not called by the frame path. */
int rd_votes_planes_device(int device, int iw, int ih, int nsteps, int nb, const int32_t *masks, const int32_t *boundaries,
                           const int32_t *ring_nonzero, const float *minerror, const int32_t *size_thre, const int32_t *form, int clean,
                           int max_records, int pack_records, const int32_t *rflags, int32_t guard, int probes_ints, int pack_ints,
                           int32_t *ids_out, void *lslist_out, int32_t *ctr_out, int32_t *table_out, int32_t *tlist_out, int32_t *claim_out, int32_t *probes_out, int32_t *pack_out);
/* the constants the vote stage's crafted cases are placed by: out[0] distinct boundary ids of a 7 x 7 window one pass of the vote kernels holds, [1] slots of a block's claim
 * hash and [2] the slots a claim tries before it goes straight to memory, [3] and [4] the same for a block's box hash, [5] threads per block and [6] blocks per frame of the
 * claim and the box kernel, [7] frames per launch at most, [8] the word of an unclaimed `claim` entry, then the hand-over block's layout in ints: [9] where the region flags
 * start and [10] how many there are, [11] where the absorption's status words start and [12] how many, [13] where those status words lie in rflags, [14] where the records
 * start, [15] ints per record, [16] ints of probes per record; [17..23] 0.  Runs without a GPU. */
#define RD_VOTES_LIMITS_INTS 24
void rd_votes_limits(int32_t out[RD_VOTES_LIMITS_INTS]);

/* ---- rectified patches: what is INSIDE a quad, as an upright image of fixed size (rd_k_rectify.hip, rd_rectify.hip).
 * The reference only draws outlines (rect.cpp, vidrect.cpp), so the arithmetic is defined here - exactly, so that an independent restatement (tests/rectify.py,
 * numpy float64) reproduces every byte.
 *
 * A quad is four corners (x0,y0) (x1,y1) (x2,y2) (x3,y3) as doubles in the coordinates of rect_t::c2 (pixel centres at integers), in PATCH ORDER: they are where
 * the corners (0,0) (1,0) (1,1) (0,1) of the unit square land.  A patch is pw x ph pixels of 3 bytes B, G, R, rows back to back; patch k of a job starts at
 * out + k * pw * ph * 3.
 *
 * Coefficients - once per quad, on the host, IEEE double, exactly these operations, no contraction (rd_rectify_coefficients):
 *   dx1 = x1-x2;  dx2 = x3-x2;  sx = ((x0-x1)+x2)-x3                      (dy1, dy2, sy the same from y)
 *   den = dx1*dy2 - dx2*dy1
 *   g = (sx*dy2 - dx2*sy)/den;   h = (dx1*sy - sx*dy1)/den
 *   a = (x1-x0) + g*x1;  b = (x3-x0) + h*x3;  c = x0
 *   d = (y1-y0) + g*y1;  e = (y3-y0) + h*y3;  f = y0                      coef[8] = { a, b, c, d, e, f, g, h }
 * (the projective map of the unit square onto the quad: x = (a*s + b*t + c) / (g*s + h*t + 1), y = (d*s + e*t + f) / (g*s + h*t + 1)).
 * A quad is VALID (status 1) when its eight values are finite and the four cross products, i = 0..3 with indices mod 4,
 *   (x[i+1]-x[i]) * (y[i+2]-y[i+1]) - (y[i+1]-y[i]) * (x[i+2]-x[i+1])
 * are all > 0 or all < 0 - strictly convex, either orientation - and the eight coefficients came out finite (they do unless the corners are
 * so large that a product overflows).  An invalid quad has status 0, coefficients 0 and an all-zero patch.
 *
 * Patch pixel (i, j) - on the device, in double, uncontracted, in this order:
 *   s = (i + 0.5) / pw;  t = (j + 0.5) / ph;  w = (g*s + h*t) + 1.0
 *   x = ((a*s + b*t) + c) / w;   y = ((d*s + e*t) + f) / w
 *   xi = floor(x * 256.0) clamped to [0, (iw-1)*256] and then taken as an integer      (yi the same with ih; the clamp is made in double: anything not above 0 - a NaN too - gives 0)
 *   x0 = xi >> 8;  fx = xi & 255;  x1 = min(x0+1, iw-1)                                (y0, fy, y1 the same)
 * and per channel, in int32, with p(x, y) the channel's byte of source pixel (x, y):
 *   top = p(x0,y0)*(256-fx) + p(x1,y0)*fx;   bot = p(x0,y1)*(256-fx) + p(x1,y1)*fx
 *   out = (top*(256-fy) + bot*fy + 32768) >> 16
 * p is the (B, G, R) of the source pixel under the conversion contract above: for NV12 and I420 each of the four taps is converted first (BT.601 fixed point,
 * 2x2 nearest chroma) and blended afterwards, so the patch from a frame in any format equals, bit for bit, the patch from the BGR frame the contract gives for it.
 * Why double: two correctly rounded divisions per pixel cost nothing next to the detector ("Rectified patches"), and they are what lets numpy agree in every bit. */

/* the quads of n rectangles as the detector returns them (rects: n records of 176 bytes, WITHOUT the header element: pass ret + 1) in patch order: for each,
 * c2[0], c2[3], c2[2], c2[1] -> quads_out[8 * k ..].  The detector's corners run counter-clockwise on screen (y down); in this order s runs clockwise from
 * c2[0] and patches are not mirrored.  Another start corner or a mirror image: permute the corners. */
void rd_rect_quads(const void *rects, int n, double *quads_out);
/* |c3[0]-c3[1]| / |c3[1]-c3[2]| of one rectangle, each length sqrt((dx*dx + dy*dy) + dz*dz): the aspect ratio of the estimated pose (the reference's own test
 * of it: oclrect.c:641).  c3[i] is the pose of corner c2[i], and with rd_rect_quads' order a patch's rows (t) run along c2[0] -> c2[1] and its columns (s) along
 * c2[0] -> c2[3], which is parallel to c3[1] - c3[2]: the value is HEIGHT / WIDTH of a patch made with rd_rect_quads (ph = pw * aspect keeps the pose's shape;
 * 1 / aspect is width / height).  It is the ESTIMATED shape in space, not the ratio of the quad's edges on screen: under perspective, and for rectangles whose
 * pose fit is poor, the two can differ widely. */
double rd_rect_aspect(const void *rect);
/* host only: coefficients and status of one quad as above - what a job uploads */
void rd_rectify_coefficients(const double quad[8], double coef[8], int *status);

/* A rectifier makes patches of pw x ph pixels, up to max_quads per job, up to njobs jobs in flight, on one stream of its own.  NULL on bad arguments
 * (pw, ph, max_quads or njobs < 1, pw or ph > 16384, no such device). */
typedef struct rd_rectifier rd_rectifier;
rd_rectifier *rd_rectifier_create(int device, int pw, int ph, int max_quads, int njobs);
void rd_rectifier_destroy(rd_rectifier *r);      /* waits for the jobs in flight */

/* One job: n patches from one iw x ih frame in pixel format `format` (RD_PIX_*; planes / pitches as for rd_detector_enqueue_planes).
 * on_device: where the frame lies - RD_FRAME_HOST (copied into the rectifier's own device buffer, which grows on demand, before the call returns),
 *   RD_FRAME_DEVICE (read in place) or RD_FRAME_HOST_PINNED (the copy engine reads it in place; memory that is not pinned is fatal); device and pinned frames
 *   stay valid and unchanged until the job's rd_rectifier_wait returned.
 * out / out_kind: where the n patches go - RD_FRAME_DEVICE (the kernel writes there) or RD_FRAME_HOST_PINNED (the copy engine does); valid until the job's wait.
 * Returns the job's sequence number, or -1 with nothing enqueued for an argument error: an unknown format, on_device or out_kind, iw or ih < 1 or > 65536, a NULL plane the
 * format uses, a pitch smaller than its plane's row, NV12 / I420 with an odd iw or ih, n < 0, n > max_quads, n > 0 with quads or out NULL, `out` not memory of the
 * kind out_kind names (pageable memory; only the kind of the memory at `out` is asked about - that it holds n * pw * ph * 3 bytes is the caller's contract).  A call with njobs jobs already in flight is fatal, as it is for the detector. */
long rd_rectifier_enqueue(rd_rectifier *r, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const double *quads, int n, void *out, int out_kind);
/* the oldest job: blocks until its patches are where it was told to put them, returns its n and writes the n status bytes (1 valid, 0 invalid: zero patch) to
 * status_out when that is not NULL.  -1: no job in flight. */
int rd_rectifier_wait(rd_rectifier *r, uint8_t *status_out);
/* One job from the frame of the most recently polled slot of d (either kind of detector): its planes, pitches and format as they were handed over.  A host frame
 * is rectified from the copy the detector uploaded - no second transfer - which lasts until the next enqueue on d: wait for the job first.  Device and pinned
 * frames: the caller keeps the buffer until the job's wait.  A frame that came in at scale 2 (rd_detector_enqueue_scaled): quads in detector coordinates, patches from
 * the full-size source, see there.  Returns as rd_rectifier_enqueue; -1 also when nothing has been polled yet or d and r are on different devices. */
long rd_detector_rectify_polled(rd_detector *d, rd_rectifier *r, const double *quads, int n, void *out, int out_kind);

/* -- model-ready tensors: the same patches in the element type, layout and channel order the next model takes, normalised and - for a quad much larger than its
 * patch - box-filtered, from the one launch (rd_k_tensor.hip, rd_rectify.hip, rd_tensor_host.c).  Exact like everything above: tests/tensor.py restates it in numpy.
 *
 * C = 1 for RD_TENSOR_GRAY, otherwise 3.  oversample m is 1, 2 or 4.  scale and bias are indexed by OUTPUT channel - under RD_TENSOR_RGB channel 0 is R -, GRAY uses
 * index 0, and RD_TENSOR_U8 ignores them.  A spec is LEGAL for pw x ph when every enum is one of the values below, pw >= 1, ph >= 1, pw*m <= 16384, ph*m <= 16384
 * and, for the float dtypes, scale[c] and bias[c] of the C channels in use are finite.
 *
 * Element (k, c, j, i) of a job - quad k, channel c, row j, column i:
 *   1. P is the patch of quad k at (pw*m) x (ph*m) pixels, byte for byte the contract above: the coefficients, s = (i+0.5)/(pw*m), t = (j+0.5)/(ph*m), the clamps,
 *      the 8.8 blend, each tap of a YUV frame converted first.
 *   2. the channel value of a patch pixel, in int32: BGR: byte c of P;  RGB: byte 2-c of P;  GRAY: (29*B + 150*G + 77*R + 128) >> 8 ("matched quads", step 2).
 *   3. S = the sum of the channel values over the m x m patch pixels (i*m .. i*m+m-1, j*m .. j*m+m-1): an integer, 0 .. 255*m*m.
 *   4. U8:  (S + m*m/2) >> log2(m*m), one byte.
 *      the float dtypes, in binary32, uncontracted, in this order:  v = (float)S * (1.0f/(m*m))  (exact: m*m is a power of two and S < 2^12);
 *        v = v * scale[c], rounded to nearest even;  v = v + bias[c], rounded to nearest even.
 *      F32 stores v.  F16 stores v converted to binary16, round to nearest even, overflow to infinity, subnormals kept.
 *      BF16 stores the upper 16 bits of u + 0x7FFF + ((u >> 16) & 1), u the 32 bits of v: round to nearest even, overflow to infinity.  The formula would turn some
 *      NaNs into infinities, but a NaN cannot arise from a legal spec: v >= 0 is finite, so the product is finite or infinite, and the sum of that and a finite
 *      bias is never NaN.
 * The element's offset from the job's `out`, in ELEMENTS:  NHWC: ((k*ph + j)*pw + i)*C + c;   NCHW: ((k*C + c)*ph + j)*pw + i.   `out` is aligned to the element's
 * size; the job's n * rd_rectifier_patch_bytes(r) bytes are written and nothing else.  An invalid quad (status 0) gives all-zero BYTES in every dtype - not bias -
 * from the same launch.  The spec { RD_TENSOR_U8, RD_TENSOR_NHWC, RD_TENSOR_BGR, 1 } is, by this definition, exactly the patch of rd_rectifier_create;
 * { U8, either layout, GRAY, m } at pw = ph = G is the matcher's signature + 128. */
#define RD_TENSOR_U8 0    /* dtype */
#define RD_TENSOR_F16 1
#define RD_TENSOR_BF16 2
#define RD_TENSOR_F32 3
#define RD_TENSOR_NHWC 0  /* layout */
#define RD_TENSOR_NCHW 1
#define RD_TENSOR_BGR 0   /* channels */
#define RD_TENSOR_RGB 1
#define RD_TENSOR_GRAY 2
typedef struct { int32_t dtype, layout, channels, oversample; float scale[3], bias[3]; } rd_tensor_spec;   /* 40 bytes */
/* host only, no GPU needed (rd_tensor_host.c).  1 when the spec is legal for pw x ph, else 0 (a NULL spec too) */
int rd_tensor_spec_ok(const rd_tensor_spec *spec, int pw, int ph);
/* the bytes of one quad's tensor: pw * ph * C * the element's size; 0 for a spec that is not legal for pw x ph */
size_t rd_tensor_bytes(const rd_tensor_spec *spec, int pw, int ph);
/* step 4 for one element of channel c from its box sum S: writes the element's 1, 2 or 4 bytes to out and returns that count; 0, and nothing written, for a NULL
 * argument, an unknown dtype, channel kind or oversample, or c outside 0 .. C-1 */
int rd_tensor_element(const rd_tensor_spec *spec, int c, int32_t S, void *out);
/* out[0..3] <- the legal dtypes, layouts and channel kinds as bit sets (bit v: value v is legal), and the legal oversamplings ORed together (1 | 2 | 4) */
void rd_tensor_limits(int32_t out[4]);
/* A rectifier whose jobs write tensors.  NULL for the bad arguments of rd_rectifier_create, a NULL spec or a spec that is not legal for pw x ph.  The handle is an
 * ordinary rd_rectifier: rd_rectifier_enqueue, rd_rectifier_wait, rd_rectifier_destroy and rd_detector_rectify_polled work on it with every pixel format, frame
 * kind and output kind, and `out` holds n * rd_rectifier_patch_bytes(r) bytes. */
rd_rectifier *rd_rectifier_create_tensor(int device, int pw, int ph, int max_quads, int njobs, const rd_tensor_spec *spec);
/* the bytes of one quad's output: pw * ph * 3 for a rectifier made by rd_rectifier_create, rd_tensor_bytes, rd_scan_bytes, rd_grade_bytes, rd_code_bytes or rd_blob_bytes of the spec for the others; 0 for NULL */
size_t rd_rectifier_patch_bytes(const rd_rectifier *r);

/* -- scanned pages: the quad as a clean page - the patch's luma divided by its local mean (shading correction) or compared with it (adaptive threshold), as bytes
 * or as one bit per pixel in packed rows, the raster of a PBM "P4" file (rd_k_scan.hip, rd_rectify.hip, rd_scan_host.c).  Two launches per job: the G plane by the
 * tensor kernel, then the window sums and the decision.  Exact, in integers, like everything above: tests/scan.py restates it in numpy.
 *
 * A spec is LEGAL for pw x ph when mode is one of the three below, 1 <= radius <= 63, 0 <= k <= 255, 0 <= d <= 255, 1 <= white <= 255, oversample m is 1, 2 or 4,
 * invert is 0 or 1, reserved is 0, pw >= 1, ph >= 1, pw*m <= 16384 and ph*m <= 16384.
 *
 * Pixel (i, j) of quad k:
 *   1. G0(i, j) is, byte for byte, the element of the tensor spec { RD_TENSOR_U8, RD_TENSOR_NHWC, RD_TENSOR_GRAY, m } for the same quad, frame, pw and ph (steps 1-4
 *      of "model-ready tensors").  G = invert ? 255 - G0 : G0.
 *   2. The window of (i, j) is the intersection of the patch with the square of side 2*radius + 1 centred on (i, j):
 *      [max(0, i-r), min(pw-1, i+r)] x [max(0, j-r), min(ph-1, j+r)].  N is its pixel count, T the sum of G over it.  T <= 255 * 127^2, and everything below fits
 *      int32: the largest term is 256 * 127^2 * 510 = 2 105 802 240.
 *   3. ink = 256*N*(G + d) < (256 - k)*T: the pixel is darker than (1 - k/256) of its neighbourhood's mean by more than d (Bradley's ratio with OpenCV's constant).
 *      A constant patch has no ink for any k, d; an all-zero window has no ink.
 *   4. F = (T == 0) ? white : min(255, (G*N*white + (T >> 1)) / T), an integer division: a pixel equal to its neighbourhood's mean comes out as `white`.
 *   5. Output, quad k at out + k * rd_rectifier_patch_bytes(r):  RD_SCAN_FLAT: F at j*pw + i.  RD_SCAN_BILEVEL: ink ? 0 : 255 at the same place.
 *      RD_SCAN_BITS: row j starts at byte j * ((pw + 7) >> 3), pixel i is bit 7 - (i & 7) of byte i >> 3, 1 = ink, and the pad bits of a row's last byte are 0.
 *      An invalid quad (status 0) gives all-zero bytes in every mode.  The job's n * rd_rectifier_patch_bytes(r) bytes are written and nothing else. */
#define RD_SCAN_FLAT 0          /* shading-corrected gray, one byte per pixel */
#define RD_SCAN_BILEVEL 1       /* one byte per pixel: 0 = ink, 255 = paper */
#define RD_SCAN_BITS 2          /* one BIT per pixel, 1 = ink, most significant bit first, rows padded to whole bytes with 0 bits: the raster of a PBM "P4" file */
typedef struct { int32_t mode, radius, k, d, white, oversample, invert, reserved; } rd_scan_spec;   /* 32 bytes */
/* host only, no GPU needed (rd_scan_host.c).  1 when the spec is legal for pw x ph, else 0 (a NULL spec too) */
int rd_scan_spec_ok(const rd_scan_spec *spec, int pw, int ph);
/* the bytes of one quad's page: pw * ph, or ((pw + 7) >> 3) * ph for RD_SCAN_BITS; 0 for a spec that is not legal for pw x ph */
size_t rd_scan_bytes(const rd_scan_spec *spec, int pw, int ph);
/* step 1's inversion and steps 3 and 4 for one pixel: G0 in 0 .. 255, N in 1 .. 127^2, T - the sum of the INVERTED G over the window - in 0 .. 255*N.  Writes 1 or 0
 * to *ink and F to *flat (either may be NULL and is then skipped) and returns 1; returns 0 and writes nothing for a NULL spec, a spec whose k, d, white or invert
 * is not legal, or G0, N or T outside these ranges */
int rd_scan_pixel(const rd_scan_spec *spec, int G0, int N, int T, uint8_t *ink, uint8_t *flat);
/* out[0] <- the legal modes as a bit set (bit v: value v is legal), out[1] <- the legal oversamplings ORed together (1 | 2 | 4), out[2] <- the largest radius,
 * out[3], out[4] <- the width and the height, in output pixels, of the tile a block of the kernel makes, out[5..7] <- 0 */
void rd_scan_limits(int32_t out[8]);
/* A rectifier whose jobs write scanned pages.  NULL for the bad arguments of rd_rectifier_create, a NULL spec or a spec that is not legal for pw x ph.  The handle is
 * an ordinary rd_rectifier: rd_rectifier_enqueue, rd_rectifier_wait, rd_rectifier_destroy and rd_detector_rectify_polled work on it with every pixel format, frame
 * kind and output kind, and `out` holds n * rd_rectifier_patch_bytes(r) bytes. */
rd_rectifier *rd_rectifier_create_scan(int device, int pw, int ph, int max_quads, int njobs, const rd_scan_spec *spec);

/* -- graded quads: not what is in the quad but whether this frame's view of it is worth keeping - per cell of a cells x cells grid over the patch how many pixels
 * there are, how many are black, how many blown out, how many lie on an edge, and the sums from which mean, contrast and the variance of the Laplacian (sharpness)
 * follow; optionally the patch's histogram (rd_k_grade.hip, rd_rectify.hip, rd_grade_host.c).  A few dozen bytes per quad instead of pw * ph.  Two launches per job:
 * the G plane by the tensor kernel, then the statistics.  Exact, in integers, like everything above: tests/grade.py restates it in numpy.
 *
 * A spec is LEGAL for pw x ph when cells is 1, 2, 4 or 8, 0 <= dark <= 255, 0 <= bright <= 255, 0 <= edge <= 1020, oversample m is 1, 2 or 4, hist is 0 or 1, both
 * reserved words are 0, pw >= cells and ph >= cells (no cell is empty), pw*m <= 16384 and ph*m <= 16384.
 *
 * Quad k:
 *   1. G(i, j) is, byte for byte, the element of the tensor spec { RD_TENSOR_U8, RD_TENSOR_NHWC, RD_TENSOR_GRAY, m } for the same quad, frame, pw and ph (steps 1-4
 *      of "model-ready tensors"; step 1 of "scanned pages" without the inversion).
 *   2. L(i, j) = G(i-1, j) + G(i+1, j) + G(i, j-1) + G(i, j+1) - 4*G(i, j), every neighbour index clamped to the patch ([0, pw-1], [0, ph-1]: the border is
 *      replicated).  |L| <= 4 * 255 = 1020.
 *   3. Pixel (i, j) belongs to cell (cx, cy) = ((i*cells) / pw, (j*cells) / ph), integer divisions; the cell's record is number cy*cells + cx.  A pixel's L counts
 *      in the pixel's own cell, whatever cells its neighbours lie in.
 *   4. The record of a cell, over the pixels of the cell:  n = their count;  lo = how many have G <= dark;  hi = how many have G >= bright;  ne = how many have
 *      |L| >= edge;  sg = the sum of G, sgg of G*G, sl of L, sll of L*L.
 *      At 16384 x 16384 and cells = 1:  n <= 2^28,  sg <= 2^28 * 255,  sgg <= 2^28 * 65 025,  |sl| <= 2^28 * 1020,  sll <= 2^28 * 1 040 400 = 279 280 248 422 400 < 2^63:
 *      int64 holds every sum, int32 every count.  int32 would not hold the sums: a 258 x 258 patch of 255s has sgg = 66 564 * 65 025 = 4 328 324 100 > 2^32, and a
 *      64 x 128 checkerboard of 0 and 255 has sll > 2^32.
 *   5. Output, quad k at out + k * rd_rectifier_patch_bytes(r): cells*cells records of 48 bytes (rd_grade_cell), record number c at byte 48*c; with hist set, 256
 *      uint32_t follow them: word v counts the pixels of the whole patch with G == v.  patch_bytes = 48*cells*cells + 1024*hist.
 *      An invalid quad (status 0) gives all-zero bytes.  The job's n * rd_rectifier_patch_bytes(r) bytes are written and nothing else.  The bytes are complete when
 *      rd_rectifier_wait returns: they are zeroed and added to on the job's stream, and no intermediate value is visible in them after the wait.  `out` must be
 *      8-byte aligned for a grade rectifier: rd_rectifier_enqueue (and rd_detector_rectify_polled) return -1 with nothing enqueued when it is not. */
typedef struct { int32_t cells, dark, bright, edge, oversample, hist, reserved[2]; } rd_grade_spec;   /* 32 bytes */
typedef struct { int32_t n, lo, hi, ne; int64_t sg, sgg, sl, sll; } rd_grade_cell;                   /* 48 bytes */
/* host only, no GPU needed (rd_grade_host.c).  1 when the spec is legal for pw x ph, else 0 (a NULL spec too) */
int rd_grade_spec_ok(const rd_grade_spec *spec, int pw, int ph);
/* the bytes of one quad's output: 48 * cells * cells + 1024 * hist; 0 for a spec that is not legal for pw x ph */
size_t rd_grade_bytes(const rd_grade_spec *spec, int pw, int ph);
/* step 3: the number of the record that pixel (i, j) counts in; -1 for a spec that is not legal for pw x ph or a pixel outside the patch */
int rd_grade_cell_of(const rd_grade_spec *spec, int pw, int ph, int i, int j);
/* out[0] <- the legal cells ORed together (1 | 2 | 4 | 8), out[1] <- the legal oversamplings ORed together (1 | 2 | 4), out[2] <- the largest edge (1020),
 * out[3], out[4] <- the width and the height, in pixels, of the tile a block of the kernel reduces, out[5] <- sizeof(rd_grade_cell) (48), out[6] <- the bytes of
 * the histogram (1024), out[7] <- 0 */
void rd_grade_limits(int32_t out[8]);
/* the variance of the Laplacian over a cell, the usual measure of focus: 0 for n == 0 (or a NULL cell), else, in double, uncontracted, in exactly this order,
 * ((double)sll - ((double)sl * (double)sl) / (double)n) / (double)n.  Records may be added field by field first: the sharpness of a whole patch is that of the sum */
double rd_grade_sharpness(const rd_grade_cell *cell);
/* the smallest v in 0 .. 255 with cum(v) * den >= num * total, cum(v) = hist[0] + .. + hist[v], total = cum(255), in 64-bit integers: the value below which num / den
 * of the pixels lie (1, 100: the 1st percentile; 99, 100: the 99th - a `white` for a scan spec from the page itself).  -1 for a NULL hist, den < 1, den > 1 048 576
 * (the products then fit 64 bits: total < 2^40), num < 0, num > den or an empty histogram */
int rd_grade_percentile(const uint32_t hist[256], int num, int den);
/* A rectifier whose jobs write graded quads.  NULL for the bad arguments of rd_rectifier_create, a NULL spec or a spec that is not legal for pw x ph.  The handle is
 * an ordinary rd_rectifier: rd_rectifier_enqueue, rd_rectifier_wait, rd_rectifier_destroy and rd_detector_rectify_polled work on it with every pixel format, frame
 * kind and output kind, and `out` holds n * rd_rectifier_patch_bytes(r) bytes, 8-byte aligned. */
rd_rectifier *rd_rectifier_create_grade(int device, int pw, int ph, int max_quads, int njobs, const rd_grade_spec *spec);

/* -- decoded quads: what the quad SAYS - a square grid code (an ArUco / AprilTag-style fiducial, a board marker, the data cells of a label: a ring of `border`
 * cells round an n x n payload of dark and light cells) read per cell from the patch, and its id in a dictionary by Hamming distance over the four rotations
 * (rd_k_code.hip, rd_rectify.hip, rd_code_host.c).  48 bytes per quad instead of pw * ph.  Two launches per job: the G plane by the tensor kernel, then one block
 * per quad for everything else.  Exact, in integers, like everything above: tests/code.py restates it in numpy and Python integers.
 *
 * With C = n + 2*border a spec is LEGAL for pw x ph when 3 <= n <= 8, border is 1 or 2, 0 <= inset <= 3, polarity is 0 or 1, oversample m is 1, 2 or 4,
 * 0 <= contrast <= 255, 0 <= max_border <= C*C - n*n, 0 <= max_hamming <= n*n, pw <= 1024 and ph <= 1024, and pw >= C and ph >= C when inset is 0, pw >= 4*C and
 * ph >= 4*C when it is not.  Under these bounds no cell is without a counted pixel (step 2; below 4*C with an inset cells do come out empty, first at C + 1), every
 * cell sum fits int32 and 256*sg fits uint32 (step 3).
 *
 * A dictionary is ndict <= 4096 codes of 64 bits, bit r*n + c the payload cell in row r and column c, the bits at and above n*n zero; it is uploaded once, when the
 * rectifier is made.  ndict = 0 reads raw bits only.
 *
 * Quad k:
 *   1. G(i, j) is, byte for byte, the element of the tensor spec { RD_TENSOR_U8, RD_TENSOR_NHWC, RD_TENSOR_GRAY, m } for the same quad, frame, pw and ph (step 1 of
 *      "graded quads").
 *   2. The cell of a pixel, by the pixel's centre: cx = ((2*i + 1)*C) / (2*pw), fx = ((2*i + 1)*C) % (2*pw); cy, fy the same from j and ph.  The pixel COUNTS when
 *      inset*pw <= 4*fx <= (8 - inset)*pw and inset*ph <= 4*fy <= (8 - inset)*ph: the outer inset/8 of a cell on every side is ignored - that is where the
 *      neighbours bleed in.  The cell's number is cy*C + cx.
 *   3. Per cell over its counted pixels: cnt their count, sg the sum of G, M = (256*sg) / cnt, an integer division: the mean in 8.8 fixed point.  With an inset of 0
 *      a cell is at most ceil(pw / C) x ceil(ph / C) <= 205 x 205 pixels: 256*sg <= 42 025 * 255 * 256 = 2 743 392 000 needs uint32 - the kernel and the host
 *      divide unsigned; M <= 65 280.
 *   4. lo = min M and hi = max M over the C*C cells.  light = 2*M > lo + hi;  v = light XOR polarity;  margin = the minimum over the cells of |2*M - (lo + hi)|.
 *      A constant patch has every light = 0 (and margin 0).
 *   5. border_errors = how many cells of the outer `border` rings (row or column < border or >= C - border) have v = 1.  The payload cell in row r and column c of
 *      the inner n x n (cell (border + c, border + r)) gives bit r*n + c of `bits`.
 *   6. A rotation by one quarter turn clockwise: rot1(P)[r][c] = P[n-1-c][r], that is bit r*n + c of rot1(P) is bit (n-1-c)*n + r of P; rot_k applies rot1 k times.
 *   7. dist(id, k) = popcount(rot_k(bits) XOR dict[id]).  (hamming, id, rot) = the lexicographic minimum of (dist, id, k) over 0 <= id < ndict, 0 <= k < 4: the lowest
 *      id wins a tie, then the lowest k.  second = the minimum dist over every (id', k) with id' != id, 65 when ndict < 2.  With ndict = 0: id = -1, rot = 0,
 *      hamming = second = 65.
 *   8. ok = (hi - lo >= 256*contrast) && border_errors <= max_border && (ndict == 0 || hamming <= max_hamming).
 *   9. Output: one rd_code of 48 bytes, quad k's at out + 48*k, reserved = 0.  An invalid quad (status 0) gives 48 zero bytes.  Exactly n * 48 bytes are written.
 *      `out` must be 8-byte aligned: rd_rectifier_enqueue (and rd_detector_rectify_polled) return -1 with nothing enqueued when it is not. */
typedef struct { int32_t n, border, inset, polarity, oversample, contrast, max_border, max_hamming; } rd_code_spec;                /* 32 bytes */
typedef struct { uint64_t bits; int32_t id, rot, hamming, second, border_errors, lo, hi, margin, ok, reserved; } rd_code;         /* 48 bytes */
/* host only, no GPU needed (rd_code_host.c).  1 when the spec is legal for pw x ph, else 0 (a NULL spec too) */
int rd_code_spec_ok(const rd_code_spec *spec, int pw, int ph);
/* the bytes of one quad's output: 48; 0 for a spec that is not legal for pw x ph */
size_t rd_code_bytes(const rd_code_spec *spec, int pw, int ph);
/* step 2: the number of the cell pixel (i, j) lies in, and whether it counts (1 or 0) to *counted (may be NULL); -1, *counted untouched, for a spec that is not
 * legal for pw x ph or a pixel outside the patch */
int rd_code_cell_of(const rd_code_spec *spec, int pw, int ph, int i, int j, int *counted);
/* step 6: rot_k(bits) of an n x n payload, k taken modulo 4 (negative k: counter-clockwise); 0 for n outside 3 .. 8; bits at and above n*n are dropped */
uint64_t rd_code_rotate(uint64_t bits, int n, int k);
/* out[0] <- the smallest n (3), out[1] <- the largest (8), out[2] <- the largest border (2), out[3] <- the largest inset (3), out[4] <- the legal oversamplings ORed
 * together (1 | 2 | 4), out[5] <- the largest pw and ph (1024), out[6] <- the largest ndict (4096), out[7] <- sizeof(rd_code) (48) */
void rd_code_limits(int32_t out[8]);
/* what max_hamming a dictionary bears: the smallest popcount(rot_k(dict[a]) XOR dict[b]) over a < b and k = 0 .. 3, and popcount(rot_k(dict[a]) XOR dict[a]) over
 * k = 1 .. 3 (a code that looks like itself turned has distance 0: its rot cannot be told).  65 for ndict = 0; -1 for n outside 3 .. 8, ndict outside 0 .. 4096, a
 * NULL dict with ndict > 0, or an entry with bits at or above n*n */
int rd_code_distance(const uint64_t *dict, int ndict, int n);
/* a deterministic greedy dictionary.  State s = seed; a candidate: s += 0x9E3779B97F4A7C15; z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 * z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31 (splitmix64, everything modulo 2^64); cand = z & (2^(n*n) - 1).  It is accepted, and appended to out,
 * when rd_code_distance of the accepted codes with it stays >= min_dist.  Stops after `count` accepted codes or `tries` candidates; returns how many it accepted.
 * -1 for n outside 3 .. 8, count outside 0 .. 4096, min_dist < 0, tries < 0 or a NULL out with count > 0 */
int rd_code_dictionary(int n, int count, int min_dist, uint64_t seed, int tries, uint64_t *out);
/* the gray image of a code, (C*cell_px)^2 bytes, rows of C*cell_px: the ring has v = 0, payload cell (r, c) has v = bit r*n + c, a cell is light when
 * v XOR polarity, and light cells are 255, dark cells 0.  Only n, border and polarity of the spec are read.  Returns the bytes written; 0, nothing written, for a NULL
 * argument, n, border or polarity out of range, cell_px outside 1 .. 64 or bits at or above n*n */
size_t rd_code_render(const rd_code_spec *spec, uint64_t bits, int cell_px, uint8_t *out);
/* the corners from which a patch shows the code upright: out corner c = quad corner (c + 4 - rot) % 4 (4 x (x, y), patch order; rot taken modulo 4).  The quad to
 * hand to a rectifier, the compositor or a pose consumer once rd_code::rot is known; reading it again gives rot 0 and the same id.  out may not alias quad */
void rd_code_upright(const double quad[8], int rot, double out[8]);
/* A rectifier whose jobs write decoded quads.  NULL for the bad arguments of rd_rectifier_create, a NULL spec or a spec that is not legal for pw x ph, ndict outside
 * 0 .. 4096, a NULL dict with ndict > 0, or an entry with bits at or above n*n.  The dictionary is copied.  The handle is an ordinary rd_rectifier:
 * rd_rectifier_enqueue, rd_rectifier_wait, rd_rectifier_destroy and rd_detector_rectify_polled work on it with every pixel format, frame kind and output kind,
 * rd_rectifier_patch_bytes is 48, and `out` holds n * 48 bytes, 8-byte aligned. */
rd_rectifier *rd_rectifier_create_code(int device, int pw, int ph, int max_quads, int njobs, const rd_code_spec *spec, const uint64_t *dict, int ndict);

/* -- page components: the quad's page as OBJECTS - the connected ink regions of the bilevel page, each reduced to a record (bounding box, area, first pixel, coordinate
 * sums), a head of counts per quad, and optionally the page with everything outside the area filter removed (despeckle) - what OCR and layout engines, form readers
 * and dot counters take next, and what a G4 / JBIG2 encoder wants gone (rd_k_blob.hip, rd_rectify.hip, rd_blob_host.c).  Exact, in integers, like everything above:
 * tests/blobs.py restates it in numpy and Python integers, rd_blob_page_host states it in C.
 *
 * A spec is LEGAL for pw x ph when 0 <= radius <= 63, 0 <= k <= 255, 0 <= d <= 255 and d == 0 when radius == 0, oversample m is 1, 2 or 4, invert is 0 or 1,
 * connectivity is 4 or 8, 1 <= min_area <= 1<<22, max_area == 0 (no upper bound) or min_area <= max_area <= 1<<22, 1 <= max_blobs <= 4096, page is 0 or 1, both
 * reserved words are 0, pw >= 1, ph >= 1, pw*m <= 16384, ph*m <= 16384 and pw*ph <= 1<<22.
 *
 * Quad k:
 *   1. Ink.  G is, byte for byte, step 1 of "scanned pages": the { RD_TENSOR_U8, RD_TENSOR_NHWC, RD_TENSOR_GRAY, m } tensor, inverted where `invert` says so.
 *      radius >= 1: ink is step 3 of "scanned pages" with the same radius, k, d.  radius == 0: a fixed level, ink = G <= k (the inside of a large dark area - a filled
 *      check box, a dot, an LED - is never ink under an adaptive threshold).
 *   2. Components.  A component is a maximal set of ink pixels connected through 4 or 8 neighbours inside the patch.  Its `first` is the smallest j*pw + i among its
 *      pixels, `area` their count, x0, y0, x1, y1 their inclusive bounding box, sx and sy the sums of i and of j over them (int64: the sums of a full 2048 x 2048 page,
 *      4 292 870 144, do not fit int32).
 *   3. Kept.  A component is KEPT when min_area <= area and (max_area == 0 or area <= max_area).
 *   4. Head (rd_blob_head, 32 bytes): ink = ink pixels; all = components before the filter; found = kept components; written = min(found, max_blobs); ink_kept =
 *      pixels of kept components; largest = the largest area before the filter, 0 without ink; flags = bit 0 (RD_BLOB_OVERFLOW) set when found > max_blobs; reserved = 0.
 *   5. Records.  max_blobs records (rd_blob, 40 bytes) follow the head: the first `written` are the kept components in ascending `first`; on overflow the ones with
 *      the smallest `first` survive - a rule, not an accident of scheduling; the rest are zero bytes.
 *   6. Page.  With page == 1 the cleaned page follows at offset 32 + 40*max_blobs: the kept components only - all of them, whatever max_blobs - in the RD_SCAN_BITS
 *      layout with pad bits 0, padded with zero bytes to a multiple of 8 (records stay 8-aligned from quad to quad).
 *   7. Sizes.  rd_blob_bytes = 32 + 40*max_blobs, plus ((((pw + 7) >> 3)*ph + 7) & ~7) with a page.  An invalid quad (status 0) gives all-zero bytes.  The job's
 *      n * rd_rectifier_patch_bytes(r) bytes are written and nothing else; they are complete when rd_rectifier_wait returns.  `out` must be 8-byte aligned:
 *      rd_rectifier_enqueue (and rd_detector_rectify_polled) return -1 with nothing enqueued when it is not.
 *
 * Launches per job: the G plane by the tensor kernel; the ink bits by the scan kernel in RD_SCAN_BITS mode (radius >= 1: no new arithmetic, a difference from a scan
 * job is impossible by construction) or by a threshold kernel (radius == 0); then the component stage: labels per tile in LDS, tiles joined across their borders,
 * areas per run, kept roots ranked in raster order, records and the cleaned page per run (rd_k_blob.hip's head comment).  Scratch: 8 bytes per page pixel per quad
 * of a job slot, allocated on first use. */
#define RD_BLOB_OVERFLOW 1      /* rd_blob_head::flags: more kept components than max_blobs */
typedef struct { int32_t radius, k, d, oversample, invert, connectivity, min_area, max_area, max_blobs, page, reserved[2]; } rd_blob_spec;   /* 48 bytes */
typedef struct { int32_t ink, all, found, written, ink_kept, largest, flags, reserved; } rd_blob_head;                                    /* 32 bytes */
typedef struct { int32_t x0, y0, x1, y1, area, first; int64_t sx, sy; } rd_blob;                                                          /* 40 bytes */
/* host only, no GPU needed (rd_blob_host.c).  1 when the spec is legal for pw x ph, else 0 (a NULL spec too) */
int rd_blob_spec_ok(const rd_blob_spec *spec, int pw, int ph);
/* the bytes of one quad's output (step 7); 0 for a spec that is not legal for pw x ph */
size_t rd_blob_bytes(const rd_blob_spec *spec, int pw, int ph);
/* out[0] <- the legal connectivities as a bit set (bit v: value v is legal), out[1] <- the legal oversamplings ORed together (1 | 2 | 4), out[2] <- the largest
 * radius, out[3] <- the largest max_blobs, out[4] <- the largest pw*ph, out[5], out[6] <- the width and the height, in pixels, of the tile a block of the tile kernel
 * labels, out[7] <- 0 */
void rd_blob_limits(int32_t out[8]);
/* steps 2-7 for one page: `bits` is a pw x ph page in the RD_SCAN_BITS layout (its pad bits are ignored), `out` gets rd_blob_bytes(spec, pw, ph) bytes (8-byte
 * aligned).  Only connectivity, min_area, max_area, max_blobs and page of the spec decide the result.  Returns 1; returns 0 and writes nothing for a NULL argument,
 * a spec that is not legal for pw x ph, an `out` that is not 8-byte aligned or when its work space cannot be allocated.  The contract's statement in C, and the host
 * baseline of tools/bench_blobs.py; nothing in the frame path calls it. */
int rd_blob_page_host(const uint8_t *bits, int pw, int ph, const rd_blob_spec *spec, void *out);
/* A rectifier whose jobs write page components.  NULL for the bad arguments of rd_rectifier_create, a NULL spec, a spec that is not legal for pw x ph, or
 * (size_t)max_quads*pw*ph > 1<<27 (the scratch of a slot).  The handle is an ordinary rd_rectifier: rd_rectifier_enqueue, rd_rectifier_wait, rd_rectifier_destroy
 * and rd_detector_rectify_polled work on it with every pixel format, frame kind and output kind, and `out` holds n * rd_rectifier_patch_bytes(r) bytes, 8-byte
 * aligned. */
rd_rectifier *rd_rectifier_create_blobs(int device, int pw, int ph, int max_quads, int njobs, const rd_blob_spec *spec);
/* test tap: the component stage alone (steps 2-7) on n pages of the caller, through the job path's own launch function (rdk::blobs), so that crafted masks reach it
 * unchanged.  `bits`: n pages of pw x ph in the RD_SCAN_BITS layout back to back, ((pw + 7) >> 3)*ph bytes each, pad bits ignored; `out`: n * rd_blob_bytes bytes.
 * Both are host pointers.  Runs once on `device`, on a stream and scratch of its own, then frees everything.  info[0] = the path that ran (0: tiles and borders -
 * the only one), [1] = kernel launches, [2] = memsets on the stream, [3], [4] = tiles in x and in y, [5] = 1 when the border kernel ran, [6], [7] = 0.
 * Returns 0, or -1 without touching the device for a NULL pointer, n outside 1 .. 65535, a spec that is not legal for pw x ph (only the fields of steps 2-7 are
 * read beyond that) or (size_t)n*pw*ph > 1<<27.  Needs a GPU (fatal without one); not called by the frame path. */
int rd_blobs_pages_device(int device, const uint8_t *bits, int pw, int ph, int n, const rd_blob_spec *spec, void *out, int32_t info[8]);

/* ---- annotated frames: rectangles' outlines and line segments drawn INTO a frame on the device (rd_k_annotate.hip, rd_annotate.hip) - the picture vidrect.cpp /
 * rect.cpp (showRect) and vidpoly.cpp / poly.cpp make with OpenCV's line() on the host, for frames that never leave HBM.  OpenCV's round brush is not restated; the
 * arithmetic is defined here, in integers, exactly, so that an independent restatement (tests/annotate.py) reproduces every byte.
 *
 * A primitive is one line segment (x0, y0) - (x1, y1) in frame pixels, pixel centres at integers as in rect_t::c2, with a colour and a thickness.  Every coordinate lies
 * in [-1048576, 1048575] and thickness is >= 1: a job with any other primitive is refused (-1).
 *
 * Coverage - independent of the order of the endpoints:
 *   dx = x1 - x0, dy = y1 - y0.  The primitive is x-major when |dx| >= |dy|, else y-major; u is the major coordinate of a pixel, v the minor one.
 *   Swap the endpoints so that the major coordinate does not decrease: (ua, va) -> (ub, vb), D = ub - ua >= 0.
 *   The brush extends along the minor axis only: lo = (t - 1) / 2, hi = t / 2 (integer division) for thickness t.
 *   For every u in [ua, ub]:  V(u) = va + floor((2 (u - ua) (vb - va) + D) / (2 D))   (floor division; V = va when D = 0)
 *   and the primitive covers the pixels (u, V(u) + o), o in [-lo, hi].  No end caps.  Pixels outside the frame are not written; nothing clips or alters the line.
 * The same test per pixel without a division (what the kernel and rd_annot_covers evaluate, rd_annot_cover.h; int64, |e| < 2^45 at every legal coordinate):
 *   covered  <=>  ua <= u <= ub  and  -2 D hi <= e < 2 D (lo + 1)   with  e = 2 (u - ua) (vb - va) + D - 2 D (v - va);     D = 0:  -lo <= v - va <= hi.
 *
 * Painter's order: where several primitives of a job cover a pixel, the one with the HIGHEST index wins, as successive line() calls would have it.  The result is a
 * function of the job alone, never of scheduling.
 *
 * Formats: all six RD_PIX_*.  Packed formats: the pixel's B, G, R bytes, in the format's order, are written; A never is, not even by RD_ANNOT_CLEAR.  NV12 and I420 (even
 * iw and ih, as elsewhere): each primitive's colour is converted once, on the host (rd_annot_yuv; int32, arithmetic shifts)
 *   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16;   U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128;   V = ((112 R - 94 G - 18 B + 128) >> 8) + 128
 * luma is written per covered pixel, and a chroma sample takes the U, V of the highest-indexed primitive that covers ANY of its four luma pixels; it stays as it is
 * when none does.
 * RD_ANNOT_CLEAR (flags bit 0; vidpoly.cpp's and poly.cpp's picture): before drawing, every pixel's colour becomes black - B = G = R = 0, or Y = 16 and U = V = 128.
 * A job IN PLACE writes covered pixels only (with RD_ANNOT_CLEAR: every pixel's colour bytes).  A job into ANOTHER frame leaves the source as it is and writes every
 * pixel of the destination once: it is the in-place job on a copy of the source's pixels (all bytes of a pixel, A included, travel with it).  Pitch padding and
 * bytes behind the planes are never written, in either frame. */
typedef struct { int32_t x0, y0, x1, y1; uint8_t b, g, r, thickness; } rd_annot_prim;   /* 20 bytes */
#define RD_ANNOT_CLEAR 1

/* host helpers; none needs a GPU */
/* 1 when primitive p covers pixel (x, y), else 0 (p must be legal): the shared coverage test (test tap) */
int rd_annot_covers(const rd_annot_prim *p, int x, int y);
/* 1 when the kernel's binning puts p into a tile that is the pixel rectangle [x0, x1] x [y0, y1] (inclusive): it may say 1 for a tile p only passes close to, never
 * 0 for a tile with a covered pixel (test tap) */
int rd_annot_touches(const rd_annot_prim *p, int x0, int y0, int x1, int y1);
void rd_annot_yuv(uint8_t b, uint8_t g, uint8_t r, uint8_t yuv[3]);
/* out[0], out[1]: width and height of the tile of pixels one block draws (both even), out[2]: primitives the blocks test per pass = records of a tile's list held in
 * LDS at a time (lists of any length are drawn in as many passes: no capacity other than max_prims exists), out[3] = 0 */
void rd_annot_limits(int32_t out[4]);
/* Six primitives per rectangle (rects: n records of 176 bytes WITHOUT the header element: pass ret + 1) in showRect's order (vidrect.cpp:33-45): the edges
 * c2[i] -> c2[(i+1)%4], i = 0..3, then c2[0] - c2[2], then c2[1] - c2[3].  Coordinates: (int) of the double - truncation toward zero, as cvPoint does; scale 2 (the
 * rectangles of a frame that came in through rd_detector_enqueue_scaled, drawn into its full-size source): (int)(v * 2.0 + 0.5) and every thickness doubled
 * (capped at 255).  style: b, g, r, thickness for status 0, 1, 2, 3; edges take the style's thickness, diagonals 1.  NULL: vidrect.cpp's table as the bytes that land
 * in its BGR Mat - status 0 (0,255,0,1), 1 (0,200,255,2), 2 (255,0,0,1), 3 (0,0,255,2).  A rectangle with a corner that is not finite or that lands outside the
 * legal range, or with a status above 3, is skipped as a whole.  Returns the primitives written (out holds 6 n); 0 for a scale other than 1 or 2. */
int rd_annot_rects(const void *rects, int n, int scale, const uint8_t style[16], rd_annot_prim *out);
/* The segments of a linesegment_t list WITH its header (what rd_detector_poll_segments returns), thickness 1 (2 at scale 2), coordinates as rd_annot_rects.
 * RD_ANNOT_SEG_ALL: records 1..n in white (vidpoly.cpp:200-207).  RD_ANNOT_SEG_CHAINS (poly.cpp:142-153): from every head - polyid != 0 and leftPtr <= 0 - along
 * rightPtr while it stays in 1..n, at most n steps (a cycle ends there), colours (b,g,r) (255,255,100) / (100,100,255) alternating by position in the chain.  Records
 * out of range are skipped (their position still counts).  Writes at most max primitives; returns how many there are, which may exceed max. */
#define RD_ANNOT_SEG_ALL 0
#define RD_ANNOT_SEG_CHAINS 1
int rd_annot_segments(const void *lslist, int mode, int scale, rd_annot_prim *out, int max);

/* An annotator draws up to max_prims primitives per job, up to njobs jobs in flight, on one stream of its own.  NULL on bad arguments (max_prims < 1 or > 1048576,
 * njobs < 1 or > 1024, no such device). */
typedef struct rd_annotator rd_annotator;
rd_annotator *rd_annotator_create(int device, int max_prims, int njobs);
void rd_annotator_destroy(rd_annotator *a);      /* waits for the jobs in flight */
/* One job: n primitives into one iw x ih frame in pixel format `format` (planes / pitches as for rd_detector_enqueue_planes).  The primitives are copied before the
 * call returns.
 * out_planes == NULL: in place - on_device must be RD_FRAME_DEVICE; the frame is the caller's until the job's wait.
 * otherwise: the source is not modified and the annotated frame goes to out_planes / out_pitches, memory of kind out_kind: RD_FRAME_DEVICE (the kernel writes there) or
 *   RD_FRAME_HOST_PINNED (through a device buffer of the annotator, which grows on demand; the copy engine writes the rows).  The source is RD_FRAME_HOST (copied into
 *   the annotator's own device buffer before the call returns), RD_FRAME_DEVICE (read in place) or RD_FRAME_HOST_PINNED (the copy engine reads it in place; memory that
 *   is not pinned is fatal); device and pinned sources, and the output, stay valid until the job's wait returned.  Source and destination must not overlap.
 * Returns the job's sequence number, or -1 with nothing enqueued for an argument error: an unknown format, on_device or out_kind, flag bits other than RD_ANNOT_CLEAR,
 * iw or ih < 1 or > 65536, a NULL plane the format uses (source or output), a pitch smaller than its plane's row (source or output), NV12 / I420 with an odd iw or ih,
 * n < 0, n > max_prims, n > 0 with prims NULL, a primitive out of range (a coordinate, or thickness 0), in place with a frame that is not on the device, an output
 * plane that is not memory of the kind out_kind names.  A call with njobs jobs already in flight is fatal, as it is for the rectifier.
 * An in-place job on a frame that a rectifier job reads must follow that job's rd_rectifier_wait: the two objects have streams of their own. */
long rd_annotator_enqueue(rd_annotator *a, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                          const rd_annot_prim *prims, int n, int flags, void *const out_planes[3], const int out_pitches[3], int out_kind);
/* the oldest job: blocks until the frame is where it was told to go, returns its n.  -1: no job in flight. */
int rd_annotator_wait(rd_annotator *a);
/* One job on the frame of the most recently polled slot of d (either kind of detector): its planes, pitches and format as they were handed over, at the SOURCE's
 * size - a frame that came in at scale 2 (rd_detector_enqueue_scaled) is annotated at 2 iw x 2 ih, with primitives in source coordinates (rd_annot_rects and
 * rd_annot_segments with scale 2 make them from the detector's lists).  A device frame: in place (out_planes NULL) or into out_planes.  A host or pinned frame: the
 * source is the copy the detector uploaded, which must stay what the rectifier reads, so out_planes is required (-1 without); that copy lasts until the next enqueue
 * on d: wait for the job first.  Returns as rd_annotator_enqueue; -1 also when nothing has been polled yet or d and a are on different devices. */
long rd_detector_annotate_polled(rd_detector *d, rd_annotator *a, const rd_annot_prim *prims, int n, int flags,
                                 void *const out_planes[3], const int out_pitches[3], int out_kind);

/* ---- composited quads: a colour or an image written INTO every quad of a frame on the device (rd_k_composite.hip, rd_composite.hip, rd_comp_host.c) - redaction
 * (fill every detected screen) and replacement (put an image into every detected rectangle) for frames that never leave HBM.  The exact inverse of the rectifier:
 * the same quad convention, the same patch layout, the same eight coefficients.  The arithmetic is defined here, exactly, so that an independent restatement
 * (tests/composite.py, numpy float64) reproduces every byte.
 *
 * An item is a quad with either a colour or the number of a patch.  `quad`: four corners in PATCH ORDER in the coordinates of rect_t::c2, exactly as for the
 * rectifier - where the corners (0,0) (1,0) (1,1) (0,1) of the unit square land; rd_rect_quads makes them.  patch >= 0: paste patch number `patch` of the job's patch
 * array - npatches images of pw x ph pixels of 3 bytes B, G, R, rows back to back, patch k at k * pw * ph * 3: the layout rd_rectifier writes.  patch == -1: fill with
 * (b, g, r).  Any other negative value, or patch >= npatches, is an argument error.
 *
 * Per item - once, on the host, IEEE double, exactly these operations, no contraction (rd_composite_coefficients):
 *   a .. h and validity from rd_rectify_coefficients, unchanged (finite corners, strictly convex in either orientation, finite coefficients).
 *   The adjugate of the map's matrix:
 *     A = e - f*h;   B = c*h - b;   C = b*f - c*e
 *     D = f*g - d;   E = a - c*g;   F = c*d - a*f
 *     G = d*h - e*g; H = b*g - a*h; I = a*e - b*d                          inv[9] = { A, B, C, D, E, F, G, H, I }
 *   An item is also INVALID when one of the nine is not finite.  An invalid item has status 0 and writes nothing.
 *   The pixel box, in double:  fl = floor(min x_i) - 1.0;  ce = ceil(max x_i) + 1.0.  The box is EMPTY when ce < 0.0 or fl > iw-1 (compared in double); otherwise
 *     bx0 = (int)max(fl, 0.0);  bx1 = (int)min(ce, (double)(iw-1))         (by0, by1 the same from y and ih)
 *   An item with an empty box is valid and covers nothing.  box[4] = { bx0, by0, bx1, by1 }; an empty box, and the box of an invalid item, is { 0, 0, -1, -1 }.
 *
 * Per frame pixel (X, Y) - on the device, in double, uncontracted, in this order:
 *   wn = (G*X + H*Y) + I
 *   s  = ((A*X + B*Y) + C) / wn;   t = ((D*X + E*Y) + F) / wn
 *   covered  <=>  bx0 <= X <= bx1  and  by0 <= Y <= by1  and  s >= 0.0  and  s < 1.0  and  t >= 0.0  and  t < 1.0
 * A NaN or an infinity fails the comparisons: such a pixel is not covered.  s and t are rounded values: two quads that share an edge may BOTH claim a pixel centre that
 * lies on it, or NEITHER may - away from edges (further than the rounding of the map, far below 1e-6 pixel for quads of a frame's size) coverage is the inside test.
 *   Fill:  the pixel's colour is (b, g, r).
 *   Paste: u = s*pw - 0.5;  v = t*ph - 0.5;  ui = floor(u * 256.0) clamped in double to [0, (pw-1)*256] - anything not above 0, a NaN too, gives 0 - then an integer
 *          (vi the same with ph);  x0 = ui >> 8;  fx = ui & 255;  x1 = min(x0+1, pw-1)  (y0, fy, y1 the same) and per channel, in int32, with p(x, y) the channel's
 *          byte of patch pixel (x, y):  top = p(x0,y0)*(256-fx) + p(x1,y0)*fx;  bot = p(x0,y1)*(256-fx) + p(x1,y1)*fx;  out = (top*(256-fy) + bot*fy + 32768) >> 16
 *          - the rectifier's blend over the patch's bytes.
 * With the axis-aligned quad (x0-0.5, y0-0.5) (x0+N-0.5, y0-0.5) (x0+N-0.5, y0+N-0.5) (x0-0.5, y0+N-0.5) and pw = ph = N a power of two, coverage is exactly the N x N
 * pixels, u and v are the integer column and row, and rectify followed by composite reproduces the frame's bytes.
 *
 * Painter's order: where several items of a job cover a pixel, the one with the HIGHEST index wins.  The result is a function of the job alone, never of scheduling.
 *
 * Formats: all six RD_PIX_*.  Packed formats: the pixel's B, G, R bytes, in the format's order, are written; A never is.  NV12 and I420 (even iw and ih, as
 * elsewhere): the luma of a covered pixel is Y of its final colour (rd_annot_yuv).  A chroma sample is written when n >= 1 of its four luma pixels are covered: with
 * S_c the sum of channel c over those n pixels' final colours, M_c = (S_c + n/2) / n in integer division, and U, V are those of rd_annot_yuv(M_b, M_g, M_r).  A
 * sample none of whose four pixels is covered stays as it is.
 *
 * IN PLACE only covered pixels are written, and no pixel is ever read: there is no alpha and no read-modify-write.  A job into ANOTHER frame is the in-place job on
 * a copy of the source's pixels, with the annotator's rules: the source is unchanged, every pixel of the destination is written (all bytes of a pixel, A included,
 * travel with it), pitch padding and bytes behind the planes are never written.
 *
 * Out of scope: alpha blending; anti-aliased edges; patches in formats other than BGR; a mosaic of the frame's own pixels.  For the last the supported route is to
 * rectify the quad into a small patch, 8 x 8 for example, and paste it back: a redaction that never leaves the device (examples/rdredact.c, "mosaic"). */
typedef struct { double quad[8]; int32_t patch; uint8_t b, g, r, pad; } rd_comp_item;   /* 72 bytes */

/* host taps; none needs a GPU */
/* the adjugate, the pixel box and the status of one quad in an iw x ih frame as above - what a job uploads per item.  Invalid: zeros, the empty box, status 0. */
void rd_composite_coefficients(const double quad[8], int iw, int ih, double inv[9], int32_t box[4], int *status);
/* 1 when the quad covers pixel (x, y) of an iw x ih frame, else 0: the per-pixel test on the host, in the same operations.  st != NULL: st[0] = s, st[1] = t when
 * the quad is valid and its box holds the pixel, else zeros. */
int rd_composite_covers(const double quad[8], int iw, int ih, int x, int y, double st[2]);
/* The tiles an in-place job of these items launches: the union of the valid items' boxes in tiles of rd_comp_limits' width and height (tile (tx, ty) starts at pixel
 * (tx * width, ty * height)), each once, in raster order.  Writes up to max pairs tx, ty to tiles_xy (may be NULL with max 0) and returns how many there are, which may
 * exceed max; -1 for iw or ih < 1 or > 65536, n < 0 or n > 0 with items NULL.  Only the quads are looked at. */
int rd_composite_tiles(const rd_comp_item *items, int n, int iw, int ih, int32_t *tiles_xy, int max);
/* out[0], out[1]: width and height of the tile of pixels one wave composites (both even), out[2]: items whose boxes a wave tests per pass (any number of items up to
 * max_items may overlap one tile: no other capacity exists), out[3] = 0 */
void rd_comp_limits(int32_t out[4]);

/* A compositor writes up to max_items items per job, pasting patches of pw x ph pixels, up to njobs jobs in flight, on one stream of its own.  NULL on bad arguments
 * (pw, ph, max_items or njobs < 1, pw or ph > 16384, max_items > 1048576, njobs > 1024, no such device). */
typedef struct rd_compositor rd_compositor;
rd_compositor *rd_compositor_create(int device, int pw, int ph, int max_items, int njobs);
void rd_compositor_destroy(rd_compositor *c);      /* waits for the jobs in flight */
/* One job: n items into one iw x ih frame in pixel format `format` (planes / pitches as for rd_detector_enqueue_planes).  The items are validated and turned into
 * device records before the call returns; the caller may reuse the array.
 * out_planes == NULL: in place - on_device must be RD_FRAME_DEVICE; the frame is the caller's until the job's wait.
 * otherwise: the source - RD_FRAME_HOST (copied before the call returns), RD_FRAME_DEVICE or RD_FRAME_HOST_PINNED (memory that is not pinned is fatal) - is not
 *   modified and the frame goes to out_planes / out_pitches, memory of kind out_kind: RD_FRAME_DEVICE or RD_FRAME_HOST_PINNED (through a device buffer of the
 *   compositor, which grows on demand).  Device and pinned sources, and the output, stay valid until the job's wait returned.  Source and destination must not overlap.
 * patches / npatches / patches_kind: the patch array the items' `patch` numbers refer to - RD_FRAME_DEVICE (read in place until the job's wait), RD_FRAME_HOST_PINNED
 *   (the copy engine brings it into a device buffer of the compositor, which grows on demand; valid until the job's wait; memory that is not pinned is fatal) or
 *   RD_FRAME_HOST (copied before the call returns).  A job of fills alone may pass NULL and 0.
 * Returns the job's sequence number, or -1 with nothing enqueued for an argument error: the annotator's - an unknown format, on_device or out_kind, iw or ih < 1 or
 * > 65536, a NULL plane the format uses (source or output), a pitch smaller than its plane's row (source or output), NV12 / I420 with an odd iw or ih, n < 0,
 * n > max_items, n > 0 with items NULL, in place with a frame that is not on the device, an output plane that is not memory of the kind out_kind names - and an item
 * whose `patch` is below -1 or not below npatches, npatches < 0, and, while some item pastes, patches NULL, an unknown patches_kind or patches of kind RD_FRAME_DEVICE
 * that are not device memory.  A call with njobs jobs already in flight is fatal, as it is for the annotator.
 * An in-place job on a frame that a rectifier job reads must follow that job's rd_rectifier_wait: the two objects have streams of their own. */
long rd_compositor_enqueue(rd_compositor *c, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                           const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                           void *const out_planes[3], const int out_pitches[3], int out_kind);
/* the oldest job: blocks until the frame is where it was told to go, returns its n and writes the n status bytes (1 valid, 0 invalid: nothing written) to status_out
 * when that is not NULL.  -1: no job in flight. */
int rd_compositor_wait(rd_compositor *c, uint8_t *status_out);
/* One job on the frame of the most recently polled slot of d (either kind of detector): its planes, pitches and format as they were handed over, at the SOURCE's size.
 * A frame that came in at scale 2 (rd_detector_enqueue_scaled): the items' quads in DETECTOR coordinates - what rd_rect_quads gives for that frame's rectangles - each
 * corner mapped on the host, in double, X = x * 2.0 + 0.5, Y = y * 2.0 + 0.5, as rd_detector_rectify_polled maps them; the job runs on the full-size source.  A device
 * frame: in place (out_planes NULL) or into out_planes.  A host or pinned frame: the source is the copy the detector uploaded, which must stay what the rectifier
 * reads, so out_planes is required (-1 without); that copy lasts until the next enqueue on d: wait for the job first.  Returns as rd_compositor_enqueue; -1 also when
 * nothing has been polled yet or d and c are on different devices. */
long rd_detector_composite_polled(rd_detector *d, rd_compositor *c, const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                                  void *const out_planes[3], const int out_pitches[3], int out_kind);

/* ---- matched quads: WHICH known thing is inside a quad - a screen, a card, a poster, a sign, a fiducial - decided on the device (rd_k_match.hip, rd_match.hip,
 * rd_match_host.c).  A matcher holds a library of templates; a job returns, per quad, the best template, its orientation, its score and the runner-up: a few dozen
 * bytes instead of a patch.  Everything is defined in integers plus a handful of correctly rounded double operations, so that an independent restatement
 * (tests/match.py, numpy int64 / float64) reproduces every value.
 *
 * Signature of a quad - parameters: a grid G in {8, 16, 32, 64} and an oversampling m in {1, 2, 4}:
 *   1. the rectifier's patch of the quad at pw = ph = G*m - "rectified patches" above, byte for byte: coefficients, s = (i+0.5)/pw, the 8.8 blend, the conversion
 *      of every tap of an NV12 / I420 frame, the clamps;
 *   2. per patch pixel, in int32:  grey = (29*B + 150*G + 77*R + 128) >> 8                                     (0 .. 255)
 *   3. per cell (i, j) of the G x G grid, over the m x m patch pixels (i*m .. i*m+m-1, j*m .. j*m+m-1):
 *        cell = (sum of the greys + m*m/2) >> log2(m*m);   a = cell - 128 as int8                              (-128 .. 127)
 *   4. the signature is the D = G*G values a in row-major order, rows along t: value number j*G + i is cell (i, j);
 *   5. alongside, in integers:  sa = sum of a,  saa = sum of a*a.
 * An invalid quad (the rectifier's status 0) has no signature.
 *
 * Library.  A matcher holds up to max_templates templates, numbered from 0 in the order they were added.  A template is the signature of a quad in an image the
 * caller hands over (rd_matcher_add); a NULL quad is the whole image: corners (-0.5,-0.5) (iw-0.5,-0.5) (iw-0.5,ih-0.5) (-0.5,ih-0.5).  Template k occupies the
 * library's columns 4k .. 4k+3: column 4k+r is the template's signature S turned r quarter turns as a pure permutation of its cells,
 *   rot(S)[j][i] = S[G-1-i][j]     (row j, column i)     applied r times
 * - the picture turned clockwise on screen (y down) by r quarter turns; nothing is resampled.  A quad whose best column is 4k+r therefore shows template k with
 * the template's FIRST corner (its patch corner (0,0)) at the quad's corner number r, and the template's corners follow in the quad's own order: the quad's corners
 * r, r+1, r+2, r+3 (mod 4) are the template's 0, 1, 2, 3 - the start corner a caller permutes to for an upright patch.  Every column keeps sb = sum of b and
 * sbb = sum of b*b (the same for the four columns of a template).  A template with D*sbb - sb*sb == 0 (a flat image) or from an invalid quad is refused.
 *
 * Scores - for quad q (signature a) and column c (signature b), all exact:
 *   dot = sum of a_i * b_i                       int32   (|dot| <= 4096 * 2^14 = 2^26)
 *   num = D*dot - sa*sb                          int64   (magnitude below 2^39)
 *   va  = D*saa - sa*sa;   vb = D*sbb - sb*sb    int64   (0 <= va, vb < 2^39: every conversion to double below is exact)
 * Selection - on the device, in double, uncontracted, in this order:
 *   key_c = ((double)num * fabs((double)num)) / (double)vb_c
 * The best column is the one with the greatest key, the LOWEST column among equal keys.  The runner-up is the best column, by the same rule, among the columns
 * whose template differs from the best's (the best's other three rotations never are the runner-up); there is none when the library holds one template.
 * Score - on the HOST, in plain C from the integers the device returned (rd_match_score, rd_match_host.c; the device never takes a square root):
 *   score = (double)num / sqrt((double)va * (double)vb)                 - the correlation coefficient of the two signatures, in [-1, 1] up to rounding.
 *
 * The record of a quad:
 *   status  0: an invalid quad;  1: matched;  2: a flat signature (va == 0: no correlation exists);  3: an empty library.  Tested in the order 0, 3, 2.
 *   tmpl, rot, dot      the best column 4*tmpl + rot and its dot
 *   tmpl2, rot2, dot2   the runner-up's; -1, 0, 0 when there is none
 *   sa, saa             the quad's sums
 *   score, score2       as above from the best's and the runner-up's integers; score2 = 0.0 when there is no runner-up
 * With a status other than 1 every other field is zero. */
typedef struct { int32_t status, tmpl, rot, dot, tmpl2, rot2, dot2, sa; int64_t saa; double score, score2; } rd_match;   /* 56 bytes */
#define RD_MATCH_DOTS 1               /* flags of a job: keep the whole dot matrix for rd_matcher_wait */
#define RD_MATCH_MAX_TEMPLATES 4096
#define RD_MATCH_MAX_QUADS 1024

/* host helpers; none needs a GPU */
/* Completes a record the device made: score from (dot, sa, saa) and the best column's sb, sbb, score2 from (dot2, sa, saa) and sb2, sbb2 (ignored when tmpl2 < 0:
 * score2 = 0.0) for a matcher of grid `grid` (D = grid * grid).  A record whose status is not 1 gets every other field zeroed. */
void rd_match_score(rd_match *rec, int grid, int32_t sb, int64_t sbb, int32_t sb2, int64_t sbb2);
/* out[0]: the legal grids ORed together (8 | 16 | 32 | 64), out[1]: the legal oversamplings ORed together (1 | 2 | 4), out[2] = RD_MATCH_MAX_TEMPLATES,
 * out[3] = RD_MATCH_MAX_QUADS */
void rd_match_limits(int32_t out[4]);

/* A matcher scores up to max_quads quads per job against up to max_templates templates, up to njobs jobs in flight, on one stream of its own.  NULL on bad arguments
 * (a grid or an oversampling other than the above, max_templates < 1 or > RD_MATCH_MAX_TEMPLATES, max_quads < 1 or > RD_MATCH_MAX_QUADS, njobs < 1 or > 1024, no such
 * device).  Device memory: the library (4 * max_templates * D bytes) and the dot matrix (max_quads x 4 * max_templates int32, both rounded up to 16). */
typedef struct rd_matcher rd_matcher;
rd_matcher *rd_matcher_create(int device, int grid, int oversample, int max_templates, int max_quads, int njobs);
void rd_matcher_destroy(rd_matcher *m);      /* waits for the jobs in flight */
/* Adds a template: the signature of `quad` (8 doubles, patch order; NULL: the whole image) in an iw x ih image in pixel format `format` (planes / pitches / on_device
 * as for rd_rectifier_enqueue; a pinned image that is not pinned memory is fatal).  Waits for the matcher's stream - jobs already enqueued were scored against the
 * library as it was - and returns when the template is in the library: the image may be reused.  Returns the template's number; -1 for an argument error (the frame
 * checks of rd_rectifier_enqueue; a full library); -2 for a flat template or an invalid quad.  Nothing changes on -1 and -2. */
int rd_matcher_add(rd_matcher *m, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device, const double *quad);
int rd_matcher_templates(rd_matcher *m);      /* how many templates the library holds */
/* test tap: the D bytes of column 4 * tmpl + rot to `out` and its sb, sbb to sums[0], sums[1] (either may be NULL); waits for the matcher's stream.  0, or -1 when
 * there is no such column. */
int rd_matcher_signature(rd_matcher *m, int tmpl, int rot, int8_t *out, int32_t sums[2]);
/* One job: the records of n quads (8 doubles each, patch order) of one iw x ih frame in pixel format `format`.  Frame kinds, their lifetimes and the argument checks
 * are rd_rectifier_enqueue's: RD_FRAME_HOST (copied before the call returns), RD_FRAME_DEVICE (read in place until the job's wait), RD_FRAME_HOST_PINNED (memory that
 * is not pinned is fatal).  The caller hands over no output buffer: results travel to pinned memory of the job and rd_matcher_wait copies them out.  flags:
 * RD_MATCH_DOTS keeps the job's dot matrix too (its pinned block is allocated with the first job that asks).  The job is scored against the library as it is NOW:
 * T = rd_matcher_templates at this call.  n == 0 is a legal job.  Returns the job's sequence number, or -1 with nothing enqueued for an argument error: the frame's
 * (as the rectifier), flag bits other than RD_MATCH_DOTS, n < 0, n > max_quads, n > 0 with quads NULL.  A call with njobs jobs already in flight is fatal. */
long rd_matcher_enqueue(rd_matcher *m, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device, const double *quads, int n, int flags);
/* the oldest job: blocks until it is done, completes its n records (rd_match_score) into `out` (may be NULL) and returns n.  dots_out: NULL, or - for a job enqueued
 * with RD_MATCH_DOTS - space for n x 4T int32, T the job's: dots_out[q * 4T + c] = dot of quad q and column c (a row of zeros for an invalid quad).  -1: no job in
 * flight. */
int rd_matcher_wait(rd_matcher *m, rd_match *out, int32_t *dots_out);
/* One job from the frame of the most recently polled slot of d (either kind of detector), as rd_detector_rectify_polled: no second transfer of a host frame; quads
 * of a frame that came in at scale 2 in DETECTOR coordinates, each corner mapped X = x * 2.0 + 0.5, Y = y * 2.0 + 0.5, the signature taken from the full-size source.
 * Returns as rd_matcher_enqueue; -1 also when nothing has been polled yet or d and m are on different devices. */
long rd_detector_match_polled(rd_detector *d, rd_matcher *m, const double *quads, int n, int flags);

/* ---- remapped frames: the frame an IDEAL pinhole camera would have seen, made on the device from the frame a real lens gave (rd_k_remap.hip, rd_remap.hip,
 * rd_remap_host.c) - lens undistortion ahead of the detector, whose polyline stage, quad vote and pose fit all assume straight lines and a pinhole.  The reference
 * leaves this to OpenCV on the host (cv::remap), so the arithmetic is defined here - exactly, so that an independent restatement (tests/remap.py, numpy float64)
 * reproduces every byte.
 *
 * rd_lens is the SOURCE camera: focal lengths and principal point in pixels and the Brown-Conrady coefficients in OpenCV's order (k1, k2, p1, p2, k3).  rd_view is
 * the ideal camera of the OUTPUT.  Pixel centres sit at integers.
 *
 * Source position (X, Y) of output pixel (u, v) - IEEE double, exactly these operations in this order, no contraction (rd_remap_points):
 *   x = (u - view.cx) / view.fx;   y = (v - view.cy) / view.fy
 *   xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy
 *   rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0
 *   xd = (x*rad + (2.0*p1)*xy) + p2*(r2 + 2.0*xx)
 *   yd = (y*rad + p1*(r2 + 2.0*yy)) + (2.0*p2)*xy
 *   X = lens.fx*xd + lens.cx;   Y = lens.fy*yd + lens.cy
 * (Believed to be the map of OpenCV's initUndistortRectifyMap with R = I, up to the order of roundings; not checked - there is no OpenCV to check against.)
 *
 * Table entry of (u, v): two int32.  The position is INSIDE when X >= 0 && X <= iw-1 && Y >= 0 && Y <= ih-1 for an iw x ih source - compared in double, so a NaN or
 * an infinity is outside; X = -0.0 and X = iw-1 are inside.
 *   inside:   xi = (int)floor(X * 256.0);   yi = (int)floor(Y * 256.0)
 *   outside:  xi = yi = -1
 * The table is ow * oh entries, rows back to back: entry (u, v) at table[2 * (v*ow + u)], xi first.
 *
 * A caller's own map: two planes of ow * oh float32, mapx and mapy, rows back to back - what cv::initUndistortRectifyMap(..., CV_32FC1), a fisheye calibration or
 * a stereo rectification hands out.  With X = (double)mapx[v*ow + u] and Y = (double)mapy[v*ow + u] the same entry rule applies (rd_remap_table_map): both sources
 * end in the one table, and one kernel applies it.
 *
 * Output pixel (u, v): 3 bytes B, G, R at out + v * out_pitch + 3 * u.  An outside entry gives the job's fill colour.  Otherwise
 *   x0 = xi >> 8;  fx = xi & 255;  x1 = min(x0+1, iw-1)                                (y0, fy, y1 the same with yi and ih)
 * and per channel, in int32, with p(x, y) the channel's byte of source pixel (x, y):
 *   top = p(x0,y0)*(256-fx) + p(x1,y0)*fx;   bot = p(x0,y1)*(256-fx) + p(x1,y1)*fx
 *   out = (top*(256-fy) + bot*fy + 32768) >> 16
 * - the rectifier's blend.  p is the (B, G, R) of the source pixel under the conversion contract above: for NV12 and I420 each of the four taps is converted first and
 * blended afterwards, so the output from a frame in any format equals, byte for byte, the output from the BGR frame the contract gives for it. */
typedef struct { double fx, fy, cx, cy, k1, k2, p1, p2, k3; } rd_lens;   /* 72 bytes: the SOURCE camera; OpenCV's order of the Brown-Conrady coefficients */
typedef struct { double fx, fy, cx, cy; } rd_view;                       /* 32 bytes: the ideal camera of the OUTPUT */

/* host helpers; none needs a GPU */
/* the map above for n arbitrary points: uv[2k], uv[2k+1] = (u, v) -> XY[2k], XY[2k+1] = (X, Y).  The definition the table is built from - and what draws something
 * detected in the undistorted frame onto the ORIGINAL one.  No argument is checked. */
void rd_remap_points(const rd_lens *lens, const rd_view *view, const double *uv, int n, double *XY);
/* The table of an ow x oh output from an iw x ih source, from a lens and a view or from a caller's maps.  Both return the number of INSIDE entries, or -1 with
 * nothing written for bad arguments: a NULL pointer, ow or oh < 1 or > 16384, iw or ih < 1 or > 65536, a lens or view field that is not finite, a view with fx or
 * fy equal to 0. */
int rd_remap_table_lens(const rd_lens *lens, const rd_view *view, int ow, int oh, int iw, int ih, int32_t *table);
int rd_remap_table_map(const float *mapx, const float *mapy, int ow, int oh, int iw, int ih, int32_t *table);
/* (double)(ow / 2) / view->fx, with the integer half width the pose fit uses: the tanAOV to pass to rd_detector_poll for frames made with this view */
double rd_view_tan_aov(const rd_view *view, int ow);
/* out[0], out[1]: the smallest and the largest ow and oh (1, 16384); out[2], out[3]: the smallest and the largest iw and ih (1, 65536) */
void rd_remap_limits(int32_t out[4]);

/* A remapper makes ow x oh BGR frames from iw x ih source frames, up to njobs jobs in flight, on one stream of its own.  Create builds the table on the host with the
 * functions above and uploads it once (8 bytes per output pixel of device memory).  NULL on their argument errors, njobs < 1 or > 1024, no such device. */
typedef struct rd_remapper rd_remapper;
rd_remapper *rd_remapper_create_lens(int device, const rd_lens *lens, const rd_view *view, int ow, int oh, int iw, int ih, int njobs);
rd_remapper *rd_remapper_create_map(int device, const float *mapx, const float *mapy, int ow, int oh, int iw, int ih, int njobs);
void rd_remapper_destroy(rd_remapper *r);                 /* waits for the jobs in flight */
int rd_remapper_inside(const rd_remapper *r);             /* entries of its table that are inside; -1 for a bad handle */
/* One job: the ow x oh output of one source frame - iw x ih, the remapper's - in pixel format `format` (RD_PIX_*; planes / pitches as for rd_detector_enqueue_planes).
 * on_device: where the source lies, as for rd_rectifier_enqueue - RD_FRAME_HOST (copied into the remapper's own device buffer, which grows on demand, before the call
 *   returns), RD_FRAME_DEVICE (read in place) or RD_FRAME_HOST_PINNED (the copy engine reads it in place; memory that is not pinned is fatal); device and pinned frames
 *   stay valid and unchanged until the job's rd_remapper_wait returned.
 * fill_bgr: the colour of outside pixels, B | G << 8 | R << 16.
 * out / out_pitch / out_kind: where the frame goes, its row stride in bytes (>= 3 * ow) and what memory it is - RD_FRAME_DEVICE (the kernel writes there) or
 *   RD_FRAME_HOST_PINNED (the copy engine does).  Only the 3 * ow row bytes are written: the pitch padding of `out` is left alone.  Valid until the job's wait.
 * Returns the job's sequence number, or -1 with nothing enqueued for an argument error: an unknown format, on_device or out_kind, a NULL plane the format uses, a pitch
 * smaller than its plane's row, NV12 / I420 with an odd iw or ih, out NULL, out_pitch < 3 * ow, `out` not memory of the kind out_kind names (pageable memory; only the
 * kind of the memory at `out` is asked about - that it holds (oh-1) * out_pitch + 3 * ow bytes is the caller's contract).  A call with njobs jobs already in flight is
 * fatal, as it is for the detector.
 *
 * Hand-over to the detector: after rd_remapper_wait the caller passes a device `out` to rd_detector_enqueue(d, out, out_pitch, RD_FRAME_DEVICE) of a detector of
 * ow x oh pixels, polls with rd_view_tan_aov(view, ow), and keeps `out` until that frame's poll returned; every rd_detector_*_polled service then reads the
 * undistorted frame in place.  With njobs > 1 and as many `out` frames the remap of frame n+1 runs while frame n is detected.  Rectangles come back in the
 * coordinates of the OUTPUT; rd_remap_points takes them to the original frame. */
long rd_remapper_enqueue(rd_remapper *r, int format, const void *const planes[3], const int pitches[3], int on_device, uint32_t fill_bgr, void *out, int out_pitch,
                         int out_kind);
int rd_remapper_wait(rd_remapper *r);                     /* the oldest job: blocks until its frame is where it was told to go; 0, or -1: no job in flight */

/* ---- synthetic frames (csrc/rd_synth.c) */
int rd_synth_num_quads(int iw, int ih);
void rd_synth_frame(uint8_t *bgr, int iw, int ih, int ws, uint64_t seed, int t, int noise);

#if defined(__cplusplus)
}
#endif
#endif
