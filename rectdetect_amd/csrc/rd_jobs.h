// rectdetect-mi355x: what the services behind the detector's poll share on the host - the rectifier (rd_rectify.hip), the annotator (rd_annotate.hip), the
// compositor (rd_composite.hip) and the matcher (rd_match.hip): the layout of a frame's planes, a device buffer that grows, the ring of jobs in flight on a stream of the service's own, the checks
// of a frame's and a destination's arguments, and a frame's way to the device and back to pinned memory.  Helpers that a service's enqueue calls, top to bottom;
// nothing here knows a kernel, a record or what a job's items are.  No graphs, no threads, no environment switches.
#pragma once
#include "rd_internal.h"
#include "rd_pix.h"
#include <stdlib.h>
#include <string.h>

#pragma GCC visibility push(hidden)      // (helpers of the library's own translation units: none of them is an exported symbol)
namespace rdjob {

// the planes a format uses, their row bytes and rows; and the layout of a frame packed into a buffer of the library's own (row strides rounded up to 4 bytes, so
// that kernels read them a dword per lane; every format then still fits 4 bytes per pixel)
struct PixLayout { int iw, ih, np, row[3], rows[3], pitch[3]; size_t off[3], bytes; };
inline PixLayout pix_layout(int fmt, int iw, int ih) {
  PixLayout L;
  memset(&L, 0, sizeof(L));
  L.iw = iw; L.ih = ih; L.np = rdpix::planes(fmt);
  L.row[0] = iw * rdpix::bpp(fmt); L.rows[0] = ih;
  for (int k = 1; k < L.np; k++) { L.row[k] = L.np == 2 ? iw : iw / 2; L.rows[k] = ih / 2; }      // 4:2:0 chroma: U, V interleaved in one plane, or a plane each
  for (int k = 0; k < L.np; k++) { L.pitch[k] = (L.row[k] + 3) & ~3; L.off[k] = L.bytes; L.bytes += (size_t)L.pitch[k] * L.rows[k]; }
  return L;
}

// what kind of memory the runtime says p is (hipMemoryTypeUnregistered: pageable, or unknown to it); asked per job - a microsecond - because a caller may free a
// buffer and get pageable memory at the same address
inline hipMemoryType memory_type(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return hipMemoryTypeUnregistered; }
  return at.type;
}
// is p what a caller that says `kind` (RD_FRAME_DEVICE or RD_FRAME_HOST_PINNED) must hand over?
inline bool is_kind(const void *p, int kind) { return memory_type(p) == (kind == RD_FRAME_DEVICE ? hipMemoryTypeDevice : hipMemoryTypeHost); }

// a frame where a job reads or writes it (device planes): where the caller's lie
using rdpix::PixFrame;
inline PixFrame planes_at(const void *const planes[3], const int pitches[3], const PixLayout &L) {
  PixFrame f = { { NULL, NULL, NULL }, { 0, 0, 0 }, L.iw, L.ih };
  for (int k = 0; k < L.np; k++) { f.pl[k] = (uint8_t *)planes[k]; f.pitch[k] = pitches[k]; }
  return f;
}

// a device buffer that grows on demand and never shrinks; jobs follow one another on the service's stream, so one buffer serves them all
struct DevBuf {
  uint8_t *p; size_t bytes;
  void grow(hipStream_t st, size_t want) {
    if (bytes >= want) return;
    RD_HIP(hipStreamSynchronize(st));      // (jobs in flight use the old one)
    if (p) RD_HIP(hipFree(p));
    RD_HIP(hipMalloc((void **)&p, want));
    bytes = want;
  }
  void release() { if (p) RD_HIP(hipFree(p)); p = NULL; bytes = 0; }
  PixFrame packed(const PixLayout &L) const {      // a frame packed into it
    PixFrame f = { { NULL, NULL, NULL }, { 0, 0, 0 }, L.iw, L.ih };
    for (int k = 0; k < L.np; k++) { f.pl[k] = p + L.off[k]; f.pitch[k] = L.pitch[k]; }
    return f;
  }
};

// What every service's handle begins with: which service it is, where it lives, how many items one of its jobs takes - and its jobs in flight: one non-blocking
// stream, one event and one item count per slot; a job's own blocks stay with the service, in an array of its own by slot number
#define RD_MAGIC_RECTIFIER 0x52445246u
#define RD_MAGIC_ANNOTATOR 0x5244414eu
#define RD_MAGIC_COMPOSITOR 0x5244434fu
#define RD_MAGIC_MATCHER 0x52444d41u
#define RD_MAGIC_REMAPPER 0x5244524du
struct Ring {
  uint32_t magic;
  int device, per_job, njobs;
  hipStream_t st;
  hipEvent_t *done;
  int *n;
  long next_enqueue, next_wait;
};

// is h a live service of this kind on this device?  The most items one of its jobs takes, or -1
inline int service_capacity(const void *h, uint32_t magic, int device) {
  const Ring *r = (const Ring *)h;
  return r && r->magic == magic && r->device == device ? r->per_job : -1;
}
inline Ring *ring_of(void *h, uint32_t magic, const char *who) {
  Ring *r = (Ring *)h;
  if (!r || r->magic != magic) exitf(-1, "%s: bad handle\n", who);
  return r;
}
inline bool ring_args_ok(int device, int njobs) { return njobs >= 1 && njobs <= 1024 && device >= 0 && device < rd_device_count(); }
inline void ring_create(Ring *r, uint32_t magic, int device, int per_job, int njobs) {      // (r: zeroed; ring_args_ok)
  RD_HIP(hipSetDevice(device));
  r->magic = magic; r->device = device; r->per_job = per_job; r->njobs = njobs;
  RD_HIP(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
  r->done = (hipEvent_t *)calloc(njobs, sizeof(hipEvent_t));
  r->n = (int *)calloc(njobs, sizeof(int));
  for (int k = 0; k < njobs; k++) RD_HIP(hipEventCreateWithFlags(&r->done[k], hipEventDisableTiming));
}
// waits for everything on the stream; the service frees its jobs' blocks and its buffers behind this
inline void ring_destroy(Ring *r) {
  RD_HIP(hipSetDevice(r->device));
  RD_HIP(hipStreamSynchronize(r->st));
  for (int k = 0; k < r->njobs; k++) RD_HIP(hipEventDestroy(r->done[k]));
  RD_HIP(hipStreamDestroy(r->st));
  free(r->done); free(r->n);
  r->magic = 0;
}
// the slot of the next job, of n items; fatal when njobs are in flight
inline int ring_claim(Ring *r, const char *who, int n) {
  if (r->next_enqueue - r->next_wait >= r->njobs) exitf(-1, "%s: %d jobs already in flight (wait first)\n", who, r->njobs);
  const int slot = (int)(r->next_enqueue % r->njobs);
  r->n[slot] = n;
  return slot;
}
// the claimed job ends here on the stream: its sequence number
inline long ring_record(Ring *r) {
  RD_HIP(hipEventRecord(r->done[r->next_enqueue % r->njobs], r->st));
  return r->next_enqueue++;
}
// waits for the oldest job: its slot (its item count: r->n[slot]), or -1 when none is in flight
inline int ring_wait(Ring *r) {
  if (r->next_wait >= r->next_enqueue) return -1;
  RD_HIP(hipSetDevice(r->device));
  const int slot = (int)(r->next_wait++ % r->njobs);
  RD_HIP(hipEventSynchronize(r->done[slot]));
  return slot;
}

// ---- argument checks: false is an argument error (the entry point returns -1; nothing has changed)
inline bool frame_ok(int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device, PixLayout *L) {
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches || iw < 1 || ih < 1 || iw > 65536 || ih > 65536) return false;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return false;
  if (rdpix::is_yuv(format) && ((iw | ih) & 1)) return false;
  *L = pix_layout(format, iw, ih);
  for (int k = 0; k < L->np; k++) if (!planes[k] || pitches[k] < L->row[k]) return false;
  return true;
}
// a destination frame; none (out_planes NULL) is the job in place, which only a device frame can have
inline bool dest_ok(const PixLayout &L, void *const out_planes[3], const int out_pitches[3], int out_kind, int on_device) {
  if (!out_planes) return on_device == RD_FRAME_DEVICE;
  if ((out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) || !out_pitches) return false;
  for (int k = 0; k < L.np; k++) if (!out_planes[k] || out_pitches[k] < L.row[k]) return false;
  return true;
}
// ... and is every plane of it the memory out_kind says (the runtime is asked: the service's device is current)
inline bool dest_memory_ok(const PixLayout &L, void *const out_planes[3], int out_kind) {
  if (out_planes) for (int k = 0; k < L.np; k++) if (!is_kind(out_planes[k], out_kind)) return false;
  return true;
}

// ---- a frame's moves, row bytes only: pitch padding is neither read nor written
// the caller's frame - host, pinned or device memory - to device planes on st; who: the entry point, for the fatal message about planes that are not pinned
inline void bring(hipStream_t st, const char *who, const PixLayout &L, const PixFrame &to, const void *const planes[3], const int pitches[3], int on_device) {
  if (on_device == RD_FRAME_HOST_PINNED)
    for (int k = 0; k < L.np; k++)
      if (memory_type(planes[k]) != hipMemoryTypeHost)
        exitf(-1, "%s: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", who, k, planes[k]);
  for (int k = 0; k < L.np; k++)
    RD_HIP(hipMemcpy2DAsync(to.pl[k], to.pitch[k], planes[k], pitches[k], L.row[k], L.rows[k], on_device == RD_FRAME_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (on_device == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(st));      // (pageable memory: the caller may reuse the buffer when this call returns)
}
// device planes to the caller's pinned planes on st: the caller's pitch padding stays as it is
inline void send(hipStream_t st, const PixLayout &L, void *const out_planes[3], const int out_pitches[3], const PixFrame &from) {
  for (int k = 0; k < L.np; k++)
    RD_HIP(hipMemcpy2DAsync(out_planes[k], out_pitches[k], from.pl[k], from.pitch[k], L.row[k], L.rows[k], hipMemcpyDeviceToHost, st));
}

}  // namespace rdjob
#pragma GCC visibility pop
