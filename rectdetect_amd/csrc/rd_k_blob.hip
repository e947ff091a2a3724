// rectdetect-mi355x: page components for gfx950 - the component stage of a blobs job, and the ink decision of its fixed level (radius == 0).  The contract is in
// include/rectdetect_hip.h ("page components"): from n pages of ONE BIT per pixel (the RD_SCAN_BITS layout, written by rdk::scan or by k_blob_level here) to a head,
// max_blobs records and, where the spec asks for it, the cleaned page per quad.  Integers only; every sum that crosses threads is a sum of integers added with
// atomics, every box edge an atomic minimum or maximum: any order gives the same bytes.  The output is zeroed on the stream first, as the grade job's is.
//
// Scratch per quad: `labels`, an int per page pixel (-1: no ink; otherwise the page index j*pw + i of a pixel of the same component, nearer to its root; a root
// points at itself), and `areas`, an int per page pixel.  Hooks always go towards the SMALLER index, so a component's root IS its `first`.  The bits lie at the
// start of `areas` when the stage begins: the tile kernel is their only reader, and the stream zeroes `areas` behind it.  Nothing of a previous job survives:
// `labels` is set to -1 and `areas` to 0 on the stream in every job.
//
// The launches (quad = blockIdx.z; an invalid quad's blocks return at once - its bytes are zero already):
//   1. k_blob_tile, a block of 4 waves per tile of 64 x 32 pixels (rd_blob_tile.h), wave w its rows 8w .. 8w+7, the 64 lanes 64 consecutive pixels of ONE row: the
//      row's ink as a ballot; a pixel's label starts as the first pixel of its run (from the ballot, no read); the first lane of each run then unites it in LDS with
//      every run of the row above that it touches (the mask of the row above, cut to the run's reach - one column further on each side under 8-connectivity -, one
//      union per run of that cut); every ink pixel walks to its root and stores it as a page index.  A tile without ink returns behind the ballots.
//   2. k_blob_border, a thread per pixel of a tile's first column or first row (not the page's): unites the pixel with its neighbours in the tile to the left
//      (W, and NW, SW under 8-connectivity) or above (N, and NW, NE) on the global plane with atomic-min hooks.  Of any two neighbours in different tiles one lies
//      on such a column or row and has the other among these - the diagonal across a tile CORNER included.  Not launched for a page of one tile.
//   3. k_blob_area: every ink pixel walks to its root and stores it (labels are flat from here on); the first lane of each run (of a wave's 64 pixels) adds the
//      run's length to areas[root]: one atomic per run, not per pixel.
//   4. k_blob_rank, ONE block of 16 waves per quad: wave w takes the w-th sixteenth of the page in raster order, 64 pixels at a time.  A first walk counts the
//      roots, the kept ones, the ink, the kept ink and the largest area; the waves' kept counts are prefixed in LDS; a second walk gives every kept root its rank -
//      the wave's base + the kept roots before it, popcounts of ballots - so ranks ascend with `first` whatever the scheduling.  It overwrites areas[root] with the
//      rank (-1: not kept) and, where rank < max_blobs, WRITES the record's area, first, y0 (the first pixel's row: no pixel lies above it) and the INITIAL x0 (the
//      first pixel's column - the record pass lowers it; the stream's zero would win every minimum).  x1, y1, sx, sy start from the stream's zero.  Thread 0 writes the head.
//   5. k_blob_records: per run atomicMin on x0, atomicMax on x1 and y1, 64-bit atomicAdd of the closed-form sum of i and of len * j into record `rank` where
//      rank < max_blobs; and the cleaned page, a ballot of "my root is kept" per 64 pixels, stored as rdk::scan stores RD_SCAN_BITS rows.
// Every index is bounded by the page: a label is only ever a page index of an ink pixel written by these kernels, lanes beyond pw or ph neither load nor store.
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include "rd_blob_tile.h"

namespace {

constexpr int TW = RD_BLOB_TILE_W, TH = RD_BLOB_TILE_H, WAVES = 4, ROWS = TH / WAVES, RANK_WAVES = 16;
static_assert(TW == RD_WAVE && TH % WAVES == 0, "a wave row is 64 pixels");
static_assert(sizeof(rd_blob_head) == 32 && sizeof(rd_blob) == 40, "the head and the records lie back to back, the 64-bit sums aligned");

__device__ __forceinline__ int ld_lds(const int *lab, int a) { return __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ld_dev(const int *lab, int a) { return __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool LDS> __device__ __forceinline__ int find(const int *lab, int a) {
  int l = LDS ? ld_lds(lab, a) : ld_dev(lab, a);
  while (l != a) { a = l; l = LDS ? ld_lds(lab, a) : ld_dev(lab, a); }
  return a;
}
// hooks the larger root under the smaller; where somebody else hooked it meanwhile, goes on with what it hung under
template <bool LDS> __device__ __forceinline__ void unite(int *lab, int a, int b) {
  for (;;) {
    a = find<LDS>(lab, a);
    b = find<LDS>(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ unsigned long long below(int lane) { return (1ull << lane) - 1ull; }
// the length of the run of ones of m that starts at `lane` (m has bit `lane` set)
__device__ __forceinline__ int run_length(unsigned long long m, int lane) {
  const unsigned long long x = ~(m >> lane);
  return x ? __builtin_ctzll(x) : RD_WAVE;      // (x == 0: lane 0 of a full row)
}
// pixel i of a row of packed bits; 0 beyond pw: the pad bits are never read as ink
__device__ __forceinline__ bool page_bit(const uint8_t *row, int i, int pw) { return i < pw && (row[i >> 3] >> (7 - (i & 7)) & 1); }

// row j of a page of packed bits, the 64 pixels from column tx0 (a multiple of 64): as rd_k_scan.hip stores RD_SCAN_BITS rows.  Called by whole waves; v is false beyond pw
__device__ __forceinline__ void store_bits(uint8_t *page, int pw, int tx0, int j, int lane, bool v) {
  const unsigned long long rev = __builtin_bswap64(__builtin_bitreverse64(__ballot(v)));      // byte b: pixels 8b .. 8b+7, the first in bit 7
  const int rb = (pw + 7) >> 3, nb = min(8, rb - (tx0 >> 3));
  uint8_t *row = page + (size_t)j * rb + (tx0 >> 3);
  if (nb == 8 && ((uintptr_t)row & 7) == 0) { if (lane == 0) *(unsigned long long *)row = rev; }
  else if (lane < nb) row[lane] = (uint8_t)(rev >> (8 * lane));
}

// radius == 0: ink = G <= k on the (inverted) G plane, packed as the scan kernel packs it
__global__ __launch_bounds__(TW * WAVES) void k_blob_level(uint8_t *bits, const uint8_t *plane, const rdk::RectifyQuad *quads, int pw, int ph, int k, int invert) {
  const int lane = threadIdx.x, tx0 = blockIdx.x * TW, i = tx0 + lane, j = blockIdx.y * WAVES + rd::rd_ty();
  if (j >= ph || !quads[blockIdx.z].status) return;      // (the whole wave; an invalid quad's bits are never read)
  const uint8_t *src = plane + (size_t)blockIdx.z * ((size_t)pw * ph);
  bool ink = false;
  if (i < pw) { const int g = src[(size_t)j * pw + i]; ink = (invert ? 255 - g : g) <= k; }
  store_bits(bits + (size_t)blockIdx.z * ((size_t)((pw + 7) >> 3) * ph), pw, tx0, j, lane, ink);
}

__global__ __launch_bounds__(TW * WAVES) void k_blob_tile(int *labels, const uint8_t *bits, const rdk::RectifyQuad *quads, int pw, int ph, int reach) {
  __shared__ int lab[TH * TW];
  __shared__ unsigned long long rowmask[TH];
  const int lane = threadIdx.x, wave = rd::rd_ty();
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, i = tx0 + lane;
  if (quads && !quads[blockIdx.z].status) return;      // (the whole block)
  const int rb = (pw + 7) >> 3;
  const uint8_t *page = bits + (size_t)blockIdx.z * ((size_t)rb * ph);
  int *L = labels + (size_t)blockIdx.z * ((size_t)pw * ph);

  // the rows' ink; a pixel's label: the first pixel of its run
  unsigned long long seen = 0;
#pragma unroll
  for (int q = 0; q < ROWS; q++) {
    const int jl = wave * ROWS + q, j = ty0 + jl;
    const bool ink = j < ph && page_bit(page + (size_t)j * rb, i, pw);
    const unsigned long long m = __ballot(ink), gaps = ~m & below(lane);
    seen |= m;
    if (lane == 0) rowmask[jl] = m;
    lab[jl * TW + lane] = ink ? jl * TW + (gaps ? 64 - __clzll((long long)gaps) : 0) : -1;
  }
  if (!__syncthreads_or(seen != 0)) return;      // a tile without ink

  // the first lane of each run: the runs of the row above that it touches
#pragma unroll
  for (int q = 0; q < ROWS; q++) {
    const int jl = wave * ROWS + q;
    if (jl == 0) continue;
    const unsigned long long m = rowmask[jl], up = rowmask[jl - 1];
    if ((m >> lane & 1) && (lane == 0 || !(m >> (lane - 1) & 1))) {
      const int lo = max(lane - reach, 0), hi = min(lane + run_length(m, lane) - 1 + reach, RD_WAVE - 1);
      unsigned long long ov = up & ~below(lo) & (hi == RD_WAVE - 1 ? ~0ull : below(hi + 1));
      while (ov) {
        const int b = __builtin_ctzll(ov);
        unite<true>(lab, jl * TW + lane, (jl - 1) * TW + b);
        ov &= ov + (1ull << b);      // (drops the lowest run of ones: one union per run above)
      }
    }
  }
  __syncthreads();

  // roots as page indices
#pragma unroll
  for (int q = 0; q < ROWS; q++) {
    const int jl = wave * ROWS + q, j = ty0 + jl;
    if (j < ph && i < pw && (rowmask[jl] >> lane & 1)) {
      const int r = find<true>(lab, jl * TW + lane);
      L[j * pw + i] = (ty0 + r / TW) * pw + tx0 + (r & (TW - 1));
    }
  }
}

// a thread per pixel of the first column of a tile column (the first nv threads: column c * TW, c >= 1, row t % ph) or of the first row of a tile row
__global__ __launch_bounds__(256) void k_blob_border(int *labels, const rdk::RectifyQuad *quads, int pw, int ph, int nv, int total, int reach) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total || (quads && !quads[blockIdx.z].status)) return;
  int *L = labels + (size_t)blockIdx.z * ((size_t)pw * ph);
  int i, j;
  const bool vertical = t < nv;
  if (vertical) { i = (t / ph + 1) * TW; j = t % ph; }
  else { const int u = t - nv; j = (u / pw + 1) * TH; i = u % pw; }
  const int p = j * pw + i;
  if (ld_dev(L, p) < 0) return;
  if (vertical) {      // W, NW, SW
    for (int dj = -reach; dj <= reach; dj++) {
      const int y = j + dj;
      if (y >= 0 && y < ph && ld_dev(L, y * pw + i - 1) >= 0) unite<false>(L, p, y * pw + i - 1);
    }
  } else {             // N, NW, NE
    for (int di = -reach; di <= reach; di++) {
      const int x = i + di;
      if (x >= 0 && x < pw && ld_dev(L, (j - 1) * pw + x) >= 0) unite<false>(L, p, (j - 1) * pw + x);
    }
  }
}

__global__ __launch_bounds__(TW * WAVES) void k_blob_area(int *labels, int *areas, const rdk::RectifyQuad *quads, int pw, int ph) {
  const int lane = threadIdx.x, tx0 = blockIdx.x * TW, i = tx0 + lane, j = blockIdx.y * WAVES + rd::rd_ty();
  if (j >= ph || (quads && !quads[blockIdx.z].status)) return;      // (the whole wave)
  int *L = labels + (size_t)blockIdx.z * ((size_t)pw * ph), *A = areas + (size_t)blockIdx.z * ((size_t)pw * ph);
  const int p = j * pw + i;
  const bool ink = i < pw && ld_dev(L, p) >= 0;
  const unsigned long long m = __ballot(ink);
  if (!ink) return;
  const int root = find<false>(L, p);
  L[p] = root;      // (an ancestor of p, as every value this word ever held: a walk that passes here meanwhile still ends at the root)
  if (lane == 0 || !(m >> (lane - 1) & 1)) atomicAdd(&A[root], run_length(m, lane));
}

__global__ __launch_bounds__(RD_WAVE * RANK_WAVES) void k_blob_rank(uint8_t *out, const int *labels, int *areas, const rdk::RectifyQuad *quads, int pw, int ph, size_t patch_bytes,
                                                                    int min_area, int max_area, int max_blobs) {
  __shared__ int sums[RANK_WAVES][4], most[RANK_WAVES];
  const int lane = threadIdx.x, wave = rd::rd_ty(), npix = pw * ph;
  if (quads && !quads[blockIdx.x].status) return;      // (the whole block)
  const int *L = labels + (size_t)blockIdx.x * (size_t)npix;
  int *A = areas + (size_t)blockIdx.x * (size_t)npix;
  uint8_t *quad = out + (size_t)blockIdx.x * patch_bytes;
  const int span = ((npix + RANK_WAVES - 1) / RANK_WAVES + RD_WAVE - 1) / RD_WAVE * RD_WAVE, p0 = min(wave * span, npix), p1 = min(p0 + span, npix);

  int all = 0, found = 0, ink = 0, kept_ink = 0, largest = 0;      // per lane; added up below
  for (int q = p0; q < p1; q += RD_WAVE) {
    const int p = q + lane;
    const bool root = p < p1 && L[p] == p;
    const int a = root ? A[p] : 0;
    const bool kept = root && a >= min_area && (max_area == 0 || a <= max_area);
    all += root; found += kept; ink += a; kept_ink += kept ? a : 0; largest = max(largest, a);
  }
#pragma unroll
  for (int o = RD_WAVE / 2; o > 0; o >>= 1) {
    all += __shfl_down(all, o, RD_WAVE); found += __shfl_down(found, o, RD_WAVE); ink += __shfl_down(ink, o, RD_WAVE); kept_ink += __shfl_down(kept_ink, o, RD_WAVE);
    largest = max(largest, __shfl_down(largest, o, RD_WAVE));
  }
  if (lane == 0) { sums[wave][0] = all; sums[wave][1] = found; sums[wave][2] = ink; sums[wave][3] = kept_ink; most[wave] = largest; }
  __syncthreads();
  int rank0 = 0;
  for (int w = 0; w < wave; w++) rank0 += sums[w][1];

  rd_blob *recs = (rd_blob *)(quad + sizeof(rd_blob_head));
  for (int q = p0; q < p1; q += RD_WAVE) {
    const int p = q + lane;
    const bool root = p < p1 && L[p] == p;
    const int a = root ? A[p] : 0;
    const bool kept = root && a >= min_area && (max_area == 0 || a <= max_area);
    const unsigned long long km = __ballot(kept);
    const int rank = rank0 + __popcll(km & below(lane));
    if (root) A[p] = kept ? rank : -1;
    if (kept && rank < max_blobs) {
      rd_blob *r = recs + rank;
      const int y = p / pw;
      r->x0 = p - y * pw; r->y0 = y; r->area = a; r->first = p;
    }
    rank0 += __popcll(km);
  }
  if (wave == 0 && lane == 0) {
    rd_blob_head h = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int w = 0; w < RANK_WAVES; w++) { h.all += sums[w][0]; h.found += sums[w][1]; h.ink += sums[w][2]; h.ink_kept += sums[w][3]; h.largest = max(h.largest, most[w]); }
    h.written = min(h.found, max_blobs);
    h.flags = h.found > max_blobs ? RD_BLOB_OVERFLOW : 0;
    *(rd_blob_head *)quad = h;
  }
}

template <int PAGE> __global__ __launch_bounds__(TW * WAVES) void k_blob_records(uint8_t *out, const int *labels, const int *areas, const rdk::RectifyQuad *quads, int pw, int ph,
                                                                                 size_t patch_bytes, int max_blobs) {
  const int lane = threadIdx.x, tx0 = blockIdx.x * TW, i = tx0 + lane, j = blockIdx.y * WAVES + rd::rd_ty();
  if (j >= ph || (quads && !quads[blockIdx.z].status)) return;      // (the whole wave)
  const int *L = labels + (size_t)blockIdx.z * ((size_t)pw * ph), *A = areas + (size_t)blockIdx.z * ((size_t)pw * ph);
  uint8_t *quad = out + (size_t)blockIdx.z * patch_bytes;
  const int root = i < pw ? L[j * pw + i] : -1;
  const int rank = root >= 0 ? A[root] : -1;      // (-1: no ink here, or a component that is not kept)
  const unsigned long long m = __ballot(rank >= 0);      // (a run of kept ink is a run of ONE component: ink pixels side by side are connected)
  if (PAGE) store_bits(quad + sizeof(rd_blob_head) + sizeof(rd_blob) * (size_t)max_blobs, pw, tx0, j, lane, rank >= 0);
  if (rank >= 0 && rank < max_blobs && (lane == 0 || !(m >> (lane - 1) & 1))) {
    rd_blob *r = (rd_blob *)(quad + sizeof(rd_blob_head)) + rank;
    const long long len = run_length(m, lane);
    atomicMin(&r->x0, i);
    atomicMax(&r->x1, i + (int)len - 1);
    atomicMax(&r->y1, j);
    atomicAdd((unsigned long long *)&r->sx, (unsigned long long)(len * i + len * (len - 1) / 2));
    atomicAdd((unsigned long long *)&r->sy, (unsigned long long)(len * j));
  }
}

}  // namespace

namespace rdk {

void blob_level(hipStream_t s, uint8_t *bits, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_blob_spec &spec) {
  if (n <= 0) return;
  const dim3 block(TW, WAVES), grid((pw + TW - 1) / TW, (ph + WAVES - 1) / WAVES, n);
  hipLaunchKernelGGL(k_blob_level, grid, block, 0, s, bits, plane, quads, pw, ph, spec.k, spec.invert);
}

void blobs(hipStream_t s, uint8_t *out, int *labels, int *areas, const RectifyQuad *quads, int n, int pw, int ph, const rd_blob_spec &spec, int info[8]) {
  if (info) for (int k = 0; k < 8; k++) info[k] = 0;
  if (n <= 0) return;
  const size_t patch_bytes = rd_blob_bytes(&spec, pw, ph), npix = (size_t)pw * ph;
  if (!patch_bytes) { fprintf(stderr, "rdk::blobs: not a legal blob spec for %d x %d\n", pw, ph); abort(); }      // (rd_rectifier_create_blobs refuses it first)
  const int ntx = (pw + TW - 1) / TW, nty = (ph + TH - 1) / TH, reach = spec.connectivity == 8 ? 1 : 0;
  const int nv = (ntx - 1) * ph, total = nv + (nty - 1) * pw;
  const dim3 block(TW, WAVES), rows(ntx, (ph + WAVES - 1) / WAVES, n);
  (void)hipMemsetAsync(out, 0, (size_t)n * patch_bytes, s);      // (a failure shows at the caller's check of the launches)
  (void)hipMemsetAsync(labels, 0xff, (size_t)n * npix * sizeof(int), s);
  hipLaunchKernelGGL(k_blob_tile, dim3(ntx, nty, n), block, 0, s, labels, (const uint8_t *)areas, quads, pw, ph, reach);
  (void)hipMemsetAsync(areas, 0, (size_t)n * npix * sizeof(int), s);      // (behind the only reader of the bits)
  if (total > 0) hipLaunchKernelGGL(k_blob_border, dim3((total + 255) / 256, 1, n), dim3(256), 0, s, labels, quads, pw, ph, nv, total, reach);
  hipLaunchKernelGGL(k_blob_area, rows, block, 0, s, labels, areas, quads, pw, ph);
  hipLaunchKernelGGL(k_blob_rank, dim3(n), dim3(RD_WAVE, RANK_WAVES), 0, s, out, labels, areas, quads, pw, ph, patch_bytes, spec.min_area, spec.max_area, spec.max_blobs);
  if (spec.page) hipLaunchKernelGGL((k_blob_records<1>), rows, block, 0, s, out, labels, areas, quads, pw, ph, patch_bytes, spec.max_blobs);
  else hipLaunchKernelGGL((k_blob_records<0>), rows, block, 0, s, out, labels, areas, quads, pw, ph, patch_bytes, spec.max_blobs);
  if (info) { info[0] = 0; info[1] = 4 + (total > 0); info[2] = 3; info[3] = ntx; info[4] = nty; info[5] = total > 0; }
}

}  // namespace rdk
