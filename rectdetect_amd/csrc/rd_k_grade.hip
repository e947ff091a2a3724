// rectdetect-mi355x: graded quads for gfx950 - the second launch of a grade job: from the G plane the tensor kernel wrote (rd_k_tensor.hip, { U8, NHWC, GRAY, m }) to
// the records of a cells x cells grid and, where the spec asks for it, the patch's histogram.  The arithmetic is the contract in include/rectdetect_hip.h ("graded
// quads").  The first kernel of the job family that sums ACROSS blocks: a cell of a large patch is many tiles, so a block adds what it found to the quad's records
// with atomics.  Every sum is a sum of integers - any order gives the same bits - which is what makes atomics acceptable in a tree whose contracts are exact; the
// records are zeroed on the job's stream before the launch (rd_rectify.hip) and nothing reads them before the job's event.
//
// Launch shape: the scan kernel's grid (tiles in x, tiles in y, quads); a block is 4 waves and reduces a tile of 64 x 16 pixels (rd_grade_tile.h); wave w takes rows
// 4w .. 4w+3 of it, its 64 lanes 64 consecutive pixels of ONE row.
//   0. g[18][66] bytes in LDS: the tile with a one-pixel halo, coordinates clamped to the patch (the replicated border of step 2), every load issued before the first
//      is used.  An invalid quad's block leaves here: its bytes are zero already.
//   1. a lane makes G, L and the four predicates of its pixel in each of the wave's rows and adds them up in registers for as long as the rows lie in one cell row
//      (cy is a scalar; the lane's cx never changes): six 32-bit words - n | lo << 16, hi | ne << 16, sg, sgg, sl, sll; a wave's four rows cannot overflow them
//      (256 pixels: counts <= 256, sll <= 256 * 1 040 400).
//   2. across the wave by shuffles: where the row lies in one cell (always when 64 * cells <= pw) a plain reduction to lane 0, otherwise the same six steps
//      segmented by cx - lanes of a cell are consecutive, a lane adds its partner's value only where the partner is in its own cell - to the first lane of each cell.
//   3. those lanes add the eight fields to the block's slots in LDS, one per cell the tile can touch (8 x 8, 32-bit: a tile is 1024 pixels, sll <= 1024 * 1 040 400
//      < 2^31), with LDS atomics: four waves, at most eight cells each.
//   4. the block adds every slot field that is not zero to the quad's record: one global atomic per field, 32-bit for the counts, 64-bit for the sums (a touched
//      cell has n > 0; slots of cells the tile does not reach stay zero and cost nothing).
// Histogram: a sub-histogram per wave in LDS (LDS atomics, no wave waits for another), merged by bin and added to the quad's 256 words once per block, zero bins skipped.
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include "rd_grade_tile.h"

// a timing-only build (tools/variants.sh, tools/bench_grade.py --variant): 0 lets one tile per quad flush - wrong records, the reduction kept - to show what step 4 costs
#ifndef RD_GRADE_FLUSH
#define RD_GRADE_FLUSH 1
#endif

namespace {

constexpr int TW = RD_GRADE_TILE_W, TH = RD_GRADE_TILE_H, WAVES = 4, ROWS = TH / WAVES, GW = TW + 2, GH = TH + 2, MAXC = RD_GRADE_MAX_CELLS, FIELDS = 8;
static_assert(TW == RD_WAVE && TH % WAVES == 0, "a wave row is 64 pixels");
static_assert(sizeof(rd_grade_cell) == 48 && sizeof(rd_grade_cell) % 8 == 0, "records lie back to back, their 64-bit sums aligned");

struct Acc { uint32_t c0, c1, sg, sgg, sl, sll; };      // (sl: two's complement)

// one step of the reduction: v of the lane o further on, added where `take`
__device__ __forceinline__ void step(Acc &a, int o, bool take) {
  const uint32_t c0 = __shfl_down(a.c0, o, RD_WAVE), c1 = __shfl_down(a.c1, o, RD_WAVE), sg = __shfl_down(a.sg, o, RD_WAVE), sgg = __shfl_down(a.sgg, o, RD_WAVE),
                 sl = __shfl_down(a.sl, o, RD_WAVE), sll = __shfl_down(a.sll, o, RD_WAVE);
  if (take) { a.c0 += c0; a.c1 += c1; a.sg += sg; a.sgg += sgg; a.sl += sl; a.sll += sll; }
}

// steps 2 and 3: what the wave's lanes hold for cell row lcy (tile-local) into the block's slots.  one: every lane of the wave has the same cx (a scalar)
__device__ __forceinline__ void wave_to_slots(Acc a, uint32_t *slots, int lcy, int lcx, int cx, int lane, bool one) {
  bool head;
  if (one) {
#pragma unroll
    for (int o = 1; o < RD_WAVE; o <<= 1) step(a, o, true);      // (lanes near the end add values they need not: only lane 0's sum is used, and it is right)
    head = lane == 0;
  } else {
#pragma unroll
    for (int o = 1; o < RD_WAVE; o <<= 1) {
      const int pcx = __shfl_down(cx, o, RD_WAVE);
      step(a, o, lane + o < RD_WAVE && pcx == cx);
    }
    const int before = __shfl_up(cx, 1, RD_WAVE);
    head = lane == 0 || before != cx;
  }
  if (head) {
    uint32_t *s = slots + (lcy * MAXC + lcx) * FIELDS;
    atomicAdd(s + 0, a.c0 & 0xffffu); atomicAdd(s + 1, a.c0 >> 16); atomicAdd(s + 2, a.c1 & 0xffffu); atomicAdd(s + 3, a.c1 >> 16);
    atomicAdd(s + 4, a.sg); atomicAdd(s + 5, a.sgg); atomicAdd(s + 6, a.sl); atomicAdd(s + 7, a.sll);
  }
}

template <int HIST> __global__ __launch_bounds__(TW * WAVES) void k_grade(uint8_t *out, const uint8_t *plane, const rdk::RectifyQuad *quads, int pw, int ph, size_t patch_bytes,
                                                                          int cells, int dark, int bright, int edge) {
  __shared__ uint8_t g[GH * GW];
  __shared__ uint32_t slots[MAXC * MAXC * FIELDS];
  __shared__ uint32_t hist[HIST ? WAVES * 256 : 1];
  const int lane = threadIdx.x, wave = rd::rd_ty(), tid = wave * TW + lane;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, i = tx0 + lane;
  if (!quads[blockIdx.z].status) return;      // (the whole block; the stream zeroed the quad's bytes)
  const uint8_t *src = plane + (size_t)blockIdx.z * ((size_t)pw * ph);

  // 0. the tile and its halo, the slots and the sub-histograms
  rd::stage_cells<GH * GW, TW * WAVES>(tid, src,
    [&](int t, int &a) { const int y = t / GW, x = t - y * GW; a = rd::clampi(ty0 - 1 + y, 0, ph - 1) * pw + rd::clampi(tx0 - 1 + x, 0, pw - 1); return true; },      // (below 2^28)
    [&](int t, bool, uint8_t v) { g[t] = v; });
  for (int t = tid; t < MAXC * MAXC * FIELDS; t += TW * WAVES) slots[t] = 0;
  if (HIST) for (int t = tid; t < WAVES * 256; t += TW * WAVES) hist[t] = 0;
  __syncthreads();

  // 1.-3. this wave's rows
  const int cx0 = (tx0 * cells) / pw, cy0 = (ty0 * cells) / ph;      // the first cell the tile touches
  const int cx = (min(i, pw - 1) * cells) / pw;                     // (lanes beyond the patch: the last cell, with nothing to add)
  const bool one = __builtin_amdgcn_readfirstlane(cx) == __builtin_amdgcn_readlane(cx, RD_WAVE - 1);
  const bool in = i < pw;
  Acc a = { 0, 0, 0, 0, 0, 0 };
  int cur = -1;
  for (int q = 0; q < ROWS; q++) {
    const int jl = wave * ROWS + q, j = ty0 + jl;
    if (j >= ph) break;      // (the whole wave)
    const int cy = (j * cells) / ph;
    if (cy != cur && cur >= 0) { wave_to_slots(a, slots, cur - cy0, cx - cx0, cx, lane, one); a = Acc{ 0, 0, 0, 0, 0, 0 }; }
    cur = cy;
    if (in) {
      const uint8_t *c = g + (jl + 1) * GW + lane + 1;
      const int G = c[0], L = (int)c[-1] + (int)c[1] + (int)c[-GW] + (int)c[GW] - 4 * G;
      a.c0 += 1u | (uint32_t)(G <= dark) << 16;
      a.c1 += (uint32_t)(G >= bright) | (uint32_t)(abs(L) >= edge) << 16;
      a.sg += (uint32_t)G; a.sgg += (uint32_t)(G * G);
      a.sl += (uint32_t)L; a.sll += (uint32_t)(L * L);
      if (HIST) atomicAdd(&hist[wave * 256 + G], 1u);
    }
  }
  if (cur >= 0) wave_to_slots(a, slots, cur - cy0, cx - cx0, cx, lane, one);
  __syncthreads();

  // 4. the block's share of the quad's records
  if (!RD_GRADE_FLUSH && (blockIdx.x | blockIdx.y)) return;
  uint8_t *quad = out + (size_t)blockIdx.z * patch_bytes;
  for (int t = tid; t < MAXC * MAXC * FIELDS; t += TW * WAVES) {
    const uint32_t v = slots[t];
    if (!v) continue;
    const int f = t & (FIELDS - 1), lc = t / FIELDS, ccx = cx0 + (lc & (MAXC - 1)), ccy = cy0 + lc / MAXC;      // (v != 0: a cell the tile touched, so inside the grid)
    uint8_t *rec = quad + (size_t)(ccy * cells + ccx) * sizeof(rd_grade_cell);
    if (f < 4) atomicAdd((int *)rec + f, (int)v);
    else atomicAdd((unsigned long long *)(rec + 16) + (f - 4), f == 6 ? (unsigned long long)(long long)(int)v : (unsigned long long)v);      // (sl: sign-extended)
  }
  if (HIST) {
    uint32_t *qh = (uint32_t *)(quad + (size_t)cells * cells * sizeof(rd_grade_cell));
    const uint32_t v = hist[tid] + hist[256 + tid] + hist[512 + tid] + hist[768 + tid];      // (256 threads, 256 bins)
    if (v) atomicAdd(qh + tid, v);
  }
}
static_assert(TW * WAVES == 256, "a thread per bin");

}  // namespace

namespace rdk {

void grade(hipStream_t s, uint8_t *out, const uint8_t *plane, const RectifyQuad *quads, int n, int pw, int ph, const rd_grade_spec &spec) {
  if (n <= 0) return;
  const dim3 block(TW, WAVES), grid((pw + TW - 1) / TW, (ph + TH - 1) / TH, n);
  const size_t patch_bytes = rd_grade_bytes(&spec, pw, ph);
  if (!patch_bytes) { fprintf(stderr, "rdk::grade: not a legal grade spec for %d x %d\n", pw, ph); abort(); }      // (rd_rectifier_create_grade refuses it first)
  if (spec.hist) hipLaunchKernelGGL((k_grade<1>), grid, block, 0, s, out, plane, quads, pw, ph, patch_bytes, spec.cells, spec.dark, spec.bright, spec.edge);
  else hipLaunchKernelGGL((k_grade<0>), grid, block, 0, s, out, plane, quads, pw, ph, patch_bytes, spec.cells, spec.dark, spec.bright, spec.edge);
}

}  // namespace rdk
