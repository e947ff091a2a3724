// rectdetect-mi355x: matched quads for gfx950 - the signature of each quad of a job, its dots with every column of the library on the matrix cores, and the
// choice of the best column and the runner-up.  The arithmetic is the contract in include/rectdetect_hip.h ("matched quads"): integers throughout, and a handful of
// double operations in k_match_pick that nothing here may reorder or contract (-ffp-contract=off, see rd_device.h).
//
// k_signature: a block is ONE wave of 8 x 8 threads and a thread makes one cell of the G x G grid from its m x m patch pixels (rd_rectify_px.h: the rectifier's own
//   pixel), so a wave covers 8m x 8m patch pixels - the rectifier's near-square footprint in the source; no LDS, no barrier.  sa and saa are summed over the wave
//   and added to the quad's two integers atomically: integer sums, any order gives the same result.
// k_match_dots: one wave per 16 x 16 tile of the dot matrix, v_mfma_i32_16x16x64_i8 over D / 64 steps into one accumulator.  Lane l reads 16 bytes of row
//   (l & 15) of A - the job's signatures - and 16 bytes of column (l & 15) of B - the library, a column's D bytes contiguous - at THE SAME byte offset
//   64 * step + 16 * (l >> 4): whatever order the hardware gives the 64 values of k inside a fragment, both operands follow it, and an integer sum has no order.
//   The C/D map - lane l, register r: row 4 * (l >> 4) + r, column l & 15 - is pinned by the exact-data test (tests/test_gpu_match.py).  DESIGN.md, "Matched quads".
// k_match_pick: one wave per quad scans its row of dots twice: the greatest key, then the greatest key among the other templates.
// k_match_rotations: a template's signature into its four columns, a pure permutation.
#include <stdio.h>
#include <stdlib.h>
#include "rd_rectify_px.h"

namespace {

template <int FMT> __global__ __launch_bounds__(64) void k_signature(int8_t *sig, int *sums, PixFrame S, const rdk::RectifyQuad *quads, int G, int m) {
  const int i = blockIdx.x * 8 + threadIdx.x, j = blockIdx.y * 8 + threadIdx.y;      // (G is a multiple of 8: every thread has a cell)
  const rdk::RectifyQuad Q = quads[blockIdx.z];
  int8_t *dst = sig + (size_t)blockIdx.z * G * G + (size_t)j * G + i;
  if (!Q.status) { *dst = 0; return; }      // an invalid quad: no signature (a row of zeros, so that its dots are zeros; its record says status 0)
  const int pw = G * m;
  int sum = 0;
  for (int dj = 0; dj < m; dj++)
    for (int di = 0; di < m; di++) {
      uint8_t o[3];
      patch_pixel<FMT>(S, Q, i * m + di, j * m + dj, pw, pw, o);
      sum += (29 * o[0] + 150 * o[1] + 77 * o[2] + 128) >> 8;
    }
  const int mm = m * m, sh = m == 1 ? 0 : (m == 2 ? 2 : 4);
  const int a = ((sum + mm / 2) >> sh) - 128;
  *dst = (int8_t)a;
  int sa = a, saa = a * a;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { sa += __shfl_xor(sa, d, 64); saa += __shfl_xor(saa, d, 64); }
  if (threadIdx.x == 0 && threadIdx.y == 0) { atomicAdd(&sums[2 * blockIdx.z], sa); atomicAdd(&sums[2 * blockIdx.z + 1], saa); }
}

typedef int v4i __attribute__((ext_vector_type(4)));

// dots[(16 by + 4 (l >> 4) + r) * ld + 16 bx + (l & 15)] = sum over k of A[16 by + ..][k] * B[16 bx + ..][k]; A, B: rows of D bytes, both padded to 16 rows
__global__ __launch_bounds__(64) void k_match_dots(int *dots, const int8_t *A, const int8_t *B, int D, int ld) {
  const int l = threadIdx.x, rc = l & 15, kq = l >> 4;
  const int8_t *a = A + ((size_t)blockIdx.y * 16 + rc) * D + kq * 16;
  const int8_t *b = B + ((size_t)blockIdx.x * 16 + rc) * D + kq * 16;
  v4i acc = { 0, 0, 0, 0 };
  for (int k = 0; k < D; k += 64) {
    const v4i av = *(const v4i *)(a + k), bv = *(const v4i *)(b + k);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc, 0, 0, 0);
  }
  int *o = dots + ((size_t)blockIdx.y * 16 + kq * 4) * ld + (size_t)blockIdx.x * 16 + rc;
#pragma unroll
  for (int r = 0; r < 4; r++) o[(size_t)r * ld] = acc[r];
}

// the greater key, the lower column among equal keys (col < 0: none yet)
__device__ __forceinline__ void better(double &key, int &col, double k2, int c2) {
  if (c2 >= 0 && (col < 0 || k2 > key || (k2 == key && c2 < col))) { key = k2; col = c2; }
}
__device__ __forceinline__ void wave_best(double &key, int &col) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double k2 = __shfl_xor(key, d, 64);
    const int c2 = __shfl_xor(col, d, 64);
    better(key, col, k2, c2);
  }
}

// one wave per quad: its record without the scores.  colsums: sb, sbb per column; ncols = 4 T
__global__ __launch_bounds__(64) void k_match_pick(rd_match *recs, const int *dots, int ld, const int *colsums, int ncols, const int *sums, const rdk::RectifyQuad *quads, int D) {
  const int q = blockIdx.x, l = threadIdx.x;
  const int *row = dots + (size_t)q * ld;
  const long long sa = sums[2 * q], saa = sums[2 * q + 1];
  const long long va = (long long)D * saa - sa * sa;
  const int status = !quads[q].status ? 0 : (ncols == 0 ? 3 : (va == 0 ? 2 : 1));
  rd_match R;
  R.status = status; R.tmpl = R.rot = R.dot = R.tmpl2 = R.rot2 = R.dot2 = R.sa = 0; R.saa = 0; R.score = R.score2 = 0.0;
  if (status == 1) {
    int col = -1, col2 = -1;
    for (int pass = 0; pass < 2; pass++) {
      double bk = 0.0;
      int bc = -1;
      for (int c = l; c < ncols; c += 64) {
        if (pass == 1 && (c >> 2) == (col >> 2)) continue;
        const long long sb = colsums[2 * c], sbb = colsums[2 * c + 1];
        const long long num = (long long)D * row[c] - sa * sb, vb = (long long)D * sbb - sb * sb;
        const double n = (double)num;
        better(bk, bc, (n * fabs(n)) / (double)vb, c);
      }
      wave_best(bk, bc);
      if (pass == 0) col = bc; else col2 = bc;
    }
    R.tmpl = col >> 2; R.rot = col & 3; R.dot = row[col];
    if (col2 >= 0) { R.tmpl2 = col2 >> 2; R.rot2 = col2 & 3; R.dot2 = row[col2]; } else R.tmpl2 = -1;
    R.sa = (int)sa; R.saa = saa;
  }
  if (l == 0) recs[q] = R;
}

// columns 0..3 of a template at lib from its signature S (D = G * G bytes): column r is rot applied r times, rot(S)[j][i] = S[G-1-i][j]
__global__ void k_match_rotations(int8_t *lib, const int8_t *S, int G) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, D = G * G;
  if (p >= D) return;
  int row = p / G, col = p - row * G;      // (row, col) of the cell of S that output cell p of column r takes
  for (int r = 0; r < 4; r++) {
    lib[(size_t)r * D + p] = S[row * G + col];
    const int nr = G - 1 - col, nc = row;      // one more turn: the source of (row, col) under rot is (G-1-col, row)
    row = nr; col = nc;
  }
}

}  // namespace

namespace rdk {

void match_signatures(hipStream_t s, int8_t *sig, int *sums, int fmt, const PixFrame &S, const RectifyQuad *quads, int n, int G, int m) {
  if (n <= 0) return;
  const dim3 block(8, 8), grid(G / 8, G / 8, n);
  if (!dispatch(fmt, [&](auto f) { hipLaunchKernelGGL(k_signature<f.value>, grid, block, 0, s, sig, sums, S, quads, G, m); })) {
    fprintf(stderr, "rdk::match_signatures: unknown pixel format %d\n", fmt); abort();      // (the entry points refuse it first)
  }
}

void match_dots(hipStream_t s, int *dots, int ld, const int8_t *sig, int n, const int8_t *lib, int ncols, int D) {
  if (n <= 0 || ncols <= 0) return;
  hipLaunchKernelGGL(k_match_dots, dim3((ncols + 15) / 16, (n + 15) / 16), dim3(64), 0, s, dots, sig, lib, D, ld);
}

void match_pick(hipStream_t s, rd_match *recs, const int *dots, int ld, const int *colsums, int ncols, const int *sums, const RectifyQuad *quads, int n, int D) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_match_pick, dim3(n), dim3(64), 0, s, recs, dots, ld, colsums, ncols, sums, quads, D);
}

void match_rotations(hipStream_t s, int8_t *lib4, const int8_t *sig, int G) {
  hipLaunchKernelGGL(k_match_rotations, dim3((G * G + 255) / 256), dim3(256), 0, s, lib4, sig, G);
}

}  // namespace rdk
