// rectdetect-mi355x: the lane -> element map of v_mfma_i32_16x16x64_i8 on gfx950, MEASURED with one-hot data - what rd_k_match.hip (k_match_dots) relies on and
// DESIGN.md ("Matched quads") records.  Not part of the library:
//   hipcc --offload-arch=gfx950 -O2 tools/mfma_i8_map.hip -o mfma_i8_map && ./mfma_i8_map
// Three experiments, each one MFMA per case on a single wave:
//   rows:    A = ones in ONE lane, B = ones everywhere      -> which (lane, register) of D is non-zero: the row of A that lane holds, and the C/D map
//   columns: B = ones in ONE lane, A = ones everywhere      -> the column of B that lane holds
//   k:       A = one byte (lane group g, byte j) of row 0, B = one byte (g', j') of column 0 -> D[0][0] = 1 exactly when the two bytes meet at the same k
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef int v4i __attribute__((ext_vector_type(4)));

__global__ void k_probe(int *d, const int8_t *a, const int8_t *b, int cases) {
  const int l = threadIdx.x;
  for (int c = 0; c < cases; c++) {
    const v4i av = *(const v4i *)(a + ((size_t)c * 64 + l) * 16), bv = *(const v4i *)(b + ((size_t)c * 64 + l) * 16);
    v4i acc = { 0, 0, 0, 0 };
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) d[((size_t)c * 64 + l) * 4 + r] = acc[r];
  }
}

#define OK(e) do { hipError_t s_ = (e); if (s_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(s_)); return 1; } } while (0)

static int run(const int8_t *a, const int8_t *b, int *d, int cases) {
  int8_t *da, *db; int *dd;
  const size_t nb = (size_t)cases * 64 * 16;
  OK(hipMalloc((void **)&da, nb)); OK(hipMalloc((void **)&db, nb)); OK(hipMalloc((void **)&dd, nb));
  OK(hipMemcpy(da, a, nb, hipMemcpyHostToDevice)); OK(hipMemcpy(db, b, nb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, dd, da, db, cases);
  OK(hipDeviceSynchronize());
  OK(hipMemcpy(d, dd, nb, hipMemcpyDeviceToHost));
  OK(hipFree(da)); OK(hipFree(db)); OK(hipFree(dd));
  return 0;
}

int main(void) {
  enum { N = 64 * 64 };
  static int8_t a[N * 64 * 16], b[N * 64 * 16];
  static int d[N * 64 * 4];
  int bad = 0;
  // rows and columns: case c < 64 lights lane c of A, case 64 + c lane c of B
  memset(a, 0, sizeof(a)); memset(b, 0, sizeof(b));
  for (int c = 0; c < 64; c++) {
    memset(a + ((size_t)c * 64 + c) * 16, 1, 16); memset(b + (size_t)c * 64 * 16, 1, 64 * 16);
    memset(b + ((size_t)(64 + c) * 64 + c) * 16, 1, 16); memset(a + (size_t)(64 + c) * 64 * 16, 1, 64 * 16);
  }
  if (run(a, b, d, 128)) return 1;
  // expected: A lane l is row l & 15, B lane l is column l & 15, D (lane, reg) is row 4 * (lane >> 4) + reg, column lane & 15; a lit lane adds its 16 bytes
  for (int c = 0; c < 128; c++)
    for (int l = 0; l < 64; l++)
      for (int r = 0; r < 4; r++) {
        const int row = 4 * (l >> 4) + r, col = l & 15, lit = c & 63;
        const int want = c < 64 ? (row == (lit & 15) ? 16 : 0) : (col == (lit & 15) ? 16 : 0);
        if (d[((size_t)c * 64 + l) * 4 + r] != want) { if (bad++ < 8) printf("case %d lane %d reg %d: %d, expected %d\n", c, l, r, d[((size_t)c * 64 + l) * 4 + r], want); }
      }
  printf("A: lane l holds row l & 15; B: lane l holds column l & 15; C/D: lane l, register r is row 4 * (l >> 4) + r, column l & 15: %s\n", bad ? "NOT what was measured" : "measured");
  // k: byte (g, j) of A's row 0 against byte (g', j') of B's column 0
  memset(a, 0, sizeof(a)); memset(b, 0, sizeof(b));
  for (int p = 0; p < 64; p++)
    for (int q = 0; q < 64; q++) {
      const size_t c = (size_t)p * 64 + q;
      a[(c * 64 + 16 * (p >> 4)) * 16 + (p & 15)] = 3;
      b[(c * 64 + 16 * (q >> 4)) * 16 + (q & 15)] = 5;
    }
  if (run(a, b, d, N)) return 1;
  int kbad = 0;
  for (int p = 0; p < 64; p++)
    for (int q = 0; q < 64; q++) {
      const size_t c = (size_t)p * 64 + q;
      for (int l = 0; l < 64; l++)
        for (int r = 0; r < 4; r++) {
          const int want = (l == 0 && r == 0 && p == q) ? 15 : 0;
          if (d[(c * 64 + l) * 4 + r] != want) { if (kbad++ < 8) printf("k case A byte %d, B byte %d, lane %d reg %d: %d, expected %d\n", p, q, l, r, d[(c * 64 + l) * 4 + r], want); }
        }
    }
  printf("k: byte j of lane group g of A meets byte j' of lane group g' of B exactly when g == g' and j == j' (64 x 64 pairs): %s\n", kbad ? "NOT what was measured" : "measured");
  return bad || kbad ? 1 : 0;
}
