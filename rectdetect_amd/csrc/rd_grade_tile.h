/* rectdetect-mi355x: graded quads - what the kernel (rd_k_grade.hip) and the host's rd_grade_limits (rd_grade_host.c) must agree on.  Plain C. */
#ifndef RD_GRADE_TILE_H_INCLUDED
#define RD_GRADE_TILE_H_INCLUDED

#define RD_GRADE_MAX_CELLS 8
#define RD_GRADE_MAX_EDGE 1020 /* 4 * 255: the largest |L| */
#define RD_GRADE_TILE_W 64     /* pixels of a block: one wave row is 64 consecutive pixels, as in rd_scan_tile.h - the two kernels run on the same grid */
#define RD_GRADE_TILE_H 16     /* four waves, four rows each */

#endif
