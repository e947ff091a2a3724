/* rectdetect-mi355x: decoded quads - what the kernel (rd_k_code.hip), the rectifier (rd_rectify.hip) and the host's helpers (rd_code_host.c) must agree on.  Plain C. */
#ifndef RD_CODE_TILE_H_INCLUDED
#define RD_CODE_TILE_H_INCLUDED

#define RD_CODE_MIN_N 3
#define RD_CODE_MAX_N 8          /* a payload is one 64-bit word, one bit per lane of a wave */
#define RD_CODE_MAX_BORDER 2
#define RD_CODE_MAX_INSET 3      /* eighths of a cell ignored on every side */
#define RD_CODE_MAX_SIDE 1024    /* pw, ph: a cell then holds at most 205 x 205 pixels and 256 * sg fits uint32 */
#define RD_CODE_MAX_DICT 4096    /* an id is 12 bits of the search's packed key */
#define RD_CODE_MAX_CELLS 144    /* (8 + 2 * 2)^2 */
#define RD_CODE_WAVES 16         /* waves of the kernel's block: 64 * RD_CODE_WAVES threads stride over the dictionary, so entry id is thread id % 1024's (the tests place codes on both sides of that stride) */
#define RD_CODE_PLANE_PAD 16    /* the kernel reads the G planes as 16-byte words: the planes start on such a boundary and that many bytes behind the last one are readable */
#define RD_CODE_NONE 65         /* a distance no code has: hamming and second without a dictionary entry to measure */

#endif
