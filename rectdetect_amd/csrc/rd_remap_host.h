/* rectdetect-mi355x: remapped frames - what the host computes once per remapper (the contract: include/rectdetect_hip.h, "remapped frames").  Plain C, no HIP:
 * rd_remap_host.c is built into the library with the host compiler, and tests/native/remap_host_check.c builds it on its own under the sanitizers. */
#ifndef RD_REMAP_HOST_H
#define RD_REMAP_HOST_H
#include <stdint.h>
#if defined(__cplusplus)
extern "C" {
#endif

enum { RD_REMAP_MAX_OUT = 16384, RD_REMAP_MAX_SRC = 65536 };      /* the largest side of an output and of a source: an 8.8 coordinate of the source fits an int32 */

/* are the sizes of a table legal?  (the first of the argument checks of rd_remap_table_lens / _map: the service asks before it allocates the table) */
int rd_remap_sizes_ok(int ow, int oh, int iw, int ih);

#if defined(__cplusplus)
}
#endif
#endif
