/*
 * A read-only counter of the PROFILING build of the engine (jubjub_schnorr_amd/libjjs_gpu_prof.so); the product library
 * libjjs_gpu.so does not export it.  It sits beside include/jjs_gpu_profiling.h, whose entry points all change what the
 * engine does: this one changes nothing.
 */
#ifndef JJS_GPU_KEY_MEMO_H
#define JJS_GPU_KEY_MEMO_H

#include "jjs_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The key-table calls that have ended on the current device, summed: out[0] = distinct keys found in their slot's memo of
 * the previous call (no validity test, no chain, no tables), out[1] = distinct keys built.  Like jjs_path_stats it counts a
 * call when the library next looks at its slot: after the stream has drained, every finished call is in. */
int jjs_debug_key_memo_stats(uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* JJS_GPU_KEY_MEMO_H */
