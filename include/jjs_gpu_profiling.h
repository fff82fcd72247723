/*
 * Extra entry points of the PROFILING build of the engine (jubjub_schnorr_amd/libjjs_gpu_prof.so, compiled from
 * the same sources with -DJJS_PROFILING).  They switch verification work off or let several logical devices share
 * one card, so they are compiled OUT of the product library libjjs_gpu.so (tests/test_abi.py checks that the
 * symbols are absent there).  Used only by the tools under jubjub_schnorr_amd/tools/ and by the child processes of the GPU tests.
 */
#ifndef JJS_GPU_PROFILING_H
#define JJS_GPU_PROFILING_H

#include "jjs_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ablations (results become meaningless): skip phases of the verify kernels in later launches; bit0 = point
 * validity, bit1 = challenge hash, bit2 = equations, bit3 = Euclid (stand-in scalars), bit4 = every window / comb
 * lookup of the throughput path, and every comb lookup of the key-table path, reads from a cache-resident subset of
 * its table (what the gathers cost); 0 restores the full path. */
int jjs_debug_skip_phases(unsigned mask);
/* Path selection for A/B timing (results stay exact): 0 = by batch size and key repetition (product behaviour),
 * 1 = never the latency path, 3 = never the latency path and never the key tables (every key a fresh variable
 * point), 2 = the latency path for every single / double call of at most 16 384 items; 0x42 / 0x82 = the
 * latency path with the scalars cut into 4 / 8 pieces whatever the size; 0x500 = 5-bit windows whenever the key
 * tables engage (the product takes 6-bit windows from 128 signatures per key); 0x1000 = the key-table path takes the
 * items in the caller's order instead of grouping them by key, and so does the share pass of jjs_msig_group_combine_dev
 * instead of running a wave over the transcripts of one participant; for jjs_verify_all_*: 0x2000 = the verdict algorithm at
 * any size, 0x4000 = the per-item path and its tally at any size, plus (w << 16) = the MSM's window width w (8-16; 0 by
 * size); for jjs_sign_vargen_pt* with one generator for the call: 0x8000 = the shared-generator route at any n,
 * 0x200000 = the per-item route at any n; for jjs_sign_fixed* with one key for the call (n_sk == 1): 0x400000 = the keyed
 * route at any n, 0x800000 = the per-item route at any n; for jjs_digest*: 0x1000000 = eight lanes per item at any n,
 * 0x2000000 = one lane per item at any n, 0x4000000 = the lanes of a ragged call take the items in input order. */
int jjs_debug_force_path(int which);
/* Test mode for boxes with one GPU: a later jjs_init(k) with k above the visible device count creates k logical
 * devices (own stream, tables, workspace, staging each) that share the visible cards round-robin; the tallies are
 * then summed on the host, since two ranks on one card cannot form an RCCL clique. */
int jjs_debug_allow_virtual_devices(int allow);
/* on != 0: the next calls find that the pool of the per-key tables "cannot be allocated" (the branch a device short of
 * memory takes): they run the throughput path; 0 restores the product behaviour. */
int jjs_debug_fail_key_arena(int on);
/* on != 0: the dedup hash of the key tables runs with seed 0 instead of a fresh seed per call, so that a test can
 * present keys crafted to collide in it (what the seed keeps a sender from doing).  on & 2, in addition: jjs_verify_all_*
 * draw their weights from the fixed ChaCha20 key 00 01 02 .. 1f instead of 32 fresh bytes of getrandom per call, so that
 * tests and A/B runs repeat. */
int jjs_debug_pin_hash_seed(int on);
/* Where the last host-buffer call on one device spent its host time, in seconds: out[0] waiting for the staging copy
 * of a piece to finish (it runs one piece ahead on helper threads), out[1] starting the next one (includes waiting for
 * its pinned slot), out[2] the whole block, out[3] pieces, out[4] from the entry to the first upload being queued,
 * out[5] until everything was queued, out[6] waiting for the device to drain after that, out[7] copying the statuses
 * out. */
int jjs_debug_host_timing(double out[8]);
/* The bucket MSM of jjs_verify_all_* over the caller's own terms, every stage's output copied out (tests/test_msm_gpu.py).
 * points: n_kinds * n affine points (64 bytes, canonical); scalars: as many, 32 bytes each, below 2^252 (short_shape != 0:
 * within msm_weight_bits(c) bits); term t is negated when bit t / n of neg_kinds is set; c: the window width, 8 .. 16.
 * The call carves the slot's verdict scratch, stores the terms, clears what a verdict call clears and runs the call's own
 * MSM launches.  off_out: W * B + 1 words, the buckets' offsets; order_out: room for n_kinds * n * W words, of which
 * off[W * B] are written, the sorted entries (term, bit 31: negated); win_out: W extended points (X, Y, Z, T of 9 limbs
 * each, Montgomery form); total_out: one extended point, the windows combined.  Device pointers, 16-byte aligned;
 * asynchronous on `stream`. */
int jjs_debug_msm_dev(const void* points, const void* scalars, size_t n, unsigned n_kinds, unsigned neg_kinds, int c, int short_shape,
                      void* off_out, void* order_out, void* win_out, void* total_out, void* stream);
/* The run sums and key points of jjs_keyset_verify_all* under the caller's own scalar columns: the call's grouping of the
 * items by key, then its run and key kernels.  key_idx: n indices inside the set; a0, a1: n x 32 bytes, every value below r,
 * the items' scalars on point column 0 / 1 (a1 is not read for a set with one point column).  sums_out: S_k of every
 * (point column, key), 32 bytes each, column 0 first; point_out: one extended point, the sum of S_k * P_k over both
 * columns.  Device pointers, 16-byte aligned; asynchronous on `stream`. */
int jjs_debug_keyset_sums_dev(jjs_keyset ks, const void* key_idx, const void* a0, const void* a1, size_t n, void* sums_out, void* point_out,
                              void* stream);
/* The per-item pass of jjs_verify_all_* with what it wrote copied out (tests/test_fr_gpu.py): the descriptor, scratch, clear
 * and item kernel exactly as a verdict call runs them, the weights drawn under the call's seed (jjs_debug_pin_hash_seed(2)
 * fixes it) with the bits of window width c (8 .. 16).  d0 .. d5: the scheme's affine columns in the order of
 * jjs_verify_all_*_dev (the unused ones null).  blocks: the item kernel's grid, 0 = the call's own (at most ceil(n / 256)).
 * scalars_out: n_kinds * n scalars of 32 bytes, kind k's at k * n (single: z on R, z c on PK; double: the same for the second
 * equation behind them; per-item generator: z on R, z c on PK, z u on Gen); partial_out: 64 bytes per block, its sum of z u
 * and of z' u mod r; fail_out: the fail word; zu_out: 64 bytes, the two totals as the final kernel adds the partial sums up.
 * *blocks_out (host) is the grid that ran, written before the call returns.  Device pointers, 16-byte aligned; asynchronous
 * on `stream`. */
int jjs_debug_verdict_items_dev(int scheme, const void* d0, const void* d1, const void* d2, const void* d3, const void* d4, const void* d5,
                                size_t n, int c, unsigned blocks, void* scalars_out, void* partial_out, void* fail_out, void* zu_out,
                                unsigned* blocks_out, void* stream);
/* The same for jjs_keyset_verify_all* (affine signatures): the grouping by key and the keyed item kernel as a verdict call
 * runs them.  scalars_out: n_eq * n weights on R (and R'); a0_out, a1_out: n x 32 bytes, the items' scalars on point column 0 / 1
 * of their key (a1_out is not written for a set with one point column); the rest as above. */
int jjs_debug_keyset_items_dev(jjs_keyset ks, const void* key_idx, const void* u, const void* R, const void* Rp, const void* m, size_t n, int c,
                               unsigned blocks, void* scalars_out, void* a0_out, void* a1_out, void* partial_out, void* fail_out, void* zu_out,
                               unsigned* blocks_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JJS_GPU_PROFILING_H */
