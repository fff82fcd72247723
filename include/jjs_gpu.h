/*
 * libjjs_gpu -- batch Schnorr-on-JubJub verification on AMD MI355X (gfx950).
 *
 * C ABI that a host-language shim binds (Rust `extern "C"`, ctypes, ...).  It is the batch
 * drop-in for the `verify` hot path of dusk-network/jubjub-schnorr:
 *
 *   jjs_verify_single*  <->  PublicKey::verify        reference src/keys/public.rs:114-135
 *   jjs_verify_double*  <->  PublicKeyDouble::verify  reference src/keys/public/double.rs:86-117
 *   jjs_verify_vargen*  <->  PublicKeyVarGen::verify  reference src/keys/public/var_gen.rs:107-133
 *   status codes        <->  Result<(), Error>        reference src/error.rs:13-19
 *   jjs_challenge_*     <->  challenge_hash           reference src/signatures.rs:122-140,
 *                             src/signatures/double.rs:151-177, src/signatures/var_gen.rs:121-142
 *   jjs_sign_*          <->  SecretKey::sign & co.    reference src/keys/secret.rs:174-194,
 *                             src/keys/secret/double.rs:56-85, src/keys/secret/var_gen.rs:228-256
 *                             (test-vector / benchmark-input generator: NOT constant time)
 *
 * Data layout (all entry points): structure of arrays, item i of an array at offset i*size.
 *   field element / scalar : 32 bytes, little-endian, canonical (BlsScalar::to_bytes,
 *                            JubJubScalar::to_bytes)
 *   point                  : 64 bytes = affine u || v, each 32 bytes little-endian canonical
 *                            (what JubJubExtended::to_hash_inputs() returns, reference
 *                            src/signatures.rs:127-128)
 * Every buffer must be 16-byte aligned.
 *
 * status[i]: 0 = Ok, 1 = InvalidPoint, 2 = InvalidSignature (reference src/error.rs:17-19 with the
 * precedence of src/keys/public.rs:119-132), 3 = Malformed (a coordinate or message >= q, or
 * u >= r: unreachable through the Rust types, defined so that this ABI is total).
 * tally[k] = number of items with status k.
 *
 * Return value: 0 = success; negative = engine error, in which case outputs are unspecified:
 *   -1 bad argument, -2 HIP error, -3 collective (RCCL) error, -4 not initialised.
 * No exceptions, no aborts.  jjs_last_error() describes the last failure of the calling THREAD (the
 * buffer is thread-local: the pointer stays valid and is only rewritten by later failures of the same thread).
 *
 * Ownership: the caller owns every buffer passed in; the library keeps nothing after a blocking
 * call returns (after the stream has drained, for the *_dev calls).  The library owns its device
 * tables, workspaces, streams and RCCL communicators between jjs_init and jjs_shutdown.
 *
 * There are no switches, environment variables or hidden entry points that turn a check off: the profiling
 * ablations and the logical-device test mode live in a separate build (libjjs_gpu_prof.so, -DJJS_PROFILING,
 * include/jjs_gpu_profiling.h) that the product never loads.
 *
 * Threading: jjs_init / jjs_shutdown are not re-entrant.  All other calls may come from any host
 * thread.  One internal mutex guards the engine's state; it is held while a call is QUEUED, never while a call waits:
 * the *_dev calls are asynchronous, jjs_stream_sync waits outside it, and a blocking host-buffer call holds it only while
 * its launches are queued.  Host-buffer calls of at most 16 384 items run on staging lanes (eight per device), side by side
 * on the device; those of at most 4 096 items of one scheme and input format that arrive while another is running share
 * one launch (JJS_PATH_LANE_LAUNCHES / JJS_PATH_LANE_CALLS count them): four threads of 1 024-signature calls complete
 * about three times the calls per second of one thread, eight threads four times; 64 threads of ONE-signature calls about thirty
 * times (the callers of a shared launch other than the one that drives it sleep, so a service may have many more threads than
 * cores).  Larger host-buffer calls are pipelines of
 * uploads and launches that fill the device: they run one at a time per device (other threads' calls are queued meanwhile;
 * with several driven devices such a call holds the mutex for its duration).  A call takes one of the engine's call slots by size (six for calls of
 * at most 16 384 items, three for at most 131 072, two for larger ones): calls in different slots share no buffer and
 * overlap on the device when they are issued on different streams; calls in one slot are ordered on the device (each
 * waits for the previous one, also across streams).
 *
 * Method: the engine picks, per call, from the batch size and the repetition of its keys alone (no configuration):
 * at most 16 384 items -> latency path (a signature spread over many lanes: 0.37 ms single, 0.50 ms double, 0.41-0.47 ms
 * var-generator for a call of a few hundred items, 0.55 / 0.71 / 0.85 ms at 4 096); larger -> one signature per lane; at least 65 536 items (32 768 for double
 * and var-generator signatures) whose public keys (and per-item generators) repeat 16 times or more on average ->
 * per-key tables built inside the call.  The
 * status bytes are the same on every path.
 */
#ifndef JJS_GPU_H
#define JJS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JJS_OK 0
#define JJS_ERR_ARG (-1)
#define JJS_ERR_HIP (-2)
#define JJS_ERR_COLLECTIVE (-3)
#define JJS_ERR_NOT_INIT (-4)

#define JJS_STATUS_OK 0
#define JJS_STATUS_INVALID_POINT 1
#define JJS_STATUS_INVALID_SIGNATURE 2
#define JJS_STATUS_MALFORMED 3

/* Sets up the devices this process drives: builds the fixed-base tables for G and G' on each, allocates
 * the per-lane workspaces and one stream per device.
 *   device_count == 1 : the calling thread's current HIP device only (one process per GPU: what a
 *                       torch.distributed / torchrun rank uses);
 *   device_count == k : HIP devices 0 .. k-1 in this one process (2 <= k <= 16);
 *   device_count == 0 : every visible HIP device.
 * With several devices the host-buffer calls below cut each batch into one contiguous block of
 * ceil(n / devices) items per device, run the blocks concurrently and sum the four tally counters with
 * one RCCL all-reduce (4 x u64, the only collective; RCCL is loaded on demand and not at all for one
 * device).  The *_dev calls always act on the calling thread's current device, which must be one of the
 * devices set up here.  Idempotent for a repeated identical request. */
int jjs_init(int device_count);
void jjs_shutdown(void);
/* Number of devices the process drives (0 before jjs_init). */
int jjs_device_count(void);
/* Ranks of the in-library RCCL clique that sums the tallies of the host-buffer calls: the number of devices when
 * jjs_init set up more than one (real) device, else 0 (one device: nothing to sum). */
int jjs_collective_ranks(void);
const char* jjs_last_error(void);
/* ABI version: bumped on any signature change. */
int jjs_abi_version(void);

/* ---- host buffers, blocking: copy in, verify, copy out -------------------------------------- */
int jjs_verify_single(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* m, size_t n,
                      uint8_t* status, uint64_t tally[4]);
int jjs_verify_double(const uint8_t* u, const uint8_t* R, const uint8_t* R_prime, const uint8_t* PK,
                      const uint8_t* PK_prime, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
int jjs_verify_vargen(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* Gen, const uint8_t* m,
                      size_t n, uint8_t* status, uint64_t tally[4]);

/* ---- device buffers (resident data), asynchronous on `stream` ------------------------------------
 * All pointers are device pointers on the engine's device.  `status` (n bytes) and `tally`
 * (4 x uint64, zeroed by the call) may each be NULL.  `stream` is a hipStream_t passed as void*
 * (NULL = the device's default stream, as in HIP).  The call enqueues and returns; use jjs_stream_sync or any
 * HIP synchronisation on that stream before reading the outputs. */
int jjs_verify_single_dev(const void* u, const void* R, const void* PK, const void* m, size_t n, void* status,
                          void* tally, void* stream);
int jjs_verify_double_dev(const void* u, const void* R, const void* R_prime, const void* PK, const void* PK_prime,
                          const void* m, size_t n, void* status, void* tally, void* stream);
int jjs_verify_vargen_dev(const void* u, const void* R, const void* PK, const void* Gen, const void* m, size_t n,
                          void* status, void* tally, void* stream);
int jjs_stream_sync(void* stream);

/* Which method the calls on the calling thread's device took since jjs_init (the engine chooses per call; see "Method"
 * above): out[k] = number of calls, k one of the JJS_PATH_* indices; out[JJS_PATH_KEY_POOL_BYTES] = device memory the
 * per-key tables hold right now.  A call that tried the key tables is counted under what the device decided for it
 * (WIDE / NARROW: tables with 6- / 5-bit windows; DO_NOT_REPEAT: fewer than 16 signatures per key on average;
 * PROBE_LIMIT: keys that collide in the dedup table; POOL_TOO_SMALL: the keys repeat but their tables did not fit -- the
 * pool has grown by the slot's next call; the last three ran the throughput path) once that call has finished; NO_MEMORY
 * counts allocations of the table pool that the device refused (those calls ran the throughput path, too).  So a caller
 * can see when its batches fall off the fast path.  Host-buffer calls count once per device block. */
#define JJS_PATH_LATENCY 0
#define JJS_PATH_THROUGHPUT 1
#define JJS_PATH_KEY_TABLES_WIDE 2
#define JJS_PATH_KEY_TABLES_NARROW 3
#define JJS_PATH_KEYS_DO_NOT_REPEAT 4
#define JJS_PATH_KEYS_PROBE_LIMIT 5
#define JJS_PATH_KEYS_POOL_TOO_SMALL 6
#define JJS_PATH_KEYS_NO_MEMORY 7
#define JJS_PATH_KEY_POOL_BYTES 8
/* blocking host-buffer calls of at most 131 072 items: launches on the staging lanes, and calls they served (calls of at
 * most 4 096 items of one scheme and format that arrive while such a launch runs share the next one) */
#define JJS_PATH_LANE_LAUNCHES 9
#define JJS_PATH_LANE_CALLS 10
#define JJS_PATH_STATS 11
int jjs_path_stats(uint64_t out[JJS_PATH_STATS]);

/* ---- pre-sizing, trimming -----------------------------------------------------------------------------------
 * The engine's buffers are grow-only and allocated on first use: the first call of a larger size than any before it
 * allocates (never waits for the device: a replaced buffer is kept until jjs_trim / jjs_shutdown), which costs that call
 * the allocation time.  A service that knows its call shapes pre-sizes at start-up:
 *   jjs_reserve(scheme, format, n_items, host_buffers) allocates what a verification call of that scheme (JJS_SCHEME_*),
 *   input format (JJS_FORMAT_*) and at most n_items items needs, in every call slot such a call can land in; with
 *   host_buffers != 0 also the staging of the blocking host-buffer entry point of that shape (for every driven device).
 *   A reserve may come from any thread at any time, also beside live calls of any kind; no call then sees a buffer replaced
 *   under it, and every call's statuses are what they would have been.  What such a reserve guarantees:
 *     - it never waits for the device and frees nothing (what it replaces is kept until jjs_trim / jjs_shutdown);
 *     - a staging lane of the small host-buffer calls (at most 16 384 items) that is in use when the reserve comes keeps its
 *       areas and grows to the reserved size when it is next opened, by the call that opens it: after a reserve beside live
 *       host-buffer calls up to eight later calls, one per lane that was busy, may still allocate.  Lanes that were idle,
 *       and so every lane of a reserve at start-up, hold the size when the reserve returns;
 *     - a reserve of more than 16 384 items sizes what a large host-buffer call (more than 16 384 items, one driven device) uses
 *       while it runs; it waits for such a call in progress to return, as jjs_trim does, and the next one starts behind it.
 *       Resident calls and small host-buffer calls of other threads go on meanwhile.
 * jjs_trim() waits for the devices to go idle and frees the retired buffers and the key-table pools (which come back,
 * at the size they had, with the next call that takes the key tables).  jjs_memory_stats: bytes held, by kind. */
#define JJS_SCHEME_SINGLE 0
#define JJS_SCHEME_DOUBLE 1
#define JJS_SCHEME_VARGEN 2
#define JJS_FORMAT_AFFINE 0
#define JJS_FORMAT_EXT 1
#define JJS_FORMAT_WIRE 2
int jjs_reserve(int scheme, int format, size_t n_items, int host_buffers);
int jjs_trim(void);
#define JJS_MEMORY_KEY_POOLS 0
#define JJS_MEMORY_SLOT_BUFFERS 1
#define JJS_MEMORY_HOST_STAGING 2
#define JJS_MEMORY_RETIRED 3
#define JJS_MEMORY_STATS 4
int jjs_memory_stats(uint64_t out[JJS_MEMORY_STATS]);

/* ---- registered key sets ----------------------------------------------------------------------------------
 * Callers that know their keys ahead of time (a validator set, a wallet's accounts, the signers of a contract) register
 * them once and then verify against them by index: each key is decoded or normalised, gets its `is_valid` test and its
 * window tables {0 .. 2^(w-1)} * 2^(w i) * PK (w = 6) on every driven device, once; a call then carries a 4-byte index per
 * item instead of the key, and no per-call dedup, chains or tables run, whatever the call's size and however often its keys
 * repeat within it (measured against the inline calls: profiles/r05_keyset.jsonl).
 *   jjs_keyset_create(scheme, format, keys, keys2, n_keys, key_status, out): scheme JJS_SCHEME_*, key format JJS_FORMAT_*.
 *     The set holds the public-key type of its scheme: PublicKey, PublicKeyDouble (pk, pk') or PublicKeyVarGen (pk, generator).
 *     Affine / extended keys: keys = the first point column (n x 64 / n x 96), keys2 = the second (NULL for single).  Wire
 *     keys: keys = the layout of the _wire calls (n x 32 single, n x 64 pk || pk' or pk || generator), keys2 = NULL.  The
 *     bytes are copied.  key_status[k] (nullable): 0 valid, 1 not `is_valid` (extended Z = 0 included), 3 a non-canonical
 *     coordinate or an encoding that does not decode; the worse of the two points wins.  Invalid keys stay registered.
 *     Blocking: the set is built before the call returns, outside the engine's mutex and on streams of its own (other
 *     threads' calls go on meanwhile); it is published under the mutex once every device's copy is complete.
 *   jjs_keyset_verify(_dev)(ks, format, key_idx, s0, s1, s2, m, n, ...): signature columns by format: affine s0 = u (n x 32),
 *     s1 = R (n x 64), s2 = R' (double only); ext s0 = u, s1 = R (n x 96), s2 = R'; wire s0 = sig (n x 64, n x 96 double),
 *     s1 = s2 = NULL.  key_idx: n x uint32.  The status of an item is the one the inline entry point of the signature's
 *     format returns for it given the registered key as its affine point, combined with key_status[key_idx[i]] (Malformed >
 *     InvalidPoint > InvalidSignature); key_idx[i] >= n_keys gives 3 (checked on the device).  _dev: device pointers
 *     (key_idx 4-byte, the others 16-byte aligned), asynchronous on `stream`, like the other _dev calls.  Host buffers: blocking,
 *     on the calling thread's current device, one such call at a time per device (they share the device's staging and
 *     its large host-call lock): the columns are uploaded whole, then verified, with no overlap of uploads and work and no
 *     combining of several threads' small calls.  profiles/r05_keyset.jsonl measures what that costs: a 2^20-item host call
 *     1.16x the inline one, eight threads of 64-signature calls 0.29x the inline rate.
 *     Calls of at most 16 384 items take the latency variant (eight hash lanes per item and the R points' subgroup tests
 *     beside them, then 4-16 lanes per equation over the tables); larger ones group the items by key (a cursor per key of
 *     the SET is cleared and scanned by every large call, and every slot's index buffer holds one: a per-call cost that
 *     grows with the set, not with the call) and take one lane per item.
 *   jjs_keyset_destroy(ks): the handle becomes stale (-1 from then on).  Launches already queued still read the set's
 *     device memory, which jjs_trim or jjs_shutdown frees; jjs_trim never frees a live set, jjs_shutdown frees every set.
 *   jjs_keyset_info(ks, out): JJS_KEYSET_* words below.
 * Memory per key on each device: 64 B + 1 B + 43 x 33 x 144 B = 204 KB per point column (twice that for double and var-gen),
 * and at most 65 B for the lookup table of the by-key calls below.
 * Threading: every keyset call may come from any thread; the registry is read and changed under the engine's mutex, which
 * no keyset call holds while it waits for the device.
 * Return codes: -4 before jjs_init; -1 for an unknown or destroyed handle, a bad scheme or format, a NULL column the
 * format needs or n_keys == 0; -2 when the set cannot be allocated (no partial set is left behind). */
typedef uint64_t jjs_keyset;                      /* 0 is never a valid handle */
#define JJS_KEYSET_SCHEME 0
#define JJS_KEYSET_KEYS 1
#define JJS_KEYSET_VALID_KEYS 2
#define JJS_KEYSET_WINDOW_BITS 3
#define JJS_KEYSET_DEVICE_BYTES 4                 /* per device */
#define JJS_KEYSET_SMALL_CALLS 5                  /* calls served by the latency variant */
#define JJS_KEYSET_LARGE_CALLS 6                  /* ... and by the large one */
#define JJS_KEYSET_INFO 7
int jjs_keyset_create(int scheme, int format, const uint8_t* keys, const uint8_t* keys2, size_t n_keys, uint8_t* key_status,
                      jjs_keyset* out);
int jjs_keyset_destroy(jjs_keyset ks);
int jjs_keyset_info(jjs_keyset ks, uint64_t out[JJS_KEYSET_INFO]);
int jjs_keyset_verify(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2,
                      const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
int jjs_keyset_verify_dev(jjs_keyset ks, int format, const void* key_idx, const void* s0, const void* s1, const void* s2,
                          const void* m, size_t n, void* status, void* tally, void* stream);

/* ---- registered key sets by key ------------------------------------------------------------------
 * The reference's `PublicKey::verify(&self, &Signature, BlsScalar)` arrives with a KEY, not an index.  Every set carries a
 * lookup table over its keys (built with the set, on every driven device: at most 64 B per key), and these calls take the
 * key columns of the inline call of the set's scheme in `format` where jjs_keyset_verify takes key_idx:
 *   affine / extended: K0 = PK, K1 = PK' (double) or Gen (var-gen), n x 64 / n x 96; K1 = NULL for single;
 *   wire:              K0 = the `pk` column of the _wire calls (n x 32, or n x 64 for the two-point schemes), K1 = NULL.
 * A key is FOUND when it is the point (pair of points) registered at some index: an affine query by equality of its 64 (128)
 * bytes with the set's canonical affine key, an extended one after normalisation (a point with U, V or Z >= q or Z = 0 is
 * found nowhere), a wire one by equality of its encoding with that of a registered key that is on the curve -- the result
 * of jjs_decompress_dev followed by the affine lookup.  Keys registered but not `is_valid` are found (their items get
 * status 1, as inline); a key registered as malformed (key_status 3) has no canonical bytes and is never found.  A key
 * registered at several indices is found at the LOWEST of them.
 *   jjs_keyset_find(_dev)(ks, format, K0, K1, n, idx_out): idx_out[i] = the index of item i's key, or 0xFFFFFFFF.  These are
 *     the indices jjs_keyset_verify*, jjs_keyset_verify_all* and the jjs_multisig_*_keyset* calls take: those calls have no
 *     by-key form of their own.  _dev: device pointers (K0, K1 16-byte, idx_out 4-byte aligned), asynchronous on `stream`.
 *   jjs_keyset_verify_keys_dev(ks, format, K0, K1, s0, s1, s2, m, n, status, tally, idx_out, stream): asynchronous; s0..s2, m,
 *     alignment and return codes of jjs_keyset_verify_dev; idx_out nullable (as jjs_keyset_find_dev).  An item whose key is
 *     found gets exactly the status of jjs_keyset_verify_dev with that index; one whose key is not gets
 *     JJS_STATUS_KEY_NOT_IN_SET and is counted in NO tally word (tally[0..3] sum to n minus the misses); no lane addresses
 *     the set for it.  The call counts under JJS_KEYSET_SMALL_CALLS / JJS_KEYSET_LARGE_CALLS as the by-index call does.
 *   jjs_keyset_verify_keys(...): from HOST buffers, blocking, on the route of jjs_keyset_verify (and with its cost against
 *     the inline host calls, see above).  A drop-in for the inline host call: status and tally are byte for byte those of
 *     jjs_verify_{single,double,vargen}{,_ext,_wire} on the same columns, for every item, whatever the set holds -- the items
 *     whose key is not in the set are gathered on the host and verified by that inline call once the by-key call has left
 *     the device's host-call lock.  idx_out (nullable) tells which items were found.  When every key is registered there is
 *     one device round trip and no inline call.
 * Cost: the by-index call plus the probe, one lane per item (and the normalisation of the key columns for extended keys).
 * Measured resident, by key against inline (profiles/r13_keyset_by_key.jsonl): 2^17 single signatures over
 * 2^15 keys 0.55x (affine), 0.60x (ext), 0.56x (wire); calls of 1 .. 16 384 items 0.80-0.94x single, 0.64-0.97x double,
 * 0.55-0.88x var-gen; against the by-index call a small call takes 2-10 us longer (two more launches).  2^20 items over
 * 4 096 keys LOSES to inline, 1.01x (inside the spread), as the by-index call does: the keys repeat within that call.
 * n == 0, stale handles, a NULL column the format needs and -4 before jjs_init: as jjs_keyset_verify(_dev). */
#define JJS_STATUS_KEY_NOT_IN_SET 6
int jjs_keyset_find_dev(jjs_keyset ks, int format, const void* K0, const void* K1, size_t n, void* idx_out, void* stream);
int jjs_keyset_find(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint32_t* idx_out);
int jjs_keyset_verify_keys_dev(jjs_keyset ks, int format, const void* K0, const void* K1, const void* s0, const void* s1,
                               const void* s2, const void* m, size_t n, void* status, void* tally, void* idx_out, void* stream);
int jjs_keyset_verify_keys(jjs_keyset ks, int format, const uint8_t* K0, const uint8_t* K1, const uint8_t* s0, const uint8_t* s1,
                           const uint8_t* s2, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4], uint32_t* idx_out);

/* ---- adding keys to a live key set ------------------------------------------------------------------
 * A validator set, a wallet's accounts and the signers of a contract gain keys over time.  jjs_keyset_add extends a set where
 * it stands: old indices never change, the old keys are neither decoded nor tabled again, and calls against the set go on
 * meanwhile -- they see the old set or the new one, never a mixture.
 *   jjs_keyset_add(ks, format, keys, keys2, n, mode, key_status, idx_out, n_added): keys, keys2 and format as
 *     jjs_keyset_create takes them for the set's scheme; host buffers; blocking.  key_status (n bytes), idx_out (n x uint32)
 *     and n_added are nullable.
 *     JJS_KEYSET_ADD_APPEND  candidate i is registered at index n_old + i whatever it is -- malformed keys, keys that are not
 *       `is_valid` and duplicates included, as jjs_keyset_create registers them.  idx_out[i] = n_old + i, *n_added = n,
 *       key_status as jjs_keyset_create writes it.  Afterwards the set is indistinguishable from jjs_keyset_create of the old
 *       keys followed by the new ones: every jjs_keyset_* and jjs_multisig_*_keyset* call gives the same bytes.
 *     JJS_KEYSET_ADD_UNIQUE  for sets populated from traffic: the caller need not know what the set holds.  A candidate with
 *       key_status 3 is not registered and gets idx_out[i] = 0xFFFFFFFF.  Any other candidate is compared by the canonical
 *       affine row(s) jjs_keyset_create would store for it: if jjs_keyset_find would find that row, idx_out[i] is that (lowest)
 *       index and nothing is registered (counted under JJS_KEYSET_ADD_KNOWN); otherwise the first occurrence in input order is
 *       registered at n_old + (the number of earlier first occurrences) and every later equal candidate gets the same index.
 *       Keys that are not `is_valid` are registered.  *n_added = the number of first occurrences; key_status[i] is the status
 *       of the key at idx_out[i] (3 for a candidate that was not registered).  The indices are a function of the input alone.
 *       Afterwards the set equals jjs_keyset_create of the old keys followed by the first occurrences in order.
 *   Capacity.  jjs_keyset_create allocates exactly its keys.  An add that fits the capacity writes the new rows, flags, tables
 *     and lookup entries in place behind the old ones and moves nothing.  One that does not fit allocates room for
 *     max(needed, capacity + capacity / 2) keys (at most 2^24), copies device to device, builds the new keys and retires the old
 *     allocation, which launches already queued still read and jjs_trim frees.
 *     JJS_KEYSET_DEVICE_BYTES counts the set's one allocation; every add in place also takes a 256-byte block for the new
 *     size (4 KB per 16 adds, kept until the set moves or is destroyed), which that word leaves out.
 *   jjs_keyset_reserve(ks, n_keys_total): grows the capacity to exactly n_keys_total keys; nothing when the set has that much.
 *   jjs_keyset_growth(ks, out): JJS_KEYSET_CAPACITY .. JJS_KEYSET_ADD_KNOWN below.
 * One add or reserve runs at a time per set; another waits for it.  jjs_shutdown waits for an add in progress, and so does
 * jjs_trim.  A jjs_keyset_destroy that overtakes an add makes the add return -1; nothing leaks.  A failed add leaves the set
 * as it was.
 * Return codes: those of jjs_keyset_create; n == 0 returns 0 and changes nothing; -1 when n_old + n or n_keys_total exceeds
 * 2^24 or the mode is unknown.
 * Measured (profiles/r19_keyset_add.jsonl, tools/keyset_add_rate.py), an add against jjs_keyset_create of all the
 * keys: 64 keys added to 32 768 in place 1.00 ms against 11.5 ms (0.09x), moving the set 4.0 ms (0.35x); 4 096 added to 32 768
 * 2.2 / 5.3 against 12.7 ms; to 4 096 keys 0.47-0.64x in place, 0.65-0.74x moving; to a set of 64 keys an add costs what the
 * create costs (0.99-1.05x: about 1 ms either way, the floor of a blocking call that allocates).  jjs_keyset_verify_dev against a
 * grown set and a created one: equal within the spread (1.000-1.005x).  The existing routes against the parent commit, processes
 * alternating in swapped order (scripts/keyset_add_ab.sh): level at 1, 64 and 131 072 items and in bench.py (median +0.06 %). */
#define JJS_KEYSET_ADD_APPEND 0
#define JJS_KEYSET_ADD_UNIQUE 1
int jjs_keyset_add(jjs_keyset ks, int format, const uint8_t* keys, const uint8_t* keys2, size_t n, int mode, uint8_t* key_status,
                   uint32_t* idx_out, size_t* n_added);
int jjs_keyset_reserve(jjs_keyset ks, size_t n_keys_total);
#define JJS_KEYSET_CAPACITY 0                     /* keys the copies hold room for */
#define JJS_KEYSET_ADD_CALLS 1
#define JJS_KEYSET_RELOCATIONS 2                  /* adds / reserves that moved the copies to a larger allocation */
#define JJS_KEYSET_LOOKUP_REBUILDS 3              /* adds after which the lookup table has more slots */
#define JJS_KEYSET_ADD_KNOWN 4                    /* UNIQUE candidates answered with an index that already existed */
#define JJS_KEYSET_GROWTH 5
int jjs_keyset_growth(jjs_keyset ks, uint64_t out[JJS_KEYSET_GROWTH]);

/* ---- removing keys from a live key set, and compacting it -------------------------------------------
 * A validator that is slashed or rotates out, a contract signer that is revoked, must stop verifying -- at once, without the
 * set being built again and without any other index changing.
 *   jjs_keyset_remove(ks, idx, n, result, n_removed): idx is a host buffer of n key indices; blocking; in place.  Afterwards the
 *     set is indistinguishable from jjs_keyset_create of the same keys in the same order with every removed key replaced by a
 *     malformed one (64 bytes of 0xFF per point column): every jjs_keyset_* and jjs_multisig_*_keyset* call and a later
 *     jjs_keyset_add in either mode give the same bytes -- statuses, tallies, found indices, outputs.
 *       Indices   no index moves and a removed index is never used again; JJS_KEYSET_KEYS does not change, JJS_KEYSET_VALID_KEYS
 *                 drops by the number of removed keys that had status 0.
 *       By index  an item that names a removed key gets status 3, as an index beyond the set does; a multisig transcript that
 *                 names one gets status 3 and no outputs.
 *       By key    a removed key is found nowhere (0xFFFFFFFF, JJS_STATUS_KEY_NOT_IN_SET): a key registered at several indices
 *                 is found at the lowest surviving one, and the host form of jjs_keyset_verify_keys verifies a miss inline.
 *       A later JJS_KEYSET_ADD_UNIQUE registers a key equal to a removed one anew, at a new index.
 *     result (nullable, n bytes): the key's status before this call -- 0, 1 or 3; JJS_KEY_WAS_REMOVED for a key that had been
 *     removed already; JJS_KEY_NOT_IN_RANGE for idx[i] >= the set's keys, which addresses nothing.  An index named twice in one
 *     call gets the same answer both times.  *n_removed (nullable): the distinct indices this call removed.  Both are a function
 *     of the input and the set alone.
 *     A remove frees nothing: JJS_KEYSET_DEVICE_BYTES is unchanged.  jjs_keyset_compact gives the memory back.
 *     Return codes: n == 0 returns 0 and changes nothing; -4 before jjs_init; -1 for a stale handle or a null idx; -2 for a
 *     device failure -- a remove that failed may be repeated (removing is idempotent); the set's counts change only on success.
 *   Calls that overlap a remove.  A remove writes flag bytes and lookup slots that launches already queued read.  A call that
 *     names no key being removed is unaffected.  Each item of jjs_keyset_verify* / jjs_keyset_verify_keys* that names a key being
 *     removed gets its status from before the remove or from after it (by index: the before status or 3; by key: the before
 *     status or JJS_STATUS_KEY_NOT_IN_SET, which it may also get while a higher duplicate of the key survives; with a status
 *     column a by-key item never reports 3 for a key removed under it, unless the call was queued before the set's first
 *     jjs_keyset_remove ever came in).  The jjs_multisig_*_keyset* calls read a row's flags once, in the pass that gathers the
 *     keys: a transcript that names keys being removed gets the answer from before the remove (every such row read before) or
 *     status 3 and no outputs (any row read after), never outputs of neither state.  jjs_keyset_verify_all* reads the flags in
 *     two passes: a batch that names a key being removed gets the verdict from before the remove or the verdict 0 with the
 *     per-item statuses described above, never a verdict 1 that neither state gives.  Calls issued after
 *     jjs_keyset_remove has returned see it complete.
 *   jjs_keyset_compact(ks, map_out, map_len, n_keys_out): afterwards the handle names a set that is jjs_keyset_create of the
 *     surviving keys in their order, byte for byte through every call; keys that were registered malformed or not `is_valid`
 *     and never removed survive.  map_out (nullable; map_len must equal the old JJS_KEYSET_KEYS, else -1): map_out[i] is the
 *     new index of old index i, 0xFFFFFFFF for a removed one.  *n_keys_out (nullable): the new count.  No survivors: -1, nothing
 *     changes (destroy the set instead).  Nothing removed: 0, the identity map, nothing changes.  The set moves to a new
 *     allocation that holds exactly the survivors (a later add is in place or moving by the usual capacity rule); the old one
 *     is retired as jjs_keyset_destroy retires it: launches already queued still read it, WITH THE OLD INDICES, and jjs_trim
 *     frees it.  The move counts under JJS_KEYSET_RELOCATIONS.  EVERY INDEX CHANGES: quiescing the callers that still hold old
 *     indices (key_idx columns, multisig committees, indices JJS_KEYSET_ADD_UNIQUE handed out) is the caller's business.
 *   jjs_keyset_removal(ks, out): JJS_KEYSET_REMOVED_KEYS .. JJS_KEYSET_COMPACT_CALLS below.
 * One add, reserve, remove or compact runs at a time per set; another waits.  jjs_shutdown and jjs_trim wait for one in progress.
 * Measured (profiles/r20_keyset_remove.jsonl, tools/keyset_remove_rate.py), against jjs_keyset_destroy plus
 * jjs_keyset_create of the survivors: a remove of 1, 64 or 4 096 keys from 32 768 takes 0.45-0.49 ms against 9.6-11.2 ms
 * (0.04-0.05x), from 4 096 keys 0.42-0.44 against 2.1-2.2 ms (0.19-0.20x): what the call costs does not grow with k.  A compact
 * of 32 768 keys with a quarter / a half removed 2.71 / 2.68 ms against 8.7 / 6.5 ms (0.31 / 0.41x), of 4 096 keys 0.69 / 0.60
 * against 1.90 / 1.61 ms; the survivors' tables move at 2.5-3.7 TB/s read plus written, counted over the whole call.
 * jjs_keyset_verify_dev against a set with half its keys removed, its compacted form and a created set of the survivors: equal
 * within the spreads at 1, 64 and 131 072 items (1.000-1.003x).  The existing routes against the parent commit, processes
 * alternating in swapped order (scripts/keyset_remove_ab.sh): level at 1, 64 and 131 072 items and in bench.py (eight pairs,
 * medians 8.465 against 8.446 ms per step, either tree 8.41-8.50). */
#define JJS_KEY_WAS_REMOVED 8                     /* result[] only */
#define JJS_KEY_NOT_IN_RANGE 0xFF                 /* result[] only */
int jjs_keyset_remove(jjs_keyset ks, const uint32_t* idx, size_t n, uint8_t* result, size_t* n_removed);
int jjs_keyset_compact(jjs_keyset ks, uint32_t* map_out, size_t map_len, size_t* n_keys_out);
#define JJS_KEYSET_REMOVED_KEYS 0                 /* indices currently removed */
#define JJS_KEYSET_LIVE_KEYS 1                    /* JJS_KEYSET_KEYS minus the above */
#define JJS_KEYSET_REMOVE_CALLS 2
#define JJS_KEYSET_COMPACT_CALLS 3
#define JJS_KEYSET_REMOVAL 4
int jjs_keyset_removal(jjs_keyset ks, uint64_t out[JJS_KEYSET_REMOVAL]);

/* ---- `is_valid` alone: keys and signatures checked without verifying anything --------------------
 * The reference's six validity predicates -- PublicKey / PublicKeyDouble / PublicKeyVarGen::is_valid, Signature /
 * SignatureDouble / SignatureVarGen::is_valid -- and the `from_bytes` of those types, in bulk: what a caller runs when a key or
 * a signature arrives from outside and nothing is to be verified yet.  scheme JJS_SCHEME_*, format JJS_FORMAT_*.
 * Columns: the ones of the verification calls.
 *   keys        K0, K1 of jjs_keyset_verify_keys: affine / extended K0 = PK, K1 = PK' (double) or Gen (var-gen), n x 64 /
 *               n x 96, K1 = NULL for single; wire K0 = the `pk` column of the _wire calls (n x 32, or n x 64), K1 = NULL;
 *   signatures  s0, s1, s2 of jjs_keyset_verify: affine / extended s0 = u (n x 32), s1 = R, s2 = R' (double only), n x 64 /
 *               n x 96; wire s0 = n x 64 (u || R) or n x 96 (u || R || R'), s1 = s2 = NULL.
 * status[i] (nullable, n bytes) is 0, 1 or 3, never 2:
 *   3  a coordinate >= q (extended: also Z >= q); a wire encoding jjs_decompress_dev refuses (v >= q, no square root, u = 0
 *      with the sign bit set); a signature's scalar u >= r;
 *   1  not 3, and some point is not on the curve, is the identity, is not torsion-free, or has Z = 0: `is_valid` is false;
 *   0  every point `is_valid`.
 * An item with two points has the status of the worse one (3 > 1 > 0).  For keys these are, byte for byte, the key_status
 * jjs_keyset_create reports for the same keys in the same format -- without the 204 KB of tables per key.
 * tally (nullable): tally[k] = the items with status k, tally[2] = 0; on the device 4 x uint64.
 * Outputs, all nullable: A0_out, A1_out, R_out, Rp_out n x 64, the canonical affine point of the column (for wire input what
 * jjs_decompress_dev writes for a decodable encoding, for extended input U/Z, V/Z reduced, for affine input the input);
 * u_out n x 32, the scalar copied.  Every output row of an item with status 3 is zero bytes, and so is the row of a point with
 * Z = 0; an item with status 1 that has its points gets its points.  An output of a column the scheme does not have (A1_out
 * for single keys, Rp_out unless double) must be NULL.
 *   _dev: device pointers, 16-byte aligned (the tally 8), asynchronous on `stream`, on the calling thread's current device.
 *     One lane per point.  Extended input without point outputs runs no inversion (the tests are projective); with A0_out,
 *     A1_out, R_out or Rp_out it is normalised first, one shared inversion per lane's items, in a call slot's wire area.
 *   Host buffers: blocking, on the calling thread's current device, through the device's key-set staging area and stream under
 *     the device's host-call lock, as jjs_keyset_find: one such call at a time per device.  No alignment is asked.
 * n == 0 returns 0 and writes only a zero tally.  -4 before jjs_init; -1 for a scheme or format out of range, a NULL column
 * the format needs, a non-NULL column or output it does not take, a misaligned device pointer.
 * Measured resident against jjs_verify_single_dev of as many signatures (profiles/r16_points_check.jsonl): never
 * slower at any of 48 shapes; one key 0.49-0.53x (affine, ext), 0.66-0.72x (ext with outputs), 0.89-0.93x (wire: one square root and
 * one residue test in a row); 2^20 keys 0.09-0.10x, wire 0.18-0.19x; two points per item cost twice one.  The host form against
 * jjs_keyset_create + jjs_keyset_destroy of the same keys: 0.18-0.28x at one key, 0.02-0.04x at 2^15. */
int jjs_keys_check_dev(int scheme, int format, const void* K0, const void* K1, size_t n, void* status, void* tally, void* A0_out,
                       void* A1_out, void* stream);
int jjs_keys_check(int scheme, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint8_t* status, uint64_t tally[4],
                   uint8_t* A0_out, uint8_t* A1_out);
int jjs_signatures_check_dev(int scheme, int format, const void* s0, const void* s1, const void* s2, size_t n, void* status,
                             void* tally, void* u_out, void* R_out, void* Rp_out, void* stream);
int jjs_signatures_check(int scheme, int format, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, size_t n,
                         uint8_t* status, uint64_t tally[4], uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out);

/* ---- one verdict per batch: randomized batch verification -------------------------------------
 * Affine columns in the layouts of jjs_verify_*.  The verdict is 1 (accepted) or 0.
 *   * It never rejects a valid batch: when every item would get status 0 from jjs_verify_* of the same scheme, the
 *     verdict is 1.
 *   * It never accepts a malformed encoding, an invalid point or an identity point: these are checked per item as the
 *     inline entry points check them -- scalars u < r, every coordinate and m < q, every point on the curve, every point
 *     torsion-free (its own pairing residue test, point by point), no point the identity.
 *   * It accepts a batch that contains an item with a failing equation with probability at most 2^-128: the equations
 *     are combined as sum_i z_i (u_i G + c_i PK_i - R_i) == O (z'_i for the double scheme's second equation) with z_i
 *     uniform in [0, 2^128), drawn per call from a ChaCha20 keystream keyed with 32 bytes of getrandom; every
 *     D_i = u_i G + c_i PK_i - R_i has order 1 or r ~ 2^252 once the points are torsion-free, so a non-zero D_j is
 *     cancelled by at most one value of z_j.  The equation is not cofactored and torsion is not batched.
 * The product library has no way to fix the weights (jjs_gpu_profiling.h jjs_debug_pin_hash_seed(2) does, in the profiling
 * build only).  Where the verdict algorithm is not measured faster than the per-item path (the routing
 * table), these calls run the per-item path and reduce its tally instead, so they are never slower than jjs_verify_*
 * followed by a check of tally[0] == n.
 *   Host buffers: blocking, on the calling thread's current device; n = 0 gives verdict 1.  status (nullable, n bytes)
 *     receives the statuses of jjs_verify_* of the same scheme, byte for byte, whenever the verdict is 0 (they are then
 *     computed by the per-item path); when the verdict is 1 it is all zero.  When the verdict algorithm runs, the columns
 *     are uploaded whole to the device's key-set staging area (one such call at a time per device).
 *   _dev: device pointers (16-byte aligned), asynchronous on `stream`; `verdict` is a 4-byte aligned device uint32
 *     written by the call.  No statuses: a caller who gets 0 runs jjs_verify_*_dev for them. */
int jjs_verify_all_single(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* m, size_t n, uint8_t* status,
                          int* verdict);
int jjs_verify_all_double(const uint8_t* u, const uint8_t* R, const uint8_t* R_prime, const uint8_t* PK, const uint8_t* PK_prime,
                          const uint8_t* m, size_t n, uint8_t* status, int* verdict);
int jjs_verify_all_vargen(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* Gen, const uint8_t* m, size_t n,
                          uint8_t* status, int* verdict);
int jjs_verify_all_single_dev(const void* u, const void* R, const void* PK, const void* m, size_t n, void* verdict, void* stream);
int jjs_verify_all_double_dev(const void* u, const void* R, const void* R_prime, const void* PK, const void* PK_prime,
                              const void* m, size_t n, void* verdict, void* stream);
int jjs_verify_all_vargen_dev(const void* u, const void* R, const void* PK, const void* Gen, const void* m, size_t n,
                              void* verdict, void* stream);

/* ---- one verdict per batch against a registered key set ---------------------------------------
 * jjs_keyset_verify_all(_dev)(ks, format, key_idx, s0, s1, s2, m, n, ...): the columns, formats (affine / ext / wire
 * signatures), alignment, threading and return codes of jjs_keyset_verify(_dev); the verdict contract of jjs_verify_all_*:
 *   * The verdict is 1 exactly when jjs_keyset_verify would give every item status 0; such a batch is never rejected.
 *   * It never accepts a malformed encoding, an invalid or identity R, an index >= n_keys, or an item that names a key
 *     whose key_status is not 0: these are checked per item.
 *   * It accepts a batch with a failing equation with probability at most 2^-128.  The verdict algorithm collapses the
 *     key terms of the combined equation per key,
 *         sum_i z_i (u_i G + c_i PK_k(i) - R_i) = (sum_i z_i u_i) G + sum_k S_k PK_k - sum_i z_i R_i,  S_k = sum_{k(i) = k} z_i c_i mod r,
 *     multiplies each S_k over the window tables the set holds and runs the bucket method over the R terms alone; the
 *     collapse is an identity in the group, so the argument above holds unchanged, also for two bad items under one key.
 *   * n = 0 gives 1.
 * Routing: the per-item route (jjs_keyset_verify(_dev) and a check of its tally) serves every call for which the verdict
 * algorithm is not measured faster in profiles/r07_keyset_verify_all.jsonl (the table and the rule), so the
 * call is never slower than jjs_keyset_verify followed by tally[0] == n.  Signatures in the ext and wire formats always
 * take the per-item route.  Counters: a call served by the per-item route counts under JJS_KEYSET_SMALL_CALLS /
 * JJS_KEYSET_LARGE_CALLS exactly as jjs_keyset_verify does; a call served by the verdict algorithm counts under neither
 * (the per-item run that fetches the statuses after a verdict of 0 counts as the jjs_keyset_verify call it is).
 *   Host buffers: blocking; status (nullable, n bytes) holds the statuses of jjs_keyset_verify, byte for byte, when the
 *     verdict is 0, and is all zero when it is 1.
 *   _dev: writes only the 4-byte aligned device uint32 `verdict`; asynchronous on `stream`. */
int jjs_keyset_verify_all(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* s0, const uint8_t* s1,
                          const uint8_t* s2, const uint8_t* m, size_t n, uint8_t* status, int* verdict);
int jjs_keyset_verify_all_dev(jjs_keyset ks, int format, const void* key_idx, const void* s0, const void* s1, const void* s2,
                              const void* m, size_t n, void* verdict, void* stream);

/* ---- wire formats (reference `to_bytes` / `from_bytes`), device buffers, asynchronous ------------------
 * Points travel compressed (32 bytes: little-endian v, parity of u in bit 255) and are decoded on the
 * device; an item with any undecodable point (v >= q, no square root, or u = 0 with the sign bit set)
 * or a scalar out of range gets status 3, where the Rust `from_bytes` would have returned an error.
 *   single : sig = n x 64 (u || R)        reference src/signatures.rs:104-119 ; pk = n x 32  src/keys/public.rs:83-93
 *   double : sig = n x 96 (u || R || R')  src/signatures/double.rs:126-148    ; pk = n x 64 (pk || pk')  src/keys/public/double.rs:169-186
 *   vargen : sig = n x 64 (u || R)        src/signatures/var_gen.rs:95-113    ; pk = n x 64 (pk || generator)  src/keys/public/var_gen.rs:54-79
 *   m      : n x 32 (BlsScalar::to_bytes)
 * 132 / 196 / 164 bytes per verification instead of 196 / 324 / 260. */
int jjs_verify_single_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally,
                               void* stream);
int jjs_verify_double_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally,
                               void* stream);
int jjs_verify_vargen_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally,
                               void* stream);
/* the same from host buffers, blocking (copy in, decode, verify, copy out) */
int jjs_verify_single_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
int jjs_verify_double_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
int jjs_verify_vargen_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
/* JubJubAffine::from_bytes / to_bytes in bulk: in n x 32 -> affine n x 64 + ok n bytes; affine n x 64 -> n x 32 */
int jjs_decompress_dev(const void* in, size_t n, void* affine_out, void* ok_out, void* stream);
int jjs_compress_dev(const void* affine, size_t n, void* out, void* stream);

/* ---- extended coordinates: what the Rust types hold --------------------------------------------------------
 * `PublicKey::verify(&self, &Signature, BlsScalar)` receives `JubJubExtended` points (reference src/keys/public.rs:
 * 114-118, src/signatures.rs:62-65) and normalises them itself with one field inversion per point
 * (`to_hash_inputs()`, src/signatures.rs:127-128).  These entry points take every point as 96 bytes =
 * U || V || Z (three canonical field elements; the affine point is (U/Z, V/Z); `get_u()/get_v()/get_z()` of the
 * Rust type -- reference tests/keys.rs:48-50 -- through `BlsScalar::to_bytes`) and normalise on the device with one inversion shared by many items,
 * so a shim does no field arithmetic at all.  Scalars and m as everywhere else.  Same statuses; additionally a
 * coordinate >= q gives 3 and Z = 0 (not a curve point in any representation) gives 1.  Argument order as the
 * affine entry points. */
int jjs_verify_single_ext_dev(const void* u, const void* R_ext, const void* PK_ext, const void* m, size_t n, void* status,
                              void* tally, void* stream);
int jjs_verify_double_ext_dev(const void* u, const void* R_ext, const void* R_prime_ext, const void* PK_ext,
                              const void* PK_prime_ext, const void* m, size_t n, void* status, void* tally, void* stream);
int jjs_verify_vargen_ext_dev(const void* u, const void* R_ext, const void* PK_ext, const void* Gen_ext, const void* m, size_t n,
                              void* status, void* tally, void* stream);
/* the same from host buffers, blocking */
int jjs_verify_single_ext(const uint8_t* u, const uint8_t* R_ext, const uint8_t* PK_ext, const uint8_t* m, size_t n,
                          uint8_t* status, uint64_t tally[4]);
int jjs_verify_double_ext(const uint8_t* u, const uint8_t* R_ext, const uint8_t* R_prime_ext, const uint8_t* PK_ext,
                          const uint8_t* PK_prime_ext, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]);
int jjs_verify_vargen_ext(const uint8_t* u, const uint8_t* R_ext, const uint8_t* PK_ext, const uint8_t* Gen_ext, const uint8_t* m,
                          size_t n, uint8_t* status, uint64_t tally[4]);

/* ---- multisignature: batch verify_share / combine (reference src/multisig.rs:284-387, 440-500) -------
 * Transcript t owns participants [offsets[t], offsets[t+1]) of the flattened device arrays z (N x 32),
 * PK, R, S (N x 64 affine); m is B x 32.  `offsets` is a HOST array of B + 1 non-decreasing entries starting at 0.
 * A transcript may have any number of participants (the reference takes any non-empty transcript); one without
 * participants gets transcript_status 5, the reference's InvalidMultisigTranscript, and does not affect the others.
 * (The two sponge tags of a transcript of more than 256 participants are computed on the device inside the call.  The hashes
 * of a transcript are sponge chains -- (2 + 2n) / 4 permutations for each of the n delinearisation hashes, which run side by
 * side, and (3 + 4n) / 4 for the binding hash, which is ONE chain -- so the time of a call grows linearly with its longest
 * transcript: about 0.2 ms per participant, 1 000 participants 0.21-0.24 s; a call with few items runs these chains on eight
 * lanes each.)
 * Outputs (device): share_status[i] = 0 when z_i*G + (c*d_i)*PK_i == R_i + a*S_i, 4 (InvalidMultisigShare)
 * when not, 3 for a non-canonical encoding (z_i, a coordinate, or the transcript's m); transcript_status[t]
 * (B bytes, nullable) = 0 when `combine` returns a signature, else the status of the transcript's first failing
 * share (the reference's `combine` stops there, src/multisig.rs:340-353), or 5; agg_pk[t] = aggregate_pk(pk_vec) (64 B
 * affine); and what `combine` returns: sig_u[t] = sum z_i (32 B), sig_R[t] = RSa (64 B affine) -- both all-zero
 * for a transcript whose status is not 0 (no signature comes out of bad shares).
 * Like the reference, the points are not validated.  Asynchronous on `stream`. */
#define JJS_STATUS_INVALID_SHARE 4
#define JJS_STATUS_INVALID_TRANSCRIPT 5
int jjs_multisig_combine_dev(const void* z, const void* PK, const void* R, const void* S, const void* m,
                             const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                             void* agg_pk, void* sig_u, void* sig_R, void* stream);

/* ---- multisig signer groups: register the signers once, combine by group ------------------------------------
 * A committee that signs many messages pays, in the call above, for work that depends on its ordered key vector alone: the n
 * delinearisation hashes of (2 + 2n) / 4 permutations each, d_i * PK_i, the aggregate key, and a window table of every key
 * built inside the lane.  jjs_msig_group_create(PK, n, out) does that once (PK: HOST, n x 64 affine, the ordered pk_vec; the
 * bytes are copied) and keeps on every driven device d_i, aggregate_pk(pk_vec), the tag of the binding hash and the window
 * tables {0 .. 32} * 2^(6 i) * PK_i of every key: 32 B + 43 x 33 x 144 B = 204 KB per participant.  Blocking; built outside the
 * engine's mutex on streams of its own and published under it, as jjs_keyset_create.  Points are NOT validated, as in the
 * reference: the identity, small-order points and repeated keys register.  -1 for n == 0 (the reference's
 * InvalidMultisigTranscript belongs to the vector: there is no group), for more than 2^24 participants and for a coordinate
 * >= q (which keeps the per-call statuses defined); -2 when the group's memory cannot be allocated (nothing is left behind).
 *   jjs_msig_group_combine_dev(g, z, R, S, m, n_transcripts, ...): every transcript has exactly the group's n participants in
 *     the group's order; share (t, i) is row t n + i of z (B n x 32), R and S (B n x 64 affine); m is B x 32.  Device pointers,
 *     16-byte aligned, asynchronous on `stream` on the calling thread's current device.  share_status (B n bytes),
 *     transcript_status (B bytes, nullable), sig_u (B x 32) and sig_R (B x 64) are, byte for byte, what
 *     jjs_multisig_combine_dev writes for the same transcripts with PK tiled B times and offsets[t] = t n, the zeroed outputs
 *     of a transcript whose status is not 0 included (the lane computes the same equation, (c d_i mod r) * PK_i over the stored
 *     tables of PK_i, so this holds for keys with a small-order part as well; for a "key" that is not on the curve neither call
 *     is defined).  agg_pk is not a per-call output: jjs_msig_group_aggregate_pk(g, out) gives the 64 host bytes every row of
 *     the inline call's agg_pk holds.  n_transcripts == 0 returns 0 and writes nothing; n_transcripts * n >= 2^32 returns -1.
 *     Per share the call runs its 1/n part of the binding hash, ONE variable-base multiplication (a * S_i), a comb and one walk
 *     of 43 additions over the stored tables, against (2 + 2n) / 4 more permutations, three variable-base multiplications and
 *     a comb inline (12.0-12.7 M shares/s at 8 participants).  These are operation counts; the rates of the group call are
 *     taken by tools/msig_group_rate.py into profiles/r09_msig_group.jsonl, not by this header.
 *   jjs_msig_group_destroy(g): the handle becomes stale (-1 from then on); launches already queued still read the group's
 *     memory, which jjs_trim or jjs_shutdown frees; jjs_trim never frees a live group, jjs_shutdown frees every group.
 *   jjs_msig_group_info(g, out): JJS_MSIG_GROUP_* words below (the group's memory is reported here, not in jjs_memory_stats).
 * -4 before jjs_init; -1 for an unknown or destroyed handle.  Every call may come from any thread. */
typedef uint64_t jjs_msig_group;                  /* 0 is never a valid handle */
#define JJS_MSIG_GROUP_PARTICIPANTS 0
#define JJS_MSIG_GROUP_WINDOW_BITS 1
#define JJS_MSIG_GROUP_DEVICE_BYTES 2             /* per device */
#define JJS_MSIG_GROUP_CALLS 3                    /* calls served */
#define JJS_MSIG_GROUP_INFO 4
int jjs_msig_group_create(const uint8_t* PK, size_t n, jjs_msig_group* out);
int jjs_msig_group_destroy(jjs_msig_group g);
int jjs_msig_group_info(jjs_msig_group g, uint64_t out[JJS_MSIG_GROUP_INFO]);
int jjs_msig_group_aggregate_pk(jjs_msig_group g, uint8_t out[64]);
int jjs_msig_group_combine_dev(jjs_msig_group g, const void* z, const void* R, const void* S, const void* m,
                               size_t n_transcripts, void* share_status, void* transcript_status, void* sig_u, void* sig_R,
                               void* stream);

/* ---- multisignature from extended coordinates, and from host buffers ------------------------------------------
 * The reference's verify_share / combine receive &[PublicKey], &[JubJubExtended], &[JubJubExtended] (src/multisig.rs:284-291,
 * 332-338): the *_ext calls take PK, R and S as N x 96 = U || V || Z, three canonical field elements per point (the group call:
 * R and S; jjs_msig_group_create_ext: the n keys), and normalise them on the device with one inversion shared by many rows
 * (msig_normalize_kernel in front of the first pass, on the caller's stream), so that a host shim inverts nothing.  Everything
 * else -- arguments, checks, n_transcripts == 0, the 2^32 limit of the group call, return codes, outputs (agg_pk and sig_R stay
 * 64-byte affine) -- is that of the affine call of the same shape.
 * Contract of the extended form: a point is UNUSABLE when U, V or Z is >= q or Z = 0 (the Rust type cannot hold such a value;
 * the rule makes the ABI total).  The outputs of an _ext call are, byte for byte, the outputs of the affine call of the same
 * shape on derived columns in which every usable point is the canonical (U/Z, V/Z) and every unusable point is 64 bytes of
 * 0xFF.  A share with an unusable point therefore gets status 3 from the range test of its coordinates and its transcript
 * gets no signature; whatever the affine call does with the rest of such a transcript, the extended call does too.  Z = 0
 * gives status 3 here, NOT InvalidPoint (2) as in jjs_verify_*_ext: the multisignature calls validate no points and have no
 * such status.  jjs_msig_group_create_ext refuses a set with an unusable key with -1, as jjs_msig_group_create refuses a
 * coordinate >= q; a group registered from extended keys is the group registered from their affine forms (the same
 * aggregate_pk, the same bytes out of every call).
 * jjs_multisig_combine / jjs_msig_group_combine: the same two calls from HOST buffers, blocking; format = JJS_FORMAT_AFFINE or
 * JJS_FORMAT_EXT (JJS_FORMAT_WIRE: -1).  No alignment is asked of the pointers; transcript_status may be NULL.  The columns are
 * uploaded whole into a grow-only staging area of the calling thread's current device (reported under JJS_MEMORY_HOST_STAGING;
 * jjs_trim frees it) and the call runs on a stream of the engine, one such call at a time per device. */
int jjs_multisig_combine_ext_dev(const void* z, const void* PK_ext, const void* R_ext, const void* S_ext, const void* m,
                                 const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                 void* agg_pk, void* sig_u, void* sig_R, void* stream);
int jjs_msig_group_create_ext(const uint8_t* PK_ext, size_t n, jjs_msig_group* out);
int jjs_msig_group_combine_ext_dev(jjs_msig_group g, const void* z, const void* R_ext, const void* S_ext, const void* m,
                                   size_t n_transcripts, void* share_status, void* transcript_status, void* sig_u, void* sig_R,
                                   void* stream);
int jjs_multisig_combine(int format, const uint8_t* z, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                         const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                         uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R);
int jjs_msig_group_combine(jjs_msig_group g, int format, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                           size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R);

/* ---- multisignature from wire encodings ------------------------------------------------------------------------
 * What the parties of the protocol hold when they first touch the data: a verifier receives PublicKey::to_bytes() (32 bytes a
 * key) and Signature::to_bytes() (64 bytes = u || R); a combiner receives every signer's key, its two nonce commitments and its
 * share over the network, 32 bytes a point.  The *_wire calls are the multisignature calls of the other sections -- inline, by
 * signer group, by key set, combine and the verifier's two -- with every point column as N x 32 = JubJubAffine::to_bytes, decoded
 * on the device (msig_decode_kernel in front of the first pass, on the caller's stream, one lane per point).  The `format`
 * argument of the calls that have one keeps refusing JJS_FORMAT_WIRE with -1: these entry points are the wire form.
 * Layouts.  Points: N x 32 (the key-set forms: R_w and S_w; jjs_msig_group_create_wire: the n keys).  z, m, offsets, key_idx
 * and every output: unchanged -- agg_pk and sig_R stay 64-byte affine as in the extended form (jjs_compress_dev turns them into
 * wire bytes).  The aggregate signature of the verifier's calls is ONE column sig_w, B x 64 = u || R, the layout of
 * jjs_verify_single_wire, where the other forms take u and R.
 * Contract.  An encoding is UNDECODABLE by the rules of jjs_decompress_dev, unchanged: v >= q, (v^2 - 1) / (1 + d v^2) not a
 * square, or u = 0 with the sign bit set.  The outputs of a wire call are, byte for byte, the outputs of the affine call of the
 * same shape on derived columns in which every decodable encoding is the point jjs_decompress_dev writes for it and every
 * undecodable encoding is 64 bytes of 0xFF.  A share, key or signature with an undecodable point therefore gets status 3 from
 * the range test of its coordinates -- the family's rule, and the status jjs_verify_single_wire gives -- and its transcript or
 * vector gets no signature or aggregate; whatever the affine call does with the rest of it, the wire call does too.  Decodable
 * points are on the curve but need not be in the prime-order subgroup: they pass through unvalidated, as everywhere in this
 * family.  Alignment (16 bytes for the _dev forms, none for the host forms), asynchrony, n_transcripts == 0, limits and return
 * codes are those of the affine call of the same shape; -4 before jjs_init, before any argument is looked at.
 * jjs_msig_group_create_wire refuses a vector with an undecodable key with -1, as jjs_msig_group_create_ext refuses an unusable
 * one; a group registered from wire keys is the group registered from the affine keys they decode to (the same aggregate_pk,
 * the same bytes out of every call, whatever the format of the call).
 * The signer's half (jjs_multisig_round1_dev, jjs_multisig_sign*) has no wire form: it takes values its caller made.
 * Measured (profiles/r15_msig_wire.jsonl, tools/msig_wire_rate.py: one MI355X, resident all-decodable inputs, 8 / 64 / 256
 * participants at 1 / 64 / 4 096 transcripts, 7 rounds, medians; (a) the wire call, (b) one jjs_decompress_dev per point column
 * then the affine call, (c) the affine call alone).  The decode is a small share of a call: (a)/(c) is 0.97-1.04 for combine,
 * 1.00-1.07 by group (two shapes aside, below), 1.00-1.17 for the verifier's calls, largest where the call is shortest.  Against
 * (b) the wire call wins beyond the spreads at 12 of 36 shapes, all combine and group calls (0.92-0.99 of b's time; 0.81 at one group call of 256 participants, B = 1), loses at 4
 * and is level at 20: the verifier's calls are level everywhere but three shapes lost by 0.04-0.23 ms (1.005-1.012), and one
 * group call of 64 participants, B = 1, is lost by 1.75 ms (12.4 against 10.7, 1.164).  What the wire form buys a caller is the
 * contract (one call, statuses folded), not time. */
int jjs_multisig_combine_wire_dev(const void* z, const void* PK_w, const void* R_w, const void* S_w, const void* m,
                                  const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                  void* agg_pk, void* sig_u, void* sig_R, void* stream);
int jjs_multisig_combine_wire(const uint8_t* z, const uint8_t* PK_w, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                              const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                              uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R);
int jjs_msig_group_create_wire(const uint8_t* PK_w, size_t n, jjs_msig_group* out);
int jjs_msig_group_combine_wire_dev(jjs_msig_group g, const void* z, const void* R_w, const void* S_w, const void* m,
                                    size_t n_transcripts, void* share_status, void* transcript_status, void* sig_u, void* sig_R,
                                    void* stream);
int jjs_msig_group_combine_wire(jjs_msig_group g, const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                                size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u,
                                uint8_t* sig_R);
int jjs_multisig_combine_keyset_wire_dev(jjs_keyset ks, const void* key_idx, const void* z, const void* R_w, const void* S_w,
                                         const void* m, const uint32_t* offsets_host, size_t n_transcripts, void* share_status,
                                         void* transcript_status, void* agg_pk, void* sig_u, void* sig_R, void* stream);
int jjs_multisig_combine_keyset_wire(jjs_keyset ks, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R_w,
                                     const uint8_t* S_w, const uint8_t* m, const uint32_t* offsets, size_t n_transcripts,
                                     uint8_t* share_status, uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u,
                                     uint8_t* sig_R);
int jjs_multisig_aggregate_pk_wire_dev(const void* PK_w, const uint32_t* offsets_host, size_t n_transcripts, void* agg_pk,
                                       void* vec_status, void* stream);
int jjs_multisig_aggregate_pk_wire(const uint8_t* PK_w, const uint32_t* offsets, size_t n_transcripts, uint8_t* agg_pk,
                                   uint8_t* vec_status);
int jjs_multisig_verify_wire_dev(const void* PK_w, const uint32_t* offsets_host, const void* sig_w, const void* m,
                                 size_t n_transcripts, void* agg_pk, void* status, void* tally, void* stream);
int jjs_multisig_verify_wire(const uint8_t* PK_w, const uint32_t* offsets, const uint8_t* sig_w, const uint8_t* m,
                             size_t n_transcripts, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]);
int jjs_multisig_verify_keyset_wire_dev(jjs_keyset ks, const void* key_idx, const uint32_t* offsets_host, const void* sig_w,
                                        const void* m, size_t n_transcripts, void* agg_pk, void* status, void* tally, void* stream);
int jjs_multisig_verify_keyset_wire(jjs_keyset ks, const uint32_t* key_idx, const uint32_t* offsets, const uint8_t* sig_w,
                                    const uint8_t* m, size_t n_transcripts, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]);

/* ---- multisignature for committees drawn from a registered key set ----------------------------------------------
 * A validator set registered once (jjs_keyset_create, JJS_SCHEME_SINGLE, any key format) of which every message is signed by
 * another ordered subset: d_i = H(pk_i, pk_1 .. pk_n) changes with the subset, so a signer group does not fit, and the inline
 * call rebuilds, in every lane, window tables the set already keeps on the device.  These calls take the inline call's ragged
 * transcripts with the keys named by index: key_idx is N x uint32 (4-byte aligned for the _dev form), one entry per share,
 * instead of the PK column (4 bytes a share instead of 64 or 96; no key is normalised in the extended format).  `format` is
 * that of R and S: JJS_FORMAT_AFFINE (N x 64) or JJS_FORMAT_EXT (N x 96, normalised on the device as in
 * jjs_msig_group_combine_ext_dev); JJS_FORMAT_WIRE gives -1.  z, m, offsets, n_transcripts, every output and its layout, the
 * limits, the alignment and the asynchrony on `stream` are those of jjs_multisig_combine_dev.  The call acts on the calling
 * thread's current device and uses that device's copy of the set; launches already queued keep reading a destroyed set until
 * jjs_trim, as for jjs_keyset_verify_dev.  -1 for a set of another scheme and for an unknown or destroyed handle; -4 before
 * jjs_init; n_transcripts == 0 returns 0 and writes nothing.
 * Contract.  A row is USABLE when key_idx[i] < n_keys and key_status[key_idx[i]] == 0.
 *   A transcript whose rows are all usable: every output (share_status, transcript_status, agg_pk, sig_u, sig_R) is, byte for
 *     byte, what jjs_multisig_combine_dev writes for it with PK[i] = the registered key's canonical affine bytes (extended
 *     format: what jjs_multisig_combine_ext_dev writes on the same affine keys expanded with Z = 1) -- rows with z >= r,
 *     m >= q, or an R or S coordinate >= q or unusable included.  Only the two products by PK_i change method (a walk of 43
 *     additions over the set's stored tables instead of a table built in the lane and a multiplication); a registered valid key
 *     is on the curve, so both give the same group element, and every comparison and output is made in affine form.
 *   A transcript that names an unusable row: every share of it gets status 3, transcript_status is 3, agg_pk[t], sig_u[t] and
 *     sig_R[t] are all zero; the other transcripts of the call are not affected.  No lane reads outside the set: an unusable
 *     row is replaced by a stand-in before any key or table is addressed.
 *   An empty transcript gives status 5, as inline.
 *   DIFFERENCE FROM THE REFERENCE: its multisignature validates no key; a key set refuses the identity, small-order and
 *     off-curve keys (key_status 1) and non-canonical ones (3).  A committee with such a key uses the inline call.
 * Per share the call runs the inline call's hashes, ONE variable-base multiplication (a * S_i), a comb and two walks of 43
 * additions, against three variable-base multiplications and a comb inline.  These are operation counts; rates against the
 * inline call: not measured (the record profiles/r11_msig_keyset.jsonl of tools/msig_keyset_rate.py does not exist yet).
 * jjs_multisig_combine_keyset: the same from HOST buffers, blocking, as jjs_multisig_combine: no alignment is asked of the
 * pointers, transcript_status may be NULL, one such call at a time per device. */
int jjs_multisig_combine_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const void* z, const void* R, const void* S,
                                    const void* m, const uint32_t* offsets_host, size_t n_transcripts, void* share_status,
                                    void* transcript_status, void* agg_pk, void* sig_u, void* sig_R, void* stream);
int jjs_multisig_combine_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R,
                                const uint8_t* S, const uint8_t* m, const uint32_t* offsets, size_t n_transcripts,
                                uint8_t* share_status, uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R);

/* ---- verifying aggregate multisignatures: aggregate_pk, and aggregate_pk followed by PublicKey::verify ------------
 * The verifier's half of the scheme (reference src/multisig.rs:90-92: pk = aggregate_pk(&pk_vec); pk.verify(&sig, message)).
 * A verifier receives (key vector, message, aggregate signature) and never sees a share, so the combine calls do not serve
 * it.  Two operations, aggregation alone and aggregation followed by the single-scheme verification, each with the keys
 * inline or named by index into a JJS_SCHEME_SINGLE key set, each as a _dev call (device pointers, asynchronous on `stream`)
 * and as a blocking host-buffer call.  Layouts are those of the multisig calls: offsets is a HOST array of B + 1 non-decreasing
 * uint32 starting at 0 (vector t owns rows [offsets[t], offsets[t+1])); PK is N x 64 affine or N x 96 extended; key_idx is
 * N x uint32; u is B x 32, R is B x 64 or B x 96, m is B x 32; agg_pk is B x 64 affine and a required output of every call;
 * vec_status and status are B bytes, tally is 4 x uint64 (status, tally and vec_status may each be NULL).
 * `format` is JJS_FORMAT_AFFINE or JJS_FORMAT_EXT (JJS_FORMAT_WIRE: -1); for the inline calls it describes PK and R, for the
 * key-set calls R alone.
 * Unusable key vectors.  A vector is UNUSABLE when
 *   inline affine:   a coordinate of one of its keys is >= q, or a key is not on the curve;
 *   inline extended: a key is unusable by the rule of jjs_multisig_combine_ext_dev (U, V or Z >= q, or Z = 0), or its
 *                    normalised point is not on the curve;
 *   key set:         key_idx[i] >= n_keys or key_status[key_idx[i]] != 0 (as in jjs_multisig_combine_keyset, no lane
 *                    addresses the set before the row has been replaced by its stand-in).
 *   The on-curve test is particular to these calls: a few products per key, unreachable through the Rust types (which cannot
 *   hold an off-curve point), and what makes a verifier's call total on bytes it did not produce.  Apart from it keys are not
 *   validated, as in the reference: the identity, small-order points and repeated keys aggregate, and for such vectors agg_pk
 *   is what jjs_multisig_combine_dev writes for the same PK and offsets.
 * Aggregation.  agg_pk[t] = aggregate_pk(pk_vec_t), byte for byte the agg_pk row of jjs_multisig_combine_dev for every
 *   usable, non-empty vector; vec_status[t] = 0.  An unusable vector gets vec_status 3 and agg_pk[t] all zero; the other
 *   vectors are not affected.  An EMPTY vector is usable: aggregate_pk(&[]) is the identity (src/multisig.rs:416-429), so
 *   agg_pk[t] is the affine bytes of (0, 1) and vec_status 0 -- on purpose unlike combine, which rejects an empty transcript
 *   with status 5: aggregate_pk has no error.
 * Verification.  agg_pk as above.  status[t] is exactly what jjs_verify_single returns for (u[t], R[t], PK = agg_pk[t], m[t]),
 *   with its statuses and their precedence: an aggregate that is the identity or has a torsion part gives 1, and so does an
 *   empty vector.  An unusable vector gives status 3 and agg_pk[t] all zero, whatever the signature holds.  tally counts the
 *   statuses as jjs_verify_single_dev does.
 * Extended format.  The outputs are, byte for byte, those of the affine call on derived columns in which every usable point
 *   is its canonical (U/Z, V/Z) and every unusable point is 64 bytes of 0xFF.  An unusable R therefore gives 3, not 1: this
 *   is the multisignature family's rule ("multisignature from extended coordinates" above), NOT that of jjs_verify_single_ext,
 *   where Z = 0 is InvalidPoint.
 * n_transcripts == 0 returns 0, zeroes tally if given and writes nothing else.  -4 before jjs_init; -1 for a bad format, a
 * NULL or misaligned pointer, offsets that do not start at 0 or decrease, an unknown or destroyed handle, a set of another
 * scheme.  _dev pointers are 16-byte aligned (key_idx 4-byte, tally 8-byte, vec_status none); the host forms ask for no
 * alignment, upload whole columns into the multisig staging area and run one such call at a time per device, as
 * jjs_multisig_combine does.  Scratch is the grow-only multisignature scratch; no call allocates per call.
 * Per vector of n keys the call runs n hashes of 2 + 2n inputs, n multiplications (key set: walks of the stored tables), one
 * inversion, and for a verification one five-input hash and one equation: the first two of the combine call's seven passes.
 * Rates (profiles/r12_msig_verify.jsonl, the record of tools/msig_verify_rate.py: one MI355X, resident inputs, 7 rounds, medians;
 * DESIGN.md 6.6) against the only earlier route, jjs_multisig_combine_dev with dummy shares followed by jjs_verify_single_dev:
 * faster at all 18 recorded shapes by more than the spread of either side -- vectors of 8 keys 2.3-2.8x inline and 3.1-4.7x by
 * key set (B = 1, 64, 4 096: 2.1 / 2.1 / 2.9 ms inline, 1.3 / 1.4 / 2.1 ms key set), 64 keys 2.7-2.9x and 3.1-3.5x at B <= 64,
 * 1.57x and 1.75x at B = 4 096 (30.2 and 27.2 ms), 256 keys 3.1x at B = 1 (19.6 ms), 2.1-2.2x at B = 64, 1.16x and 1.21x at
 * B = 4 096 (411 and 396 ms for 2^20 key rows: the n hashes of 2 + 2n inputs are then nearly all of either route).  Against
 * jjs_oracle_c on 16 host threads (jjo_multisig_combine, which has no aggregate-only entry, and jjo_verify_single; timed on the
 * distinct vectors and scaled to B): 4x at one vector of 8 keys, 110x at one vector of 256, about 800-1 700x at B = 4 096. */
int jjs_multisig_aggregate_pk_dev(int format, const void* PK, const uint32_t* offsets_host, size_t n_transcripts,
                                  void* agg_pk, void* vec_status, void* stream);
int jjs_multisig_aggregate_pk(int format, const uint8_t* PK, const uint32_t* offsets, size_t n_transcripts,
                              uint8_t* agg_pk, uint8_t* vec_status);
int jjs_multisig_aggregate_pk_keyset_dev(jjs_keyset ks, const void* key_idx, const uint32_t* offsets_host,
                                         size_t n_transcripts, void* agg_pk, void* vec_status, void* stream);
int jjs_multisig_aggregate_pk_keyset(jjs_keyset ks, const uint32_t* key_idx, const uint32_t* offsets,
                                     size_t n_transcripts, uint8_t* agg_pk, uint8_t* vec_status);
int jjs_multisig_verify_dev(int format, const void* PK, const uint32_t* offsets_host, const void* u, const void* R,
                            const void* m, size_t n_transcripts, void* agg_pk, void* status, void* tally, void* stream);
int jjs_multisig_verify(int format, const uint8_t* PK, const uint32_t* offsets, const uint8_t* u, const uint8_t* R,
                        const uint8_t* m, size_t n_transcripts, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]);
int jjs_multisig_verify_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const uint32_t* offsets_host,
                                   const void* u, const void* R, const void* m, size_t n_transcripts,
                                   void* agg_pk, void* status, void* tally, void* stream);
int jjs_multisig_verify_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint32_t* offsets,
                               const uint8_t* u, const uint8_t* R, const uint8_t* m, size_t n_transcripts,
                               uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]);

/* ---- multisignature: the signer's half (csrc/msig_sign.h; reference src/multisig.rs sign_round_1 :169-184, sign_round_2
 * :213-257) ----
 * GENERATORS OF TEST AND BENCHMARK MATERIAL, as jjs_sign_*: NOT constant time -- table look-ups and branches depend on sk, r
 * and s.  Never use them with production keys.  A C ABI also cannot enforce the one-shot MultisigNonce of the reference
 * (src/multisig.rs:131-141, consumed by sign_round_2): using a pair (r, s) in two calls, or in two rows, is the caller's error.
 * jjs_multisig_round1_dev is sign_round_1 given the two RNG draws: R[i] = r[i] * G, S[i] = s[i] * G (n x 64 affine each; r, s
 * n x 32).  bad_out (nullable, n bytes) is 1 where r[i] or s[i] is >= the group order, and both output rows are then zero.
 * Device pointers, 16-byte aligned (bad_out none), asynchronous on `stream`.
 * jjs_multisig_sign_dev is sign_round_2 over whole ragged batches.  The transcripts (PK, R, S, m, offsets_host,
 * n_transcripts) are exactly what jjs_multisig_combine_dev takes, with its offsets rules, limits, alignment and asynchrony;
 * `format` describes PK, R and S and is JJS_FORMAT_AFFINE or JJS_FORMAT_EXT (JJS_FORMAT_WIRE: -1).  Extended points are
 * normalised in poison mode: an unusable point becomes 64 bytes of 0xFF and its transcript therefore gets status 3, the
 * multisignature family's rule.  signer_row is n_signing x uint32 (4-byte aligned): the global row (over all transcripts) each
 * signing row's share belongs to; NULL means n_signing == N and signing row j belongs to row j, the whole-transcript generator
 * (NULL with n_signing != N: -1).  sk, r, s and z_out are n_signing x 32; sign_status is n_signing bytes and required.
 * Row search.  sign_round_2 searches pk_vec for the signer's key; these calls are TOLD the row.  A wrong row gives status 5
 * even when the key stands elsewhere in the transcript (include/jjs_schnorr.hpp and Engine.multisig_sign_round2's callers do
 * the search on the host).
 * sign_status[j], with i = signer_row[j] and t the transcript of row i -- the first rule that matches:
 *   3  i >= N (nothing is addressed through i); sk[j], r[j] or s[j] >= the group order; or an encoding of transcript t is out
 *      of range: a coordinate of any PK, R or S of the transcript >= q (every signing row of the transcript gets 3), m[t] >= q
 *   5  (JJS_STATUS_INVALID_TRANSCRIPT) sk[j] * G != PK[i]; PK[i] stands at another row of the transcript as well ("occurs
 *      exactly once", src/multisig.rs:223-231: both rows get 5); r[j] * G != R[i]; s[j] * G != S[i]
 *   7  (JJS_STATUS_DUPLICATED_NONCE) two rows of transcript t hold the same R, or the same S (src/multisig.rs:238-246);
 *      the same point in two DIFFERENT transcripts is not a duplicate
 *   0  z_out[j] = r + s * a - (c * d_i) * sk mod the group order: byte for byte the reference's share
 * This is the reference's order of checks with the encoding test in front, as everywhere in this ABI.  Equality of points is
 * equality of their 64 canonical affine bytes.  For every status other than 0, z_out[j] is 32 zero bytes.
 * n_transcripts == 0 or n_signing == 0 returns 0 and writes nothing.  -4 before jjs_init, -1 for a bad format, a NULL or
 * misaligned pointer or unacceptable offsets.  Scratch is the grow-only multisignature scratch, enlarged by the flag words of
 * the check pass (4 bytes per row, 136 per transcript); no call allocates per call.
 * jjs_multisig_sign is the same from host buffers, blocking, on the route of jjs_multisig_combine: no alignment is asked of the
 * pointers, one such call runs at a time per device, and the staged bytes of sk, r and s are cleared on the stream behind the
 * share pass, before the call returns.
 * Per transcript of n participants a call runs the five front passes of the combine call, a scan of n^2 / 2 byte compares
 * spread over n lanes, and per signing row three fixed-base multiplications.  Rates (profiles/r14_msig_sign.jsonl, the record of
 * tools/msig_sign_rate.py: one MI355X, resident inputs made on the device, signer_row = NULL, 7 rounds, medians; DESIGN.md
 * 6.6): 0.85-0.99 of the time of jjs_multisig_combine_dev on the same transcripts -- 4.7 / 4.4 / 5.1 ms at B = 1, 64, 4 096
 * transcripts of 8 participants (6.4 M shares/s at the last), 16 / 16 / 44 ms at 64, 58 / 70 / 465 ms at 256 (2.3 M shares/s);
 * one transcript of 1 000 participants 224 ms, of whose kernel time the check pass is 0.3 %. */
#define JJS_STATUS_DUPLICATED_NONCE 7
int jjs_multisig_round1_dev(const void* r, const void* s, size_t n, void* R_out, void* S_out, void* bad_out, void* stream);
int jjs_multisig_sign_dev(int format, const void* PK, const void* R, const void* S, const void* m,
                          const uint32_t* offsets_host, size_t n_transcripts,
                          const void* signer_row, const void* sk, const void* r, const void* s, size_t n_signing,
                          void* z_out, void* sign_status, void* stream);
int jjs_multisig_sign(int format, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                      const uint32_t* offsets, size_t n_transcripts,
                      const uint32_t* signer_row, const uint8_t* sk, const uint8_t* r, const uint8_t* s, size_t n_signing,
                      uint8_t* z_out, uint8_t* sign_status);

/* ---- multisignature: verify_share on its own (csrc/msig_share.h; reference src/multisig.rs verify_share :284-309,
 * verify_share_with_coefficients :366-387) ----
 * verify_share(share, participant_index, pk_vec, R_vec, S_vec, msg) for single shares: the check a coordinator makes as shares
 * arrive, before anyone may combine.  A call takes B transcripts exactly as the combine call of the same route takes them
 * (jjs_multisig_combine_dev: PK, R, S, m, offsets_host; jjs_msig_group_combine_dev: R, S, m for B transcripts of the group's n
 * participants; jjs_multisig_combine_keyset_dev: key_idx, R, S, m, offsets_host), with that call's offsets rules and limits,
 * and Q = n_shares queries: share_transcript[q] (uint32) the transcript t the share belongs to, share_slot[q] (uint32) the
 * reference's participant_index inside that transcript, z[q] (32 bytes) the share.  Several queries on one transcript or on
 * one slot (with equal or different z), queries in any order and transcripts without a query are all legal; Q may exceed the
 * number of rows.  `format` describes the point columns and is JJS_FORMAT_AFFINE, _EXT or _WIRE; extended and wire points go
 * through the combine calls' ingest in poison mode (an unusable point becomes 64 bytes of 0xFF).
 * share_status[q] (required, Q bytes) -- the first rule that matches:
 *   3  share_transcript[q] >= B
 *   3  z[q] >= the group order
 *   3  an encoding of transcript t is unusable: a coordinate of any PK, R or S >= q, or m[t] >= q (affine); what poison mode
 *      turns into 0xFF rows (extended, wire); an index outside the set, or a key the set refused or has removed (key set).
 *      Every query of that transcript gets 3: jjs_multisig_sign's rule
 *   5  (JJS_STATUS_INVALID_TRANSCRIPT) transcript t has no participants, or share_slot[q] >= its number of participants
 *      (src/multisig.rs:292-298)
 *   4  z * G + (c * d_j mod r) * PK_j != R_j + a * S_j, with c * d_j reduced before the point is multiplied (csrc/msig_group.h)
 *   0  otherwise
 * A query whose status is 3 or 5 addresses nothing through its indices.
 * sig_R (nullable, B x 64) receives the aggregate commitment RSa of EVERY transcript, named by a query or not: byte for byte
 * what the combine call returns as R for that transcript with valid shares, and 64 zero bytes for a transcript to which the
 * third rule or the rule of status 5 applies.  A coordinate set < q that names no point of the curve has no defined outputs.
 * n_transcripts == 0 returns 0 and writes nothing; so does n_shares == 0 with sig_R == NULL; with sig_R given a call without
 * queries still fills it.  -4 before jjs_init; -1 for a bad format, a NULL or misaligned pointer, an unknown handle or
 * unacceptable offsets.  The _dev forms take device pointers, the columns 16-byte aligned, the two query index columns (and
 * key_idx) 4-byte aligned, share_status unaligned, and are asynchronous on `stream` on the calling thread's device.  The
 * forms without _dev are the same from host buffers, blocking, on the route of jjs_multisig_combine: no alignment is asked,
 * one such call runs at a time per device.  Group calls count in JJS_MSIG_GROUP_CALLS.
 * Scratch is the grow-only multisignature scratch, enlarged by one extended point per query (144 bytes), one flag word per
 * transcript and the two columns a call may have no output for (132 bytes per transcript); no call allocates per call.
 * What a call runs.  Per transcript of n participants: the front of the route's combine call (inline: the map, n hashes and
 * n products d_i * PK_i, pk_agg and a; group: the hash of a alone; key set: the gather, n hashes and n table walks, pk_agg and
 * a), n range tests, then 2 n point additions, ONE variable-base product (RSa = sum R_i + a * sum S_i -- the same group element
 * as the combine call's sum of n products, on the whole curve: DESIGN.md 6.6) and the hash of c.  Per query: one product
 * a * S_j, and the equation -- a comb and one product by PK_j (inline) or one walk over the stored tables (group, key set).  The
 * combine route to the same answer runs n products a * S_i, n products by PK_i and n combs per transcript, and clears sig_R
 * when the filler shares fail.
 * Rates (profiles/r21_msig_share.jsonl, the record of tools/msig_share_rate.py: one MI355X, resident inputs made on the device, one
 * query per transcript against the route's combine call with the query's z at its row and zero filler, alternating, 7 rounds,
 * medians), time of the new call / time of the combine route.  Where the device is full the saved work shows:
 * B = 4 096 transcripts of 64 and 256 participants 0.86 and 0.94 inline, 0.78 and 0.70 by group (10.9 against 14.0 ms, 37.9
 * against 54.2 ms), 0.90 and 0.96 by key set.  At B = 64 (8, 64, 256 participants) and at B = 4 096 of 8 it is 1.01-1.06 on
 * every route: no faster, inside the 10 % spread between boxes and runs.  At B = 1 it is SLOWER than that margin on seven of
 * twelve shapes: 8 participants 1.08 / 1.15 / 1.23 (inline / group / key set: 5.9 against 5.5 ms, 3.4 against 3.0, 4.7 against
 * 3.8), 64 participants 0.96 / 1.13 / 1.12, 256 participants 1.15 / 1.01 / 1.11, one transcript of 1 000 participants 1.08 /
 * 0.99 / 1.16 (223 against 206 ms inline).  A call with one transcript is as long as its longest lane: the products and combs the
 * new call leaves out ran in lanes that were idle anyway, while its sums lane does 2 n additions, two inversions and a product
 * one after the other where the combine call spreads the products over n lanes. */
int jjs_multisig_verify_share_dev(int format, const void* PK, const void* R, const void* S, const void* m,
                                  const uint32_t* offsets_host, size_t n_transcripts,
                                  const void* share_transcript, const void* share_slot, const void* z, size_t n_shares,
                                  void* share_status, void* sig_R, void* stream);
int jjs_multisig_verify_share(int format, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                              const uint32_t* offsets, size_t n_transcripts,
                              const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z, size_t n_shares,
                              uint8_t* share_status, uint8_t* sig_R);
int jjs_msig_group_verify_share_dev(jjs_msig_group g, int format, const void* R, const void* S, const void* m,
                                    size_t n_transcripts,
                                    const void* share_transcript, const void* share_slot, const void* z, size_t n_shares,
                                    void* share_status, void* sig_R, void* stream);
int jjs_msig_group_verify_share(jjs_msig_group g, int format, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                                size_t n_transcripts,
                                const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z, size_t n_shares,
                                uint8_t* share_status, uint8_t* sig_R);
int jjs_multisig_verify_share_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const void* R, const void* S,
                                         const void* m, const uint32_t* offsets_host, size_t n_transcripts,
                                         const void* share_transcript, const void* share_slot, const void* z, size_t n_shares,
                                         void* share_status, void* sig_R, void* stream);
int jjs_multisig_verify_share_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* R, const uint8_t* S,
                                     const uint8_t* m, const uint32_t* offsets, size_t n_transcripts,
                                     const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z,
                                     size_t n_shares, uint8_t* share_status, uint8_t* sig_R);

/* ---- transcript parity (debug export): c_out = n x 32 bytes, the 250-bit challenge per item ---- */
int jjs_challenge_single_dev(const void* R, const void* PK, const void* m, size_t n, void* c_out, void* stream);
int jjs_challenge_double_dev(const void* R, const void* R_prime, const void* PK, const void* PK_prime, const void* m,
                             size_t n, void* c_out, void* stream);
int jjs_challenge_vargen_dev(const void* R, const void* PK, const void* Gen, const void* m, size_t n, void* c_out,
                             void* stream);

/* ---- key derivation (reference `PublicKey::from(&SecretKey)` src/keys/public.rs:54-60, `PublicKeyDouble::from`
 * src/keys/public/double.rs:47-57): PK[i] = sk[i] * G and, when PKp_out is not NULL, PK'[i] = sk[i] * G'
 * (64 B affine each).  bad_out (nullable, n bytes) is set to 1 where sk[i] >= r.  Fixed-base comb, device
 * pointers, asynchronous on `stream`.  NOT constant time: for public test material, not for live secrets. */
int jjs_public_keys_dev(const void* sk, size_t n, void* PK_out, void* PKp_out, void* bad_out, void* stream);

/* ---- signing: generator of synthetic inputs (NOT constant time, not for production keys) -------
 * sk, rnd: scalars < r; m: field element < q.  rnd is the RNG draw the reference's hedged nonce
 * mixes in (reference src/nonce.rs:32-44).  Outputs: u (n x 32), points (n x 64 affine). */
int jjs_sign_single_dev(const void* sk, const void* rnd, const void* m, size_t n, void* u_out, void* R_out,
                        void* PK_out, void* stream);
int jjs_sign_double_dev(const void* sk, const void* rnd, const void* m, size_t n, void* u_out, void* R_out,
                        void* R_prime_out, void* PK_out, void* PK_prime_out, void* stream);
/* gen_scalar: per-item generator = gen_scalar * G (reference src/keys/secret/var_gen.rs:162-172) */
int jjs_sign_vargen_dev(const void* sk, const void* gen_scalar, const void* rnd, const void* m, size_t n, void* u_out,
                        void* R_out, void* PK_out, void* Gen_out, void* stream);

/* ---- var-generator signing and key derivation with the generator as a POINT (csrc/sign_vargen.h) ----
 * The reference's SecretKeyVarGen holds { sk, generator: JubJubExtended } (src/keys/secret/var_gen.rs:98-101); `new` (:147),
 * SecretKey::with_variable_generator and from_bytes (:109-131, 64 bytes = sk || generator compressed) all take the generator as
 * a point, which in real use has no known discrete logarithm.  jjs_sign_vargen_dev above takes a SCALAR and serves
 * SecretKeyVarGen::random alone; these calls take the point.
 * GENERATORS OF TEST AND BENCHMARK MATERIAL, as jjs_sign_*: NOT constant time -- table look-ups and branches depend on sk and
 * on the nonce; never use with production keys.
 * format describes Gen: JJS_FORMAT_AFFINE n_gen x 64, JJS_FORMAT_EXT n_gen x 96 (U || V || Z), JJS_FORMAT_WIRE n_gen x 32
 * (JubJubAffine::to_bytes).  sk, rnd: n x 32 scalars; m: n x 32.  The n_gen rule: n_gen is n (one generator per item) or 1 (one
 * generator for the whole call: with_variable_generator over many keys); any other value gives -1; n_gen == 1 with n == 1 is
 * the per-item call.
 * Outputs: u_out n x 32; R_out, PK_out n x 64 affine; Gen_out n_gen x 64, the canonical affine generator (what
 * to_hash_inputs() returns); status n bytes.  status, u_out and R_out are required, PK_out too for the derivation call; PK_out
 * of the signing call and Gen_out may be NULL.
 * status[i] is 0 or 3 (the reference's signer has no error; the ABI is total).  3: sk[i] >= r, rnd[i] >= r (the reference draws
 * a JubJubScalar, src/nonce.rs:92), m[i] >= q, or the item's generator is unusable: a coordinate >= q; extended, Z >= q or
 * Z = 0; a wire encoding that jjs_decompress_dev refuses; or a point that is not on the curve (the test jjs_multisig_verify
 * applies to inline keys, for the same reason: off the curve the addition law computes nothing).  Every output row of a
 * status-3 item is zero bytes; when a shared generator is unusable every item gets 3 and Gen_out is zero.  0: everything else.
 * The generator is NOT validated, as in the reference: the identity, small-order points, points with a torsion part and sk = 0
 * (tests/schnorr_var_generator.rs:119) sign and derive.
 * For status 0 the values are byte for byte the reference's: r = H(rnd, sk, gen_u, gen_v, m) truncated, R = r * Gen,
 * PK = sk * Gen, c = H(R, PK, Gen, m), u = r - c * sk (oracle/jjs_oracle.py sign_vargen_with_rand, mul).
 * Extended and wire formats follow the multisignature family's rule: the outputs are those of the affine call on derived
 * columns in which every usable point is its canonical affine form and every unusable point 64 bytes of 0xFF, which the range
 * test turns into status 3.
 * _dev: device pointers, 16-byte aligned (status: any alignment), asynchronous on `stream`, ordered with the other signing
 * calls as they order themselves (they share a workspace).  The host forms are blocking, ask no alignment, take the route of
 * jjs_multisig_sign, one at a time per device; the staged bytes of sk and rnd are cleared on the stream behind the last kernel,
 * before the call returns.  n == 0 returns 0 and writes nothing.  -4 before jjs_init, before any argument is looked at; -1 for
 * a bad format, a bad n_gen, a NULL required pointer or a misaligned device pointer.  No call allocates once the engine's
 * buffers have reached its shape; jjs_trim frees what this adds.
 * Two routes.  Per item (n_gen == n, and n_gen == 1 below 64 items): one lane per item builds the 4-bit table of its generator and
 * runs two multiplications of 252 doublings; R and PK share ONE inversion; a shared generator is read with stride 0.  Shared
 * generator (a signing call with n_gen == 1 and n >= 64): the 6-bit window tables of the one generator are built once per call
 * (204 KB of grow-only scratch), and each lane walks them twice, 43 additions a walk and no doubling.  The two routes give the
 * same bytes for every point of the curve.  jjs_debug_sign_limits reports the 64; the derivation call always runs per item.
 * Rates (profiles/r17_sign_vargen_pt.jsonl, the record of tools/sign_vargen_pt_rate.py: one MI355X, resident inputs made on the
 * device, 7 rounds, medians, the variants alternating; ms per call): against jjs_sign_vargen_dev on gen_scalar with
 * Gen = gen_scalar * G, the per-item route takes 0.93-0.95x its time from 64 items on (2^20 items: 39.8 ms against 42.3, 26.3 M
 * against 24.8 M signatures/s; extended 40.0 ms, wire 41.5 ms; one item: 3.0 against 3.3 ms, within the spread of 0.9).  With
 * one generator for the call the shared route against the per-item route: 2.25 against 2.72 ms at 64 items, 2.32 / 2.76 at 1 024,
 * 2.30 / 2.82 at 16 384, 5.35 / 10.2 at 2^18 and 17.8 / 39.7 ms at 2^20 (58.9 M signatures/s), each difference beyond the spread
 * of either side; at one item 2.41 against 2.88 ms with spreads of 0.4 and 0.7: no winner, hence the threshold of 64.
 */
int jjs_public_keys_vargen_dev(int format, const void* sk, const void* Gen, size_t n_gen, size_t n,
                               void* PK_out, void* Gen_out, void* status, void* stream);
int jjs_sign_vargen_pt_dev(int format, const void* sk, const void* Gen, size_t n_gen, const void* rnd, const void* m, size_t n,
                           void* u_out, void* R_out, void* PK_out, void* Gen_out, void* status, void* stream);
int jjs_public_keys_vargen(int format, const uint8_t* sk, const uint8_t* Gen, size_t n_gen, size_t n,
                           uint8_t* PK_out, uint8_t* Gen_out, uint8_t* status);
int jjs_sign_vargen_pt(int format, const uint8_t* sk, const uint8_t* Gen, size_t n_gen, const uint8_t* rnd, const uint8_t* m, size_t n,
                       uint8_t* u_out, uint8_t* R_out, uint8_t* PK_out, uint8_t* Gen_out, uint8_t* status);
/* [0] lanes of the signing kernels resident at once on the current device, [1] the smallest n the shared-generator route
 * serves (UINT64_MAX: none).  Negative return: an error code. */
int jjs_debug_sign_limits(uint64_t out[2]);

/* ---- signing and key derivation with a SecretKey, single and double scheme (csrc/sign_fixed.h) ----
 * What a holder of the reference's SecretKey calls: PublicKey::from(&sk) (src/keys/public.rs:54-60), PublicKeyDouble::from(&sk)
 * (src/keys/public/double.rs:47-57), SecretKey::sign (src/keys/secret.rs:174-194) and sign_double (src/keys/secret/double.rs:56-85),
 * with range checks and statuses, host buffers and wire bytes out.  jjs_sign_single_dev, jjs_sign_double_dev and
 * jjs_public_keys_dev above stay as they are.
 * GENERATORS OF TEST AND BENCHMARK MATERIAL, as jjs_sign_*: NOT constant time -- table look-ups and branches depend on sk and
 * on the nonce; never use with production keys.
 * scheme: JJS_SCHEME_SINGLE or JJS_SCHEME_DOUBLE; JJS_SCHEME_VARGEN and anything else give -1 (that scheme has
 * jjs_sign_vargen_pt).  The n_sk rule: n_sk is n (a key per item) or 1 (one key for the call: sk is one row, and PK_out, PKp_out
 * and pk_w_out are one row); any other value gives -1; n_sk == 1 with n == 1 is the per-item call.
 * Layouts: sk n_sk x 32 and rnd n x 32 scalars; m n x 32; u_out n x 32; R_out, Rp_out n x 64 affine; PK_out, PKp_out n_sk x 64
 * affine; sig_w_out n x 64 (single) or n x 96 (double), Signature::to_bytes = u || compress(R) [|| compress(R')]; pk_w_out
 * n_sk x 32 (single) or n_sk x 64 (double), PublicKey::to_bytes = compress(PK) [|| compress(PK')]; status n bytes, any
 * alignment.  compress is jjs_compress_dev's: little-endian v, the parity of u in bit 255.
 * Required: the inputs and status.  Every output is nullable on its own; a signing call with u_out, R_out, Rp_out and sig_w_out
 * all NULL gives -1, and so does a derivation call with all three outputs NULL.  Rp_out and PKp_out must be NULL for the single
 * scheme (the rule of jjs_keys_check for a column the scheme does not have).
 * status[i] is 0 or 3 (the reference's signer has no error; the ABI is total).  3: sk >= r, rnd[i] >= r (the reference draws a
 * JubJubScalar, src/nonce.rs:92) or m[i] >= q; the derivation call tests sk[i] alone.  Every output row a status-3 item owns is
 * zero bytes.  With n_sk == 1 the key rows belong to the call: they are the key's whatever the items' rnd and m are, and an
 * unusable key gives every item 3 and zero key rows.  sk is the only validated input: sk = 0 signs, its key is the identity.
 * For status 0 the values are byte for byte the reference's: r = H(rnd, sk, tag, m) truncated with tag 1 (single) or 2 (double),
 * R = r * G, R' = r * G', c the 5-input or the tagged 10-input challenge, u = r - c * sk; the affine outputs are byte for byte
 * what jjs_sign_single_dev / jjs_sign_double_dev write for the same sk, rnd and m, and the wire outputs what jjs_compress_dev
 * makes of them.
 * _dev: device pointers, 16-byte aligned (status: any alignment), asynchronous on `stream`, ordered with the other signing
 * calls as they order themselves (they share a workspace).  The host forms are blocking, ask no alignment, take the route of
 * jjs_sign_vargen_pt, one at a time per device; the staged bytes of sk and rnd are cleared on the stream behind the last kernel,
 * before the call returns, on every way out.  n == 0 returns 0 and writes nothing.  -4 before jjs_init, before any argument is
 * looked at; -1 for the cases above, a NULL required pointer or a misaligned device pointer; -2 when scratch cannot be
 * allocated.  A refused call writes nothing.  No call allocates once the engine's buffers have reached its shape; jjs_trim frees
 * what this adds.
 * One lane per item; all the points of an item share ONE field inversion (jjs_sign_*_dev: one per point).  Two routes for
 * n_sk == 1.  Per item: every lane reads the one key row and multiplies it out again.  Keyed: a one-lane launch in front derives
 * PK (and PK') once into 256 bytes of grow-only scratch, and each lane runs r * G (and r * G') alone.  Both give the same bytes.
 * A call with n_sk == 1 takes the keyed route from 2^20 items on (jjs_debug_sign_fixed_limits reports it); the derivation call
 * always runs per item.
 * Rates (profiles/r18_sign_fixed.jsonl, the record of tools/sign_fixed_rate.py: one MI355X, resident inputs made on the device,
 * 7 rounds, medians, the variants alternating; ms per call, max - min of the rounds in brackets).  Against jjs_sign_single_dev /
 * jjs_sign_double_dev with n_sk = n: single 0.78x their time at one item (0.83 against 1.07 ms), 0.94-0.95x from 64 to 2^18 and
 * 0.96x at 2^20 (11.15 (0.19) against 11.60 (0.22) ms, 94.1 M against 90.4 M signatures/s); double level at one item (1.30
 * against 1.30 ms) and 0.89-0.91x from 64 items on (2^20: 15.93 (0.14) against 17.60 (0.12) ms, 65.8 M against 59.6 M/s); at no
 * recorded shape slower beyond the spreads.  The wire outputs add at most 1 % from 64 items on (2^20: 11.19 and 16.00 ms); at
 * one item 0.94 against 0.83 ms (single) and 1.50 against 1.30 ms (double, 1.16x the old signer's time: the one shape at which a
 * new call is slower than the old one).  One key for the call, keyed against per item: slower by 5-10 % from 64 to 16 384 items
 * in both schemes (single 0.882 against 0.828 ms at 64) and by 31 % at one double item (1.58 against 1.20 ms); single within the
 * spread at 2^18 (2.67 against 2.73 ms, spreads to 0.08) and 0.95x at 2^20 (10.41 (0.08) against 10.95 (0.12) ms, 100.7 M/s);
 * double 0.95x at 2^18 (3.66 against 3.85 ms) and 0.92x at 2^20 (14.40 (0.25) against 15.59 (0.13) ms, 72.8 M/s): hence the
 * threshold of 2^20, the first shape at which both schemes win.  Derivation against jjs_public_keys_dev: single level
 * (0.94-1.02x, 1.32 against 1.31 ms at 2^20, with the range test and status it adds), double 0.65-0.83x (2.06 against 2.74 ms at
 * 2^20: one inversion instead of two).
 */
int jjs_sign_fixed_dev(int scheme, const void* sk, size_t n_sk, const void* rnd, const void* m, size_t n,
                       void* u_out, void* R_out, void* Rp_out, void* PK_out, void* PKp_out,
                       void* sig_w_out, void* pk_w_out, void* status, void* stream);
int jjs_sign_fixed(int scheme, const uint8_t* sk, size_t n_sk, const uint8_t* rnd, const uint8_t* m, size_t n,
                   uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out, uint8_t* PK_out, uint8_t* PKp_out,
                   uint8_t* sig_w_out, uint8_t* pk_w_out, uint8_t* status);
int jjs_public_keys_fixed_dev(int scheme, const void* sk, size_t n, void* PK_out, void* PKp_out, void* pk_w_out,
                              void* status, void* stream);
int jjs_public_keys_fixed(int scheme, const uint8_t* sk, size_t n, uint8_t* PK_out, uint8_t* PKp_out,
                          uint8_t* pk_w_out, uint8_t* status);
/* [0] lanes of the SecretKey signing kernels resident at once on the current device, [1] the smallest n the keyed route
 * serves (UINT64_MAX: none).  Negative return: an error code. */
int jjs_debug_sign_fixed_limits(uint64_t out[2]);

/* ---- Poseidon digests of ragged inputs (csrc/digest.h) ----
 * What a caller who holds payloads calls before the first verify, sign or multisig call: out[i] is
 * dusk_poseidon::Hash::digest(Domain::Other, &item_i)[0] and, with JJS_DIGEST_TRUNCATED in flags, Hash::digest_truncated
 * (the low 250 bits) -- 32 bytes, canonical, little endian: the `m` column of every other call as it stands.  It equals
 * oracle/jjs_oracle.py poseidon_digest(item i) bit for bit.
 * Input: `in` is ONE column of elements, the items back to back.  offsets_host == NULL: every item has k elements.  Otherwise
 * offsets_host holds n + 1 words in HOST memory that start at 0 and never decrease, item i is elements [offsets[i],
 * offsets[i + 1]) and k is ignored (the convention of the multisignature calls); the words are read before the call returns.
 * format: JJS_DIGEST_CANONICAL, elements of 32 bytes little endian, each < q; JJS_DIGEST_WIDE, elements of 64 bytes little
 * endian reduced mod q (BlsScalar::from_bytes_wide, the reference's own way from bytes to a field element, src/nonce.rs:98-99).
 * status: nullable, n bytes, any alignment.  0, or 3 when a canonical-format element of the item is >= q; such an item gets a
 * zero row, with or without a status column, and touches no other item.  The wide format never gives 3.
 * -1: a format other than the two, a flag bit other than bit 0, a NULL `in` or `out`, a misaligned device pointer, offsets that
 * do not start at 0 or that decrease, an item of no elements (k == 0 too: no vector of the reference pins the empty absorb), an
 * item of more than 2^31 - 1 elements (the SAFE tag encodes 0x80000000 | length), more than 2^32 - 1 items.  -4 before
 * jjs_init, before any argument is looked at.  n == 0 returns 0 and writes nothing.  `out` must not overlap `in`.
 * _dev: device pointers, 16-byte aligned (status: any alignment), asynchronous on `stream`.  A uniform call uploads nothing; a
 * ragged call uploads its offsets and an order of its items into grow-only scratch and is ordered with the signing calls as they
 * order themselves.  No call allocates once that scratch has reached its shape; jjs_trim frees it.  The host form is blocking,
 * asks no alignment and takes the route of jjs_multisig_sign, one such call at a time per device.
 * Two routes, chosen by n alone: up to the limit jjs_debug_digest_limits reports, eight lanes share an item's permutations
 * (the latency route); beyond, an item has one lane (the throughput route), and the lanes of a ragged call take the items by
 * their count of sponge blocks, longest first, so that a wave's lanes end together.  Both give the same bytes.  Lengths up to
 * 1 027 take their SAFE tag from a table; a longer item's tag is computed on the device, once per item.
 * Rates (profiles/r22_digest.jsonl, the record of tools/digest_rate.py: one MI355X, resident inputs, 5 rounds, medians, every side in
 * a process of its own, this commit's library and the parent's alternating; ms per call).  k = 5 truncated against the parent's
 * jjs_challenge_single_dev: 0.271 against 0.485 at one item and 0.276 / 0.461 at 1 024 (0.56-0.60x: the eight-lane route), 0.506 /
 * 0.515 at 2^16, 5.79 / 5.73 at 2^20 (1.01x, spreads 0.21 and 0.23; 181 M digests/s).  k = 16 against the parent's
 * jjs_debug_poseidon_dev: 0.533 / 0.976 at one item, 0.526 / 0.900 at 1 024, 0.923 / 0.938 at 2^16, 10.99 / 10.10 at 2^20 (1.09x,
 * beyond the spreads of 0.06: the canonical one-lane kernel holds three waves per SIMD where that kernel holds four; 95 M digests/s).
 * Routes forced in turn: eight lanes 0.55-0.66x of one lane up to 8 192 items, level at 16 384, 1.7-4.2x from 32 768 on.  2^18 ragged
 * items of 1-131 elements: 15.2 ms with the order against 25.0 in input order (0.61x); with one item of 1 031 among them 66 against
 * 70 ms (spreads 8-11): that item's 258 permutations on one lane outlast the rest of the call either way.  oracle poseidon_any on 16
 * threads: 6.6 s for 2^20 items of 5, 13.1 s for 2^20 of 16 (1 100x the call).
 */
#define JJS_DIGEST_CANONICAL 0   /* elements n_el x 32 B little endian, each < q              */
#define JJS_DIGEST_WIDE      1   /* elements n_el x 64 B little endian, reduced mod q         */
#define JJS_DIGEST_TRUNCATED 1   /* flags bit 0: keep the low 250 bits (digest_truncated)     */
int jjs_digest_dev(int format, int flags, const void* in, const uint32_t* offsets_host, size_t k, size_t n,
                   void* out, void* status, void* stream);
int jjs_digest(int format, int flags, const uint8_t* in, const uint32_t* offsets, size_t k, size_t n,
               uint8_t* out, uint8_t* status);
/* [0] the largest n the eight-lanes-per-item route serves, [1] the lanes of the one-lane-per-item kernel's grid on the current
 * device (a call of more items takes a second trip through its grid-stride loop).  Negative return: an error code. */
int jjs_debug_digest_limits(uint64_t out[2]);

/* ---- primitives exposed for parity tests ------------------------------------------------------ */
/* out[i] = a[i] * b[i] mod q (canonical bytes in and out) */
int jjs_debug_fq_mul_dev(const void* a, const void* b, size_t n, void* out, void* stream);
/* out[i] = untruncated Poseidon digest of the k field elements at in[(i*k + j)*32] */
int jjs_debug_poseidon_dev(const void* in, size_t k, size_t n, void* out, void* stream);
/* out[i] bit0 = on curve, bit1 = torsion free (pairing test, as used by verify; identity counts as
 * torsion free), bit2 = identity, bit3 = torsion free by the reference's definition [r]P == O */
int jjs_debug_point_flags_dev(const void* points, size_t n, void* out, void* stream);
/* The half-size scalars the verify kernels derive from a challenge (csrc/verify_core.h half_size_scalars, the
 * device code path): for c[i] (n x 32 bytes, canonical, < r) a_out[i], b_out[i] (n x 16 bytes each, little-endian)
 * and b_neg_out[i] (n bytes) with a = +-b*c (mod r), a, |b| < 2^126: Euclid's algorithm on (r, c) stopped at the
 * first remainder below 2^126.  Device pointers, 16-byte aligned. */
int jjs_debug_half_scalars_dev(const void* c, size_t n, void* a_out, void* b_out, void* b_neg_out, void* stream);
/* copies the fixed-base table of G (which = 0) or G' (which = 1) to host memory; size in bytes via
 * jjs_debug_comb_table_bytes() */
size_t jjs_debug_comb_table_bytes(void);
int jjs_debug_comb_table(int which, void* host_out);
/* copies the square-root tables of the current device (csrc/decode.h) to host memory: 7 x 256 x 9 uint32 of powers of the
 * root of unity in Montgomery form, and the 65536-byte table of the logarithms in the order-256 subgroup */
int jjs_debug_dlog_tables(void* pow_host_out, void* hash_host_out);
/* Loads RCCL, forms a one-rank clique on the current device and all-reduces a known 4 x u64 vector on the
 * engine stream: the call sequence of the multi-device tally reduction, runnable with a single GPU. */
int jjs_debug_rccl_selftest(void);
/* The lanes of the multisignature kernel that are resident at once on the current device (its grid limit times its block
 * size, from the occupancy query at jjs_init): a call with more shares than this takes a second trip through the kernel's
 * grid-stride loop.  Negative: an error code. */
int jjs_debug_msig_resident_lanes(void);

#ifdef __cplusplus
}
#endif
#endif /* JJS_GPU_H */
