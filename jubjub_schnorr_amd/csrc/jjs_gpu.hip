// libjjs_gpu.so: HIP kernels (gfx950) + the C ABI of include/jjs_gpu.h.
//
// A verification call takes one of three paths, chosen from its size and from how often its keys repeat (nothing
// else: no switch, no environment variable), all with the same statuses:
//   throughput  (verify_core.h)   one signature per lane: prepare_kernel (hash, scalar lattice, pairing tests; four
//               waves per SIMD), verify_kernel (the equations; a persistent pass whose grid is what the chip holds
//               resident, each lane owning WS_WORDS_PER_LANE words of workspace for its window tables) and
//               resolve_kernel (the items verify_kernel could not decide);
//   key tables  (key_tables.h)    >= 65 536 items whose keys repeat >= 16 times on average: keys deduplicated on the
//               device, validity and window tables once per key (second stream, beside the hashes), additions only
//               per signature (key_verify_kernel); decided on the device, no host round trip;
//   latency     (small_batch.h)   <= 16 384 items: one signature spread over 11-45 lanes in two launches.
// The per-status tally is reduced with wave ballots and one atomic per wave per status.  One process can drive
// several devices (jjs_init); all state is per device, per-call state lives in call slots (call_slot).
//
// This translation unit in parts (textual includes inside one anonymous namespace, in this order):
//   device_kernels.h   every __global__ entry
//   device_owners.h    the owners of device and pinned memory, grow-only buffers, streams and events; when one may free
//   engine_state.h     device state, call slots, staging threads, errors, slot ordering, the retired list
//   verify_job.h       the arenas of the key-table path; a verification call in stages (begin, ingest, keys, hash, finish)
//   (here)             device set-up and tear-down, the RCCL clique
//   host_calls.h       the large blocking host-buffer calls: upload plan, staging copies, the pipeline
//   (here)             the multisignature scratch (msig_scratch.h: its layout and growth, plain C++), the frame of the calls over it,
//                      the schedule of msig_kernel's passes
//   msig_host_calls.h  the blocking host-buffer forms of the multisignature calls
//   msig_keyset_calls.h  the multisignature call against a registered key set, both forms
//   msig_verify_calls.h  the verifier's half: aggregate_pk, and aggregate_pk followed by the single-scheme verification
//   msig_sign_calls.h  the signer's half: sign_round_1, and sign_round_2 over whole ragged batches (a generator of test material)
//   msig_share_calls.h  verify_share on its own: single shares by transcript and slot, inline, by signer group and by key set
//   sign_vargen_calls.h  var-generator signing and key derivation with the generator as a point, both forms (test material)
//   sign_fixed_calls.h  signing and key derivation with a SecretKey in the single and double schemes, both forms (test material)
//   digest_calls.h     Poseidon digests of ragged inputs, both forms: the routes, the order of a ragged call's items
//   host_lanes.h       the small ones (included among the entry points, behind the table of call shapes): staging lanes
//                      outside the engine's mutex, calls of several threads in one launch
//   (here)             the table of call shapes and the staged_call builder it drives; the extern "C" entry points
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <optional>
#include <random>
#include <sched.h>
#include <climits>
#include <linux/futex.h>
#include <sys/random.h>
#include <sys/syscall.h>
#include <cerrno>
#include <unistd.h>
#include <thread>
#include <vector>

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif
#include <rccl/rccl.h>

#include "../../include/jjs_gpu.h"
#include "schemes.h"
#include "decode.h"
#include "normalize.h"
#include "small_batch.h"
#include "key_tables.h"
#include "keyset.h"
#include "keyset_lookup.h"
#include "keyset_add.h"
#include "keyset_remove.h"
#include "sign_core.h"
#include "sign_vargen.h"
#include "sign_fixed.h"
#include "multisig_core.h"
#include "msig_group.h"
#include "msig_keyset.h"
#include "msig_verify.h"
#include "msig_sign.h"
#include "msig_share.h"
#include "msig_scratch.h"
#include "batch_verdict.h"
#include "keyset_verdict.h"
#include "points_check.h"
#include "digest.h"
#include "jjs_sponge_tags_long.inc"

using namespace jjs;

namespace {

#include "device_kernels.h"
#include "verdict_kernels.h"
#include "keyset_verdict_kernels.h"
#include "keyset_add_kernels.h"
#include "keyset_remove_kernels.h"
#include "digest_kernels.h"
#include "device_owners.h"
#include "engine_state.h"
#include "verify_job.h"

// Every entry point works on the calling thread's current HIP device, which must be one jjs_init set up.
int check_ready() {
    if (L.devs.empty()) return fail(JJS_ERR_NOT_INIT, "jjs_init has not been called");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    for (device_state* d : L.devs)
        if (d->device == dev) { g = d; return JJS_OK; }
    return fail(JJS_ERR_NOT_INIT, "the current HIP device (%d) is not one of the %zu this process initialised", dev,
                L.devs.size());
}

template <typename... Ptrs>
bool all_ok(Ptrs... p) {
    return ((p != nullptr && aligned16(p)) && ...);
}

int init_device(device_state& d, int ordinal) {
    d.device = ordinal;
    HIP_TRY(hipSetDevice(ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    HIP_TRY(d.stream.create(hipStreamNonBlocking));
    for (stream_owner& side : d.side) HIP_TRY(side.create(hipStreamNonBlocking));
    HIP_TRY(d.host_begin.create(hipEventDisableTiming));
    HIP_TRY(d.copy_stream.create(hipStreamNonBlocking));
    HIP_TRY(d.ks_stream.create(hipStreamNonBlocking));
    {   // the per-key kernels are few, long waves that must finish before the challenge hashes do: dispatch them first
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        d.key_priority = hi;
        d.table_priority = lo;
    }
    HIP_TRY(d.side_join.create(hipEventDisableTiming));
    HIP_TRY(d.ingest_done.create(hipEventDisableTiming));
    for (size_t i = 0; i < HOST_MAX_PIECES; ++i) {
        HIP_TRY(d.chunk_up[i].create(hipEventDisableTiming));
        HIP_TRY(d.chunk_done[i].create(hipEventDisableTiming));
    }
    HIP_TRY(d.last_use.create(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(d.last_use, d.stream));
    int per_cu_v = 0, per_cu_s = 0, per_cu_m = 0, per_cu_r = 0;
    int per_cu_p = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_p, prepare_kernel, BLOCK, 0));
    d.grid_prepare = prop.multiProcessorCount * (per_cu_p < 1 ? 1 : per_cu_p) * 4;   // not persistent: a few blocks per slot
    int per_cu_k = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_k, key_verify_kernel, BLOCK, 0));
    d.grid_key_verify = prop.multiProcessorCount * (per_cu_k < 1 ? 1 : per_cu_k) * 4;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_r, resolve_kernel, BLOCK, 0));
    d.grid_resolve = prop.multiProcessorCount * (per_cu_r < 1 ? 1 : per_cu_r);
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_v, verify_kernel, BLOCK, 0));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_s, sign_kernel, BLOCK, 0));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_m, msig_kernel, BLOCK, 0));
    if (per_cu_v < 1) per_cu_v = 1;
    if (per_cu_s < 1) per_cu_s = 1;
    if (per_cu_m < 1) per_cu_m = 1;
    d.grid_sign = prop.multiProcessorCount * per_cu_s;
    d.grid_msig = prop.multiProcessorCount * per_cu_m;
    // slot 0: the workspace of the largest persistent grid (verify, sign, multisig share it); small slots: one
    // lane's worth per item of the largest call they take
    d.slots[0].grid_verify = prop.multiProcessorCount * per_cu_v;
    int lanes_blocks = d.slots[0].grid_verify > d.grid_sign ? d.slots[0].grid_verify : d.grid_sign;
    if (d.grid_msig > lanes_blocks) lanes_blocks = d.grid_msig;
    {   // the SecretKey signers (sign_fixed.h): one grid for their four kernels, within the lanes the workspace is sized for
        int per_cu_f = 0, least = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&least, sign_fixed_single_kernel, BLOCK, 0));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_f, sign_fixed_double_kernel, BLOCK, 0));
        if (per_cu_f < least) least = per_cu_f;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_f, sign_fixed_keyed_single_kernel, BLOCK, 0));
        if (per_cu_f < least) least = per_cu_f;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_f, sign_fixed_keyed_double_kernel, BLOCK, 0));
        if (per_cu_f < least) least = per_cu_f;
        d.grid_sign_fixed = prop.multiProcessorCount * (least < 1 ? 1 : least);
        if (d.grid_sign_fixed > lanes_blocks) d.grid_sign_fixed = lanes_blocks;
    }
    {   // the digest kernels (digest.h): one grid for the four, the lanes resident at once
        int per_cu_d = 0, least = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&least, digest_kernel<DG_CANONICAL>, BLOCK, 0));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, digest_kernel<DG_WIDE>, BLOCK, 0));
        if (per_cu_d < least) least = per_cu_d;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, digest_coop_kernel<DG_CANONICAL>, BLOCK, 0));
        if (per_cu_d < least) least = per_cu_d;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, digest_coop_kernel<DG_WIDE>, BLOCK, 0));
        if (per_cu_d < least) least = per_cu_d;
        d.grid_digest = prop.multiProcessorCount * (least < 1 ? 1 : least);
    }
    for (int i = 0; i < N_SLOTS; ++i) {
        call_slot& c = d.slots[i];
        const bool big = i == 0 || i == SECOND_BIG_SLOT;
        const size_t slot_items = i <= N_SMALL_SLOTS ? SMALL_SLOT_ITEMS : MEDIUM_SLOT_ITEMS;
        c.grid_verify = big ? d.slots[0].grid_verify : (int)(slot_items / BLOCK);
        // slot 0 also serves the signer and the multisig kernels, whose grids may be larger than the verify grid
        const size_t lanes = i == 0 ? (size_t)lanes_blocks * BLOCK : (big ? (size_t)c.grid_verify * BLOCK : slot_items);
        HIP_TRY(c.workspace.alloc(lanes * WS_WORDS_PER_LANE * sizeof(uint32_t)));
        HIP_TRY(c.last_use.create(hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c.last_use, d.stream));
        if (i == 0 || i > N_SMALL_SLOTS) {       // slots whose calls can be large enough for the key tables: a key stream each
            HIP_TRY(c.key_fork.create(hipEventDisableTiming));
            HIP_TRY(c.key_mid.create(hipEventDisableTiming));
            HIP_TRY(c.key_join.create(hipEventDisableTiming));
            HIP_TRY(c.key_ahead.create(hipEventDisableTiming));
            HIP_TRY(c.key_chains.create(hipEventDisableTiming));
            HIP_TRY(c.key_cleared.create(hipEventDisableTiming));
            HIP_TRY(c.seen.alloc(sizeof(key_feedback)));
            memset(c.seen.get(), 0, sizeof(key_feedback));
        }
    }
    // The priority streams, in the order of their importance: the runtime hands its high-priority hardware queues out in
    // creation order, and the key streams of the big slots must have one each (scripts/timeline.sh: created behind two
    // other priority streams, the small launches of the first big slot's key stream waited 0.3-0.5 ms each for wave slots
    // instead of 0.1, and a resident 2^20 batch took 0.5 ms longer).
    // The two streams on which a host-buffer call normalises extended points come right behind the big slots' key streams: a
    // large host call runs in the second big slot, and with its ingest stream on the hardware queue of that slot's key stream the
    // normalisation of its last range waited 1.6 ms behind the key chains and tables (scripts/host_timeline.sh ... ext; a 2^20-item
    // single call 12.1-12.3 -> 11.6-11.8 ms, profiles/r04_host_ext_ab.jsonl).
    {
        static_assert(N_MEDIUM_SLOTS == 3 && N_BIG_SLOTS == 2, "one entry per slot that has a key stream");
        for (int i : {0, SECOND_BIG_SLOT}) HIP_TRY(d.slots[i].key_stream.create(hipStreamNonBlocking, d.key_priority));
        for (stream_owner& is : d.ingest) HIP_TRY(is.create(hipStreamNonBlocking, d.key_priority));
        for (int i : {1 + N_SMALL_SLOTS, 2 + N_SMALL_SLOTS, 3 + N_SMALL_SLOTS})
            HIP_TRY(d.slots[i].key_stream.create(hipStreamNonBlocking, d.key_priority));
    }
    for (call_slot& c : d.slots)
        if (c.key_stream) HIP_TRY(c.table_stream.create(hipStreamNonBlocking, d.table_priority));
    HIP_TRY(d.comb_g.alloc(COMB_TABLE_WORDS * sizeof(uint32_t)));
    HIP_TRY(d.comb_gn.alloc(COMB_TABLE_WORDS * sizeof(uint32_t)));
    HIP_TRY(d.tag.alloc(32));
    HIP_TRY(d.tally.alloc(4 * sizeof(unsigned long long)));
    HIP_TRY(d.dlog_pow.alloc(DLOG_POW_WORDS * sizeof(uint32_t)));
    HIP_TRY(d.dlog_hash.alloc(65536));
    HIP_TRY(hipMemsetAsync(d.dlog_hash, 0, 65536, d.stream));
    hipLaunchKernelGGL(dlog_table_kernel, dim3(7), dim3(BLOCK), 0, d.stream, d.dlog_pow, d.dlog_hash);
    HIP_TRY(d.tags_long.alloc(sizeof(JJS_SPONGE_TAG_LONG)));
    HIP_TRY(hipMemcpyAsync(d.tags_long, JJS_SPONGE_TAG_LONG, sizeof(JJS_SPONGE_TAG_LONG), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.tag, JJS_DOUBLE_TAG_WORDS, 32, hipMemcpyHostToDevice, d.stream));
    const int blocks = (COMB_WINDOWS * COMB_ENTRIES + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(comb_kernel, dim3(blocks), dim3(BLOCK), 0, d.stream, d.comb_g, 0);
    hipLaunchKernelGGL(comb_kernel, dim3(blocks), dim3(BLOCK), 0, d.stream, d.comb_gn, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d.stream));
    return JJS_OK;
}

// The end of a device's state, whole or half set up (the way out of a failed jjs_init): nobody queues work any more.  The device
// is drained, so what growth and destroyed objects retired can be freed; the staging threads end before the pinned memory they
// copy into goes; then the members let go of what they own (device_owners.h) -- on a drained device, in whatever order they
// are declared.
void free_device(device_state* d) {
    if (d->device >= 0) {
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();
        free_retired(*d);
        d->stagers.reset();
    }
    delete d;
}

int load_rccl() {
    rccl_api& r = L.rccl;
    if (r.handle) return JJS_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(JJS_ERR_COLLECTIVE, "cannot load RCCL: %s", dlerror());
    r.CommInitAll = (decltype(r.CommInitAll))dlsym(h, "ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(h, "ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllReduce || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
        dlclose(h);
        r = rccl_api{};
        return fail(JJS_ERR_COLLECTIVE, "RCCL library lacks a required symbol");
    }
    r.handle = h;
    return JJS_OK;
}

// One communicator per driven device, all in this process (ranks = positions in L.devs).
int start_comms() {
    if (int rc = load_rccl()) return rc;
    int ords[MAX_DEVICES];
    for (size_t i = 0; i < L.devs.size(); ++i) ords[i] = L.devs[i]->device;
    RCCL_TRY(L.rccl.CommInitAll(L.comms, (int)L.devs.size(), ords));
    L.comms_up = true;
    return JJS_OK;
}

// Sum of the 4-counter tallies over the driven devices, in place in every device's buffer; queued on each
// device's stream behind the launch that produced the counters (the only collective).
int allreduce_tallies() {
    RCCL_TRY(L.rccl.GroupStart());
    for (size_t i = 0; i < L.devs.size(); ++i) {
        device_state& d = *L.devs[i];
        ncclResult_t r = L.rccl.AllReduce(d.tally, d.tally, 4, ncclUint64, ncclSum, L.comms[i], d.stream);
        if (r != ncclSuccess) {
            (void)L.rccl.GroupEnd();
            return fail(JJS_ERR_COLLECTIVE, "ncclAllReduce: %s", L.rccl.GetErrorString(r));
        }
    }
    RCCL_TRY(L.rccl.GroupEnd());
    return JJS_OK;
}

void shutdown_locked() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    g_keysets.retire_all();
    g_msig_groups.retire_all();
    for (device_state* d : L.devs)
        if (d->stream) { (void)hipSetDevice(d->device); (void)hipStreamSynchronize(d->stream); }
    if (L.comms_up) {
        for (size_t i = 0; i < L.devs.size(); ++i) (void)L.rccl.CommDestroy(L.comms[i]);
        L.comms_up = false;
    }
    for (device_state* d : L.devs) free_device(d);
    L.devs.clear();
    L.virtual_devices = false;
    g = nullptr;
    if (prev >= 0) (void)hipSetDevice(prev);
}

struct device_restore {   // puts the calling thread back on the device it came in with
    int prev = -1;
    device_restore() { (void)hipGetDevice(&prev); }
    ~device_restore() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- the staged_call of every scheme and input format --------------------------------------------------------------
// The shape of every verification entry point: its columns in the order of the entry point's arguments -- width in bytes, the
// group that decides when a large host-buffer call uploads the column (host_calls.h), and what the column is.  This table is
// the only place that knows an entry point's argument order.
enum col_role : uint8_t {
    COL_SCALAR,        // u, 32 bytes
    COL_R,             // an R point, affine or extended
    COL_KEY,           // a key point (the generator of a var-gen signature is one), affine or extended
    COL_MESSAGE,       // m, 32 bytes
    COL_SIG_WIRE,      // u || R (|| R'), 32 bytes each: the R points are decoded per item
    COL_KEYS_WIRE,     // pk (|| pk' or the generator), 32 bytes each: decoded per key or per item (job_keys / job_hash)
};
struct call_shape {
    int scheme, format;
    size_t n_cols;
    struct { size_t width; uint32_t group; col_role role; } col[8];
    int wire_points;              // R points per signature that a wire call decodes per item
};
const call_shape SHAPES[3][3] = {       // [JJS_SCHEME_*][JJS_FORMAT_*]
    {{JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, 4, {{32, COLS_LATE, COL_SCALAR}, {64, COLS_REST, COL_R}, {64, COLS_KEYS, COL_KEY}, {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_SINGLE, JJS_FORMAT_EXT, 4, {{32, COLS_LATE, COL_SCALAR}, {96, COLS_REST, COL_R}, {96, COLS_KEYS, COL_KEY}, {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_SINGLE, JJS_FORMAT_WIRE, 3, {{64, COLS_REST, COL_SIG_WIRE}, {32, COLS_KEYS, COL_KEYS_WIRE}, {32, COLS_REST, COL_MESSAGE}}, 1}},
    {{JJS_SCHEME_DOUBLE, JJS_FORMAT_AFFINE, 6, {{32, COLS_LATE, COL_SCALAR}, {64, COLS_REST, COL_R}, {64, COLS_REST, COL_R}, {64, COLS_KEYS, COL_KEY},
                                               {64, COLS_KEYS, COL_KEY}, {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_DOUBLE, JJS_FORMAT_EXT, 6, {{32, COLS_LATE, COL_SCALAR}, {96, COLS_REST, COL_R}, {96, COLS_REST, COL_R}, {96, COLS_KEYS, COL_KEY},
                                            {96, COLS_KEYS, COL_KEY}, {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_DOUBLE, JJS_FORMAT_WIRE, 3, {{96, COLS_REST, COL_SIG_WIRE}, {64, COLS_KEYS, COL_KEYS_WIRE}, {32, COLS_REST, COL_MESSAGE}}, 2}},
    {{JJS_SCHEME_VARGEN, JJS_FORMAT_AFFINE, 5, {{32, COLS_LATE, COL_SCALAR}, {64, COLS_REST, COL_R}, {64, COLS_KEYS, COL_KEY}, {64, COLS_KEYS, COL_KEY},
                                               {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_VARGEN, JJS_FORMAT_EXT, 5, {{32, COLS_LATE, COL_SCALAR}, {96, COLS_REST, COL_R}, {96, COLS_KEYS, COL_KEY}, {96, COLS_KEYS, COL_KEY},
                                            {32, COLS_REST, COL_MESSAGE}}, 0},
     {JJS_SCHEME_VARGEN, JJS_FORMAT_WIRE, 3, {{64, COLS_REST, COL_SIG_WIRE}, {64, COLS_KEYS, COL_KEYS_WIRE}, {32, COLS_REST, COL_MESSAGE}}, 1}},
};

// A slot's wire area (call_slot::wire; WIRE_ITEM_BYTES per item of its capacity): where its parts begin.
uint8_t* wire_pts(int k) { return sl->wire + (size_t)k * sl->wire.capacity() * 64; }
uint8_t* wire_bad() { return sl->wire + sl->wire.capacity() * WIRE_FLAGS_AT; }
uint32_t* wire_scratch(int k) { return reinterpret_cast<uint32_t*>(sl->wire + sl->wire.capacity() * (WIRE_SCRATCH_AT + WIRE_SCRATCH_BYTES * k)); }

// the scheme's verification descriptor over affine columns (Rp, PK2: the columns the scheme has; PK2 of a var-gen call: the generator)
verify_params scheme_params(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PK2,
                            const uint8_t* m, size_t n, const out_ptrs& o) {
    if (scheme == JJS_SCHEME_SINGLE) return params_single(u, R, PK, m, n, g->comb_g, o);
    if (scheme == JJS_SCHEME_DOUBLE) return params_double(u, R, Rp, PK, PK2, m, n, g->tag, g->comb_g, g->comb_gn, o);
    return params_vargen(u, R, PK, PK2, m, n, o);
}

// Builds the call of shape S from the device arrays d[0..] (in the order of the entry point's arguments): picks the call slot,
// sizes what the format needs in it and fills in the descriptors.  Resident calls launch it at once (launch_staged), host-buffer
// calls feed it piece by piece (run_host_block).
// Points that are converted on the device land in wire_pts(k), the R points ahead of the keys: extended coordinates (U, V, Z)
// are normalised (N[grp]: the columns of that group), compressed R points are decoded per item (W.sig) and compressed keys per
// key or per item (W.comp); the flags of rejected encodings are P.pre_malformed.  The descriptor then reads affine columns.
int build_call(const call_shape& S, const void* const* d, size_t n, void* status, void* tally, hipStream_t s, staged_call& C) {
    for (size_t k = 0; k < S.n_cols; ++k)
        if (n && !all_ok(d[k])) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    pick_slot(n, s);
    const bool affine = S.format == JJS_FORMAT_AFFINE;
    if (!affine)
        if (int rc = sl->wire.ensure(n)) return rc;
    C = staged_call{};
    const uint8_t *u = nullptr, *m = nullptr, *R[2] = {}, *PK[2] = {};
    uint32_t n_r = 0, n_pk = 0, sig_width = 0;
    for (size_t k = 0; k < S.n_cols; ++k) {
        const uint8_t* const p = (const uint8_t*)d[k];
        const uint32_t width = (uint32_t)S.col[k].width;
        switch (S.col[k].role) {
        case COL_SCALAR: u = p; break;
        case COL_MESSAGE: m = p; break;
        case COL_R: case COL_KEY: {
            const uint8_t* point = p;
            if (!affine) {                // normalised into the next wire column, with the other columns of its group
                uint8_t* const out = wire_pts((int)(n_r + n_pk));
                for (uint32_t grp = COLS_KEYS; grp <= COLS_ALL; ++grp) {
                    normalize_params& N = C.N[grp];
                    if (!(S.col[k].group & grp)) continue;
                    N.src[N.n_src] = fe_src{p, width, 0};
                    N.out[N.n_src] = out;
                    ++N.n_src;
                }
                point = out;
            }
            (S.col[k].role == COL_R ? R[n_r++] : PK[n_pk++]) = point;
            break;
        }
        case COL_SIG_WIRE:
            u = p; sig_width = width;
            for (; n_r < (uint32_t)S.wire_points; ++n_r) {
                C.W.sig.src[n_r] = fe_src{p, width, 32 + 32 * n_r};
                C.W.sig.out[n_r] = wire_pts((int)n_r);
                R[n_r] = wire_pts((int)n_r);
            }
            break;
        case COL_KEYS_WIRE:
            for (; n_pk < width / 32; ++n_pk) {
                C.W.comp[n_pk] = fe_src{p, width, 32 * n_pk};
                C.W.out[n_pk] = wire_pts((int)(n_r + n_pk));
                PK[n_pk] = wire_pts((int)(n_r + n_pk));
            }
            C.W.n_cols = n_pk;
            break;
        }
    }
    C.P = scheme_params(S.scheme, u, R[0], R[1], PK[0], PK[1], m, n, out_ptrs{(uint8_t*)status, (unsigned long long*)tally, nullptr, sl->workspace});
    if (S.format == JJS_FORMAT_EXT) {
        C.ext = true;
        for (uint32_t grp = COLS_KEYS; grp <= COLS_ALL; ++grp) {
            C.N[grp].bad = wire_bad();
            C.N[grp].scratch = wire_scratch(grp == COLS_KEYS ? 1 : 0);
        }
        C.P.pre_malformed = wire_bad();
    } else if (S.format == JJS_FORMAT_WIRE) {
        C.wire = true;
        C.W.sig.n_src = n_r; C.W.sig.n = n; C.W.sig.bad = wire_bad();
        C.W.bad = wire_bad();
        C.P.u = fe_src{u, sig_width, 0};
        C.P.pre_malformed = wire_bad();
        C.P.decoded_points = 1;
    }
    return JJS_OK;
}

#include "host_calls.h"

}  // namespace

extern "C" {

#if defined(JJS_LANE_TRACE)
static void lane_trace_dump();     // host_lanes.h, investigation builds
#endif
int jjs_abi_version(void) { return 5; }
const char* jjs_last_error(void) { return t_err; }

int jjs_init(int device_count) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (device_count < 0 || device_count > MAX_DEVICES)
        return fail(JJS_ERR_ARG, "device_count must be in [0, %d] (got %d)", MAX_DEVICES, device_count);
    int visible = 0, current = -1;
    HIP_TRY(hipGetDeviceCount(&visible));
    HIP_TRY(hipGetDevice(&current));
    if (visible < 1) return fail(JJS_ERR_HIP, "no HIP device visible");
#if defined(JJS_PROFILING)
    const bool allow_virtual = g_allow_virtual;   // logical devices sharing one card: test builds only
#else
    const bool allow_virtual = false;
#endif
    const int want = device_count == 0 ? visible : device_count;
    if (!L.devs.empty()) {   // idempotent for the same request
        if (device_count == 1) return check_ready();
        if ((size_t)want == L.devs.size()) return JJS_OK;
        return fail(JJS_ERR_ARG, "already initialised with %zu device(s); call jjs_shutdown first", L.devs.size());
    }
    if (want > visible && !allow_virtual)
        return fail(JJS_ERR_ARG, "device_count=%d but only %d HIP device(s) are visible", want, visible);
    L.virtual_devices = want > visible;
    for (int i = 0; i < want; ++i) {
        device_state* d = new device_state();
        L.devs.push_back(d);
        int rc = init_device(*d, device_count == 1 ? current : i % visible);
        if (rc) { shutdown_locked(); (void)hipSetDevice(current); return rc; }
    }
    HIP_TRY(hipSetDevice(current));
    if (L.devs.size() > 1 && !L.virtual_devices) {
        int rc = start_comms();
        if (rc) { shutdown_locked(); return rc; }
    }
    return JJS_OK;
}

void jjs_shutdown(void) {
    {   // a large host-buffer call in progress finishes first (it holds its device's host_mu, not the engine's mutex)
        std::vector<device_state*> devs;
        { std::lock_guard<std::mutex> lock(L.mu); devs = L.devs; }
        for (device_state* d : devs) { std::lock_guard<std::mutex> big(d->host_mu); }
    }
    std::unique_lock<std::mutex> lock(L.mu);
    // host-buffer calls that hold a lane finish first (they wait for the device outside the mutex)
    L.lane_cv.wait(lock, [] {
        if (g_blocking_calls) return false;             // blocking calls that hold a device pointer outside the mutex
        for (device_state* d : L.devs)
            for (const host_lane& l : d->lanes)
                if (l.state != host_lane::FREE) return false;
        return true;
    });
    shutdown_locked();
    L.lane_cv.notify_all();
#if defined(JJS_LANE_TRACE)
    lane_trace_dump();
#endif
}

int jjs_device_count(void) {
    std::lock_guard<std::mutex> lock(L.mu);
    return (int)L.devs.size();
}

int jjs_collective_ranks(void) {
    std::lock_guard<std::mutex> lock(L.mu);
    return L.comms_up ? (int)L.devs.size() : 0;
}

int jjs_stream_sync(void* stream) {
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (L.devs.empty()) return fail(JJS_ERR_NOT_INIT, "jjs_init has not been called");
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));     // waits without holding the engine's mutex
    return JJS_OK;
}

// a resident call: device pointers d[], asynchronous on `stream`
static int resident_call(const call_shape& S, const void* const* d, size_t n, void* status, void* tally, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (status && !aligned16(status)) return fail(JJS_ERR_ARG, "status must be 16-byte aligned");
    if (n == 0) {
        if (tally) HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(unsigned long long), s));
        return JJS_OK;
    }
    staged_call C;
    if (int rc = build_call(S, d, n, status, tally, s, C)) return rc;
    return launch_staged(C, s);
}

#include "host_lanes.h"
#include "keyset_calls.h"
#include "keyset_add_calls.h"
#include "keyset_remove_calls.h"
#include "points_check_calls.h"

// a host-buffer call: blocking
static int host_call(int scheme, int format, const uint8_t* const* ptrs, size_t n, uint8_t* status, uint64_t tally[4]) {
    const call_shape& S = SHAPES[scheme][format];
    for (size_t k = 0; k < S.n_cols; ++k)
        if (n && !ptrs[k]) return fail(JJS_ERR_ARG, "null input pointer");
    bool one_device = false;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        one_device = L.devs.size() == 1;
    }
    if (n == 0) {
        if (tally) for (int k = 0; k < 4; ++k) tally[k] = 0;
        return JJS_OK;
    }
    if (one_device && n <= LANE_MAX_ITEMS) return lane_call(scheme, format, ptrs, n, status, tally);
    if (one_device) {
        // A large call fills the device by itself: such calls run one at a time per device (host_mu; they share the device's
        // staging), but outside the engine's mutex, which they take only to pick their slot -- other threads' calls are queued
        // meanwhile.  (jjs_shutdown and jjs_trim take host_mu, too.)
        device_state* dev = nullptr;
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (int rc = check_ready()) return rc;
            dev = g;
        }
        std::lock_guard<std::mutex> big(dev->host_mu);
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (L.devs.empty() || check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine was shut down during the call");
        }
        return no_throw([&] { return run_host(S, ptrs, n, status, tally, true); });
    }
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    return no_throw([&] { return run_host(S, ptrs, n, status, tally); });
}

// ---- affine inputs: device-buffer and host-buffer entry points ----------------------------------------------
int jjs_verify_single_dev(const void* u, const void* R, const void* PK, const void* m, size_t n, void* status,
                          void* tally, void* stream) {
    const void* d[] = {u, R, PK, m};
    return resident_call(SHAPES[JJS_SCHEME_SINGLE][JJS_FORMAT_AFFINE], d, n, status, tally, stream);
}
int jjs_verify_double_dev(const void* u, const void* R, const void* Rp, const void* PK, const void* PKp, const void* m,
                          size_t n, void* status, void* tally, void* stream) {
    const void* d[] = {u, R, Rp, PK, PKp, m};
    return resident_call(SHAPES[JJS_SCHEME_DOUBLE][JJS_FORMAT_AFFINE], d, n, status, tally, stream);
}
int jjs_verify_vargen_dev(const void* u, const void* R, const void* PK, const void* Gen, const void* m, size_t n,
                          void* status, void* tally, void* stream) {
    const void* d[] = {u, R, PK, Gen, m};
    return resident_call(SHAPES[JJS_SCHEME_VARGEN][JJS_FORMAT_AFFINE], d, n, status, tally, stream);
}
int jjs_verify_single(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* m, size_t n,
                      uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, PK, m};
    return host_call(JJS_SCHEME_SINGLE, JJS_FORMAT_AFFINE, p, n, status, tally);
}
int jjs_verify_double(const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PKp,
                      const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, Rp, PK, PKp, m};
    return host_call(JJS_SCHEME_DOUBLE, JJS_FORMAT_AFFINE, p, n, status, tally);
}
int jjs_verify_vargen(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* Gen, const uint8_t* m,
                      size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, PK, Gen, m};
    return host_call(JJS_SCHEME_VARGEN, JJS_FORMAT_AFFINE, p, n, status, tally);
}

// ---- one verdict per batch (batch_verdict.h) -------------------------------------------------------------------
#include "verdict_calls.h"
#include "keyset_verdict_calls.h"

// ---- wire formats: on-device decoding, then the same verify kernels -----------------------------------
int jjs_verify_single_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally, void* stream) {
    const void* d[] = {sig, pk, m};
    return resident_call(SHAPES[JJS_SCHEME_SINGLE][JJS_FORMAT_WIRE], d, n, status, tally, stream);
}
int jjs_verify_double_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally, void* stream) {
    const void* d[] = {sig, pk, m};
    return resident_call(SHAPES[JJS_SCHEME_DOUBLE][JJS_FORMAT_WIRE], d, n, status, tally, stream);
}
int jjs_verify_vargen_wire_dev(const void* sig, const void* pk, const void* m, size_t n, void* status, void* tally, void* stream) {
    const void* d[] = {sig, pk, m};
    return resident_call(SHAPES[JJS_SCHEME_VARGEN][JJS_FORMAT_WIRE], d, n, status, tally, stream);
}
int jjs_verify_single_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {sig, pk, m};
    return host_call(JJS_SCHEME_SINGLE, JJS_FORMAT_WIRE, p, n, status, tally);
}
int jjs_verify_double_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {sig, pk, m};
    return host_call(JJS_SCHEME_DOUBLE, JJS_FORMAT_WIRE, p, n, status, tally);
}
int jjs_verify_vargen_wire(const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {sig, pk, m};
    return host_call(JJS_SCHEME_VARGEN, JJS_FORMAT_WIRE, p, n, status, tally);
}

// ---- extended coordinates (U, V, Z): normalised on the device, then the same verify kernels -----------------
int jjs_verify_single_ext_dev(const void* u, const void* R, const void* PK, const void* m, size_t n, void* status, void* tally,
                              void* stream) {
    const void* d[] = {u, R, PK, m};
    return resident_call(SHAPES[JJS_SCHEME_SINGLE][JJS_FORMAT_EXT], d, n, status, tally, stream);
}
int jjs_verify_double_ext_dev(const void* u, const void* R, const void* Rp, const void* PK, const void* PKp, const void* m,
                              size_t n, void* status, void* tally, void* stream) {
    const void* d[] = {u, R, Rp, PK, PKp, m};
    return resident_call(SHAPES[JJS_SCHEME_DOUBLE][JJS_FORMAT_EXT], d, n, status, tally, stream);
}
int jjs_verify_vargen_ext_dev(const void* u, const void* R, const void* PK, const void* Gen, const void* m, size_t n,
                              void* status, void* tally, void* stream) {
    const void* d[] = {u, R, PK, Gen, m};
    return resident_call(SHAPES[JJS_SCHEME_VARGEN][JJS_FORMAT_EXT], d, n, status, tally, stream);
}
int jjs_verify_single_ext(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* m, size_t n, uint8_t* status,
                          uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, PK, m};
    return host_call(JJS_SCHEME_SINGLE, JJS_FORMAT_EXT, p, n, status, tally);
}
int jjs_verify_double_ext(const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* PK, const uint8_t* PKp,
                          const uint8_t* m, size_t n, uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, Rp, PK, PKp, m};
    return host_call(JJS_SCHEME_DOUBLE, JJS_FORMAT_EXT, p, n, status, tally);
}
int jjs_verify_vargen_ext(const uint8_t* u, const uint8_t* R, const uint8_t* PK, const uint8_t* Gen, const uint8_t* m, size_t n,
                          uint8_t* status, uint64_t tally[4]) {
    const uint8_t* p[] = {u, R, PK, Gen, m};
    return host_call(JJS_SCHEME_VARGEN, JJS_FORMAT_EXT, p, n, status, tally);
}

// ---- pre-sizing and trimming ------------------------------------------------------------------------------------
// What a call of this shape and size would allocate on first use, allocated now, in EVERY slot (and lane) such a call can
// land in: a service calls this once per call shape at start-up and no later call of at most that size allocates.
// BESIDE LIVE CALLS it replaces nothing a call uses outside the engine's mutex:
//   - a lane that is not FREE keeps its areas and grows at its next open (host_lanes.h reserve_lane);
//   - a large host-buffer call (one device: run_host under host_mu) reads the device's staging anew for every piece, and sizes and
//     feeds the slot it owns -- a medium or the second big one -- without the mutex: a reserve that reaches either, i.e. one of
//     more items than a lane or a small slot takes, holds host_mu of every device first, in jjs_trim's order.  It then waits for
//     such a call in progress to return, never for the device: nothing here synchronises or frees.
int jjs_reserve(int scheme, int format, size_t n_items, int host_buffers) {
    std::vector<device_state*> devs;
    std::vector<std::unique_lock<std::mutex>> big;
    if (n_items > (LANE_MAX_ITEMS < SMALL_SLOT_ITEMS ? LANE_MAX_ITEMS : SMALL_SLOT_ITEMS)) {
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (int rc = check_ready()) return rc;
            devs = L.devs;
        }
        try { for (device_state* d : devs) big.emplace_back(d->host_mu); } catch (...) { return fail(JJS_ERR_HIP, "host-side failure"); }
    }
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!big.empty() && devs != L.devs) return fail(JJS_ERR_NOT_INIT, "the engine was re-initialised during the call");
    if (scheme < 0 || scheme > 2 || format < 0 || format > 2) return fail(JJS_ERR_ARG, "scheme / format out of range");
    if (n_items == 0) return JJS_OK;
    const call_shape& S = SHAPES[scheme][format];
    struct unforce { ~unforce() { forced_slot = nullptr; } } unforce_on_every_way_out;
    return no_throw([&]() -> int {
        device_restore restore;
        std::vector<device_state*> targets;
        if (L.devs.size() == 1 || !host_buffers) targets.push_back(g); else targets = L.devs;
        size_t per = host_buffers ? (n_items + targets.size() - 1) / targets.size() : n_items;
        // small host-buffer calls combine: the launch their slot sees may carry up to COMBINE_CAP_ITEMS items
        const size_t call_items = per;
        if (host_buffers && targets.size() == 1 && per <= COMBINE_MAX_CALL_ITEMS) per = COMBINE_CAP_ITEMS;
        for (device_state* d : targets) {
            g = d;
            HIP_TRY(hipSetDevice(d->device));
            int lo, hi;
            if (per <= SMALL_SLOT_ITEMS) { lo = 1; hi = N_SMALL_SLOTS; }
            else if (per <= MEDIUM_SLOT_ITEMS) { lo = 1 + N_SMALL_SLOTS; hi = N_SMALL_SLOTS + N_MEDIUM_SLOTS; }
            else { lo = 0; hi = SECOND_BIG_SLOT; }
            for (int i = lo; i <= hi; ++i) {
                if (lo == 0 && i != 0 && i != SECOND_BIG_SLOT) continue;
                forced_slot = &d->slots[i];
                // the builder sizes what the format needs in the slot; its descriptors (built from a placeholder address,
                // never dereferenced) tell which path the call would take
                const void* in[8];
                for (size_t k = 0; k < S.n_cols; ++k) in[k] = reinterpret_cast<const void*>(uintptr_t(4096));
                staged_call C;
                int rc = build_call(S, in, per, nullptr, nullptr, nullptr, C);
                forced_slot = nullptr;
                if (rc) return rc;
                if (int r = reserve_for(C.P)) return r;
            }
            if (host_buffers) {
                if (targets.size() == 1 && per <= LANE_MAX_ITEMS) {
                    const lane_layout Y = lane_layout_for(S, lane_cap_for(nullptr, scheme, format, call_items));
                    for (host_lane& l : d->lanes)
                        if (int r = reserve_lane(l, Y.total)) return r;
                } else {
                    if (int r = reserve_host_block(S, per)) return r;
                }
            }
        }
        g = targets[0];
        return JJS_OK;
    });
}
// Waits for the devices to go idle, then frees what growth has retired and every slot's key-table pool (a later call that
// takes the key tables allocates its pool again, at the size the slot had learnt).
int jjs_trim(void) {
    std::vector<device_state*> devs;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        devs = L.devs;
    }
    std::vector<std::unique_lock<std::mutex>> big;            // no large host-buffer call in progress on any device
    for (device_state* d : devs) big.emplace_back(d->host_mu);
    std::unique_lock<std::mutex> lock(L.mu);
    // a key set that grows in place may have been destroyed meanwhile: what it still writes is not freed under it (keyset_add_calls.h)
    L.lane_cv.wait(lock, [] { return g_keyset_grows == 0; });
    if (int rc = check_ready()) return rc;
    if (devs != L.devs) return fail(JJS_ERR_NOT_INIT, "the engine was re-initialised during the call");
    device_restore restore;
    for (device_state* d : L.devs) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipDeviceSynchronize());
        free_retired(*d);
        HIP_TRY(d->sign_tables.free());                        // the tables of a signing call's shared generator
        HIP_TRY(d->sign_key.free());                           // the key record of a signing call with one key
        HIP_TRY(d->digest_scratch.free());                     // the offsets and the order of a ragged digest call
        HIP_TRY(d->msig_stage.free());                         // the staging of the host-buffer multisig calls (host_mu is held)
        for (call_slot& c : d->slots) {
            if (!c.key_pool) continue;
            if (c.key_pool.bytes() > c.key_pool_want) c.key_pool_want = c.key_pool.bytes();
            HIP_TRY(c.key_pool.free());
            HIP_TRY(c.key_memo.free());                        // the memo goes with the tables it describes
            c.memo_cap = 0; c.memo_flush = true;
        }
    }
    return JJS_OK;
}
int jjs_memory_stats(uint64_t out[JJS_MEMORY_STATS]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    uint64_t pool = 0, slots = 0, lanes = 0;
    for (const call_slot& c : g->slots) {
        pool += c.key_pool.bytes() + c.key_memo.bytes();
        slots += c.pending.reported_bytes() + c.prep.reported_bytes() + c.wire.reported_bytes() + c.small.reported_bytes() + c.keys.reported_bytes() +
                 c.verdict.reported_bytes() + c.found.reported_bytes();
    }
    for (const host_lane& l : g->lanes) lanes += l.dev.reported_bytes() + l.pinned.reported_bytes();
    out[JJS_MEMORY_KEY_POOLS] = pool;
    out[JJS_MEMORY_SLOT_BUFFERS] = slots + g->sign_tables.reported_bytes() + g->sign_key.reported_bytes() + g->digest_scratch.reported_bytes();
    out[JJS_MEMORY_HOST_STAGING] = lanes + g->stage.reported_bytes() + g->pinned.reported_bytes() + g->msig_stage.reported_bytes();
    out[JJS_MEMORY_RETIRED] = g->retired_bytes;
    return JJS_OK;
}

// Which method the calls on the current device took (include/jjs_gpu.h).  Calls that tried the key tables are counted
// when the library next looks at their slot (their decision is made on the device): after the stream has drained,
// every finished call is in.
int jjs_path_stats(uint64_t out[JJS_PATH_STATS]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    size_t pool = 0;
    for (call_slot& c : g->slots) {
        sl = &c;
        if (c.key_stream && !c.host_owned) note_key_feedback();     // (a slot a large host-buffer call is feeding: counted by that call's successor)
        pool += c.key_pool.bytes();
    }
    for (int i = 0; i < JJS_PATH_STATS; ++i) out[i] = g->stats[i];
    out[JJS_PATH_KEY_POOL_BYTES] = pool;
    return JJS_OK;
}

static int launch_decode(decode_params D, hipStream_t s) {
    D.dlog = dlog_tables{g->dlog_pow, g->dlog_hash};
    if (int rc = begin_shared(s)) return rc;
    size_t blocks = (D.n + BLOCK - 1) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, D);
    HIP_TRY(hipGetLastError());
    return end_shared(s);
}

int jjs_decompress_dev(const void* in, size_t n, void* affine_out, void* ok_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(in, affine_out) || !ok_out) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    decode_params D{};
    D.n_src = 1; D.n = n; D.ok = (uint8_t*)ok_out;
    D.src[0] = fe_src{(const uint8_t*)in, 32, 0}; D.out[0] = (uint8_t*)affine_out;
    big_slot();
    return launch_decode(D, (hipStream_t)stream);
}
int jjs_compress_dev(const void* affine, size_t n, void* out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(affine, out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipLaunchKernelGGL(compress_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t*)affine, (uint64_t)n, (uint8_t*)out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}

// ---- multisig: batch verify_share / combine -------------------------------------------
// The device's multisignature scratch (g->msig, grow-only, holding room for g->msig_held): msig_scratch.h has its regions and its
// growth.  It belongs to slot 0.
static int ensure_msig_scratch(const msig_caps& need) {
    const msig_caps caps = msig_caps_grown(g->msig_held, need);
    if (caps == g->msig_held) return JJS_OK;
    device_mem<uint8_t> fresh;
    HIP_TRY(fresh.alloc(msig_scratch_layout(nullptr, caps).bytes));
    g->msig.replace(std::move(fresh));
    g->msig_held = caps;
    return JJS_OK;
}
extern "C++" {
// The frame of a call on device columns over the scratch, on stream s (under the engine's mutex, g the device): queue(W) queues the
// call's work given the carved scratch.  What a call refuses, it refuses before it comes here.
template <class Queue>
static int msig_scratch_call(const msig_caps& need, hipStream_t s, Queue&& queue) {
    if (int rc = ensure_msig_scratch(need)) return rc;
    const msig_scratch W = msig_scratch_layout(g->msig.get(), g->msig_held).W;
    big_slot();
    if (int rc = begin_shared(s)) return rc;
    const int rc = queue(W);
    sl = &g->slots[0];                          // the scratch's slot again, should the call have moved on (msig_verify_calls.h)
    const int rc2 = end_shared(s);              // the slot's event covers whatever was queued, also when a step failed
    return rc ? rc : rc2;
}
// What the calls over the scratch set alike in their msig_params.  a_c false: a verifier's call, which computes neither a nor c and
// leaves their words unset -- as every field a call does not set stays: the kernels read those as flags.
static void msig_params_common(msig_params& P, const msig_scratch& W, size_t n_transcripts, size_t n, bool a_c = true) {
    P.n_transcripts = (uint32_t)n_transcripts; P.n_total = n;
    P.tr_of = W.tr_of; P.d_words = W.d_words; P.dpk = W.dpk; P.offsets = W.offsets;
    if (a_c) { P.a_words = W.a_words; P.c_words = W.c_words; }
    P.tags = g->tags_long; P.comb_g = g->comb_g; P.lane_ws = g->slots[0].workspace;
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = W.long_tags;
}
// the key-set fields of a call against copy c of set k; `refused`: the word of every transcript that the gather flags
static void msig_keyset_fill(msig_keyset_params& K, const keyset_entry& k, const keyset_copy& c, const void* key_idx, const msig_scratch& W,
                             uint32_t* refused) {
    K.key_idx = (const uint32_t*)key_idx; K.n_keys = k.n_keys;
    K.keys = c.keys[0]; K.flags = c.flags[0]; K.tables = c.tables[0];
    K.pk_col = W.ks_pk; K.row_key = W.ks_row_key; K.refused = refused;
}
// the signer-group fields (of msig_group_params, msig_share_params) of a call against copy c of group k
template <class Params>
static void msig_group_fill(Params& G, const msig_group_entry& k, const msig_group_copy& c) {
    G.participants = k.participants;
    G.d_words = c.d_words; G.tables = c.tables; G.tag_a = c.tag_a + 9;
}
}  // extern "C++"
// The normalisation in front of the passes of an extended call: `cols` columns of n rows (96 bytes a point) into the scratch's
// normalised columns, one item per row, in poison mode; col[] is re-aimed at the normalised columns.
static int msig_normalize(const msig_scratch& W, const uint8_t** col, uint32_t cols, size_t n, hipStream_t s) {
    normalize_params N{};
    N.n_src = cols; N.poison = 1; N.scratch = W.prefix;
    for (uint32_t k = 0; k < cols; ++k) {
        N.src[k] = fe_src{col[k], 96, 0};
        N.out[k] = W.norm[k];
        col[k] = W.norm[k];
    }
    return launch_normalize(N, 0, n, n, s);
}
// The decoding in front of the passes of a wire call: `cols` columns of n rows (32 bytes a point, column k at src[k]) into out[k],
// one lane per (row, column), in poison mode (decode.h).
static int launch_msig_decode(msig_decode_params D, size_t n, hipStream_t s) {
    if (!D.n_src || !n) return JJS_OK;
    D.n = n;
    D.dlog = dlog_tables{g->dlog_pow, g->dlog_hash};
    hipLaunchKernelGGL(msig_decode_kernel, dim3((unsigned)grid_for(8192, n * D.n_src)), dim3(BLOCK), 0, s, D);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
// ... of packed columns into the scratch's normalised columns; col[] is re-aimed at them (the contract of msig_normalize).
static int msig_decode(const msig_scratch& W, const uint8_t** col, uint32_t cols, size_t n, hipStream_t s) {
    msig_decode_params D{};
    D.n_src = cols;
    for (uint32_t k = 0; k < cols; ++k) {
        D.src[k] = fe_src{col[k], 32, 0};
        D.out[k] = W.norm[k];
        col[k] = W.norm[k];
    }
    return launch_msig_decode(D, n, s);
}
// the point columns of a call in format fmt (JJS_FORMAT_*) made affine in the scratch; an affine call keeps its columns
static int msig_ingest(int fmt, const msig_scratch& W, const uint8_t** col, uint32_t cols, size_t n, hipStream_t s) {
    if (fmt == JJS_FORMAT_EXT) return msig_normalize(W, col, cols, n, s);
    if (fmt == JJS_FORMAT_WIRE) return msig_decode(W, col, cols, n, s);
    return JJS_OK;
}
// n = the shares of a call whose host offsets are acceptable
static int msig_check_offsets(const uint32_t* offsets_host, size_t n_transcripts, size_t& n) {
    if (!offsets_host || offsets_host[0] != 0) return fail(JJS_ERR_ARG, "offsets must start at 0");
    // A transcript takes any number of participants: none is the reference's InvalidMultisigTranscript (status 5 for that
    // transcript, the others are not affected), and beyond the JJS_MSIG_MAX_PARTICIPANTS the tag table covers the two
    // SAFE tags of the transcript are computed by the first pass on the device (csrc/safe_tag.h).
    for (size_t t = 0; t < n_transcripts; ++t) {
        if (offsets_host[t + 1] < offsets_host[t]) return fail(JJS_ERR_ARG, "transcript %zu: offsets must not decrease", t);
        const uint64_t cnt = offsets_host[t + 1] - offsets_host[t];
        if (cnt > JJS_MSIG_PARTICIPANTS_LIMIT)
            return fail(JJS_ERR_ARG, "transcript %zu: %llu participants (the hash transcripts are indexed with 32 bits: at most %u)", t,
                        (unsigned long long)cnt, (unsigned)JJS_MSIG_PARTICIPANTS_LIMIT);
    }
    n = offsets_host[n_transcripts];
    return JJS_OK;
}
// The call on device columns, queued on s (under the engine's mutex, g the device; n_transcripts > 0).  fmt (JJS_FORMAT_*): PK, R, S are
// N x 64, N x 96 or N x 32.
static int msig_combine_locked(int fmt, const void* z, const void* PK, const void* R, const void* S, const void* m,
                               const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                               void* agg_pk, void* sig_u, void* sig_R, hipStream_t s) {
    size_t n = 0;
    if (int rc = msig_check_offsets(offsets_host, n_transcripts, n)) return rc;
    if ((n && !all_ok(z, PK, R, S)) || !all_ok(m, agg_pk, sig_u, sig_R) || (n && !share_status)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    msig_caps need;
    need.rows = n; need.transcripts = n_transcripts;
    if (fmt != JJS_FORMAT_AFFINE) need.ext_rows = n;
    return msig_scratch_call(need, s, [&](const msig_scratch& W) -> int {
        const uint8_t* pts[3] = {(const uint8_t*)PK, (const uint8_t*)R, (const uint8_t*)S};
        msig_params P{};
        msig_params_common(P, W, n_transcripts, n);
        P.z = (const uint8_t*)z; P.m = (const uint8_t*)m;
        P.share_status = (uint8_t*)share_status; P.agg_pk = (uint8_t*)agg_pk; P.sig_u = (uint8_t*)sig_u; P.sig_R = (uint8_t*)sig_R;
        P.transcript_status = (uint8_t*)transcript_status;
        P.e_pt = W.e_pt;
        HIP_TRY(hipMemcpyAsync(W.offsets, offsets_host, (n_transcripts + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (int rc = msig_ingest(fmt, W, pts, 3, n, s)) return rc;
        P.PK = pts[0]; P.R = pts[1]; P.S = pts[2];
        for (int pass = 0; pass < 7; ++pass) launch_msig_pass(P, pass, s);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}
// the three formats of jjs_multisig_combine*_dev
static int msig_combine_dev(int fmt, const void* z, const void* PK, const void* R, const void* S, const void* m, const uint32_t* offsets_host,
                            size_t n_transcripts, void* share_status, void* transcript_status, void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n_transcripts == 0) return JJS_OK;
    return msig_combine_locked(fmt, z, PK, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R,
                               (hipStream_t)stream);
}
int jjs_multisig_combine_dev(const void* z, const void* PK, const void* R, const void* S, const void* m,
                             const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                             void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_combine_dev(JJS_FORMAT_AFFINE, z, PK, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R, stream);
}
int jjs_multisig_combine_ext_dev(const void* z, const void* PK_ext, const void* R_ext, const void* S_ext, const void* m,
                                 const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                 void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_combine_dev(JJS_FORMAT_EXT, z, PK_ext, R_ext, S_ext, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R,
                            stream);
}
int jjs_multisig_combine_wire_dev(const void* z, const void* PK_w, const void* R_w, const void* S_w, const void* m,
                                  const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                  void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_combine_dev(JJS_FORMAT_WIRE, z, PK_w, R_w, S_w, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R,
                            stream);
}

// The square-root tables of decode.h on the host, built once by dlog_table_entry after a cleared hash, as the device builds its
// own: jjs_msig_group_create_wire decodes the keys of a group before it registers them.
static const dlog_tables& host_dlog_tables() {
    struct built {
        std::vector<uint32_t> pow;
        std::vector<uint8_t> hash;
        dlog_tables T;
        built() : pow(DLOG_POW_WORDS, 0u), hash(65536, 0) {
            for (int i = 0; i < 7; ++i)
                for (int j = 0; j < 256; ++j) dlog_table_entry(pow.data(), hash.data(), i, j);
            T = dlog_tables{pow.data(), hash.data()};
        }
    };
    static const built b;
    return b.T;
}

#include "msig_group_calls.h"
#include "staged_host_call.h"
#include "msig_host_calls.h"
#include "msig_keyset_calls.h"
#include "msig_verify_calls.h"
#include "msig_sign_calls.h"
#include "msig_share_calls.h"

// ---- challenge export ---------------------------------------------------------------------------
static int launch_challenge(challenge_params P, void* stream) {
    if (P.n == 0) return JJS_OK;
    if (!P.c_out || !aligned16(P.c_out)) return fail(JJS_ERR_ARG, "c_out null or misaligned");
    hipStream_t s = (hipStream_t)stream;
    size_t blocks = (P.n + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(challenge_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, P);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
int jjs_challenge_single_dev(const void* R, const void* PK, const void* m, size_t n, void* c_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(R, PK, m)) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    verify_params V = params_single((const uint8_t*)m, (const uint8_t*)R, (const uint8_t*)PK, (const uint8_t*)m, n, nullptr, out_ptrs{});
    challenge_params P{};
    P.n_hash = V.n_hash; P.n = n; P.c_out = (uint8_t*)c_out;
    for (uint32_t i = 0; i < V.n_hash; ++i) P.hash_in[i] = V.hash_in[i];
    return launch_challenge(P, stream);
}
int jjs_challenge_double_dev(const void* R, const void* Rp, const void* PK, const void* PKp, const void* m, size_t n,
                             void* c_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(R, Rp, PK, PKp, m)) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    verify_params V = params_double((const uint8_t*)m, (const uint8_t*)R, (const uint8_t*)Rp, (const uint8_t*)PK,
                                    (const uint8_t*)PKp, (const uint8_t*)m, n, g->tag, nullptr, nullptr, out_ptrs{});
    challenge_params P{};
    P.n_hash = V.n_hash; P.n = n; P.c_out = (uint8_t*)c_out;
    for (uint32_t i = 0; i < V.n_hash; ++i) P.hash_in[i] = V.hash_in[i];
    return launch_challenge(P, stream);
}
int jjs_challenge_vargen_dev(const void* R, const void* PK, const void* Gen, const void* m, size_t n, void* c_out,
                             void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(R, PK, Gen, m)) return fail(JJS_ERR_ARG, "null or misaligned input pointer");
    verify_params V = params_vargen((const uint8_t*)m, (const uint8_t*)R, (const uint8_t*)PK, (const uint8_t*)Gen,
                                    (const uint8_t*)m, n, out_ptrs{});
    challenge_params P{};
    P.n_hash = V.n_hash; P.n = n; P.c_out = (uint8_t*)c_out;
    for (uint32_t i = 0; i < V.n_hash; ++i) P.hash_in[i] = V.hash_in[i];
    return launch_challenge(P, stream);
}

// ---- signing (input generator) ------------------------------------------------------------------
static int launch_sign(sign_params P, void* stream) {
    if (P.n == 0) return JJS_OK;
    hipStream_t s = (hipStream_t)stream;
    P.comb_g = g->comb_g; P.comb_gn = g->comb_gn; P.workspace = g->slots[0].workspace;
    big_slot();
    if (int rc = begin_shared(s)) return rc;
    hipLaunchKernelGGL(sign_kernel, dim3(grid_for(g->grid_sign, P.n)), dim3(BLOCK), 0, s, P);
    HIP_TRY(hipGetLastError());
    return end_shared(s);
}
int jjs_sign_single_dev(const void* sk, const void* rnd, const void* m, size_t n, void* u_out, void* R_out, void* PK_out,
                        void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(sk, rnd, m, u_out, R_out, PK_out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    sign_params P{};
    P.scheme = SCHEME_SINGLE; P.sk = (const uint8_t*)sk; P.rnd = (const uint8_t*)rnd; P.m = (const uint8_t*)m; P.n = n;
    P.u_out = (uint8_t*)u_out; P.R_out = (uint8_t*)R_out; P.PK_out = (uint8_t*)PK_out;
    return launch_sign(P, stream);
}
int jjs_sign_double_dev(const void* sk, const void* rnd, const void* m, size_t n, void* u_out, void* R_out, void* Rp_out,
                        void* PK_out, void* PKp_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(sk, rnd, m, u_out, R_out, Rp_out, PK_out, PKp_out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    sign_params P{};
    P.scheme = SCHEME_DOUBLE; P.sk = (const uint8_t*)sk; P.rnd = (const uint8_t*)rnd; P.m = (const uint8_t*)m; P.n = n;
    P.u_out = (uint8_t*)u_out; P.R_out = (uint8_t*)R_out; P.Rp_out = (uint8_t*)Rp_out; P.PK_out = (uint8_t*)PK_out;
    P.PKp_out = (uint8_t*)PKp_out;
    return launch_sign(P, stream);
}
int jjs_sign_vargen_dev(const void* sk, const void* gen_scalar, const void* rnd, const void* m, size_t n, void* u_out,
                        void* R_out, void* PK_out, void* Gen_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n && !all_ok(sk, gen_scalar, rnd, m, u_out, R_out, PK_out, Gen_out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    sign_params P{};
    P.scheme = SCHEME_VARGEN; P.sk = (const uint8_t*)sk; P.gen_scalar = (const uint8_t*)gen_scalar;
    P.rnd = (const uint8_t*)rnd; P.m = (const uint8_t*)m; P.n = n;
    P.u_out = (uint8_t*)u_out; P.R_out = (uint8_t*)R_out; P.PK_out = (uint8_t*)PK_out; P.Gen_out = (uint8_t*)Gen_out;
    return launch_sign(P, stream);
}

int jjs_public_keys_dev(const void* sk, size_t n, void* PK_out, void* PKp_out, void* bad_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(sk, PK_out) || (PKp_out && !aligned16(PKp_out))) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(derive_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const uint8_t*)sk,
                       (uint64_t)n, g->comb_g, g->comb_gn, (uint8_t*)PK_out, (uint8_t*)PKp_out, (uint8_t*)bad_out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}

#include "sign_vargen_calls.h"
#include "sign_fixed_calls.h"
#include "digest_calls.h"

// ---- debug primitives ------------------------------------------------------------------------------
int jjs_debug_fq_mul_dev(const void* a, const void* b, size_t n, void* out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(a, b, out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dbg_fq_mul_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                       (const uint8_t*)a, (const uint8_t*)b, (uint64_t)n, (uint8_t*)out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
int jjs_debug_poseidon_dev(const void* in, size_t k, size_t n, void* out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (k < 1 || k > JJS_MAX_HASH_INPUTS) return fail(JJS_ERR_ARG, "k out of range");
    if (n == 0) return JJS_OK;
    if (!all_ok(in, out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dbg_poseidon_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                       (const uint8_t*)in, (uint32_t)k, (uint64_t)n, (uint8_t*)out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
int jjs_debug_point_flags_dev(const void* points, size_t n, void* out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!points || !aligned16(points) || !out) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dbg_point_flags_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                       (const uint8_t*)points, (uint64_t)n, (uint8_t*)out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
int jjs_debug_half_scalars_dev(const void* c, size_t n, void* a_out, void* b_out, void* b_neg_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(c, a_out, b_out) || !b_neg_out) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    hipLaunchKernelGGL(dbg_half_scalars_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t*)c, (uint64_t)n, (uint8_t*)a_out, (uint8_t*)b_out, (uint8_t*)b_neg_out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}
#if defined(JJS_PROFILING)
// include/jjs_gpu_profiling.h: these two exist only in libjjs_gpu_prof.so
int jjs_debug_skip_phases(unsigned mask) {
    std::lock_guard<std::mutex> lock(L.mu);
    g_skip_phases = mask & 31u;
    return JJS_OK;
}
int jjs_debug_force_path(int which) {
    std::lock_guard<std::mutex> lock(L.mu);
    g_force_path = which & 3;                       // 0 by size and keys, 1 throughput (key tables allowed), 2 latency, 3 throughput without key tables
    g_force_positions = ((which >> 4) & 15) == 4 || ((which >> 4) & 15) == 8 ? ((which >> 4) & 15) : (((which >> 4) & 15) == 15 ? 16 : 0);    // 0x42 / 0x82 / 0xF2: latency path, 4 / 8 / 16 pieces
    g_keep_order = (which & 0x1000) != 0;
    g_force_window = ((which >> 8) & 15) == KT_WINDOW_NARROW ? ((which >> 8) & 15) : 0;   // 0x500: narrow key-table windows whatever the keys
    g_force_verdict = (which & 0x2000) ? 1 : ((which & 0x4000) ? 2 : 0);   // jjs_verify_all_*: 0x2000 the verdict algorithm, 0x4000 the per-item path
    g_force_sign_shared = (which & 0x8000) ? 1 : ((which & 0x200000) ? 2 : 0);   // jjs_sign_vargen_pt* with one generator: 0x8000 the shared-generator route at any n, 0x200000 the per-item route
    g_force_sign_keyed = (which & 0x400000) ? 1 : ((which & 0x800000) ? 2 : 0);   // jjs_sign_fixed* with one key: 0x400000 the keyed route at any n, 0x800000 the per-item route
    g_force_digest_route = (which & 0x1000000) ? 1 : ((which & 0x2000000) ? 2 : 0);   // jjs_digest*: 0x1000000 eight lanes per item at any n, 0x2000000 one lane
    g_digest_keep_order = (which & 0x4000000) != 0;                                 // ... 0x4000000: ragged items in input order
    g_force_msm_window = (which >> 16) & 31;                                // ... and bits 16-20 its window width (8-16; 0 by size)
    return JJS_OK;
}
int jjs_debug_host_timing(double out[8]) {
    std::lock_guard<std::mutex> lock(L.mu);
    for (int i = 0; i < 8; ++i) out[i] = g_host_timing[i];
    return JJS_OK;
}
int jjs_debug_pin_hash_seed(int on) {
    std::lock_guard<std::mutex> lock(L.mu);
    g_pin_hash_seed = on != 0;
    g_pin_batch_seed = (on & 2) != 0;                // jjs_verify_all_*: weights from a fixed key (verdict_calls.h)
    return JJS_OK;
}
int jjs_debug_fail_key_arena(int on) {
    std::lock_guard<std::mutex> lock(L.mu);
    g_fail_key_arena = on != 0;
    return JJS_OK;
}
// include/jjs_gpu_key_memo.h
int jjs_debug_key_memo_stats(uint64_t out[2]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    for (call_slot& c : g->slots) {
        sl = &c;
        if (c.key_stream && !c.host_owned) note_key_feedback();
    }
    out[0] = g->memo_stats[0]; out[1] = g->memo_stats[1];
    return JJS_OK;
}
int jjs_debug_allow_virtual_devices(int allow) {
    std::lock_guard<std::mutex> lock(L.mu);
    g_allow_virtual = allow != 0;
    return JJS_OK;
}
#endif
// Loads RCCL, forms a one-rank clique on the current device and sums a known 4 x u64 vector in place: checks
// the library, the symbols and the call sequence of allreduce_tallies() on a box with a single GPU.
int jjs_debug_rccl_selftest(void) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (int rc = load_rccl()) return rc;
    ncclComm_t comm;
    int ord = g->device;
    RCCL_TRY(L.rccl.CommInitAll(&comm, 1, &ord));
    const unsigned long long in[4] = {3, 1, 4, 0x100000001ull};
    unsigned long long out[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(g->tally, in, sizeof(in), hipMemcpyHostToDevice, g->stream));
    ncclResult_t r = L.rccl.GroupStart();
    if (r == ncclSuccess) r = L.rccl.AllReduce(g->tally, g->tally, 4, ncclUint64, ncclSum, comm, g->stream);
    ncclResult_t r2 = L.rccl.GroupEnd();
    if (r == ncclSuccess) r = r2;
    hipError_t e = hipMemcpyAsync(out, g->tally, sizeof(out), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    (void)L.rccl.CommDestroy(comm);
    if (r != ncclSuccess) return fail(JJS_ERR_COLLECTIVE, "RCCL self-test: %s", L.rccl.GetErrorString(r));
    if (e != hipSuccess) return fail(JJS_ERR_HIP, "RCCL self-test: %s", hipGetErrorString(e));
    if (memcmp(in, out, sizeof(in)) != 0) return fail(JJS_ERR_COLLECTIVE, "RCCL self-test: wrong sum");
    return JJS_OK;
}
size_t jjs_debug_comb_table_bytes(void) { return COMB_TABLE_WORDS * sizeof(uint32_t); }
int jjs_debug_comb_table(int which, void* host_out) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!host_out) return fail(JJS_ERR_ARG, "null pointer");
    HIP_TRY(hipMemcpy(host_out, which ? g->comb_gn : g->comb_g, COMB_TABLE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return JJS_OK;
}
int jjs_debug_dlog_tables(void* pow_host_out, void* hash_host_out) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!pow_host_out || !hash_host_out) return fail(JJS_ERR_ARG, "null pointer");
    HIP_TRY(hipMemcpy(pow_host_out, g->dlog_pow, DLOG_POW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hash_host_out, g->dlog_hash, 65536, hipMemcpyDeviceToHost));
    return JJS_OK;
}
int jjs_debug_msig_resident_lanes(void) { std::lock_guard<std::mutex> lock(L.mu); if (int rc = check_ready()) return rc; return g->grid_msig * BLOCK; }

}  // extern "C"
