// Part of jjs_gpu.hip (included among the extern "C" entry points, in front of msig_host_calls.h): the frame of a blocking
// host-buffer call whose columns are staged whole, from pageable memory, in the calling thread's current device's
// device_state::msig_stage (a grow_only that jjs_trim frees) -- the multisignature combine, verify, verify_share and sign calls and
// the SecretKey and var-generator signers.  Uploads, passes and the copy of the outputs back run on the device's key-set stream,
// one such call at a time per device (host_mu), and the engine's mutex is held while the call is queued, never across an upload,
// a wait or the copy back.  A call counts itself among g_blocking_calls so that jjs_shutdown does not free its device before it
// has left.
extern "C++" {
// One part of the area.  Every part is padded to 256 bytes, and a part of 0 bytes -- a column the call does not have, the
// columns of a call without shares -- still takes 256, so that every pointer handed to the passes is a distinct, valid, aligned
// address.
struct stage_part {
    size_t bytes;
    const void* src;       // host memory uploaded into the part if it has bytes (null: nothing to upload)
    void* dst;             // host memory the part is copied back to if it has bytes (null: no output, or not wanted)
};
// a run of adjacent parts that hold secret key material (count 0: the call stages none)
struct stage_secrets { size_t first, count; };

// enter(go): the call's own checks, registry lookups and zero-size results, under the engine's mutex behind check_ready; a
//   refusal is its return code, go = false with JJS_OK is a call with nothing to do.
// parts(): the list of parts, from what enter computed.
// queue(part, s): under the engine's mutex again, g the device the call entered on: looks a registered object up once more
//   and queues the call's *_locked function on s over the part pointers.
template <class Enter, class Parts, class Queue>
static int staged_host_call(Enter&& enter, Parts&& parts, Queue&& queue, stage_secrets secret = {0, 0}) {
    device_state* dev = nullptr;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        bool go = false;
        if (int rc = enter(go)) return rc;
        if (!go) return JJS_OK;
        dev = g;
        ++g_blocking_calls;              // jjs_shutdown does not free `dev` before this call has left
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        const std::vector<stage_part> P = parts();
        std::vector<size_t> off(P.size() + 1);
        size_t total = 0;
        for (size_t i = 0; i < P.size(); ++i) { off[i] = total; total += pad256(P[i].bytes ? P[i].bytes : 1); }
        off[P.size()] = total;
        HIP_TRY(hipSetDevice(dev->device));
        // (the area grows under the engine's mutex too, because jjs_memory_stats reads its size under that mutex alone)
        if (dev->msig_stage.capacity() < total) {
            std::lock_guard<std::mutex> lock(L.mu);
            if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
            if (int rc = dev->msig_stage.ensure(total)) return rc;
        }
        const hipStream_t s = dev->ks_stream;
        std::vector<uint8_t*> part(P.size());
        for (size_t i = 0; i < P.size(); ++i) part[i] = dev->msig_stage + off[i];
        // whatever happens behind this point, the staged secrets (adjacent parts) are cleared before the call returns
        struct wipe {
            uint8_t* at; size_t bytes; hipStream_t st;
            ~wipe() { if (bytes) { (void)hipMemsetAsync(at, 0, bytes, st); (void)hipStreamSynchronize(st); } }
        } wipe_secrets{dev->msig_stage + off[secret.first], off[secret.first + secret.count] - off[secret.first], s};
        for (size_t i = 0; i < P.size(); ++i)
            if (P[i].src && P[i].bytes) HIP_TRY(hipMemcpyAsync(part[i], P[i].src, P[i].bytes, hipMemcpyHostToDevice, s));
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
            if (int rc = queue(part.data(), s)) return rc;
        }
        // the outputs back to the caller, and the wait for everything the call queued
        for (size_t i = 0; i < P.size(); ++i)
            if (P[i].dst && P[i].bytes) HIP_TRY(hipMemcpyAsync(P[i].dst, part[i], P[i].bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    });
}
}  // extern "C++"
