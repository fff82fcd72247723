// Part of jjs_gpu.hip (included among the extern "C" entry points, behind msig_group_calls.h): the blocking host-buffer forms of
// the multisignature calls, jjs_multisig_combine and jjs_msig_group_combine.  They follow the key-set host call
// (keyset_calls.h): the columns are uploaded whole from pageable memory into a staging area of the calling thread's current
// device (device_state::msig_stage, a grow_only that jjs_trim frees), uploads, passes and the copy of the outputs back run on
// the device's key-set stream, one such call at a time per device (host_mu), and the engine's mutex is held while the call is
// queued, never while it waits.  A call counts itself among g_blocking_calls so that jjs_shutdown waits for it.
extern "C++" {
struct msig_stage {
    const void* in[5];     // z, PK, R, S, m (a group call has no PK)
    uint8_t* out[5];       // share_status, transcript_status, agg_pk, sig_u, sig_R
    hipStream_t s;
};
// Column i of in_bytes[i] bytes copied from src[i], then output areas of out_bytes[j] bytes, each part padded to 256 bytes (a
// part of 0 bytes -- a column the call does not have, the columns of a call without shares -- still gets 256 bytes, so that every
// pointer handed to the passes is a distinct, valid, aligned address).  Under dev->host_mu, g = dev; the area grows under the
// engine's mutex too, because jjs_memory_stats reads its size under that mutex alone.
static int msig_stage_in(device_state* dev, const void* const* src, const size_t* in_bytes, const size_t* out_bytes, msig_stage& S) {
    size_t off[10], total = 0;
    for (int i = 0; i < 5; ++i) { off[i] = total; total += pad256(in_bytes[i] ? in_bytes[i] : 1); }
    for (int j = 0; j < 5; ++j) { off[5 + j] = total; total += pad256(out_bytes[j] ? out_bytes[j] : 1); }
    HIP_TRY(hipSetDevice(dev->device));
    if (dev->msig_stage.capacity() < total) {
        std::lock_guard<std::mutex> lock(L.mu);
        if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
        if (int rc = dev->msig_stage.ensure(total)) return rc;
    }
    S.s = dev->ks_stream;
    for (int i = 0; i < 5; ++i) {
        S.in[i] = dev->msig_stage + off[i];
        if (in_bytes[i]) HIP_TRY(hipMemcpyAsync(dev->msig_stage + off[i], src[i], in_bytes[i], hipMemcpyHostToDevice, S.s));
    }
    for (int j = 0; j < 5; ++j) S.out[j] = dev->msig_stage + off[5 + j];
    return JJS_OK;
}
// the outputs back to the caller (dst[j] null: not wanted), and the wait for everything the call queued
static int msig_stage_out(const msig_stage& S, uint8_t* const* dst, const size_t* out_bytes) {
    for (int j = 0; j < 5; ++j)
        if (dst[j] && out_bytes[j]) HIP_TRY(hipMemcpyAsync(dst[j], S.out[j], out_bytes[j], hipMemcpyDeviceToHost, S.s));
    HIP_TRY(hipStreamSynchronize(S.s));
    return JJS_OK;
}
static int msig_format(int format, bool& ext) {
    if (format != JJS_FORMAT_AFFINE && format != JJS_FORMAT_EXT)
        return fail(JJS_ERR_ARG, "the multisignature calls take affine or extended points (format %d)", format);
    ext = format == JJS_FORMAT_EXT;
    return JJS_OK;
}
// bytes of a point in the columns of a call in format fmt (JJS_FORMAT_*)
static size_t msig_point_bytes(int fmt) { return fmt == JJS_FORMAT_EXT ? 96 : (fmt == JJS_FORMAT_WIRE ? 32 : 64); }
// the format of a call: that of a *_wire entry point (wire), which has no format argument to refuse, or the one `format` names
static int msig_call_format(int format, bool wire, int& fmt) {
    bool ext = false;
    fmt = JJS_FORMAT_WIRE;
    if (wire) return JJS_OK;
    if (int rc = msig_format(format, ext)) return rc;
    fmt = ext ? JJS_FORMAT_EXT : JJS_FORMAT_AFFINE;
    return JJS_OK;
}

static int msig_combine_host(int format, bool wire, const uint8_t* z, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                         const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                         uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    device_state* dev = nullptr;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        if (int rc = msig_call_format(format, wire, fmt)) return rc;
        if (n_transcripts == 0) return JJS_OK;
        if (int rc = msig_check_offsets(offsets, n_transcripts, n)) return rc;
        if ((n && (!z || !PK || !R || !S || !share_status)) || !m || !agg_pk || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
        dev = g;
        ++g_blocking_calls;              // jjs_shutdown does not free `dev` before this call has left
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        const size_t B = n_transcripts, w = msig_point_bytes(fmt);
        const void* src[5] = {z, PK, R, S, m};
        const size_t in_bytes[5] = {n * 32, n * w, n * w, n * w, B * 32}, out_bytes[5] = {n, B, B * 64, B * 32, B * 64};
        msig_stage St{};
        if (int rc = msig_stage_in(dev, src, in_bytes, out_bytes, St)) return rc;
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
            if (int rc = msig_combine_locked(fmt, St.in[0], St.in[1], St.in[2], St.in[3], St.in[4], offsets, B, St.out[0],
                                             transcript_status ? St.out[1] : nullptr, St.out[2], St.out[3], St.out[4], St.s))
                return rc;
        }
        uint8_t* const dst[5] = {share_status, transcript_status, agg_pk, sig_u, sig_R};
        return msig_stage_out(St, dst, out_bytes);
    });
}

static int msig_group_combine_host(jjs_msig_group h, int format, bool wire, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                           size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    device_state* dev = nullptr;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        msig_group_entry* k = g_msig_groups.find(h);
        if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
        if (int rc = msig_call_format(format, wire, fmt)) return rc;
        if (n_transcripts == 0) return JJS_OK;
        const uint64_t per = k->participants;
        if (n_transcripts >= (1ull << 32) / per + ((1ull << 32) % per ? 1u : 0u))
            return fail(JJS_ERR_ARG, "%zu transcripts of %llu participants: the shares are indexed with 32 bits", n_transcripts, (unsigned long long)per);
        if (!z || !R || !S || !m || !share_status || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
        n = n_transcripts * per;
        dev = g;
        ++g_blocking_calls;              // jjs_shutdown does not free `dev` before this call has left
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        const size_t B = n_transcripts, w = msig_point_bytes(fmt);
        const void* src[5] = {z, nullptr, R, S, m};
        const size_t in_bytes[5] = {n * 32, 0, n * w, n * w, B * 32}, out_bytes[5] = {n, B, 0, B * 32, B * 64};
        msig_stage St{};
        if (int rc = msig_stage_in(dev, src, in_bytes, out_bytes, St)) return rc;
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
            // (the group is looked up again: it may have been destroyed, or registered with other participants, meanwhile)
            msig_group_entry* k = g_msig_groups.find(h);
            if (!k || (size_t)k->participants * B != n) return fail(JJS_ERR_ARG, "the signer group was destroyed during the call");
            if (int rc = msig_group_combine_locked(h, fmt, St.in[0], St.in[2], St.in[3], St.in[4], B, St.out[0],
                                                   transcript_status ? St.out[1] : nullptr, St.out[3], St.out[4], St.s))
                return rc;
        }
        uint8_t* const dst[5] = {share_status, transcript_status, nullptr, sig_u, sig_R};
        return msig_stage_out(St, dst, out_bytes);
    });
}

}  // extern "C++"

extern "C" {

int jjs_multisig_combine(int format, const uint8_t* z, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                         const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                         uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_combine_host(format, false, z, PK, R, S, m, offsets, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R);
}
int jjs_multisig_combine_wire(const uint8_t* z, const uint8_t* PK_w, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                              const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                              uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_combine_host(JJS_FORMAT_WIRE, true, z, PK_w, R_w, S_w, m, offsets, n_transcripts, share_status, transcript_status, agg_pk, sig_u,
                             sig_R);
}
int jjs_msig_group_combine(jjs_msig_group h, int format, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                           size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_group_combine_host(h, format, false, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
}
int jjs_msig_group_combine_wire(jjs_msig_group h, const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                                size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_group_combine_host(h, JJS_FORMAT_WIRE, true, z, R_w, S_w, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
}

}  // extern "C"
