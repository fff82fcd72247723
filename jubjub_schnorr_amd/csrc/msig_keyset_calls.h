// Part of jjs_gpu.hip (included among the extern "C" entry points, behind msig_host_calls.h): the multisignature call against
// a registered key set (msig_keyset.h, include/jjs_gpu.h jjs_multisig_combine_keyset[_dev]) -- the inline call's launches with
// a gather behind pass 0, passes 1 and 5 over the set's tables, and the refusals behind pass 6.

extern "C++" {
// the set a call names: a live JJS_SCHEME_SINGLE set with a copy on device `dev` (under the engine's mutex)
static int msig_keyset_find(jjs_keyset h, const device_state* dev, keyset_entry*& k, const keyset_copy*& c) {
    k = g_keysets.find(h);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed key set");
    if (k->scheme != JJS_SCHEME_SINGLE) return fail(JJS_ERR_ARG, "the multisignature call takes a key set of JJS_SCHEME_SINGLE");
    c = copy_for(*k, dev);
    if (!c) return fail(JJS_ERR_ARG, "the key set has no copy on this device");
    return JJS_OK;
}
// The call on device columns, queued on s (under the engine's mutex, g the device; n_transcripts > 0).  fmt (JJS_FORMAT_*): R, S are N x 64, N x 96 or N x 32.
static int msig_keyset_combine_locked(const keyset_entry& k, const keyset_copy& c, int fmt, const void* key_idx, const void* z, const void* R,
                                      const void* S, const void* m, const uint32_t* offsets_host, size_t n_transcripts, void* share_status,
                                      void* transcript_status, void* agg_pk, void* sig_u, void* sig_R, hipStream_t s) {
    size_t n = 0;
    if (int rc = msig_check_offsets(offsets_host, n_transcripts, n)) return rc;
    if ((n && (!all_ok(z, R, S) || !key_idx || (reinterpret_cast<uintptr_t>(key_idx) & 3u))) || !all_ok(m, agg_pk, sig_u, sig_R) ||
        (n && !share_status))
        return fail(JJS_ERR_ARG, "null or misaligned pointer");
    msig_caps need;
    need.rows = n; need.transcripts = n_transcripts;
    if (fmt != JJS_FORMAT_AFFINE) need.ext_rows = n;
    need.ks_rows = n ? n : 1; need.ks_transcripts = n_transcripts;
    return msig_scratch_call(need, s, [&](const msig_scratch& W) -> int {
        const uint8_t* pts[2] = {(const uint8_t*)R, (const uint8_t*)S};
        msig_keyset_params K{};
        msig_params& P = K.M;
        msig_params_common(P, W, n_transcripts, n);
        P.z = (const uint8_t*)z; P.m = (const uint8_t*)m;
        P.share_status = (uint8_t*)share_status; P.agg_pk = (uint8_t*)agg_pk; P.sig_u = (uint8_t*)sig_u; P.sig_R = (uint8_t*)sig_R;
        P.transcript_status = (uint8_t*)transcript_status;
        P.e_pt = W.e_pt;
        P.PK = W.ks_pk;
        msig_keyset_fill(K, k, c, key_idx, W, W.ks_refused);
        HIP_TRY(hipMemcpyAsync(W.offsets, offsets_host, (n_transcripts + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(W.ks_refused, 0, n_transcripts * sizeof(uint32_t), s));
        if (int rc = msig_ingest(fmt, W, pts, 2, n, s)) return rc;
        P.R = pts[0]; P.S = pts[1];
        const dim3 per_share(grid_for(g->grid_msig, n)), per_transcript(grid_for(g->grid_msig, n_transcripts));
        launch_msig_pass(P, 0, s);
        hipLaunchKernelGGL(msig_keyset_gather_kernel, per_share, dim3(BLOCK), 0, s, K);   // behind the map: it reads tr_of
        const dim3 delin(msig_pass_grid(P, 1));
        hipLaunchKernelGGL(msig_keyset_delin_kernel, delin, dim3(BLOCK), 0, s, K);        // pass 1 over the set's tables
        for (int pass = 2; pass < 5; ++pass) launch_msig_pass(P, pass, s);
        const dim3 shares(msig_pass_grid(P, 5));
        hipLaunchKernelGGL(msig_keyset_share_kernel, shares, dim3(BLOCK), 0, s, K);       // pass 5 over the set's tables
        launch_msig_pass(P, 6, s);
        hipLaunchKernelGGL(msig_keyset_refuse_kernel, per_transcript, dim3(BLOCK), 0, s, K);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}

static int msig_keyset_combine_dev(jjs_keyset ks, int format, unsigned formats, const void* key_idx, const void* z, const void* R, const void* S, const void* m,
                                    const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                    void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = nullptr;
    const keyset_copy* c = nullptr;
    int fmt = JJS_FORMAT_AFFINE;
    if (int rc = msig_keyset_find(ks, g, k, c)) return rc;
    if (int rc = msig_format(format, formats, fmt)) return rc;
    if (n_transcripts == 0) return JJS_OK;
    return no_throw([&] {
        return msig_keyset_combine_locked(*k, *c, fmt, key_idx, z, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk,
                                          sig_u, sig_R, (hipStream_t)stream);
    });
}

// parts: as the inline call's (msig_host_calls.h); the indices travel in its PK column, 4 bytes a share
static int msig_keyset_combine_host(jjs_keyset ks, int format, unsigned formats, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R, const uint8_t* S,
                                const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    const size_t B = n_transcripts;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            keyset_entry* k = nullptr;
            const keyset_copy* c = nullptr;
            if (int rc = msig_keyset_find(ks, g, k, c)) return rc;
            if (int rc = msig_format(format, formats, fmt)) return rc;
            if (B == 0) return JJS_OK;
            if (int rc = msig_check_offsets(offsets, B, n)) return rc;
            if ((n && (!key_idx || !z || !R || !S || !share_status)) || !m || !agg_pk || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
            go = true;
            return JJS_OK;
        },
        [&] {
            const size_t w = msig_point_bytes(fmt);
            return std::vector<stage_part>{{n * 32, z, nullptr}, {n * 4, key_idx, nullptr}, {n * w, R, nullptr}, {n * w, S, nullptr}, {B * 32, m, nullptr},
                                           {n, nullptr, share_status}, {B, nullptr, transcript_status}, {B * 64, nullptr, agg_pk},
                                           {B * 32, nullptr, sig_u}, {B * 64, nullptr, sig_R}};
        },
        [&](uint8_t* const* p, hipStream_t s) -> int {
            // (the set is looked up again: it may have been destroyed meanwhile)
            keyset_entry* k = nullptr;
            const keyset_copy* c = nullptr;
            if (int rc = msig_keyset_find(ks, g, k, c)) return rc;
            return msig_keyset_combine_locked(*k, *c, fmt, p[1], p[0], p[2], p[3], p[4], offsets, B, p[5], transcript_status ? p[6] : nullptr, p[7],
                                              p[8], p[9], s);
        });
}
}  // extern "C++"

extern "C" {

int jjs_multisig_combine_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const void* z, const void* R, const void* S, const void* m,
                                    const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                    void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_keyset_combine_dev(ks, format, MSIG_FORMATS_POINTS, key_idx, z, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk,
                                   sig_u, sig_R, stream);
}
int jjs_multisig_combine_keyset_wire_dev(jjs_keyset ks, const void* key_idx, const void* z, const void* R_w, const void* S_w, const void* m,
                                         const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                         void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_keyset_combine_dev(ks, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, key_idx, z, R_w, S_w, m, offsets_host, n_transcripts, share_status,
                                   transcript_status, agg_pk, sig_u, sig_R, stream);
}
int jjs_multisig_combine_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R, const uint8_t* S,
                                const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_keyset_combine_host(ks, format, MSIG_FORMATS_POINTS, key_idx, z, R, S, m, offsets, n_transcripts, share_status, transcript_status, agg_pk,
                                    sig_u, sig_R);
}
int jjs_multisig_combine_keyset_wire(jjs_keyset ks, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w,
                                     const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                     uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_keyset_combine_host(ks, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, key_idx, z, R_w, S_w, m, offsets, n_transcripts, share_status,
                                    transcript_status, agg_pk, sig_u, sig_R);
}

}  // extern "C"
