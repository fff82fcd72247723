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
    if (int rc = ensure_msig_scratch(n, n_transcripts, fmt != JJS_FORMAT_AFFINE ? n : 0, n ? n : 1, n_transcripts)) return rc;
    const msig_scratch W = msig_scratch_carve();
    const uint8_t* pts[2] = {(const uint8_t*)R, (const uint8_t*)S};
    msig_keyset_params K{};
    msig_params& P = K.M;
    P.z = (const uint8_t*)z; P.m = (const uint8_t*)m;
    P.n_transcripts = (uint32_t)n_transcripts; P.n_total = n;
    P.share_status = (uint8_t*)share_status; P.agg_pk = (uint8_t*)agg_pk; P.sig_u = (uint8_t*)sig_u; P.sig_R = (uint8_t*)sig_R;
    P.transcript_status = (uint8_t*)transcript_status;
    P.tr_of = W.tr_of; P.d_words = W.d_words; P.dpk = W.dpk; P.e_pt = W.e_pt;
    P.a_words = W.a_words; P.c_words = W.c_words; P.offsets = W.offsets;
    P.tags = g->tags_long; P.comb_g = g->comb_g; P.lane_ws = g->slots[0].workspace;
    P.max_table_participants = JJS_MSIG_MAX_PARTICIPANTS;
    P.long_tags = W.long_tags;
    P.PK = W.ks_pk;
    K.key_idx = (const uint32_t*)key_idx; K.n_keys = k.n_keys;
    K.keys = c.keys[0]; K.flags = c.flags[0]; K.tables = c.tables[0];
    K.pk_col = W.ks_pk; K.row_key = W.ks_row_key; K.refused = W.ks_refused;
    big_slot();
    if (int rc = begin_shared(s)) return rc;
    auto queue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(W.offsets, offsets_host, (n_transcripts + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(W.ks_refused, 0, n_transcripts * sizeof(uint32_t), s));
        if (int rc = msig_ingest(fmt, W, pts, 2, n, s)) return rc;
        P.R = pts[0]; P.S = pts[1];
        const dim3 per_share(grid_for(g->grid_msig, n)), per_transcript(grid_for(g->grid_msig, n_transcripts));
        for (int pass = 0; pass < 7; ++pass) {
            const size_t count = (pass == 0 || pass == 2 || pass == 4 || pass == 6) ? n_transcripts : n;
            // a pass with a hash chain and few items: eight lanes per item (multisig_core.h hash_lanes)
            P.hash_lanes = (pass == 1 || pass == 2 || pass == 4) ? msig_hash_lanes(count) : 1u;
            if (pass == 1) {
                hipLaunchKernelGGL(msig_keyset_delin_kernel, dim3(grid_for(g->grid_msig, n * P.hash_lanes)), dim3(BLOCK), 0, s, K);
            } else if (pass == 5) {
                hipLaunchKernelGGL(msig_keyset_share_kernel, per_share, dim3(BLOCK), 0, s, K);
            } else {
                hipLaunchKernelGGL(msig_kernel, dim3(grid_for(g->grid_msig, count * P.hash_lanes)), dim3(BLOCK), 0, s, P, pass);
            }
            if (pass == 0) hipLaunchKernelGGL(msig_keyset_gather_kernel, per_share, dim3(BLOCK), 0, s, K);   // behind the map: it reads tr_of
        }
        hipLaunchKernelGGL(msig_keyset_refuse_kernel, per_transcript, dim3(BLOCK), 0, s, K);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    };
    const int rc = queue();
    const int rc2 = end_shared(s);              // the slot's event covers whatever was queued, also when a step failed
    return rc ? rc : rc2;
}

static int msig_keyset_combine_dev(jjs_keyset ks, int format, bool wire, const void* key_idx, const void* z, const void* R, const void* S, const void* m,
                                    const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                    void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    keyset_entry* k = nullptr;
    const keyset_copy* c = nullptr;
    int fmt = JJS_FORMAT_AFFINE;
    if (int rc = msig_keyset_find(ks, g, k, c)) return rc;
    if (int rc = msig_call_format(format, wire, fmt)) return rc;
    if (n_transcripts == 0) return JJS_OK;
    return no_throw([&] {
        return msig_keyset_combine_locked(*k, *c, fmt, key_idx, z, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk,
                                          sig_u, sig_R, (hipStream_t)stream);
    });
}

static int msig_keyset_combine_host(jjs_keyset ks, int format, bool wire, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R, const uint8_t* S,
                                const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    device_state* dev = nullptr;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        keyset_entry* k = nullptr;
        const keyset_copy* c = nullptr;
        if (int rc = msig_keyset_find(ks, g, k, c)) return rc;
        if (int rc = msig_call_format(format, wire, fmt)) return rc;
        if (n_transcripts == 0) return JJS_OK;
        if (int rc = msig_check_offsets(offsets, n_transcripts, n)) return rc;
        if ((n && (!key_idx || !z || !R || !S || !share_status)) || !m || !agg_pk || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
        dev = g;
        ++g_blocking_calls;              // jjs_shutdown does not free `dev` before this call has left
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        const size_t B = n_transcripts, w = msig_point_bytes(fmt);
        const void* src[5] = {z, key_idx, R, S, m};            // the indices travel in the inline call's PK column: 4 bytes a share
        const size_t in_bytes[5] = {n * 32, n * 4, n * w, n * w, B * 32}, out_bytes[5] = {n, B, B * 64, B * 32, B * 64};
        msig_stage St{};
        if (int rc = msig_stage_in(dev, src, in_bytes, out_bytes, St)) return rc;
        {
            std::lock_guard<std::mutex> lock(L.mu);
            if (check_ready() != JJS_OK || g != dev) return fail(JJS_ERR_NOT_INIT, "the engine's devices changed during the call");
            // (the set is looked up again: it may have been destroyed meanwhile)
            keyset_entry* k = nullptr;
            const keyset_copy* c = nullptr;
            if (int rc = msig_keyset_find(ks, dev, k, c)) return rc;
            if (int rc = msig_keyset_combine_locked(*k, *c, fmt, St.in[1], St.in[0], St.in[2], St.in[3], St.in[4], offsets, B, St.out[0],
                                                    transcript_status ? St.out[1] : nullptr, St.out[2], St.out[3], St.out[4], St.s))
                return rc;
        }
        uint8_t* const dst[5] = {share_status, transcript_status, agg_pk, sig_u, sig_R};
        return msig_stage_out(St, dst, out_bytes);
    });
}
}  // extern "C++"

extern "C" {

int jjs_multisig_combine_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const void* z, const void* R, const void* S, const void* m,
                                    const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                    void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_keyset_combine_dev(ks, format, false, key_idx, z, R, S, m, offsets_host, n_transcripts, share_status, transcript_status, agg_pk,
                                   sig_u, sig_R, stream);
}
int jjs_multisig_combine_keyset_wire_dev(jjs_keyset ks, const void* key_idx, const void* z, const void* R_w, const void* S_w, const void* m,
                                         const uint32_t* offsets_host, size_t n_transcripts, void* share_status, void* transcript_status,
                                         void* agg_pk, void* sig_u, void* sig_R, void* stream) {
    return msig_keyset_combine_dev(ks, JJS_FORMAT_WIRE, true, key_idx, z, R_w, S_w, m, offsets_host, n_transcripts, share_status,
                                   transcript_status, agg_pk, sig_u, sig_R, stream);
}
int jjs_multisig_combine_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R, const uint8_t* S,
                                const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_keyset_combine_host(ks, format, false, key_idx, z, R, S, m, offsets, n_transcripts, share_status, transcript_status, agg_pk,
                                    sig_u, sig_R);
}
int jjs_multisig_combine_keyset_wire(jjs_keyset ks, const uint32_t* key_idx, const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w,
                                     const uint8_t* m, const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status,
                                     uint8_t* transcript_status, uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_keyset_combine_host(ks, JJS_FORMAT_WIRE, true, key_idx, z, R_w, S_w, m, offsets, n_transcripts, share_status,
                                    transcript_status, agg_pk, sig_u, sig_R);
}

}  // extern "C"
