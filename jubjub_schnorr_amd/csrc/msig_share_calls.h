// Part of jjs_gpu.hip (included among the extern "C" entry points, behind msig_sign_calls.h): verify_share on its own
// (msig_share.h, include/jjs_gpu.h jjs_multisig_verify_share*, jjs_msig_group_verify_share*, jjs_multisig_verify_share_keyset*) --
// the front of the combine call of the same route, then the check pass, the sums pass with the first step of the query pass in one
// launch, and the second step of the query pass.  The passes use the multisignature scratch, which belongs to slot 0; pk_agg, and
// RSa when the caller does not ask for it, are columns of that scratch.

extern "C++" {
enum { MSH_INLINE = 0, MSH_GROUP = 1, MSH_KEYSET = 2 };
struct msh_call {
    int route, fmt;
    uint64_t handle;                     // the signer group or the key set
    const void *keys, *R, *S, *m;        // keys: PK (inline), key_idx (key set), nothing (group)
    const uint32_t* offsets_host;        // inline, key set
    size_t B;
    const void *qt, *qs, *z;
    size_t Q;
    void *status, *sig_R;
};
// the rows of a call whose transcripts are acceptable: the combine call's own rules (under the engine's mutex)
static int msh_rows(const msh_call& A, size_t& n) {
    if (A.route != MSH_GROUP) return msig_check_offsets(A.offsets_host, A.B, n);
    msig_group_entry* k = g_msig_groups.find(A.handle);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    return msig_group_rows(*k, A.B, n);
}
// The call on device columns, queued on st (under the engine's mutex, g the device; B > 0, and Q > 0 or sig_R given).
static int msig_share_locked(const msh_call& A, hipStream_t st) {
    size_t n = 0;
    if (int rc = msh_rows(A, n)) return rc;
    const size_t B = A.B, Q = A.Q;
    const bool has_keys = A.route != MSH_GROUP;
    if ((n && (!all_ok(A.R, A.S) || (has_keys && !A.keys))) || !all_ok(A.m) || (A.sig_R && !aligned16(A.sig_R)) ||
        (reinterpret_cast<uintptr_t>(A.keys) & (A.route == MSH_KEYSET ? 3u : 15u)))
        return fail(JJS_ERR_ARG, "null or misaligned pointer");
    if (Q && (!all_ok(A.z) || !A.qt || !A.qs || !A.status || ((reinterpret_cast<uintptr_t>(A.qt) | reinterpret_cast<uintptr_t>(A.qs)) & 3u)))
        return fail(JJS_ERR_ARG, "null or misaligned pointer");
    msig_group_entry* grp = nullptr;
    const msig_group_copy* gc = nullptr;
    keyset_entry* ks = nullptr;
    const keyset_copy* kc = nullptr;
    if (A.route == MSH_GROUP) {
        grp = g_msig_groups.find(A.handle);
        gc = grp ? copy_for(*grp, g) : nullptr;
        if (!gc) return fail(JJS_ERR_ARG, "the signer group has no copy on this device");
    } else if (A.route == MSH_KEYSET) {
        if (int rc = msig_keyset_find(A.handle, g, ks, kc)) return rc;
    }
    const bool keyset = A.route == MSH_KEYSET;
    msig_caps need;
    need.rows = n; need.transcripts = B;
    if (A.fmt != JJS_FORMAT_AFFINE) need.ext_rows = n;
    if (keyset) { need.ks_rows = n ? n : 1; need.ks_transcripts = B; }
    need.share_queries = Q ? Q : 1; need.share_transcripts = B;
    if (grp) ++grp->calls;
    return msig_scratch_call(need, st, [&](const msig_scratch& W) -> int {
        const uint8_t* pts[3] = {(const uint8_t*)A.keys, (const uint8_t*)A.R, (const uint8_t*)A.S};
        const uint32_t n_pts = A.route == MSH_INLINE ? 3u : 2u;
        const uint8_t** cols = A.route == MSH_INLINE ? pts : pts + 1;
        msig_share_params X{};
        msig_params& P = X.M;
        msig_params_common(P, W, B, n);
        P.m = (const uint8_t*)A.m;
        P.sig_R = A.sig_R ? (uint8_t*)A.sig_R : W.share_rsa;
        P.agg_pk = A.route == MSH_GROUP ? gc->agg_pk : W.share_agg;
        P.e_pt = W.share_pt;
        X.q_transcript = (const uint32_t*)A.qt; X.q_slot = (const uint32_t*)A.qs; X.q_z = (const uint8_t*)A.z;
        X.n_queries = Q; X.q_status = (uint8_t*)A.status;
        X.bad = W.share_bad;
        X.check_pk = A.route == MSH_INLINE ? 1u : 0u;
        X.d_words = W.d_words;
        if (A.route == MSH_GROUP) {
            msig_group_fill(X, *grp, *gc);
        } else if (keyset) {
            X.tables = kc->tables[0]; X.row_key = W.ks_row_key;
        }
        if (A.route != MSH_GROUP) HIP_TRY(hipMemcpyAsync(W.offsets, A.offsets_host, (B + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(W.share_bad, 0, B * sizeof(uint32_t), st));
        if (int rc = msig_ingest(A.fmt, W, cols, n_pts, n, st)) return rc;
        P.R = pts[1]; P.S = pts[2];
        P.PK = keyset ? W.ks_pk : pts[0];
        const dim3 per_row(grid_for(g->grid_msig, n));
        const uint32_t hl_transcripts = msig_hash_lanes(B);
        // the front of the route's combine call: a_words, and for ragged transcripts the map, d_words and pk_agg
        if (A.route == MSH_GROUP) {
            msig_group_params G{};
            G.M = P; G.M.hash_lanes = hl_transcripts;
            msig_group_fill(G, *grp, *gc);
            hipLaunchKernelGGL(msig_group_kernel, dim3(grid_for(g->grid_msig, B * hl_transcripts)), dim3(BLOCK), 0, st, G, 0);
        } else {
            launch_msig_pass(P, 0, st);
            if (keyset) {
                msig_keyset_params K{};
                K.M = P;
                msig_keyset_fill(K, *ks, *kc, A.keys, W, W.share_bad);                           // the gather flags the transcript itself
                const dim3 delin(msig_pass_grid(K.M, 1));                                        // (the gather, too, sees pass 1's hash_lanes)
                if (n) {
                    hipLaunchKernelGGL(msig_keyset_gather_kernel, per_row, dim3(BLOCK), 0, st, K);
                    hipLaunchKernelGGL(msig_keyset_delin_kernel, delin, dim3(BLOCK), 0, st, K);
                }
            } else if (n) {
                launch_msig_pass(P, 1, st);
            }
            launch_msig_pass(P, 2, st);
        }
        P.hash_lanes = 1;
        if (n) hipLaunchKernelGGL(msig_share_check_kernel, per_row, dim3(BLOCK), 0, st, X);          // behind the map: it reads tr_of
        P.hash_lanes = hl_transcripts;
        // (the sums pass and, in the lanes behind it, the first step of the query pass)
        hipLaunchKernelGGL(msig_share_sums_kernel, dim3(grid_for(g->grid_msig, msh_first_query_lane(B * hl_transcripts) + Q)), dim3(BLOCK), 0, st, X);
        P.hash_lanes = 1;
        if (Q) {
            const dim3 per_query(grid_for(g->grid_msig, Q));
            if (A.route == MSH_INLINE) hipLaunchKernelGGL(msig_share_inline_kernel, per_query, dim3(BLOCK), 0, st, X);
            else hipLaunchKernelGGL(msig_share_tables_kernel, per_query, dim3(BLOCK), 0, st, X);
        }
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}
// what every form looks at first (under the engine's mutex, behind check_ready): JJS_OK with go = false: nothing to do
static int msh_enter(msh_call& A, int format, bool& go) {
    go = false;
    if (A.route == MSH_GROUP && !g_msig_groups.find(A.handle)) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    if (A.route == MSH_KEYSET) {
        keyset_entry* k = nullptr;
        const keyset_copy* c = nullptr;
        if (int rc = msig_keyset_find(A.handle, g, k, c)) return rc;
    }
    if (int rc = msig_format(format, MSIG_FORMATS_POINTS | MSIG_FORMATS_WIRE, A.fmt)) return rc;
    go = A.B != 0 && (A.Q != 0 || A.sig_R != nullptr);
    return JJS_OK;
}
static int msig_share_dev(msh_call A, int format, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    bool go = false;
    if (int rc = msh_enter(A, format, go)) return rc;
    if (!go) return JJS_OK;
    return no_throw([&] { return msig_share_locked(A, (hipStream_t)stream); });
}
// The same from host buffers, blocking, on the frame of staged_host_call.h.
// parts: keys (PK, key_idx, or empty for a group), R, S, m, share_transcript, share_slot, z in; share_status, sig_R out
static int msig_share_host(msh_call A, int format) {
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            if (int rc = msh_enter(A, format, go)) return rc;
            if (!go) return JJS_OK;
            if (int rc = msh_rows(A, n)) return rc;
            if ((n && (!A.R || !A.S || (A.route != MSH_GROUP && !A.keys))) || !A.m || (A.Q && (!A.qt || !A.qs || !A.z || !A.status)))
                return fail(JJS_ERR_ARG, "null pointer");
            return JJS_OK;
        },
        [&] {
            const size_t B = A.B, Q = A.Q, w = msig_point_bytes(A.fmt);
            const size_t key_bytes = A.route == MSH_GROUP ? 0 : (A.route == MSH_KEYSET ? n * 4 : n * w);
            return std::vector<stage_part>{{key_bytes, A.keys, nullptr}, {n * w, A.R, nullptr}, {n * w, A.S, nullptr}, {B * 32, A.m, nullptr},
                                           {Q * 4, A.qt, nullptr}, {Q * 4, A.qs, nullptr}, {Q * 32, A.z, nullptr},
                                           {Q, nullptr, A.status}, {B * 64, nullptr, A.sig_R}};
        },
        [&](uint8_t* const* p, hipStream_t st) -> int {
            // (a group or a set is looked up again by the call: it may have been destroyed, or registered anew, meanwhile)
            msh_call D = A;
            D.keys = p[0]; D.R = p[1]; D.S = p[2]; D.m = p[3]; D.qt = p[4]; D.qs = p[5]; D.z = p[6];
            D.status = p[7]; D.sig_R = A.sig_R ? p[8] : nullptr;
            size_t n_now = 0;
            if (int rc = msh_rows(D, n_now)) return rc;
            if (n_now != n) return fail(JJS_ERR_ARG, "the signer group was destroyed during the call");
            return msig_share_locked(D, st);
        });
}
static msh_call msh_make(int route, uint64_t handle, const void* keys, const void* R, const void* S, const void* m, const uint32_t* offsets,
                         size_t B, const void* qt, const void* qs, const void* z, size_t Q, void* status, void* sig_R) {
    msh_call A{};
    A.route = route; A.handle = handle; A.keys = keys; A.R = R; A.S = S; A.m = m; A.offsets_host = offsets; A.B = B;
    A.qt = qt; A.qs = qs; A.z = z; A.Q = Q; A.status = status; A.sig_R = sig_R;
    return A;
}
}  // extern "C++"

extern "C" {

int jjs_multisig_verify_share_dev(int format, const void* PK, const void* R, const void* S, const void* m, const uint32_t* offsets_host,
                                  size_t n_transcripts, const void* share_transcript, const void* share_slot, const void* z, size_t n_shares,
                                  void* share_status, void* sig_R, void* stream) {
    return msig_share_dev(msh_make(MSH_INLINE, 0, PK, R, S, m, offsets_host, n_transcripts, share_transcript, share_slot, z, n_shares,
                                   share_status, sig_R), format, stream);
}
int jjs_multisig_verify_share(int format, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m, const uint32_t* offsets,
                              size_t n_transcripts, const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z,
                              size_t n_shares, uint8_t* share_status, uint8_t* sig_R) {
    return msig_share_host(msh_make(MSH_INLINE, 0, PK, R, S, m, offsets, n_transcripts, share_transcript, share_slot, z, n_shares,
                                    share_status, sig_R), format);
}
int jjs_msig_group_verify_share_dev(jjs_msig_group h, int format, const void* R, const void* S, const void* m, size_t n_transcripts,
                                    const void* share_transcript, const void* share_slot, const void* z, size_t n_shares,
                                    void* share_status, void* sig_R, void* stream) {
    return msig_share_dev(msh_make(MSH_GROUP, h, nullptr, R, S, m, nullptr, n_transcripts, share_transcript, share_slot, z, n_shares,
                                   share_status, sig_R), format, stream);
}
int jjs_msig_group_verify_share(jjs_msig_group h, int format, const uint8_t* R, const uint8_t* S, const uint8_t* m, size_t n_transcripts,
                                const uint32_t* share_transcript, const uint32_t* share_slot, const uint8_t* z, size_t n_shares,
                                uint8_t* share_status, uint8_t* sig_R) {
    return msig_share_host(msh_make(MSH_GROUP, h, nullptr, R, S, m, nullptr, n_transcripts, share_transcript, share_slot, z, n_shares,
                                    share_status, sig_R), format);
}
int jjs_multisig_verify_share_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const void* R, const void* S, const void* m,
                                         const uint32_t* offsets_host, size_t n_transcripts, const void* share_transcript,
                                         const void* share_slot, const void* z, size_t n_shares, void* share_status, void* sig_R,
                                         void* stream) {
    return msig_share_dev(msh_make(MSH_KEYSET, ks, key_idx, R, S, m, offsets_host, n_transcripts, share_transcript, share_slot, z, n_shares,
                                   share_status, sig_R), format, stream);
}
int jjs_multisig_verify_share_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                                     const uint32_t* offsets, size_t n_transcripts, const uint32_t* share_transcript,
                                     const uint32_t* share_slot, const uint8_t* z, size_t n_shares, uint8_t* share_status, uint8_t* sig_R) {
    return msig_share_host(msh_make(MSH_KEYSET, ks, key_idx, R, S, m, offsets, n_transcripts, share_transcript, share_slot, z, n_shares,
                                    share_status, sig_R), format);
}

}  // extern "C"
