// Part of jjs_gpu.hip (included among the extern "C" entry points, behind msig_verify_calls.h): the signer's half of the
// multisignature scheme (msig_sign.h, include/jjs_gpu.h jjs_multisig_round1_dev, jjs_multisig_sign*) -- the front of the combine
// call (passes 0-3) with the check pass behind pass 0, pass 4 without a column of shares, and the share pass.  Generators of test
// and benchmark material, NOT constant time.  The passes use the multisignature scratch, which belongs to slot 0; pk_agg and RSa,
// which a signing call does not return, are columns of that scratch.

extern "C++" {
struct ms_call {
    bool ext;
    const void *PK, *R, *S, *m;
    const void *signer_row, *sk, *r, *s;
    size_t n_signing;
    void *z_out, *status;
};
// The call on device columns, queued on st (under the engine's mutex, g the device; n_transcripts > 0, n_signing > 0).
static int msig_sign_locked(const ms_call& A, const uint32_t* offsets_host, size_t n_transcripts, hipStream_t st) {
    size_t n = 0;
    if (int rc = msig_check_offsets(offsets_host, n_transcripts, n)) return rc;
    if (!A.signer_row && A.n_signing != n)
        return fail(JJS_ERR_ARG, "without signer_row a call signs every row: %zu signing rows, %zu participant rows", A.n_signing, n);
    if ((n && !all_ok(A.PK, A.R, A.S)) || !all_ok(A.m, A.sk, A.r, A.s, A.z_out) || !A.status || (reinterpret_cast<uintptr_t>(A.signer_row) & 3u))
        return fail(JJS_ERR_ARG, "null or misaligned pointer");
    const size_t B = n_transcripts;
    msig_caps need;
    need.rows = n; need.transcripts = B;
    if (A.ext) need.ext_rows = n;
    need.sign_rows = n ? n : 1; need.sign_transcripts = B;
    return msig_scratch_call(need, st, [&](const msig_scratch& W) -> int {
        const uint8_t* pts[3] = {(const uint8_t*)A.PK, (const uint8_t*)A.R, (const uint8_t*)A.S};
        msig_sign_params G{};
        msig_params& P = G.M;
        msig_params_common(P, W, B, n);
        P.m = (const uint8_t*)A.m;
        P.agg_pk = W.sign_agg; P.sig_R = W.sign_rsa;
        P.e_pt = W.e_pt;
        G.pk_repeats = W.pk_repeats; G.bad_enc = W.bad_enc; G.dup_nonce = W.dup_nonce;
        G.signer_row = (const uint32_t*)A.signer_row;
        G.sk = (const uint8_t*)A.sk; G.r = (const uint8_t*)A.r; G.s = (const uint8_t*)A.s;
        G.n_signing = A.n_signing;
        G.z_out = (uint8_t*)A.z_out; G.status = (uint8_t*)A.status;
        HIP_TRY(hipMemcpyAsync(W.offsets, offsets_host, (B + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(W.pk_repeats, 0, W.sign_flag_words * sizeof(uint32_t), st));
        if (A.ext && n)
            if (int rc = msig_normalize(W, pts, 3, n, st)) return rc;
        P.PK = pts[0]; P.R = pts[1]; P.S = pts[2];
        launch_msig_pass(P, 0, st);
        if (n) {
            hipLaunchKernelGGL(msig_sign_check_kernel, dim3(grid_for(g->grid_msig, n)), dim3(BLOCK), 0, st, G);   // behind the map: it reads tr_of
            for (int pass = 1; pass < 4; ++pass) launch_msig_pass(P, pass, st);
            const dim3 closing(msig_pass_grid(P, 4));
            hipLaunchKernelGGL(msig_sign_final_kernel, closing, dim3(BLOCK), 0, st, P);           // pass 4 without a column of shares
            P.hash_lanes = 1;
        }
        hipLaunchKernelGGL(msig_sign_share_kernel, dim3(grid_for(g->grid_msig, A.n_signing)), dim3(BLOCK), 0, st, G);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}
}  // extern "C++"

extern "C" {

int jjs_multisig_round1_dev(const void* r, const void* s, size_t n, void* R_out, void* S_out, void* bad_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (n == 0) return JJS_OK;
    if (!all_ok(r, s, R_out, S_out)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(msig_round1_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const uint8_t*)r, (const uint8_t*)s,
                       (uint64_t)n, g->comb_g, (uint8_t*)R_out, (uint8_t*)S_out, (uint8_t*)bad_out);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}

int jjs_multisig_sign_dev(int format, const void* PK, const void* R, const void* S, const void* m, const uint32_t* offsets_host,
                          size_t n_transcripts, const void* signer_row, const void* sk, const void* r, const void* s, size_t n_signing,
                          void* z_out, void* sign_status, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    ms_call A{};
    int fmt = JJS_FORMAT_AFFINE;
    if (int rc = msig_format(format, MSIG_FORMATS_POINTS, fmt)) return rc;
    if (n_transcripts == 0 || n_signing == 0) return JJS_OK;
    A.ext = fmt == JJS_FORMAT_EXT;
    A.PK = PK; A.R = R; A.S = S; A.m = m; A.signer_row = signer_row; A.sk = sk; A.r = r; A.s = s; A.n_signing = n_signing;
    A.z_out = z_out; A.status = sign_status;
    return no_throw([&] { return msig_sign_locked(A, offsets_host, n_transcripts, (hipStream_t)stream); });
}

// The same from host buffers, blocking, on the frame of staged_host_call.h.  The staged sk, r and s are marked secret: the frame
// clears them on the stream behind the share pass, before the call returns.
// parts: PK, R, S, m, signer_row, sk, r, s in; z_out, sign_status out
int jjs_multisig_sign(int format, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m, const uint32_t* offsets,
                      size_t n_transcripts, const uint32_t* signer_row, const uint8_t* sk, const uint8_t* r, const uint8_t* s, size_t n_signing,
                      uint8_t* z_out, uint8_t* sign_status) {
    const size_t B = n_transcripts, k = n_signing;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            if (int rc = msig_format(format, MSIG_FORMATS_POINTS, fmt)) return rc;
            if (B == 0 || k == 0) return JJS_OK;
            if (int rc = msig_check_offsets(offsets, B, n)) return rc;
            if (!signer_row && k != n)
                return fail(JJS_ERR_ARG, "without signer_row a call signs every row: %zu signing rows, %zu participant rows", k, n);
            if ((n && (!PK || !R || !S)) || !m || !sk || !r || !s || !z_out || !sign_status) return fail(JJS_ERR_ARG, "null pointer");
            go = true;
            return JJS_OK;
        },
        [&] {
            const size_t w = msig_point_bytes(fmt);
            return std::vector<stage_part>{{n * w, PK, nullptr}, {n * w, R, nullptr}, {n * w, S, nullptr}, {B * 32, m, nullptr},
                                           {signer_row ? k * 4 : 0, signer_row, nullptr}, {k * 32, sk, nullptr}, {k * 32, r, nullptr},
                                           {k * 32, s, nullptr}, {k * 32, nullptr, z_out}, {k, nullptr, sign_status}};
        },
        [&](uint8_t* const* p, hipStream_t st) {
            ms_call A{};
            A.ext = fmt == JJS_FORMAT_EXT; A.PK = p[0]; A.R = p[1]; A.S = p[2]; A.m = p[3]; A.signer_row = signer_row ? p[4] : nullptr;
            A.sk = p[5]; A.r = p[6]; A.s = p[7]; A.n_signing = k; A.z_out = p[8]; A.status = p[9];
            return msig_sign_locked(A, offsets, B, st);
        },
        stage_secrets{5, 3});
}

}  // extern "C"
