// Part of jjs_gpu.hip (included among the extern "C" entry points, behind msig_keyset_calls.h): the verifier's half of the
// multisignature scheme (msig_verify.h, include/jjs_gpu.h jjs_multisig_aggregate_pk*, jjs_multisig_verify*) -- the two front
// passes of the combine call with a check (or the key set's gather) between them, the sum pass, and for a verification call the
// resident single-scheme call on the aggregate column with the clear pass behind it.
// Lifetime: the passes use the multisignature scratch, which belongs to slot 0; the verification stage runs in a slot of its
// own choosing and reads the aggregate from the caller's memory, but in the extended format its R column is the normalised
// one in that scratch.  So slot 0's event is recorded only after the verification's launches and the clear pass have been
// queued: the scratch's next user, on whatever stream, waits for all of them.
// The wire format: the keys and R are decoded into those columns (msig_decode_kernel), R out of the R half of the u || R rows;
// the resident single-scheme call reads packed columns, so u is copied out of its half of the rows into the column behind R's.

extern "C++" {
struct mv_call {
    bool keyset, verify;
    int fmt;                              // JJS_FORMAT_*: of the inline form's PK and R, of the key-set form's R.  Wire: u and R are
                                          // the two halves of the B x 64 signature rows (u = sig_w, R = sig_w + 32, stride 64)
    const keyset_entry* k;                // the key-set form: the set and its copy on the device
    const keyset_copy* c;
    const void *keys;                     // PK (N x 64 / N x 96 / N x 32) or key_idx (N x uint32)
    const void *u, *R, *m;                // a verification call
    void *agg_pk, *vec_status, *status, *tally;
};
// one column of `rows` points in format fmt (extended, or wire at `wire_stride` bytes a row) into normalised column `slot` of the
// scratch, in poison mode; col is re-aimed at it
static int mv_ingest(int fmt, const msig_scratch& W, const uint8_t*& col, int slot, size_t rows, uint32_t wire_stride, hipStream_t s) {
    if (fmt == JJS_FORMAT_WIRE) {
        msig_decode_params D{};
        D.n_src = 1;
        D.src[0] = fe_src{col, wire_stride, 0};
        D.out[0] = W.norm[slot];
        col = W.norm[slot];
        return launch_msig_decode(D, rows, s);
    }
    normalize_params N{};
    N.n_src = 1; N.poison = 1; N.scratch = W.prefix;
    N.src[0] = fe_src{col, 96, 0};
    N.out[0] = W.norm[slot];
    col = W.norm[slot];
    return launch_normalize(N, 0, rows, rows, s);
}
// The call on device columns, queued on s (under the engine's mutex, g the device; n_transcripts > 0).
static int msig_verify_locked(const mv_call& A, const uint32_t* offsets_host, size_t n_transcripts, hipStream_t s) {
    size_t n = 0;
    if (int rc = msig_check_offsets(offsets_host, n_transcripts, n)) return rc;
    if (n && (A.keyset ? (!A.keys || (reinterpret_cast<uintptr_t>(A.keys) & 3u)) : !all_ok(A.keys))) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    if (!all_ok(A.agg_pk)) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    if (A.verify && (!all_ok(A.u, A.R, A.m) || (A.status && !aligned16(A.status)) || (reinterpret_cast<uintptr_t>(A.tally) & 7u)))
        return fail(JJS_ERR_ARG, "null or misaligned pointer");
    const size_t B = n_transcripts;
    const bool ingest = A.fmt != JJS_FORMAT_AFFINE, wire = A.fmt == JJS_FORMAT_WIRE;
    msig_caps need;
    need.rows = n; need.transcripts = B;
    if (ingest) need.ext_rows = A.keyset ? (A.verify ? B : 0) : (A.verify && B > n ? B : n);
    if (A.keyset) { need.ks_rows = n ? n : 1; need.ks_transcripts = B; }
    return msig_scratch_call(need, s, [&](const msig_scratch& W) -> int {
        msig_verify_keyset_params VK{};
        msig_params& P = VK.K.M;
        msig_params_common(P, W, B, n, false);
        P.agg_pk = (uint8_t*)A.agg_pk;
        VK.vec_status = (uint8_t*)A.vec_status; VK.poison = A.verify ? 1u : 0u;
        if (A.keyset) {
            P.PK = W.ks_pk;
            msig_keyset_fill(VK.K, *A.k, *A.c, A.keys, W, W.ks_refused);
        } else {
            VK.K.refused = W.a_words;          // the inline form: a verifier's call computes no `a`, its words hold the refused flags
        }
        const uint8_t *pk = A.keyset ? nullptr : (const uint8_t*)A.keys, *r = (const uint8_t*)A.R, *u = (const uint8_t*)A.u;
        HIP_TRY(hipMemcpyAsync(W.offsets, offsets_host, (B + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(VK.K.refused, 0, B * sizeof(uint32_t), s));
        if (ingest && !A.keyset)
            if (int rc = mv_ingest(A.fmt, W, pk, 0, n, 32, s)) return rc;
        if (ingest && A.verify)
            if (int rc = mv_ingest(A.fmt, W, r, A.keyset ? 0 : 1, B, 64, s)) return rc;
        if (wire && A.verify) {
            uint8_t* packed = W.norm[A.keyset ? 1 : 2];              // B x 32 in a column of at least B rows of 64
            HIP_TRY(hipMemcpy2DAsync(packed, 32, u, 64, 32, B, hipMemcpyDeviceToDevice, s));
            u = packed;
        }
        if (!A.keyset) P.PK = pk;
        const dim3 per_row(grid_for(g->grid_msig, n)), per_vector(grid_for(g->grid_msig, B));
        launch_msig_pass(P, 0, s);
        if (n) {
            // the gather or the check, behind the map (both read tr_of), then pass 1
            if (A.keyset) {
                hipLaunchKernelGGL(msig_keyset_gather_kernel, per_row, dim3(BLOCK), 0, s, VK.K);
                const dim3 delin(msig_pass_grid(P, 1));
                hipLaunchKernelGGL(msig_keyset_delin_kernel, delin, dim3(BLOCK), 0, s, VK.K);
            } else {
                hipLaunchKernelGGL(msig_verify_check_kernel, per_row, dim3(BLOCK), 0, s, mv_of(VK));
                launch_msig_pass(P, 1, s);
            }
            P.hash_lanes = 1;
        }
        hipLaunchKernelGGL(msig_verify_sum_kernel, per_vector, dim3(BLOCK), 0, s, mv_of(VK));
        HIP_TRY(hipGetLastError());
        if (!A.verify) return JJS_OK;
        // The verification stage: the resident single-scheme affine call on (u, R, agg_pk, m), in a slot of its own (build_call moves
        // sl; the frame puts it back), on the same stream, under this hold of the mutex.
        const void* d[4] = {u, r, A.agg_pk, A.m};
        staged_call C;
        if (int rc = build_call(SHAPES[JJS_SCHEME_SINGLE][JJS_FORMAT_AFFINE], d, B, A.status, A.tally, s, C)) return rc;
        if (int rc = launch_staged(C, s)) return rc;
        hipLaunchKernelGGL(msig_verify_clear_kernel, per_vector, dim3(BLOCK), 0, s, mv_of(VK));
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}

// a _dev entry point: the checks in front of the call, under the engine's mutex
static int msig_verify_dev(mv_call A, const jjs_keyset* ks, int format, unsigned formats, const uint32_t* offsets_host, size_t n_transcripts, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (ks) {
        keyset_entry* k = nullptr;
        if (int rc = msig_keyset_find(*ks, g, k, A.c)) return rc;
        A.k = k;
    }
    if (int rc = msig_format(format, formats, A.fmt)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_transcripts == 0) {
        if (A.verify && A.tally) HIP_TRY(hipMemsetAsync(A.tally, 0, 4 * sizeof(unsigned long long), s));
        return JJS_OK;
    }
    return no_throw([&] { return msig_verify_locked(A, offsets_host, n_transcripts, s); });
}

// a host-buffer entry point: blocking, on the frame of staged_host_call.h.  A's pointers are the caller's host buffers.
// parts: keys (PK or key_idx), u, R, m and an empty one in; agg_pk, status, tally, vec_status and an empty one out.  A wire call
// uploads its u || R rows as one column in u's part, R's part is empty, and R = u's part + 32.
static int msig_verify_host(mv_call A, const jjs_keyset* ks, int format, unsigned formats, const uint32_t* offsets, size_t n_transcripts, uint64_t* tally) {
    const size_t B = n_transcripts;
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            if (ks) {
                keyset_entry* k = nullptr;
                if (int rc = msig_keyset_find(*ks, g, k, A.c)) return rc;
            }
            if (int rc = msig_format(format, formats, A.fmt)) return rc;
            if (B == 0) {
                if (A.verify && tally) for (int k = 0; k < 4; ++k) tally[k] = 0;
                return JJS_OK;
            }
            if (int rc = msig_check_offsets(offsets, B, n)) return rc;
            if ((n && !A.keys) || !A.agg_pk || (A.verify && (!A.u || !A.R || !A.m))) return fail(JJS_ERR_ARG, "null pointer");
            go = true;
            return JJS_OK;
        },
        [&] {
            const bool wire = A.fmt == JJS_FORMAT_WIRE;
            const size_t w = msig_point_bytes(A.fmt), v = A.verify ? 1 : 0;
            return std::vector<stage_part>{{n * (A.keyset ? 4 : w), A.keys, nullptr}, {v * B * (wire ? 64 : 32), A.u, nullptr},
                                           {wire ? 0 : v * B * w, A.R, nullptr}, {v * B * 32, A.m, nullptr}, {0, nullptr, nullptr},
                                           {B * 64, nullptr, A.agg_pk}, {v * B, nullptr, A.status}, {v * 32, nullptr, tally},
                                           {(1 - v) * B, nullptr, A.vec_status}, {0, nullptr, nullptr}};
        },
        [&](uint8_t* const* p, hipStream_t s) -> int {
            mv_call D = A;
            if (ks) {                    // (the set is looked up again: it may have been destroyed meanwhile)
                keyset_entry* k = nullptr;
                if (int rc = msig_keyset_find(*ks, g, k, D.c)) return rc;
                D.k = k;
            }
            D.keys = p[0]; D.u = p[1]; D.R = A.fmt == JJS_FORMAT_WIRE ? p[1] + 32 : p[2]; D.m = p[3];
            D.agg_pk = p[5];
            D.status = A.status ? p[6] : nullptr;
            D.tally = tally ? p[7] : nullptr;
            D.vec_status = A.vec_status ? p[8] : nullptr;
            return msig_verify_locked(D, offsets, B, s);
        });
}
}  // extern "C++"

extern "C" {

int jjs_multisig_aggregate_pk_dev(int format, const void* PK, const uint32_t* offsets_host, size_t n_transcripts, void* agg_pk,
                                  void* vec_status, void* stream) {
    mv_call A{};
    A.keys = PK; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_dev(A, nullptr, format, MSIG_FORMATS_POINTS, offsets_host, n_transcripts, stream);
}
int jjs_multisig_aggregate_pk(int format, const uint8_t* PK, const uint32_t* offsets, size_t n_transcripts, uint8_t* agg_pk,
                              uint8_t* vec_status) {
    mv_call A{};
    A.keys = PK; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_host(A, nullptr, format, MSIG_FORMATS_POINTS, offsets, n_transcripts, nullptr);
}
int jjs_multisig_aggregate_pk_keyset_dev(jjs_keyset ks, const void* key_idx, const uint32_t* offsets_host, size_t n_transcripts,
                                         void* agg_pk, void* vec_status, void* stream) {
    mv_call A{};
    A.keyset = true; A.keys = key_idx; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_dev(A, &ks, JJS_FORMAT_AFFINE, MSIG_FORMATS_POINTS, offsets_host, n_transcripts, stream);
}
int jjs_multisig_aggregate_pk_keyset(jjs_keyset ks, const uint32_t* key_idx, const uint32_t* offsets, size_t n_transcripts,
                                     uint8_t* agg_pk, uint8_t* vec_status) {
    mv_call A{};
    A.keyset = true; A.keys = key_idx; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_host(A, &ks, JJS_FORMAT_AFFINE, MSIG_FORMATS_POINTS, offsets, n_transcripts, nullptr);
}

int jjs_multisig_verify_dev(int format, const void* PK, const uint32_t* offsets_host, const void* u, const void* R, const void* m,
                            size_t n_transcripts, void* agg_pk, void* status, void* tally, void* stream) {
    mv_call A{};
    A.verify = true; A.keys = PK; A.u = u; A.R = R; A.m = m; A.agg_pk = agg_pk; A.status = status; A.tally = tally;
    return msig_verify_dev(A, nullptr, format, MSIG_FORMATS_POINTS, offsets_host, n_transcripts, stream);
}
int jjs_multisig_verify(int format, const uint8_t* PK, const uint32_t* offsets, const uint8_t* u, const uint8_t* R, const uint8_t* m,
                        size_t n_transcripts, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]) {
    mv_call A{};
    A.verify = true; A.keys = PK; A.u = u; A.R = R; A.m = m; A.agg_pk = agg_pk; A.status = status;
    return msig_verify_host(A, nullptr, format, MSIG_FORMATS_POINTS, offsets, n_transcripts, tally);
}
int jjs_multisig_verify_keyset_dev(jjs_keyset ks, int format, const void* key_idx, const uint32_t* offsets_host, const void* u,
                                   const void* R, const void* m, size_t n_transcripts, void* agg_pk, void* status, void* tally,
                                   void* stream) {
    mv_call A{};
    A.keyset = true; A.verify = true; A.keys = key_idx; A.u = u; A.R = R; A.m = m; A.agg_pk = agg_pk; A.status = status; A.tally = tally;
    return msig_verify_dev(A, &ks, format, MSIG_FORMATS_POINTS, offsets_host, n_transcripts, stream);
}
int jjs_multisig_verify_keyset(jjs_keyset ks, int format, const uint32_t* key_idx, const uint32_t* offsets, const uint8_t* u,
                               const uint8_t* R, const uint8_t* m, size_t n_transcripts, uint8_t* agg_pk, uint8_t* status,
                               uint64_t tally[4]) {
    mv_call A{};
    A.keyset = true; A.verify = true; A.keys = key_idx; A.u = u; A.R = R; A.m = m; A.agg_pk = agg_pk; A.status = status;
    return msig_verify_host(A, &ks, format, MSIG_FORMATS_POINTS, offsets, n_transcripts, tally);
}

// the wire forms: PK_w is N x 32, sig_w is B x 64 = u || R (the layout of jjs_verify_single_wire)
static mv_call mv_verify_wire_call(bool keyset, const void* keys, const void* sig_w, const void* m, void* agg_pk, void* status, void* tally) {
    mv_call A{};
    A.keyset = keyset; A.verify = true; A.keys = keys; A.m = m;
    A.u = sig_w; A.R = sig_w ? (const uint8_t*)sig_w + 32 : nullptr;
    A.agg_pk = agg_pk; A.status = status; A.tally = tally;
    return A;
}
int jjs_multisig_aggregate_pk_wire_dev(const void* PK_w, const uint32_t* offsets_host, size_t n_transcripts, void* agg_pk, void* vec_status,
                                       void* stream) {
    mv_call A{};
    A.keys = PK_w; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_dev(A, nullptr, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets_host, n_transcripts, stream);
}
int jjs_multisig_aggregate_pk_wire(const uint8_t* PK_w, const uint32_t* offsets, size_t n_transcripts, uint8_t* agg_pk, uint8_t* vec_status) {
    mv_call A{};
    A.keys = PK_w; A.agg_pk = agg_pk; A.vec_status = vec_status;
    return msig_verify_host(A, nullptr, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets, n_transcripts, nullptr);
}
int jjs_multisig_verify_wire_dev(const void* PK_w, const uint32_t* offsets_host, const void* sig_w, const void* m, size_t n_transcripts,
                                 void* agg_pk, void* status, void* tally, void* stream) {
    mv_call A = mv_verify_wire_call(false, PK_w, sig_w, m, agg_pk, status, tally);
    return msig_verify_dev(A, nullptr, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets_host, n_transcripts, stream);
}
int jjs_multisig_verify_wire(const uint8_t* PK_w, const uint32_t* offsets, const uint8_t* sig_w, const uint8_t* m, size_t n_transcripts,
                             uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]) {
    mv_call A = mv_verify_wire_call(false, PK_w, sig_w, m, agg_pk, status, nullptr);
    return msig_verify_host(A, nullptr, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets, n_transcripts, tally);
}
int jjs_multisig_verify_keyset_wire_dev(jjs_keyset ks, const void* key_idx, const uint32_t* offsets_host, const void* sig_w, const void* m,
                                        size_t n_transcripts, void* agg_pk, void* status, void* tally, void* stream) {
    mv_call A = mv_verify_wire_call(true, key_idx, sig_w, m, agg_pk, status, tally);
    return msig_verify_dev(A, &ks, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets_host, n_transcripts, stream);
}
int jjs_multisig_verify_keyset_wire(jjs_keyset ks, const uint32_t* key_idx, const uint32_t* offsets, const uint8_t* sig_w, const uint8_t* m,
                                    size_t n_transcripts, uint8_t* agg_pk, uint8_t* status, uint64_t tally[4]) {
    mv_call A = mv_verify_wire_call(true, key_idx, sig_w, m, agg_pk, status, nullptr);
    return msig_verify_host(A, &ks, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, offsets, n_transcripts, tally);
}

}  // extern "C"
