// Part of jjs_gpu.hip (included among the extern "C" entry points, behind keyset_calls.h, whose column widths and staging it
// shares): jjs_keys_check(_dev) and jjs_signatures_check(_dev) -- `is_valid` alone (points_check.h, include/jjs_gpu.h).

static_assert(PC_AFFINE == JJS_FORMAT_AFFINE && PC_EXT == JJS_FORMAT_EXT && PC_WIRE == JJS_FORMAT_WIRE, "points_check.h counts the formats as the ABI does");
static points_check_call keys_check_call(int scheme, int format, const void* K0, const void* K1, void* A0_out, void* A1_out) {
    return pc_keys_call(keyset_cols(scheme), (uint32_t)format, K0, K1, A0_out, A1_out);
}
static points_check_call signatures_check_call(int scheme, int format, const void* s0, const void* s1, const void* s2, void* u_out, void* R_out,
                                               void* Rp_out) {
    return pc_signatures_call(scheme == JJS_SCHEME_DOUBLE ? 2u : 1u, (uint32_t)format, s0, s1, s2, u_out, R_out, Rp_out);
}

// The launches of one call on stream s (g is the device): the tally cleared, then one lane per point.  Extended points whose
// affine form is wanted are normalised first (normalize.h, plain mode: one shared inversion per lane's items) into the output
// columns -- into the wire area of a call slot where the caller wants only one of two -- and checked there in affine mode;
// that is the only shape that takes a slot.
static int points_check_launch(const points_check_call& Q, size_t n, void* status, void* tally, hipStream_t s) {
    points_check_params C = pc_params(Q, n, (uint8_t*)status, (unsigned long long*)tally, dlog_tables{g->dlog_pow, g->dlog_hash});
    const bool normalise = pc_normalises(Q);
    clear_params Z{};
    Z.p[0] = tally; Z.bytes[0] = tally ? 4 * sizeof(unsigned long long) : 0;
    if (normalise) {
        pick_slot(n, s);
        if (int rc = sl->wire.ensure(n)) return rc;
        if (int rc = begin_shared(s)) return rc;
        Z.p[1] = wire_bad(); Z.bytes[1] = n;
    }
    if (tally || normalise) {
        const uint64_t units = n / 16 / BLOCK + 1;
        hipLaunchKernelGGL(clear_kernel, dim3((unsigned)(units < 256 ? units : 256)), dim3(BLOCK), 0, s, Z);
    }
    const dim3 grid((unsigned)(((uint64_t)n * Q.n_pts + BLOCK - 1) / BLOCK));                   // n <= 2^32: points_check_args
    if (normalise) {
        normalize_params N{};
        N.n_src = Q.n_pts; N.bad = wire_bad(); N.scratch = wire_scratch(0);
        for (uint32_t k = 0; k < Q.n_pts; ++k) {
            N.src[k] = Q.src[k];
            N.out[k] = C.out[k] ? C.out[k] : wire_pts((int)k);
        }
        if (int rc = launch_normalize(N, 0, n, n, s)) return rc;
        pc_over_normalised(C, N);
        hipLaunchKernelGGL(points_check_kernel<PC_AFFINE>, grid, dim3(BLOCK), 0, s, C);
        HIP_TRY(hipGetLastError());
        return end_shared(s);
    }
    if (Q.format == JJS_FORMAT_AFFINE) hipLaunchKernelGGL(points_check_kernel<PC_AFFINE>, grid, dim3(BLOCK), 0, s, C);
    else if (Q.format == JJS_FORMAT_EXT) hipLaunchKernelGGL(points_check_kernel<PC_EXT>, grid, dim3(BLOCK), 0, s, C);
    else hipLaunchKernelGGL(points_check_kernel<PC_WIRE>, grid, dim3(BLOCK), 0, s, C);
    HIP_TRY(hipGetLastError());
    return JJS_OK;
}

// The arguments of a call: `cols` input columns of w[i] bytes per item (0: the format does not take the column, which must
// then be NULL) and `outs` nullable outputs of out_w[j] bytes per item, the statuses first (0: the scheme has no such output,
// which must then be NULL); device pointers must be 16-byte aligned (the tally 8).
static int points_check_args(int scheme, int format, const size_t* w, const void* const* col, size_t cols, const void* const* out, size_t outs,
                             const size_t* out_w, size_t n, const void* tally, bool device) {
    if (scheme < 0 || scheme > 2 || format < 0 || format > 2) return fail(JJS_ERR_ARG, "scheme / format out of range");
    if (n > ((size_t)1 << 32)) return fail(JJS_ERR_ARG, "a call checks at most 2^32 items");
    for (size_t i = 0; i < cols; ++i) {
        if (w[i] && (!col[i] || (device && !aligned16(col[i])))) return fail(JJS_ERR_ARG, "null or misaligned column %zu", i);
        if (!w[i] && col[i]) return fail(JJS_ERR_ARG, "column %zu is not one of this scheme and format", i);
    }
    for (size_t j = 0; j < outs; ++j) {
        if (out[j] && !out_w[j]) return fail(JJS_ERR_ARG, "output %zu is not one of this scheme", j);
        if (device && out[j] && !aligned16(out[j])) return fail(JJS_ERR_ARG, "misaligned output %zu", j);
    }
    if (device && (reinterpret_cast<uintptr_t>(tally) & 7u)) return fail(JJS_ERR_ARG, "misaligned tally");
    return JJS_OK;
}
static int points_check_dev(int scheme, int format, const size_t* w, const void* const* col, size_t cols, void* const* out, size_t outs,
                            const size_t* out_w, const points_check_call& Q, size_t n, void* status, void* tally, void* stream) {
    if (int rc = points_check_args(scheme, format, w, col, n ? cols : 0, out, n ? outs : 0, out_w, n, tally, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (tally) HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(unsigned long long), s));
        return JJS_OK;
    }
    return no_throw([&] { return points_check_launch(Q, n, status, tally, s); });
}

// From host buffers, blocking: the route of jjs_keyset_find -- the columns go to the device's key-set staging area, the call
// runs on the device's key-set stream, the statuses, the tally and the requested outputs come back.  One such call at a time per
// device (host_mu); the engine's mutex is held only to check the arguments and to queue the launches.
// out[0] is the status column (1 byte per item), out[1..] the outputs of the call in its order, out_w their bytes per item.
extern "C++" {
template <class MakeCall>
static int points_check_host(int scheme, int format, const size_t* w, const void* const* col, size_t cols, void* const* out, size_t outs,
                             const size_t* out_w, size_t n, uint64_t tally[4], MakeCall make_call) {
    device_state* dev = nullptr;
    {
        std::lock_guard<std::mutex> lock(L.mu);
        if (int rc = check_ready()) return rc;
        if (int rc = points_check_args(scheme, format, w, col, n ? cols : 0, out, n ? outs : 0, out_w, n, nullptr, false)) return rc;
        if (n == 0) {
            if (tally) for (int i = 0; i < 4; ++i) tally[i] = 0;
            return JJS_OK;
        }
        dev = g;
        ++g_blocking_calls;
    }
    blocking_call_leave leave_on_every_way_out;
    std::lock_guard<std::mutex> big(dev->host_mu);
    g = dev;
    return no_throw([&]() -> int {
        size_t out_bytes[5] = {};
        out_bytes[0] = 256;                                   // the tally; then the statuses and the outputs the caller wants
        for (size_t j = 0; j < outs; ++j) out_bytes[1 + j] = (j == 0 || out[j]) ? out_w[j] * n : 0;
        keyset_stage S{};
        if (int rc = keyset_stage_in(dev, w, col, cols, n, out_bytes, outs + 1, S)) return rc;
        if (int rc = keyset_launch_locked(dev, nullptr, [&](keyset_entry*, const keyset_copy*) {
                return points_check_launch(make_call(S), n, S.out[1], S.out[0], S.s);
            }))
            return rc;
        for (size_t j = 0; j < outs; ++j)
            if (out[j]) HIP_TRY(hipMemcpyAsync(out[j], S.out[1 + j], out_w[j] * n, hipMemcpyDeviceToHost, S.s));
        unsigned long long t[4] = {};
        HIP_TRY(hipMemcpyAsync(t, S.out[0], sizeof(t), hipMemcpyDeviceToHost, S.s));
        HIP_TRY(hipStreamSynchronize(S.s));
        if (tally) for (int i = 0; i < 4; ++i) tally[i] = t[i];
        return JJS_OK;
    });
}
}  // extern "C++"

extern "C" {

int jjs_keys_check_dev(int scheme, int format, const void* K0, const void* K1, size_t n, void* status, void* tally, void* A0_out, void* A1_out,
                       void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    size_t w[2] = {};
    if (scheme >= 0 && scheme <= 2 && format >= 0 && format <= 2) keyset_key_widths(keyset_cols(scheme), format, w);
    const void* col[2] = {K0, K1};
    void* out[3] = {status, A0_out, A1_out};
    const size_t out_w[3] = {1, 64, scheme == JJS_SCHEME_SINGLE ? 0u : 64u};
    return points_check_dev(scheme, format, w, col, 2, out, 3, out_w, keys_check_call(scheme, format, K0, K1, A0_out, A1_out), n, status, tally, stream);
}

int jjs_keys_check(int scheme, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint8_t* status, uint64_t tally[4], uint8_t* A0_out,
                   uint8_t* A1_out) {
    size_t w[2] = {};
    if (scheme >= 0 && scheme <= 2 && format >= 0 && format <= 2) keyset_key_widths(keyset_cols(scheme), format, w);
    const void* col[2] = {K0, K1};
    void* out[3] = {status, A0_out, A1_out};
    const size_t out_w[3] = {1, 64, scheme == JJS_SCHEME_SINGLE ? 0u : 64u};
    return points_check_host(scheme, format, w, col, 2, out, 3, out_w, n, tally, [&](const keyset_stage& S) {
        return keys_check_call(scheme, format, S.d[0], S.d[1], A0_out ? S.out[2] : nullptr, A1_out ? S.out[3] : nullptr);
    });
}

int jjs_signatures_check_dev(int scheme, int format, const void* s0, const void* s1, const void* s2, size_t n, void* status, void* tally,
                             void* u_out, void* R_out, void* Rp_out, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    size_t w[3] = {};
    if (scheme >= 0 && scheme <= 2 && format >= 0 && format <= 2) keyset_sig_widths(scheme, format, w);
    const void* col[3] = {s0, s1, s2};
    void* out[4] = {status, u_out, R_out, Rp_out};
    const size_t out_w[4] = {1, 32, 64, scheme == JJS_SCHEME_DOUBLE ? 64u : 0u};
    return points_check_dev(scheme, format, w, col, 3, out, 4, out_w, signatures_check_call(scheme, format, s0, s1, s2, u_out, R_out, Rp_out), n,
                            status, tally, stream);
}

int jjs_signatures_check(int scheme, int format, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, size_t n, uint8_t* status,
                         uint64_t tally[4], uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out) {
    size_t w[3] = {};
    if (scheme >= 0 && scheme <= 2 && format >= 0 && format <= 2) keyset_sig_widths(scheme, format, w);
    const void* col[3] = {s0, s1, s2};
    void* out[4] = {status, u_out, R_out, Rp_out};
    const size_t out_w[4] = {1, 32, 64, scheme == JJS_SCHEME_DOUBLE ? 64u : 0u};
    return points_check_host(scheme, format, w, col, 3, out, 4, out_w, n, tally, [&](const keyset_stage& S) {
        return signatures_check_call(scheme, format, S.d[0], S.d[1], S.d[2], u_out ? S.out[2] : nullptr, R_out ? S.out[3] : nullptr,
                                     Rp_out ? S.out[4] : nullptr);
    });
}

}  // extern "C"
