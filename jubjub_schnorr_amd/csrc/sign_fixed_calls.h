// Part of jjs_gpu.hip (included among the extern "C" entry points, behind the var-generator signers): signing and key derivation
// with a SecretKey in the single and double schemes (sign_fixed.h, include/jjs_gpu.h jjs_sign_fixed*, jjs_public_keys_fixed*).
// Generators of test and benchmark material, NOT constant time.  The kernels use the lane workspace of slot 0, as sign_kernel
// does, and are ordered with the other signing calls by that slot's event.

// A signing call with one key for all its items takes the keyed route (sign_fixed.h) from this many items on.  By record, as
// SIGN_SHARED_MIN_ITEMS (sign_vargen_calls.h): the smallest recorded n from which the keyed route beats the per-item route (the key
// row read with stride 0) by more than the spread of either side, there and at every larger recorded shape.  The pre-pass puts a
// launch and an inversion in front of every lane, and below 2^18 items a call is one trip of a fraction of the resident lanes whose
// time is one lane's latency: there the keyed route is the slower one.  profiles/r18_sign_fixed.jsonl, variants d and e, ms per
// call, per item / keyed (spreads in brackets):
//   single  n = 1 1.073 / 1.012 (0.02: a win); 64 0.828 / 0.882; 1 024 0.859 / 0.943; 16 384 0.881 / 0.948 -- three losses;
//           2^18 2.731 / 2.668 (0.08: within the spread); 2^20 10.95 / 10.41 (0.12: a win)
//   double  n = 1 1.201 / 1.577; 64 1.153 / 1.239; 1 024 1.203 / 1.269; 16 384 1.224 / 1.297 -- four losses;
//           2^18 3.849 / 3.663 (0.06: a win); 2^20 15.59 / 14.40 (0.25: a win)
// One constant serves both schemes, so it is the first shape at which both win and keep winning: 2^20.  (The double scheme alone
// would have 2^18; the single scheme's win at one item is followed by losses and does not count.)
constexpr size_t SIGN_KEYED_MIN_ITEMS = size_t(1) << 20;
constexpr size_t SIGN_KEY_BYTES = SF_KEY_WORDS * 4;
#if defined(JJS_PROFILING)
static int g_force_sign_keyed = 0;           // jjs_debug_force_path 0x400000: the keyed route at any n; 0x800000: at none
#endif

extern "C++" {
struct sf_call {
    int scheme;
    bool sign;                               // false: the derivation call (rnd, m and the signature outputs unused)
    const void *sk, *rnd, *m;
    size_t n_sk;
    void *u_out, *R_out, *Rp_out, *PK_out, *PKp_out, *sig_w, *pk_w, *status;
};
// What every form checks before anything else is looked at: the scheme and the n_sk rule.
static int sf_shape(int scheme, size_t n_sk, size_t n) {
    if (scheme != JJS_SCHEME_SINGLE && scheme != JJS_SCHEME_DOUBLE)
        return fail(JJS_ERR_ARG, "scheme must be JJS_SCHEME_SINGLE or JJS_SCHEME_DOUBLE (the var-generator scheme signs with jjs_sign_vargen_pt)");
    if (n && n_sk != n && n_sk != 1) return fail(JJS_ERR_ARG, "n_sk must be n (a key per item) or 1 (one for the call): %zu for %zu items", n_sk, n);
    return JJS_OK;
}
static int sf_pointers(const sf_call& A, bool device) {
    if (!A.sk || !A.status || (A.sign && (!A.rnd || !A.m))) return fail(JJS_ERR_ARG, "null pointer");
    if (A.sign ? !(A.u_out || A.R_out || A.Rp_out || A.sig_w) : !(A.PK_out || A.PKp_out || A.pk_w)) return fail(JJS_ERR_ARG, "the call has no output");
    if (A.scheme == JJS_SCHEME_SINGLE && (A.Rp_out || A.PKp_out)) return fail(JJS_ERR_ARG, "the single scheme has no R' and no PK'");
    if (device && (!aligned16(A.sk) || !aligned16(A.rnd) || !aligned16(A.m) || !aligned16(A.u_out) || !aligned16(A.R_out) || !aligned16(A.Rp_out) ||
                   !aligned16(A.PK_out) || !aligned16(A.PKp_out) || !aligned16(A.sig_w) || !aligned16(A.pk_w)))
        return fail(JJS_ERR_ARG, "misaligned pointer");
    return JJS_OK;
}
static bool sf_keyed_route(const sf_call& A, size_t n) {
    if (!A.sign || A.n_sk != 1) return false;
#if defined(JJS_PROFILING)
    if (g_force_sign_keyed) return g_force_sign_keyed == 1;
#endif
    return n > 1 && n >= SIGN_KEYED_MIN_ITEMS;
}
// The call on device columns, queued on st (under the engine's mutex, g the device; n > 0, the shape and the pointers checked).
static int sf_locked(const sf_call& A, size_t n, hipStream_t st) {
    big_slot();
    const bool keyed = sf_keyed_route(A, n), dbl = A.scheme == JJS_SCHEME_DOUBLE;
    if (keyed)
        if (int rc = g->sign_key.ensure(SIGN_KEY_BYTES)) return rc;
    sign_fixed_params P{};
    P.sk = (const uint8_t*)A.sk; P.rnd = (const uint8_t*)A.rnd; P.m = (const uint8_t*)A.m;
    P.sk_stride = (A.n_sk == 1 && n > 1) ? 0u : 32u;
    P.u_out = (uint8_t*)A.u_out; P.R_out = (uint8_t*)A.R_out; P.Rp_out = (uint8_t*)A.Rp_out; P.PK_out = (uint8_t*)A.PK_out;
    P.PKp_out = (uint8_t*)A.PKp_out; P.sig_w = (uint8_t*)A.sig_w; P.pk_w = (uint8_t*)A.pk_w; P.status = (uint8_t*)A.status;
    P.comb_g = g->comb_g; P.comb_gn = g->comb_gn; P.n = n; P.workspace = g->slots[0].workspace;
    if (int rc = begin_shared(st)) return rc;
    auto queue = [&]() -> int {
        const dim3 grid(grid_for(g->grid_sign_fixed, n));
        if (!A.sign) {
            size_t blocks = (n + BLOCK - 1) / BLOCK;
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL(derive_fixed_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, P, dbl ? 1 : 0);
        } else if (keyed) {
            P.key = reinterpret_cast<uint32_t*>(g->sign_key.get());
            hipLaunchKernelGGL(sign_fixed_key_kernel, dim3(1), dim3(BLOCK), 0, st, P, dbl ? 1 : 0);
            if (dbl) hipLaunchKernelGGL(sign_fixed_keyed_double_kernel, grid, dim3(BLOCK), 0, st, P);
            else hipLaunchKernelGGL(sign_fixed_keyed_single_kernel, grid, dim3(BLOCK), 0, st, P);
        } else if (dbl) hipLaunchKernelGGL(sign_fixed_double_kernel, grid, dim3(BLOCK), 0, st, P);
        else hipLaunchKernelGGL(sign_fixed_single_kernel, grid, dim3(BLOCK), 0, st, P);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    };
    const int rc = queue();
    const int rc2 = end_shared(st);             // the slot's event covers whatever was queued, also when a step failed
    return rc ? rc : rc2;
}
static int sf_dev(const sf_call& A, size_t n, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (int rc = sf_shape(A.scheme, A.n_sk, n)) return rc;
    if (n == 0) return JJS_OK;
    if (int rc = sf_pointers(A, true)) return rc;
    return no_throw([&] { return sf_locked(A, n, (hipStream_t)stream); });
}
// The same from host buffers, blocking, on the frame of staged_host_call.h.  The staged sk and rnd are marked secret: the frame
// clears them on the stream behind the last kernel, before the call returns.
// parts: m, sk, rnd in; u_out, R_out, Rp_out, PK_out, PKp_out, sig_w, pk_w, status out (an output the caller does not ask for: empty)
static int sf_host(const sf_call& H, size_t n) {
    return staged_host_call(
        [&](bool& go) -> int {
            if (int rc = sf_shape(H.scheme, H.n_sk, n)) return rc;
            if (n == 0) return JJS_OK;
            go = true;
            return sf_pointers(H, false);
        },
        [&] {
            const size_t nk = H.n_sk, dbl = H.scheme == JJS_SCHEME_DOUBLE ? 1 : 0, in = H.sign ? n * 32 : 0;
            auto out = [](void* dst, size_t bytes) { return stage_part{dst ? bytes : 0, nullptr, dst}; };
            return std::vector<stage_part>{{in, H.m, nullptr}, {nk * 32, H.sk, nullptr}, {in, H.rnd, nullptr},
                                           out(H.u_out, n * 32), out(H.R_out, n * 64), out(H.Rp_out, n * 64), out(H.PK_out, nk * 64),
                                           out(H.PKp_out, nk * 64), out(H.sig_w, n * (64 + 32 * dbl)), out(H.pk_w, nk * (32 + 32 * dbl)),
                                           out(H.status, n)};
        },
        [&](uint8_t* const* p, hipStream_t st) {
            sf_call A = H;
            A.m = H.sign ? p[0] : nullptr; A.sk = p[1]; A.rnd = H.sign ? p[2] : nullptr;
            void** const col[8] = {&A.u_out, &A.R_out, &A.Rp_out, &A.PK_out, &A.PKp_out, &A.sig_w, &A.pk_w, &A.status};
            for (int j = 0; j < 8; ++j)
                if (*col[j]) *col[j] = p[3 + j];
            return sf_locked(A, n, st);
        },
        stage_secrets{1, 2});
}
}  // extern "C++"

extern "C" {

int jjs_sign_fixed_dev(int scheme, const void* sk, size_t n_sk, const void* rnd, const void* m, size_t n, void* u_out, void* R_out, void* Rp_out,
                       void* PK_out, void* PKp_out, void* sig_w_out, void* pk_w_out, void* status, void* stream) {
    sf_call A{scheme, true, sk, rnd, m, n_sk, u_out, R_out, Rp_out, PK_out, PKp_out, sig_w_out, pk_w_out, status};
    return sf_dev(A, n, stream);
}
int jjs_sign_fixed(int scheme, const uint8_t* sk, size_t n_sk, const uint8_t* rnd, const uint8_t* m, size_t n, uint8_t* u_out, uint8_t* R_out,
                   uint8_t* Rp_out, uint8_t* PK_out, uint8_t* PKp_out, uint8_t* sig_w_out, uint8_t* pk_w_out, uint8_t* status) {
    sf_call A{scheme, true, sk, rnd, m, n_sk, u_out, R_out, Rp_out, PK_out, PKp_out, sig_w_out, pk_w_out, status};
    return sf_host(A, n);
}
int jjs_public_keys_fixed_dev(int scheme, const void* sk, size_t n, void* PK_out, void* PKp_out, void* pk_w_out, void* status, void* stream) {
    sf_call A{scheme, false, sk, nullptr, nullptr, n, nullptr, nullptr, nullptr, PK_out, PKp_out, nullptr, pk_w_out, status};
    return sf_dev(A, n, stream);
}
int jjs_public_keys_fixed(int scheme, const uint8_t* sk, size_t n, uint8_t* PK_out, uint8_t* PKp_out, uint8_t* pk_w_out, uint8_t* status) {
    sf_call A{scheme, false, sk, nullptr, nullptr, n, nullptr, nullptr, nullptr, PK_out, PKp_out, nullptr, pk_w_out, status};
    return sf_host(A, n);
}
// [0] the lanes of the SecretKey signing kernels that are resident at once on the current device (their grid limit times the block
// size: a call of more items takes a second trip through the grid-stride loop); [1] the smallest n the keyed route serves --
// UINT64_MAX: no call takes it by size, one key for the call is read by the per-item route with stride 0 at every n.
int jjs_debug_sign_fixed_limits(uint64_t out[2]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[0] = (uint64_t)g->grid_sign_fixed * BLOCK;
    out[1] = SIGN_KEYED_MIN_ITEMS == SIZE_MAX ? UINT64_MAX : (uint64_t)(SIGN_KEYED_MIN_ITEMS < 2 ? 2 : SIGN_KEYED_MIN_ITEMS);
    return JJS_OK;
}

}  // extern "C"
