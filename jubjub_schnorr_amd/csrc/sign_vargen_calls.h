// Part of jjs_gpu.hip (included among the extern "C" entry points, behind the signers): var-generator signing and key derivation
// with the generator as a point (sign_vargen.h, include/jjs_gpu.h jjs_sign_vargen_pt*, jjs_public_keys_vargen*).  Generators of
// test and benchmark material, NOT constant time.  The kernels use the lane workspace of slot 0, as sign_kernel does, and are
// ordered with the other signing calls by that slot's event; extended and wire generators are first brought to an affine column
// in slot 0's wire area, in poison mode.

// A signing call with one generator for all its items takes the shared-generator route (sign_vargen.h) from this many items on.
// By record, as VERDICT_MIN_ITEMS (verdict_calls.h): the smallest recorded n from which the shared route beats the per-item route by
// more than the spread of either side, there and at every larger recorded shape (profiles/r17_sign_vargen_pt.jsonl, variants e
// and f, ms per call: n = 1 2.88 against 2.41 with spreads of 0.7 and 0.4 -- no winner; 64 2.72 / 2.25; 1 024 2.76 / 2.32;
// 16 384 2.82 / 2.30; 2^18 10.2 / 5.35; 2^20 39.7 / 17.8, the spreads at most 0.3).
constexpr size_t SIGN_SHARED_MIN_ITEMS = 64;
constexpr size_t SIGN_BASES_BYTES = (MG_BASE_WORDS_PER_KEY * 4 + 255) / 256 * 256, SIGN_TABLE_BYTES = SIGN_BASES_BYTES + MG_TABLE_WORDS_PER_KEY * 4;
#if defined(JJS_PROFILING)
static int g_force_sign_shared = 0;          // jjs_debug_force_path 0x8000: the shared-generator route at any n; 0x200000: at none
#endif

extern "C++" {
static bool svg_shared_route(const struct svg_call& A, size_t n);
struct svg_call {
    int format;
    bool sign;                               // false: the derivation call (rnd, m, u_out, R_out unused)
    const void *sk, *Gen, *rnd, *m;
    size_t n_gen;
    void *u_out, *R_out, *PK_out, *Gen_out, *status;
};
static size_t svg_gen_width(int format) { return format == JJS_FORMAT_AFFINE ? 64 : (format == JJS_FORMAT_EXT ? 96 : 32); }
// What every form checks before anything else is looked at: the format and the n_gen rule.
static int svg_shape(int format, size_t n_gen, size_t n) {
    if (format != JJS_FORMAT_AFFINE && format != JJS_FORMAT_EXT && format != JJS_FORMAT_WIRE) return fail(JJS_ERR_ARG, "format out of range");
    if (n && n_gen != n && n_gen != 1) return fail(JJS_ERR_ARG, "n_gen must be n (a generator per item) or 1 (one for the call): %zu for %zu items", n_gen, n);
    return JJS_OK;
}
static int svg_pointers(const svg_call& A, bool device) {
    const bool need = A.sk && A.Gen && A.status && (A.sign ? (A.rnd && A.m && A.u_out && A.R_out) : A.PK_out != nullptr);
    if (!need) return fail(JJS_ERR_ARG, "null pointer");
    if (device && (!aligned16(A.sk) || !aligned16(A.Gen) || !aligned16(A.rnd) || !aligned16(A.m) || !aligned16(A.u_out) || !aligned16(A.R_out) ||
                   !aligned16(A.PK_out) || !aligned16(A.Gen_out)))
        return fail(JJS_ERR_ARG, "misaligned pointer");
    return JJS_OK;
}
static bool svg_shared_route(const svg_call& A, size_t n) {
    if (!A.sign || A.n_gen != 1) return false;
#if defined(JJS_PROFILING)
    if (g_force_sign_shared) return g_force_sign_shared == 1;
#endif
    return n >= SIGN_SHARED_MIN_ITEMS;
}
// The call on device columns, queued on st (under the engine's mutex, g the device; n > 0, the shape and the pointers checked).
static int svg_locked(const svg_call& A, size_t n, hipStream_t st) {
    big_slot();
    const uint8_t* gen = (const uint8_t*)A.Gen;
    if (A.format != JJS_FORMAT_AFFINE)
        if (int rc = sl->wire.ensure(A.n_gen)) return rc;
    const bool tabled = svg_shared_route(A, n);
    if (tabled)
        if (int rc = g->sign_tables.ensure(SIGN_TABLE_BYTES)) return rc;
    sign_vargen_params P{};
    P.sk = (const uint8_t*)A.sk; P.rnd = (const uint8_t*)A.rnd; P.m = (const uint8_t*)A.m;
    P.gen_stride = (A.n_gen == 1 && n > 1) ? 0u : 64u;
    P.u_out = (uint8_t*)A.u_out; P.R_out = (uint8_t*)A.R_out; P.PK_out = (uint8_t*)A.PK_out; P.Gen_out = (uint8_t*)A.Gen_out;
    P.status = (uint8_t*)A.status; P.n = n; P.workspace = g->slots[0].workspace;
    if (int rc = begin_shared(st)) return rc;
    auto queue = [&]() -> int {
        if (A.format == JJS_FORMAT_EXT) {
            normalize_params N{};
            N.n_src = 1; N.poison = 1; N.scratch = wire_scratch(0);
            N.src[0] = fe_src{gen, 96, 0}; N.out[0] = wire_pts(0);
            if (int rc = launch_normalize(N, 0, A.n_gen, A.n_gen, st)) return rc;
            gen = wire_pts(0);
        } else if (A.format == JJS_FORMAT_WIRE) {
            msig_decode_params D{};
            D.n_src = 1; D.src[0] = fe_src{gen, 32, 0}; D.out[0] = wire_pts(0);
            if (int rc = launch_msig_decode(D, A.n_gen, st)) return rc;
            gen = wire_pts(0);
        }
        P.gen = gen;
        const dim3 grid(grid_for(g->grid_sign, n));
        if (tabled) {
            // the tables of the one generator, whatever point it is (an unusable one: every lane refuses its item before it reads them)
            uint32_t* bases = reinterpret_cast<uint32_t*>(g->sign_tables.get());
            uint32_t* tables = reinterpret_cast<uint32_t*>(g->sign_tables.get() + SIGN_BASES_BYTES);
            hipLaunchKernelGGL(msig_group_chain_kernel, dim3(1), dim3(BLOCK), 0, st, gen, 1u, bases);
            hipLaunchKernelGGL(msig_group_table_kernel, dim3((unsigned)((kt_positions(MG_WINDOW) + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
                               (const uint32_t*)bases, tables, 1u);
            P.tables = tables;
            hipLaunchKernelGGL(sign_vargen_shared_kernel, grid, dim3(BLOCK), 0, st, P);
        } else if (A.sign) hipLaunchKernelGGL(sign_vargen_pt_kernel, grid, dim3(BLOCK), 0, st, P);
        else hipLaunchKernelGGL(derive_vargen_pt_kernel, grid, dim3(BLOCK), 0, st, P);
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    };
    const int rc = queue();
    const int rc2 = end_shared(st);             // the slot's event covers whatever was queued, also when a step failed
    return rc ? rc : rc2;
}
static int svg_dev(const svg_call& A, size_t n, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (int rc = svg_shape(A.format, A.n_gen, n)) return rc;
    if (n == 0) return JJS_OK;
    if (int rc = svg_pointers(A, true)) return rc;
    return no_throw([&] { return svg_locked(A, n, (hipStream_t)stream); });
}
// The same from host buffers, blocking, on the frame of staged_host_call.h.  The staged sk and rnd are marked secret: the frame
// clears them on the stream behind the last kernel, before the call returns.
// parts: Gen, m, sk, rnd in; u_out, R_out, PK_out, Gen_out, status out (an output the call does not have or the caller does not
// ask for: empty)
static int svg_host(const svg_call& H, size_t n) {
    return staged_host_call(
        [&](bool& go) -> int {
            if (int rc = svg_shape(H.format, H.n_gen, n)) return rc;
            if (n == 0) return JJS_OK;
            go = true;
            return svg_pointers(H, false);
        },
        [&] {
            const size_t ng = H.n_gen, w = svg_gen_width(H.format), sn = H.sign ? n : 0;
            return std::vector<stage_part>{{ng * w, H.Gen, nullptr}, {sn * 32, H.m, nullptr}, {n * 32, H.sk, nullptr}, {sn * 32, H.rnd, nullptr},
                                           {sn * 32, nullptr, H.u_out}, {sn * 64, nullptr, H.R_out}, {H.PK_out ? n * 64 : 0, nullptr, H.PK_out},
                                           {H.Gen_out ? ng * 64 : 0, nullptr, H.Gen_out}, {n, nullptr, H.status}};
        },
        [&](uint8_t* const* p, hipStream_t st) {
            svg_call A = H;
            A.Gen = p[0]; A.m = H.sign ? p[1] : nullptr; A.sk = p[2]; A.rnd = H.sign ? p[3] : nullptr;
            A.u_out = H.sign ? p[4] : nullptr; A.R_out = H.sign ? p[5] : nullptr;
            A.PK_out = H.PK_out ? p[6] : nullptr; A.Gen_out = H.Gen_out ? p[7] : nullptr; A.status = p[8];
            return svg_locked(A, n, st);
        },
        stage_secrets{2, 2});
}
}  // extern "C++"

extern "C" {

int jjs_public_keys_vargen_dev(int format, const void* sk, const void* Gen, size_t n_gen, size_t n, void* PK_out, void* Gen_out, void* status,
                               void* stream) {
    svg_call A{};
    A.format = format; A.sign = false; A.sk = sk; A.Gen = Gen; A.n_gen = n_gen; A.PK_out = PK_out; A.Gen_out = Gen_out; A.status = status;
    return svg_dev(A, n, stream);
}
int jjs_sign_vargen_pt_dev(int format, const void* sk, const void* Gen, size_t n_gen, const void* rnd, const void* m, size_t n, void* u_out,
                           void* R_out, void* PK_out, void* Gen_out, void* status, void* stream) {
    svg_call A{};
    A.format = format; A.sign = true; A.sk = sk; A.Gen = Gen; A.n_gen = n_gen; A.rnd = rnd; A.m = m;
    A.u_out = u_out; A.R_out = R_out; A.PK_out = PK_out; A.Gen_out = Gen_out; A.status = status;
    return svg_dev(A, n, stream);
}
int jjs_public_keys_vargen(int format, const uint8_t* sk, const uint8_t* Gen, size_t n_gen, size_t n, uint8_t* PK_out, uint8_t* Gen_out,
                           uint8_t* status) {
    svg_call A{};
    A.format = format; A.sign = false; A.sk = sk; A.Gen = Gen; A.n_gen = n_gen; A.PK_out = PK_out; A.Gen_out = Gen_out; A.status = status;
    return svg_host(A, n);
}
int jjs_sign_vargen_pt(int format, const uint8_t* sk, const uint8_t* Gen, size_t n_gen, const uint8_t* rnd, const uint8_t* m, size_t n,
                       uint8_t* u_out, uint8_t* R_out, uint8_t* PK_out, uint8_t* Gen_out, uint8_t* status) {
    svg_call A{};
    A.format = format; A.sign = true; A.sk = sk; A.Gen = Gen; A.n_gen = n_gen; A.rnd = rnd; A.m = m;
    A.u_out = u_out; A.R_out = R_out; A.PK_out = PK_out; A.Gen_out = Gen_out; A.status = status;
    return svg_host(A, n);
}
// [0] the lanes of the signing kernels that are resident at once on the current device (their grid limit times the block size: a
// call of more items takes a second trip through the grid-stride loop); [1] the smallest n the shared-generator route serves --
// UINT64_MAX: no call takes it by size, a shared generator is read by the per-item route with stride 0 at every n.
int jjs_debug_sign_limits(uint64_t out[2]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[0] = (uint64_t)g->grid_sign * BLOCK;
    out[1] = SIGN_SHARED_MIN_ITEMS == SIZE_MAX ? UINT64_MAX : (uint64_t)SIGN_SHARED_MIN_ITEMS;
    return JJS_OK;
}

}  // extern "C"
