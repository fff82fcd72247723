// Part of jjs_gpu.hip (included among the extern "C" entry points): multisig signer groups (msig_group.h, include/jjs_gpu.h
// jjs_msig_group_*) -- building a group on every driven device, the registry, and the call against a group.

// A call has at least this many transcripts when its share pass runs a wave over the transcripts of ONE participant
// (msig_group_params::by_participant): below, a wave would span several participants anyway.
constexpr size_t MSIG_GROUP_BY_PARTICIPANT_FROM = 64;

// One device's copy of a group (g is that device), on stream s: d_j and D_j = d_j * PK_j by the inline call's own pass 1 over a
// one-transcript descriptor, their sum, and the chains and window tables of the keys.  `tags`: the two SAFE tags, from the host.
// ext: PK holds n x 96 extended keys (every one usable: the caller has looked), normalised here in front of everything else.
static int msig_group_build_copy(msig_group_entry& k, msig_group_copy& c, const uint8_t* PK, bool ext, const uint32_t (*tags)[9], uint8_t* agg_out,
                                 hipStream_t s) {
    const uint32_t n = k.participants;
    const size_t d_bytes = pad256((size_t)n * 32), table_bytes = (size_t)n * MG_TABLE_WORDS_PER_KEY * 4;
    // the build area: the keys, pass 1's participant map, offsets and D_j, the chains of bases, the lanes' workspaces
    const uint32_t hash_lanes = msig_hash_lanes(n);
    const int delin_grid = grid_for(g->grid_msig, (size_t)n * hash_lanes);
    const size_t pk_bytes = pad256((size_t)n * 64), map_bytes = pad256((size_t)n * 4), dpk_bytes = pad256((size_t)n * EXT_WORDS * 4);
    const size_t base_bytes = pad256((size_t)n * MG_BASE_WORDS_PER_KEY * 4), ws_bytes = (size_t)delin_grid * BLOCK * WS_WORDS_PER_LANE * 4;
    const size_t ext_bytes = ext ? pad256((size_t)n * 96) : 0, prefix_bytes = ext ? pad256((size_t)n * 36) : 0;
    const size_t tmp_bytes = pk_bytes + map_bytes + 256 + dpk_bytes + base_bytes + ext_bytes + prefix_bytes + ws_bytes;
    const uint32_t offsets[2] = {0, n};          // host memory the queued copies read: the frame drains the stream before it goes
    return build_device_copy(c, 256 + d_bytes + pad256(table_bytes), tmp_bytes, "signer group", s, [&](uint8_t* tmp) -> int {
        c.agg_pk = c.mem;
        c.tag_a = reinterpret_cast<uint32_t*>(c.mem + 64);
        c.d_words = reinterpret_cast<uint32_t*>(c.mem + 256);
        c.tables = reinterpret_cast<uint32_t*>(c.mem + 256 + d_bytes);
        uint8_t* q = tmp;
        uint8_t* pk = q; q += pk_bytes;
        uint32_t* tr_of = reinterpret_cast<uint32_t*>(q); q += map_bytes;
        uint32_t* d_off = reinterpret_cast<uint32_t*>(q); q += 256;
        uint32_t* dpk = reinterpret_cast<uint32_t*>(q); q += dpk_bytes;
        uint32_t* bases = reinterpret_cast<uint32_t*>(q); q += base_bytes;
        uint8_t* pk_ext = q; q += ext_bytes;
        uint32_t* prefix = reinterpret_cast<uint32_t*>(q); q += prefix_bytes;
        uint32_t* ws = reinterpret_cast<uint32_t*>(q);
        if (ext) {
            HIP_TRY(hipMemcpyAsync(pk_ext, PK, (size_t)n * 96, hipMemcpyHostToDevice, s));
            normalize_params N{};
            N.n_src = 1; N.poison = 1; N.scratch = prefix;
            N.src[0] = fe_src{pk_ext, 96, 0}; N.out[0] = pk;
            if (int rc = launch_normalize(N, 0, n, n, s)) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(pk, PK, (size_t)n * 64, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemcpyAsync(c.tag_a, tags, 2 * 9 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(offsets), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(tr_of, 0, (size_t)n * 4, s));
        msig_params P{};
        P.PK = pk; P.offsets = d_off; P.n_transcripts = 1; P.n_total = n;
        P.tr_of = tr_of; P.d_words = c.d_words; P.dpk = dpk;
        P.long_tags = c.tag_a; P.max_table_participants = 0;          // both tags come from the group's own rows
        P.hash_lanes = hash_lanes; P.lane_ws = ws;
        hipLaunchKernelGGL(msig_kernel, dim3(delin_grid), dim3(BLOCK), 0, s, P, 1);
        hipLaunchKernelGGL(msig_group_agg_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)dpk, n, c.agg_pk);
        hipLaunchKernelGGL(msig_group_chain_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, (const uint8_t*)pk, n, bases);
        hipLaunchKernelGGL(msig_group_table_kernel, dim3((unsigned)(((uint64_t)n * kt_positions(MG_WINDOW) + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                           (const uint32_t*)bases, c.tables, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(agg_out, c.agg_pk, 64, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return JJS_OK;
    });
}

// jjs_msig_group_create / _ext / _wire: PK is n x 64 affine, n x 96 extended, or n x 32 compressed.  Wire keys are decoded here, on
// the host (mg_wire_keys_decode: the refusal of an undecodable key comes before anything is built), and registered as the affine
// keys they decode to.
static int msig_group_create(const uint8_t* PK, int fmt, size_t n, jjs_msig_group* out) {
    const bool ext = fmt == JJS_FORMAT_EXT, wire = fmt == JJS_FORMAT_WIRE;
    registration<msig_group_entry> call;
    if (int rc = call.enter([&] {
            if (!out || !PK || n == 0) return fail(JJS_ERR_ARG, "a signer group needs at least one key and an output handle");
            if (n > JJS_MSIG_PARTICIPANTS_LIMIT) return fail(JJS_ERR_ARG, "%zu participants (at most %u)", n, (unsigned)JJS_MSIG_PARTICIPANTS_LIMIT);
            return (int)JJS_OK;
        }))
        return rc;
    msig_group_entry& k = *call.e;
    const size_t width = ext ? 96 : (wire ? 32 : 64);
    std::vector<u32x4> keys, decoded;       // the caller's bytes, aligned for the range test; the affine keys of a wire vector
    bool wire_ok = true;
    if (int rc = no_throw([&]() -> int {
            keys.resize(n * width / 16);
            memcpy(keys.data(), PK, n * width);
            if (wire) {
                decoded.resize(n * 4);
                wire_ok = mg_wire_keys_decode(reinterpret_cast<const uint8_t*>(keys.data()), n, host_dlog_tables(),
                                              reinterpret_cast<uint8_t*>(decoded.data()));
            }
            return JJS_OK;
        }))
        return rc;
    const uint8_t* pk = reinterpret_cast<const uint8_t*>(wire ? decoded.data() : keys.data());
    if (!wire_ok) return fail(JJS_ERR_ARG, "the encoding of a key does not decode");
    if (ext ? !mg_ext_keys_usable(pk, n) : !mg_keys_acceptable(pk, n))
        return fail(JJS_ERR_ARG, ext ? "a key is unusable: a coordinate is not below q, or Z is zero" : "a coordinate of a key is not below q");
    k.participants = (uint32_t)n;
    uint32_t tags[2][9];
    for (int which = 0; which < 2; ++which) {
        const uint32_t n_in = which ? 3u + 4u * (uint32_t)n : 2u + 2u * (uint32_t)n;
        if (n <= JJS_MSIG_MAX_PARTICIPANTS) memcpy(tags[which], JJS_SPONGE_TAG_LONG[n_in], sizeof(tags[which]));
        else safe_tag_limbs(n_in, JJS_Q_WORDS, tags[which]);
    }
    if (int rc = call.build([&](msig_group_copy& c, hipStream_t s) { return msig_group_build_copy(k, c, pk, ext, tags, k.agg_pk, s); })) return rc;
    return call.publish(g_msig_groups, "signer group", out);
}

extern "C" {

int jjs_msig_group_create(const uint8_t* PK, size_t n, jjs_msig_group* out) { return msig_group_create(PK, JJS_FORMAT_AFFINE, n, out); }
int jjs_msig_group_create_ext(const uint8_t* PK_ext, size_t n, jjs_msig_group* out) { return msig_group_create(PK_ext, JJS_FORMAT_EXT, n, out); }
int jjs_msig_group_create_wire(const uint8_t* PK_w, size_t n, jjs_msig_group* out) { return msig_group_create(PK_w, JJS_FORMAT_WIRE, n, out); }

int jjs_msig_group_destroy(jjs_msig_group h) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    if (!g_msig_groups.destroy(h)) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    return JJS_OK;
}

int jjs_msig_group_info(jjs_msig_group h, uint64_t out[JJS_MSIG_GROUP_INFO]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    msig_group_entry* k = g_msig_groups.find(h);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    out[JJS_MSIG_GROUP_PARTICIPANTS] = k->participants;
    out[JJS_MSIG_GROUP_WINDOW_BITS] = (uint64_t)MG_WINDOW;
    out[JJS_MSIG_GROUP_DEVICE_BYTES] = k->copies.empty() ? 0 : k->copies[0].mem.bytes();
    out[JJS_MSIG_GROUP_CALLS] = k->calls;
    return JJS_OK;
}

int jjs_msig_group_aggregate_pk(jjs_msig_group h, uint8_t out[64]) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    msig_group_entry* k = g_msig_groups.find(h);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    if (!out) return fail(JJS_ERR_ARG, "null pointer");
    memcpy(out, k->agg_pk, 64);
    return JJS_OK;
}

// n = the shares of n_transcripts transcripts of group k: fewer than 2^32, they are indexed with 32 bits
static int msig_group_rows(const msig_group_entry& k, size_t n_transcripts, size_t& n) {
    const uint64_t per = k.participants;
    if (n_transcripts >= (1ull << 32) / per + ((1ull << 32) % per ? 1u : 0u))
        return fail(JJS_ERR_ARG, "%zu transcripts of %llu participants: the shares are indexed with 32 bits", n_transcripts, (unsigned long long)per);
    n = n_transcripts * per;
    return JJS_OK;
}

// The call against group h on device columns, queued on s (under the engine's mutex, g the device).  fmt (JJS_FORMAT_*): R, S are
// B n x 64, B n x 96 or B n x 32.
static int msig_group_combine_locked(jjs_msig_group h, int fmt, const void* z, const void* R, const void* S, const void* m, size_t n_transcripts,
                                     void* share_status, void* transcript_status, void* sig_u, void* sig_R, hipStream_t s) {
    msig_group_entry* k = g_msig_groups.find(h);
    if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
    if (n_transcripts == 0) return JJS_OK;
    size_t n = 0;
    if (int rc = msig_group_rows(*k, n_transcripts, n)) return rc;
    if (!all_ok(z, R, S, m, sig_u, sig_R) || !share_status) return fail(JJS_ERR_ARG, "null or misaligned pointer");
    const msig_group_copy* c = copy_for(*k, g);
    if (!c) return fail(JJS_ERR_ARG, "the signer group has no copy on this device");
    msig_caps need;
    need.rows = n; need.transcripts = n_transcripts;
    if (fmt != JJS_FORMAT_AFFINE) need.ext_rows = n;
    ++k->calls;
    return msig_scratch_call(need, s, [&](const msig_scratch& W) -> int {
        const uint8_t* pts[2] = {(const uint8_t*)R, (const uint8_t*)S};
        msig_group_params G{};
        msig_params& P = G.M;
        P.z = (const uint8_t*)z; P.m = (const uint8_t*)m;
        P.n_transcripts = (uint32_t)n_transcripts; P.n_total = n;
        P.share_status = (uint8_t*)share_status; P.sig_u = (uint8_t*)sig_u; P.sig_R = (uint8_t*)sig_R;
        P.transcript_status = (uint8_t*)transcript_status;
        P.agg_pk = c->agg_pk;                                            // read only: the group's
        P.e_pt = W.e_pt; P.a_words = W.a_words; P.c_words = W.c_words;
        P.comb_g = g->comb_g; P.lane_ws = g->slots[0].workspace;
        msig_group_fill(G, *k, *c);
        G.by_participant = n_transcripts >= MSIG_GROUP_BY_PARTICIPANT_FROM ? 1u : 0u;
#if defined(JJS_PROFILING)
        if (g_keep_order) G.by_participant = 0;                          // A/B of the lane mapping (jjs_debug_force_path 0x1000)
#endif
        if (int rc = msig_ingest(fmt, W, pts, 2, n, s)) return rc;
        P.R = pts[0]; P.S = pts[1];
        // msig_group_kernel's own schedule: pass 1 runs one lane per share, the others one per transcript; 0 and 2 have the hash chains
        for (int pass = 0; pass < 5; ++pass) {
            if (pass == 3) {
                hipLaunchKernelGGL(msig_group_share_kernel, dim3(grid_for(g->grid_msig, n)), dim3(BLOCK), 0, s, G);
                continue;
            }
            const size_t count = pass == 1 ? n : n_transcripts;
            P.hash_lanes = (pass == 0 || pass == 2) ? msig_hash_lanes(count) : 1u;
            hipLaunchKernelGGL(msig_group_kernel, dim3(grid_for(g->grid_msig, count * P.hash_lanes)), dim3(BLOCK), 0, s, G, pass);
        }
        HIP_TRY(hipGetLastError());
        return JJS_OK;
    });
}

// the three formats of jjs_msig_group_combine*_dev
static int msig_group_combine_dev(jjs_msig_group h, int fmt, const void* z, const void* R, const void* S, const void* m, size_t n_transcripts,
                                  void* share_status, void* transcript_status, void* sig_u, void* sig_R, void* stream) {
    std::lock_guard<std::mutex> lock(L.mu);
    if (int rc = check_ready()) return rc;
    return msig_group_combine_locked(h, fmt, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, (hipStream_t)stream);
}
int jjs_msig_group_combine_dev(jjs_msig_group h, const void* z, const void* R, const void* S, const void* m, size_t n_transcripts,
                               void* share_status, void* transcript_status, void* sig_u, void* sig_R, void* stream) {
    return msig_group_combine_dev(h, JJS_FORMAT_AFFINE, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
}
int jjs_msig_group_combine_ext_dev(jjs_msig_group h, const void* z, const void* R_ext, const void* S_ext, const void* m, size_t n_transcripts,
                                   void* share_status, void* transcript_status, void* sig_u, void* sig_R, void* stream) {
    return msig_group_combine_dev(h, JJS_FORMAT_EXT, z, R_ext, S_ext, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
}
int jjs_msig_group_combine_wire_dev(jjs_msig_group h, const void* z, const void* R_w, const void* S_w, const void* m, size_t n_transcripts,
                                    void* share_status, void* transcript_status, void* sig_u, void* sig_R, void* stream) {
    return msig_group_combine_dev(h, JJS_FORMAT_WIRE, z, R_w, S_w, m, n_transcripts, share_status, transcript_status, sig_u, sig_R, stream);
}

}  // extern "C"
