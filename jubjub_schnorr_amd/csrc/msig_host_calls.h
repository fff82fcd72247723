// Part of jjs_gpu.hip (included among the extern "C" entry points, behind staged_host_call.h): the blocking host-buffer forms of
// the multisignature calls, jjs_multisig_combine and jjs_msig_group_combine, on the frame of staged_host_call.h.
extern "C++" {
// The format of a call, out of those it allows (bit JJS_FORMAT_* of `allowed`).  A *_wire entry point, which has no format argument
// to refuse, allows and passes JJS_FORMAT_WIRE alone.
constexpr unsigned MSIG_FORMATS_POINTS = 1u << JJS_FORMAT_AFFINE | 1u << JJS_FORMAT_EXT, MSIG_FORMATS_WIRE = 1u << JJS_FORMAT_WIRE;
static int msig_format(int format, unsigned allowed, int& fmt) {
    if (format < JJS_FORMAT_AFFINE || format > JJS_FORMAT_WIRE || !(allowed >> format & 1u))
        return fail(JJS_ERR_ARG, allowed & MSIG_FORMATS_WIRE ? "verify_share takes affine, extended or wire points (format %d)"
                                                            : "the multisignature calls take affine or extended points (format %d)", format);
    fmt = format;
    return JJS_OK;
}
// bytes of a point in the columns of a call in format fmt (JJS_FORMAT_*)
static size_t msig_point_bytes(int fmt) { return fmt == JJS_FORMAT_EXT ? 96 : (fmt == JJS_FORMAT_WIRE ? 32 : 64); }

// parts: z, PK, R, S, m in; share_status, transcript_status, agg_pk, sig_u, sig_R out
static int msig_combine_host(int format, unsigned formats, const uint8_t* z, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                         const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                         uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    const size_t B = n_transcripts;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            if (int rc = msig_format(format, formats, fmt)) return rc;
            if (B == 0) return JJS_OK;
            if (int rc = msig_check_offsets(offsets, B, n)) return rc;
            if ((n && (!z || !PK || !R || !S || !share_status)) || !m || !agg_pk || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
            go = true;
            return JJS_OK;
        },
        [&] {
            const size_t w = msig_point_bytes(fmt);
            return std::vector<stage_part>{{n * 32, z, nullptr}, {n * w, PK, nullptr}, {n * w, R, nullptr}, {n * w, S, nullptr}, {B * 32, m, nullptr},
                                           {n, nullptr, share_status}, {B, nullptr, transcript_status}, {B * 64, nullptr, agg_pk},
                                           {B * 32, nullptr, sig_u}, {B * 64, nullptr, sig_R}};
        },
        [&](uint8_t* const* p, hipStream_t s) {
            return msig_combine_locked(fmt, p[0], p[1], p[2], p[3], p[4], offsets, B, p[5], transcript_status ? p[6] : nullptr, p[7], p[8], p[9], s);
        });
}

// parts: as the inline call's; a group call has no PK and no agg_pk, and their parts are empty
static int msig_group_combine_host(jjs_msig_group h, int format, unsigned formats, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                           size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    const size_t B = n_transcripts;
    int fmt = JJS_FORMAT_AFFINE;
    size_t n = 0;
    return staged_host_call(
        [&](bool& go) -> int {
            msig_group_entry* k = g_msig_groups.find(h);
            if (!k) return fail(JJS_ERR_ARG, "unknown or destroyed signer group");
            if (int rc = msig_format(format, formats, fmt)) return rc;
            if (B == 0) return JJS_OK;
            if (int rc = msig_group_rows(*k, B, n)) return rc;
            if (!z || !R || !S || !m || !share_status || !sig_u || !sig_R) return fail(JJS_ERR_ARG, "null pointer");
            go = true;
            return JJS_OK;
        },
        [&] {
            const size_t w = msig_point_bytes(fmt);
            return std::vector<stage_part>{{n * 32, z, nullptr}, {0, nullptr, nullptr}, {n * w, R, nullptr}, {n * w, S, nullptr}, {B * 32, m, nullptr},
                                           {n, nullptr, share_status}, {B, nullptr, transcript_status}, {0, nullptr, nullptr},
                                           {B * 32, nullptr, sig_u}, {B * 64, nullptr, sig_R}};
        },
        [&](uint8_t* const* p, hipStream_t s) -> int {
            // (the group is looked up again: it may have been destroyed, or registered with other participants, meanwhile)
            msig_group_entry* k = g_msig_groups.find(h);
            if (!k || (size_t)k->participants * B != n) return fail(JJS_ERR_ARG, "the signer group was destroyed during the call");
            return msig_group_combine_locked(h, fmt, p[0], p[2], p[3], p[4], B, p[5], transcript_status ? p[6] : nullptr, p[8], p[9], s);
        });
}

}  // extern "C++"

extern "C" {

int jjs_multisig_combine(int format, const uint8_t* z, const uint8_t* PK, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                         const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                         uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_combine_host(format, MSIG_FORMATS_POINTS, z, PK, R, S, m, offsets, n_transcripts, share_status, transcript_status, agg_pk, sig_u, sig_R);
}
int jjs_multisig_combine_wire(const uint8_t* z, const uint8_t* PK_w, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                              const uint32_t* offsets, size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status,
                              uint8_t* agg_pk, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_combine_host(JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, z, PK_w, R_w, S_w, m, offsets, n_transcripts, share_status, transcript_status, agg_pk, sig_u,
                             sig_R);
}
int jjs_msig_group_combine(jjs_msig_group h, int format, const uint8_t* z, const uint8_t* R, const uint8_t* S, const uint8_t* m,
                           size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_group_combine_host(h, format, MSIG_FORMATS_POINTS, z, R, S, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
}
int jjs_msig_group_combine_wire(jjs_msig_group h, const uint8_t* z, const uint8_t* R_w, const uint8_t* S_w, const uint8_t* m,
                                size_t n_transcripts, uint8_t* share_status, uint8_t* transcript_status, uint8_t* sig_u, uint8_t* sig_R) {
    return msig_group_combine_host(h, JJS_FORMAT_WIRE, MSIG_FORMATS_WIRE, z, R_w, S_w, m, n_transcripts, share_status, transcript_status, sig_u, sig_R);
}

}  // extern "C"
