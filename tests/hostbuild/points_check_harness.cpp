// CPU build of csrc/points_check.h (`is_valid` alone) for tests/test_points_check_host.py: the JJS_HD functions of the device's
// lanes -- pc_point_lane, pc_item_status, pc_finish_lane -- over the columns of jjs_keys_check / jjs_signatures_check, the
// lanes of an item one after the other on this thread; extended points whose affine form is wanted go through normalize.h first,
// as the device's call does.
#include "host_harness.cpp"
#include "points_check.h"

namespace {

template <uint32_t MODE>
void run_lanes(const points_check_params& C) {
    for (uint64_t item = 0; item < C.n; ++item) {
        uint32_t st = 0;
        for (uint32_t k = 0; k < C.n_pts; ++k) st = pc_item_status(st, pc_point_lane<MODE>(C, item, k, true));
        for (uint32_t k = 0; k < C.n_pts; ++k) pc_finish_lane(C, item, k, st);
        if (C.status) C.status[item] = (uint8_t)st;
        if (C.tally) C.tally[st]++;
    }
}

int run_call(const points_check_call& Q, size_t n, uint8_t* status, uint64_t* tally) {
    unsigned long long t[4] = {};
    points_check_params C = pc_params(Q, n, status, t, host_dlog());
    std::vector<uint32_t> scratch(9 * n + 16);
    std::vector<uint8_t> bad(n + 16, 0), spare[2];
    if (pc_normalises(Q)) {
        normalize_params N{};
        N.n_src = Q.n_pts; N.bad = bad.data(); N.scratch = scratch.data(); N.n = n; N.first = 0;
        for (uint32_t k = 0; k < Q.n_pts; ++k) {
            spare[k].assign(64 * n + 80, 0);
            N.src[k] = Q.src[k];
            N.out[k] = C.out[k] ? C.out[k] : (uint8_t*)(((uintptr_t)spare[k].data() + 15) & ~(uintptr_t)15);
        }
        if (n) normalize_lane(N, 0, 1);
        pc_over_normalised(C, N);
        run_lanes<PC_AFFINE>(C);
    } else if (Q.format == PC_AFFINE) run_lanes<PC_AFFINE>(C);
    else if (Q.format == PC_EXT) run_lanes<PC_EXT>(C);
    else if (Q.format == PC_WIRE) run_lanes<PC_WIRE>(C);
    else return -1;
    if (tally) for (int k = 0; k < 4; ++k) tally[k] = t[k];
    return 0;
}

}  // namespace

extern "C" {

// the arguments of jjs_keys_check; every buffer 16-byte aligned
int jjs_pc_host_keys_check(int scheme, int format, const uint8_t* K0, const uint8_t* K1, size_t n, uint8_t* status, uint64_t* tally,
                           uint8_t* A0_out, uint8_t* A1_out) {
    if (scheme < 0 || scheme > 2) return -1;
    return run_call(pc_keys_call(scheme == 0 ? 1u : 2u, (uint32_t)format, K0, K1, A0_out, A1_out), n, status, tally);
}
// the arguments of jjs_signatures_check
int jjs_pc_host_signatures_check(int scheme, int format, const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, size_t n, uint8_t* status,
                                 uint64_t* tally, uint8_t* u_out, uint8_t* R_out, uint8_t* Rp_out) {
    if (scheme < 0 || scheme > 2) return -1;
    return run_call(pc_signatures_call(scheme == 1 ? 2u : 1u, (uint32_t)format, s0, s1, s2, u_out, R_out, Rp_out), n, status, tally);
}
// one point by each per-point function, for the cases the test restates with Python integers
uint32_t jjs_pc_host_affine_point(const uint8_t* p) {
    words8 u, v;
    memcpy(u.w, p, 32); memcpy(v.w, p + 32, 32);
    return pc_affine_point(u, v);
}
uint32_t jjs_pc_host_ext_point(const uint8_t* p) {
    words8 u, v, z;
    memcpy(u.w, p, 32); memcpy(v.w, p + 32, 32); memcpy(z.w, p + 64, 32);
    return pc_ext_point(u, v, z);
}
uint32_t jjs_pc_host_wire_point(const uint8_t* p, uint8_t* out) {
    words8 e;
    memcpy(e.w, p, 32);
    const decoded_point d = decompress_point(e, host_dlog());
    memcpy(out, d.u.w, 32); memcpy(out + 32, d.v.w, 32);
    return pc_wire_point(d);
}

}  // extern "C"
