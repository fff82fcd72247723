// CPU build of the wire ingest of the multisignature calls for tests/test_msig_wire_host.py: msig_decode_lane (csrc/decode.h),
// the lane body of msig_decode_kernel, as the *_wire entry points queue that kernel in front of pass 0 -- `lanes` is the launch
// shape: a lane owns the points lane, lane + lanes, ... of the n * k points of the call -- and mg_wire_keys_decode
// (csrc/msig_group.h), what jjs_msig_group_create_wire runs on a group's keys.  The square-root tables come from
// host_harness.cpp; the passes behind the decode are those of the other harnesses, which the tests run on the decoded columns.
#include "host_harness.cpp"
#include "msig_group.h"

extern "C" {

// k <= 3 sources of n compressed points, source i at src[i] + row * stride[i] + off[i], into k columns of n x 64.  Every
// address a lane loads from or stores to is 16-byte aligned.
int jjs_msig_wire_host_decode(const uint8_t* const* src, const uint32_t* stride, const uint32_t* off, int k, size_t n, size_t lanes,
                              uint8_t* const* out) {
    if (k < 1 || k > 3 || lanes == 0) return -1;
    msig_decode_params P{};
    P.n_src = (uint32_t)k; P.n = n; P.dlog = host_dlog();
    for (int i = 0; i < k; ++i) { P.src[i] = fe_src{src[i], stride[i], off[i]}; P.out[i] = out[i]; }
    for (size_t lane = 0; lane < lanes; ++lane) msig_decode_lane(P, lane, lanes);
    return 0;
}
// n x 32 keys -> n x 64 affine; -1 when one does not decode (or there is none), as jjs_msig_group_create_wire
int jjs_msig_wire_host_keys(const uint8_t* PK_w, size_t n, uint8_t* out) { return mg_wire_keys_decode(PK_w, n, host_dlog(), out) ? 0 : -1; }

}  // extern "C"
