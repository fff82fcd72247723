// jjs::multisig::SignerGroup (include/jjs_schnorr.hpp) the way a committee's client uses it: the key vector registered once,
// then a call on device buffers.  Input: a text file of hex lines -- "pk" (n x 64 bytes), "z", "R", "S" (B n rows), "m" (B x 32),
// then the expected "agg" (64), "u" (B x 32), "rsa" (B x 64).  With --compile-only semantics the program is only built (no GPU).
// Exit code 0 = all expectations met.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

#include <hip/hip_runtime.h>

#include "jjs_schnorr.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
#define HIP_OK(x) do { if ((x) != hipSuccess) { std::printf("FAIL %s\n", #x); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { std::puts("usage: test_msig_group transcript.txt"); return 2; }
    std::map<std::string, std::vector<uint8_t>> f;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key, hex;
        ls >> key >> hex;
        f[key] = unhex(hex);
    }
    jjs::Engine engine;
    const size_t n = f["pk"].size() / 64, B = f["m"].size() / 32;
    std::vector<jjs::AffinePoint> keys(n);
    for (size_t i = 0; i < n; ++i) std::memcpy(keys[i].data(), f["pk"].data() + 64 * i, 64);
    jjs::multisig::SignerGroup made(keys);
    jjs::multisig::SignerGroup group(std::move(made));           // move-only: the handle travels, the source is empty
    int failures = 0;
    if (made.handle() != 0 || group.participants() != n || group.info()[JJS_MSIG_GROUP_PARTICIPANTS] != n) { std::puts("FAIL move / info"); ++failures; }
    if (std::memcmp(group.aggregate_pk().data(), f["agg"].data(), 64) != 0) { std::puts("FAIL aggregate_pk"); ++failures; }
    uint8_t *z, *R, *S, *m, *st, *ts, *su, *sr;
    HIP_OK(hipMalloc(&z, B * n * 32)); HIP_OK(hipMalloc(&R, B * n * 64)); HIP_OK(hipMalloc(&S, B * n * 64)); HIP_OK(hipMalloc(&m, B * 32));
    HIP_OK(hipMalloc(&st, B * n)); HIP_OK(hipMalloc(&ts, B)); HIP_OK(hipMalloc(&su, B * 32)); HIP_OK(hipMalloc(&sr, B * 64));
    HIP_OK(hipMemcpy(z, f["z"].data(), B * n * 32, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(R, f["R"].data(), B * n * 64, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(S, f["S"].data(), B * n * 64, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(m, f["m"].data(), B * 32, hipMemcpyHostToDevice));
    group.combine_dev(z, R, S, m, B, st, ts, su, sr);
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint8_t> hst(B * n), hts(B), hsu(B * 32), hsr(B * 64);
    HIP_OK(hipMemcpy(hst.data(), st, B * n, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hts.data(), ts, B, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hsu.data(), su, B * 32, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hsr.data(), sr, B * 64, hipMemcpyDeviceToHost));
    for (uint8_t x : hst) if (x) { std::puts("FAIL share status"); ++failures; break; }
    for (uint8_t x : hts) if (x) { std::puts("FAIL transcript status"); ++failures; break; }
    if (hsu != f["u"]) { std::puts("FAIL sig_u"); ++failures; }
    if (hsr != f["rsa"]) { std::puts("FAIL sig_R"); ++failures; }
    if (group.info()[JJS_MSIG_GROUP_CALLS] != 1) { std::puts("FAIL calls served"); ++failures; }
    std::printf("%zu participants, %zu transcripts, %d failures\n", n, B, failures);
    return failures ? 1 : 0;
}
