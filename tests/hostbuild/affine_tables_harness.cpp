// The key-table stages of tools/scalar_stages.h (kt_chain_key, kt_build_table, kt_add_scalar, kt_add_challenge) on the CPU as
// a stand-alone program: the records of a file in, their outputs to a file out, one item after the other.  A program of its
// own and not a library for python, so that it can be built with the host sanitizers (tests/test_affine_tables_host.py does,
// with JJS_HOST_SANITIZE=1).  It only executes; the test writes the inputs and checks every output against the Python oracle.
//
//   affine_tables_harness IN OUT
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../jubjub_schnorr_amd/tools/scalar_stages.h"

using namespace jjs;

struct host_records {
    const uint32_t* in;
    size_t in_words, pos = 0;
    int records = 0;
    std::vector<uint32_t> out;
    sc::ctx C;
    template <typename S>
    int step(uint32_t n) {
        static_assert(S::IN % 4 == 0, "16-byte loads");
        if (S::LANES != 1 || !sc::record_fits<S>(in_words, pos, n)) return 1;
        std::vector<uint32_t> item(S::IN + 4), scratch(S::SCRATCH + 4), res((size_t)S::OUT + 4);
        uint32_t* it = (uint32_t*)(((uintptr_t)item.data() + 15) & ~(uintptr_t)15);
        uint32_t* sp = (uint32_t*)(((uintptr_t)scratch.data() + 15) & ~(uintptr_t)15);
        uint32_t* rp = (uint32_t*)(((uintptr_t)res.data() + 15) & ~(uintptr_t)15);
        for (uint32_t i = 0; i < n; ++i) {
            memcpy(it, in + pos + (size_t)S::IN * i, 4 * S::IN);
            memset(rp, 0xff, 4 * (size_t)S::OUT);
            S::run(C, it, rp, sp, 0);
            out.insert(out.end(), rp, rp + S::OUT);
        }
        pos += (size_t)S::IN * n;
        return 0;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: affine_tables_harness IN OUT\n");
        return 1;
    }
    std::vector<uint32_t> in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    // the key-table stages only: a record of another kind would need the comb tables, which this program does not build
    for (size_t p = 0; p + 2 <= in.size();) {
        const uint32_t kind = in[p] >> 24, n = in[p + 1];
        if (kind != sc::K_KT && kind != sc::K_KT_DUMP && kind != sc::K_KT_CHALLENGE) { fprintf(stderr, "not a key-table record\n"); return 3; }
        p += 2 + (size_t)24 * n;
    }
    host_records x{in.data(), in.size()};
    x.C = sc::ctx{{nullptr, nullptr}};
    const int rc = sc::run_records(x);
    if (rc) { fprintf(stderr, "record %d failed with %d\n", x.records, rc); return rc; }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(x.out.data(), 4, x.out.size(), g) != x.out.size() || fclose(g) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    return 0;
}
