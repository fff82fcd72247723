// The scalar multiplications on the device with caller-chosen scalars and points: the stages of tools/scalar_stages.h (the same
// bodies the CPU build of tests/hostbuild runs) -- comb_mul, build_point_table + table_mul, check_equation with a fixed and a
// per-item generator, the key tables for both window widths, the latency path at 4, 8 and 16 positions -- plus what only the
// device has: kt_chain_key_quad and sb_chain_lane_quad on four lanes.  The comb tables are built here with build_comb_entry,
// one entry per lane, as the library builds them.  This program only executes: tests/test_scalar_mul_gpu.py writes the
// inputs, runs it once under its own time limit and checks every output against the Python oracle.
//
//   scalarcheck IN OUT          (record format: tools/scalar_stages.h)
// One launch per record.  An unknown code, a short file or a HIP error ends the run with a non-zero status.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "scalar_stages.h"

using namespace jjs;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__global__ void __launch_bounds__(256) k_comb(uint32_t* table, int which) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < COMB_WINDOWS * COMB_ENTRIES) build_comb_entry(table, which ? JJS_GN : JJS_G, t / COMB_ENTRIES, t % COMB_ENTRIES);
}

template <typename S>
__global__ void __launch_bounds__(64) k_run(sc::ctx C, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                            uint32_t* __restrict__ scratch, uint32_t n) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x, item = t / S::LANES, j = t % S::LANES;
    if (item < n) S::run(C, in + (size_t)S::IN * item, out + (size_t)S::OUT * item, scratch + (size_t)S::SCRATCH * item, j);   // whole groups leave together
}

struct device_records {
    const uint32_t* in;
    size_t in_words, pos = 0;
    int records = 0;
    std::vector<uint32_t> out;
    sc::ctx C;
    template <typename S>
    int step(uint32_t n) {
        static_assert(S::IN % 4 == 0 && S::OUT % 2 == 0 && S::SCRATCH % 4 == 0 && 64 % S::LANES == 0, "aligned items, whole groups in a wave");
        if (!sc::record_fits<S>(in_words, pos, n)) {
            fprintf(stderr, "record of %u items does not fit\n", n);
            return 1;
        }
        const size_t iw = (size_t)S::IN * n, ow = (size_t)S::OUT * n, sw = (size_t)S::SCRATCH * n + 4;
        uint32_t *din = nullptr, *dout = nullptr, *dscr = nullptr;
        CHECK(hipMalloc(&din, iw * 4));
        CHECK(hipMalloc(&dout, ow * 4));
        CHECK(hipMalloc(&dscr, sw * 4));
        CHECK(hipMemcpy(din, in + pos, iw * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dout, 0xff, ow * 4));
        const uint32_t threads = n * S::LANES;
        hipLaunchKernelGGL(k_run<S>, dim3((threads + 63) / 64), dim3(64), 0, 0, C, din, dout, dscr, n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        const size_t at = out.size();
        out.resize(at + ow);
        CHECK(hipMemcpy(out.data() + at, dout, ow * 4, hipMemcpyDeviceToHost));
        CHECK(hipFree(din));
        CHECK(hipFree(dout));
        CHECK(hipFree(dscr));
        printf("scalarcheck: record %08x, %u items\n", in[pos - 2], n);
        pos += iw;
        return 0;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: scalarcheck IN OUT\n");
        return 1;
    }
    std::vector<uint32_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        uint32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
        fclose(f);
    }
    uint32_t* comb[2] = {nullptr, nullptr};
    for (int which = 0; which < 2; ++which) {
        CHECK(hipMalloc(&comb[which], COMB_TABLE_WORDS * 4));
        hipLaunchKernelGGL(k_comb, dim3((COMB_WINDOWS * COMB_ENTRIES + 255) / 256), dim3(256), 0, 0, comb[which], which);
        CHECK(hipGetLastError());
    }
    CHECK(hipDeviceSynchronize());
    device_records x{in.data(), in.size()};
    x.C = sc::ctx{{comb[0], comb[1]}};
    const int rc = sc::run_records(x);
    if (rc) {
        fprintf(stderr, "record %d failed with %d (3: unknown stage code)\n", x.records, rc);
        return rc;
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(x.out.data(), 4, x.out.size(), g) != x.out.size() || fclose(g) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    printf("scalarcheck: %d records, %zu output words\n", x.records, x.out.size());
    return 0;
}
