// The arithmetic modulo the group order r, truncate250, the ChaCha20 block and the batch weights on the device with
// caller-chosen inputs: the stages of tools/fr_stages.h (the same bodies the CPU build of tests/hostbuild runs), one lane per
// item in whole waves.  This program only executes: tests/test_fr_gpu.py writes the inputs, runs it once under its own time
// limit and checks every output word with Python integers.
//
//   frcheck IN OUT          (record format: tools/fr_stages.h)
// One launch per record.  An unknown code, a short file or a HIP error ends the run with a non-zero status.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "fr_stages.h"

using namespace jjs;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

template <typename S>
__global__ void __launch_bounds__(64) k_run(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t item = blockIdx.x * 64u + threadIdx.x;
    if (item < n) S::run(in + (size_t)S::IN * item, out + (size_t)S::OUT * item);
}

struct device_records {
    const uint32_t* in;
    size_t in_words, pos = 0;
    int records = 0;
    std::vector<uint32_t> out;

    template <typename S>
    int step(uint32_t n) {
        if (!fr::record_fits<S>(in_words, pos, n)) {
            fprintf(stderr, "record of %u items does not fit\n", n);
            return 1;
        }
        const size_t iw = (size_t)S::IN * n, ow = (size_t)S::OUT * n;
        uint32_t *din = nullptr, *dout = nullptr;
        CHECK(hipMalloc(&din, iw * 4));
        CHECK(hipMalloc(&dout, ow * 4));
        CHECK(hipMemcpy(din, in + pos, iw * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dout, 0xff, ow * 4));
        hipLaunchKernelGGL(k_run<S>, dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        const size_t at = out.size();
        out.resize(at + ow);
        CHECK(hipMemcpy(out.data() + at, dout, ow * 4, hipMemcpyDeviceToHost));
        CHECK(hipFree(din));
        CHECK(hipFree(dout));
        printf("frcheck: record %08x, %u items\n", in[pos - 2], n);
        pos += iw;
        return 0;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: frcheck IN OUT\n");
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
    device_records x{in.data(), in.size()};
    const int rc = fr::run_records(x);
    if (rc) {
        fprintf(stderr, "record %d failed with %d (3: unknown stage code)\n", x.records, rc);
        return rc;
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(x.out.data(), 4, x.out.size(), g) != x.out.size() || fclose(g) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    printf("frcheck: %d records, %zu output words\n", x.records, x.out.size());
    return 0;
}
