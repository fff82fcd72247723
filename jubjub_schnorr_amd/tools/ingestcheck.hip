// Inversion, inverse square roots, point decoding and the normalisation of extended coordinates on the device with
// caller-chosen inputs: the stages of tools/ingest_stages.h (the same bodies the CPU build of tests/hostbuild runs).  The
// square-root tables are built here with dlog_table_entry, one entry per lane after a cleared hash, as the library builds
// them.  This program only executes: tests/test_ingest_gpu.py writes the inputs, runs it once under its own time limit and
// checks every output word with Python integers.
//
//   ingestcheck IN OUT          (record format: tools/ingest_stages.h)
// One launch per record.  An unknown code, a short file, a header that does not fit its buffers or a HIP error ends the run
// with a non-zero status.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "ingest_stages.h"

using namespace jjs;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__global__ void __launch_bounds__(256) k_tables(uint32_t* pow, uint8_t* hash) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 7 * 256) dlog_table_entry(pow, hash, t / 256, t % 256);
}

template <typename S>
__global__ void __launch_bounds__(64) k_run(ig::ctx C, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t item = blockIdx.x * 64u + threadIdx.x;
    if (item < n) S::run(C, in + (size_t)S::IN * item, out + (size_t)S::OUT * item);
}

__global__ void __launch_bounds__(64) k_normalize(normalize_params P, uint32_t lanes) {
    const uint32_t lane = blockIdx.x * 64u + threadIdx.x;
    if (lane < lanes) normalize_lane(P, lane, lanes);
}

struct device_records {
    const uint32_t* in;
    size_t in_words, pos = 0;
    int records = 0;
    std::vector<uint32_t> out;
    ig::ctx C;
    uint32_t* d_pow;
    uint8_t* d_hash;

    int collect(const uint32_t* dout, size_t ow) {
        const size_t at = out.size();
        out.resize(at + ow);
        CHECK(hipMemcpy(out.data() + at, dout, ow * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    template <typename S>
    int step(uint32_t n) {
        if (!ig::record_fits<S>(in_words, pos, n)) {
            fprintf(stderr, "record of %u items does not fit\n", n);
            return 1;
        }
        const size_t iw = (size_t)S::IN * n, ow = (size_t)S::OUT * n;
        uint32_t *din = nullptr, *dout = nullptr;
        CHECK(hipMalloc(&din, iw * 4));
        CHECK(hipMalloc(&dout, ow * 4));
        CHECK(hipMemcpy(din, in + pos, iw * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dout, 0xff, ow * 4));
        hipLaunchKernelGGL(k_run<S>, dim3((n + 63) / 64), dim3(64), 0, 0, C, din, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        if (int rc = collect(dout, ow)) return rc;
        CHECK(hipFree(din));
        CHECK(hipFree(dout));
        printf("ingestcheck: record %08x, %u items\n", in[pos - 2], n);
        pos += iw;
        return 0;
    }
    int normalize(uint32_t n_src, uint32_t rows) {
        ig::norm_header H;
        if (!ig::norm_fits(in_words, pos, n_src, rows, in, H)) {
            fprintf(stderr, "normalisation record of %u rows does not fit\n", rows);
            return 1;
        }
        const size_t iw = ig::norm_in_words(n_src, rows), ew = iw - ig::NORM_HEADER, ow = ig::norm_out_words(n_src, rows);
        std::vector<uint32_t> fill(ow);
        ig::norm_prefill(H, fill.data());
        uint32_t *dext = nullptr, *dout = nullptr, *dscr = nullptr;
        CHECK(hipMalloc(&dext, ew * 4));
        CHECK(hipMalloc(&dout, ow * 4));
        CHECK(hipMalloc(&dscr, ig::norm_scratch_words(rows) * 4));
        CHECK(hipMemcpy(dext, in + pos + ig::NORM_HEADER, ew * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dout, fill.data(), ow * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_normalize, dim3((H.lanes + 63) / 64), dim3(64), 0, 0, ig::norm_params(H, dext, dout, dscr), H.lanes);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        if (int rc = collect(dout, ow)) return rc;
        CHECK(hipFree(dext));
        CHECK(hipFree(dout));
        CHECK(hipFree(dscr));
        printf("ingestcheck: record %08x, %u rows, items %u..%u on %u lanes\n", in[pos - 2], rows, H.first, H.first + H.n - 1, H.lanes);
        pos += iw;
        return 0;
    }
    int tables(uint32_t n) {
        if (n != 1) return 1;
        if (int rc = collect(d_pow, DLOG_POW_WORDS)) return rc;
        if (int rc = collect(reinterpret_cast<const uint32_t*>(d_hash), ig::DLOG_HASH_BYTES / 4)) return rc;
        printf("ingestcheck: record %08x, the tables\n", in[pos - 2]);
        return 0;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: ingestcheck IN OUT\n");
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
    uint32_t* pow = nullptr;
    uint8_t* hash = nullptr;
    CHECK(hipMalloc(&pow, DLOG_POW_WORDS * 4));
    CHECK(hipMalloc(&hash, ig::DLOG_HASH_BYTES));
    CHECK(hipMemsetAsync(hash, 0, ig::DLOG_HASH_BYTES, 0));
    hipLaunchKernelGGL(k_tables, dim3(7), dim3(256), 0, 0, pow, hash);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    device_records x{in.data(), in.size()};
    x.C = ig::ctx{dlog_tables{pow, hash}};
    x.d_pow = pow;
    x.d_hash = hash;
    const int rc = ig::run_records(x);
    if (rc) {
        fprintf(stderr, "record %d failed with %d (3: unknown stage code)\n", x.records, rc);
        return rc;
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(x.out.data(), 4, x.out.size(), g) != x.out.size() || fclose(g) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    printf("ingestcheck: %d records, %zu output words\n", x.records, x.out.size());
    return 0;
}
