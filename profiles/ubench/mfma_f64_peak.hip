// mfma_f64_peak.hip — the rate of v_mfma_f64_16x16x4_f64 on this chip, measured: independent accumulator chains on every SIMD.
//
//   hipcc -O3 --offload-arch=gfx950 profiles/ubench/mfma_f64_peak.hip -o profiles/ubench/mfma_f64_peak
//   profiles/ubench/mfma_f64_peak > profiles/ubench/mfma_f64_peak.result.txt
//
// A wave runs CH independent chains acc_c = mfma(a, b, acc_c), nothing else in the loop; workgroups of 4 waves (one per SIMD),
// WPS workgroups per compute unit.  One MFMA is 16 x 16 x 4 x 2 = 2048 flop.  Every (CH, WPS) is timed three times with device
// events after a warm-up launch; the best figure over the grid is the chip's rate for this instruction, printed last as one JSON
// line (profiles/f64_timing.py reads it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

template <int CH>
__global__ __launch_bounds__(256) void chains(double* __restrict__ out, int iters) {
    d4 acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    const double a = 1e-3 * (1 + (threadIdx.x & 3)), b = 1e-3 * (1 + (threadIdx.x & 7));
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CH; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int CH>
static int run(int cus, int wps, int iters, double* out, double* best) {
    const int blocks = cus * wps;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(chains<CH>, dim3(blocks), dim3(256), 0, 0, out, iters / 8);   // warm-up
    CHECK(hipDeviceSynchronize());
    std::vector<double> tf;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(chains<CH>, dim3(blocks), dim3(256), 0, 0, out, iters);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        tf.push_back((double)blocks * 4.0 * iters * CH * 2048.0 / (ms * 1e-3) / 1e12);
    }
    std::sort(tf.begin(), tf.end());
    std::printf("chains per wave %d, workgroups per CU %d (%d waves per SIMD): %.2f / %.2f / %.2f TFLOP/s (min / median / max of 3)\n",
                CH, wps, wps, tf[0], tf[1], tf[2]);
    if (tf[1] > *best) *best = tf[1];
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    std::printf("%s, %d compute units, %d MHz\n", prop.gcnArchName, cus, prop.clockRate / 1000);
    double* out = nullptr;
    CHECK(hipMalloc(&out, (size_t)cus * 4 * 256 * sizeof(double)));
    double best = 0.0;
    const int iters = 200000;   // x CH MFMAs per wave: tens of milliseconds a launch
    for (int wps : {1, 2, 4}) {
        if (run<1>(cus, wps, iters * 4, out, &best)) return 1;
        if (run<2>(cus, wps, iters * 2, out, &best)) return 1;
        if (run<4>(cus, wps, iters, out, &best)) return 1;
        if (run<8>(cus, wps, iters / 2, out, &best)) return 1;
    }
    CHECK(hipFree(out));
    std::printf("{\"instruction\": \"v_mfma_f64_16x16x4_f64\", \"measured_peak_tflops\": %.2f, \"compute_units\": %d}\n", best, cus);
    return 0;
}
