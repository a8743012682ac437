// Peak rate of the f64 vector FMA (v_fma_f64 / v_fmac_f64) on this GPU beside the f64 MFMA's, and
// of both engines at once.  Three measurements with the launch geometry of mfma_f64_peak.hip
// (4, 8, 16 waves per CU):
//   valu : every wave runs 32 independent per-lane FMA chains in plain C++ (__builtin_fma): 8
//          wave-uniform operands x 4 per-lane operands, the shape of a conv with lane = position.
//   mfma : every wave issues independent v_mfma_f64_16x16x4f64 into 4 accumulators.
//   both : workgroups of 8 waves; waves 0-3 (one per SIMD) run the MFMA loop, waves 4-7 the FMA
//          loop (mode 1: the reverse), all for the same wall-clock budget; each wave counts its
//          iterations, the two rates and their sum are reported.  Modes 2 / 3 run every wave on the
//          MFMA / FMA loop in the same kernel, as the like-for-like single-engine rates.
// Every timed launch runs for about 20 ms behind a warm-up launch of the same length, so the clocks
// have settled.
// Build: hipcc --offload-arch=gfx950 -O3.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int NW = 8, NX = 4;  // FMA chains per lane: NW uniform x NX per-lane operands

struct FmaState {
    double acc[NW][NX], w[NW], x[NX];
    __device__ void init(double a0) {
        for (int c = 0; c < NW; ++c) {
            w[c] = a0 + c;  // from a kernel argument: wave-uniform
            for (int p = 0; p < NX; ++p) acc[c][p] = 0.0;
        }
        for (int p = 0; p < NX; ++p) x[p] = a0 * 0.25 + threadIdx.x + 64 * p;
    }
    __device__ __forceinline__ void step() {
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int p = 0; p < NX; ++p) acc[c][p] = __builtin_fma(w[c], x[p], acc[c][p]);
    }
    __device__ double sum() const {
        double s = 0;
        for (int c = 0; c < NW; ++c)
            for (int p = 0; p < NX; ++p) s += acc[c][p];
        return s;
    }
};

constexpr int NACC = 4;
struct MfmaState {
    f64x4_t acc[NACC];
    double a, b;
    __device__ void init(double a0) {
        for (int t = 0; t < NACC; ++t) acc[t] = (f64x4_t){0.0, 0.0, 0.0, 0.0};
        a = a0 + threadIdx.x, b = a0 * 0.5 + blockIdx.x;
    }
    __device__ __forceinline__ void step() {
#pragma unroll
        for (int t = 0; t < NACC; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
    }
    __device__ double sum() const {
        double s = 0;
        for (int t = 0; t < NACC; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
        return s;
    }
};
constexpr double FMA_FLOPS = 64.0 * NW * NX * 2;           // per wave per step
constexpr double MFMA_FLOPS = NACC * 16.0 * 16 * 4 * 2;    // per wave per step

__global__ __launch_bounds__(256) void k_valu(double * out, int iters, double a0) {
    FmaState st;
    st.init(a0);
    for (int i = 0; i < iters; ++i) st.step();
    const double s = st.sum();
    if (s == 12345.0) out[0] = s;  // keep the loop
}

__global__ __launch_bounds__(256) void k_mfma(double * out, int iters, double a0) {
    MfmaState st;
    st.init(a0);
    for (int i = 0; i < iters; ++i) st.step();
    const double s = st.sum();
    if (s == 12345.0) out[0] = s;
}

// mode 0: waves 0-3 of a workgroup run the MFMA loop and waves 4-7 the FMA loop; 1: the reverse; 2: all
// MFMA; 3: all FMA; until `ticks` of the constant 100 MHz clock have passed.  cnt[global wave] = steps
// done (in batches of 64), bit 31 set on MFMA waves.
__global__ __launch_bounds__(512) void k_both(double * out, unsigned * cnt, long long ticks, double a0, int mode) {
    const int wave = threadIdx.x >> 6;
    const bool mf = mode == 2 || (mode == 0 && wave < 4) || (mode == 1 && wave >= 4);
    const long long t0 = wall_clock64();
    unsigned n = 0;
    double s;
    if (mf) {  // wave-uniform branch
        MfmaState st;
        st.init(a0);
        do {
            for (int i = 0; i < 64; ++i) st.step();
            n += 64;
        } while (wall_clock64() - t0 < ticks);
        s = st.sum();
    } else {
        FmaState st;
        st.init(a0);
        do {
            for (int i = 0; i < 64; ++i) st.step();
            n += 64;
        } while (wall_clock64() - t0 < ticks);
        s = st.sum();
    }
    if ((threadIdx.x & 63) == 0) cnt[blockIdx.x * 8 + wave] = n | (mf ? 0x80000000u : 0u);
    if (s == 12345.0) out[0] = s;
}

template <typename F>
static float timed(F launch) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    launch();  // warm-up
    (void)hipEventRecord(e0);
    launch();
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
}

int main() {
    double * d;
    unsigned * cnt;
    const int max_waves = 256 * 16;
    (void)hipMalloc(&d, 8);
    (void)hipMalloc(&cnt, max_waves * sizeof(unsigned));
    for (int wpc : {4, 8, 16}) {  // waves per CU
        const int blocks = 256 * wpc / 4, iters = 8192 * 160 / wpc;
        float ms = timed([&] { hipLaunchKernelGGL(k_valu, dim3(blocks), dim3(256), 0, 0, d, iters, 1.0); });
        printf("{\"case\": \"valu\", \"chains\": %d, \"waves_per_cu\": %d, \"ms\": %.3f, \"tflops_f64_fma\": %.2f}\n", NW * NX, wpc, ms,
               (double)blocks * 4 * iters * FMA_FLOPS / ms / 1e9);
        ms = timed([&] { hipLaunchKernelGGL(k_mfma, dim3(blocks), dim3(256), 0, 0, d, iters / 2, 1.0); });
        printf("{\"case\": \"mfma\", \"acc\": %d, \"waves_per_cu\": %d, \"ms\": %.3f, \"tflops_f64_mfma\": %.2f}\n", NACC, wpc, ms,
               (double)blocks * 4 * (iters / 2) * MFMA_FLOPS / ms / 1e9);
    }
    for (int mode : {0, 1, 2, 3})
        for (int wpc : {8, 16}) {  // modes 0 / 1: half of every SIMD's waves on each engine
            const int blocks = 256 * wpc / 8;
            const long long ticks = 2000000;  // 20 ms of the 100 MHz clock
            const float ms = timed([&] {
                (void)hipMemsetAsync(cnt, 0, max_waves * sizeof(unsigned), 0);
                hipLaunchKernelGGL(k_both, dim3(blocks), dim3(512), 0, 0, d, cnt, ticks, 1.0, mode);
            });
            std::vector<unsigned> h(blocks * 8);
            (void)hipMemcpy(h.data(), cnt, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
            double nm = 0, nf = 0;
            for (unsigned v : h) (v >> 31 ? nm : nf) += v & 0x7fffffffu;
            const double tm = nm * MFMA_FLOPS / ms / 1e9, tf = nf * FMA_FLOPS / ms / 1e9;
            printf("{\"case\": \"both\", \"mode\": %d, \"waves_per_cu\": %d, \"ms\": %.3f, \"tflops_f64_mfma\": %.2f, \"tflops_f64_fma\": %.2f, \"tflops_sum\": %.2f}\n",
                   mode, wpc, ms, tm, tf, tm + tf);
        }
    return 0;
}
