// What do line-straddling wave stores and 8-byte edge stores cost the tridiagonal storing launch's store stream, apart from the rest
// of the kernel?  A store-only stream of 240 MB (3 x 10^7 doubles, the nzval of the N = 10^7 tridiagonal CSC Jacobian): every
// wavefront writes one 3072-B span with three 1024-B non-temporal store instructions (16 B per lane), in two shapes:
//   aligned : the span starts on a 128-B line (fd_band_emit_wave_lines): three instructions, each fills 8 whole lines
//   shifted : the span's three instructions start 16 B BEFORE a line (fd_band_emit_wave with an odd first index): each touches 9
//             lines, lane 0 of the first writes 8 B instead of 16 (the other half is the neighbour's), lane 63 adds an 8-B store
//             behind the last -- five store instructions per wavefront, every line assembled from two of them
// Same grid, same workgroup size (256) and same bytes as the storing launch; values come from registers (no loads, no LDS).
// Build:  hipcc --offload-arch=gfx950 -O3 -o store_align_probe store_align_probe.hip     Run:  ./store_align_probe [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double __attribute__((ext_vector_type(2))) d2;
constexpr int BS = 256;

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); exit(1); } } while (0)

// out: 128-B aligned, nwaves * 384 + 16 doubles behind it AND 2 doubles of room before it (the shifted shape starts 16 B early)
template <bool SHIFTED>
__global__ void __launch_bounds__(BS) k_store(double* __restrict__ out, long long nwaves)
{
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const double v = (double)gw + 0.001 * lane;
    if (!SHIFTED) {
        double* base = out + 384 * gw;
#pragma unroll
        for (int a = 0; a < 3; ++a) __builtin_nontemporal_store(d2{v, v + a}, (d2*)(base + 2 * (64 * a + lane)));
    } else {
        // the wavefront's values are the elements 384 gw - 1 .. 384 gw + 382; slot 0 of its window is element 384 gw - 2
        double* base = out + 384 * gw - 2;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int sl = 2 * (64 * a + lane);
            if (sl == 0) base[1] = v;
            else __builtin_nontemporal_store(d2{v, v + a}, (d2*)(base + sl));
        }
        if (lane == 63) base[384] = v;
    }
}

template <bool SHIFTED>
static void run(const char* name, double* out, long long nwaves, int reps)
{
    const unsigned grid = (unsigned)((nwaves + BS / 64 - 1) / (BS / 64));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (int i = 0; i < 5; ++i) hipLaunchKernelGGL(k_store<SHIFTED>, dim3(grid), dim3(BS), 0, 0, out, nwaves);
    CHECK(hipDeviceSynchronize());
    std::vector<float> us;
    for (int i = 0; i < reps; ++i) {
        CHECK(hipEventRecord(a, 0));
        hipLaunchKernelGGL(k_store<SHIFTED>, dim3(grid), dim3(BS), 0, 0, out, nwaves);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        us.push_back(ms * 1000.0f);
    }
    CHECK(hipGetLastError());
    std::sort(us.begin(), us.end());
    const double bytes = (double)nwaves * 3072.0;
    printf("%-8s %6.1f MB  min %7.2f us  median %7.2f us  p90 %7.2f us  (%.2f TB/s at the median)\n", name, bytes / 1e6, us.front(),
           us[us.size() / 2], us[us.size() * 9 / 10], bytes / (us[us.size() / 2] * 1e-6) / 1e12);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
}

int main(int argc, char** argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 50;
    const long long nwaves = 78125;                 // 78125 x 3072 B = 240 MB
    double* buf = nullptr;
    CHECK(hipMalloc((void**)&buf, ((size_t)nwaves * 384 + 64) * sizeof(double)));
    double* out = buf + 16;                         // hipMalloc returns at least 256-B alignment: out is on a line, with room before it
    if (((unsigned long long)out & 127) != 0) { fprintf(stderr, "unexpected allocation alignment\n"); return 1; }
    // two rounds, alternating, so that a drift of the device's clocks shows up as a difference between the rounds
    for (int round = 0; round < 2; ++round) {
        run<false>("aligned", out, nwaves, reps);
        run<true>("shifted", out, nwaves, reps);
    }
    CHECK(hipFree(buf));
    return 0;
}
