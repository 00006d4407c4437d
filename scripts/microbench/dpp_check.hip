// Checks the DPP lane-group exchanges of the step kernels (gsel, gscan of
// marl-snake_amd/csrc/step_lanes.h, the code that ships) against their
// definitions on random values: prints "dpp ok" or the first mismatches.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../marl-snake_amd/csrc dpp_check.hip -o dpp_check
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "step_lanes.h"

using namespace snake;

template <int G>
__global__ void k(const int *in, int *out)
{
    const int lane = threadIdx.x, k = lane % G;
    const int v = in[lane];
    unroll<G>([&](auto J) { out[J * 64 + lane] = gsel<G, J>(v); });
    out[G * 64 + lane] = gscan<G>(v, k);
}

template <int G>
int check(const int *din, int *dout, const int *hin)
{
    int h[17 * 64];
    hipLaunchKernelGGL(k<G>, dim3(1), dim3(64), 0, 0, din, dout);
    hipMemcpy(h, dout, sizeof(int) * (G + 1) * 64, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int l = 0; l < 64; l++) {
        const int gb = l / G * G;
        for (int j = 0; j < G; j++)
            if (h[j * 64 + l] != hin[gb + j]) { if (bad++ < 5) printf("G=%d gsel J=%d lane %d: %d != %d\n", G, j, l, h[j * 64 + l], hin[gb + j]); }
        int s = 0;
        for (int j = gb; j <= l; j++) s += hin[j];
        if (h[G * 64 + l] != s) { if (bad++ < 5) printf("G=%d gscan lane %d: %d != %d\n", G, l, h[G * 64 + l], s); }
    }
    return bad;
}

int main()
{
    int hin[64];
    srand(1);
    for (int i = 0; i < 64; i++) hin[i] = rand() % 1000 - 300;
    int *din, *dout;
    hipMalloc(&din, 64 * 4);
    hipMalloc(&dout, 17 * 64 * 4);
    hipMemcpy(din, hin, 64 * 4, hipMemcpyHostToDevice);
    const int bad = check<4>(din, dout, hin) + check<8>(din, dout, hin) + check<16>(din, dout, hin);
    printf(bad ? "dpp MISMATCH %d\n" : "dpp ok\n", bad);
    return bad != 0;
}
