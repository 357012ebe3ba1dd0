// ds_read_b32 rate with the three address patterns of k_resample (afx_resample.hip), 512-thread workgroups, 1 and 2 per CU:
//   linear: lane-linear dwords, conflict-free -- the instruction's own rate;
//   table:  lane l starts at (140 l) mod 185 and walks in steps of 185 dwords -- the table reads of 44100 -> 16000
//           (step 185; the phase advances by frac(1 / ratio) 185 = 140 entries from one output to the next);
//   input:  lane l reads dword floor(2.75625 l) - u -- the staged samples under consecutive outputs of that ratio.
// Prints the aggregate rate in G reads/s per lane-dword: tools/bench_resample.py divides the kernel's LDS reads by it.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/lds_read_b32_rate.hip -o lds_read_b32_rate
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr int WORDS = 16384;  // 64 KB: two workgroups fit a CU

template <int MODE>
__global__ __launch_bounds__(512) void k(float *out, int iters) {
    __shared__ float lds[WORDS];
    for (int i = threadIdx.x; i < WORDS; i += blockDim.x) lds[i] = (float)i;
    __syncthreads();
    const int l = threadIdx.x;
    int first;       // dword of the lane's first read
    if (MODE == 0) first = l;
    else if (MODE == 1) first = (140 * l) % 185;
    else first = (int)(2.75625f * l) + 16;
    const unsigned base = (unsigned)(size_t)(lds + first);
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        float r[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            // linear: + 512 dwords; table: + 185 dwords; input: - 1 dword (16 reads stay inside the array)
            if (MODE == 0) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r[u]) : "v"(base), "n"(u * 2048));
            else if (MODE == 1) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r[u]) : "v"(base), "n"(u * 740));
            else asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r[u]) : "v"(base - 64), "n"((15 - u) * 4));
        }
        asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
        for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(r[u]));
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += r[u];
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

template <int MODE>
void run(const char *name, int perCu) {
    const int blocks = 256 * perCu, iters = 4000;
    float *d;
    if (hipMalloc(&d, sizeof(float) * blocks * 512) != hipSuccess) return;
    k<MODE><<<blocks, 512>>>(d, iters);
    hipDeviceSynchronize();
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0);
    k<MODE><<<blocks, 512>>>(d, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    const double reads = (double)blocks * 512 * iters * 16;
    printf("{\"pattern\": \"%s\", \"workgroups_per_cu\": %d, \"ms\": %.3f, \"g_reads_per_s\": %.0f, \"tb_per_s\": %.1f}\n", name, perCu, ms,
           reads / ms / 1e6, reads * 4 / ms / 1e9);
    hipFree(d);
}

int main() {
    for (int perCu : {1, 2}) {
        run<0>("linear", perCu);
        run<1>("table", perCu);
        run<2>("input", perCu);
    }
    return 0;
}
