// kbench_ldsdma.hip — developer micro-benchmark: a once-read 134 MB stream brought in by LDS-DMA (global_load_lds_dwordx4, 1 KiB of
// consecutive bytes per wave-instruction, four per wave into the wave's own 4 KiB of LDS, read back at 64 bytes per lane), default
// cache policy against non-temporal, beside the plain-load forms of the same traffic — read-only and compress-shaped (16 bytes per lane
// out through a non-temporal store).  Traffic-only stand-ins for w4_quant_pack_lean_kernel / w4_quant_pack_lds_kernel (HISTORY 5.1).
//   hipcc --offload-arch=gfx950 -O3 kbench_ldsdma.hip -o kbench_ldsdma
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

// SRC 0: four plain 16-byte loads per lane, 64 bytes apart (the lean kernel); 1: lane-contiguous plain loads (1 KiB per instruction; the lane
// then holds units l, l + 64, ...: not the lean layout); 2: LDS-DMA, default policy; 3: LDS-DMA, nt.   STORE: 16 bytes per lane out (nt)
template <int SRC, bool STORE>
__global__ __launch_bounds__(256) void stream(const u32x4* __restrict__ in, u32x4* __restrict__ out, uint32_t* __restrict__ sink) {
    __shared__ u32x4 stage[SRC >= 2 ? 1024 : 1];
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    u32x4 r[4];
    if constexpr (SRC == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = in[g * 4 + i];
    } else if constexpr (SRC == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = in[(g - lane) * 4 + 64 * i + lane];
    } else {
        u32x4* mine = stage + (threadIdx.x & ~63u) * 4;
        const u32x4* src = in + (g - lane) * 4 + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 64 * i),
                                             (__attribute__((address_space(3))) void*)(mine + 64 * i), 16, 0, SRC == 3 ? 2 : 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = mine[lane * 4 + i];
    }
    const u32x4 v = r[0] ^ r[1] ^ r[2] ^ r[3];
    if constexpr (STORE) __builtin_nontemporal_store(v, out + g);
    else if ((v.x ^ v.y ^ v.z ^ v.w) == 0x12345678u) sink[threadIdx.x] = v.x;  // never true for the test data; keeps the loads alive
}

int main() {
    const int64_t bytes = 134217728, lanes = bytes / 64;
    const int nsets = 6;
    std::vector<u32x4*> bufs(nsets), outs(nsets);
    for (auto& b : bufs) { CK(hipMalloc(&b, bytes)); CK(hipMemset(b, 0x5a, bytes)); }
    for (auto& b : outs) { CK(hipMalloc(&b, bytes / 4)); }
    uint32_t* sink; CK(hipMalloc(&sink, 4096));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto run = [&](const char* name, auto launch, int64_t moved) {
        for (int i = 0; i < 400; ++i) launch(i);
        CK(hipDeviceSynchronize());
        std::vector<double> per;
        for (int blk = 0; blk < 5; ++blk) {
            CK(hipEventRecord(a, 0));
            for (int i = 0; i < 60; ++i) launch(i);
            CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b)); per.push_back(ms * 1000.0 / 60);
        }
        std::sort(per.begin(), per.end());
        printf("%-64s median %6.2f us (min %6.2f max %6.2f)  %7.1f GB/s\n", name, per[2], per[0], per[4], moved / per[2] / 1e3); fflush(stdout);
    };
#define L(SRC, ST) [&](int i) { hipLaunchKernelGGL((stream<SRC, ST>), dim3((unsigned)(lanes / 256)), dim3(256), 0, 0, (const u32x4*)bufs[i % nsets], outs[i % nsets], sink); }
    for (int rep = 0; rep < 3; ++rep) {  // the forms alternate: a drift of the machine shows as a drift of every row
        run("read 134 MB: plain, 64 B per lane (4 x 16 B strided)", L(0, false), bytes);
        run("read 134 MB: plain, lane-contiguous (1 KiB per instruction)", L(1, false), bytes);
        run("read 134 MB: LDS-DMA, default policy", L(2, false), bytes);
        run("read 134 MB: LDS-DMA, nt", L(3, false), bytes);
        run("compress-shaped 134 in / 34 out: plain, 64 B per lane", L(0, true), bytes + bytes / 4);
        run("compress-shaped: LDS-DMA, default policy", L(2, true), bytes + bytes / 4);
        run("compress-shaped: LDS-DMA, nt", L(3, true), bytes + bytes / 4);
    }
    return 0;
}
