// Does global_load_lds_dwordx4 accept 4-byte-aligned per-lane source addresses?  One wave copies 64 x 16 B from
// src + off floats (off = 0..3) with a row-stride of 261 floats pattern, through LDS, to out.  Host compares.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k(const float* src, float* out, int off, int stride) {
    __shared__ __attribute__((aligned(1024))) float img[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // lane -> row (lane >> 4) of a [4][64] block with row stride `stride` floats, 16-byte column lane & 15
    const float* g = src + off + (size_t)(4 * wave + (lane >> 4)) * stride + 4 * (lane & 15);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)&img[wave][0], 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int i = threadIdx.x; i < 1024; i += 256) out[i] = (&img[0][0])[i];
}
int main() {
    const int stride = 261, n = 16 * stride + 64;
    std::vector<float> h(n);
    for (int i = 0; i < n; ++i) h[i] = (float)i;
    float *d, *o;
    if (hipMalloc(&d, n * 4) != hipSuccess || hipMalloc(&o, 4096) != hipSuccess) return 2;
    hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice);
    int bad_total = 0;
    for (int off = 0; off < 4; ++off) {
        hipMemset(o, 0, 4096);
        hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, 0, d, o, off, stride);
        if (hipDeviceSynchronize() != hipSuccess) { printf("off %d: launch failed\n", off); return 3; }
        std::vector<float> r(1024);
        hipMemcpy(r.data(), o, 4096, hipMemcpyDeviceToHost);
        int bad = 0;
        for (int row = 0; row < 16; ++row)
            for (int c = 0; c < 64; ++c)
                if (r[row * 64 + c] != (float)(off + row * stride + c)) ++bad;
        printf("glds16 source offset %d floats, row stride %d floats: %d of 1024 wrong (first row starts: %g %g %g %g)\n", off, stride, bad,
               r[0], r[64], r[128], r[192]);
        bad_total += bad;
    }
    printf("RESULT unaligned_glds16 %s\n", bad_total ? "WRONG" : "OK");
    return 0;
}
