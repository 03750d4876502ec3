// devprims.hip -- both sides of every device-only helper branch of jda_device_core.h behind one C interface.
//
// Test infrastructure (tests/test_devprims_cpu.py, tests/test_gpu_devprims.py), built with the product's own compiler flags so
// that the device code is what the product's build makes of the header.  devprims_host_* run the helpers' host sides in a loop,
// devprims_device_* their device sides in a plain kernel: lane = element, bounds-checked, every access inside the buffers handed
// in (device pointers of the caller's, sized as the host arrays are).  The launches are on the null stream; the call returns
// the hipError_t after the device is idle again.  Nothing of the product's runtime is used.
#include <hip/hip_runtime.h>

#include "devprims_ops.h"

#define DP_EXPORT extern "C" __attribute__((visibility("default")))

__global__ void dp_k_val(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = dp_val(op, a[i], b[i], c[i]);
}
// one wavefront a workgroup, every lane present (n is a multiple of 64)
__global__ void __launch_bounds__(64) dp_k_wave(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if ((int)(blockIdx.x * 64u) + 64 > n) return;                 // (uniform: a whole wavefront or none)
    uint32_t r0, r1;
    dp_wave(op, threadIdx.x, a[i], b[i], nullptr, r0, r1);
    out[2 * i] = r0; out[2 * i + 1] = r1;
}
// the window behind a 16-byte pad, so that it is 16-byte aligned and not at LDS address 0 (jda_wr_init)
struct dp_lds_window { uint32_t pad[DP_WIN_PAD / 4u]; uint32_t w[DP_WIN_BYTES / 4u]; };
__global__ void __launch_bounds__(64) dp_k_wr(const uint32_t *win, const uint32_t *start, const uint8_t *steps, uint32_t *out, int nwalks, int maxsteps)
{
    __shared__ __attribute__((aligned(16))) dp_lds_window L;
    if (threadIdx.x < DP_WIN_PAD / 4u) L.pad[threadIdx.x] = 0x5a5a5a5au;
    L.w[threadIdx.x] = win[threadIdx.x];                           // 64 lanes, 64 dwords
    __syncthreads();
    const int w = (int)(blockIdx.x * 64u + threadIdx.x);
    if (w < nwalks)
        dp_wr_walk((const uint8_t *)L.w, start[w] >> 3, start[w] & 7u, steps + (size_t)w * maxsteps, out + (size_t)w * maxsteps, (uint32_t)maxsteps);
}
__global__ void __launch_bounds__(64) dp_k_lds(int op, const uint32_t *win, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    __shared__ __attribute__((aligned(16))) dp_lds_window L;
    if ((int)(blockIdx.x * 64u) + 64 > n) return;                 // (uniform)
    if (threadIdx.x < DP_WIN_PAD / 4u) L.pad[threadIdx.x] = 0x5a5a5a5au;
    L.w[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (op == DP_COEF_STORE) {
        dp_coef_store((uint8_t *)L.w, a[i], b[i]);
        __syncthreads();
        out[i] = L.w[threadIdx.x];
    } else
        out[i] = dp_lds_read(op, (const uint8_t *)L.w, a[i], b[i]);
}
__global__ void dp_k_cube(int op, uint32_t *out, uint32_t first, int n)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = dp_cube(op, first + (uint32_t)i);
}

static int dp_finish()
{
    const hipError_t launch = hipGetLastError();
    const hipError_t sync = hipDeviceSynchronize();
    return (int)(launch != hipSuccess ? launch : sync);
}
static unsigned dp_blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

DP_EXPORT int devprims_ops(int family)
{
    return family == 1 ? DP_VAL_OPS : family == 2 ? DP_WAVE_OPS : family == 3 ? DP_LDS_OPS : family == 4 ? DP_CUBE_OPS : 0;
}
DP_EXPORT void devprims_host_val(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n) { dp_host_val(op, a, b, c, out, n); }
DP_EXPORT void devprims_host_wave(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n) { dp_host_wave(op, a, b, out, n); }
DP_EXPORT void devprims_host_wr(const uint32_t *win, const uint32_t *start, const uint8_t *steps, uint32_t *out, int nwalks, int maxsteps) { dp_host_wr(win, start, steps, out, nwalks, maxsteps); }
DP_EXPORT void devprims_host_lds(int op, const uint32_t *win, const uint32_t *a, const uint32_t *b, uint32_t *out, int n) { dp_host_lds(op, win, a, b, out, n); }
DP_EXPORT void devprims_host_cube(int op, uint32_t *out, uint32_t first, int n) { dp_host_cube(op, out, first, n); }

DP_EXPORT int devprims_device_val(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dp_k_val, dim3(dp_blocks(n, 256)), dim3(256), 0, 0, op, a, b, c, out, n);
    return dp_finish();
}
DP_EXPORT int devprims_device_wave(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    if (n < 64) return 0;
    hipLaunchKernelGGL(dp_k_wave, dim3((unsigned)(n / 64)), dim3(64), 0, 0, op, a, b, out, n);
    return dp_finish();
}
DP_EXPORT int devprims_device_wr(const uint32_t *win, const uint32_t *start, const uint8_t *steps, uint32_t *out, int nwalks, int maxsteps)
{
    if (nwalks <= 0 || maxsteps <= 0) return 0;
    hipLaunchKernelGGL(dp_k_wr, dim3(dp_blocks(nwalks, 64)), dim3(64), 0, 0, win, start, steps, out, nwalks, maxsteps);
    return dp_finish();
}
DP_EXPORT int devprims_device_lds(int op, const uint32_t *win, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    if (n < 64) return 0;
    hipLaunchKernelGGL(dp_k_lds, dim3((unsigned)(n / 64)), dim3(64), 0, 0, op, win, a, b, out, n);
    return dp_finish();
}
DP_EXPORT int devprims_device_cube(int op, uint32_t *out, uint32_t first, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dp_k_cube, dim3(dp_blocks(n, 256)), dim3(256), 0, 0, op, out, first, n);
    return dp_finish();
}
