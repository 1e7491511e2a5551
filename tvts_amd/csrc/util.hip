// HIP-event helpers exported through the C ABI so bench.py can time kernels on the launch stream.
#include "common.h"
extern "C" int tvts_event_create(void** ev) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    *ev = (void*)e;
    return (int)rc;
}
extern "C" int tvts_event_record(void* ev, hipStream_t stream) { return (int)hipEventRecord((hipEvent_t)ev, stream); }
extern "C" int tvts_event_elapsed_ms(void* start, void* stop, float* ms) {
    hipError_t rc = hipEventSynchronize((hipEvent_t)stop);
    if (rc != hipSuccess) return (int)rc;
    return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}
extern "C" int tvts_event_destroy(void* ev) { return (int)hipEventDestroy((hipEvent_t)ev); }

// rate of the constant counter (s_memrealtime / wall_clock64) in kHz, and the CU count of the device
extern "C" int tvts_device_clock_info(int device, int* wall_clock_khz, int* cu_count, int* max_shader_khz) {
    hipError_t e = hipDeviceGetAttribute(wall_clock_khz, hipDeviceAttributeWallClockRate, device);
    if (e != hipSuccess) return (int)e;
    e = hipDeviceGetAttribute(cu_count, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceGetAttribute(max_shader_khz, hipDeviceAttributeClockRate, device);
}

// p[0:nbytes] = 0: 16-byte stores on the aligned body [head, head + 16 * n16), single bytes on the < 16-byte head and tail
static __global__ void zero_bytes_kernel(unsigned char* __restrict__ p, long head, long n16, long nbytes) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    uint4* body = reinterpret_cast<uint4*>(p + head);
    for (long i = tid; i < n16; i += stride) body[i] = make_uint4(0u, 0u, 0u, 0u);
    const long tail0 = head + 16 * n16;
    if (tid < head) p[tid] = 0;
    if (tid < nbytes - tail0) p[tail0 + tid] = 0;
}

// zero fill: the flat gradient buffer at the start of a step (optimizer.zero_grad(), v2/trainer/trainer.py:476), loss accumulators,
// the dense gradient buffers of the non-pruned paths.  A kernel, not hipMemsetAsync: captured memset nodes did not reliably zero
// their buffer on hipGraph replay (ROCm 7.x: the second replay of the captured small-architecture step left garbage in the gradient)
extern "C" int tvts_zero_bytes(void* p, long nbytes, hipStream_t stream) {
    if (nbytes == 0) return TVTS_OK;  // an empty tensor: nothing to write, whatever its (possibly null) data pointer
    if (!p || nbytes < 0) return TVTS_EINVAL;
    const long mis = (long)((16 - ((uintptr_t)p & 15)) & 15);
    const long head = mis < nbytes ? mis : nbytes;
    const long n16 = (nbytes - head) / 16;
    long blocks = (n16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(zero_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (unsigned char*)p, head, n16, nbytes);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
