// Link stubs for oracle/ref_core_probe.cpp (test infrastructure): the CUDA runtime calls of BVH_Handle (BVH.cu:110-130) as host
// malloc / memcpy / free, so that BVH_Handle::Factory's node arrays and the BVH built over them live in host memory and the
// reference's BVH::ClosestIntersection runs on the host.  They copy bytes only.  prelude.h's newOnDevice takes its memory from this
// cudaMalloc, so every block the reference hands to cudaFree came from malloc.
#include <cstdlib>
#include <cstring>

#include <cuda_runtime.h>

extern "C" {
cudaError_t cudaMalloc(void** p, size_t size) {
    *p = std::malloc(size ? size : 1);
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
cudaError_t cudaMemcpy(void* dst, const void* src, size_t count, enum cudaMemcpyKind) {
    std::memcpy(dst, src, count);
    return cudaSuccess;
}
cudaError_t cudaFree(void* p) {
    std::free(p);
    return cudaSuccess;
}
}
