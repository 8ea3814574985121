// -include prelude for oracle/ref_core_probe.cpp (test infrastructure).
//
// The reference's utilities/cuda_utilities/cuError.h (needs <format>) and cuda_utils.cuh (launches a kernel with <<<1,1>>>) are
// kept out by predefining their include guards (-DCUDA_UTILITIES_H -DCUDA_UTILITIES_CUH).  The pinned files use three names
// from them; this file gives each a host meaning of its own:
//   CUDA_ASSERT(call)   runs the call; a status other than cudaSuccess ends the probe
//   newOnDevice<T>(...) constructs a T in host memory taken from cudaMalloc (= malloc, cuda_link_stubs.cpp), so the reference's
//                       own cudaFree (BVH.cu:127: free) releases it; like the reference, no destructor runs
//   cuda_swap(a, b)     std::swap
// None of them touches a value the fixtures pin.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <new>
#include <utility>

#include <cuda_runtime.h>

namespace ref_shim {
inline void check(cudaError_t status, const char* what) {
    if (status == cudaSuccess) return;
    std::fprintf(stderr, "ref shim: %s returned %d\n", what, (int)status);
    std::abort();
}
}  // namespace ref_shim

#define CUDA_ASSERT(call) ref_shim::check((call), #call)

template <class T, class... A>
T* newOnDevice(const A&... a) {
    void* mem = nullptr;
    ref_shim::check(cudaMalloc(&mem, sizeof(T)), "cudaMalloc");
    return ::new (mem) T(a...);
}

template <class T>
void cuda_swap(T& a, T& b) { std::swap(a, b); }
