// curand_kernel.h stand-in for oracle/ref_core_probe.cpp (test infrastructure; found first on -Iref_shim).
//
// cuRAND is not available where the fixtures are generated, and the product replaced the reference's XORWOW streams by its own
// generator on purpose: the random SOURCE is not part of the contract.  What the pins check is which draws
// the reference takes, in what order, and the arithmetic applied to them.  So this header serves curand_uniform() from a tape of
// integers k in [1, 2^24], u = k * 2^-24 — exactly the values the product's generator can produce (rt_math.hpp, Rng::next) — and
// counts the draws.  The reference's own cuRandom.cuh and glm::cuRandomInUnit / cuRandomOnUnit (glm_utils.h:73-100, enabled by
// CURAND_KERNEL_H_ below) stay in the pinned code.  Running past the end of the tape aborts: no value is ever invented.
#ifndef CURAND_KERNEL_H_
#define CURAND_KERNEL_H_

#include <cstdint>
#include <cstdio>
#include <cstdlib>

struct curandStateXORWOW { int unused; };
typedef struct curandStateXORWOW curandStateXORWOW_t;

namespace ref_tape {
inline const uint32_t* k = nullptr;   // the tape
inline size_t n = 0;                  // its length
inline size_t pos = 0;                // draws consumed so far
inline void load(const uint32_t* tape, size_t len) { k = tape; n = len; pos = 0; }
}  // namespace ref_tape

// the seed / sequence / offset of the reference's per-pixel streams select a cuRAND stream; the tape replaces all of them
inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandStateXORWOW_t*) {}
inline void skipahead(unsigned long long n, curandStateXORWOW_t*) {
    std::fprintf(stderr, "curand stand-in: skipahead(%llu) is not served by a tape\n", n);
    std::abort();
}
inline float curand_uniform(curandStateXORWOW_t*) {
    if (ref_tape::pos >= ref_tape::n) {
        std::fprintf(stderr, "curand stand-in: tape overrun after %zu draws\n", ref_tape::n);
        std::abort();
    }
    const uint32_t k = ref_tape::k[ref_tape::pos++];
    if (k < 1u || k > (1u << 24)) {
        std::fprintf(stderr, "curand stand-in: tape value %u outside [1, 2^24]\n", k);
        std::abort();
    }
    return (float)k * 0x1p-24f;   // exact: k has at most 24 significant bits
}

#endif  // CURAND_KERNEL_H_
