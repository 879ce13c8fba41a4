// What every internal header of libmbar_hip.so starts from: the HIP runtime, the public header, MBAR_HD, and the two pieces that
// kernel families share across their own headers -- the counter-based bootstrap stream (mbar_k_rows.hip and mbar_k_batch.hip draw
// from it, mbar_host.cpp states it for the host) and the vector fill of mbar_k_rows.hip (the context layer and mbar_batch.cpp).
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mbar_hip.h"

namespace mbar {

#if defined(__HIPCC__)
#define MBAR_HD __host__ __device__
#else
#define MBAR_HD
#endif

// Bootstrap draws as a counter-based stream (mbar_ctx_draw_bootstrap_weights on the device, mbar_bootstrap_draws on the host: the
// same function of (seed, replicate, slot)): slot j of a state with n samples draws position bootstrap_draw(...) in [0, n).
// Two rounds of the splitmix64 finaliser over key and counter; the range reduction is a 64 x 64 -> high-64 multiply (bias <= n / 2^64).
MBAR_HD inline uint64_t bootstrap_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
MBAR_HD inline int64_t bootstrap_draw(uint64_t seed, uint64_t replicate, uint64_t slot, uint64_t n) {
    const uint64_t key = bootstrap_mix64(seed + 0x9E3779B97F4A7C15ull * (replicate + 1));
    const uint64_t z = bootstrap_mix64(bootstrap_mix64(key ^ (slot * 0xD1342543DE82EF95ull)) + slot);
    return (int64_t)(((unsigned __int128)z * (unsigned __int128)n) >> 64);
}

// v[i] = value, i < n (mbar_k_rows.hip)
hipError_t launch_fill(hipStream_t s, double* v, double value, int64_t n);

}  // namespace mbar
