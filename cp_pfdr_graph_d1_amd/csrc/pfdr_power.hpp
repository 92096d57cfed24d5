// What the power methods of the dense and of the sparse operator norm share
// (pfdr_gram.hip owns the kernels; pfdr_sparse_norm.hip is the other user).
#pragma once
#include "pfdr_dev.hpp"

namespace pfdr {

// Starting value number i: U[-1, 1) from splitmix64 (deterministic).  Both
// entries number their values i = r + c n (coordinate r of start c, vectors of
// length n), c counted across batches: start c is the same vector in any batch.
__device__ __forceinline__ double power_start_value(unsigned long long i) {
    unsigned long long z = i * 0xD1B54A32D192ED03ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// k_power_step on stream s: the reference's per-start stopping rule over the
// B <= 64 starts of a batch (a = new norms, b = old; state[c]: 0 running, 1
// stopped; *running += the starts still running, zeroed by the caller).
template <typename real>
void power_step(int B, const real *a, real *b, int *state, real nTol, int *running,
                hipStream_t s);

}  // namespace pfdr
