// py_random.h -- CPython's `random` on top of the tempered MT19937 word u32()
// (Modules/_randommodule.c, Lib/random.py), and the sizes random.sample and the
// sample kernel derive from the batch. Host and device arithmetic.
//   getrandbits(k), 1 <= k <= 32   u32() >> (32 - k): the TOP bits
//   _randbelow(n), 1 <= n < 2^31   k = n.bit_length(); getrandbits(k) until < n
//   random()                       a = u32() >> 5, b = u32() >> 6,
//                                  (a * 67108864 + b) / 2^53, exact in a double
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace snake {
namespace pyrandom {

constexpr int kMaxActions = 127;    // an action is an int8
constexpr int kMaxBatch = 4096;
constexpr int kMaxTries = 256;      // words one draw may reject (each rejects with probability < 9/16)
constexpr int kHashMax = 8192;      // entries of the selected indices' hash at kMaxBatch
constexpr uint32_t kEmpty = 0xffffffffu;    // (no index: n < 2^31)
constexpr int kWin = 16;            // key words an env's lane of the act kernel reads at a time
constexpr int kRowBits = 12;        // the sample kernel's per-row table of lane ids: 4096 bytes

// 32 - n.bit_length(): _randbelow(n) is u32() >> this, until below n
__host__ __device__ inline int randbelow_shift(uint32_t n) { return __builtin_clz(n); }

__host__ __device__ inline double random_double(uint32_t w0, uint32_t w1)
{
    return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
}

// random.sample's setsize: 21, and for k > 5 also 4 ** ceil(log(3 k, 4)), the
// smallest power of four that is at least 3 k (3 k is never one itself)
__host__ __device__ inline int sample_setsize(int k)
{
    int setsize = 21;
    if (k > 5) {
        int p = 1;
        while (p < 3 * k) p *= 4;
        setsize += p;
    }
    return setsize;
}

// the hash holds at most k indices in 2^bits >= 2 k entries
__host__ __device__ inline int sample_hash_bits(int k)
{
    int bits = 6;
    while ((1 << bits) < 2 * k) bits++;
    return bits;
}

__host__ __device__ inline uint32_t hash_slot(uint32_t v, int bits) { return (v * 2654435761u) >> (32 - bits); }

}  // namespace pyrandom
}  // namespace snake
