// ceg_philox.h -- the counter-based random stream of the Monte-Carlo sweeps (ceg_mc_group_sweep), host and device.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   (k0, k1) += (W0, W1) between rounds,
// M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85.  Known answers: include/ceg_hip.h, tests/test_mc_sweep_host.py.
// The Python restatement is ceg_hip/mcrng.py; both follow the same specification word for word.
#ifndef CEG_PHILOX_H
#define CEG_PHILOX_H

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CEG_PHILOX_HD __host__ __device__ __forceinline__
#else
#define CEG_PHILOX_HD inline
#endif

namespace ceg_philox {

struct Block { uint32_t w[4]; };

CEG_PHILOX_HD Block philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Block{{c0, c1, c2, c3}};
}

// U(a, b) = ((a << 21) | (b >> 11)) 2^-53 in [0, 1): 32 bits of a above the top 21 bits of b
CEG_PHILOX_HD double uniform(uint32_t a, uint32_t b)
{
    return (double)(((uint64_t)a << 21) | (uint64_t)(b >> 11)) * 0x1.0p-53;
}

// the block of (seed, absolute step, stream, purpose): key = (seed low, seed high), counter = (step low, step high, stream, purpose)
CEG_PHILOX_HD Block draw(uint64_t seed, uint64_t step, uint32_t stream, uint32_t purpose)
{
    return philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), stream, purpose, (uint32_t)seed, (uint32_t)(seed >> 32));
}

enum : uint32_t { SELECT = 0, GEOMETRY_A = 1, GEOMETRY_B = 2, ACCEPT = 3 };
// ceg_mc_group_sweep_gcmc: species and move kind; molecule and swap direction; random_translation (x, y), (z, theta of random_rotation),
// axis of random_rotation
enum : uint32_t { GCMC_SELECT = 4, GCMC_MOLECULE = 5, GCMC_RANDOM_A = 6, GCMC_RANDOM_B = 7, GCMC_RANDOM_C = 8 };
// attempt t = 0..999 of a proposal that choose_step! retries (block pockets): purposes 6-8 with counter word 3 = purpose | (t << 8);
// attempt 0 is the plain purpose
constexpr uint32_t GCMC_ATTEMPTS = 1000;
CEG_PHILOX_HD uint32_t attempt_purpose(uint32_t purpose, uint32_t attempt) { return purpose | (attempt << 8); }
// ceg_mc_group_set_tempering: the draw of a replica exchange, on the stream of the pair's chain on the lower rung
enum : uint32_t { EXCHANGE = 9 };

}  // namespace ceg_philox

#endif  // CEG_PHILOX_H
