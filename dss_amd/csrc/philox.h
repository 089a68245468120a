// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out: a
// counter-based generator -- four output words are a pure function of a 128-bit counter and a 64-bit key, so a sample's
// randomness depends on nothing but its own index and the seed.  Plain C++ that the host compiler takes as well; the
// three published known answers of the Random123 distribution are held by tests/test_mesh_sample_cpu.py on the numpy
// restatement, and the GPU tests hold this file to that restatement bit for bit.
#pragma once
#include <stdint.h>
#include "tile_rect.h"   // DSS_HD

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u   // Weyl sequence of the key: golden ratio
#define PHILOX_W1 0xBB67AE85u   //                            sqrt(3) - 1

namespace dss {

struct Philox4 {
    uint32_t r[4];
};

// ten rounds; the key is bumped between rounds (nine times)
DSS_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    Philox4 out;
    out.r[0] = c0; out.r[1] = c1; out.r[2] = c2; out.r[3] = c3;
    return out;
}

}  // namespace dss
