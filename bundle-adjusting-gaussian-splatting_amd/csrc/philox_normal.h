// philox_normal.h -- the counter-based normal generator of densify.hip (children of a split row) and mcmc.hip (the SGLD noise),
// stated once: the same bits from the same (seed, row, child) in both.
#pragma once
#include "bags_common.h"

__device__ __forceinline__ void philox_round(u32& c0, u32& c1, u32& c2, u32& c3, const u32 k0, const u32 k1)
{
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
    c1 = (u32)p1; c3 = (u32)p0; c0 = n0; c2 = n2;
}
__device__ __forceinline__ float unit_open(const u32 x) { return fmaf((float)x, 2.3283064365386963e-10f, 1.1641532182693481e-10f); }   // (x + 0.5) / 2^32, in (0, 1]

// Three standard normals for (seed, source row, child): Philox-4x32-10 on the counter (row, child, 0, 0), Box-Muller on its four words.
// Depends on nothing but the key and the counter: the same children from the same seed whatever the compaction, on every rank.
__device__ __forceinline__ void normal3(const u32 seed_lo, const u32 seed_hi, const u32 row, const u32 child, float z[3])
{
    u32 c0 = row, c1 = child, c2 = 0u, c3 = 0u, k0 = seed_lo, k1 = seed_hi;
#pragma unroll
    for (int i = 0; i < 10; ++i) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const float ra = sqrtf(-2.0f * logf(unit_open(c0))), ta = 6.28318530717958647692f * unit_open(c1);
    const float rb = sqrtf(-2.0f * logf(unit_open(c2))), tb = 6.28318530717958647692f * unit_open(c3);
    z[0] = ra * cosf(ta); z[1] = ra * sinf(ta); z[2] = rb * cosf(tb);
}
