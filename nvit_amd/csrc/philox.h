// Philox4x32-10 (Salmon et al. 2011), the counter-based generator of every on-device draw (augment.hip, crop.hip):
// one call = four 32-bit words from a 128-bit counter and a 64-bit key.  Integer arithmetic only, so the numpy twins
// (tests/augment_ref.py, tests/mix_ref.py) give the same words.
#pragma once
#include "common.h"

struct Philox4 {
  unsigned v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
