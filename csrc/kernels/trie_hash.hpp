// (parent node, item) -> node open-addressing hash over an itemset trie, shared by the rule engine
// (rules.hip) and the closed / maximal flag kernel (closed.hip).  Keys are (parent + 1) << 32 |
// item, slots are claimed by CAS (rules.hip k_hash_build, closed.hip's narrow-width twin) and
// probed linearly.  The tables are sized to a load factor of at most 0.5, so a probe for an
// absent key always ends at an empty slot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kmls {
namespace kern {

constexpr unsigned long long kTrieHashEmpty = ~0ull;

__device__ __forceinline__ unsigned long long hkey(int64_t parent, int32_t item) {
  return ((unsigned long long)(parent + 1) << 32) | (unsigned long long)(uint32_t)item;
}
__device__ __forceinline__ unsigned long long hmix(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  return k;
}

// node of (parent's itemset + item), or -2 if the trie has none
__device__ __forceinline__ int32_t hlookup(const unsigned long long* __restrict__ keys,
                                           const int32_t* __restrict__ vals,
                                           unsigned long long mask, int32_t parent, int32_t item) {
  const unsigned long long k = hkey(parent, item);
  unsigned long long h = hmix(k) & mask;
  while (true) {
    const unsigned long long kk = keys[h];
    if (kk == k) return vals[h];
    if (kk == kTrieHashEmpty) return -2;
    h = (h + 1) & mask;
  }
}

}  // namespace kern
}  // namespace kmls
