// Closed / maximal itemset flags over an itemset trie that is closed under subsets.
//
// An itemset is CLOSED (bit 0) when no proper superset in the trie has the same support and
// MAXIMAL (bit 1) when it has no proper superset in the trie at all (mlxtend's fpmax).  Immediate
// supersets decide both: a frequent superset implies one a single item larger, and an equal-support
// superset implies an equal-support one-item extension.  So every node S of k >= 2 items visits
// its k subsets of k - 1 items and marks each "has a superset", and "has an equal-support
// superset" when the counts tie; a node's flags are the complement of its marks.
//
// S minus its j-th item is found through the (parent, item) -> node hash of the rule engine
// (trie_hash.hpp): from S's ancestor of j items, descend through the later items of S's path, one
// probe each (every trie follows one global item order along its paths); dropping the last item
// is the parent itself.  Nodes with the same parent P share all but the last probe of every
// chain, so a wave works on a run of consecutive siblings (at most 64) at once:
//   1. lane 0 chases P's path (items and ancestors, up to 62) into LDS;
//   2. lane j < |P| finds Q_j = node(P minus its j-th item): |P| - 1 - j probes;
//   3. the (sibling, j) grid, 64 cells per step: node(S minus item j) = child(Q_j, item[S]),
//      ONE probe per subset; then every sibling marks P.
// A run is whatever stretch of consecutive nodes shares a parent — siblings that are not adjacent
// (the device trie is size-major and only mostly sibling-contiguous) just form several runs.
// Waves take fixed chunks of kChunk consecutive nodes grid-stride: no ticket atomics.
//
// Marks: thousands of supersets mark the same few small itemsets (every pair marks its two
// singletons), so the marks are idempotent plain byte stores of 1 into two arrays (one per
// mark), skipped when the byte already reads 1 — no atomics, and a stale read only repeats a
// store of the same value.  k_closed_fold then turns the two arrays into the flag byte.
// A subset that the trie lacks sets the error word (1), as does a path longer than 63 (2).
//
// GENERATOR (bit 2) is the dual of closed: no immediate subset has the same count.  The same
// count tie that marks the subset "not closed" marks S "not a generator" (a third byte array, at
// S, same discipline), so the generator variant of k_closed_mark (a compile-time bool; the
// two-bit instantiation is the code above and nothing more) visits nothing new.  When closure ids
// are asked for, the tie also lowers up[sub] to min(up[sub], S) — the smallest equal-count
// superset one item larger — with an atomicMin issued only when the value read is larger.
// k_closure_resolve then follows up[] from every node until kClosureNone (each step adds an item:
// at most 63 steps) and writes the end point over up[v]: in a trie closed under subsets that is
// the closed superset of equal support, whichever superset is taken at each step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "kernels.hpp"
#include "trie_hash.hpp"

#define KMLS_HIP(expr)                                                                  \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) +      \
                               " at " + __FILE__ + ":" + std::to_string(__LINE__));     \
  } while (0)

namespace kmls {
namespace kern {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 256;  // consecutive nodes per wave step
constexpr int kMaxK = 63;    // longest itemset

// rules.hip's k_hash_build for the device-resident trie's widths (i32 parents, u16 / i32 items)
template <typename P, typename I>
__global__ void k_closed_hash_build(const P* __restrict__ parent, const I* __restrict__ item,
                                    int64_t n, unsigned long long* __restrict__ keys,
                                    int32_t* __restrict__ vals, unsigned long long mask) {
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += nthr) {
    const unsigned long long k = hkey((int64_t)parent[v], (int32_t)item[v]);
    unsigned long long h = hmix(k) & mask;
    while (true) {
      const unsigned long long prev = atomicCAS(&keys[h], kTrieHashEmpty, k);
      if (prev == kTrieHashEmpty || prev == k) {
        vals[h] = (int32_t)v;
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename C>
__device__ __forceinline__ void mark(const C* __restrict__ count, unsigned char* sup,
                                     unsigned char* eq, int32_t sub, C c) {
  if (sup[sub] != 1) sup[sub] = 1;
  if (count[sub] == c && eq[sub] != 1) eq[sub] = 1;
}

// the generator variant: S (node id s) marks its subset sub, and on a tie itself and up[sub]
template <typename C>
__device__ __forceinline__ void mark_gen(const C* __restrict__ count, unsigned char* sup,
                                         unsigned char* eq, unsigned char* gen, unsigned int* up,
                                         int32_t sub, int64_t s, C c) {
  if (sup[sub] != 1) sup[sub] = 1;
  if (count[sub] != c) return;
  if (eq[sub] != 1) eq[sub] = 1;
  if (gen[s] != 1) gen[s] = 1;
  if (up != nullptr && __atomic_load_n(&up[sub], __ATOMIC_RELAXED) > (unsigned int)s)
    atomicMin(&up[sub], (unsigned int)s);
}

template <bool kGen, typename P, typename I, typename C>
__global__ __launch_bounds__(kBlock) void k_closed_mark(
    const P* __restrict__ parent, const I* __restrict__ item, const C* __restrict__ count,
    const unsigned char* __restrict__ depth, int64_t n,
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ vals,
    unsigned long long mask, unsigned char* sup, unsigned char* eq, unsigned int* error,
    unsigned char* gen, unsigned int* up) {
  __shared__ int32_t s_path[kWaves][64];  // items of the run's parent P, root first
  __shared__ int32_t s_anc[kWaves][64];   // s_anc[i] = node of P's first i items (-1 for i = 0)
  __shared__ int32_t s_q[kWaves][64];     // s_q[j] = node of P minus its j-th item
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n_chunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = (int64_t)blockIdx.x * kWaves + w; c < n_chunks;
       c += (int64_t)gridDim.x * kWaves) {
    const int64_t c1 = min(n, (c + 1) * kChunk);
    int64_t s0 = c * kChunk;
    while (s0 < c1) {  // wave-uniform: one run of siblings per turn
      const int64_t par = (int64_t)parent[s0];
      const int k = depth[s0];
      const int64_t me = s0 + lane;
      const bool same = me < c1 && (int64_t)parent[me] == par && depth[me] == k;
      const unsigned long long bal = __ballot(same);
      const int r = ~bal == 0ull ? 64 : __builtin_ctzll(~bal);  // >= 1: lane 0 is the run's head
      if (k < 2 || k > kMaxK || par < 0 || par >= n) {
        // singletons mark nothing; anything else here is not a trie this kernel can walk
        if (lane == 0 && !(k == 1 && par < 0)) atomicExch(error, k > kMaxK ? 2u : 1u);
        s0 += r;
        continue;
      }
      const int kp = k - 1;  // |P|
      if (lane == 0) {
        int64_t v = par;
        bool ok = true;
        for (int i = kp; i >= 1; --i) {
          if (v < 0 || v >= n) {
            ok = false;
            break;
          }
          s_anc[w][i] = (int32_t)v;
          s_path[w][i - 1] = (int32_t)item[v];
          v = (int64_t)parent[v];
        }
        s_anc[w][0] = -1;
        if (!ok || v != -1) {  // depth and parents disagree: no chain starts
          atomicExch(error, 1u);
          for (int i = 0; i <= kp; ++i) s_anc[w][i] = -2;
        }
      }
      wave_sync();
      if (lane < kp) {
        int32_t q = s_anc[w][lane];
        for (int i = lane + 1; i < kp && q >= -1; ++i)
          q = hlookup(keys, vals, mask, q, s_path[w][i]);
        if (q < -1) atomicExch(error, 1u);
        s_q[w][lane] = q;
      }
      wave_sync();
      const int cells = r * kp;
      for (int t = lane; t < cells; t += 64) {
        const int sib = t / kp, j = t - sib * kp;
        const int64_t s = s0 + sib;
        const int32_t q = s_q[w][j];
        if (q < -1) continue;
        const int32_t sub = hlookup(keys, vals, mask, q, (int32_t)item[s]);
        if (sub < 0) atomicExch(error, 1u);
        else if constexpr (kGen) mark_gen(count, sup, eq, gen, up, sub, s, count[s]);
        else mark(count, sup, eq, sub, count[s]);
      }
      if constexpr (kGen) {
        if (lane < r) mark_gen(count, sup, eq, gen, up, (int32_t)par, s0 + lane, count[s0 + lane]);
      } else {
        if (lane < r) mark(count, sup, eq, (int32_t)par, count[s0 + lane]);
      }
      wave_sync();  // the next run rewrites the LDS rows
      s0 += r;
    }
  }
}

__global__ void k_closed_fold(unsigned char* __restrict__ sup, const unsigned char* __restrict__ eq,
                              int64_t n) {
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += nthr)
    sup[v] = (unsigned char)((eq[v] == 1 ? 0 : kFlagClosed) | (sup[v] == 1 ? 0 : kFlagMaximal));
}

// three-bit fold: bit 2 is the complement of the generator mark
__global__ void k_closed_fold_gen(unsigned char* __restrict__ sup,
                                  const unsigned char* __restrict__ eq,
                                  const unsigned char* __restrict__ gen, int64_t n) {
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += nthr)
    sup[v] = (unsigned char)((eq[v] == 1 ? 0 : kFlagClosed) | (sup[v] == 1 ? 0 : kFlagMaximal) |
                             (gen[v] == 1 ? 0 : kFlagGenerator));
}

// up[v] becomes the end of v's chain.  In place: every value a slot ever holds (the next step,
// then the chain's end; the end's own slot holds itself) lies on its node's chain, so a walk that
// reads a slot another thread has already resolved only skips ahead
__global__ void k_closure_resolve(unsigned int* up, int64_t n) {
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += nthr) {
    unsigned int x = (unsigned int)v;
    for (int step = 0; step < kMaxK; ++step) {
      const unsigned int u = __atomic_load_n(&up[x], __ATOMIC_RELAXED);
      if (u == kClosureNone || u == x || (int64_t)u >= n) break;
      x = u;
    }
    __atomic_store_n(&up[v], x, __ATOMIC_RELAXED);
  }
}

template <typename P, typename I, typename C>
void run_marks(const P* parent, const I* item, const C* count, const unsigned char* depth,
               int64_t n, const ClosedScratch& x, int n_cus, hipStream_t s) {
  const int64_t n_chunks = (n + kChunk - 1) / kChunk;
  const int g = (int)std::min<int64_t>((int64_t)std::max(1, n_cus) * 8,
                                       (n_chunks + kWaves - 1) / kWaves);
  const int gf = (int)std::min<int64_t>(8192, (n + kBlock - 1) / kBlock);
  if (x.gen == nullptr) {
    if (x.up != nullptr) throw std::invalid_argument("closed flags: closure ids need the generator marks");
    hipLaunchKernelGGL((k_closed_mark<false, P, I, C>), dim3(g), dim3(kBlock), 0, s, parent, item,
                       count, depth, n, (const unsigned long long*)x.keys, (const int32_t*)x.vals,
                       x.mask, x.flags, x.eq, x.error, (unsigned char*)nullptr,
                       (unsigned int*)nullptr);
    KMLS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_closed_fold, dim3(gf), dim3(kBlock), 0, s, x.flags, x.eq, n);
    KMLS_HIP(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL((k_closed_mark<true, P, I, C>), dim3(g), dim3(kBlock), 0, s, parent, item,
                     count, depth, n, (const unsigned long long*)x.keys, (const int32_t*)x.vals,
                     x.mask, x.flags, x.eq, x.error, x.gen, x.up);
  KMLS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_closed_fold_gen, dim3(gf), dim3(kBlock), 0, s, x.flags, x.eq,
                     (const unsigned char*)x.gen, n);
  KMLS_HIP(hipGetLastError());
  if (x.up != nullptr) {
    hipLaunchKernelGGL(k_closure_resolve, dim3(gf), dim3(kBlock), 0, s, x.up, n);
    KMLS_HIP(hipGetLastError());
  }
}

void clear_marks(const ClosedScratch& x, int64_t n, hipStream_t s) {
  KMLS_HIP(hipMemsetAsync(x.flags, 0, (size_t)n, s));
  KMLS_HIP(hipMemsetAsync(x.eq, 0, (size_t)n, s));
  if (x.gen != nullptr) KMLS_HIP(hipMemsetAsync(x.gen, 0, (size_t)n, s));
  if (x.up != nullptr) KMLS_HIP(hipMemsetAsync(x.up, 0xFF, (size_t)n * 4, s));  // kClosureNone
}

void clear(const ClosedScratch& x, int64_t n, hipStream_t s) {
  KMLS_HIP(hipMemsetAsync(x.keys, 0xFF, (size_t)(x.mask + 1) * 8, s));
  clear_marks(x, n, s);
  KMLS_HIP(hipMemsetAsync(x.error, 0, 4, s));
}

template <typename I>
void narrow(const int32_t* parent, const I* item, const uint16_t* count,
            const unsigned char* depth, int64_t n, const ClosedScratch& x, int n_cus,
            hipStream_t s) {
  const int g = (int)std::min<int64_t>(8192, (n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((k_closed_hash_build<int32_t, I>), dim3(g), dim3(kBlock), 0, s, parent, item,
                     n, x.keys, x.vals, x.mask);
  KMLS_HIP(hipGetLastError());
  run_marks(parent, item, count, depth, n, x, n_cus, s);
}

}  // namespace

uint64_t closed_hash_slots(int64_t n) {
  uint64_t cap = 1;
  while (cap < (uint64_t)std::max<int64_t>(n, 1) * 2) cap <<= 1;
  return cap;
}

void closed_flags(const int64_t* parent, const int32_t* item, const uint32_t* count,
                  const unsigned char* depth, int64_t n, const ClosedScratch& x, int n_cus,
                  hipStream_t s) {
  if (n <= 0) return;
  clear(x, n, s);
  rules_hash_build(parent, item, n, x.keys, x.vals, x.mask, s);
  run_marks(parent, item, count, depth, n, x, n_cus, s);
}

void closed_marks(const int64_t* parent, const int32_t* item, const uint32_t* count,
                  const unsigned char* depth, int64_t n, const ClosedScratch& x, int n_cus,
                  hipStream_t s) {
  if (n <= 0) return;
  clear_marks(x, n, s);
  run_marks(parent, item, count, depth, n, x, n_cus, s);
}

void closed_flags_narrow(const int32_t* parent, const void* item, bool item16,
                         const uint16_t* count, const unsigned char* depth, int64_t n,
                         const ClosedScratch& x, int n_cus, hipStream_t s) {
  if (n <= 0) return;
  clear(x, n, s);
  if (item16) narrow(parent, (const uint16_t*)item, count, depth, n, x, n_cus, s);
  else narrow(parent, (const int32_t*)item, count, depth, n, x, n_cus, s);
}

}  // namespace kern
}  // namespace kmls
