// Closed / maximal itemset flags on the CPU (the twin of csrc/kernels/closed.hip; same bytes,
// same errors).
//
// An itemset is closed when no proper superset in the trie has the same support and maximal when
// it has no proper superset in the trie (mlxtend's fpmax).  Immediate supersets decide both, so
// every node S of k >= 2 items visits its k subsets of k - 1 items: S minus its j-th item is
// reached from S's ancestor of j items by descending through the later items of S's path in a
// (parent node, item) -> child hash (the miners extend classes in one global item order).  Each
// subset is marked "has a superset", and "has an equal-support superset" when the counts tie;
// the flags are the complement of the marks.  Work is split over threads by node block; the
// marks are idempotent relaxed byte stores, so the result does not depend on the schedule.
//
// itemset_condense adds the generator bit (no immediate subset has the same count: the same tie,
// marked at S) and closure ids: the tie lowers up[subset] to the smallest such S, and every node
// then follows up[] to its end, the closed superset of equal support.
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "kmls/host.hpp"

namespace kmls {

namespace {

constexpr uint64_t kEmpty = ~0ull;

inline uint64_t key_of(int64_t parent, int32_t item) {
  return ((uint64_t)(parent + 1) << 32) | (uint64_t)(uint32_t)item;
}
inline uint64_t mix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  return k;
}

struct ChildMap {  // open addressing, load factor <= 0.5
  std::vector<uint64_t> keys;
  std::vector<int32_t> vals;
  uint64_t mask = 0;
  explicit ChildMap(int64_t n) {
    uint64_t cap = 1;
    while (cap < (uint64_t)std::max<int64_t>(n, 1) * 2) cap <<= 1;
    keys.assign((size_t)cap, kEmpty);
    vals.assign((size_t)cap, -1);
    mask = cap - 1;
  }
  void put(int64_t parent, int32_t item, int32_t node) {
    const uint64_t k = key_of(parent, item);
    uint64_t h = mix(k) & mask;
    while (keys[(size_t)h] != kEmpty && keys[(size_t)h] != k) h = (h + 1) & mask;
    keys[(size_t)h] = k;
    vals[(size_t)h] = node;
  }
  int64_t get(int64_t parent, int32_t item) const {
    const uint64_t k = key_of(parent, item);
    uint64_t h = mix(k) & mask;
    while (true) {
      if (keys[(size_t)h] == k) return vals[(size_t)h];
      if (keys[(size_t)h] == kEmpty) return -2;
      h = (h + 1) & mask;
    }
  }
};

}  // namespace

void validate_trie_shape(const int64_t* parent, const uint8_t* depth, int64_t n_nodes,
                         const char* who) {
  for (int64_t v = 0; v < n_nodes; ++v) {
    const int64_t p = parent[v];
    const bool ok = p == -1 ? depth[v] == 1
                            : (p >= 0 && p < v && (int)depth[v] == (int)depth[p] + 1);
    KMLS_CHECK(ok, std::string(who) + ": malformed trie (a parent must precede its child and "
                                      "hold one item less)");
  }
}

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// flags_out: two bits, or three when generators; closure_out (optional) needs generators
void flags_impl(const int64_t* parent, const int32_t* item, const uint32_t* count,
                const uint8_t* depth, int64_t n_nodes, uint8_t* flags_out, bool generators,
                int32_t* closure_out, int threads) {
  if (n_nodes == 0) return;
  KMLS_CHECK(n_nodes < (1ll << 31) - 1, "itemset flags: trie larger than 2^31 nodes");
  validate_trie_shape(parent, depth, n_nodes, "itemset flags");
  ChildMap child(n_nodes);
  for (int64_t v = 0; v < n_nodes; ++v) child.put(parent[v], item[v], (int32_t)v);
  std::vector<uint8_t> sup((size_t)n_nodes, 0), eq((size_t)n_nodes, 0);
  std::vector<uint8_t> gen(generators ? (size_t)n_nodes : 0, 0);
  std::vector<uint32_t> up(closure_out ? (size_t)n_nodes : 0, kNone);
  auto mark = [&](int64_t sub, int64_t s) {
    __atomic_store_n(&sup[(size_t)sub], (uint8_t)1, __ATOMIC_RELAXED);
    if (count[sub] != count[s]) return;
    __atomic_store_n(&eq[(size_t)sub], (uint8_t)1, __ATOMIC_RELAXED);
    if (!generators) return;
    __atomic_store_n(&gen[(size_t)s], (uint8_t)1, __ATOMIC_RELAXED);
    if (closure_out) {
      uint32_t old = __atomic_load_n(&up[(size_t)sub], __ATOMIC_RELAXED);
      while ((uint32_t)s < old &&
             !__atomic_compare_exchange_n(&up[(size_t)sub], &old, (uint32_t)s, true,
                                          __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
      }
    }
  };
  const int nth = (int)std::max<int64_t>(
      1, std::min<int64_t>(threads > 0 ? threads : default_threads(), (n_nodes + 4095) / 4096));
  std::atomic<int64_t> next{0};
  std::atomic<int> bad{0};
  constexpr int64_t kBlock = 1024;
  auto worker = [&]() {
    int32_t path[64];
    int64_t anc[64];  // anc[i] = node of the first i items
    while (true) {
      const int64_t b0 = next.fetch_add(kBlock);
      if (b0 >= n_nodes) break;
      const int64_t b1 = std::min(n_nodes, b0 + kBlock);
      for (int64_t s = b0; s < b1; ++s) {
        const int k = depth[s];
        if (k < 2) continue;
        if (k > 63) {
          bad = 2;
          continue;
        }
        int64_t v = s;
        for (int i = k; i >= 1; --i) {
          anc[i] = v;
          path[i - 1] = item[v];
          v = parent[v];
        }
        anc[0] = -1;
        mark(anc[k - 1], s);  // dropping the last item: the parent
        for (int j = 0; j + 1 < k; ++j) {
          int64_t q = anc[j];
          for (int i = j + 1; i < k && q >= -1; ++i) q = child.get(q, path[i]);
          if (q < 0) bad = 1;
          else mark(q, s);
        }
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nth; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
  KMLS_CHECK(bad == 0, "itemset flags: a subset of a frequent itemset is missing from the trie "
                       "(trie not closed under subsets, or itemset longer than 63)");
  for (int64_t v = 0; v < n_nodes; ++v)
    flags_out[v] = (uint8_t)((eq[(size_t)v] ? 0 : kItemsetClosed) |
                             (sup[(size_t)v] ? 0 : kItemsetMaximal) |
                             (generators && !gen[(size_t)v] ? kItemsetGenerator : 0));
  if (!closure_out) return;
  next = 0;
  auto resolve = [&]() {
    while (true) {
      const int64_t b0 = next.fetch_add(kBlock);
      if (b0 >= n_nodes) break;
      const int64_t b1 = std::min(n_nodes, b0 + kBlock);
      for (int64_t v = b0; v < b1; ++v) {
        uint32_t x = (uint32_t)v;  // each step adds an item: at most 63 steps
        while (up[(size_t)x] != kNone) x = up[(size_t)x];
        closure_out[v] = (int32_t)x;
      }
    }
  };
  pool.clear();
  for (int t = 1; t < nth; ++t) pool.emplace_back(resolve);
  resolve();
  for (auto& th : pool) th.join();
}

}  // namespace

void itemset_flags(const int64_t* parent, const int32_t* item, const uint32_t* count,
                   const uint8_t* depth, int64_t n_nodes, uint8_t* flags_out, int threads) {
  flags_impl(parent, item, count, depth, n_nodes, flags_out, false, nullptr, threads);
}

void itemset_condense(const int64_t* parent, const int32_t* item, const uint32_t* count,
                      const uint8_t* depth, int64_t n_nodes, uint8_t* flags_out,
                      int32_t* closure_out, int threads) {
  flags_impl(parent, item, count, depth, n_nodes, flags_out, true, closure_out, threads);
}

}  // namespace kmls
