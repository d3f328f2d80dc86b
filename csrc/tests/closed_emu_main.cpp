// The closed / maximal flag kernel (csrc/kernels/closed.hip: the node hash, the sibling-run
// chains in LDS, the idempotent byte marks, the fold) runs on the CPU wave emulator under
// AddressSanitizer/UBSan (tests/test_emu_closed.py), in the host trie's widths (hash built by
// rules.hip's rules_hash_build) and the device-resident trie's (i32 parents, u16 or i32 items,
// u16 counts).  Every flag must equal the transaction-based definition computed here: S is closed
// iff the AND of the transactions holding S has no item outside S, maximal iff no item outside S
// keeps the support at the threshold.
//
//   closed_emu clique <n_items>                 the all-ties clique (40 full rows + singletons)
//   closed_emu random <n_tx> <n_items> <seed> <min_count>
//   closed_emu missing                          a trie lacking a subset: the error word must be 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../kernels/kernels.hpp"

using namespace kmls;

namespace {

struct Trie {
  std::vector<int64_t> parent;
  std::vector<int32_t> item;
  std::vector<uint32_t> count;
  std::vector<uint8_t> depth;
  std::vector<std::vector<int32_t>> tids;  // per node (the oracle's input)
  std::vector<std::vector<int32_t>> sets;
};

// host tid-list miner, size-major (breadth first) so that parents precede children
Trie mine(const std::vector<std::vector<int32_t>>& tid_of, uint32_t minc) {
  Trie t;
  std::vector<int64_t> level;
  for (int32_t x = 0; x < (int32_t)tid_of.size(); ++x)
    if (tid_of[(size_t)x].size() >= minc) {
      level.push_back((int64_t)t.item.size());
      t.parent.push_back(-1);
      t.item.push_back(x);
      t.count.push_back((uint32_t)tid_of[(size_t)x].size());
      t.depth.push_back(1);
      t.tids.push_back(tid_of[(size_t)x]);
      t.sets.push_back({x});
    }
  while (!level.empty()) {
    std::vector<int64_t> nxt;
    for (int64_t p : level)
      for (int32_t x = t.item[(size_t)p] + 1; x < (int32_t)tid_of.size(); ++x) {
        std::vector<int32_t> nt;
        std::set_intersection(t.tids[(size_t)p].begin(), t.tids[(size_t)p].end(),
                              tid_of[(size_t)x].begin(), tid_of[(size_t)x].end(),
                              std::back_inserter(nt));
        if (nt.size() < minc) continue;
        nxt.push_back((int64_t)t.item.size());
        t.parent.push_back(p);
        t.item.push_back(x);
        t.count.push_back((uint32_t)nt.size());
        t.depth.push_back((uint8_t)(t.depth[(size_t)p] + 1));
        t.tids.push_back(std::move(nt));
        std::vector<int32_t> s = t.sets[(size_t)p];
        s.push_back(x);
        t.sets.push_back(std::move(s));
      }
    level.swap(nxt);
  }
  return t;
}

// the definition, from the transactions alone
std::vector<uint8_t> oracle(const Trie& t, const std::vector<std::vector<int32_t>>& tid_of,
                            uint32_t minc) {
  const int64_t n = (int64_t)t.item.size();
  std::vector<uint8_t> f((size_t)n);
  for (int64_t v = 0; v < n; ++v) {
    bool closed = true, maximal = true;
    for (int32_t x = 0; x < (int32_t)tid_of.size(); ++x) {
      if (std::find(t.sets[(size_t)v].begin(), t.sets[(size_t)v].end(), x) != t.sets[(size_t)v].end())
        continue;
      std::vector<int32_t> nt;
      std::set_intersection(t.tids[(size_t)v].begin(), t.tids[(size_t)v].end(),
                            tid_of[(size_t)x].begin(), tid_of[(size_t)x].end(),
                            std::back_inserter(nt));
      if (nt.size() == t.tids[(size_t)v].size()) closed = false;
      if (nt.size() >= minc) maximal = false;
    }
    f[(size_t)v] = (uint8_t)((closed ? kern::kFlagClosed : 0) | (maximal ? kern::kFlagMaximal : 0));
  }
  return f;
}

struct Scratch {
  std::vector<unsigned long long> keys;
  std::vector<int32_t> vals;
  std::vector<unsigned char> flags, eq;
  unsigned int error = 0xCDCDCDCDu;
  kern::ClosedScratch x;
  explicit Scratch(int64_t n) {
    const uint64_t cap = kern::closed_hash_slots(n);
    keys.assign((size_t)cap, 0xCDCDCDCDCDCDCDCDull);  // device memory starts as garbage
    vals.assign((size_t)cap, (int32_t)0xCDCDCDCD);
    flags.assign((size_t)n, 0xCD);
    eq.assign((size_t)n, 0xCD);
    x = kern::ClosedScratch{keys.data(), vals.data(), cap - 1, flags.data(), eq.data(), &error};
  }
};

// 0 = wide widths, 1 = i32 / u16 / u16, 2 = i32 / i32 / u16; returns the error word
unsigned run(const Trie& t, int widths, std::vector<unsigned char>& out) {
  const int64_t n = (int64_t)t.item.size();
  Scratch sc(n);
  if (widths == 0) {
    kern::closed_flags(t.parent.data(), t.item.data(), t.count.data(), t.depth.data(), n, sc.x, 2,
                       nullptr);
  } else {
    std::vector<int32_t> p32(t.parent.begin(), t.parent.end());
    std::vector<uint16_t> c16(t.count.begin(), t.count.end());
    std::vector<uint16_t> i16(t.item.begin(), t.item.end());
    kern::closed_flags_narrow(p32.data(), widths == 1 ? (const void*)i16.data() : (const void*)t.item.data(),
                              widths == 1, c16.data(), t.depth.data(), n, sc.x, 2, nullptr);
  }
  out = sc.flags;
  return sc.error;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: closed_emu clique N | random n_tx n_items seed min_count | missing\n");
    return 2;
  }
  const std::string mode = argv[1];
  std::vector<std::vector<int32_t>> tid_of;
  uint32_t minc = 1;
  if (mode == "clique" || mode == "missing") {
    const int I = mode == "clique" && argc > 2 ? std::atoi(argv[2]) : 5;
    tid_of.assign((size_t)I, {});
    for (int x = 0; x < I; ++x) {
      for (int32_t tx = 0; tx < 40; ++tx) tid_of[(size_t)x].push_back(tx);
      tid_of[(size_t)x].push_back(40 + x);
    }
    minc = 36;
  } else {
    if (argc < 6) return 2;
    const int64_t T = std::atoll(argv[2]), I = std::atoll(argv[3]);
    std::mt19937_64 rng((unsigned)std::atoi(argv[4]));
    minc = (uint32_t)std::atoi(argv[5]);
    tid_of.assign((size_t)I, {});
    std::geometric_distribution<int> pick(4.0 / (double)I);
    for (int64_t tx = 0; tx < T; ++tx) {
      const int len = (int)(rng() % 13);
      std::vector<int32_t> row;
      while ((int)row.size() < len) {
        const int32_t x = (int32_t)(pick(rng) % I);
        if (std::find(row.begin(), row.end(), x) == row.end()) row.push_back(x);
      }
      // a few items always come together: equal-support supersets (non-closed itemsets)
      if (std::find(row.begin(), row.end(), 0) != row.end() &&
          std::find(row.begin(), row.end(), 1) == row.end())
        row.push_back(1);
      for (int32_t x : row) tid_of[(size_t)x].push_back((int32_t)tx);
    }
  }
  Trie t = mine(tid_of, minc);
  const int64_t n = (int64_t)t.item.size();
  int max_depth = 0;
  for (uint8_t d : t.depth) max_depth = std::max<int>(max_depth, d);
  if (mode == "missing") {
    // drop a pair that has no children in the trie but whose supersets remain: {3, 4}
    int64_t gone = -1;
    for (int64_t v = 0; v < n; ++v)
      if (t.sets[(size_t)v] == std::vector<int32_t>{3, 4}) gone = v;
    if (gone < 0) return 3;
    Trie u;
    for (int64_t v = 0; v < n; ++v) {
      if (v == gone) continue;
      const int64_t p = t.parent[(size_t)v];
      u.parent.push_back(p > gone ? p - 1 : p);
      u.item.push_back(t.item[(size_t)v]);
      u.count.push_back(t.count[(size_t)v]);
      u.depth.push_back(t.depth[(size_t)v]);
    }
    int64_t bad = 0;
    for (int w = 0; w < 3; ++w) {
      std::vector<unsigned char> got;
      if (run(u, w, got) != 1u) ++bad;
    }
    std::printf("{\"itemsets\": %lld, \"bad\": %lld}\n", (long long)u.item.size(), (long long)bad);
    return bad ? 1 : 0;
  }
  const std::vector<uint8_t> want = oracle(t, tid_of, minc);
  int64_t bad = 0, closed = 0, maximal = 0;
  for (int64_t v = 0; v < n; ++v) {
    closed += (want[(size_t)v] & kern::kFlagClosed) != 0;
    maximal += (want[(size_t)v] & kern::kFlagMaximal) != 0;
  }
  for (int w = 0; w < 3; ++w) {
    std::vector<unsigned char> got;
    const unsigned err = run(t, w, got);
    if (err != 0) {
      std::fprintf(stderr, "widths %d: error word %u\n", w, err);
      ++bad;
    }
    int shown = 0;
    for (int64_t v = 0; v < n; ++v)
      if (got[(size_t)v] != want[(size_t)v]) {
        ++bad;
        if (shown++ < 5)
          std::fprintf(stderr, "widths %d: node %lld (size %d): want %d, got %d\n", w, (long long)v,
                       (int)t.depth[(size_t)v], (int)want[(size_t)v], (int)got[(size_t)v]);
      }
  }
  std::printf("{\"itemsets\": %lld, \"closed\": %lld, \"maximal\": %lld, \"max_depth\": %d, "
              "\"bad\": %lld}\n", (long long)n, (long long)closed, (long long)maximal, max_depth,
              (long long)bad);
  return bad ? 1 : 0;
}
