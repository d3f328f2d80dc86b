// Generator flags, closure ids and the min-max rule basis on the CPU wave emulator under
// AddressSanitizer/UBSan (tests/test_emu_basis.py): closed.hip's generator variant of the mark
// kernel, the three-bit fold and k_closure_resolve in all three width sets, and rules.hip's
// k_rules (both passes, with the emulator's scan in between) in the host trie's widths, over the
// same hash table.  Everything is checked against definitions computed here from the
// transactions alone: S is a generator iff dropping any one item strictly raises the support,
// closure(S) is every item held by all transactions holding S, and the basis is every closed S
// with every generator g that is a proper non-empty subset of S.
//
//   basis_emu clique <n_items>                 the all-ties clique (40 full rows + singletons)
//   basis_emu random <n_tx> <n_items> <seed> <min_count>   plus a duplicated and an AND-ed column
//   basis_emu missing                          a trie lacking a subset: the error word must be 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../kernels/kernels.hpp"

using namespace kmls;

namespace {

using Tids = std::vector<int32_t>;

struct Trie {
  std::vector<int64_t> parent;
  std::vector<int32_t> item;
  std::vector<uint32_t> count;
  std::vector<uint8_t> depth;
  std::vector<Tids> tids;
  std::vector<std::vector<int32_t>> sets;
};

Tids meet(const Tids& a, const Tids& b) {
  Tids o;
  std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(o));
  return o;
}

// host tid-list miner, size-major (breadth first) so that parents precede children
Trie mine(const std::vector<Tids>& tid_of, uint32_t minc) {
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
        Tids nt = meet(t.tids[(size_t)p], tid_of[(size_t)x]);
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

size_t support_of(const std::vector<int32_t>& s, const std::vector<Tids>& tid_of, int32_t n_tx) {
  if (s.empty()) return (size_t)n_tx;
  Tids cur = tid_of[(size_t)s[0]];
  for (size_t i = 1; i < s.size(); ++i) cur = meet(cur, tid_of[(size_t)s[i]]);
  return cur.size();
}

struct Want {
  std::vector<uint8_t> flags;     // three bits
  std::vector<int32_t> closure;   // node ids
};

// the definitions, from the transactions alone
Want oracle(const Trie& t, const std::vector<Tids>& tid_of, uint32_t minc, int32_t n_tx) {
  const int64_t n = (int64_t)t.item.size();
  std::map<std::vector<int32_t>, int32_t> id;
  for (int64_t v = 0; v < n; ++v) id[t.sets[(size_t)v]] = (int32_t)v;
  Want w;
  w.flags.resize((size_t)n);
  w.closure.resize((size_t)n);
  for (int64_t v = 0; v < n; ++v) {
    const std::vector<int32_t>& s = t.sets[(size_t)v];
    bool closed = true, maximal = true, generator = true;
    std::vector<int32_t> clo = s;
    for (int32_t x = 0; x < (int32_t)tid_of.size(); ++x) {
      if (std::find(s.begin(), s.end(), x) != s.end()) continue;
      const Tids nt = meet(t.tids[(size_t)v], tid_of[(size_t)x]);
      if (nt.size() == t.tids[(size_t)v].size()) {
        closed = false;
        clo.push_back(x);
      }
      if (nt.size() >= minc) maximal = false;
    }
    if (s.size() > 1)
      for (size_t j = 0; j < s.size(); ++j) {
        std::vector<int32_t> sub = s;
        sub.erase(sub.begin() + (long)j);
        if (support_of(sub, tid_of, n_tx) == t.tids[(size_t)v].size()) generator = false;
      }
    std::sort(clo.begin(), clo.end());
    const auto it = id.find(clo);
    w.closure[(size_t)v] = it == id.end() ? -1 : it->second;
    w.flags[(size_t)v] = (uint8_t)((closed ? kern::kFlagClosed : 0) |
                                   (maximal ? kern::kFlagMaximal : 0) |
                                   (generator ? kern::kFlagGenerator : 0));
  }
  return w;
}

struct Scratch {
  std::vector<unsigned long long> keys;
  std::vector<int32_t> vals;
  std::vector<unsigned char> flags, eq, gen;
  std::vector<unsigned int> up;
  unsigned int error = 0xCDCDCDCDu;
  kern::ClosedScratch x;
  explicit Scratch(int64_t n) {
    const uint64_t cap = kern::closed_hash_slots(n);
    keys.assign((size_t)cap, 0xCDCDCDCDCDCDCDCDull);  // device memory starts as garbage
    vals.assign((size_t)cap, (int32_t)0xCDCDCDCD);
    flags.assign((size_t)n, 0xCD);
    eq.assign((size_t)n, 0xCD);
    gen.assign((size_t)n, 0xCD);
    up.assign((size_t)n, 0xCDCDCDCDu);
    x = kern::ClosedScratch{keys.data(), vals.data(), cap - 1, flags.data(), eq.data(), &error};
    x.gen = gen.data();
    x.up = up.data();
  }
};

// 0 = wide widths, 1 = i32 / u16 / u16, 2 = i32 / i32 / u16; returns the error word
unsigned run_flags(const Trie& t, int widths, Scratch& sc) {
  const int64_t n = (int64_t)t.item.size();
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
  return sc.error;
}

struct Rule {
  int64_t s, a, c;
  double conf, lift;
  bool operator==(const Rule& o) const {
    return s == o.s && a == o.a && c == o.c && conf == o.conf && lift == o.lift;
  }
};

// both passes of k_rules over the hash table and flag bytes that run_flags(widths 0) left in sc
std::vector<Rule> run_rules(const Trie& t, Scratch& sc, int32_t n_tx, int basis, double thr,
                            unsigned* err_out) {
  const int64_t n = (int64_t)t.item.size();
  const int grid = 2;
  const int64_t waves = (int64_t)grid * kern::rules_waves_per_block();
  unsigned long long ticket = 0;
  unsigned int error = 0;
  std::vector<int64_t> nr((size_t)n + 1, 0), off((size_t)n + 1, 0);
  int kmax = 0;
  for (uint8_t d : t.depth) kmax = std::max<int>(kmax, d);
  const int sbits = kmax > 12 ? kmax : 0;
  std::vector<int32_t> scratch(sbits ? (size_t)waves << sbits : 1, (int32_t)0xCDCDCDCD);
  kern::RuleArgs a{};
  a.parent = t.parent.data();
  a.item = t.item.data();
  a.count = t.count.data();
  a.depth = t.depth.data();
  a.n = n;
  a.T = (double)n_tx;
  a.metric = 0;
  a.thr = thr;
  a.max_ante = 0;
  a.keys = sc.keys.data();
  a.vals = sc.vals.data();
  a.mask = sc.x.mask;
  a.scratch = sbits ? scratch.data() : nullptr;
  a.scratch_bits = sbits;
  a.ticket = &ticket;
  a.error = &error;
  a.pass = 0;
  a.nrules = nr.data();
  a.set_flags = basis ? sc.flags.data() : nullptr;
  a.basis = basis;
  kern::rules_pass(a, grid, nullptr);
  size_t tb = kern::rules_scan_temp_bytes(n);
  std::vector<unsigned char> tmp(tb + 1);
  kern::rules_scan(nr.data(), off.data(), n, tmp.data(), tb, nullptr);
  const int64_t total = off[(size_t)n];
  std::vector<int64_t> o_s((size_t)total + 1), o_a((size_t)total + 1), o_c((size_t)total + 1);
  std::vector<double> o_conf((size_t)total + 1), o_lift((size_t)total + 1);
  ticket = 0;
  a.pass = 1;
  a.off = off.data();
  a.o_itemset = o_s.data();
  a.o_ante = o_a.data();
  a.o_cons = o_c.data();
  a.o_conf = o_conf.data();
  a.o_lift = o_lift.data();
  kern::rules_pass(a, grid, nullptr);
  *err_out = error;
  std::vector<Rule> out((size_t)total);
  for (int64_t i = 0; i < total; ++i)
    out[(size_t)i] = Rule{o_s[(size_t)i], o_a[(size_t)i], o_c[(size_t)i], o_conf[(size_t)i],
                          o_lift[(size_t)i]};
  return out;
}

// every rule (basis = 0) or the basis, by definition: itemset order, then subset mask
std::vector<Rule> want_rules(const Trie& t, const Want& w, int32_t n_tx, int basis, double thr) {
  const int64_t n = (int64_t)t.item.size();
  std::map<std::vector<int32_t>, int32_t> id;
  for (int64_t v = 0; v < n; ++v) id[t.sets[(size_t)v]] = (int32_t)v;
  std::vector<Rule> out;
  for (int64_t s = 0; s < n; ++s) {
    const std::vector<int32_t>& set = t.sets[(size_t)s];
    const int k = (int)set.size();
    if (k < 2) continue;
    if (basis && !(w.flags[(size_t)s] & kern::kFlagClosed)) continue;
    for (uint32_t m = 1; m + 1 < (1u << k); ++m) {
      std::vector<int32_t> A, C;
      for (int i = 0; i < k; ++i) ((m >> i) & 1u ? A : C).push_back(set[(size_t)i]);
      const int32_t na = id.at(A), nc = id.at(C);
      if (basis && !(w.flags[(size_t)na] & kern::kFlagGenerator)) continue;
      const double conf = (double)t.count[(size_t)s] / (double)t.count[(size_t)na];
      if (!(conf >= thr)) continue;
      out.push_back(Rule{s, na, nc, conf, conf * (double)n_tx / (double)t.count[(size_t)nc]});
    }
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: basis_emu clique N | random n_tx n_items seed min_count | missing\n");
    return 2;
  }
  const std::string mode = argv[1];
  std::vector<Tids> tid_of;
  uint32_t minc = 1;
  int32_t n_tx = 0;
  if (mode == "clique" || mode == "missing") {
    const int I = mode == "clique" && argc > 2 ? std::atoi(argv[2]) : 5;
    tid_of.assign((size_t)I, {});
    for (int x = 0; x < I; ++x) {
      for (int32_t tx = 0; tx < 40; ++tx) tid_of[(size_t)x].push_back(tx);
      tid_of[(size_t)x].push_back(40 + x);
    }
    n_tx = 40 + I;
    minc = 36;
  } else {
    if (argc < 6) return 2;
    const int64_t T = std::atoll(argv[2]), I = std::atoll(argv[3]);
    std::mt19937_64 rng((unsigned)std::atoi(argv[4]));
    minc = (uint32_t)std::atoi(argv[5]);
    n_tx = (int32_t)T;
    tid_of.assign((size_t)I + 2, {});
    std::geometric_distribution<int> pick(4.0 / (double)I);
    for (int64_t tx = 0; tx < T; ++tx) {
      const int len = (int)(rng() % 13);
      std::vector<int32_t> row;
      while ((int)row.size() < len) {
        const int32_t x = (int32_t)(pick(rng) % I);
        if (std::find(row.begin(), row.end(), x) == row.end()) row.push_back(x);
      }
      for (int32_t x : row) tid_of[(size_t)x].push_back((int32_t)tx);
    }
    // ties: column I duplicates column 12, column I + 1 is column 6 AND column 7 (mid-frequency
    // columns: the ties reach a few sizes up without doubling the trie)
    tid_of[(size_t)I] = tid_of[12 % (size_t)I];
    tid_of[(size_t)I + 1] = meet(tid_of[6 % (size_t)I], tid_of[7 % (size_t)I]);
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
      Scratch sc((int64_t)u.item.size());
      if (run_flags(u, w, sc) != 1u) ++bad;
      if (w == 0) {  // the rule kernel over the same table reports the same missing subset
        unsigned err = 0;
        run_rules(u, sc, n_tx, 1, 0.0, &err);
        if (err != 1u) ++bad;
      }
    }
    std::printf("{\"itemsets\": %lld, \"bad\": %lld}\n", (long long)u.item.size(), (long long)bad);
    return bad ? 1 : 0;
  }
  const Want want = oracle(t, tid_of, minc, n_tx);
  int64_t bad = 0, closed = 0, generators = 0;
  for (int64_t v = 0; v < n; ++v) {
    closed += (want.flags[(size_t)v] & kern::kFlagClosed) != 0;
    generators += (want.flags[(size_t)v] & kern::kFlagGenerator) != 0;
    if (want.closure[(size_t)v] < 0) ++bad;  // the closure of a frequent itemset is frequent
    if ((want.closure[(size_t)v] == v) != ((want.flags[(size_t)v] & kern::kFlagClosed) != 0)) ++bad;
  }
  int64_t n_basis = 0, n_exact = 0, n_all = 0;
  for (int w = 0; w < 3; ++w) {
    Scratch sc(n);
    const unsigned err = run_flags(t, w, sc);
    if (err != 0) {
      std::fprintf(stderr, "widths %d: error word %u\n", w, err);
      ++bad;
    }
    int shown = 0;
    for (int64_t v = 0; v < n; ++v)
      if (sc.flags[(size_t)v] != want.flags[(size_t)v] ||
          (int64_t)sc.up[(size_t)v] != (int64_t)want.closure[(size_t)v]) {
        ++bad;
        if (shown++ < 5)
          std::fprintf(stderr, "widths %d: node %lld (size %d): want %d / %d, got %d / %lld\n", w,
                       (long long)v, (int)t.depth[(size_t)v], (int)want.flags[(size_t)v],
                       (int)want.closure[(size_t)v], (int)sc.flags[(size_t)v],
                       (long long)sc.up[(size_t)v]);
      }
    if (w != 0) continue;
    // every rule (basis 0) and a second threshold only where they are cheap on the emulator
    const bool cheap = mode == "clique";
    for (int basis = 1; basis >= (cheap ? 0 : 1); --basis)
      for (double thr : {0.0, 0.95}) {
        if (thr > 0.0 && !cheap) continue;
        unsigned rerr = 0;
        const std::vector<Rule> got = run_rules(t, sc, n_tx, basis, thr, &rerr);
        const std::vector<Rule> exp = want_rules(t, want, n_tx, basis, thr);
        if (rerr != 0 || !(got == exp)) {
          std::fprintf(stderr, "rules basis %d thr %.1f: error %u, %zu rules, want %zu\n", basis,
                       thr, rerr, got.size(), exp.size());
          ++bad;
        }
        if (thr == 0.0 && basis) {
          n_basis = (int64_t)got.size();
          for (const Rule& r : got) n_exact += r.conf == 1.0;
        }
        if (thr == 0.0 && !basis) n_all = (int64_t)got.size();
      }
  }
  std::printf("{\"itemsets\": %lld, \"closed\": %lld, \"generators\": %lld, \"max_depth\": %d, "
              "\"basis_rules\": %lld, \"exact_rules\": %lld, \"all_rules\": %lld, \"bad\": %lld}\n",
              (long long)n, (long long)closed, (long long)generators, max_depth,
              (long long)n_basis, (long long)n_exact, (long long)n_all, (long long)bad);
  return bad ? 1 : 0;
}
