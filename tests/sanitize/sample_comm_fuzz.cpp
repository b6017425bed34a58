// sample_comm_fuzz.cpp — stand-alone driver of the host sampler's multi-rank window (cooc_sample.cpp,
// Sampler::RankCut), built with -fsanitize=address,undefined by tests/test_sampled_comm_cpu.py.
//
// W samplers stand for the ranks of a job; the item-cut exchange between them (ItemCutExchange on the device) is
// restated here on the host: every rank's sorted (item << 32 | records) histogram, the bases over lower ranks, the
// totals at each item's lowest listing rank.  On random logs the ranks' decisions, concatenated in rank order, must
// equal those of one sampler fed each window as R_0 || R_1 || ... || R_{W-1}; the item counters must be identical
// on every rank after every window, and the decision counters must add up.
#include <algorithm>
#include <cstdio>
#include <random>
#include <unordered_map>
#include <vector>

#include "../../flink-cooccurrence_amd/csrc/cooc_sample.h"

using cooc::Sampler;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "sample_comm_fuzz: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

struct Rank {
  Sampler sm;
  std::unordered_map<int32_t, int32_t> slot_of;
  std::vector<int32_t> users, slots, items, trace;
  std::vector<uint64_t> hist;
  std::vector<int32_t> base;
};

static int64_t find(const std::vector<uint64_t> &list, uint32_t item) {
  auto it = std::lower_bound(list.begin(), list.end(), uint64_t(item) << 32);
  return it != list.end() && uint32_t(*it >> 32) == item ? int64_t(uint32_t(*it)) : 0;
}

static int fuzz_one(uint64_t seed, int W, int32_t n_items, int32_t item_cut, int32_t user_cut, int n_windows, int n_rec,
                    int n_users) {
  std::mt19937_64 rng(seed);
  std::vector<Rank> ranks(static_cast<size_t>(W));
  Sampler one;
  one.enable(n_items, item_cut, user_cut, seed * 0x9E37u);
  std::unordered_map<int32_t, int32_t> one_slot;
  std::vector<int32_t> one_trace;
  one.set_trace(&one_trace);
  for (Rank &r : ranks) {
    r.sm.enable(n_items, item_cut, user_cut, seed * 0x9E37u);
    r.sm.set_trace(&r.trace);
  }
  for (int w = 0; w < n_windows; w++) {
    const int quiet = w % 3 == 2 ? int(rng() % uint64_t(W)) : -1;  // a rank without records
    for (Rank &r : ranks) {
      r.users.clear();
      r.slots.clear();
      r.items.clear();
      r.trace.clear();
    }
    for (int k = 0; k < n_rec; k++) {
      const int32_t u = int32_t(rng() % uint64_t(n_users));
      const int q = u % W;
      if (q == quiet) continue;
      Rank &r = ranks[size_t(q)];
      auto it = r.slot_of.find(u);
      if (it == r.slot_of.end()) it = r.slot_of.emplace(u, int32_t(r.slot_of.size())).first;
      r.users.push_back(u);
      r.slots.push_back(it->second);
      r.items.push_back(int32_t(rng() % 100 < 60 ? rng() % 3 : rng() % uint64_t(n_items)));
    }
    // the exchange: histograms, bases, totals at the owner slots
    size_t lmax = 0;
    for (Rank &r : ranks) {
      std::vector<int32_t> s(r.items);
      std::sort(s.begin(), s.end());
      r.hist.clear();
      for (size_t i = 0; i < s.size();) {
        size_t j = i;
        while (j < s.size() && s[j] == s[i]) j++;
        r.hist.push_back((uint64_t(uint32_t(s[i])) << 32) | uint64_t(j - i));
        i = j;
      }
      lmax = std::max(lmax, r.hist.size());
    }
    std::vector<uint64_t> all(lmax * size_t(W), 0);
    std::vector<int32_t> tot(lmax * size_t(W), -1);
    for (int q = 0; q < W; q++) {
      Rank &r = ranks[size_t(q)];
      r.base.assign(r.hist.size(), 0);
      for (size_t j = 0; j < r.hist.size(); j++) {
        const uint32_t item = uint32_t(r.hist[j] >> 32);
        int64_t lower = 0, sum = int64_t(uint32_t(r.hist[j]));
        for (int o = 0; o < W; o++) {
          if (o == q) continue;
          const int64_t h = find(ranks[size_t(o)].hist, item);
          if (o < q) lower += h;
          sum += h;
        }
        r.base[j] = int32_t(lower);
        all[size_t(q) * lmax + j] = r.hist[j];
        tot[size_t(q) * lmax + j] = lower > 0 ? -1 : int32_t(sum);
      }
    }
    std::vector<int32_t> su, ss, si;
    for (Rank &r : ranks) {
      Sampler::RankCut cut;
      cut.n_local = int64_t(r.hist.size());
      cut.local = r.hist.data();
      cut.base = r.base.data();
      cut.n_slots = int64_t(all.size());
      cut.all = all.data();
      cut.tot = tot.data();
      r.sm.window(int64_t(r.users.size()), r.users.data(), r.slots.data(), r.items.data(), &cut);
      for (size_t k = 0; k < r.users.size(); k++) {
        auto it = one_slot.find(r.users[k]);
        if (it == one_slot.end()) it = one_slot.emplace(r.users[k], int32_t(one_slot.size())).first;
        su.push_back(r.users[k]);
        ss.push_back(it->second);
        si.push_back(r.items[k]);
      }
    }
    for (int q = 0; q < W; q++)  // the feedbacks that arose on q, subtracted on every other rank
      for (int32_t item : ranks[size_t(q)].sm.feedback())
        for (int o = 0; o < W; o++)
          if (o != q) ranks[size_t(o)].sm.peer_feedback(item);
    one_trace.clear();
    one.window(int64_t(su.size()), su.data(), ss.data(), si.data());
    std::vector<int32_t> cat;
    for (Rank &r : ranks) cat.insert(cat.end(), r.trace.begin(), r.trace.end());
    CHECK(cat == one_trace);
    int64_t c1[6], sum[6] = {0, 0, 0, 0, 0, 0};
    one.counters(c1);
    for (Rank &r : ranks) {
      int64_t c[6];
      r.sm.counters(c);
      for (int k = 0; k < 5; k++) sum[k] += c[k];
      CHECK(c[5] == c1[5]);
      for (int32_t i = 0; i < n_items; i++) CHECK(r.sm.item_count(i) == one.item_count(i));
    }
    for (int k = 0; k < 5; k++) CHECK(sum[k] == c1[k]);
    for (const auto &kv : one_slot) {
      Rank &r = ranks[size_t(kv.first % W)];
      const int32_t slot = r.slot_of.at(kv.first);
      CHECK(r.sm.length(slot) == one.length(kv.second) && r.sm.total(slot) == one.total(kv.second));
    }
  }
  return 0;
}

int main() {
  const int32_t cuts[][2] = {{1, 1}, {2, 1}, {3, 2}, {5, 2}, {20, 4}, {500, 64}, {32767, 7}};
  uint64_t seed = 1;
  for (int W = 2; W <= 4; W++)
    for (const auto &c : cuts)
      for (int rep = 0; rep < 4; rep++)
        if (fuzz_one(seed++, W, rep % 2 ? 24 : 1000, c[0], c[1], 9, 300, rep < 2 ? 7 : 60)) return 1;
  puts("sample_comm_fuzz ok");
  return 0;
}
