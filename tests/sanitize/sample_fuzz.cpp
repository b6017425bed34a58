// sample_fuzz.cpp — stand-alone driver of the sampled mode's host side (cooc_sample.cpp), built with
// -fsanitize=address,undefined by tests/test_sampled_cpu.py.
//
//   sample_fuzz                  random logs: every draw k < total, item counters in [0, item_cut], |H| <= user_cut,
//                                replaced slots inside the reservoir, the counters' balance
//   sample_fuzz LOG ic uc seed n_items   the decisions of a log ("u i" per record, "w" ends a window), one line
//                                per record: r (rejected), f (fill), k<slot> (replacement), b (feedback)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_map>
#include <vector>

#include "../../flink-cooccurrence_amd/csrc/cooc_sample.h"

using cooc::Sampler;

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      fprintf(stderr, "sample_fuzz: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static int fuzz_one(uint64_t seed, int32_t n_items, int32_t item_cut, int32_t user_cut, int n_windows, int n_rec,
                    int n_users) {
  std::mt19937_64 rng(seed);
  Sampler sm;
  sm.enable(n_items, item_cut, user_cut, seed * 0x9E37u);
  std::unordered_map<int32_t, int32_t> slot_of;
  std::vector<int32_t> users, slots, items, trace, user_of_slot;
  std::vector<std::vector<int32_t>> H;
  sm.set_trace(&trace);
  int64_t n_total = 0;
  for (int w = 0; w < n_windows; w++) {
    users.clear();
    slots.clear();
    items.clear();
    trace.clear();
    for (int r = 0; r < n_rec; r++) {
      // (negative and large ids too: the key of the draw takes the id's 32 bits)
      int32_t u = int32_t(rng() % uint64_t(n_users));
      if (u % 7 == 3) u = -u - 1;
      if (u % 11 == 5) u += 1 << 30;
      auto it = slot_of.find(u);
      if (it == slot_of.end()) {
        it = slot_of.emplace(u, int32_t(slot_of.size())).first;
        H.emplace_back();
        user_of_slot.push_back(u);
      }
      users.push_back(u);
      slots.push_back(it->second);
      const uint64_t z = rng() % 100;
      items.push_back(int32_t(z < 60 ? rng() % 3 : rng() % uint64_t(n_items)));  // a hot head reaches the item cut
    }
    sm.window(n_rec, users.data(), slots.data(), items.data());
    n_total += n_rec;
    CHECK(int(trace.size()) == n_rec);
    for (int32_t j = 0; j < sm.n_changed(); j++) {
      const Sampler::Changed &c = sm.changed(j);
      CHECK(c.slot >= 0 && size_t(c.slot) < H.size() && user_of_slot[c.slot] == c.user);
      CHECK(!c.appended.empty() || !c.replaced.empty());
      CHECK(c.replaced.size() % 2 == 0);
      std::vector<int32_t> &h = H[c.slot];
      h.insert(h.end(), c.appended.begin(), c.appended.end());
      CHECK(int32_t(h.size()) <= user_cut);
      for (size_t r = 0; r < c.replaced.size(); r += 2) {
        CHECK(c.replaced[r] >= 0 && c.replaced[r] < int32_t(h.size()) && int32_t(h.size()) == user_cut);
        CHECK(c.replaced[r + 1] >= 0 && c.replaced[r + 1] < n_items);
        h[size_t(c.replaced[r])] = c.replaced[r + 1];
      }
      CHECK(sm.length(c.slot) == int32_t(h.size()));
    }
    for (int r = 0; r < n_rec; r++) {
      const int32_t t = sm.total(slots[size_t(r)]);
      CHECK(t >= 1);
      if (trace[size_t(r)] >= 0) CHECK(trace[size_t(r)] < user_cut);
    }
    for (int32_t i = 0; i < n_items; i++) CHECK(sm.item_count(i) >= 0 && sm.item_count(i) <= item_cut);
    int64_t c6[6];
    sm.counters(c6);
    CHECK(c6[0] + c6[1] + c6[2] + c6[3] == n_total);  // every record takes exactly one branch
    CHECK(c6[5] == c6[1] + c6[2]);                    // sampled records that stayed: fills + replacements
    int64_t with = 0, len_sum = 0;
    for (const auto &h : H) {
      with += !h.empty();
      len_sum += int64_t(h.size());
    }
    CHECK(c6[4] == with && len_sum == c6[1]);
  }
  return 0;
}

static int fuzz_draws() {
  std::mt19937_64 rng(99);
  for (int i = 0; i < 2000000; i++) {
    const int32_t total = int32_t(1 + rng() % (i % 3 == 0 ? 0x7fffffffull : 70000ull));
    const int64_t k = cooc::sample_draw(rng(), int32_t(uint32_t(rng())), total);
    CHECK(k >= 0 && k < total);
  }
  CHECK(cooc::sample_draw(0, 0, 1) == 0);
  CHECK(cooc::sample_draw(~0ull, -1, 0x7fffffff) < 0x7fffffff);
  return 0;
}

static int decisions(const char *path, int32_t item_cut, int32_t user_cut, uint64_t seed, int32_t n_items) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "sample_fuzz: cannot open %s\n", path);
    return 2;
  }
  Sampler sm;
  sm.enable(n_items, item_cut, user_cut, seed);
  std::unordered_map<int32_t, int32_t> slot_of;
  std::vector<int32_t> users, slots, items, trace;
  sm.set_trace(&trace);
  char line[128];
  while (fgets(line, sizeof(line), f)) {
    if (line[0] == 'w') {
      trace.clear();
      sm.window(int64_t(users.size()), users.data(), slots.data(), items.data());
      for (int32_t t : trace) {
        if (t == Sampler::kRejected) puts("r");
        else if (t == Sampler::kFill) puts("f");
        else if (t == Sampler::kFeedback) puts("b");
        else printf("k%d\n", t);
      }
      puts("w");
      users.clear();
      slots.clear();
      items.clear();
      continue;
    }
    int u = 0, i = 0;
    if (sscanf(line, "%d %d", &u, &i) != 2 || i < 0 || i >= n_items) {
      fclose(f);
      fprintf(stderr, "sample_fuzz: bad line %s", line);
      return 2;
    }
    auto it = slot_of.find(u);
    if (it == slot_of.end()) it = slot_of.emplace(u, int32_t(slot_of.size())).first;
    users.push_back(u);
    slots.push_back(it->second);
    items.push_back(i);
  }
  fclose(f);
  int64_t c6[6];
  sm.counters(c6);
  printf("counters %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", c6[0], c6[1], c6[2],
         c6[3], c6[4], c6[5]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 6)
    return decisions(argv[1], int32_t(atoi(argv[2])), int32_t(atoi(argv[3])), strtoull(argv[4], nullptr, 0),
                     int32_t(atoi(argv[5])));
  if (fuzz_draws()) return 1;
  const int32_t cuts[][2] = {{1, 1}, {2, 1}, {3, 2}, {20, 4}, {500, 64}, {32767, 7}, {5, 32767}};
  uint64_t seed = 1;
  for (const auto &c : cuts)
    for (int rep = 0; rep < 6; rep++)
      if (fuzz_one(seed++, rep % 2 ? 24 : 1000, c[0], c[1], 12, 400, rep < 3 ? 5 : 60)) return 1;
  puts("sample_fuzz ok");
  return 0;
}
