// snapshot_parts_fuzz.cpp — the host-only checks across the parts of one checkpoint (snap_check_parts, the second
// step of cooc_restore_finish_parts) under AddressSanitizer + UndefinedBehaviorSanitizer.
// tests/test_snapshot_parts_cpu.py builds this with g++ -fsanitize=address,undefined against
// flink-cooccurrence_amd/csrc/cooc_snapshot.cpp (host-only: no HIP) and runs it.
//
// Consistent sets of part heads (rank i of W, one configuration, equal job-wide totals, one watermark that is also
// the agreed one, nothing pending at or below it, as many row sums of other ranks as the other parts have rows)
// must pass and give the summed accumulators; every single-field disagreement, permuted and duplicated ranks,
// n_parts of 0 and below, and random heads must be COOC_ERR_ARG.  Every set is handed over in a heap buffer of
// exactly n_parts heads, so a read past the end aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../flink-cooccurrence_amd/csrc/cooc_snapshot.h"

namespace {

using cooc::SnapPartHead;
constexpr int32_t kItems = 1000, kCut = 7;
constexpr int64_t kWindow = 1000;
int g_checks = 0;

#define REQUIRE(c)                                                  \
  do {                                                              \
    g_checks++;                                                     \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      return 1;                                                     \
    }                                                               \
  } while (0)

std::vector<SnapPartHead> consistent(int64_t W, std::mt19937_64 &rng) {
  std::vector<SnapPartHead> v(static_cast<size_t>(W));
  const int64_t wm = int64_t(rng() % 1000000) - 500000;
  const int64_t ref = int64_t(rng() % 100000), s2 = int64_t(rng() % 100000), s3 = int64_t(rng() % 100000);
  int64_t rows = 0;
  for (int64_t i = 0; i < W; i++) {
    SnapPartHead &p = v[size_t(i)];
    std::memset(&p, 0, sizeof(p));
    p.h.n_items = kItems;
    p.h.user_cut = kCut;
    p.h.window_size_ms = kWindow;
    p.h.rank = int32_t(i);
    p.h.world = int32_t(W);
    p.h.sec[cooc::kSnapRowIds - 1].count = int64_t(rng() % 3);
    rows += p.h.sec[cooc::kSnapRowIds - 1].count;
    p.scalars[cooc::kScObservedExact] = int64_t(rng() % 1000);
    p.scalars[cooc::kScRowsumAcc] = int64_t(rng() % 1000);
    p.scalars[cooc::kScRescoredItems] = int64_t(rng() % 1000);
    p.scalars[cooc::kScLateElements] = int64_t(rng() % 1000);
    p.scalars[cooc::kScObservedRef] = ref;
    p.scalars[cooc::kScScal2] = s2;
    p.scalars[cooc::kScScal3] = s3;
    p.scalars[cooc::kScWatermark] = wm;
    p.scalars[cooc::kScAgreed] = W > 1 ? wm : INT64_MIN;
    p.first_pending = (rng() & 1) ? INT64_MAX : wm + 1 + int64_t(rng() % 5000);
  }
  for (auto &p : v) p.h.sec[cooc::kSnapXsumIds - 1].count = rows - p.h.sec[cooc::kSnapRowIds - 1].count;
  return v;
}

int check(const std::vector<SnapPartHead> &v, int64_t *merged = nullptr) {
  // an exact-size heap copy: a read past the last head is a heap-buffer-overflow
  SnapPartHead *heap = v.empty() ? nullptr : new SnapPartHead[v.size()];
  for (size_t i = 0; i < v.size(); i++) heap[i] = v[i];
  int64_t m[cooc::kSnapScalarWords];
  std::string why;
  const int r = cooc::snap_check_parts(heap, int64_t(v.size()), kItems, kWindow, kCut, merged ? merged : m, &why);
  delete[] heap;
  if (r != COOC_OK && why.empty()) return -1;  // a refusal says why
  return r;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  // ---- consistent sets pass, and the merged scalars are the rule's
  for (int64_t W : {int64_t(1), int64_t(2), int64_t(3), int64_t(8), int64_t(5000)}) {
    for (int rep = 0; rep < (W > 100 ? 2 : 50); rep++) {
      const std::vector<SnapPartHead> v = consistent(W, rng);
      int64_t m[cooc::kSnapScalarWords];
      REQUIRE(check(v, m) == COOC_OK);
      for (int k : {int(cooc::kScObservedExact), int(cooc::kScRowsumAcc), int(cooc::kScRescoredItems), int(cooc::kScLateElements)}) {
        int64_t sum = 0;
        for (const auto &p : v) sum += p.scalars[k];
        REQUIRE(m[k] == sum);
      }
      REQUIRE(m[cooc::kScObservedRef] == v[0].scalars[cooc::kScObservedRef] && m[cooc::kScScal2] == v[0].scalars[cooc::kScScal2]);
      REQUIRE(m[cooc::kScScal3] == v[0].scalars[cooc::kScScal3] && m[cooc::kScWatermark] == v[0].scalars[cooc::kScWatermark]);
      REQUIRE(m[cooc::kScAgreed] == m[cooc::kScWatermark] && m[cooc::kScRegather] == 0);
    }
  }
  // ---- n_parts of 0 (and a NULL array), below 0, NULL outputs
  {
    int64_t m[cooc::kSnapScalarWords];
    std::string why;
    REQUIRE(check({}) == COOC_ERR_ARG);
    const std::vector<SnapPartHead> v = consistent(2, rng);
    REQUIRE(cooc::snap_check_parts(v.data(), 0, kItems, kWindow, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), -1, kItems, kWindow, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), int64_t(1) << 40, kItems, kWindow, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(nullptr, 2, kItems, kWindow, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), 2, kItems, kWindow, kCut, nullptr, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), 2, kItems, kWindow, kCut, m, nullptr) == COOC_OK);
    // the context's configuration, not only the parts' agreement
    REQUIRE(cooc::snap_check_parts(v.data(), 2, kItems + 1, kWindow, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), 2, kItems, kWindow + 1, kCut, m, &why) == COOC_ERR_ARG);
    REQUIRE(cooc::snap_check_parts(v.data(), 2, kItems, kWindow, kCut + 1, m, nullptr) == COOC_ERR_ARG);
  }
  // ---- every single-field disagreement, in every part of sets of 2, 3 and 8
  using Edit = std::function<void(SnapPartHead &)>;
  const std::vector<Edit> edits = {
      [](SnapPartHead &p) { p.h.n_items++; },
      [](SnapPartHead &p) { p.h.user_cut++; },
      [](SnapPartHead &p) { p.h.window_size_ms++; },
      [](SnapPartHead &p) { p.h.world++; },
      [](SnapPartHead &p) { p.h.world = 1; },
      [](SnapPartHead &p) { p.h.rank++; },
      [](SnapPartHead &p) { p.h.rank = p.h.rank ? 0 : 1; },  // a rank twice
      [](SnapPartHead &p) { p.scalars[cooc::kScObservedRef]++; },
      [](SnapPartHead &p) { p.scalars[cooc::kScScal2]--; },
      [](SnapPartHead &p) { p.scalars[cooc::kScScal3]++; },
      [](SnapPartHead &p) { p.scalars[cooc::kScRegather] = 1; },
      [](SnapPartHead &p) { p.scalars[cooc::kScWatermark]++; p.scalars[cooc::kScAgreed]++; },
      [](SnapPartHead &p) { p.scalars[cooc::kScAgreed]--; },
      [](SnapPartHead &p) { p.first_pending = p.scalars[cooc::kScWatermark]; },
      [](SnapPartHead &p) { p.first_pending = p.scalars[cooc::kScWatermark] - 1; },
      [](SnapPartHead &p) { p.first_pending = INT64_MIN; },
      [](SnapPartHead &p) { p.h.sec[cooc::kSnapXsumIds - 1].count++; },
      [](SnapPartHead &p) { p.h.sec[cooc::kSnapRowIds - 1].count++; },
      [](SnapPartHead &p) { p.scalars[cooc::kScObservedExact] = INT64_MAX; },  // the sum overflows (below)
  };
  for (int64_t W : {int64_t(2), int64_t(3), int64_t(8)}) {
    for (size_t e = 0; e < edits.size(); e++) {
      for (int64_t i = 0; i < W; i++) {
        std::vector<SnapPartHead> v = consistent(W, rng);
        for (auto &p : v) p.scalars[cooc::kScObservedExact] += 1;  // (so that INT64_MAX in one part overflows the sum)
        REQUIRE(check(v) == COOC_OK);
        edits[e](v[size_t(i)]);
        REQUIRE(check(v) == COOC_ERR_ARG);
      }
    }
  }
  // one part: no agreement to check, everything else still holds
  {
    std::vector<SnapPartHead> v = consistent(1, rng);
    v[0].scalars[cooc::kScAgreed] = v[0].scalars[cooc::kScWatermark] - 5;
    REQUIRE(check(v) == COOC_OK);
    v[0].scalars[cooc::kScRegather] = 1;
    REQUIRE(check(v) == COOC_ERR_ARG);
    v = consistent(1, rng);
    v[0].h.world = 2;
    REQUIRE(check(v) == COOC_ERR_ARG);
    v = consistent(1, rng);
    v[0].h.sec[cooc::kSnapXsumIds - 1].count = 1;
    REQUIRE(check(v) == COOC_ERR_ARG);
  }
  // ---- permuted ranks: every swap of two parts, a rotation, a reversal
  for (int64_t W : {int64_t(2), int64_t(3), int64_t(5)}) {
    const std::vector<SnapPartHead> good = consistent(W, rng);
    for (int64_t a = 0; a < W; a++)
      for (int64_t b = a + 1; b < W; b++) {
        std::vector<SnapPartHead> v = good;
        std::swap(v[size_t(a)], v[size_t(b)]);
        REQUIRE(check(v) == COOC_ERR_ARG);
        v = good;
        v[size_t(b)] = v[size_t(a)];  // a part twice
        REQUIRE(check(v) == COOC_ERR_ARG);
      }
    std::vector<SnapPartHead> v(good.rbegin(), good.rend());
    REQUIRE(check(v) == COOC_ERR_ARG);
    v = good;
    v.pop_back();  // a part missing
    REQUIRE(check(v) == COOC_ERR_ARG);
    v = good;
    v.push_back(good.back());  // one too many
    REQUIRE(check(v) == COOC_ERR_ARG);
  }
  // ---- random heads
  for (int rep = 0; rep < 20000; rep++) {
    std::vector<SnapPartHead> v(size_t(1 + rng() % 4));
    for (auto &p : v) {
      uint64_t w[sizeof(SnapPartHead) / 8];
      for (auto &x : w) x = rng();
      std::memcpy(&p, w, sizeof(p));
      if (rep & 1) {  // the configuration right, so that the later checks see the random fields
        p.h.n_items = kItems;
        p.h.user_cut = kCut;
        p.h.window_size_ms = kWindow;
        p.h.world = int32_t(v.size());
        p.h.rank = int32_t(&p - v.data());
      }
    }
    REQUIRE(check(v) == COOC_ERR_ARG);
  }
  std::printf("snapshot_parts_fuzz ok (%d checks)\n", g_checks);
  return 0;
}
