// cooc_sample.h — host side of the sampled streaming mode (cooc_sampling_enable): the item cut, the per-user
// reservoir decisions and the feedback of one window, record by record.  No HIP: cooc_sample.cpp also builds
// stand-alone under the host sanitizers (tests/sanitize/sample_fuzz.cpp).
//
// Restates ItemInteractionCounterTwoInputStreamOperator.java:119-143 (item cut), :94-116 (feedback) and
// UserInteractionCounterOneInputStreamOperator.java:145-257 (reservoir), with the reference's two races
// serialised as include/cooc.h states them: a counter-based draw and the feedback applied at the window's end.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cooc {

// (constexpr: the device sampler, cooc_sample_dev.hip, calls the same two functions from its kernels)
constexpr uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The reservoir slot drawn for user u's total-th interaction (total >= 1): uniform on [0, total) up to total / 2^32.
constexpr int64_t sample_draw(uint64_t seed, int32_t user, int32_t total) {
  const uint64_t key = (uint64_t(uint32_t(user)) << 32) | uint64_t(uint32_t(total));
  return int64_t(((splitmix64(seed ^ key) >> 32) * uint64_t(uint32_t(total))) >> 32);
}

struct Snapshotter;  // cooc_snapshot_impl.h: a sampled context's checkpoint reads and writes the samplers' state

class Sampler {
 public:
  // One user whose reservoir a window changed: the items appended (the fill branch) and the (slot, item)
  // replacements, both in arrival order.
  struct Changed {
    int32_t slot = 0;  // the caller's dense index of the user
    int32_t user = 0;
    std::vector<int32_t> appended;
    std::vector<int32_t> replaced;  // 2 per replacement: slot, item
  };

  void enable(int32_t n_items, int32_t item_cut, int32_t user_cut, uint64_t seed);
  bool enabled() const { return item_cut_ > 0; }
  int32_t item_cut() const { return item_cut_; }
  int32_t user_cut() const { return user_cut_; }
  uint64_t seed() const { return seed_; }
  // back to the state enable() left: no counter, no user, the decision counters 0 (the cuts and the seed stay)
  void reset();

  // World > 1 (include/cooc.h, the item cut across ranks): what the ranks' exchanged histograms say about this
  // rank's window.  The job's window is the ranks' records in rank order, so base[k] records of local item k stand
  // before this rank's; the item counters are replicated, so every item of the gathered union is committed from
  // the job's records of it (tot, at the one slot that owns the item; -1 elsewhere), also without a local record.
  struct RankCut {
    int64_t n_local = 0;            // this rank's distinct items of the window
    const uint64_t *local = nullptr;  // their (item << 32 | records) words, ascending item
    const int32_t *base = nullptr;    // [n_local] the item's records on lower ranks
    int64_t n_slots = 0;            // the gathered lists' slots
    const uint64_t *all = nullptr;  // [n_slots] (item << 32 | records), valid where tot >= 0
    const int32_t *tot = nullptr;   // [n_slots] the job's records of the item, -1: not the item's owner slot
  };

  // One window: n records in arrival order (user id, the caller's dense index of that user, item in
  // [0, n_items)).  Afterwards changed()[0, n_changed()) are the users with a changed slot, in the order of
  // their first change.  cut (world > 1): the record of item i with rank rho among this rank's records of i is
  // sampled iff count[i] + base + rho < item_cut, and the counters are committed from the totals; the feedbacks
  // that arose here are applied and left in feedback() for the peers, theirs arrive through peer_feedback().
  void window(int64_t n, const int32_t *users, const int32_t *slots, const int32_t *items,
              const RankCut *cut = nullptr);
  const std::vector<int32_t> &feedback() const { return feedback_; }  // the last window's, one item per feedback
  void peer_feedback(int32_t item) { item_count_[item]--; }
  int32_t n_changed() const { return n_changed_; }
  const Changed &changed(int32_t j) const { return changed_[j]; }

  int32_t length(int32_t slot) const { return std::size_t(slot) < len_.size() ? len_[slot] : 0; }
  int32_t total(int32_t slot) const { return std::size_t(slot) < total_.size() ? total_[slot] : 0; }
  int16_t item_count(int32_t item) const { return item_count_[item]; }
  // [0] records rejected by the item cut, [1] fills, [2] replacements, [3] feedback decrements, [4] users with
  // a reservoir, [5] sum of the item counters
  void counters(int64_t out[6]) const;
  // Tests: every record's decision is appended to *trace (kRejected, kFill, kFeedback, or the replaced slot).
  static constexpr int32_t kRejected = -1, kFill = -2, kFeedback = -3;
  void set_trace(std::vector<int32_t> *trace) { trace_ = trace; }

 private:
  friend struct Snapshotter;
  int32_t item_cut_ = 0, user_cut_ = 0;
  uint64_t seed_ = 0;
  std::vector<int16_t> item_count_;     // itemInteractions (a Java short)
  std::vector<int32_t> len_, total_;    // per user index: |H_u| and userInteractionsTotal
  std::vector<int64_t> stamp_;          // per user index: window_seq_ when in changed_
  std::vector<int32_t> pos_;            // per user index: its entry of changed_
  std::vector<Changed> changed_;        // reused across windows
  std::vector<int32_t> feedback_;       // items of the window's rejected samples
  std::vector<int32_t> rho_;            // world > 1: per local item, its records seen so far in the window
  std::vector<int32_t> *trace_ = nullptr;
  int32_t n_changed_ = 0;
  int64_t window_seq_ = 0;
  int64_t rejected_ = 0, fills_ = 0, replacements_ = 0, feedbacks_ = 0, n_users_ = 0;
};

}  // namespace cooc
