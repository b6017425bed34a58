// cooc_sample.cpp — the sampled mode's per-record decisions on the host (cooc_sample.h).  O(records) per window,
// as the fill path's staging (StreamState::submit); the pair work stays on the device.
#include "cooc_sample.h"

#include <algorithm>

namespace cooc {

void Sampler::enable(int32_t n_items, int32_t item_cut, int32_t user_cut, uint64_t seed) {
  item_cut_ = item_cut;
  user_cut_ = user_cut;
  seed_ = seed;
  item_count_.assign(size_t(std::max(n_items, 0)), 0);
}

void Sampler::reset() {
  std::fill(item_count_.begin(), item_count_.end(), int16_t(0));
  len_.clear();
  total_.clear();
  stamp_.clear();
  pos_.clear();
  feedback_.clear();
  n_changed_ = 0;
  window_seq_ = 0;
  rejected_ = fills_ = replacements_ = feedbacks_ = n_users_ = 0;
}

void Sampler::window(int64_t n, const int32_t *users, const int32_t *slots, const int32_t *items,
                     const RankCut *cut) {
  n_changed_ = 0;
  feedback_.clear();
  if (cut) rho_.assign(size_t(cut->n_local), 0);
  auto entry = [&](int32_t slot, int32_t user) -> Changed & {
    if (stamp_[slot] != window_seq_) {
      stamp_[slot] = window_seq_;
      pos_[slot] = n_changed_;
      if (int32_t(changed_.size()) <= n_changed_) changed_.emplace_back();
      Changed &c = changed_[n_changed_++];
      c.slot = slot;
      c.user = user;
      c.appended.clear();
      c.replaced.clear();
      return c;
    }
    return changed_[pos_[slot]];
  };
  for (int64_t r = 0; r < n; r++) {
    const int32_t u = users[r], slot = slots[r], item = items[r];
    if (size_t(slot) >= len_.size()) {
      const size_t grown = std::max<size_t>(size_t(slot) + 1, len_.size() * 2);
      len_.resize(grown, 0);
      total_.resize(grown, 0);
      stamp_.resize(grown, -1);
      pos_.resize(grown, 0);
    }
    // 1. item cut (ItemInteractionCounter...java:119-143)
    bool sample;
    if (!cut) {
      sample = item_count_[item] < item_cut_;
      if (sample) item_count_[item]++;
    } else {  // the counter stays at the window's start until the commit below
      const uint64_t *w = std::lower_bound(cut->local, cut->local + cut->n_local, uint64_t(uint32_t(item)) << 32);
      const size_t k = size_t(w - cut->local);
      sample = k < size_t(cut->n_local) && int32_t(*w >> 32) == item &&
               int64_t(item_count_[item]) + cut->base[k] + rho_[k]++ < item_cut_;
    }
    if (!sample) rejected_++;
    // 2. user stage (UserInteractionCounter...java:145-257)
    total_[slot]++;
    if (!sample) {
      if (trace_) trace_->push_back(kRejected);
      continue;
    }
    if (len_[slot] < user_cut_) {  // the fill branch, :168-205
      if (len_[slot]++ == 0) n_users_++;
      entry(slot, u).appended.push_back(item);
      fills_++;
      if (trace_) trace_->push_back(kFill);
      continue;
    }
    const int64_t k = sample_draw(seed_, u, total_[slot]);
    if (k < user_cut_) {  // :206-240: slot k is replaced
      Changed &c = entry(slot, u);
      c.replaced.push_back(int32_t(k));
      c.replaced.push_back(item);
      replacements_++;
      if (trace_) trace_->push_back(int32_t(k));
    } else {
      feedback_.push_back(item);  // the rejected sample goes back to its item counter
      if (trace_) trace_->push_back(kFeedback);
    }
  }
  if (cut)  // the job's sampled records of every item of the union
    for (int64_t k = 0; k < cut->n_slots; k++) {
      if (cut->tot[k] < 0) continue;
      int16_t &c = item_count_[size_t(cut->all[k] >> 32)];
      const int32_t room = item_cut_ - c;
      if (room > 0) c = int16_t(c + std::min(cut->tot[k], room));
    }
  // 3. feedback (ItemInteractionCounter...java:94-116), at the end of the window it arose in
  for (int32_t item : feedback_) item_count_[item]--;
  feedbacks_ += int64_t(feedback_.size());
  window_seq_++;
}

void Sampler::counters(int64_t out[6]) const {
  out[0] = rejected_;
  out[1] = fills_;
  out[2] = replacements_;
  out[3] = feedbacks_;
  out[4] = n_users_;
  int64_t sum = 0;
  for (int16_t c : item_count_) sum += c;
  out[5] = sum;
}

}  // namespace cooc
