// cooc_sample_stream.h — the sampled streaming mode decided on the device (cooc_sampling_enable_device): the
// carried state of cooc_sample_dev.hip's sample_window held for the life of a context, and one window of it in a
// decision-emitting form.  StreamState::finish_sampled runs it in place of the host sampler (cooc_sample.h).
#pragma once

#include <cstdint>
#include <vector>

#include "cooc_device.h"

namespace cooc {

// One user whose reservoir a window changed, as both samplers hand it to finish_sampled: fills appended items at
// app[app_begin ..), n_rep (slot, item) replacements at rep[2 rep_begin ..), both in arrival order; n_old_distinct =
// the distinct replaced slots below len_old (those existed before the window).  32 bytes.
struct SmChange {
  int32_t slot;     // the caller's dense index of the user
  int32_t len_old;  // |H_u| before the window, as the sampler holds it
  int32_t fills, n_rep, n_old_distinct, app_begin, rep_begin;
  int32_t pad;
};

constexpr int64_t kSstSlots0 = 1024;  // per-slot state (L, T) of a new context; doubled as slots appear

struct Snapshotter;  // cooc_snapshot_impl.h: a sampled context's checkpoint reads and writes the sampler's state

class SampleStream {
 public:
  Status enable(int32_t n_items, int32_t item_cut, int32_t user_cut, uint64_t seed, hipStream_t s);
  bool enabled() const { return item_cut_ > 0; }
  // One window: n records in arrival order as rec3 = n slots, then their n user ids, then their n items (host
  // memory; items in [0, n_items), slots in [0, n_slots)); n_distinct: an upper bound of the window's distinct
  // slots.  Steps 1-3 of the contract are applied to the device state; *changed = the users with a fill or a
  // replacement (any order), their lists in app() and rep().  Synchronises s.
  Status window(hipStream_t s, int64_t n, const int32_t *rec3, int64_t n_slots, int64_t n_distinct,
                std::vector<SmChange> *changed);
  const int32_t *app() const { return app_; }
  const int32_t *rep() const { return rep_; }
  // cooc_sampling_counters / cooc_copy_user_history's total: small synchronous copies, not on the window path
  Status counters(hipStream_t s, int64_t out[6]);
  Status total(hipStream_t s, int32_t slot, int32_t *total);
  void release();

 private:
  friend struct Snapshotter;
  Status grow_slots(int64_t n_slots, hipStream_t s);
  Status grow_window(int64_t m, hipStream_t s);

  int32_t n_items_ = 0, item_cut_ = 0, user_cut_ = 0;
  uint64_t seed_ = 0;
  int64_t slot_cap_ = 0, m_cap_ = 0;
  DevBuf count_, len_, total_, ctr_, win_, rec_, out_;
  int32_t *app_ = nullptr, *rep_ = nullptr;
};

}  // namespace cooc
