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
class Comm;

// The item cut across ranks (include/cooc.h, sampled mode at world > 1): every rank's list of 8-byte words
// all-gathered (the lengths, then the lists padded to the longest), and the kernels that read the gathered lists.
// Two kinds of list go through it each window: the window's per-item histogram, (item << 32 | records) words
// sorted by item, and the items of the feedbacks that arose on the rank (one word each, any order).  Both
// samplers use it: the device sampler hands it device lists, the host sampler uploads its own and reads the
// results back.  Every rank calls gather() for every list of every window, with an empty list if it has none.
class ItemCutExchange {
 public:
  // n words at d_src (device; ignored when n == 0) from every rank.  Synchronises s (the lengths are read).
  Status gather(Comm &c, hipStream_t s, const uint64_t *d_src, int64_t n);
  Status gather_host(Comm &c, hipStream_t s, const uint64_t *h_src, int64_t n);  // the same from host memory
  int64_t lmax() const { return lmax_; }  // the longest list; 0: every rank's list is empty
  int64_t slots() const { return lmax_ * int64_t(lens_.size()); }
  int64_t words() const;  // the ranks' lengths summed
  const std::vector<int64_t> &lens() const { return lens_; }
  // after gather() of the histograms: base()[r] = the records of local run r's item on lower ranks, tot()[slot] =
  // the job's records of the slot's item where this slot is the lowest rank's that lists it, -1 elsewhere
  Status resolve(hipStream_t s);
  const int32_t *base() const { return base_.as<int32_t>(); }
  const int32_t *tot() const { return tot_.as<int32_t>(); }
  const uint64_t *all() const { return all_.as<uint64_t>(); }  // [world * lmax], rank q's list at q * lmax
  // count[i] += min(the job's records of i, max(0, item_cut - count[i])) for every item of the gathered union
  Status commit(hipStream_t s, int32_t *count, int32_t n_items, int32_t item_cut);
  // after gather() of the feedback lists: count[i] -= 1 per entry of every other rank
  Status subtract_peers(hipStream_t s, int32_t *count, int32_t n_items);
  // the gathered lists (and, after resolve(), the bases of the local runs and the totals) on the host
  Status read_back(hipStream_t s, std::vector<uint64_t> *all, std::vector<int32_t> *base, std::vector<int32_t> *tot);
  void release() { *this = ItemCutExchange(); }

 private:
  int32_t rank_ = 0;
  bool err_live_ = false;  // the err word holds a window's bits that no one has read yet
  int64_t lmax_ = 0, n_local_ = 0;
  std::vector<int64_t> lens_;
  DevBuf dlens_, send_, all_, base_, tot_, err_;
};

class SampleStream {
 public:
  Status enable(int32_t n_items, int32_t item_cut, int32_t user_cut, uint64_t seed, hipStream_t s);
  bool enabled() const { return item_cut_ > 0; }
  // One window: n records in arrival order as rec3 = n slots, then their n user ids, then their n items (host
  // memory; items in [0, n_items), slots in [0, n_slots)); n_distinct: an upper bound of the window's distinct
  // slots.  Steps 1-3 of the contract are applied to the device state; *changed = the users with a fill or a
  // replacement (any order), their lists in app() and rep().  Synchronises s.
  // comm (world > 1; NULL otherwise): the item cut over the ranks' records in rank order and the feedbacks of every
  // rank, exchanged through *icx; the call is a collective, made also with n == 0.
  Status window(hipStream_t s, int64_t n, const int32_t *rec3, int64_t n_slots, int64_t n_distinct,
                std::vector<SmChange> *changed, Comm *comm = nullptr, ItemCutExchange *icx = nullptr);
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
  DevBuf count_, len_, total_, ctr_, win_, rec_, out_, hist_, fb_;
  int32_t *app_ = nullptr, *rep_ = nullptr;
};

}  // namespace cooc
