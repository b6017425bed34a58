// cooc_stream.cpp — host side of the resident streaming state and of the operator mirror.
//
// StreamState restates, per tumbling window, NonSampledUserInteractionCounterOneInputStreamOperator
// .onEventTime (:113-165: expand every buffered interaction against the user's history, then
// append it), the two window aggregators (ItemRowAggregator.java:26-56, RowSumAggregator.java:
// 25-71) and ItemRowRescorerTwoInputStreamOperator.processWatermark (:116-241).  The expansion and
// reductions run on the device (cooc_count.hip); this file only keeps per-user metadata, stages
// the window's interactions and moves results.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cooc_ctx.h"
#include "cooc_rescore.h"
#include "cooc_stream_kernels.h"
#include "cooc_window.h"

namespace cooc {

namespace {

// (window_max_ts, the TumblingEventTimeWindows assignment: cooc_window.h, shared with the device log preparation)

template <class T>
Status upload(DevBuf &b, const std::vector<T> &v, hipStream_t s) {
  COOC_TRY(b.reserve(sizeof(T) * (v.size() + 1)));
  if (!v.empty()) COOC_HIP_TRY(hipMemcpyAsync(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s));
  return Status::Ok();
}

// COOC_TRACE=1: per-window phase times on stderr (host wall; device phases end at a sync).
struct PhaseTrace {
  bool on = getenv("COOC_TRACE") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  char buf[512];
  int len = 0;
  void mark(const char *name, hipStream_t s = nullptr) {
    if (!on) return;
    if (s) (void)hipStreamSynchronize(s);
    const auto now = std::chrono::steady_clock::now();
    len += snprintf(buf + len, sizeof(buf) - len, " %s=%.3f", name,
                    std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
  void done(int64_t ts) {
    if (on)
      fprintf(stderr, "[cooc] window %lld:%s total=%.3f ms\n", (long long)ts, buf,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// The counter's totals of its last run, its error bits decoded (the stream must have drained).
Status counter_totals(cooc_ctx &ctx, PlanTotals *t) {
  COOC_TRY(ctx.counter.read_totals(t));
  if (t->err & 8) return Status{COOC_ERR_STATE, "internal bounds check failed"};
  if (t->err & 2) return Status{COOC_ERR_OVERFLOW, "a co-occurrence count exceeded uint32"};
  if (t->err & 4) return Status{COOC_ERR_OOM, "the sparse output region is exhausted"};
  return Status::Ok();
}

// The first of the n item ids outside [0, M), or NULL (no Status is built per call: submit asks once per user).
const int32_t *bad_item(const int32_t *items, int64_t n, int32_t M) {
  for (int64_t i = 0; i < n; i++)
    if (items[i] < 0 || items[i] >= M) return items + i;
  return nullptr;
}

Status item_error(int32_t item) {
  return Status{COOC_ERR_ARG, "item id " + std::to_string(item) + " outside [0, n_items)"};
}

}  // namespace

// Frees all device memory of the state (Snapshotter::wipe after a refused restore); the host vectors and the
// samplers' enabled state stay.
void StreamState::release() {
  w_ = Scratch();
  d_scan_tmp_.release();
  arena_.release();
  d_global_.release();
  d_grs_.release();
  d_scal_.release();
  gs_.release();
  dev_sampler_.release();
  icx_.release();
  global_ready_ = false;
  sparse_global_ = false;
}

Status StreamState::window_open(int64_t ts) const {
  if (staged_ && ts != staged_ts_)
    return Status{COOC_ERR_STATE, "window " + std::to_string(staged_ts_) + " is staged; finish it before submitting " +
                                      std::to_string(ts)};
  return Status::Ok();
}

// Keyed user state lookup (userHistoryState, NonSampled...java:129-132): a dense table for
// non-negative ids below 2^26, a hash map otherwise.
int32_t StreamState::slot_for(int32_t uid) {
  int32_t slot = -1;
  if (uid >= 0 && uid < (1 << 26)) {
    if (size_t(uid) >= dense_slot_.size()) dense_slot_.resize(std::max<size_t>(size_t(uid) + 1, dense_slot_.size() * 2), -1);
    slot = dense_slot_[uid];
  } else {
    auto it = slot_of_.find(uid);
    if (it != slot_of_.end()) slot = it->second;
  }
  if (slot >= 0) return slot;
  slot = int32_t(h_off_.size());  // userHistoryState.value() == null -> new IntArrayList(), :130-132
  if (uid >= 0 && uid < (1 << 26)) dense_slot_[uid] = slot;
  else slot_of_.emplace(uid, slot);
  h_off_.push_back(0);
  h_len_.push_back(0);
  h_cap_.push_back(0);
  staged_stamp_.push_back(-1);
  staged_pos_.push_back(0);
  return slot;
}

Status StreamState::submit(cooc_ctx &ctx, int64_t ts, int32_t n_users, const int32_t *user_ids,
                           const int64_t *user_ptr, const int32_t *items) {
  COOC_TRY(window_open(ts));
  for (int32_t u = 0; u < n_users; u++) {
    if (user_ptr[u + 1] < user_ptr[u]) return Status{COOC_ERR_ARG, "user_ptr must be non-decreasing"};
    if (const int32_t *bad = bad_item(items + user_ptr[u], user_ptr[u + 1] - user_ptr[u], ctx.cfg.n_items))
      return item_error(*bad);
  }
  if (sampled()) {  // the CSR order (user after user, item after item) is the arrival order
    for (int32_t u = 0; u < n_users; u++)
      for (int64_t i = user_ptr[u]; i < user_ptr[u + 1]; i++) {
        rec_users_.push_back(user_ids[u]);
        rec_items_.push_back(items[i]);
      }
    staged_ = true;
    staged_ts_ = ts;
    return Status::Ok();
  }
  const int64_t cut = ctx.cfg.user_cut;
  for (int32_t u = 0; u < n_users; u++) {
    const int32_t slot = slot_for(user_ids[u]);
    const bool staged = staged_stamp_[slot] == window_seq_;
    int64_t take = user_ptr[u + 1] - user_ptr[u];
    if (cut > 0) {
      // kMax: `userInteractions < userCut` (UserInteractionCounter...java:168) -- every accepted
      // interaction appends once to the history, so the accepted count is the history length
      const int64_t seen = int64_t(h_len_[slot]) + (staged ? int64_t(staged_items_[staged_pos_[slot]].size()) : 0);
      take = std::max<int64_t>(0, std::min<int64_t>(take, cut - seen));
      if (take == 0) continue;  // nothing of this user enters the window
    }
    int32_t j;
    if (!staged) {  // first appearance of this user in the window
      staged_stamp_[slot] = window_seq_;
      j = n_staged_++;
      staged_pos_[slot] = j;
      if (int32_t(staged_slots_.size()) < n_staged_) {
        staged_slots_.push_back(slot);
        staged_items_.emplace_back();
      } else {
        staged_slots_[j] = slot;
        staged_items_[j].clear();  // keeps the capacity of earlier windows
      }
    } else {
      j = staged_pos_[slot];
    }
    auto &dst = staged_items_[j];
    dst.insert(dst.end(), items + user_ptr[u], items + user_ptr[u] + take);
  }
  staged_ = true;
  staged_ts_ = ts;
  return Status::Ok();
}

Status StreamState::grow_arena(cooc_ctx &ctx, int64_t need) {
  if (int64_t(arena_.cap / sizeof(int32_t)) >= need) return Status::Ok();
  DevBuf bigger;
  COOC_TRY(bigger.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(need, 2 * int64_t(arena_.cap / 4)))));
  if (arena_.p && arena_used_ > 0) {
    // arena_used_ already includes the new reservations; copy the whole old capacity
    COOC_HIP_TRY(hipMemcpyAsync(bigger.p, arena_.p, arena_.cap, hipMemcpyDeviceToDevice, ctx.stream));
    COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  }
  arena_ = std::move(bigger);
  return Status::Ok();
}

Status StreamState::ensure_global(cooc_ctx &ctx) {
  if (global_ready_) return Status::Ok();
  const int64_t M = ctx.cfg.n_items;
  auto zeroed = [&](DevBuf &b, size_t bytes) -> Status {
    COOC_TRY(b.reserve(bytes));
    COOC_HIP_TRY(hipMemsetAsync(b.p, 0, bytes, ctx.stream));
    return Status::Ok();
  };
  if (!ctx.counter.batch_ok()) {  // large universe: sorted row slabs, grown per window
    sparse_global_ = true;
    COOC_TRY(zeroed(gs_.base, sizeof(int64_t) * size_t(M)));
    COOC_TRY(zeroed(gs_.len, sizeof(int32_t) * size_t(M)));
    gs_.cap = gs_.bump = gs_.live = gs_.compactions = 0;
  } else {
    const size_t g_bytes = sizeof(uint32_t) * size_t(M) * size_t(M);
    size_t free_b = 0, total_b = 0;
    COOC_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (g_bytes > free_b / 10 * 8)
      return Status{COOC_ERR_OOM, "dense global rows need " + std::to_string(g_bytes) +
                                      " B of HBM (n_items^2 x 4); sparse global rows are not built yet"};
    COOC_TRY(zeroed(d_global_, g_bytes));
  }
  COOC_TRY(zeroed(d_grs_, sizeof(int64_t) * M));
  COOC_TRY(zeroed(d_scal_, sizeof(int64_t) * 8));
  global_ready_ = true;
  return Status::Ok();
}

void StreamState::reserve_history(int32_t slot, int64_t need, std::vector<int64_t> *reloc) {
  if (need <= h_cap_[slot]) return;
  const int64_t old = h_len_[slot];
  const int64_t cap = std::max<int64_t>(16, std::max<int64_t>(2 * int64_t(h_cap_[slot]), need));
  const int64_t off = arena_used_;
  arena_used_ += cap;
  if (old > 0) {
    reloc->push_back(h_off_[slot]);
    reloc->push_back(off);
    reloc->push_back(old);
  }
  h_off_[slot] = off;
  h_cap_[slot] = int32_t(std::min<int64_t>(cap, INT32_MAX));
}

// The book-keeping of every finished window.
void StreamState::close_window(cooc_window_info *info) {
  staged_ = false;
  n_staged_ = 0;
  window_seq_++;
  have_window_ = true;
  *info = last_;
}

void StreamState::close_empty_window(cooc_ctx &ctx, int64_t ts, cooc_window_info *info) {
  delta_ = WindowDelta();
  std::memset(&last_, 0, sizeof(last_));
  last_.ts = ts;
  last_.topk = ctx.cfg.topk;
  n_touched_ = 0;
  close_window(info);
}

Status StreamState::finish(cooc_ctx &ctx, int64_t ts, cooc_window_info *info) {
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  if (staged_ && ts != staged_ts_)
    return Status{COOC_ERR_STATE, "finish_window(" + std::to_string(ts) + ") but window " +
                                      std::to_string(staged_ts_) + " is staged"};
  if (sampled()) return finish_sampled(ctx, ts, info);
  ctx.snapshot_release();  // a snapshot image describes the state before this window
  hipStream_t s = ctx.stream;
  const int64_t n_act = n_staged_;
  PhaseTrace tr;
  delta_packed_ = false;  // the packed copy-out view belongs to the previous window
  // p > 1 subtasks: every subtask takes part in every window's exchange, also with no user of its own
  const bool multi = ctx.comm && ctx.comm->world() > 1;
  if (multi && n_act == 0) {
    int64_t obs_total = 0;
    COOC_TRY(exchange_window(ctx, s, nullptr, 0, &obs_total));
    COOC_TRY(ensure_global(ctx));
    return finish_owned(ctx, s, ts, 0, obs_total, info);
  }
  if (n_act == 0) {
    // every interaction of the window was cut (user_cut): onEventTime emits nothing, no row is
    // touched and the global state is unchanged
    close_empty_window(ctx, ts, info);
    return Status::Ok();
  }

  // ---- host plan: history capacity (relocation on growth), append destinations, contributions
  std::vector<int64_t> act_off(n_act), cbase(n_act + 1, 0), new_ptr(n_act + 1, 0), new_dst(n_act), reloc;
  std::vector<int32_t> act_len(n_act), act_old(n_act), new_items;
  int64_t observed_window = 0;
  for (int64_t j = 0; j < n_act; j++) {
    const int32_t slot = staged_slots_[j];
    const int64_t old = h_len_[slot], w = int64_t(staged_items_[j].size());
    const int64_t need = old + w;
    if (need > int64_t(INT32_MAX)) return Status{COOC_ERR_ARG, "user history longer than 2^31"};
    reserve_history(slot, need, &reloc);
    act_off[j] = h_off_[slot];
    act_len[j] = int32_t(need);
    act_old[j] = int32_t(old);
    cbase[j + 1] = cbase[j] + need;
    new_dst[j] = h_off_[slot] + old;
    new_ptr[j + 1] = new_ptr[j] + w;
    new_items.insert(new_items.end(), staged_items_[j].begin(), staged_items_[j].end());
    observed_window += need * (need - 1) - old * (old - 1);  // sum over new positions of 2*|history|
    h_len_[slot] = int32_t(need);
  }
  tr.mark("host_plan");
  COOC_TRY(grow_arena(ctx, std::max<int64_t>(arena_used_, 1024)));
  COOC_TRY(upload(w_.reloc, reloc, s));
  COOC_TRY(upload(w_.new_items, new_items, s));
  COOC_TRY(upload(w_.new_dst_ptr, new_ptr, s));
  COOC_TRY(upload(w_.new_dst, new_dst, s));
  COOC_TRY(launch_relocate(s, int64_t(reloc.size() / 3), w_.reloc.as<int64_t>(), arena_.as<int32_t>()));
  COOC_TRY(launch_append(s, n_act, w_.new_dst_ptr.as<int64_t>(), w_.new_dst.as<int64_t>(), w_.new_items.as<int32_t>(),
                         arena_.as<int32_t>()));
  tr.mark("upload_append", s);

  // ---- expansion + keyed reduce of the window (the hot path)
  CountResult r;
  COOC_TRY(count_window(ctx, s, n_act, act_off, act_len, act_old, cbase, new_ptr[n_act], arena_.as<int32_t>(),
                        arena_used_, &r));
  tr.mark("count", s);

  if (multi) {  // ---- the owners' rows, then the same merge and rescoring over them
    int64_t obs_total = 0;
    COOC_TRY(exchange_window(ctx, s, &r, observed_window, &obs_total));
    COOC_TRY(ensure_global(ctx));
    return finish_owned(ctx, s, ts, observed_window, obs_total, info);
  }
  COOC_TRY(merge_and_rescore(ctx, s, ts, observed_window, r.observed, info));
  tr.mark("merge_rescore", s);
  tr.done(ts);
  return Status::Ok();
}

Status StreamState::count_window(cooc_ctx &ctx, hipStream_t s, int64_t n, const std::vector<int64_t> &off,
                                 const std::vector<int32_t> &len, const std::vector<int32_t> &old,
                                 const std::vector<int64_t> &cbase, int64_t n_new, const int32_t *src, int64_t span,
                                 CountResult *r) {
  COOC_TRY(upload(w_.act_off, off, s));
  COOC_TRY(upload(w_.act_len, len, s));
  COOC_TRY(upload(w_.act_old, old, s));
  COOC_TRY(upload(w_.cbase, cbase, s));
  if (ctx.counter.batch_ok()) {  // n_items < 40,320: the batch planner + k_acc_batch
    ActiveUsers au;
    au.n_active = n;
    au.off = w_.act_off.as<int64_t>();
    au.len = w_.act_len.as<int32_t>();
    au.old = w_.act_old.as<int32_t>();
    au.cbase = w_.cbase.as<int64_t>();
    au.n_contrib = cbase[n];
    au.n_new = n_new;
    au.arena = src;
    au.arena_span = span;
    COOC_TRY(ctx.counter.run_window(au, s, r, ctx.timer.enabled ? &ctx.timer : nullptr));  // (cooc_last_kernel_ms)
  } else {  // n_items >= 40,320 (or COOC_FLAG_GENERAL_PLANNER): the large-universe planner, old / new positions in one pass
    COOC_TRY(count_large_window(ctx, s, n, off, len, old, cbase[n], r, src));
  }
  delta_ = WindowDelta();
  delta_.row_base = r->row_base;
  delta_.row_nnz = r->row_nnz;
  delta_.col = r->col;
  delta_.cnt = r->cnt;
  delta_.rowsum = r->rowsum;
  delta_.runs = 1;
  return Status::Ok();
}

// ---- global merge + rescoring (ItemRowRescorer...java:144-228) of a single-subtask window's delta rows
Status StreamState::merge_and_rescore(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t observed_window,
                                      int64_t observed_info, cooc_window_info *info) {
  COOC_TRY(ensure_global(ctx));
  const WindowDelta &d = delta_;
  COOC_TRY(launch_merge_global(s, ctx.cfg.n_items, d.row_base, d.row_nnz, d.col, d.cnt, d.rowsum,
                               sparse_global_ ? nullptr : d_global_.as<uint32_t>(), d_grs_.as<int64_t>(),
                               d_scal_.as<int64_t>(), observed_window));
  return finish_tail(ctx, s, ts, observed_window, observed_info, 1, info);
}

// dense or sparse global rows: the touched rows' top-k (ItemRowRescorer...java:179-228)
Status StreamState::rescore_touched(cooc_ctx &ctx, hipStream_t s) {
  const int32_t M = ctx.cfg.n_items, topk = ctx.cfg.topk;
  if (topk <= 0) return Status::Ok();
  COOC_TRY(w_.topk_size.reserve(sizeof(int32_t) * M));
  COOC_TRY(w_.topk_val.reserve(sizeof(int32_t) * size_t(M) * topk));
  COOC_TRY(w_.topk_score.reserve(sizeof(double) * size_t(M) * topk));
  const bool exact = (ctx.cfg.flags & COOC_FLAG_EXACT_SCORES) != 0;
  int64_t *scal = d_scal_.as<int64_t>();
  if (sparse_global_)
    return launch_rescore_sparse(s, w_.touched.as<int32_t>(), scal, M, gs_, d_grs_.as<int64_t>(), exact, topk, M,
                                 w_.llr_terms, w_.topk_size.as<int32_t>(), w_.topk_val.as<int32_t>(),
                                 w_.topk_score.as<double>());
  return launch_rescore(s, w_.touched.as<int32_t>(), scal, M, d_global_.as<uint32_t>(), d_grs_.as<int64_t>(), exact,
                        topk, M, w_.llr_terms, w_.topk_size.as<int32_t>(), w_.topk_val.as<int32_t>(),
                        w_.topk_score.as<double>());
}

Status StreamState::finish_tail(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t obs_exact, int64_t obs_info,
                                int rowsum_slot, cooc_window_info *info) {
  const int32_t M = ctx.cfg.n_items;
  int64_t *scal = d_scal_.as<int64_t>();
  WindowDelta &d = delta_;
  if (sparse_global_) {  // the window's delta rows (packed) merged into the row slabs (ItemRowRescorer...java:171-177)
    if (!d.pk_rp) {      // the counter's rows (a signed delta is born packed: a new column with net 0 is inserted
                         // with count 0; the owned rows were packed by finish_owned)
      COOC_TRY(ctx.counter.pack(s, &d.pk_rp, &d.pk_col, &d.pk_cnt));
      PlanTotals pt;
      COOC_TRY(ctx.counter.read_totals(&pt));
      d.entries = pt.nnz_total;
    }
    int64_t new_cols = 0;
    COOC_TRY(launch_gs_merge(s, M, d.pk_rp, d.pk_col, d.pk_cnt, d.entries, gs_, d_scan_tmp_, &new_cols));
  }
  COOC_TRY(w_.touched.reserve(sizeof(int32_t) * M));
  COOC_TRY(launch_touched(s, M, d.row_nnz, w_.touched.as<int32_t>(), scal, d_scan_tmp_));
  COOC_TRY(rescore_touched(ctx, s));
  int64_t h_scal[8];
  COOC_HIP_TRY(hipMemcpyAsync(h_scal, scal, sizeof(h_scal), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  PlanTotals t;
  COOC_TRY(counter_totals(ctx, &t));

  n_touched_ = int32_t(h_scal[0]);
  observed_exact += obs_exact;
  observed_ref = h_scal[2];
  rowsum_acc += h_scal[rowsum_slot];
  rescored_items += n_touched_;

  if (d.entries < 0) d.entries = t.nnz_total;  // (the counter's rows, not packed yet)
  std::memset(&last_, 0, sizeof(last_));
  last_.ts = ts;
  last_.nnz = d.entries;
  last_.observed = obs_info;
  last_.n_rows = n_touched_;
  last_.topk = ctx.cfg.topk;
  last_.n_topk = ctx.cfg.topk > 0 ? n_touched_ : 0;
  close_window(info);
  return Status::Ok();
}

// p > 1: route the window's partial delta rows (r; nullptr: this subtask has no user in the window) to their
// owners over the communicator -- row a to subtask a mod world, the keyBy(ItemCooccurrences::getItem) of
// FlinkCooccurrences.java:152 -- and merge them there (Sharder: each owned row summed in a dense LDS row, checked
// against the all-reduced row sum); the window row sums (the rowSumStream.broadcast() of :163) and the window's
// ordered pairs all-reduced.  Leaves in delta_ the owned rows as an M-row view over the merge's rows, with every
// item's all-reduced window row sum.
Status StreamState::exchange_window(cooc_ctx &ctx, hipStream_t s, const CountResult *r, int64_t obs_local,
                                    int64_t *obs_total) {
  Comm &c = *ctx.comm;
  const int32_t M = ctx.cfg.n_items, W = c.world(), part = c.rank();
  auto rows_owned = [&](int32_t q) { return int64_t(M > q ? (M - q + W - 1) / W : 0); };
  const int runs = r ? 1 : 0;
  CountResult zero;
  if (!r) {  // no user here: zero partial rows
    COOC_TRY(w_.zero.reserve(sizeof(int64_t) * size_t(M) * 2 + 64));
    COOC_HIP_TRY(hipMemsetAsync(w_.zero.p, 0, sizeof(int64_t) * size_t(M) * 2 + 64, s));
    zero.row_base = w_.zero.as<int64_t>();
    zero.rowsum = w_.zero.as<int64_t>() + M;
    zero.row_nnz = reinterpret_cast<int32_t *>(w_.zero.as<int64_t>());
    zero.col = reinterpret_cast<int32_t *>(w_.zero.as<int64_t>());
    zero.cnt = reinterpret_cast<uint32_t *>(w_.zero.as<int64_t>());
    r = &zero;
  }
  // 1. entries per owner, the owner-major row counts and entries; every subtask's counts all-gathered
  std::vector<int64_t> h_ent(W), H(size_t(W) * W);
  COOC_TRY(ctx.sharder.plan(*r, M, W, s, h_ent.data()));
  int64_t n_send = 0;
  for (int64_t v : h_ent) n_send += v;
  COOC_TRY(w_.x_nnz.reserve(sizeof(int32_t) * size_t(M) + 4));
  COOC_TRY(w_.x_ent.reserve(sizeof(uint64_t) * size_t(n_send + 1)));
  COOC_TRY(ctx.sharder.pack(*r, M, W, s, w_.x_nnz.as<int32_t>(), n_send ? w_.x_ent.as<uint64_t>() : nullptr));
  COOC_TRY(w_.x_h.reserve(sizeof(int64_t) * size_t(W) * (W + 1)));
  int64_t *dh = w_.x_h.as<int64_t>();
  COOC_HIP_TRY(hipMemcpyAsync(dh, h_ent.data(), sizeof(int64_t) * W, hipMemcpyHostToDevice, s));
  COOC_TRY(c.allgather(dh, dh + W, sizeof(int64_t) * W, s));
  COOC_HIP_TRY(hipMemcpyAsync(H.data(), dh + W, sizeof(int64_t) * W * W, hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  // 2. row counts and entries to their owners (every peer pair in one exchange)
  const int64_t R = rows_owned(part);
  std::vector<int64_t> so(W), sb(W), ro(W), rb(W);
  int64_t off = 0;
  for (int32_t q = 0; q < W; q++) {
    so[q] = off;
    sb[q] = sizeof(int32_t) * rows_owned(q);
    off += sb[q];
    ro[q] = int64_t(sizeof(int32_t)) * q * R;
    rb[q] = int64_t(sizeof(int32_t)) * R;
  }
  COOC_TRY(w_.r_nnz.reserve(sizeof(int32_t) * size_t(W * R) + 4));
  COOC_TRY(c.alltoallv(w_.x_nnz.p, so.data(), sb.data(), w_.r_nnz.p, ro.data(), rb.data(), s));
  int64_t n_recv = 0;
  off = 0;
  for (int32_t q = 0; q < W; q++) {
    so[q] = off;
    sb[q] = int64_t(sizeof(uint64_t)) * h_ent[q];
    off += sb[q];
    ro[q] = int64_t(sizeof(uint64_t)) * n_recv;
    rb[q] = int64_t(sizeof(uint64_t)) * H[size_t(q) * W + part];
    n_recv += H[size_t(q) * W + part];
  }
  COOC_TRY(w_.r_ent.reserve(sizeof(uint64_t) * size_t(n_recv + 1)));
  COOC_TRY(c.alltoallv(w_.x_ent.p, so.data(), sb.data(), w_.r_ent.p, ro.data(), rb.data(), s));
  // 3. the window row sums of every item and the window's pairs, all-reduced
  COOC_TRY(w_.rs_win.reserve(sizeof(int64_t) * (size_t(M) + 1)));
  int64_t *rs = w_.rs_win.as<int64_t>();
  COOC_HIP_TRY(hipMemcpyAsync(rs, r->rowsum, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(rs + M, &obs_local, sizeof(int64_t), hipMemcpyHostToDevice, s));
  COOC_TRY(c.allreduce_sum_i64(rs, M + 1, s));
  COOC_HIP_TRY(hipMemcpyAsync(obs_total, rs + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  // 4. the owned rows merged (checked against the all-reduced row sums), as an M-row view
  MergeResult m;
  // (a sampled window's rows hold signed nets: a key whose nets cancel across subtasks stays, with count 0)
  COOC_TRY(ctx.sharder.merge(M, W, part, w_.r_nnz.as<int32_t>(), w_.r_ent.as<uint64_t>(), rs, s, &m, sampled()));
  COOC_TRY(w_.own_base.reserve(sizeof(int64_t) * size_t(M)));
  COOC_TRY(w_.own_nnz.reserve(sizeof(int32_t) * size_t(M)));
  COOC_TRY(launch_owned_view(s, M, W, part, m.n_rows, m.row_base, m.row_nnz, w_.own_base.as<int64_t>(),
                             w_.own_nnz.as<int32_t>()));
  delta_ = WindowDelta();
  delta_.row_base = w_.own_base.as<int64_t>();
  delta_.row_nnz = w_.own_nnz.as<int32_t>();
  delta_.col = m.col;
  delta_.cnt = m.cnt;
  delta_.rowsum = rs;
  delta_.runs = runs;
  COOC_HIP_TRY(hipStreamSynchronize(s));
  return Status::Ok();
}

// p > 1: the owned delta rows merged into the resident rows, every item's row sum into the global row sums, the
// owned touched rows rescored; the window's outputs are this subtask's owned rows (each item on one subtask).
Status StreamState::finish_owned(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t obs_local, int64_t obs_total,
                                 cooc_window_info *info) {
  const int32_t M = ctx.cfg.n_items;
  WindowDelta &d = delta_;
  COOC_TRY(launch_merge_owned(s, M, d.row_base, d.row_nnz, d.col, d.cnt, d.rowsum,
                              sparse_global_ ? nullptr : d_global_.as<uint32_t>(), d_grs_.as<int64_t>(),
                              d_scal_.as<int64_t>(), obs_total));
  // the owned delta rows packed (M-row CSR, ascending columns): the window's output, and for a large universe the
  // delta merged into the resident row slabs (ItemRowRescorer...java:171-177)
  COOC_TRY(launch_pack_rows(s, M, d.row_base, d.row_nnz, d.col, d.cnt, w_.own_rp, w_.own_pcol, w_.own_pcnt,
                            d_scan_tmp_, &d.entries));  // (synchronises s)
  d.pk_rp = w_.own_rp.as<int64_t>();
  d.pk_col = w_.own_pcol.as<int32_t>();
  d.pk_cnt = w_.own_pcnt.as<uint32_t>();
  // obs_local: this subtask's users' pairs (the rescorer's total, observed_ref, is the job's); scal[4]: this
  // subtask's owned row sums: the p accumulators of either kind sum to the job's
  return finish_tail(ctx, s, ts, obs_local, obs_local, 4, info);
}

Status StreamState::count_large_window(cooc_ctx &ctx, hipStream_t s, int64_t n_act, const std::vector<int64_t> &act_off,
                                      const std::vector<int32_t> &act_len, const std::vector<int32_t> &act_old,
                                      int64_t n_full, CountResult *r, const int32_t *src) {
  // (src: the arena, or a sampled window's reordered copies of the histories)
  // every pair whose later position is new (NonSampled...java:129-161), in one pass: user j's lists A_j
  // (its whole history) and B_j (the window's items, the tail of A_j) side by side; a new position
  // walks A_j, an old one B_j (run_sparse's SparseWindow, k_sp_window_contribs): 2 new |A_j| pair work
  // per user instead of |A_j|^2 + |old|^2
  std::vector<int64_t> up2(2 * n_act + 1), dst_a(n_act), dst_b(n_act), src_b(n_act);
  std::vector<int32_t> len_b(n_act);
  int64_t o = 0;
  for (int64_t j = 0; j < n_act; j++) {
    up2[2 * j] = dst_a[j] = o;
    o += act_len[j];
    up2[2 * j + 1] = dst_b[j] = o;
    src_b[j] = act_off[j] + act_old[j];
    len_b[j] = act_len[j] - act_old[j];
    o += len_b[j];
  }
  up2[2 * n_act] = o;
  COOC_TRY(upload(w_.lw_up2, up2, s));
  COOC_TRY(upload(w_.lw_dsta, dst_a, s));
  COOC_TRY(upload(w_.lw_dstb, dst_b, s));
  COOC_TRY(upload(w_.lw_srcb, src_b, s));
  COOC_TRY(upload(w_.lw_lenb, len_b, s));
  COOC_TRY(w_.lw_items.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(o, 1))));
  int32_t *lists = w_.lw_items.as<int32_t>();
  COOC_TRY(launch_gather_lists(s, n_act, w_.act_off.as<int64_t>(), w_.act_len.as<int32_t>(), w_.lw_dsta.as<int64_t>(),
                               src, lists));
  COOC_TRY(launch_gather_lists(s, n_act, w_.lw_srcb.as<int64_t>(), w_.lw_lenb.as<int32_t>(), w_.lw_dstb.as<int64_t>(),
                               src, lists));
  SparseWindow w;
  w.n_users = n_act;
  w.old = w_.act_old.as<int32_t>();
  w.cbase = w_.cbase.as<int64_t>();
  w.n_contrib = n_full;
  return ctx.counter.run_sparse(2 * n_act, w_.lw_up2.as<int64_t>(), lists, o, s, r,
                                ctx.timer.enabled ? &ctx.timer : nullptr, nullptr, 0, nullptr, 0, &w);
}

Status StreamState::copy_delta(cooc_ctx &ctx, int32_t *rows, int64_t *row_ptr, int32_t *cols, uint32_t *cnt,
                               int16_t *cnt16) {
  if (!have_window_) return Status{COOC_ERR_STATE, "no finished window"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  if (delta_.empty()) {
    if (row_ptr) row_ptr[0] = 0;
    return Status::Ok();
  }
  COOC_TRY(pack_delta(ctx));
  const int32_t R = int32_t(delta_rows_.size());
  if (rows) std::memcpy(rows, delta_rows_.data(), sizeof(int32_t) * R);
  if (row_ptr) std::memcpy(row_ptr, delta_start_.data(), sizeof(int64_t) * (R + 1));
  return copy_entries(0, delta_start_[R], cols, cnt, cnt16);
}

// The window's delta rows packed (contiguous, ascending row then column) once per window, with the
// host list of rows that have entries and their starts in the packed arrays.
Status StreamState::pack_delta(cooc_ctx &ctx) {
  if (delta_packed_) return Status::Ok();
  const int32_t M = ctx.cfg.n_items;
  WindowDelta &d = delta_;
  if (!d.pk_rp)  // the counter's rows, not merged into row slabs: packed when a copy-out first asks
    COOC_TRY(ctx.counter.pack(ctx.stream, &d.pk_rp, &d.pk_col, &d.pk_cnt));
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  std::vector<int64_t> rp(M + 1);
  COOC_HIP_TRY(hipMemcpy(rp.data(), d.pk_rp, sizeof(int64_t) * (M + 1), hipMemcpyDeviceToHost));
  delta_rows_.clear();
  delta_start_.clear();
  for (int32_t a = 0; a < M; a++) {
    if (rp[a + 1] == rp[a]) continue;
    delta_rows_.push_back(a);
    delta_start_.push_back(rp[a]);
  }
  delta_start_.push_back(rp[M]);
  delta_packed_ = true;
  return Status::Ok();
}

Status StreamState::copy_entries(int64_t e0, int64_t e1, int32_t *cols, uint32_t *cnt, int16_t *cnt16) {
  const int64_t n = e1 - e0;
  if (n <= 0) return Status::Ok();
  if (cols) COOC_HIP_TRY(hipMemcpy(cols, delta_.pk_col + e0, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (cnt || cnt16) {
    std::vector<uint32_t> tmp;
    uint32_t *dst = cnt;
    if (!dst) {
      tmp.resize(n);
      dst = tmp.data();
    }
    COOC_HIP_TRY(hipMemcpy(dst, delta_.pk_cnt + e0, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (cnt16)  // ItemRowAggregator's Int2ShortOpenHashMap value (short addTo wraps)
      for (int64_t i = 0; i < n; i++) cnt16[i] = int16_t(uint16_t(dst[i]));
  }
  return Status::Ok();
}

Status StreamState::copy_delta_range(cooc_ctx &ctx, int32_t r0, int32_t r1, int64_t cap, int32_t *cols,
                                     uint32_t *cnt, int16_t *cnt16) {
  if (!have_window_) return Status{COOC_ERR_STATE, "no finished window"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  const int32_t R = delta_.empty() ? 0 : last_.n_rows;
  if (r0 < 0 || r1 < r0 || r1 > R)
    return Status{COOC_ERR_ARG, "delta rows [" + std::to_string(r0) + ", " + std::to_string(r1) + ") outside [0, " +
                                    std::to_string(R) + ")"};
  if (r0 == r1) return Status::Ok();
  COOC_TRY(pack_delta(ctx));
  const int64_t n = delta_start_[r1] - delta_start_[r0];
  if ((cols || cnt || cnt16) && n > cap)  // (the caller's buffers are smaller than the range)
    return Status{COOC_ERR_ARG, "delta rows [" + std::to_string(r0) + ", " + std::to_string(r1) + ") hold " +
                                    std::to_string(n) + " entries, more than the " + std::to_string(cap) + " given"};
  return copy_entries(delta_start_[r0], delta_start_[r1], cols, cnt, cnt16);
}

Status StreamState::copy_rowsums(cooc_ctx &ctx, int32_t *items, int64_t *delta, int32_t *delta32) {
  if (!have_window_) return Status{COOC_ERR_STATE, "no finished window"};
  if (delta_.empty()) return Status::Ok();
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  const int32_t M = ctx.cfg.n_items;
  std::vector<int32_t> nnz(M);
  std::vector<int64_t> rs(M);
  // (p > 1: the owned rows with a delta and their all-reduced row sums: each item on its owner only)
  // (a sampled window with replacements: the signed delta's rows and row-sum differences)
  COOC_HIP_TRY(hipMemcpy(nnz.data(), delta_.row_nnz, sizeof(int32_t) * M, hipMemcpyDeviceToHost));
  COOC_HIP_TRY(hipMemcpy(rs.data(), delta_.rowsum, sizeof(int64_t) * M, hipMemcpyDeviceToHost));
  int32_t k = 0;
  for (int32_t a = 0; a < M; a++) {
    if (nnz[a] == 0) continue;
    if (items) items[k] = a;
    if (delta) delta[k] = rs[a];
    if (delta32) delta32[k] = int32_t(uint32_t(uint64_t(rs[a])));  // Java int accumulation
    k++;
  }
  return Status::Ok();
}

Status StreamState::copy_topk(cooc_ctx &ctx, int32_t *rows, int32_t *sizes, int32_t *values, double *scores) {
  if (!have_window_) return Status{COOC_ERR_STATE, "no finished window"};
  if (ctx.cfg.topk <= 0) return Status{COOC_ERR_STATE, "rescoring is disabled (topk == 0)"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  const size_t n = size_t(n_touched_), k = size_t(ctx.cfg.topk);
  if (n == 0) return Status::Ok();
  if (rows) COOC_HIP_TRY(hipMemcpy(rows, w_.touched.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (sizes) COOC_HIP_TRY(hipMemcpy(sizes, w_.topk_size.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (values) COOC_HIP_TRY(hipMemcpy(values, w_.topk_val.p, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost));
  if (scores) COOC_HIP_TRY(hipMemcpy(scores, w_.topk_score.p, sizeof(double) * n * k, hipMemcpyDeviceToHost));
  return Status::Ok();
}

Status StreamState::global_rowsums(cooc_ctx &ctx, int64_t *exact, int32_t *v32) {
  const int32_t M = ctx.cfg.n_items;
  std::vector<int64_t> rs(M, 0);
  if (global_ready_) {
    COOC_HIP_TRY(hipSetDevice(ctx.device));
    COOC_HIP_TRY(hipMemcpy(rs.data(), d_grs_.p, sizeof(int64_t) * M, hipMemcpyDeviceToHost));
  }
  if (exact) std::memcpy(exact, rs.data(), sizeof(int64_t) * M);
  if (v32)  // globalItemRowSums (Int2IntOpenHashMap, int32 wrap)
    for (int32_t a = 0; a < M; a++) v32[a] = int32_t(uint32_t(uint64_t(rs[a])));
  return Status::Ok();
}

// A global row's entries in ascending column order: the row's slab, or the non-zero cells of the dense matrix's
// row (a key exists iff it was ever touched).  A sampled slab may keep an entry whose count went back to 0: not a
// key, skipped.
Status StreamState::read_global_row(int32_t M, int32_t item, std::vector<int32_t> *cols, std::vector<uint32_t> *cnt) {
  cols->clear();
  cnt->clear();
  if (!sparse_global_) {
    std::vector<uint32_t> row(M);
    COOC_HIP_TRY(hipMemcpy(row.data(), d_global_.as<uint32_t>() + int64_t(item) * M, sizeof(uint32_t) * M,
                           hipMemcpyDeviceToHost));
    for (int32_t b = 0; b < M; b++) {
      if (!row[b]) continue;
      cols->push_back(b);
      cnt->push_back(row[b]);
    }
    return Status::Ok();
  }
  int32_t n = 0;
  int64_t b = 0;
  COOC_HIP_TRY(hipMemcpy(&n, gs_.len.as<int32_t>() + item, sizeof(int32_t), hipMemcpyDeviceToHost));
  COOC_HIP_TRY(hipMemcpy(&b, gs_.base.as<int64_t>() + item, sizeof(int64_t), hipMemcpyDeviceToHost));
  cols->resize(n);
  cnt->resize(n);
  if (n == 0) return Status::Ok();
  COOC_HIP_TRY(hipMemcpy(cols->data(), gs_.col.as<int32_t>() + b, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  COOC_HIP_TRY(hipMemcpy(cnt->data(), gs_.cnt.as<uint32_t>() + b, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  if (sampled()) {
    int32_t k = 0;
    for (int32_t i = 0; i < n; i++) {
      if (!(*cnt)[i]) continue;
      (*cols)[k] = (*cols)[i];
      (*cnt)[k++] = (*cnt)[i];
    }
    cols->resize(k);
    cnt->resize(k);
  }
  return Status::Ok();
}

Status StreamState::global_row_nnz(cooc_ctx &ctx, int32_t item, int64_t *nnz) {
  const int32_t M = ctx.cfg.n_items;
  if (item < 0 || item >= M) return Status{COOC_ERR_ARG, "item outside [0, n_items)"};
  *nnz = 0;
  if (!global_ready_) return Status::Ok();
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  if (sparse_global_ && !sampled()) {  // every slab entry is a key: the length alone
    int32_t n = 0;
    COOC_HIP_TRY(hipMemcpy(&n, gs_.len.as<int32_t>() + item, sizeof(int32_t), hipMemcpyDeviceToHost));
    *nnz = n;
    return Status::Ok();
  }
  std::vector<int32_t> cols;
  std::vector<uint32_t> cnt;
  COOC_TRY(read_global_row(M, item, &cols, &cnt));
  *nnz = int64_t(cols.size());
  return Status::Ok();
}

Status StreamState::global_row(cooc_ctx &ctx, int32_t item, int32_t *cols, uint32_t *cnt, int16_t *cnt16) {
  const int32_t M = ctx.cfg.n_items;
  if (item < 0 || item >= M) return Status{COOC_ERR_ARG, "item outside [0, n_items)"};
  if (!global_ready_) return Status::Ok();
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  std::vector<int32_t> c;
  std::vector<uint32_t> n;
  COOC_TRY(read_global_row(M, item, &c, &n));
  for (size_t k = 0; k < c.size(); k++) {
    if (cols) cols[k] = c[k];
    if (cnt) cnt[k] = n[k];
    if (cnt16) cnt16[k] = int16_t(uint16_t(n[k]));
  }
  return Status::Ok();
}

// ---- sampled mode (cooc_sampling_enable): item cut, per-user reservoir, retractions ----------------
Status StreamState::sampling_enable(cooc_ctx &ctx, int32_t item_cut, int64_t seed, bool on_device) {
  if (ctx.cfg.user_cut <= 0)
    return Status{COOC_ERR_STATE, "sampling needs cfg.user_cut > 0 (the reservoir size)"};
  if (sampled()) return Status{COOC_ERR_STATE, "sampling is already enabled on this context"};
  if (!pristine() || !ctx.op.pristine() || ctx.restore_bytes >= 0)
    return Status{COOC_ERR_STATE, "sampling is enabled only on a context without streaming state"};
  if (item_cut < 1 || item_cut > 32767)
    return Status{COOC_ERR_ARG, "item_cut " + std::to_string(item_cut) + " outside [1, 32767]"};
  if (on_device) {
    COOC_HIP_TRY(hipSetDevice(ctx.device));
    COOC_TRY(dev_sampler_.enable(ctx.cfg.n_items, item_cut, ctx.cfg.user_cut, uint64_t(seed), ctx.stream));
  }
  sampler_.enable(ctx.cfg.n_items, item_cut, ctx.cfg.user_cut, uint64_t(seed));
  return Status::Ok();
}

Status StreamState::sampling_counters(cooc_ctx &ctx, int64_t out[6]) {
  if (!dev_sampler_.enabled()) {
    sampler_.counters(out);
    return Status::Ok();
  }
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  return dev_sampler_.counters(ctx.stream, out);
}

Status StreamState::submit_records(cooc_ctx &ctx, int64_t ts, int64_t n, const int32_t *users, const int32_t *items) {
  if (!sampled()) return Status{COOC_ERR_STATE, "record-order submit needs the sampled mode"};
  COOC_TRY(window_open(ts));
  if (const int32_t *bad = bad_item(items, n, ctx.cfg.n_items)) return item_error(*bad);
  rec_users_.insert(rec_users_.end(), users, users + n);
  rec_items_.insert(rec_items_.end(), items, items + n);
  staged_ = true;
  staged_ts_ = ts;
  return Status::Ok();
}

// The host sampler's window (Sampler::window over the staged records): its changed users as SmChange records, the
// distinct replaced slots that existed before the window by sort + unique, the lists uploaded.
Status StreamState::sampled_changes_host(cooc_ctx &ctx, hipStream_t s, std::vector<SmChange> *changed,
                                         const int32_t **d_app, const int32_t **d_rep) {
  const int64_t n_rec = int64_t(rec_users_.size());
  rec_slots_.resize(size_t(n_rec));
  for (int64_t i = 0; i < n_rec; i++) rec_slots_[i] = slot_for(rec_users_[i]);
  if (!(ctx.comm && ctx.comm->world() > 1)) {
    sampler_.window(n_rec, rec_users_.data(), rec_slots_.data(), rec_items_.data());
  } else {
    // world > 1: the window's histogram (sorted by item) through the item-cut exchange; what comes back -- the
    // lower ranks' records of every local item, the job's records of every item of the union -- decides the cut
    // and commits the counters; then the feedbacks that arose here go out and the peers' are subtracted
    Comm &c = *ctx.comm;
    const uint64_t M = uint64_t(ctx.cfg.n_items);
    icx_words_.assign(rec_items_.begin(), rec_items_.end());
    std::sort(icx_words_.begin(), icx_words_.end());
    size_t n_hist = 0;
    for (size_t i = 0; i < icx_words_.size();) {
      size_t j = i;
      while (j < icx_words_.size() && icx_words_[j] == icx_words_[i]) j++;
      icx_words_[n_hist++] = (icx_words_[i] << 32) | uint64_t(j - i);
      i = j;
    }
    icx_words_.resize(n_hist);
    COOC_TRY(icx_.gather_host(c, s, icx_words_.data(), int64_t(n_hist)));
    COOC_TRY(icx_.resolve(s));
    COOC_TRY(icx_.read_back(s, &icx_all_, &icx_base_, &icx_tot_));
    for (size_t k = 0; k < icx_all_.size(); k++)
      if (icx_tot_[k] >= 0 && (icx_all_[k] >> 32) >= M)
        return Status{COOC_ERR_STATE, "item-cut exchange: a peer's item outside [0, n_items)"};
    Sampler::RankCut cut;
    cut.n_local = int64_t(n_hist);
    cut.local = icx_words_.data();
    cut.base = icx_base_.data();
    cut.n_slots = int64_t(icx_all_.size());
    cut.all = icx_all_.data();
    cut.tot = icx_tot_.data();
    sampler_.window(n_rec, rec_users_.data(), rec_slots_.data(), rec_items_.data(), &cut);
    const std::vector<int32_t> &fb = sampler_.feedback();
    icx_words_.resize(fb.size());
    for (size_t k = 0; k < fb.size(); k++) icx_words_[k] = uint64_t(uint32_t(fb[k]));
    COOC_TRY(icx_.gather_host(c, s, icx_words_.data(), int64_t(fb.size())));
    COOC_TRY(icx_.read_back(s, &icx_all_, nullptr, nullptr));
    for (int32_t q = 0; q < c.world(); q++) {
      if (q == c.rank()) continue;
      const uint64_t *list = icx_all_.data() + size_t(q) * size_t(icx_.lmax());
      for (int64_t k = 0; k < icx_.lens()[size_t(q)]; k++) {
        if (list[k] >= M) return Status{COOC_ERR_STATE, "item-cut exchange: a peer's item outside [0, n_items)"};
        sampler_.peer_feedback(int32_t(list[k]));
      }
    }
  }
  const int64_t n_act = sampler_.n_changed();
  changed->resize(size_t(n_act));
  std::vector<int32_t> app, rep, slots_sorted;
  for (int64_t j = 0; j < n_act; j++) {
    const Sampler::Changed &c = sampler_.changed(int32_t(j));
    const int32_t need = sampler_.length(c.slot), old = need - int32_t(c.appended.size());
    // distinct replaced slots that existed before the window
    slots_sorted.clear();
    for (size_t r = 0; r < c.replaced.size(); r += 2) {
      if (c.replaced[r] < 0 || c.replaced[r] >= need)
        return Status{COOC_ERR_STATE, "internal error: replaced slot outside the reservoir"};
      if (c.replaced[r] < old) slots_sorted.push_back(c.replaced[r]);
    }
    std::sort(slots_sorted.begin(), slots_sorted.end());
    const int64_t n_ce = std::unique(slots_sorted.begin(), slots_sorted.end()) - slots_sorted.begin();
    if (app.size() + c.appended.size() > size_t(INT32_MAX) || rep.size() + c.replaced.size() > size_t(INT32_MAX))
      return Status{COOC_ERR_ARG, "more than 2^31 reservoir changes in one window"};
    (*changed)[j] = SmChange{c.slot, old, int32_t(c.appended.size()), int32_t(c.replaced.size() / 2), int32_t(n_ce),
                             int32_t(app.size()), int32_t(rep.size() / 2), 0};
    app.insert(app.end(), c.appended.begin(), c.appended.end());
    rep.insert(rep.end(), c.replaced.begin(), c.replaced.end());
  }
  if (n_act > 0) {
    COOC_TRY(upload(w_.sm_app, app, s));
    COOC_TRY(upload(w_.sm_rep, rep, s));
  }
  *d_app = w_.sm_app.as<int32_t>();
  *d_rep = w_.sm_rep.as<int32_t>();
  return Status::Ok();
}

// The device sampler's window (SampleStream::window): the host maps the ids to slots and uploads the records; the
// changed users come back as SmChange records, their lists stay on the device.
Status StreamState::sampled_changes_device(cooc_ctx &ctx, hipStream_t s, std::vector<SmChange> *changed,
                                           const int32_t **d_app, const int32_t **d_rep) {
  const size_t n_rec = rec_users_.size();
  rec_slots_.resize(3 * n_rec);  // the upload: slots, user ids, items
  int64_t n_distinct = 0;
  sm_seq_++;
  for (size_t i = 0; i < n_rec; i++) {
    const int32_t slot = slot_for(rec_users_[i]);
    rec_slots_[i] = slot;
    if (staged_stamp_[slot] != sm_seq_) {  // (the stamps of the fill path's staging: unused in this mode)
      staged_stamp_[slot] = sm_seq_;
      n_distinct++;
    }
  }
  std::copy(rec_users_.begin(), rec_users_.end(), rec_slots_.begin() + n_rec);
  std::copy(rec_items_.begin(), rec_items_.end(), rec_slots_.begin() + 2 * n_rec);
  COOC_TRY(dev_sampler_.window(s, int64_t(n_rec), rec_slots_.data(), int64_t(h_off_.size()), n_distinct, changed,
                               ctx.comm.get(), &icx_));
  *d_app = dev_sampler_.app();
  *d_rep = dev_sampler_.rep();
  return Status::Ok();
}

// One sampled window.  Every record is decided by the host sampler or, after cooc_sampling_enable_device, by the
// device sampler (the two functions above: the only difference between the modes); the users with a changed slot
// get a plus list and, when a slot that existed before the window was replaced, a minus list (k_sm_lists); the
// window counter runs over the plus lists and, if there is any minus list, once more over those; the two runs'
// packed rows combine into the signed delta (launch_signed_delta), which is merged and rescored as any window's
// delta.
Status StreamState::finish_sampled(cooc_ctx &ctx, int64_t ts, cooc_window_info *info) {
  ctx.snapshot_release();
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  delta_packed_ = false;
  const int32_t *d_app = nullptr, *d_rep = nullptr;
  if (dev_sampler_.enabled()) COOC_TRY(sampled_changes_device(ctx, s, &sm_changed_, &d_app, &d_rep));
  else COOC_TRY(sampled_changes_host(ctx, s, &sm_changed_, &d_app, &d_rep));
  rec_users_.clear();
  rec_items_.clear();
  const int64_t n_act = int64_t(sm_changed_.size());
  // p > 1 subtasks: the samplers above have exchanged the item cut and the feedback; the window's rows (the plus
  // run's, or the signed delta) go to their owners as any window's partial rows do, and every subtask takes part in
  // the exchange, also with no changed slot of its own
  const bool multi = ctx.comm && ctx.comm->world() > 1;
  auto finish_rows = [&](const CountResult *rows, int runs, int64_t observed_window) -> Status {
    if (!multi) return merge_and_rescore(ctx, s, ts, observed_window, observed_window, info);
    int64_t obs_total = 0;
    COOC_TRY(exchange_window(ctx, s, rows, observed_window, &obs_total));
    delta_.runs = runs;
    COOC_TRY(ensure_global(ctx));
    return finish_owned(ctx, s, ts, observed_window, obs_total, info);
  };
  if (n_act == 0) {
    if (multi) return finish_rows(nullptr, 0, 0);
    // no slot changed (only rejections and feedback, already applied): nothing is emitted, no row is touched
    close_empty_window(ctx, ts, info);
    return Status::Ok();
  }

  // ---- host plan: history capacity, the users' appends and replacements, the lists' places
  std::vector<SmUser> users(n_act);
  std::vector<int64_t> reloc, p_off(n_act), p_cbase(n_act + 1, 0), m_off, m_cbase(1, 0);
  std::vector<int32_t> p_len(n_act), p_old(n_act), m_len, m_old;
  int64_t observed_window = 0, lists_len = 0, p_new = 0, m_new = 0;
  for (int64_t j = 0; j < n_act; j++) {
    const SmChange &c = sm_changed_[j];
    const int32_t slot = c.slot;
    if (slot < 0 || size_t(slot) >= h_len_.size() || c.fills < 0 || c.n_rep < 0 || c.fills + c.n_rep == 0)
      return Status{COOC_ERR_STATE, "internal error: a changed user without a slot or a change"};
    const int64_t old = h_len_[slot], w = c.fills, need = old + w;
    if (need > ctx.cfg.user_cut || c.len_old != old)  // the sampler's length after the window is old + fills
      return Status{COOC_ERR_STATE, "internal error: reservoir length out of step"};
    if (c.n_old_distinct < 0 || c.n_old_distinct > old || c.n_old_distinct > c.n_rep)
      return Status{COOC_ERR_STATE, "internal error: replaced slot outside the reservoir"};
    reserve_history(slot, need, &reloc);
    SmUser &u = users[j];
    u.arena_off = h_off_[slot];
    u.len_old = int32_t(old);
    u.len_new = int32_t(need);
    u.n_unchanged = int32_t(old - c.n_old_distinct);
    u.app_begin = c.app_begin;
    u.rep_begin = c.rep_begin;
    u.n_rep = c.n_rep;
    u.plus_dst = lists_len;
    lists_len += need;
    u.minus_dst = -1;
    p_off[j] = u.plus_dst;
    p_len[j] = u.len_new;
    p_old[j] = u.n_unchanged;
    p_cbase[j + 1] = p_cbase[j] + need;
    p_new += need - u.n_unchanged;
    observed_window += need * (need - 1) - old * (old - 1);  // fills only (UserInteractionCounter...java:195)
    h_len_[slot] = int32_t(need);
  }
  for (int64_t j = 0; j < n_act; j++) {  // the minus lists behind all plus lists
    SmUser &u = users[j];
    if (u.n_unchanged == u.len_old) continue;
    u.minus_dst = lists_len;
    lists_len += u.len_old;
    m_off.push_back(u.minus_dst);
    m_len.push_back(u.len_old);
    m_old.push_back(u.n_unchanged);
    m_cbase.push_back(m_cbase.back() + u.len_old);
    m_new += u.len_old - u.n_unchanged;
  }
  const int64_t n_minus_users = int64_t(m_off.size());
  COOC_TRY(grow_arena(ctx, std::max<int64_t>(arena_used_, 1024)));
  COOC_TRY(upload(w_.reloc, reloc, s));
  COOC_TRY(upload(w_.sm_users, users, s));
  COOC_TRY(w_.sm_lists.reserve(sizeof(int32_t) * size_t(lists_len + 1)));
  COOC_TRY(w_.sm_err.reserve(sizeof(int32_t)));
  COOC_TRY(launch_relocate(s, int64_t(reloc.size() / 3), w_.reloc.as<int64_t>(), arena_.as<int32_t>()));
  COOC_TRY(launch_sm_lists(s, n_act, w_.sm_users.as<SmUser>(), d_app, d_rep, arena_.as<int32_t>(),
                           int64_t(arena_.cap / sizeof(int32_t)), w_.sm_lists.as<int32_t>(), lists_len,
                           w_.sm_err.as<int32_t>()));
  int32_t sm_err = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&sm_err, w_.sm_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (sm_err) return Status{COOC_ERR_STATE, "internal bounds check failed (reservoir lists)"};

  // ---- the window counter over the plus lists in w_.sm_lists
  const int32_t *lists = w_.sm_lists.as<int32_t>();
  CountResult r;
  COOC_TRY(count_window(ctx, s, n_act, p_off, p_len, p_old, p_cbase, p_new, lists, lists_len, &r));
  if (n_minus_users == 0)  // no slot that existed was replaced: the fill path's window
    return finish_rows(&r, 1, observed_window);

  // ---- the plus run's packed rows set aside (the counter's buffers are reused), the minus run, the signed delta
  int64_t *rp;
  int32_t *col;
  uint32_t *cnt;
  PlanTotals plus, minus;
  COOC_TRY(ctx.counter.pack(s, &rp, &col, &cnt));  // (synchronises s before it sizes the packed arrays)
  COOC_HIP_TRY(hipStreamSynchronize(s));
  COOC_TRY(counter_totals(ctx, &plus));
  const int64_t n_plus = plus.nnz_total;
  COOC_TRY(w_.sm_prp.reserve(sizeof(int64_t) * (size_t(M) + 1)));
  COOC_TRY(w_.sm_pcol.reserve(sizeof(int32_t) * size_t(n_plus + 1)));
  COOC_TRY(w_.sm_pcnt.reserve(sizeof(uint32_t) * size_t(n_plus + 1)));
  COOC_TRY(w_.sm_prs.reserve(sizeof(int64_t) * size_t(M)));
  COOC_HIP_TRY(hipMemcpyAsync(w_.sm_prp.p, rp, sizeof(int64_t) * (size_t(M) + 1), hipMemcpyDeviceToDevice, s));
  if (n_plus > 0) {
    COOC_HIP_TRY(hipMemcpyAsync(w_.sm_pcol.p, col, sizeof(int32_t) * size_t(n_plus), hipMemcpyDeviceToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(w_.sm_pcnt.p, cnt, sizeof(uint32_t) * size_t(n_plus), hipMemcpyDeviceToDevice, s));
  }
  COOC_HIP_TRY(hipMemcpyAsync(w_.sm_prs.p, r.rowsum, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  CountResult rm;
  COOC_TRY(count_window(ctx, s, n_minus_users, m_off, m_len, m_old, m_cbase, m_new, lists, lists_len, &rm));
  COOC_TRY(ctx.counter.pack(s, &rp, &col, &cnt));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  COOC_TRY(counter_totals(ctx, &minus));
  SignedDelta &sd = w_.sd;
  COOC_TRY(launch_signed_delta(s, M, w_.sm_prp.as<int64_t>(), w_.sm_pcol.as<int32_t>(), w_.sm_pcnt.as<uint32_t>(),
                               w_.sm_prs.as<int64_t>(), n_plus, rp, col, cnt, rm.rowsum, minus.nnz_total, sd,
                               d_scan_tmp_));
  delta_ = WindowDelta();
  delta_.row_base = delta_.pk_rp = sd.rp.as<int64_t>();
  delta_.row_nnz = sd.nnz.as<int32_t>();
  delta_.col = delta_.pk_col = sd.col.as<int32_t>();
  delta_.cnt = delta_.pk_cnt = sd.cnt.as<uint32_t>();
  delta_.rowsum = sd.rowsum.as<int64_t>();
  delta_.entries = sd.entries;
  delta_.runs = 2;
  CountResult signed_rows;  // (p > 1: the signed delta as this subtask's partial rows)
  signed_rows.row_base = sd.rp.as<int64_t>();
  signed_rows.row_nnz = sd.nnz.as<int32_t>();
  signed_rows.col = sd.col.as<int32_t>();
  signed_rows.cnt = sd.cnt.as<uint32_t>();
  signed_rows.rowsum = sd.rowsum.as<int64_t>();
  return finish_rows(&signed_rows, 2, observed_window);
}

int32_t StreamState::find_slot(int32_t uid) const {
  if (uid >= 0 && uid < (1 << 26)) return size_t(uid) < dense_slot_.size() ? dense_slot_[uid] : -1;
  auto it = slot_of_.find(uid);
  return it == slot_of_.end() ? -1 : it->second;
}

Status StreamState::copy_user_history(cooc_ctx &ctx, int32_t user, int32_t cap, int32_t *items, int32_t *len,
                                      int32_t *total) {
  const int32_t slot = find_slot(user);
  const int32_t n = slot < 0 ? 0 : h_len_[slot];
  if (len) *len = n;
  if (total) *total = slot < 0 ? 0 : sampled() ? sampler_.total(slot) : n;
  if (total && slot >= 0 && dev_sampler_.enabled()) {
    COOC_HIP_TRY(hipSetDevice(ctx.device));
    COOC_TRY(dev_sampler_.total(ctx.stream, slot, total));
  }
  if (!items || n == 0) return Status::Ok();
  if (cap < n)
    return Status{COOC_ERR_ARG, "user history holds " + std::to_string(n) + " items, more than the " +
                                    std::to_string(cap) + " given"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  COOC_HIP_TRY(hipMemcpy(items, arena_.as<int32_t>() + h_off_[slot], sizeof(int32_t) * size_t(n), hipMemcpyDeviceToHost));
  return Status::Ok();
}

// ---- NonSampledUserInteractionCounterOneInputStreamOperator mirror -------------------------------
Status Operator::process_elements(cooc_ctx &ctx, int64_t n, const int32_t *users, const int32_t *items,
                                  const int64_t *ts, int64_t *n_late) {
  const int32_t M = ctx.cfg.n_items;
  int64_t late = 0;
  for (int64_t i = 0; i < n; i++) {
    if (ts[i] <= watermark) {  // :89-91
      late++;
      continue;
    }
    if (items[i] < 0 || items[i] >= M) return item_error(items[i]);
    Pending &p = pending_[window_max_ts(ts[i], ctx.cfg.window_size_ms)];  // :93-100
    p.users.push_back(users[i]);
    p.items.push_back(items[i]);
  }
  late_elements += late;
  if (n_late) *n_late = late;
  return Status::Ok();
}

Status Operator::process_watermark(cooc_ctx &ctx, int64_t wm, int32_t *fired, cooc_window_info *info) {
  if (wm > watermark) watermark = wm;
  *fired = 0;
  if (ctx.comm && ctx.comm->world() > 1) {
    // p > 1: Flink does not hand every subtask the same watermarks (each is the minimum over its own input
    // channels, which arrive in their own order), so what fires is decided from all-gathered state only.  An
    // agreement step all-gathers (this subtask's watermark, its earliest pending window); agreed_ becomes the
    // minimum watermark -- every window ending at or before it is complete on every subtask, a record of it
    // arriving later being late everywhere (:89-91) -- and the earliest pending window ending there fires on
    // every subtask together (one without records in it joins with no user).  A subtask runs a step while its
    // own watermark is ahead of agreed_ (it waits there for the others to catch up) and after a step that fired
    // (more windows may be due): both conditions are functions of the all-gathered state and of watermarks that
    // only grow, so every subtask runs the same sequence of collectives whatever order its watermarks came in.
    const int world = ctx.comm->world();
    std::vector<int64_t> all(static_cast<size_t>(world));
    while (regather_ || watermark > agreed_) {
      regather_ = false;
      COOC_TRY(ctx.comm_allgather_i64(watermark, all.data()));
      const int64_t wmin = *std::min_element(all.begin(), all.end());
      const int64_t mine = pending_.empty() ? INT64_MAX : pending_.begin()->first;
      COOC_TRY(ctx.comm_allgather_i64(mine, all.data()));
      if (wmin > agreed_) agreed_ = wmin;
      const int64_t due = *std::min_element(all.begin(), all.end());
      if (due != INT64_MAX && due <= agreed_) {
        regather_ = true;
        return fire(ctx, due, mine == due, fired, info);
      }
    }
    return Status::Ok();
  }
  auto it = pending_.begin();
  if (it == pending_.end() || it->first > watermark) return Status::Ok();
  return fire(ctx, it->first, true, fired, info);
}

// onEventTime for every user of the window max_ts (mine: this subtask holds its records, the earliest pending
// window; else it joins the p > 1 exchange with no user).
Status Operator::fire(cooc_ctx &ctx, int64_t max_ts, bool mine, int32_t *fired, cooc_window_info *info) {
  StreamState &st = ctx.stream_state;
  if (mine) {
    auto it = pending_.begin();
    Pending &p = it->second;
    if (st.sampled()) {  // the item cut and the reservoir see the records in arrival order across users
      COOC_TRY(st.submit_records(ctx, max_ts, int64_t(p.users.size()), p.users.data(), p.items.data()));
    } else {
      // group the buffered interactions by user, keeping each user's arrival order (windowState list order, :118)
      std::unordered_map<int32_t, int32_t> idx;
      std::vector<int32_t> uids;
      std::vector<int64_t> counts;
      std::vector<int32_t> which(p.users.size());
      for (size_t i = 0; i < p.users.size(); i++) {
        auto f = idx.find(p.users[i]);
        int32_t j;
        if (f == idx.end()) {
          j = int32_t(uids.size());
          idx.emplace(p.users[i], j);
          uids.push_back(p.users[i]);
          counts.push_back(0);
        } else {
          j = f->second;
        }
        which[i] = j;
        counts[j]++;
      }
      std::vector<int64_t> ptr(uids.size() + 1, 0);
      for (size_t j = 0; j < uids.size(); j++) ptr[j + 1] = ptr[j] + counts[j];
      std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
      std::vector<int32_t> grouped(p.items.size());
      for (size_t i = 0; i < p.items.size(); i++) grouped[fill[which[i]]++] = p.items[i];
      COOC_TRY(st.submit(ctx, max_ts, int32_t(uids.size()), uids.data(), ptr.data(), grouped.data()));
    }
    pending_.erase(it);
  }
  COOC_TRY(st.finish(ctx, max_ts, info));
  *fired = 1;
  return Status::Ok();
}

}  // namespace cooc
