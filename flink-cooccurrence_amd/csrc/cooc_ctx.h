// cooc_ctx.h — the context behind the C-ABI handle: one per Flink subtask.
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/cooc.h"
#include "cooc_comm.h"
#include "cooc_device.h"
#include "cooc_sample.h"
#include "cooc_sample_stream.h"
#include "cooc_shard.h"
#include "cooc_stream_kernels.h"

struct cooc_ctx;

namespace cooc {

struct Snapshotter;  // cooc_snapshot_impl.h: packs the streaming state into the snapshot blob and installs one

// The delta rows of the last finished window (device pointers into the producer's buffers), filled in one place by
// each producer: the counter's result (StreamState::count_window; packed lazily by Counter::pack), the owned merge
// of p > 1 subtasks (exchange_window; packed by launch_pack_rows in finish_owned) and the signed delta of a sampled
// window with a minus run (finish_sampled; born packed).
struct WindowDelta {
  // M-row view
  const int64_t *row_base = nullptr;
  const int32_t *row_nnz = nullptr;  // NULL: the window had no rows (nothing emitted, no row touched)
  const int32_t *col = nullptr;
  const uint32_t *cnt = nullptr;
  const int64_t *rowsum = nullptr;  // every item's window row sum (p > 1: all-reduced)
  // packed M-row CSR, ascending columns (pk_rp == NULL: not packed yet)
  int64_t *pk_rp = nullptr;
  int32_t *pk_col = nullptr;
  uint32_t *pk_cnt = nullptr;
  int64_t entries = -1;  // -1: the counter's nnz_total, read with its totals
  int runs = 0;          // counting runs of this subtask that produced it (cooc_last_window_runs)
  bool empty() const { return row_nnz == nullptr; }
};

// Resident streaming state: per-user histories (device arena), global rows (dense uint32
// [n_items x n_items] in HBM), global row sums, the rescorer's observed total, and the outputs of
// the last finished window.  Restates NonSampled...java:129-161 (history), ItemRowRescorer...java:
// 33-41,144-241 (global state, merge, rescoring).
class StreamState {
 public:
  Status submit(cooc_ctx &ctx, int64_t ts, int32_t n_users, const int32_t *user_ids, const int64_t *user_ptr,
                const int32_t *items);
  Status finish(cooc_ctx &ctx, int64_t ts, cooc_window_info *info);
  // sampled mode (cooc_sampling_enable): the window's records in arrival order across users
  Status submit_records(cooc_ctx &ctx, int64_t ts, int64_t n, const int32_t *users, const int32_t *items);
  // on_device: the window's records are decided on the device (cooc_sampling_enable_device, SampleStream); the
  // context may have joined a communicator before (world > 1: the item cut and the feedback go over it)
  Status sampling_enable(cooc_ctx &ctx, int32_t item_cut, int64_t seed, bool on_device);
  bool sampled() const { return sampler_.enabled(); }
  Status sampling_counters(cooc_ctx &ctx, int64_t out[6]);
  // the resident history of a user (slot order) and its userInteractionsTotal; *len = 0 for an unknown user
  Status copy_user_history(cooc_ctx &ctx, int32_t user, int32_t cap, int32_t *items, int32_t *len, int32_t *total);
  // nothing submitted, no window finished, no state restored
  bool pristine() const { return !staged_ && window_seq_ == 0 && h_off_.empty() && !global_ready_; }
  // the last sampled window counted a minus run (a replaced slot that existed before the window)
  int64_t last_window_runs() const { return sampled() && have_window_ ? delta_.runs : 0; }
  Status copy_delta(cooc_ctx &ctx, int32_t *rows, int64_t *row_ptr, int32_t *cols, uint32_t *cnt, int16_t *cnt16);
  // entries of the delta rows [r0, r1) (row indices as in copy_delta): a window streams out in row ranges
  Status copy_delta_range(cooc_ctx &ctx, int32_t r0, int32_t r1, int64_t cap, int32_t *cols, uint32_t *cnt,
                          int16_t *cnt16);
  Status copy_rowsums(cooc_ctx &ctx, int32_t *items, int64_t *delta, int32_t *delta32);
  Status copy_topk(cooc_ctx &ctx, int32_t *rows, int32_t *sizes, int32_t *values, double *scores);
  Status global_rowsums(cooc_ctx &ctx, int64_t *exact, int32_t *v32);
  Status global_row_nnz(cooc_ctx &ctx, int32_t item, int64_t *nnz);
  Status global_row(cooc_ctx &ctx, int32_t item, int32_t *cols, uint32_t *cnt, int16_t *cnt16);
  // the sparse global rows' arena as the host tracks it (cooc_global_slab_stats); zeros with the dense matrix
  void global_slab_stats(int64_t *cap, int64_t *bump, int64_t *live, int64_t *compactions) const {
    *cap = sparse_global_ ? gs_.cap : 0;
    *bump = sparse_global_ ? gs_.bump : 0;
    *live = sparse_global_ ? gs_.live : 0;
    *compactions = sparse_global_ ? gs_.compactions : 0;
  }
  void release();

  int64_t observed_exact = 0;  // UserInteractionCounterObservedCooccurrences (NonSampled...java:80,153)
  int64_t observed_ref = 0;    // ItemRowRescorer observedCooccurrences: long += int delta (:37,154)
  int64_t rowsum_acc = 0;      // RowSumProcessWindowRowSum (RowSumAggregator.java:50,67)
  int64_t rescored_items = 0;  // ItemRowRescorerRescoredItems (ItemRowRescorer...java:60,169)

 private:
  friend struct Snapshotter;
  Status ensure_global(cooc_ctx &ctx);
  int32_t slot_for(int32_t user_id);
  Status window_open(int64_t ts) const;  // no other window is staged
  // room for `need` items of a user: on growth a doubled slab at the arena's end (reloc: old offset, new, length)
  void reserve_history(int32_t slot, int64_t need, std::vector<int64_t> *reloc);
  Status pack_delta(cooc_ctx &ctx);
  Status copy_entries(int64_t e0, int64_t e1, int32_t *cols, uint32_t *cnt, int16_t *cnt16);
  // the entries of a global row in ascending column order (dense matrix: its non-zero cells)
  Status read_global_row(int32_t M, int32_t item, std::vector<int32_t> *cols, std::vector<uint32_t> *cnt);
  Status grow_arena(cooc_ctx &ctx, int64_t need);
  Status finish_sampled(cooc_ctx &ctx, int64_t ts, cooc_window_info *info);
  // the window's decisions: the users with a changed slot and their lists (device pointers), by either sampler
  Status sampled_changes_host(cooc_ctx &ctx, hipStream_t s, std::vector<SmChange> *changed, const int32_t **app,
                              const int32_t **rep);
  Status sampled_changes_device(cooc_ctx &ctx, hipStream_t s, std::vector<SmChange> *changed, const int32_t **app,
                                const int32_t **rep);
  // one run of the window counter over n users' lists at off[] of src (span entries: the arena, or a sampled
  // window's lists): the four arrays uploaded, the planner chosen by the universe's size, the rows left in delta_
  Status count_window(cooc_ctx &ctx, hipStream_t s, int64_t n, const std::vector<int64_t> &off,
                      const std::vector<int32_t> &len, const std::vector<int32_t> &old,
                      const std::vector<int64_t> &cbase, int64_t n_new, const int32_t *src, int64_t span,
                      CountResult *r);
  // a single-subtask window's merge (launch_merge_global over delta_), then finish_tail
  Status merge_and_rescore(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t observed_window, int64_t observed_info,
                           cooc_window_info *info);
  // every window with rows, after its merge kernel: delta_ into the sparse row slabs, the touched rows rescored, the
  // counter's error bits, the accumulators (observed_exact += obs_exact, rowsum_acc += scal[rowsum_slot]), last_
  Status finish_tail(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t obs_exact, int64_t obs_info, int rowsum_slot,
                     cooc_window_info *info);
  Status rescore_touched(cooc_ctx &ctx, hipStream_t s);  // dense or sparse global rows; no-op with topk == 0
  // a window without rows (nothing left after user_cut; no slot changed): nothing emitted, no row touched
  void close_empty_window(cooc_ctx &ctx, int64_t ts, cooc_window_info *info);
  void close_window(cooc_window_info *info);  // the book-keeping of every finished window; *info = last_
  int32_t find_slot(int32_t user_id) const;
  // p > 1 subtasks (a communicator on the context): the window's partial delta rows routed to their owners
  // (a mod world) and merged there, the row-sum deltas and the observed pairs all-reduced
  Status exchange_window(cooc_ctx &ctx, hipStream_t s, const CountResult *r, int64_t obs_local, int64_t *obs_total);
  Status finish_owned(cooc_ctx &ctx, hipStream_t s, int64_t ts, int64_t obs_local, int64_t obs_total,
                      cooc_window_info *info);
  // n_items >= 40,320: one window through the large-universe planner, old / new positions in one pass
  Status count_large_window(cooc_ctx &ctx, hipStream_t s, int64_t n_act, const std::vector<int64_t> &act_off,
                            const std::vector<int32_t> &act_len, const std::vector<int32_t> &act_old,
                            int64_t n_full, CountResult *r, const int32_t *src);

  // ---- persistent state (what a snapshot holds, and what release() names) ----------------------------------
  // host metadata of the per-user histories
  std::unordered_map<int32_t, int32_t> slot_of_;  // user ids outside [0, 2^26)
  std::vector<int32_t> dense_slot_;               // user ids in [0, 2^26)
  std::vector<int64_t> h_off_;
  std::vector<int32_t> h_len_, h_cap_;
  int64_t arena_used_ = 0;
  DevBuf arena_;
  // global state
  bool global_ready_ = false;
  bool sparse_global_ = false;  // n_items >= 40,320: sorted row slabs (gs_) instead of the dense matrix
  GlobalSparse gs_;
  DevBuf d_global_, d_grs_, d_scal_;
  // sampled mode: the decisions' state
  Sampler sampler_;           // (enabled in both modes: it holds the cuts; the device mode never runs its window)
  SampleStream dev_sampler_;  // cooc_sampling_enable_device: the decisions' state on the device
  ItemCutExchange icx_;       // p > 1: the window's per-item histograms and feedbacks over the communicator
  std::vector<uint64_t> icx_words_, icx_all_;  // host mode: this subtask's list, the gathered lists
  std::vector<int32_t> icx_base_, icx_tot_;
  int64_t window_seq_ = 0;

  // ---- the staged window (host) ----------------------------------------------------------------------------
  bool staged_ = false;
  int64_t staged_ts_ = 0;
  int32_t n_staged_ = 0;
  std::vector<int64_t> staged_stamp_;  // per slot: window_seq_ when staged in the current window
  std::vector<int32_t> staged_pos_;    // per slot: index into staged_slots_/staged_items_
  std::vector<int32_t> staged_slots_;
  std::vector<std::vector<int32_t>> staged_items_;  // reused across windows
  // sampled mode: the staged records, the window's changed users
  std::vector<int32_t> rec_users_, rec_items_, rec_slots_;
  std::vector<SmChange> sm_changed_;
  int64_t sm_seq_ = 0;  // device mode: the window's number in staged_stamp_ (counts its distinct slots)

  // ---- per-window device scratch and outputs: nothing in it outlives the next window -----------------------
  DevBuf d_scan_tmp_;  // (also the Snapshotter's scratch)
  struct Scratch {
    // uploads of one window
    DevBuf act_off, act_len, act_old, cbase, new_items, new_dst_ptr, new_dst, reloc;
    // large-universe windows: the users' whole histories and new items side by side (2 lists per user)
    DevBuf lw_items, lw_up2, lw_dsta, lw_dstb, lw_srcb, lw_lenb;
    // sampled windows: the changed users and their lists, the plus run's packed rows set aside, the signed delta
    DevBuf sm_users, sm_app, sm_rep, sm_lists, sm_err, sm_prp, sm_pcol, sm_pcnt, sm_prs;
    SignedDelta sd;
    // p > 1: the owned delta rows (an M-row view over the merge's rows), the all-reduced window row sums, the
    // exchange buffers, and the owned rows packed
    DevBuf own_base, own_nnz, rs_win, x_nnz, x_ent, r_nnz, r_ent, x_h, zero;
    DevBuf own_rp, own_pcol, own_pcnt;
    // the touched rows and their top-k
    DevBuf touched, topk_val, topk_score, topk_size, llr_terms;
  } w_;
  // the last window
  bool have_window_ = false;
  WindowDelta delta_;
  cooc_window_info last_{};
  int32_t n_touched_ = 0;
  // the rows of delta_ with entries and their starts in its packed arrays, for copy-out (once per window)
  bool delta_packed_ = false;
  std::vector<int32_t> delta_rows_;
  std::vector<int64_t> delta_start_;
};

// NonSampledUserInteractionCounterOneInputStreamOperator mirror: late-element drop, tumbling
// window assignment, per-window buffering in arrival order, watermark-driven firing
// (NonSampled...java:84-165).
class Operator {
 public:
  Status process_elements(cooc_ctx &ctx, int64_t n, const int32_t *users, const int32_t *items, const int64_t *ts,
                          int64_t *n_late);
  Status process_watermark(cooc_ctx &ctx, int64_t watermark, int32_t *fired, cooc_window_info *info);

  bool pristine() const { return pending_.empty() && watermark == INT64_MIN && late_elements == 0; }

  int64_t watermark = INT64_MIN;  // timerService.currentWatermark() (this subtask's own)
  int64_t late_elements = 0;      // UserInteractionCounterLateElements

 private:
  friend struct Snapshotter;
  struct Pending {
    std::vector<int32_t> users, items;
  };
  Status fire(cooc_ctx &ctx, int64_t max_ts, bool mine, int32_t *fired, cooc_window_info *info);
  std::map<int64_t, Pending> pending_;  // window.maxTimestamp() -> buffered interactions
  // p > 1: the watermark every subtask has passed (the minimum of their watermarks at the last agreement
  // step; identical on every subtask), and whether the last step fired a window (then the next call runs
  // another step whatever its watermark, so that every subtask runs the same sequence of collectives)
  int64_t agreed_ = INT64_MIN;
  bool regather_ = false;
};

}  // namespace cooc

struct cooc_ctx {
  cooc::Status init(const cooc_config &cfg);
  ~cooc_ctx();

  cooc::Status count_device(int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items, int64_t n_interactions,
                            hipStream_t s, cooc_device_result *out);
  cooc::Status count_device_owned(int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                                  int64_t n_interactions, const int32_t *d_owner, int32_t part,
                                  const int64_t *d_item_counts, int64_t n_total, hipStream_t s,
                                  cooc_device_result *out);
  // user_cut > 0: replaces the CSR by its capped copy (b_cut_*); no-op otherwise
  cooc::Status apply_user_cut(int64_t n_users, const int64_t **d_user_ptr, const int32_t **d_items,
                              int64_t *n_interactions, hipStream_t s);
  cooc::Status finish_batch(const cooc::CountResult &r, hipStream_t s, cooc_device_result *out);
  cooc::Status count_host(int64_t n_users, const int64_t *user_ptr, const int32_t *items, cooc_window_info *info);
  cooc::Status copy_batch(int64_t *row_ptr, int32_t *cols, uint32_t *cnt, int16_t *cnt16, int64_t *rowsum,
                          int32_t *rowsum32);
  cooc::Status topk_batch(int32_t topk, int32_t flags, hipStream_t s);
  // top-k into caller device buffers; d_rowsum_global (may be NULL) replaces the batch's row sums
  // (multi-GPU: the all-reduced row sums, so that k21 and the observed total are the whole log's)
  cooc::Status topk_batch_device(int32_t topk, int32_t flags, const int64_t *d_rowsum_global, int32_t *d_sizes,
                                 int32_t *d_values, double *d_scores, hipStream_t s);
  cooc::Status copy_topk_batch(int32_t *sizes, int32_t *values, double *scores);
  // row ranges of the batch result / its top-k (a JVM operator's copy-out: no single Java array holds a C3 share)
  cooc::Status copy_batch_range(int32_t r0, int32_t r1, int64_t cap, int32_t *cols, uint32_t *cnt, int16_t *cnt16);
  cooc::Status copy_topk_batch_range(int32_t r0, int32_t r1, int32_t topk, int32_t *sizes, int32_t *values,
                                     double *scores);
  cooc::Status topk_owned_host(int32_t topk, int32_t flags);
  cooc::Status comm_allgather_i64(int64_t value, int64_t *out);
  // cooc_verify_batch: invariant checks + row fingerprints of the last batch result
  cooc::Status verify_batch(int32_t flags, uint64_t *d_row_checksum, int64_t *out8, hipStream_t s);
  cooc::Status llr(int64_t n, const int64_t *k, double *out);
  cooc::Status topk_items(int32_t k, int32_t flags, int32_t n, const int32_t *items, int32_t *sizes,
                          int32_t *values, double *scores);

  // the same from host arrays (staged on the context's stream): cooc_count_owned_host
  cooc::Status count_owned_host(int64_t n_users, const int64_t *user_ptr, const int32_t *items, cooc_owned_info *info,
                                cooc_window_info *winfo);
  // multi-GPU large-universe window over the communicator (cooc_owned.hip): cooc_count_owned / cooc_topk_owned
  cooc::Status count_owned(int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items, int64_t n_interactions,
                           hipStream_t s, cooc_owned_info *info, cooc_device_result *out);
  cooc::Status topk_owned(int32_t topk, int32_t flags, int32_t *d_sizes, int32_t *d_values, double *d_scores,
                          int64_t *d_rowsum_global, hipStream_t s);
  // the same window below 40,320 items: the pair records routed to their rows' owners (a mod world) over the
  // communicator, counted there, and the owned rows installed as the batch result through item-indexed views.
  // local: a check of this rank that failed before the call (it still takes part in the agreement)
  cooc::Status count_owned_records(int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                                   int64_t n_interactions, hipStream_t s, cooc_owned_info *info,
                                   cooc_device_result *out, const cooc::Status &local);
  // the small-universe exchange applies (cooc_count_owned's dispatch)
  bool owned_records() const { return comm != nullptr && counter.batch_ok(); }
  // Counter::pack of the batch result, through batch_result's own views when they are the expanded ones
  cooc::Status pack_batch(hipStream_t s, int64_t **row_ptr, int32_t **col, uint32_t **cnt) {
    return counter.pack(s, row_ptr, col, cnt, batch_expanded ? &batch_result : nullptr);
  }

  // cooc_sample_device (cooc_sample_dev.hip): item cut, reservoirs and feedback of a device-resident log
  cooc::Status sample_device(int64_t n_records, const int32_t *d_users, const int32_t *d_items, int32_t n_users,
                             int32_t n_windows, const int64_t *window_ptr, int32_t item_cut, int32_t user_cut,
                             int64_t seed, int64_t *d_res_ptr, int32_t *d_res_items, int64_t res_cap, int32_t *d_total,
                             int16_t *d_item_count, hipStream_t s, cooc_sample_info *info);
  // cooc_sample_owned: the same over the communicator, each rank its own users' records, the draw keyed by
  // d_user_key (NULL: the index); sample_log is the body of both
  cooc::Status sample_owned(int64_t n_records, const int32_t *d_users, const int32_t *d_items, int32_t n_users,
                            const int32_t *d_user_key, int32_t n_windows, const int64_t *window_ptr, int32_t item_cut,
                            int32_t user_cut, int64_t seed, int64_t *d_res_ptr, int32_t *d_res_items, int64_t res_cap,
                            int32_t *d_total, int16_t *d_item_count, hipStream_t s, cooc_sample_info *info);
  cooc::Status sample_log(bool owned, int64_t n_records, const int32_t *d_users, const int32_t *d_items,
                          int32_t n_users, const int32_t *d_user_key, int32_t n_windows, const int64_t *window_ptr,
                          int32_t item_cut, int32_t user_cut, int64_t seed, int64_t *d_res_ptr, int32_t *d_res_items,
                          int64_t res_cap, int32_t *d_total, int16_t *d_item_count, hipStream_t s,
                          cooc_sample_info *info);

  // cooc_parse_interactions_device / cooc_log_prepare_device (cooc_ingest_dev.hip): the text source and the late
  // drop, window assignment and keyBy(user) in front of the operators, for a device-resident log; stateless
  cooc::Status parse_device(const char *d_text, int64_t n_bytes, int64_t cap, int32_t *d_users, int32_t *d_items,
                            int64_t *d_ts, hipStream_t s, int64_t *n_records, int64_t *bad_line);
  cooc::Status log_prepare_device(int64_t n_records, const int32_t *d_users, const int32_t *d_items,
                                  const int64_t *d_ts, int64_t records_per_watermark, int32_t *d_rec_user,
                                  int32_t *d_rec_item, int32_t *d_user_ids, int64_t *d_user_ptr, int32_t *d_user_items,
                                  int64_t *window_ptr, int64_t *window_ts, int64_t cap_windows, hipStream_t s,
                                  cooc_log_info *info);

  static std::string &create_error();

  cooc_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  cooc::Counter counter;
  cooc::KernelTimer timer;
  cooc::StreamState stream_state;
  cooc::Sharder sharder;
  cooc::CountResult batch_result;
  cooc::Operator op;

  // stateless batch buffers
  cooc::DevBuf b_user_ptr, b_items, b_tk_size, b_tk_val, b_tk_score, b_obs3, b_llr_terms;
  // user_cut > 0: the capped copy of a count_device CSR (first user_cut items of every user)
  cooc::DevBuf b_cut_ptr, b_cut_items, b_cut_tmp;
  cooc::DevBuf b_verify;  // cooc_verify_batch totals
  cooc::DevBuf b_smp_state, b_smp_win;  // cooc_sample_device: the call's carried state, one window's scratch
  // cooc_sample_owned at world > 1: the agreement's words, then a window's header, histogram and feedback list;
  // the gathered lists
  cooc::DevBuf b_smp_lists;
  cooc::ItemCutExchange smp_icx;
  // the device ingest calls' scratch; aux: the line breaks of a parse, the window lists of a preparation
  cooc::DevBuf b_ingest, b_ingest_aux;
  // checkpoints (cooc_snapshot_*.hip): the packed image of cooc_snapshot_prepare (snap_bytes < 0: none), the blob a
  // restore is writing (restore_bytes < 0: none) and their scratch
  cooc::DevBuf snap_img, snap_rp, snap_col, snap_cnt, snap_live, snap_tmp, snap_tmp2, snap_sums, restore_img;
  int64_t snap_bytes = -1, restore_bytes = -1;
  // a restore from parts in progress (non-empty): part i is restore_part_len[i] bytes at restore_part_off[i] of
  // restore_img, all parts resident at once
  std::vector<int64_t> restore_part_off, restore_part_len;
  void snapshot_release();  // frees the image (cooc_snapshot_release; implied by the next finish_window / restore)
  // the communicator (cooc_comm_init*) and the owned-rows exchange's buffers
  std::unique_ptr<cooc::Comm> comm;
  cooc::DevBuf own_counts, own_sort, own_tmp, own_sizes, own_owner, own_lens, own_up, own_items, own_obs, own_rowsum;
  // the records exchange of cooc_count_owned (n_items < 40,320): the local plan (descriptors by owner, row counts in
  // owner-major order, the u16 arena), the agreement's records, the gathered arenas (the send slot after them), the
  // received row counts and descriptors, and the item-indexed views of the owned rows (base, nnz, row sums)
  cooc::DevBuf rec_desc, rec_rc, rec_arena, rec_agree, rec_arena_all, rec_rrc, rec_rdesc, rec_base, rec_nnz, rec_rs;
  int32_t batch_topk = 0;
  int32_t batch_topk_flags = 0;
  bool have_batch = false;
  // batch_result's row_base / row_nnz / rowsum are item-indexed views over the counter's compact owned rows
  // (count_owned_records): every reader takes them, not the counter's own arrays
  bool batch_expanded = false;
  bool batch_owned = false;  // the last batch counted only the rows of one part (cooc_count_device_owned)
  int64_t batch_observed = 0;
  int64_t batch_nnz = 0;
  // the batch result packed for range copies (once per batch): its row offsets on the host
  bool batch_packed = false;
  std::vector<int64_t> batch_rp_host;
  int64_t *batch_pk_rp = nullptr;
  int32_t *batch_pk_col = nullptr;
  uint32_t *batch_pk_cnt = nullptr;
};
