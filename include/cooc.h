/*
 * cooc.h — C-ABI of the MI355X co-occurrence core (pair expansion + keyed (itemA,itemB) count
 * reduction, the non-sampled path of uce/flink-cooccurrence).
 *
 * Boundary.  The entry points replace, for the `--skip-cuts` job graph of
 * FlinkCooccurrences.java:65-74,135-167, everything between the keyBy(user) edge and the sink:
 *
 *   reference (file:line, under src/main/java/com/github/uce/flinkcooccurrences/)   replaced by
 *   ------------------------------------------------------------------------------  -------------------------------
 *   NonSampledUserInteractionCounterOneInputStreamOperator.processElement :84-110   cooc_op_process_elements
 *   NonSampledUserInteractionCounterOneInputStreamOperator.onEventTime    :113-165  cooc_op_process_watermark /
 *     (+ ItemCooccurrences record & Kryo codec, ItemCooccurrences.java:14-149)        cooc_submit_batch +
 *   ItemRowAggregator.ItemCooccurrenceRowAggregateFunction.add            :26-31      cooc_finish_window
 *   ItemRowAggregator.ItemCooccurrenceRowWindowFunction.process           :50-56    cooc_copy_window_delta
 *   RowSumAggregator.RowSumAggregateFunction.add / RowSumProcessWindow    :25-71    cooc_copy_window_rowsums
 *   ItemRowRescorerTwoInputStreamOperator.processWatermark..scoreItem     :116-241  cooc_copy_window_topk
 *   LogLikelihood.logLikelihoodRatio                                       :41-57    (inside the rescoring kernel)
 *   IntDoublePriorityQueue add/update/iterator                             :132-242  (heap layout of topk output)
 *   UserInteractionCounterObservedCooccurrences / LateElements /
 *   RowSumProcessWindowRowSum / ItemRowRescorerRescoredItems accumulators            cooc_op_counters
 *
 * plus the sampled pipeline of FlinkCooccurrences.java:65-130 (item cut, per-user reservoir with retractions,
 * feedback) as a mode of the same streaming entry points (cooc_sampling_enable, "sampled mode" below), and
 * one stateless entry point over a device-resident CSR of user histories
 * (cooc_count_device): one tumbling window over empty histories, the unit the benchmark times.
 *
 * Conventions:
 *  - Every function returns an int status (COOC_OK = 0); the message of the last failure on a
 *    context is cooc_last_error(ctx).  The Java wrapper rethrows IllegalStateException /
 *    IllegalArgumentException where the reference throws them.
 *  - The library never retains caller pointers after a call returns.  Results are either copied
 *    into caller buffers (two-phase: sizes from cooc_window_info, then cooc_copy_*), or handed
 *    out as BORROWED device views that stay valid until the next call on the same context.
 *  - One context per Flink subtask; a context is not thread-safe, distinct contexts are.
 *  - Item ids must lie in [0, cfg.n_items); user ids are arbitrary int32 (keyed state).
 *  - Counts are exact (uint32, overflow is detected and reported as COOC_ERR_OVERFLOW); the
 *    reference's own int16 (Int2ShortOpenHashMap) and int32 (Int2IntOpenHashMap / IntValue) wrapped
 *    views are produced by the copy functions ("ref_compat").
 *  - There is no CPU fallback: without a usable HIP device every compute entry point fails with
 *    COOC_ERR_HIP.
 *  - Streams.  An entry point that takes device pointers and a `hip_stream` runs its kernels on that
 *    stream; NULL is the HIP null stream (which orders with hipMemcpy and with torch's default
 *    stream).  The caller must have ENQUEUED the work producing the inputs on the same stream (or
 *    ordered it before, e.g. with an event); the library never reads caller buffers from another
 *    stream.  Entry points that return host values (sizes, counts) synchronise that stream first.
 *  - No C++ exception crosses this boundary: host allocation failures return COOC_ERR_OOM, any
 *    other internal exception COOC_ERR_STATE, with the message in cooc_last_error.
 */
#ifndef COOC_H_
#define COOC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COOC_ABI_VERSION 7

#if defined(__GNUC__)
#define COOC_API __attribute__((visibility("default")))
#else
#define COOC_API
#endif

enum cooc_status {
  COOC_OK = 0,
  COOC_ERR_ARG = 1,      /* IllegalArgumentException in the reference */
  COOC_ERR_STATE = 2,    /* IllegalStateException in the reference */
  COOC_ERR_HIP = 3,      /* HIP runtime / no device */
  COOC_ERR_OOM = 4,      /* device allocation failed */
  COOC_ERR_OVERFLOW = 5  /* an exact uint32 count overflowed */
};

/* cooc_config.flags. */
#define COOC_FLAG_EXACT_SCORES 1 /* LLR on exact counts instead of the reference's wrapped int16/int32 */
/* Layout of a cooc_count_device result (default: automatic, dense when the ordered pairs cover at
 * least half of the n_items^2 matrix and it fits in HBM, else the padded CSR). */
#define COOC_FLAG_OUTPUT_CSR 2   /* always the padded CSR (row_base, row_nnz, col, cnt) */
#define COOC_FLAG_OUTPUT_DENSE 4 /* always the dense matrix (dense, row_nnz) */
/* Route every window through the large-universe planner (the path for n_items >= 40,320: per-row LDS
 * hash / dense-tile chunks) even when the batch planner applies; same results (A/B and tests). */
#define COOC_FLAG_GENERAL_PLANNER 8
/* Large universes: every whole row through the sort + segmented-reduce path (packed 64-bit (row, column)
 * pair keys, radix-sorted, runs counted) instead of the LDS hash / dense-tile chunks.  That path always
 * takes the rows whose LDS hash table overflows; the flag sends all of them (A/B and tests). */
#define COOC_FLAG_SORT_ROWS 16
/* Large universes, batch windows: keep the columns of a row in ascending id order.  By default the
 * large-universe path renumbers the columns of a batch so that its first 16,384-column tile holds the
 * batch's 16,384 most frequent items (that batch's item counts, or the global counts of
 * cooc_count_device_owned): column c < 16,384 is the c-th of those hot items in ASCENDING id order, and
 * every other item b is column b + 16,384 (the hot items leave holes there).  The renumbering is skipped
 * -- identity order -- when at least 15/16 of the hot items already have ids below 16,384 (ids numbered by
 * popularity), and for universes of one tile.  A device result's rows are in this column order, which is
 * also the order the rescorer scores them in (the top-k tie order); cooc_copy_column_order reports it.
 * The host copies (cooc_copy_batch) are always in ascending id order.  This flag keeps id order on the
 * device at the price of the renumbering's gain (ids not numbered by popularity run up to ~1.8x slower). */
#define COOC_FLAG_COLUMN_ORDER 32
/* Large universes, batch results: a row's entries may come out in any order (the row holds the same keys and
 * counts).  Without it every row is in the result's column order, which costs the LDS hash chunks a column
 * ranking of their keys; the reference's own row is an Int2ShortOpenHashMap, iterated in slot order
 * (ItemRowAggregator.java:50-56, ItemRowRescorer...java:195), so a consumer that builds maps from the rows
 * (the Flink rows operators) or only sums them needs no order.  The host copies (cooc_copy_batch,
 * cooc_copy_batch_range) still sort every row; the top-k of an unordered result feeds each heap in the row's
 * order (ties may resolve differently, as between two fastutil builds); cooc_verify_batch checks keys,
 * counts and sums but not the order (and not the symmetry: [5] = -1); cooc_partition_plan refuses such a
 * result (the partial-row merge needs ordered rows).  Streaming windows always keep column order. */
#define COOC_FLAG_ANY_ORDER 64

typedef struct cooc_ctx cooc_ctx;

typedef struct cooc_config {
  int32_t device;         /* HIP device ordinal; -1 = the current device */
  int32_t n_items;        /* item-id universe: ids in [0, n_items) */
  int32_t topk;           /* ItemRowRescorer topK (ItemRowRescorer...java:51-56, Configuration.java:153);
                             0 disables rescoring */
  int32_t flags;          /* COOC_FLAG_* */
  int64_t window_size_ms; /* TumblingEventTimeWindows.of(Time.of(windowSize, windowUnit)),
                             NonSampled...java:61-62, in milliseconds */
  int32_t user_cut;       /* kMax: 0 = off (the non-sampled path).  1..32767 (a Java short,
                             UserInteractionCounter...java:54,76): only the first user_cut
                             interactions of every user (arrival order, over all windows) are
                             expanded -- the `userInteractions < userCut` branch of
                             UserInteractionCounter...java:168-205; later interactions are dropped.
                             After cooc_sampling_enable it is the reservoir size of the sampled
                             streaming mode (the reservoir branch, :206-240, with retractions);
                             the batch calls keep the first-user_cut cap either way */
  int32_t reserved;
} cooc_config;

/* Sizes of one fired window's outputs (two-phase copy protocol). */
typedef struct cooc_window_info {
  int64_t ts;             /* window.maxTimestamp(): timestamp of every output record, NonSampled...java:115 */
  int64_t nnz;            /* entries over all delta rows */
  int64_t observed;       /* exact ordered pairs of the window: sum of 2*|history| (NonSampled...java:153) */
  int32_t n_rows;         /* items with a delta row (= items with a row-sum update) */
  int32_t topk;           /* columns of the top-k output (cfg.topk) */
  int32_t n_topk;         /* rescored rows (n_rows when topk > 0, else 0) */
  int32_t reserved;
} cooc_window_info;

/* Borrowed device views of a cooc_count_device result (valid until the next call on ctx).  Exactly
 * one layout is set: the padded CSR (row_base, col, cnt non-NULL, dense NULL) or the dense matrix
 * (dense non-NULL, row_base / col / cnt NULL).  Both key sets are the reference's touched keys: a
 * key exists iff its count is > 0 (every increment is +1, ItemRowAggregator.java:29). */
typedef struct cooc_device_result {
  int64_t n_items;
  int64_t nnz;            /* total entries (keys with a count > 0) */
  int64_t observed;       /* exact ordered pairs sum_u n_u (n_u - 1) */
  const int64_t *row_base;  /* [n_items]: first entry of row a in col/cnt (rows padded, not packed) */
  const int32_t *row_nnz;   /* [n_items]: entries of row a (both layouts) */
  const int32_t *col;       /* item ids, ascending within a row in the result's column order: the id itself,
                               or, for a renumbered large-universe batch (n_items >= 40,320 without
                               COOC_FLAG_COLUMN_ORDER), the hot items first in id order, then the others in
                               id order (see COOC_FLAG_COLUMN_ORDER, cooc_copy_column_order) */
  const uint32_t *cnt;      /* exact counts */
  const int64_t *rowsum;    /* [n_items]: exact row sums sum_b C[a,b] */
  const uint32_t *dense;    /* [n_items * n_items] row-major exact counts, 0 = key absent */
} cooc_device_result;

/* ---- lifecycle ------------------------------------------------------------------------------ */
COOC_API int cooc_abi_version(void);
COOC_API const char *cooc_status_string(int status);
COOC_API int cooc_create(const cooc_config *cfg, cooc_ctx **out);
/* create(cfg{devices[]}) of SURVEY §8(b): one handle per Flink subtask over the node's GPUs.  The
 * handle binds to devices[subtask % n_devices] (cfg->device is ignored); every other field as in
 * cooc_create.  A device ordinal outside [0, hipGetDeviceCount()) is COOC_ERR_ARG. */
COOC_API int cooc_create_on(const cooc_config *cfg, const int32_t *devices, int32_t n_devices, int32_t subtask,
                            cooc_ctx **out);
COOC_API void cooc_destroy(cooc_ctx *ctx);
COOC_API const char *cooc_last_error(const cooc_ctx *ctx);

/* ---- stateless one-window batch over a device CSR (the benchmarked unit) ----------------------
 * d_user_ptr: int64[n_users+1] offsets into d_items (device memory); d_items: int32[n_interactions]
 * in per-user arrival order.  hip_stream: a hipStream_t (NULL = the HIP null stream).
 * Computes C = sum over users of the ordered position pairs (p != q) -> (x_p, x_q), i.e. exactly
 * what NonSampled...java:113-165 emits for users whose histories start empty, reduced by
 * ItemRowAggregator/RowSumAggregator.  Does not touch the context's streaming state. */
COOC_API int cooc_count_device(cooc_ctx *ctx, int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                      int64_t n_interactions, void *hip_stream, cooc_device_result *out);
/* Multi-GPU for large item universes (n_items >= 40,320, the C3 / C5 configs): the keyBy(itemA) of
 * FlinkCooccurrences.java:152 as row ownership.  Counts only the rows a with d_owner[a] == part, over
 * every user given (the all-gathered log of all parts); rows owned by other parts come out empty.
 * d_item_counts int64[n_items]: the global log's item frequencies (n_total interactions in all),
 * which size the planner; out->observed = the ordered pairs of the owned rows (their sum over the
 * parts is the log's sum_u n_u (n_u - 1)).  Same borrowed padded-CSR result as cooc_count_device. */
COOC_API int cooc_count_device_owned(cooc_ctx *ctx, int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                                     int64_t n_interactions, const int32_t *d_owner, int32_t part,
                                     const int64_t *d_item_counts, int64_t n_total, void *hip_stream,
                                     cooc_device_result *out);
/* Item frequencies of a device item array (d_items int32[n_interactions]) into d_counts int64[n_items]
 * (device, overwritten) on hip_stream: the local part of the global frequencies that
 * cooc_count_device_owned's caller all-reduces (owner map, planner estimate).  Ids outside
 * [0, n_items) are not counted.  Each workgroup counts the items it meets most in an LDS table (the
 * Zipf head, whatever its ids) and sends the rest to global 64-bit atomics. */
COOC_API int cooc_item_counts(cooc_ctx *ctx, const int32_t *d_items, int64_t n_interactions, int64_t *d_counts,
                              void *hip_stream);
/* The column order of the last batch result's device rows (and of its top-k iteration, the tie order):
 * rank_of int32[n_items] gets the position of every item in that order -- after a large-universe
 * renumbering, c for the c-th hot item (ascending ids) and id + 16,384 for every other item; else the id
 * itself (see COOC_FLAG_COLUMN_ORDER for when the renumbering happens).  Only the relative order counts. */
COOC_API int cooc_copy_column_order(cooc_ctx *ctx, int32_t *rank_of);
/* Same from host buffers; afterwards cooc_copy_batch copies the packed CSR out. */
COOC_API int cooc_count_host(cooc_ctx *ctx, int64_t n_users, const int64_t *user_ptr, const int32_t *items,
                    cooc_window_info *info);
/* Packed CSR over ALL n_items rows: row_ptr int64[n_items+1]; cols/cnt/cnt16 [nnz];
 * rowsum int64[n_items], rowsum32 int32[n_items].  Any pointer may be NULL. */
COOC_API int cooc_copy_batch(cooc_ctx *ctx, int64_t *row_ptr, int32_t *cols, uint32_t *cnt, int16_t *cnt16, int64_t *rowsum,
                    int32_t *rowsum32);

/* The entries of batch rows [row_begin, row_end) only, in cooc_copy_batch's packed order (row_ptr from a
 * cooc_copy_batch call with cols/cnt/cnt16 NULL): cols/cnt/cnt16 hold at least `cap` entries; a range of more
 * entries than cap is COOC_ERR_ARG and nothing is written.  A JVM operator streams a result larger than one
 * Java array (a C3 share: ~7e9 entries; an owner's rows: ~4e9) out in row ranges (ItemRowAggregator.java:50-56's
 * one map per row).  The packed view is built once per batch. */
COOC_API int cooc_copy_batch_range(cooc_ctx *ctx, int32_t row_begin, int32_t row_end, int64_t cap, int32_t *cols,
                                   uint32_t *cnt, int16_t *cnt16);
/* LLR top-k of every row of the last cooc_count_device / cooc_count_host result: what
 * ItemRowRescorer...java:195-241 emits after that one window from an empty state (rows iterated in
 * ascending column order, LogLikelihood.java:41-57 scores, IntDoublePriorityQueue layout).  flags:
 * COOC_FLAG_EXACT_SCORES to score exact counts instead of the reference's wrapped int16/int32.
 * cooc_copy_topk_batch: sizes int32[n_items], values int32[n_items*topk], scores double[n_items*topk]
 * (heap positions 1..size, least score first; rows without entries have size 0). */
/* hip_stream NULL = the context's own stream (no caller stream is kept between calls: the count this
 * scores has drained before cooc_count_device returned, and cooc_topk_batch synchronises the stream it
 * runs on before returning). */
COOC_API int cooc_topk_batch(cooc_ctx *ctx, int32_t topk, int32_t flags, void *hip_stream);
COOC_API int cooc_copy_topk_batch(cooc_ctx *ctx, int32_t *sizes, int32_t *values, double *scores);
/* The same top-k into caller DEVICE buffers on hip_stream (ordered after the count on the caller's
 * stream; the C5 config keeps its output resident): d_sizes int32[n_items], d_values
 * int32[n_items*topk], d_scores double[n_items*topk].  d_rowsum_global (device int64[n_items], may be
 * NULL) replaces the result's own row sums: multi-GPU owners pass the all-reduced row sums (the
 * broadcast row-sum stream, FlinkCooccurrences.java:163), so that k21 = rowSum(b) - k11 and the
 * observed total (ItemRowRescorer...java:154,203-240) are the whole log's; rows the context does not
 * own have no entries and get size 0. */
COOC_API int cooc_topk_batch_device(cooc_ctx *ctx, int32_t topk, int32_t flags, const int64_t *d_rowsum_global,
                                    int32_t *d_sizes, int32_t *d_values, double *d_scores, void *hip_stream);
/* LogLikelihood.logLikelihoodRatio (LogLikelihood.java:41-57) evaluated by the device function the
 * rescoring kernels use: k = host int64[n][4] of (k11, k12, k21, k22), out = host double[n].  For
 * known-answer tests of the device scores (LogLikelihoodTest.java:14-16). */
COOC_API int cooc_llr(cooc_ctx *ctx, int64_t n, const int64_t *k, double *out);
/* The SURVEY §8(b) query topk(handle, items[], k): the top-k of the rows `items` (n of them) of the
 * last batch result, computing the batch top-k first when it has not run with this (k, flags).
 * out_sizes int32[n], out_items int32[n*k], out_scores double[n*k] (heap positions 1..size as in
 * cooc_copy_topk_batch).  The rescorer's per-row query (ItemRowRescorer...java:195-241 for the
 * given rows only); an item outside [0, n_items) is COOC_ERR_ARG. */
COOC_API int cooc_topk_items(cooc_ctx *ctx, int32_t k, int32_t flags, int32_t n, const int32_t *items,
                             int32_t *out_sizes, int32_t *out_items, double *out_scores);

/* ---- streaming (resident per-user histories, global rows, row sums) ------------------------
 * cooc_submit_batch stages the interactions of one tumbling window: n_users users with their
 * new items in arrival order (user_ptr int64[n_users+1] into items).  Several submits to the same
 * window append.  cooc_finish_window expands every staged user against its resident history,
 * reduces the window's delta rows and row sums, merges them into the global state and, if
 * topk > 0, rescores every touched row (ItemRowRescorer...java:144-228).
 * Across GPUs (a communicator of world > 1 on ctx, cooc_comm_init / cooc_comm_init_ops; any item universe: below
 * 40,320 items the owners keep dense global rows, above it sorted row slabs): each context holds the resident histories of ITS users (a keyBy(user) shard,
 * FlinkCooccurrences.java:70) and cooc_finish_window is collective: every rank expands its own users, the
 * partial delta rows go to their owners (row a on rank a mod world: the keyBy(item) of :152), the row-sum
 * deltas and the window's pairs are all-reduced (the broadcast of :163), and each owner merges its rows into
 * its resident global rows and rescores them against the job's row sums.  The window's outputs on a rank
 * are its owned rows (every row of the job on exactly one rank); info->observed is this rank's users' pairs
 * (the ObservedCooccurrences accumulator; the ranks' values add up to the job's).  Every rank finishes the
 * same windows in the same order: cooc_op_process_watermark decides from all-gathered state only (the ranks'
 * watermarks and earliest pending windows), so ranks that receive different watermark sequences still run the
 * same collectives, and a rank without records in a window still joins it.
 * In the sampled mode (cooc_sampling_enable) the CSR order of cooc_submit_batch -- submit after submit, user after
 * user, item after item -- is taken as the window's arrival order. */
COOC_API int cooc_submit_batch(cooc_ctx *ctx, int64_t window_ts, int32_t n_users, const int32_t *user_ids,
                      const int64_t *user_ptr, const int32_t *items);
COOC_API int cooc_finish_window(cooc_ctx *ctx, int64_t window_ts, cooc_window_info *info);

/* Delta rows of the last finished window (ItemCooccurrenceRowWindowFunction output):
 * rows int32[n_rows] ascending, row_ptr int64[n_rows+1], cols/cnt/cnt16 [nnz].  NULLs skipped. */
COOC_API int cooc_copy_window_delta(cooc_ctx *ctx, int32_t *rows, int64_t *row_ptr, int32_t *cols, uint32_t *cnt,
                           int16_t *cnt16);
/* The entries of delta rows [row_begin, row_end) only (row indices as in cooc_copy_window_delta's rows[]):
 * cols/cnt/cnt16 [row_ptr[row_end] - row_ptr[row_begin]], each holding at least `cap` entries: a range of
 * more entries than cap is COOC_ERR_ARG and nothing is written.  A window whose delta holds more entries than
 * one Java array can (2^31 - 1) streams out in row ranges: first cooc_copy_window_delta(rows, row_ptr,
 * NULL, NULL, NULL), then ranges sized from row_ptr.  The packed copy-out view is built once per window. */
COOC_API int cooc_copy_window_delta_range(cooc_ctx *ctx, int32_t row_begin, int32_t row_end, int64_t cap, int32_t *cols,
                                          uint32_t *cnt, int16_t *cnt16);
/* Row-sum updates of the last window, one per delta row (same order as rows): exact int64 and the
 * reference's int view (RowSumAggregator.java:25-27; the reference drops an update whose int
 * value is 0, RowSumAggregator.java:66 -- the caller applies that filter on delta32). */
COOC_API int cooc_copy_window_rowsums(cooc_ctx *ctx, int32_t *items, int64_t *delta, int32_t *delta32);
/* Top-k of every rescored row: rows int32[n_topk], sizes int32[n_topk],
 * values int32[n_topk*topk], scores double[n_topk*topk] in IntDoublePriorityQueue heap order
 * (positions 1..size, least score first: IntDoublePriorityQueue.java:215-242). */
COOC_API int cooc_copy_window_topk(cooc_ctx *ctx, int32_t *rows, int32_t *sizes, int32_t *values, double *scores);

/* Global state snapshots. */
COOC_API int cooc_global_rowsums(cooc_ctx *ctx, int64_t *exact, int32_t *v32);          /* [n_items] each */
COOC_API int cooc_global_observed(cooc_ctx *ctx, int64_t *exact, int64_t *rescorer);   /* rescorer: sum of int deltas */
COOC_API int cooc_global_row_nnz(cooc_ctx *ctx, int32_t item, int64_t *nnz);
COOC_API int cooc_global_row(cooc_ctx *ctx, int32_t item, int32_t *cols, uint32_t *cnt, int16_t *cnt16);

/* ---- operator mirror: NonSampledUserInteractionCounterOneInputStreamOperator + aggregators ----
 * cooc_op_process_elements: Tuple3(user,item,ts) records in arrival order; records with
 * ts <= current watermark are dropped and counted (NonSampled...java:89-91).
 * cooc_op_process_watermark: advances the watermark and fires AT MOST ONE pending window with
 * maxTimestamp <= watermark (the earliest); sets *fired = 1 and fills *info if one fired (its
 * outputs are then readable with cooc_copy_window_*), *fired = 0 when nothing is due.  Callers
 * loop until *fired == 0, which mirrors the Flink timer service firing timers in timestamp order.
 * With a communicator of world > 1 the call is collective and a window is due when its maxTimestamp is at or
 * below the MINIMUM watermark over the ranks (agreed by an all-gather of the watermarks and of the earliest
 * pending windows); a rank whose watermark is ahead of that minimum waits inside the call until the other
 * ranks' watermarks catch up (every rank receives Long.MAX_VALUE at the end of a bounded input). */
COOC_API int cooc_op_process_elements(cooc_ctx *ctx, int64_t n, const int32_t *users, const int32_t *items,
                             const int64_t *ts, int64_t *n_late);
COOC_API int cooc_op_process_watermark(cooc_ctx *ctx, int64_t watermark, int32_t *fired, cooc_window_info *info);
/* counters[0] UserInteractionCounterLateElements, [1] UserInteractionCounterObservedCooccurrences,
 * [2] RowSumProcessWindowRowSum, [3] ItemRowRescorerRescoredItems, [4] rescorer observed. */
COOC_API int cooc_op_counters(cooc_ctx *ctx, int64_t *counters5);

/* ---- sampled mode: item cut and per-user reservoir with retractions ------------------------------------
 * The reference's default pipeline (FlinkCooccurrences.java:65-130): ItemInteractionCounterTwoInputStreamOperator
 * applies itemCut, UserInteractionCounterOneInputStreamOperator applies userCut and a per-user reservoir and
 * retracts pairs when a reservoir slot is replaced, and a feedback edge hands rejected samples back to the item
 * counters.  The reference's own run is not reproducible (one java.util.Random per subtask consumed in timer
 * order, an asynchronous feedback queue); this mode is its algorithm with those two races serialised, restating
 * ItemInteractionCounter...java:119-143, :94-116 and UserInteractionCounter...java:145-257.  One GPU or several
 * (a communicator joined before the mode is enabled: "Sampled mode at world > 1" below), both item
 * universes; streaming entry points only (cooc_count_device and friends keep the first-user_cut cap; a log in
 * device memory reaches them through cooc_sample_device below, which returns the reservoirs as their input CSR).
 *
 * Two entry points enable it and differ only in where steps 1-3 below are decided: cooc_sampling_enable on the
 * host (the calling thread, record by record), cooc_sampling_enable_device on the GPU (data-parallel, the form
 * stated at cooc_sample_device below).  The outputs are identical.
 *
 * When a window fires, its records are processed in arrival order (cooc_op_process_elements keeps it across
 * users; cooc_submit_batch: its CSR order):
 *
 * 1. Item cut.  For each record (u, i) in arrival order:
 *    - If itemInteractions[i] < item_cut, then itemInteractions[i]++ and sample = true.
 *    - Otherwise sample = false.
 * 2. User stage.  For each record of user u, in arrival order:
 *    - total[u]++, also for unsampled records.
 *    - If sample:
 *      - If |H_u| < user_cut, append the item.  This is the existing fill branch.
 *      - Otherwise draw k (formula below).
 *        - If k < user_cut, set H_u[k] = i (a replacement).
 *        - Otherwise queue the feedback (i, -1).
 * 3. Feedback.  After every record of the window, apply the queued feedback: itemInteractions[i] -= 1.
 *    - It is applied at the end of the window in which it arose, before any later window's item cut.
 *    - This serialises the reference's asynchronous queue.
 *    - An evicted item's counter is not decremented, as in the reference.
 *
 * The draw.
 *    k = ((splitmix64(seed ^ ((uint64)(uint32)u << 32 | (uint32)total[u])) >> 32) * total[u]) >> 32
 *    with the splitmix64 spelled out at cooc_verify_batch below.  The draw is counter-based, so it does not depend
 *    on the order in which users are visited.  It is uniform on [0, total) up to total / 2^32.
 *
 * Outputs of a window.  Let H_u and H'_u be a user's reservoir before and after the window.  A slot is changed if
 * it was appended or replaced at least once, whatever value it ends with.
 *  - Delta entries.  The window's delta row a has an entry for column b iff, for some active user, (a, b) is an
 *    ordered pair of two distinct slots of H'_u or of H_u, at least one of them changed.
 *  - Delta counts.  The count is the signed net: pairs of that kind in H' minus pairs of that kind in H, summed
 *    over users.  The count may be 0 or negative.  Over a window this equals the sum of the reference's emitted
 *    +-1 records (the fill and replacement emissions telescope to C(H') - C(H)); keys that the reference touches
 *    only through a slot that is overwritten again within the same window do not appear here.
 *  - Row sums.  Row-sum deltas are the signed row sums of those counts.
 *  - Copy-out.  cooc_copy_window_delta* returns the counts as two's complement in the same uint32 buffer; cnt16
 *    is the low 16 bits, which is the reference's short arithmetic; delta32 is as in the non-sampled mode.
 *  - observed.  info.observed and cooc_op_counters [1] count fills only, |H'|(|H'|-1) - |H|(|H|-1)
 *    (UserInteractionCounter...java:195).  The rescorer's observed stays the sum of the int row-sum deltas.
 *  - Global state.  Every count is >= 0 and equals the pair count over all current reservoirs.  A global key
 *    exists iff its exact count is > 0: cooc_global_row, cooc_global_row_nnz and the rescoring do not report a
 *    key whose count went back to 0.
 *  - Rescored rows.  Every row with a delta entry is rescored, also when all its nets are 0.
 *  - A user whose window changes no slot (only rejections and feedback) contributes nothing; a window in which
 *    no user changes a slot is an empty window (n_rows = 0), but its item counters, totals and feedback are
 *    still applied.
 *
 * Sampled mode at world > 1.  The call order is: join the communicator (cooc_comm_init*), then enable sampling.  A
 * communicator of world 1 behaves exactly as none.  At world W > 1 a window fires on all ranks together, as in the
 * non-sampled mode.  Let R_r be rank r's records of that window in its local arrival order.
 *
 *    The job's arrival order for the window is R_0 || R_1 || ... || R_{W-1} (rank-major).
 *
 * Steps 1-3 apply to that order, unchanged.  This is one more serialisation of a race the reference leaves open:
 * its item counter receives the upstream subtasks' records in arbitrary interleaving.
 *  - State.  A user's records all arrive on one rank (as in the non-sampled p > 1 mode); reservoirs, lengths and
 *    totals live on that rank, and the draw stays keyed by (seed, user id, total).  itemInteractions[] is
 *    replicated: identical on every rank after every window, also for items of which a rank saw no record and on
 *    a rank with no records at all.
 *  - The equivalent data-parallel form, which is what runs.  h_q[i] = records of item i in R_q; base_r[i] =
 *    sum over q < r of h_q[i].  A record of item i on rank r, with rank rho among rank r's window records of i, is
 *    sampled iff count[i] + base_r[i] + rho < item_cut.  The user stage (fill, replace, feed back) is local.  With
 *    f_q[i] the feedbacks that arose on rank q, every rank ends the window with
 *    count[i] += min(sum_q h_q[i], max(0, item_cut - count[i])) - sum_q f_q[i].
 *    Each window the ranks all-gather their (item << 32 | records) histograms, sorted by item, and then the items
 *    of their feedbacks, 8 bytes per entry, each list padded to the longest.
 *  - Outputs.  Each rank emits its owned rows (row a on rank a mod W).  A delta entry exists iff it exists in the
 *    single-context contract applied to the serialised window, including an entry whose nets cancel across ranks
 *    (count 0).  Every owned row with a delta entry is rescored against the all-reduced row sums.  info.observed
 *    and cooc_op_counters [1] count this rank's fills; the ranks' values add up to the job's.
 *    cooc_sampling_counters [0..4] count this rank's own records and users, [5] is the job's value, the same on
 *    every rank.  cooc_last_window_runs is the rank's own value (0, 1 or 2); ranks may differ.  A window in which
 *    no rank changes a slot is an empty window on every rank; counters, totals and feedback still apply.
 *  - Consequence: the union of the ranks' outputs and state equals, bit for bit, a single sampled context fed each
 *    window as R_0 || ... || R_{W-1}: deltas, cnt16, row sums, heaps and scores, global rows, reservoirs, totals
 *    and item counters.  Both decision modes keep their promise of identical outputs.
 *  - Not yet: checkpoints of a sampled multi-rank job.  At world > 1 cooc_sampling_snapshot_prepare,
 *    cooc_sampling_restore_* and cooc_restore_*_parts return COOC_ERR_STATE and say so.  A follow-up.
 *
 *   cooc_sampling_enable    item_cut in 1..32767 (a Java short, ItemInteractionCounter...java:37; else
 *                           COOC_ERR_ARG); cfg.user_cut becomes the reservoir size.  Only on a context with
 *                           cfg.user_cut > 0 and without streaming state (as cooc_restore_begin); otherwise
 *                           COOC_ERR_STATE.  The context may have joined a communicator before.  A sampled context
 *                           still refuses, with COOC_ERR_STATE: cooc_snapshot_prepare and cooc_restore_begin /
 *                           _write / _finish (the format-1 blob has no section for the item counters and totals:
 *                           a sampled context is checkpointed through the cooc_sampling_snapshot_* /
 *                           cooc_sampling_restore_* family below, whose blob is a format of its own),
 *                           cooc_restore_*_parts (a sampled checkpoint is one blob of a world-1 job: there is
 *                           nothing to rescale) and cooc_comm_init* (the order is join, then enable).
 *                           Steps 1-3 are decided record by record on the calling thread.
 *   cooc_sampling_enable_device
 *                           the same mode with steps 1-3 of every fired window decided on the device: the item
 *                           counters, the users' reservoir lengths and totals and the decision counters live in
 *                           device memory for the life of the context; a window uploads its (slot, user id, item)
 *                           records (12 bytes each) and reads back one record per user with a changed slot.  Same
 *                           arguments, preconditions and error codes as cooc_sampling_enable; either call on a
 *                           context that is already sampled returns COOC_ERR_STATE.  For any sequence of submits,
 *                           elements and watermarks the context's outputs are identical, window by window and bit
 *                           for bit, to those of cooc_sampling_enable with the same item_cut, cfg.user_cut and
 *                           seed: deltas, row sums, heaps and scores, window info, all counters, every reservoir in
 *                           slot order and every total, the global state, cooc_last_window_runs.  (The draw is
 *                           keyed by the user's id in both; the order in which changed users reach the window
 *                           counter may differ, which no output depends on: counts are integer sums.)  The same
 *                           entry points are refused.  cooc_sampling_counters and the total of
 *                           cooc_copy_user_history then read device memory (small synchronous copies).
 *   cooc_sampling_counters  out[0] records rejected by the item cut, [1] fills, [2] replacements, [3] feedback
 *                           decrements, [4] users with a reservoir, [5] the sum of the item counters.
 *   cooc_copy_user_history  the user's resident history (the reservoir, in slot order) into items[cap] and its
 *                           length into *len, its userInteractionsTotal into *total (outside the sampled mode:
 *                           the length); any pointer may be NULL; cap < the length with items != NULL is
 *                           COOC_ERR_ARG; an unknown user has length 0.  Works in every mode, read-only. */
COOC_API int cooc_sampling_enable(cooc_ctx *ctx, int32_t item_cut, int64_t seed);
COOC_API int cooc_sampling_enable_device(cooc_ctx *ctx, int32_t item_cut, int64_t seed);
COOC_API int cooc_sampling_counters(cooc_ctx *ctx, int64_t *out6);
COOC_API int cooc_copy_user_history(cooc_ctx *ctx, int32_t user, int32_t cap, int32_t *items, int32_t *len,
                                    int32_t *total);

/* ---- device-side sampler: item cut and reservoirs of a device-resident log ------------------------------
 * The sampled pipeline is the reference job's default (-ic 500 -uc 500, FlinkCooccurrences.java:79-129).
 * cooc_sample_device applies steps 1-3 of the sampled mode above (ItemInteractionCounter...java:119-143 and :94-116,
 * UserInteractionCounter...java:145-257) to a log of (user, item) records in arrival order in device memory, cut
 * into consecutive windows, window after window from empty state, and returns the final reservoirs as a CSR.
 * That CSR is a valid input of cooc_count_device, cooc_count_owned, cooc_shard_plan and, through the count's
 * result, cooc_topk_batch*: every reservoir holds at most user_cut items, so the batch calls' first-user_cut cap is
 * a no-op on it, and the count over it is the exact global state the streaming sampled mode reaches after the same
 * windows ("every count equals the pair count over all current reservoirs").
 *
 * The same semantics, per window, from count[i], L[u] = |H_u|, T[u] = total[u] and the reservoirs at its start:
 *  1. Item cut.  rho = the record's rank among the window's records of its item, in arrival order, from 0:
 *     sample = rho < item_cut - count[i].  (The window's own feedback does not reopen the cut within the window.)
 *  2. User stage.  j = the record's rank among the window's records of its user, s = the sampled records of that
 *     user before it in the window.  total = T[u] + j + 1.  A sampled record with L[u] + s < user_cut fills slot
 *     L[u] + s; any other sampled record draws k (the draw above, keyed by u and total): k < user_cut replaces
 *     slot k, otherwise its item is fed back.
 *  3. A slot written more than once within a window keeps the writer that is last in arrival order.
 *  4. The window's end: count[i] += (sampled records of i) - (feedbacks of i), L[u] += fills, T[u] += records.
 * The outputs are bit-identical from call to call: the only atomics are integer adds and max.
 *
 *   d_users, d_items   int32[n_records] on the device.  User ids are the dense indices [0, n_users) and key the
 *                      draw; item ids are in [0, cfg.n_items).  n_records in [0, 2^31 - 1] (a total is a Java int).
 *   window_ptr         int64[n_windows + 1] on the host: starts at 0, non-decreasing, ends at n_records; a window
 *                      may be empty.  NULL with n_windows == 1: one window.
 *   item_cut, user_cut 1..32767 each (Java shorts); the context's cfg.user_cut and sampling state play no part.
 *   d_res_ptr          int64[n_users + 1], d_res_items int32[res_cap]: user u's reservoir in slot order at
 *                      [d_res_ptr[u], d_res_ptr[u + 1]).  min(n_records, n_users * user_cut) always suffices.
 *   d_total            int32[n_users] the users' totals, d_item_count int16[cfg.n_items] the item counters after
 *                      the last window; either may be NULL.
 *   info               the decision counters (as cooc_sampling_counters [0..5]) and the reservoirs' size.
 *
 * Works on any context, sampled or not, with or without a communicator, and touches neither the streaming state
 * nor the last batch result: the context provides the device, the scratch and the error text.  Runs on hip_stream
 * and synchronises it before returning (info comes from the device).
 * COOC_ERR_ARG: item_cut or user_cut outside 1..32767, n_users <= 0, a malformed window_ptr, a NULL required
 * pointer, n_records out of range; a user or item id out of range (found on the device before any output is
 * written; the message names the first such record); res_cap below the reservoirs' size (info->reservoir_items
 * then holds the size needed, the other outputs are unspecified).  The context stays usable after every failure. */
typedef struct cooc_sample_info {
  int64_t rejected, fills, replacements, feedbacks;  /* cooc_sampling_counters [0..3] */
  int64_t users;             /* users with a non-empty reservoir */
  int64_t item_counter_sum;  /* sum of the item counters after the last window */
  int64_t reservoir_items;   /* d_res_ptr[n_users]; on a too-small res_cap: the capacity needed */
  int64_t reserved;
} cooc_sample_info;          /* 64 bytes */

COOC_API int cooc_sample_device(cooc_ctx *ctx, int64_t n_records, const int32_t *d_users, const int32_t *d_items,
                                int32_t n_users, int32_t n_windows, const int64_t *window_ptr /* host, or NULL */,
                                int32_t item_cut, int32_t user_cut, int64_t seed,
                                int64_t *d_res_ptr, int32_t *d_res_items, int64_t res_cap,
                                int32_t *d_total, int16_t *d_item_count, void *hip_stream, cooc_sample_info *info);

/* ---- device-side sampler across GPUs: each rank its users' shard of the log ----------------------------
 * cooc_sample_owned is cooc_sample_device over the context's communicator (cooc_comm_init*): the sampled pipeline
 * in front of cooc_count_owned / cooc_topk_owned, where every rank holds its own users' records in device memory.
 * The call is collective.  Each rank passes its own users' records: d_users are local dense indices in
 * [0, n_users), window_ptr is over its own records, and a rank without users (n_users == 0 with n_records == 0)
 * still takes part.  A user's records all lie on one rank.
 *
 *   Window w of the job is R_0[w] || R_1[w] || ... || R_{W-1}[w], R_r[w] rank r's records of its window w.
 *
 * This is the rank-major order of "Sampled mode at world > 1" above; steps 1-4 of cooc_sample_device apply to it,
 * unchanged, in the data-parallel form stated there: a record of item i with rank rho among rank r's records of i
 * in the window is sampled iff count[i] + base_r[i] + rho < item_cut, the user stage is local, and every rank ends
 * the window with count[i] += min(sum_q h_q[i], max(0, item_cut - count[i])) - sum_q f_q[i].  Each window the ranks
 * all-gather the lengths of their histogram lists and the lists, then the lengths of their feedback lists and, unless
 * no rank has a feedback, the lists: two to four all-gathers, also on a rank with no record in the window.
 *
 *   d_user_key   int32[n_users] on the device, or NULL: d_user_key[j] >= 0 is the job-wide id of local user j and
 *                keys the draw sample_draw(seed, key, total); NULL: key = index, as cooc_sample_device.  The keys are
 *                the caller's responsibility and are not checked for uniqueness across ranks.  Both sharding
 *                conventions of the library fit: contiguous user ranges (key = u0 + j) and u mod world.
 *   d_res_ptr    int64[n_users + 1], d_res_items: the rank's reservoirs as a local CSR, a valid input of
 *                cooc_count_owned in both universes: at 40,320 items and above (the histories all-gathered) and
 *                below (the records exchange).  d_total is local.  d_item_count is replicated: identical on every
 *                rank.
 *   info         rejected, fills, replacements, feedbacks, users and reservoir_items count this rank's own records
 *                and users; item_counter_sum is the job's value, the same on every rank.
 *
 * Equivalence.  The union of the ranks' outputs equals, bit for bit, one cooc_sample_device call over the serialised
 * log with the keys as user ids: every reservoir in slot order, every total and every item counter; the four decision
 * counters summed over the ranks equal the single call's.  Two calls on the same inputs give bit-identical outputs.
 * Without a communicator, or at world 1, no collective is called and the result is cooc_sample_device's with the
 * draw keyed by d_user_key.
 *
 * Errors never leave a peer waiting.  Every rank makes its local checks first (cooc_sample_device's, the id-range
 * pass on the device included, and a negative key); then the ranks all-gather one small record: the local status,
 * n_windows, item_cut, user_cut and seed.  If any rank failed, or the four values differ, every rank returns
 * COOC_ERR_ARG before any output is written or any other collective starts; the failing rank's message names its own
 * cause, the others name the rank.  One window of a rank holds fewer than 2^30 records (a local check), and the
 * job's records of one item in one window stay below 2^30, the bound of the exchange's int32 sums: that is checked on
 * the gathered lists, which are identical on all ranks, so every rank returns COOC_ERR_ARG in the same window.  A
 * too-small res_cap stays a local error at the end, as in cooc_sample_device: info->reservoir_items reports the need.
 * The context and the communicator stay usable after every failure.  Additive: the ABI version stays 7. */
COOC_API int cooc_sample_owned(cooc_ctx *ctx, int64_t n_records, const int32_t *d_users, const int32_t *d_items,
                               int32_t n_users, const int32_t *d_user_key /* device int32[n_users], or NULL */,
                               int32_t n_windows, const int64_t *window_ptr /* host, or NULL */,
                               int32_t item_cut, int32_t user_cut, int64_t seed,
                               int64_t *d_res_ptr, int32_t *d_res_items, int64_t res_cap,
                               int32_t *d_total, int16_t *d_item_count, void *hip_stream, cooc_sample_info *info);

/* ---- checkpoints: the streaming state as one snapshot blob --------------------------------------------
 * Everything the streaming entry points above keep between windows is Flink keyed state in the reference
 * (windowState and userHistoryState, NonSampled...java:73-77; the rescorer's itemRows and globalItemRowSums,
 * ItemRowRescorer...java:33-41).  Here it lives on the GPU and in host tables, so a checkpointed job saves and
 * restores it through these calls (a Flink operator: snapshotState / initializeState over raw operator state).
 *
 * Saved: the users' histories (arrival order), the non-empty global rows (columns ascending, exact counts) and
 * their row sums, the running totals, the accumulators of cooc_op_counters, and the operator's watermark and
 * buffered windows with their records in arrival order.  Not saved: the last window's outputs, batch results,
 * scratch, and the internal layout.  The blob is canonical -- two contexts in the same logical state give
 * byte-identical blobs, whether their rows live in the dense matrix or in row slabs -- and a blob taken from one
 * representation restores into the other.  Its header carries a format version (info->format, 1), n_items,
 * window_size_ms, user_cut, rank and world; each section a 64-bit checksum, the sum over its 8-byte words w_i of
 * splitmix64(w_i ^ i) (the splitmix64 of cooc_verify_batch), computed on the device on both sides.
 *
 *   cooc_snapshot_prepare  packs the state into one device image on the context's stream and fills *info (the
 *                          stream is synchronised).  The state is untouched.  COOC_ERR_STATE while a window
 *                          staged by cooc_submit_batch is unfinished.
 *   cooc_snapshot_copy     bytes [offset, offset + n) of that image into out: a JVM streams a blob larger than
 *                          one Java array out in ranges.
 *   cooc_snapshot_release  frees the image (also implied by the next cooc_finish_window or restore).
 *   cooc_restore_begin     announces a blob of `bytes` bytes for a context WITHOUT streaming state (nothing
 *                          submitted, no element processed; else COOC_ERR_STATE);
 *   cooc_restore_write     bytes [offset, offset + n) of it, in any order;
 *   cooc_restore_finish    validates, then installs, and fills *info.  n_items, window_size_ms and user_cut must
 *                          equal the context's and (rank, world) its communicator's ((0, 1) without one: join
 *                          the communicator first); topk and COOC_FLAG_EXACT_SCORES only shape outputs and may
 *                          differ.  The blob is untrusted: header and directory, checksums, then a device pass
 *                          over the contents (ids in range, columns strictly ascending, counts non-zero,
 *                          offsets monotone and ending at their section's count, rows summing to their row
 *                          sums, user ids strictly ascending) all pass before anything is installed.  Any
 *                          failure is COOC_ERR_ARG (COOC_ERR_OOM for allocations) and leaves the context
 *                          empty and usable.  Local, not collective: across ranks the caller snapshots when
 *                          every rank has finished the same windows (each rank's cooc_op_process_watermark
 *                          loop returned fired = 0) and restores every rank from its own blob.
 *   cooc_snapshot_inspect  header and directory of a blob on the host (no context, no device): n_bytes is the
 *                          whole blob's length, of which only the first COOC_SNAPSHOT_HEADER_BYTES are read. */
#define COOC_SNAPSHOT_HEADER_BYTES 664
typedef struct cooc_snapshot_info {
  int64_t bytes;            /* size of the blob */
  int64_t n_users;          /* users with a resident history */
  int64_t history_items;    /* sum of their lengths */
  int64_t global_rows;      /* items with a non-empty global row */
  int64_t global_entries;   /* entries over those rows */
  int64_t pending_windows, pending_records;   /* windows buffered by the operator, and their records */
  int32_t format;           /* blob format version, starts at 1 */
  int32_t rank, world;      /* (0, 1) without a communicator */
  int32_t reserved;
} cooc_snapshot_info;
COOC_API int cooc_snapshot_prepare(cooc_ctx *ctx, cooc_snapshot_info *info);
COOC_API int cooc_snapshot_copy(cooc_ctx *ctx, int64_t offset, int64_t n, uint8_t *out);
COOC_API int cooc_snapshot_release(cooc_ctx *ctx);
COOC_API int cooc_restore_begin(cooc_ctx *ctx, int64_t bytes);
COOC_API int cooc_restore_write(cooc_ctx *ctx, int64_t offset, int64_t n, const uint8_t *src);
COOC_API int cooc_restore_finish(cooc_ctx *ctx, cooc_snapshot_info *info);
COOC_API int cooc_snapshot_inspect(const uint8_t *bytes, int64_t n_bytes, cooc_snapshot_info *info);

/* ---- checkpoints of a sampled context ------------------------------------------------------------------
 * A sampled context (cooc_sampling_enable / cooc_sampling_enable_device) keeps, next to the state above, the item
 * counters, every user's userInteractionsTotal and the decision counters of cooc_sampling_counters.  Its blob is
 * a format of its own (info->format 2, magic "COOCSMP2"): the same container with 20 sections, the 15 of format 1
 * with their meaning, then
 *   16  int64[8]  item_cut, seed, rejected, fills, replacements, feedbacks, 0, 0
 *   17  int32[]   the items whose counter is non-zero, strictly ascending
 *   18  int16[]   their counters, each in 1..item_cut
 *   19  int32[]   the users with a total > 0, strictly ascending: a superset of section 2 (a user whose every
 *                 record was rejected at the item cut has a total and no reservoir)
 *   20  int32[]   their totals, each >= 1 and >= the user's history length
 * The feedback queue is not state (it is applied at the end of the window it arose in, and no snapshot is taken
 * while a window is staged); the samplers' stamps, window numbers and slot numbering are layout and not saved.
 * The blob is canonical: the same logical state gives the same bytes whether the decisions are made on the host
 * or on the device and whether the global rows are the dense matrix or slabs (a global key whose count went back
 * to 0 is not saved), and a blob taken in one mode or representation restores into the other.
 *
 *   cooc_sampling_snapshot_prepare  cooc_snapshot_prepare for a sampled context, in either mode; the image is read
 *                                   and freed with cooc_snapshot_copy / cooc_snapshot_release.  COOC_ERR_STATE
 *                                   on an unsampled context or while a window is staged.
 *   cooc_sampling_restore_begin / _write / _finish
 *                                   as cooc_restore_begin / _write / _finish, for a sampled context (either mode)
 *                                   without streaming state; otherwise COOC_ERR_STATE.  n_items, window_size_ms,
 *                                   user_cut, item_cut and the seed must equal the context's; any mismatch, a
 *                                   format-1 blob, or contents that fail the validation (the checks of
 *                                   cooc_restore_finish, and: sections 17 and 19 strictly ascending and 17 in
 *                                   range, counters in 1..item_cut, totals >= 1, every user of section 2 in
 *                                   section 19 with total >= history length, every history <= user_cut) is
 *                                   COOC_ERR_ARG and leaves the context empty, sampled and usable.  Afterwards
 *                                   cooc_sampling_counters and cooc_copy_user_history read what was saved.
 *   cooc_sampling_snapshot_inspect  cooc_snapshot_inspect for the sampled format: header and directory, and the
 *                                   sampler's scalars (section 16, with its checksum) into *sinfo.  Reads the
 *                                   first COOC_SAMPLED_SNAPSHOT_HEADER_BYTES and the 64 bytes of section 16.
 * Each family rejects the other's blobs with COOC_ERR_ARG (bad magic). */
#define COOC_SAMPLED_SNAPSHOT_HEADER_BYTES 864
typedef struct cooc_sampling_snapshot_info {
  int64_t seed;
  int64_t rejected, fills, replacements, feedbacks;   /* cooc_sampling_counters [0..3] */
  int64_t counted_items;    /* items with a non-zero counter */
  int64_t total_users;      /* users with a total (>= cooc_snapshot_info.n_users) */
  int32_t item_cut;
  int32_t reserved;
} cooc_sampling_snapshot_info;   /* 64 bytes */
COOC_API int cooc_sampling_snapshot_prepare(cooc_ctx *ctx, cooc_snapshot_info *info);
COOC_API int cooc_sampling_restore_begin(cooc_ctx *ctx, int64_t bytes);
COOC_API int cooc_sampling_restore_write(cooc_ctx *ctx, int64_t offset, int64_t n, const uint8_t *src);
COOC_API int cooc_sampling_restore_finish(cooc_ctx *ctx, cooc_snapshot_info *info);
COOC_API int cooc_sampling_snapshot_inspect(const uint8_t *bytes, int64_t n_bytes, cooc_snapshot_info *info,
                                            cooc_sampling_snapshot_info *sinfo);

/* ---- rescaling: one checkpoint's blobs restored into another parallelism -------------------------------
 * The blobs of ALL subtasks of one checkpoint of a job (W_old = n_parts of them; Flink: union list state, every
 * new subtask receives all of them) determine the state of any rank of any new world: rows are owned by
 * a mod world, every rank holds every item's job-wide row sum, the rescorer's totals are job-wide, and the
 * accumulators of cooc_op_counters are per-subtask and sum to the job's.
 *
 *   cooc_restore_begin_parts   announces n_parts blobs of bytes[i] bytes for a context WITHOUT streaming state
 *                              that has already joined its communicator ((rank, world) below are its own);
 *                              1 <= n_parts <= COOC_MAX_RESTORE_PARTS, else COOC_ERR_ARG;
 *   cooc_restore_write_part    bytes [offset, offset + n) of part `part`, in any order;
 *   cooc_restore_finish_parts  validates everything, then installs: the histories of the users the route keeps
 *                              (route NULL: COOC_ROUTE_MOD; an unknown kind, reserved != 0, or a bitmap of
 *                              n_bits > 0 without bits is COOC_ERR_ARG);
 *                              the global rows a with a mod world == rank, in this context's representation;
 *                              every item's job-wide row sum; the union of the parts' pending windows (within a
 *                              window the kept records of part 0, then part 1, ..., each in its stored order; a
 *                              window without a kept record is dropped); the job-wide totals; the sum of the
 *                              parts' accumulators on rank 0 and 0 on every other rank; the parts' common
 *                              watermark (also the agreed one when world > 1).  *info describes the installed
 *                              state: what cooc_snapshot_prepare would report right now.
 * Every part passes the whole validation of cooc_restore_finish; across parts: n_items, window_size_ms and
 * user_cut equal the context's, part i was taken by rank i of n_parts, a row lives in the part that owns it, user
 * ids are disjoint, the job-wide totals agree, every part was taken after its watermark loop returned
 * fired = 0 (no window buffered at or below its watermark, no collective step outstanding), the watermarks
 * agree when n_parts > 1, and every part's row sums of other ranks are exactly the other parts' rows' sums.  Any
 * failure is COOC_ERR_ARG (COOC_ERR_OOM for allocations) and leaves the context empty and usable.
 * All parts are resident on the device at once: a restoring rank needs device memory for the whole job's blobs
 * next to its own share of the state.  Local, not collective.  With COOC_ROUTE_BITMAP the caller sees to it that
 * every user is kept by exactly one subtask; the check is that info->n_users and info->history_items summed over
 * the new ranks equal the parts' sums from cooc_snapshot_inspect.  cooc_restore_finish is unchanged: one blob,
 * the same (rank, world). */
#define COOC_MAX_RESTORE_PARTS 32768  /* Flink's upper bound of a job's parallelism; one grid row per part */
#define COOC_ROUTE_MOD    0  /* this subtask keeps user u iff floor-mod(u, world) == rank */
#define COOC_ROUTE_BITMAP 1  /* keeps user u iff 0 <= u < n_bits and bit u of bits[] (host memory) is set */
typedef struct cooc_user_route {
  int32_t kind, reserved;
  int64_t n_bits;
  const uint64_t *bits;   /* bit u: word u / 64, bit u % 64 */
} cooc_user_route;
COOC_API int cooc_restore_begin_parts(cooc_ctx *ctx, int32_t n_parts, const int64_t *bytes);
COOC_API int cooc_restore_write_part(cooc_ctx *ctx, int32_t part, int64_t offset, int64_t n, const uint8_t *src);
COOC_API int cooc_restore_finish_parts(cooc_ctx *ctx, const cooc_user_route *route, cooc_snapshot_info *info);

/* ---- multi-GPU sharding layer (the keyBy(itemA) exchange, FlinkCooccurrences.java:152,163) ---------
 * Users are sharded over GPUs; each GPU's cooc_count_device result holds PARTIAL rows.  Row a is
 * owned by GPU (a mod n_parts).  The caller moves the packed partial rows with an all-to-all
 * (RCCL over xGMI, e.g. torch.distributed.all_to_all_single) and the row sums with an all-reduce.
 *   cooc_partition_plan   entries of the last cooc_count_device result per owner -> h_entries[n_parts]
 *   cooc_partition_pack   into caller DEVICE buffers, owner-major then ascending row:
 *                         d_row_nnz int32[n_items], d_entries uint64[sum h_entries] = (col << 32 | cnt)
 *   cooc_copy_rowsum_device  the last result's exact row sums into a caller device int64[n_items]
 *   cooc_merge_partitions for owner `part`: d_recv_row_nnz int32[n_parts * rows_owned] and
 *                         d_recv_entries (both source-major, as delivered by the all-to-all);
 *                         d_rowsum_global (the all-reduced row sums, may be NULL) checks every merged
 *                         row.  Result rows r = 0..n_rows-1 are items part + r * n_parts (borrowed
 *                         device views in *out; out->n_items = rows owned).  A part >= n_items owns no
 *                         row: its result has n_items == 0 and d_recv_row_nnz may be NULL.
 * A merged count is the sum of the sources' counts modulo 2^32.  With d_rowsum_global a row whose merged
 * counts do not add up to its all-reduced row sum -- a key whose sum left uint32 -- fails the call with
 * COOC_ERR_OVERFLOW.  Without it nothing is checked, and what becomes of a key whose sum wrapped to 0 depends on
 * n_items: the dense merge (n_items <= 40,704) drops it, the sorted merge above keeps it with count 0.
 * Limit: above 40,704 items one call merges fewer than 2^31 received entries (COOC_ERR_ARG otherwise, before
 * any entry is read). */
COOC_API int cooc_partition_plan(cooc_ctx *ctx, int32_t n_parts, int64_t *h_entries);
COOC_API int cooc_partition_pack(cooc_ctx *ctx, int32_t n_parts, int32_t *d_row_nnz, uint64_t *d_entries,
                                 void *hip_stream);
COOC_API int cooc_copy_rowsum_device(cooc_ctx *ctx, int64_t *d_rowsum, void *hip_stream);
COOC_API int cooc_merge_partitions(cooc_ctx *ctx, int32_t n_parts, int32_t part, const int32_t *d_recv_row_nnz,
                                   const uint64_t *d_recv_entries, const int64_t *d_rowsum_global, void *hip_stream,
                                   cooc_device_result *out);

/* ---- communicator: the RCCL sharding layer behind the C-ABI ------------------------------------------
 * The reference's keyed exchanges -- keyBy(user) (FlinkCooccurrences.java:70), keyBy(ItemCooccurrences::
 * getItem) (:152) and rowSumStream.broadcast() (:163) -- as collectives inside the library, on the
 * context's caller stream, over RCCL (xGMI on one node).  One context per GPU process / Flink subtask; the
 * SURVEY §8(b) "refcounted device/RCCL singleton" is the process-wide RCCL library handle (dlopen'ed once;
 * a process that already loaded RCCL shares it).
 *   cooc_comm_unique_id  rank 0 creates the communicator id (COOC_COMM_ID_BYTES opaque bytes) and the
 *                        caller distributes it (Flink: the job graph's broadcast / a shared file; Python:
 *                        torch.distributed.broadcast).  Fails with COOC_ERR_HIP when RCCL is absent.
 *   cooc_comm_init       every rank: joins the world-size communicator as `rank` on the context's device.
 *   cooc_comm_init_ops   the same exchange over caller-provided collectives (any transport the caller has,
 *                        e.g. gloo in tests).  Each operation is collective over the ranks, takes device
 *                        pointers, returns 0 on success and must have completed with respect to hip_stream
 *                        when it returns (later work enqueued on that stream sees its result):
 *                          allreduce_sum_i64: d_buf[0, n) summed over the ranks, in place;
 *                          allgather: rank r's `bytes` at d_send land at d_recv + r * bytes;
 *                          alltoallv: send_bytes[p] bytes at d_send + send_off[p] go to rank p, which
 *                            receives them at d_recv + recv_off[sender]; recv_bytes[p] arrive from rank p
 *                            (host arrays of world entries). */
#define COOC_COMM_ID_BYTES 128
typedef struct cooc_comm_ops {
  int (*allreduce_sum_i64)(void *user, int64_t *d_buf, int64_t n, void *hip_stream);
  int (*allgather)(void *user, const void *d_send, void *d_recv, int64_t bytes, void *hip_stream);
  int (*alltoallv)(void *user, const void *d_send, const int64_t *send_off, const int64_t *send_bytes, void *d_recv,
                   const int64_t *recv_off, const int64_t *recv_bytes, void *hip_stream);
} cooc_comm_ops;
COOC_API int cooc_comm_unique_id(uint8_t *id);
COOC_API int cooc_comm_init(cooc_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world);
COOC_API int cooc_comm_init_ops(cooc_ctx *ctx, int32_t rank, int32_t world, const cooc_comm_ops *ops, void *user);

/* One window of the multi-GPU large-universe job (n_items >= 40,320: C3 / C5), whole inside the library on
 * hip_stream: this rank's users (keyBy(user)) -> (1) local item frequencies, all-reduced (the planner's
 * column estimate and the owner map); (2) the row owner map: rows by descending global frequency (ties:
 * smaller id), the 4,096 most frequent placed greedily on the least loaded rank, the rest dealt in snake
 * order (cooc_snake_owner); (3) the histories all-gathered (one uneven all-to-all per array: every rank
 * sends its part to every peer at once, each pair over its own xGMI link); (4) the owned rows counted over
 * all users (cooc_count_device_owned: the keyBy(getItem) as ownership -- rows are complete on their owner,
 * nothing is merged); (5) the ordered pairs all-reduced.  *out: the owned rows (borrowed, as
 * cooc_count_device_owned); *info the totals and borrowed device views of the owner map and the global
 * item frequencies.
 *
 * Small universes: below 40,320 items cooc_count_owned runs the records exchange over the communicator, and row a
 * is complete on rank a mod world.  The same call, chosen by n_items alone (with COOC_FLAG_GENERAL_PLANNER the steps
 * above apply at any size): (1) the first-user_cut cap, then this rank's local plan (as cooc_shard_plan: 8-B
 * descriptors grouped by owner, row counts in owner-major order, the padded u16 arena); a rank with n_users == 0
 * plans nothing and still takes part; (2) the agreement below; (3) the arenas all-gathered, one slot per rank of the
 * largest rank's arena ids plus one pad group of 8, padded with the sink id n_items; (4) two uneven all-to-alls:
 * rows_owned int32 row counts and the descriptors to each row's owner; (5) the owner counts its rows, complete,
 * over every rank's records (as cooc_shard_count); (6) the job's item frequencies: the local row counts widened
 * and all-reduced.  The result is always a padded CSR over all n_items rows, columns ascending, whatever the output
 * layout flags: row a of rank a mod world holds its entries, every other row has row_nnz 0, rowsum 0 and a valid
 * row_base; out->n_items == cfg.n_items and out->dense == NULL.  It is the context's batch result exactly as a
 * large-universe owned result is: cooc_copy_batch(_range), cooc_verify_batch, cooc_copy_rowsum_device,
 * cooc_topk_batch*, cooc_topk_items and cooc_topk_owned(_host) read it.  info: owner[a] = a mod world, observed the
 * job's ordered pairs (the sum of the ranks' local pairs from the agreement: no all-reduce), local_observed the
 * pairs of this rank's owned rows (the sum of their row sums), item_counts the job's frequencies after the cap,
 * gathered_bytes the peers' arena, descriptor and row-count bytes received.  A world-1 communicator runs the same
 * code with self-copies.
 *
 * Errors never leave a peer waiting (small universes).  Every rank makes its local checks first (the CSR arguments,
 * cooc_count_owned_host's checks of its host arrays, the plan's item-range pass on the device); then the ranks
 * all-gather one record of 5 + world int64: the local status, n_users, the interactions after the cap, the arena
 * ids used, the local ordered pairs and the descriptors bound for every owner.  If any rank failed, every rank
 * returns COOC_ERR_ARG before any payload moves or any other collective starts; the failing rank's message names its
 * own cause (an item out of range: the first such interaction and its id), the others name the rank.  One owner
 * takes fewer than 2^31 descriptors: that is checked on the gathered records, which are identical on all ranks, so
 * every rank returns COOC_ERR_ARG alike.  COOC_ERR_OVERFLOW (a count beyond uint32) stays local to the owner of the
 * row, after the exchange.  The context and the communicator stay usable after every failure.  Additive: the ABI
 * version stays 7. */
typedef struct cooc_owned_info {
  int32_t part, n_parts;
  int64_t observed;           /* ordered pairs of the whole job (sum over the ranks) */
  int64_t local_observed;     /* ordered pairs of this rank's owned rows */
  int64_t n_users_all, n_interactions_all;
  int64_t gathered_bytes;     /* history bytes this rank received */
  const int32_t *owner;       /* device int32[n_items] */
  const int64_t *item_counts; /* device int64[n_items]: the all-reduced frequencies */
} cooc_owned_info;
COOC_API int cooc_count_owned(cooc_ctx *ctx, int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                              int64_t n_interactions, void *hip_stream, cooc_owned_info *info,
                              cooc_device_result *out);
/* The same window from HOST arrays (a JVM subtask's buffered user shard: user_ptr int64[n_users+1] into
 * items), staged on the context's stream; *winfo as cooc_count_host (nnz, observed and rows with entries of
 * the OWNED rows).  The owned rows are then this context's batch result: cooc_copy_batch packs them (every
 * other row empty), cooc_topk_batch / cooc_topk_owned score them.  Replaces the p > 1 merge of partial
 * rows (ItemRowAggregator / RowSumAggregator windows keyed by item, FlinkCooccurrences.java:138-157) for a
 * one-window job. */
COOC_API int cooc_count_owned_host(cooc_ctx *ctx, int64_t n_users, const int64_t *user_ptr, const int32_t *items,
                                   cooc_owned_info *info, cooc_window_info *winfo);
/* C5 after cooc_count_owned: the owned rows' row sums all-reduced (the broadcast row-sum stream,
 * FlinkCooccurrences.java:163), then every owned row's LLR top-k against them (cooc_topk_batch_device).
 * d_rowsum_global (device int64[n_items], may be NULL) receives the all-reduced row sums. */
COOC_API int cooc_topk_owned(cooc_ctx *ctx, int32_t topk, int32_t flags, int32_t *d_sizes, int32_t *d_values,
                             double *d_scores, int64_t *d_rowsum_global, void *hip_stream);
/* cooc_topk_owned into the context's own buffers (a JVM subtask: GpuOwnedCooccurrenceTopKOperator), read back
 * with cooc_copy_topk_batch / cooc_copy_topk_batch_range / cooc_topk_items: every owned row's heap, scored
 * against the all-reduced row sums and the job's observed total.  Replaces the rescorer of
 * FlinkCooccurrences.java:162-167 (ItemRowRescorerTwoInputStreamOperator.java:195-226) for a one-window job. */
COOC_API int cooc_topk_owned_host(cooc_ctx *ctx, int32_t topk, int32_t flags);
/* Heaps of rows [row_begin, row_end) of the last cooc_topk_batch / cooc_topk_owned_host: sizes int32[n],
 * values int32[n*topk], scores double[n*topk] (n = row_end - row_begin, layout as cooc_copy_topk_batch).  topk
 * is the caller's buffer width and must equal the topk of that call: anything else is COOC_ERR_ARG and nothing
 * is written (the buffers are sized from it). */
COOC_API int cooc_copy_topk_batch_range(cooc_ctx *ctx, int32_t row_begin, int32_t row_end, int32_t topk,
                                        int32_t *sizes, int32_t *values, double *scores);
/* Every rank's `value` (collective over the communicator): out int64[world] in rank order.  The JVM operators
 * agree on the window they fire with it (a subtask with no records of its own joins the same window). */
COOC_API int cooc_comm_allgather_i64(cooc_ctx *ctx, int64_t value, int64_t *out);
/* The owner map of step (2) on the host (no device): counts int64[n_items] -> owner int32[n_items]. */
COOC_API int cooc_snake_owner(const int64_t *counts, int32_t n_items, int32_t world, int32_t head, int32_t *owner);

/* ---- sharded records (multi-GPU: the keyBy(itemA) of FlinkCooccurrences.java:152 on pair RECORDS) -
 * Users are sharded over n_parts GPUs (keyBy(user), :70); row a is owned by part a mod n_parts.  The
 * reference ships each pair record (itemA, the user's history) to the owner of itemA; here every
 * part ships its users' histories once (the caller all-gathers the u16 arenas) and one 8-B
 * descriptor per record (the caller all-to-alls them by owner), and each owner reduces complete
 * rows: no partial counts are exchanged and nothing is merged.
 *   cooc_shard_plan   this part's users -> into caller DEVICE buffers: d_desc uint64[n_interactions]
 *                     (descriptors grouped by owner, then by owned row), d_row_counts int32[n_items]
 *                     (row counts in the same owner-major order: owner o's rows_owned(o) counts are
 *                     contiguous), d_arena uint16[arena_cap >= n_interactions + 7 n_users + 16];
 *                     h_send[n_parts] = descriptors per owner, h_info[0] = arena ids used (a multiple
 *                     of 8), h_info[1] = this part's ordered pairs.
 *   cooc_shard_count  owner `part`: d_recv_row_counts int32[n_parts * rows_owned] and d_recv_desc
 *                     (source-major, as delivered by the all-to-all), d_arena_all the all-gathered
 *                     arenas with source s at s * arena_stride ids.  Result rows r = 0..n_rows-1 are
 *                     items part + r * n_parts (borrowed device views in *out; out->n_items = rows
 *                     owned), complete: counts, row sums and the overflow check are final. */
COOC_API int cooc_shard_plan(cooc_ctx *ctx, int64_t n_users, const int64_t *d_user_ptr, const int32_t *d_items,
                             int64_t n_interactions, int32_t n_parts, uint64_t *d_desc, int32_t *d_row_counts,
                             uint16_t *d_arena, int64_t arena_cap, void *hip_stream, int64_t *h_send,
                             int64_t *h_info);
COOC_API int cooc_shard_count(cooc_ctx *ctx, int32_t n_parts, int32_t part, const int32_t *d_recv_row_counts,
                              const uint64_t *d_recv_desc, int64_t n_recv, const uint16_t *d_arena_all,
                              int64_t arena_stride, void *hip_stream, cooc_device_result *out);

/* ---- ItemCooccurrences wire codec (ItemCooccurrences.java:113-147, Kryo 2.24 primitives) --------
 * Host-only (no device calls, no context).  A record is (item, increment int16, size other items):
 * varint item, big-endian int16 increment, varint size', size' varints -- every varint is Kryo's
 * writeInt(v, true).  For a mixed deployment that keeps the Java emitter or the Java reducer.
 *   cooc_records_encode  n records: items int32[n], increments int16[n], ks int32[n] (slot k is
 *                        skipped, ItemCooccurrences.java:124-131; NULL = all -1), rec_ptr
 *                        int64[n+1] into others.  out == NULL: *n_bytes = encoded size only;
 *                        else out must hold out_cap >= *n_bytes bytes.
 *   cooc_records_decode  bytes -> *n_records, *n_others; pass NULL arrays to size them, then
 *                        items int32[n_records], increments int16[n_records], rec_ptr
 *                        int64[n_records+1], others int32[n_others] (any may be NULL).  A truncated
 *                        record or a negative size fails with COOC_ERR_ARG. */
COOC_API int cooc_records_encode(int64_t n_records, const int32_t *items, const int16_t *increments, const int32_t *ks,
                                 const int64_t *rec_ptr, const int32_t *others, uint8_t *out, int64_t out_cap,
                                 int64_t *n_bytes);
COOC_API int cooc_records_decode(const uint8_t *bytes, int64_t n_bytes, int64_t *n_records, int64_t *n_others,
                                 int32_t *items, int16_t *increments, int64_t *rec_ptr, int32_t *others);

/* ---- text ingest (FlinkCooccurrences.java:55-61,207-229: TextInputFormat + InteractionLineSplitter) --
 * Host-only.  text: n_bytes of '\n'-delimited "user,item,timestamp" lines ("\r\n" accepted, fields after
 * the third ignored, as String.split(",") + Integer.valueOf / Long.valueOf).  users == NULL (or
 * items / ts NULL): *n_records = the number of lines only.  Else parses up to cap records; a line
 * that the reference's splitter rejects (NumberFormatException / ArrayIndexOutOfBoundsException)
 * fails with COOC_ERR_ARG and its 0-based index in *bad_line.  The watermark of the reference's
 * AscendingTimestampExtractor after a prefix of records is (largest timestamp so far) - 1. */
COOC_API int cooc_parse_interactions(const char *text, int64_t n_bytes, int64_t cap, int32_t *users, int32_t *items,
                                     int64_t *ts, int64_t *n_records, int64_t *bad_line);

/* ---- device ingest: the text source and what sits in front of every operator, on the GPU ----------------
 * cooc_parse_interactions_device is cooc_parse_interactions for a text in device memory, with the same semantics
 * byte for byte: records are the '\n'-delimited lines, a '\r' before the '\n' is dropped, a last line without
 * '\n' is a record and nothing follows a final '\n'; String.split(","): fields after the third are ignored, fewer
 * than three fail, an empty line fails; every field is an optional '+' or '-' and at least one ASCII digit,
 * range-checked as Integer.valueOf / Long.valueOf (INT32_MIN and Long.MIN_VALUE parse).
 *
 *   d_text            n_bytes of text on the device, n_bytes in [0, 2^31): line offsets are int32, and a caller
 *                     with more text cuts it at line ends.  No alignment is required.
 *   d_users, d_items  int32[cap], d_ts int64[cap] on the device.  If any of the three is NULL only *n_records (the
 *                     number of lines) is computed.
 *   n_records         host; the number of records on success.
 *   bad_line          host, may be NULL: -1, or the smallest 0-based index of a rejected line (what the host parser
 *                     reports, since it stops at the first).
 * COOC_ERR_ARG: a rejected line (*bad_line names it; the arrays are unspecified); more records than cap (*bad_line
 * is -1 unless a line below cap is rejected, as the host parser stops at whichever comes first); n_bytes out of
 * range; a NULL d_text with n_bytes > 0 or a NULL n_records.  The context provides the device, the scratch and the
 * error text: the call touches neither the streaming state nor the last batch result, runs on hip_stream and
 * synchronises it before returning, and leaves the context usable after every failure.  The only atomics are an
 * integer add and an integer min: outputs are bit-identical from call to call.
 *
 * cooc_log_prepare_device takes the log in arrival (file) order in device memory and gives what the operator holds
 * after the feed run_text_source defines ("Text ingest"): cooc_op_process_elements is fed blocks of
 * W = records_per_watermark records, each block followed by cooc_op_process_watermark(largest timestamp so far - 1),
 * and the feed ends with Long.MAX_VALUE.  The window size is cfg.window_size_ms.
 *
 *   Late.   m_b = the largest timestamp over all records of the blocks before block b, late records included.
 *           Record i of block b = i / W is late iff ts[i] = Long.MIN_VALUE, or b >= 1 and ts[i] < m_b; a record
 *           with ts[i] = m_b is kept.  W = 0: no watermark before the end, only the first rule applies.  Late
 *           records are dropped and counted in info->n_late (UserInteractionCounterLateElements).
 *   Checks. On kept records only, as the operator does: an item outside [0, cfg.n_items), or a timestamp outside
 *           [Long.MIN_VALUE + 2 size, Long.MAX_VALUE - 2 size] (where the window expression would overflow), is
 *           COOC_ERR_ARG; info->bad_record is the smallest such input index, the message names it, and no output
 *           has been written.
 *   Window. maxTimestamp = ts - (ts + size) % size + size - 1 (Java remainder), the operator's own expression.
 *   Firing order.  The kept records by ascending window end, in arrival order within a window: the order in which
 *           the operator's pending windows fire.  d_rec_item and d_rec_user hold that sequence; window_ts[w] is the
 *           w-th window end, window_ptr[w] its first record, window_ptr[n_windows] = n_kept.
 *   Users.  The distinct user ids of the kept records, ascending as signed int32, are the dense indices
 *           0..n_users-1: d_user_ids[j] is the id of index j, d_rec_user holds indices.  When all ids are >= 0,
 *           d_user_ids is a valid d_user_key of cooc_sample_owned.
 *   CSR.    d_user_ptr[0..n_users], d_user_items: every user's kept items in firing order, then arrival order: the
 *           user's history after the whole log, so cfg.user_cut keeps the same first interactions as the streaming
 *           state.
 *
 *   d_users, d_items, d_ts       int32 / int32 / int64 [n_records] on the device, n_records in [0, 2^31).
 *   d_rec_user, d_rec_item, d_user_ids, d_user_items  int32[n_records], d_user_ptr int64[n_records + 1], on the
 *                                device; n_kept / n_users (+ 1) entries are written.  Any may be NULL and is skipped.
 *   window_ptr, window_ts        int64[cap_windows + 1] / int64[cap_windows] on the host; either may be NULL.  With
 *                                cap_windows < n_windows (and at least one list given) they are not written and the
 *                                call returns COOC_ERR_ARG after writing the device outputs; info->n_windows gives
 *                                the need, as res_cap does in cooc_sample_device.
 *   n_records = 0 (or no kept record): d_user_ptr[0] = 0, window_ptr[0] = 0, info zero.
 *
 * (d_user_ptr, d_user_items) is an input of cooc_count_device, cooc_count_owned and cooc_shard_plan;
 * (d_rec_user, d_rec_item, window_ptr) one of cooc_sample_device and cooc_sample_owned.  Stateless like the parse
 * call: any context, no streaming state or batch result touched, runs on hip_stream and synchronises it.
 * COOC_ERR_ARG also for records_per_watermark < 0, n_records out of range, a NULL input or info.  Outputs are
 * bit-identical from call to call (integer atomics only; both sorts are stable).  Each rank of a multi-GPU job
 * prepares its own shard.  Additive: the ABI version stays 7. */
typedef struct cooc_log_info {
  int64_t n_kept, n_late;     /* n_late: UserInteractionCounterLateElements */
  int64_t n_users, n_windows; /* distinct users / windows among the kept records */
  int64_t bad_record;         /* -1, or the input index of the first kept record the call refuses */
  int64_t reserved[3];
} cooc_log_info;              /* 64 bytes */

COOC_API int cooc_parse_interactions_device(cooc_ctx *ctx, const char *d_text, int64_t n_bytes, int64_t cap,
                                            int32_t *d_users, int32_t *d_items, int64_t *d_ts, void *hip_stream,
                                            int64_t *n_records, int64_t *bad_line);
COOC_API int cooc_log_prepare_device(cooc_ctx *ctx, int64_t n_records, const int32_t *d_users,
                                     const int32_t *d_items, const int64_t *d_ts, int64_t records_per_watermark,
                                     int32_t *d_rec_user, int32_t *d_rec_item,       /* [n_records] */
                                     int32_t *d_user_ids,                            /* [n_records] */
                                     int64_t *d_user_ptr, int32_t *d_user_items,     /* [n_records + 1], [n_records] */
                                     int64_t *window_ptr, int64_t *window_ts, int64_t cap_windows, /* host */
                                     void *hip_stream, cooc_log_info *info);

/* ---- invariant checks of a batch result (the reference's DEVELOPMENT_MODE checks) ---------------
 * FlinkCooccurrences.java:34 switches on, among others, the row-sum consistency check of the rescorer
 * (ItemRowRescorer...java:183-193: the sum of a row == the item's row sum).  cooc_verify_batch runs it,
 * and the checks of this library's CSR contract, over the whole last cooc_count_device /
 * cooc_count_device_owned result on hip_stream (then synchronises it).  out8 (host int64[8]):
 *   [0] sum of all counts         [1] sum of the row sums (== [0] == observed for a whole result)
 *   [2] entries                   [3] rows whose counts do not sum to their row sum
 *   [4] rows with a bad entry: columns not strictly ascending or outside [0, n_items), a count of 0
 *       (dense layout: row_nnz[a] != the row's non-zero cells)
 *   [5] entries with C[a,b] != C[b,a] (only with COOC_VERIFY_SYMMETRY, padded CSR of a whole result;
 *       else -1)                  [6], [7] 0
 * d_row_checksum (device uint64[n_items], may be NULL): per row, the sum over its keys of
 * splitmix64((col << 32) ^ count) mod 2^64 (splitmix64(x): x += 0x9E3779B97F4A7C15;
 * x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), a
 * fingerprint to compare the result row by row with an independent restatement without copying it
 * out. */
#define COOC_VERIFY_SYMMETRY 1
COOC_API int cooc_verify_batch(cooc_ctx *ctx, int32_t flags, uint64_t *d_row_checksum, int64_t *out8,
                               void *hip_stream);

/* ---- diagnostics (not part of the reference surface) ------------------------------------------
 * Kernel timing of the dominant kernel (the accumulate kernel) with HIP events recorded on the
 * stream it is launched on; read back after a call that ran it. */
COOC_API int cooc_set_kernel_timing(cooc_ctx *ctx, int32_t enable);
COOC_API int cooc_last_kernel_ms(cooc_ctx *ctx, float *accumulate_ms);
/* Rows (and their ordered pairs) that the last large-universe count sent through the sort +
 * segmented-reduce path (hash table overflow, or COOC_FLAG_SORT_ROWS). */
COOC_API int cooc_last_sort_rows(cooc_ctx *ctx, int64_t *rows, int64_t *pairs);
/* Split rows whose columns above the first tile the last large-universe count took from the other rows'
 * entries (C[a, b] = C[b, a]) instead of walking them; 0 when that was off. */
COOC_API int cooc_last_mirror_rows(cooc_ctx *ctx, int64_t *rows);
/* Attempts of the last large-universe count (1; 2 after the output region was grown to the exact bound, or
 * after a mirrored attempt deferred a row and was repeated without mirroring; 3 after both) and the entries of
 * the output region the last attempt filled (every row's [row_base, row_base + row_nnz) lies inside it). */
COOC_API int cooc_last_attempts(cooc_ctx *ctx, int64_t *attempts, int64_t *region_entries);
/* The plan of the last run of the batch planner (n_items < 40,320: a batch, a streaming window or the owner side
 * of the records exchange) on the context, out8 = {partition blocks B of the histogram / scatter passes (0 on the
 * owner side, which has none), descriptors per batch of the accumulate kernel (db), chunks, split rows (rows of
 * several chunks), 1 when the dense layout was chosen, the longest list, the lists longer than 2,048 ids (filled
 * by a workgroup each), 0}.  The host's values from the run's one synchronisation: reading them launches and
 * copies nothing.  Zeros before any such run and after a large-universe run.  Read-only. */
COOC_API int cooc_last_batch_plan(cooc_ctx *ctx, int64_t *out8);
/* The arena of the streaming state's sparse global rows (n_items >= 40,320; the rescorer's itemRows,
 * ItemRowRescorer...java:35,171-177, as one sorted slab per row), as the host tracks it: its capacity in entries,
 * the bump pointer behind the last slab handed out, the live entries (the sum of the row lengths; bump - live
 * entries are slabs that rows have moved out of), and the compactions since the state was created or restored
 * (the first window's, from the empty arena, included).  Zeros with the dense global matrix and before the first
 * window.  Read-only. */
COOC_API int cooc_global_slab_stats(cooc_ctx *ctx, int64_t *cap, int64_t *bump, int64_t *live, int64_t *compactions);
/* Runs of the window counter in the last finished window of the sampled mode: 0 for an empty window, 1 when no
 * slot that existed before the window was replaced (the fill path's window, no minus lists), 2 with the minus
 * run and the signed combine.  0 outside the sampled mode. */
COOC_API int cooc_last_window_runs(cooc_ctx *ctx, int64_t *runs);
/* Self-test of the planner's single-pass device prefix sum (no context): d_out[i] = d_in[0] + .. + d_in[i]
 * (flags & 1) or + .. + d_in[i-1] over device arrays of n elements, on hip_stream (then synchronised).
 * flags: 1 inclusive, 2 tiles staged through LDS (else vectorised loads), 4 int32 output (else int64), 8 int32
 * input (else int64).  *diag (may be NULL) gets the scan's diagnostic word (bit 16: a look-back stopped waiting
 * and summed its prefix from the input). */
COOC_API int cooc_selftest_scan(const void *d_in, void *d_out, int64_t n, int32_t flags, int64_t *diag,
                                void *hip_stream);
/* Self-test of the planner's radix sort (no context): (d_keys_out, d_vals_out)[0, n) = (d_keys_in, d_vals_in)
 * stably sorted by key bits [bit0, bit1) (descending != 0: by the complemented bits, equal keys in input order),
 * keys of key_bytes (4 or 8) bytes, 32-bit values; device arrays, on hip_stream (then synchronised). */
COOC_API int cooc_selftest_radix(const void *d_keys_in, const void *d_vals_in, void *d_keys_out, void *d_vals_out,
                                 int64_t n, int32_t key_bytes, int32_t bit0, int32_t bit1, int32_t descending,
                                 void *hip_stream);
/* Self-test of the planner's flag compaction: d_out[0, *d_n_sel) = the indices i < n with d_flags[i] != 0,
 * ascending (device arrays; *d_n_sel is a device int32). */
COOC_API int cooc_selftest_select(const uint8_t *d_flags, int64_t n, int32_t *d_out, int32_t *d_n_sel,
                                  void *hip_stream);
/* Self-test of the owner's merge: cooc_merge_partitions (same arguments, same result) with the choice a sampled
 * multi-GPU window makes inside the library.  flags & 1: the counts are signed nets in two's complement; a key
 * stays when any source sent it, also at net 0, the row sums (d_rowsum_global and out->rowsum) are sums of the
 * sign-extended nets, and the dense merge then ends at 39,470 items (one touched bit per column behind the row).
 * flags == 0 is cooc_merge_partitions. */
COOC_API int cooc_selftest_merge(cooc_ctx *ctx, int32_t n_parts, int32_t part, const int32_t *d_recv_row_nnz,
                                 const uint64_t *d_recv_entries, const int64_t *d_rowsum_global, int32_t flags,
                                 void *hip_stream, cooc_device_result *out);

#ifdef __cplusplus
}
#endif
#endif /* COOC_H_ */
