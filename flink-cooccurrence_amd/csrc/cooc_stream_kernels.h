// cooc_stream_kernels.h — launch wrappers of cooc_stream.hip (resident streaming state); the rescoring of its rows:
// cooc_rescore.h.
#pragma once

#include "cooc_device.h"

namespace cooc {

Status launch_relocate(hipStream_t s, int64_t n, const int64_t *reloc, int32_t *arena);
// list j of len[j] ids at arena offset off[j] -> out[dst[j] ..) (contiguous CSR of arena slabs)
Status launch_gather_lists(hipStream_t s, int64_t n, const int64_t *off, const int32_t *len, const int64_t *dst,
                           const int32_t *arena, int32_t *out);
Status launch_append(hipStream_t s, int64_t n, const int64_t *new_ptr, const int64_t *new_dst, const int32_t *items,
                     int32_t *arena);
// scal: [0] touched rows, [1] sum of the window's int row-sum deltas, [2] rescorer observed
// (cumulative), [3] exact observed (cumulative).
Status launch_merge_global(hipStream_t s, int32_t M, const int64_t *row_base, const int32_t *row_nnz,
                           const int32_t *col, const uint32_t *cnt, const int64_t *rowsum_delta, uint32_t *G,
                           int64_t *grs, int64_t *scal, int64_t observed_window);
// p > 1 windows: the owner's merged rows (R rows a = part + r W) as an M-row view (base, nnz: zero elsewhere);
// their entries merged into the dense global rows G and every item's all-reduced row-sum delta rs_all into grs
// (scal[1]: sum of the int views over all items, scal[4]: over the owned rows with a delta); the view packed for
// copy-out (rp int64[M+1], *total entries; synchronises s).
Status launch_owned_view(hipStream_t s, int32_t M, int32_t W, int32_t part, int32_t R, const int64_t *mbase,
                         const int32_t *mnnz, int64_t *base, int32_t *nnz);
Status launch_merge_owned(hipStream_t s, int32_t M, const int64_t *base, const int32_t *nnz, const int32_t *col,
                          const uint32_t *cnt, const int64_t *rs_all, uint32_t *G, int64_t *grs, int64_t *scal,
                          int64_t observed_window);
Status launch_pack_rows(hipStream_t s, int32_t M, const int64_t *base, const int32_t *nnz, const int32_t *col,
                        const uint32_t *cnt, DevBuf &rp, DevBuf &out_col, DevBuf &out_cnt, DevBuf &tmp, int64_t *total);
// kMax cap of a device CSR: cut_ptr int64[n_users+1], cut_items int32[<= n]; *n_cut = cut_ptr[n_users]
// (read back: the caller sizes the next pass with it).
Status launch_user_cut(hipStream_t s, int64_t n_users, const int64_t *up, const int32_t *items, int32_t cut,
                       int64_t *cut_ptr, int32_t *cut_items, DevBuf &tmp, int64_t *n_cut);
Status launch_touched(hipStream_t s, int32_t M, const int32_t *row_nnz, int32_t *touched, int64_t *n_touched,
                      DevBuf &tmp);

// Sparse global rows (n_items >= 40,320; the rescorer's itemRows, ItemRowRescorer...java:35,171-177):
// row a = len[a] (column, count) entries in ascending column order at base[a] of the arena (col, cnt).
// Rows move to a new bump-allocated slab when a window touches them; live = entries of all rows;
// the arena is compacted (rows re-laid in order) when a window would not fit behind the bump
// (struct GlobalSparse, cooc_device.h).
// Merge a window's packed delta rows (drp int64[M+1], dcol, dcnt; nnz entries) into the rows;
// *new_cols = the window's new (row, column) keys.  Synchronises the stream.
Status launch_gs_merge(hipStream_t s, int32_t M, const int64_t *drp, const int32_t *dcol, const uint32_t *dcnt,
                       int64_t nnz, GlobalSparse &g, DevBuf &tmp, int64_t *new_cols);
Status compact_global(hipStream_t s, int32_t M, GlobalSparse &g, DevBuf &tmp, int64_t new_cap);

// ---- sampled mode (cooc_sampled.hip) ---------------------------------------------------------------------
// One user whose reservoir the window changed (k_sm_lists).  len_old / len_new: |H| before and after the window;
// the appended items are app[app_begin, app_begin + len_new - len_old), the replacements the (slot, item) pairs
// rep[2 rep_begin, 2 (rep_begin + n_rep)) in arrival order; n_unchanged = len_old - the distinct replaced slots
// below len_old; plus_dst / minus_dst: where the user's lists start (minus_dst < 0: no minus list).
struct SmUser {
  int64_t arena_off, plus_dst, minus_dst;
  int32_t len_old, len_new, n_unchanged, app_begin, rep_begin, n_rep;
};
// Applies the window to the arena and writes the plus and minus lists; *err (device) != 0 afterwards: a bound
// was violated (nothing was written outside the arena slabs and the lists).
Status launch_sm_lists(hipStream_t s, int64_t n, const SmUser *users, const int32_t *app, const int32_t *rep,
                       int32_t *arena, int64_t arena_len, int32_t *lists, int64_t lists_len, int32_t *err);
// The signed delta of a window: a packed M-row CSR (rp int64[M+1], col, cnt: two's complement nets, zero nets
// kept), its rows' lengths and the row-sum differences.
struct SignedDelta {
  DevBuf rp, nnz, col, cnt, rowsum, flag, opos, newpre, err;
  int64_t entries = 0;
  void release() { *this = SignedDelta(); }
};
// plus - minus over two packed M-row CSRs with ascending columns (n_plus, n_minus entries; prs, mrs their row
// sums): the union of the keys.  Synchronises the stream.
Status launch_signed_delta(hipStream_t s, int32_t M, const int64_t *prp, const int32_t *pcol, const uint32_t *pcnt,
                           const int64_t *prs, int64_t n_plus, const int64_t *mrp, const int32_t *mcol,
                           const uint32_t *mcnt, const int64_t *mrs, int64_t n_minus, SignedDelta &d, DevBuf &tmp);

}  // namespace cooc
