// cooc_snapshot_pack.hip — checkpoint of the streaming state (cooc_snapshot_prepare, cooc_snapshot_copy).
//
// Everything the streaming entry points keep between windows is Flink keyed state in the reference: windowState
// and userHistoryState (NonSampled...java:73-77), the rescorer's itemRows and globalItemRowSums
// (ItemRowRescorer...java:33-41).  Here it is packed into one canonical blob (cooc_snapshot.h):
//
//   pack     k_snap_dense_rows   dense global matrix -> packed rows: one wave per row, 16-B loads, a count pass
//                                (ballot + popcount) and, after a scan of the row counts, a write pass that
//                                places every non-zero cell by the ballots' prefix (column order)
//            launch_pack_rows    row slabs -> packed rows (cooc_stream.hip)
//            k_snap_flags + select_flagged + k_snap_gather_rows   the non-empty rows' ids, offsets, row sums
//            k_snap_copy_lists   history arena -> histories back to back (long lists in 2,048-id pieces); a restore
//                                runs it the other way (launch_copy_lists)
//   both     k_snap_checksum     per section, the sum over its 8-B words w_i of splitmix64(w_i ^ i)
//                                (launch_checksums: a restore holds the blob's sums against it)
//   sampled  a sampled context's blob is format 2 (cooc_snapshot.h): the same code with five more sections
//            ScanLiveU32 + k_snap_live_rows + k_snap_compact   slab entries whose count went back to 0 dropped
//            k_snap_count_flags + select_flagged + k_snap_gather_counts / k_snap_gather_totals   the device
//                                sampler's non-zero item counters and the users' totals, in id order
//
// All of it is bandwidth-bound and runs on the context's stream.  The restore is cooc_snapshot_restore.hip, the
// restore into another parallelism cooc_snapshot_rescale.hip.
#include <cstring>
#include <utility>

#include "cooc_radix.h"
#include "cooc_snapshot_impl.h"

namespace cooc {
namespace {

// ---- checksum -------------------------------------------------------------------------------------------------
struct SnapSpans {
  int64_t off[kSnapSectionsMax];    // in 8-B words from the image's start
  int64_t words[kSnapSectionsMax];
};

__global__ __launch_bounds__(256) void k_snap_checksum(const uint64_t *__restrict__ img, SnapSpans S,
                                                       unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long s_w[4];
  const int k = blockIdx.y;
  const uint64_t *w = img + S.off[k];
  const int64_t n = S.words[k];
  unsigned long long acc = 0;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    acc += snap_splitmix64(w[i] ^ uint64_t(i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (t) atomicAdd(&sums[k], t);  // one atomic per workgroup
  }
}

}  // namespace

Status launch_checksums(hipStream_t s, const void *img, const SnapHeader &h, unsigned long long *sums) {
  SnapSpans S = {};
  int64_t most = 1;
  for (int k = 0; k < h.n_sections; k++) {
    S.off[k] = h.sec[k].offset / 8;
    S.words[k] = snap_pad8(h.sec[k].bytes) / 8;
    most = std::max(most, S.words[k]);
  }
  COOC_HIP_TRY(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * kSnapSectionsMax, s));
  const dim3 grid(std::min<unsigned>(blocks_for(most, 256 * 8), 2048), unsigned(h.n_sections));
  k_snap_checksum<<<grid, 256, 0, s>>>(static_cast<const uint64_t *>(img), S, sums);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

namespace {

// ---- dense global matrix -> packed rows -----------------------------------------------------------------------
// One wave per row.  Row a starts at word a * M of a 256-B aligned matrix, so it is 16-B aligned only when
// a * M is a multiple of 4: up to 3 head words (one per lane), then uint4 groups (one per lane and step), then up
// to 3 tail words; nothing past the row is read.  A step's non-zero cells are found with one ballot per vector
// component; kWrite places them at the row's packed offset in column order: the cells of lower lanes (popcount
// of the ballots below this lane), then this lane's own lower components.
template <bool kWrite>
__global__ __launch_bounds__(256) void k_snap_dense_rows(int32_t M, const uint32_t *__restrict__ G,
                                                         const int64_t *__restrict__ rp, int32_t *__restrict__ nnz_out,
                                                         int32_t *__restrict__ col_out, uint32_t *__restrict__ cnt_out) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t a = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; a < M; a += n_waves) {
    const int64_t w0 = a * int64_t(M);
    const uint32_t *row = G + w0;
    const int32_t head = min(M, int32_t((4 - (w0 & 3)) & 3));
    const int32_t nvec = (M - head) >> 2, tail0 = head + nvec * 4;
    const int64_t out = kWrite ? rp[a] : 0;
    int32_t n = 0;  // the row's cells so far (wave-uniform)
    auto step = [&](uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int32_t c0) {
      const uint64_t m0 = __ballot(v0 != 0), m1 = __ballot(v1 != 0), m2 = __ballot(v2 != 0), m3 = __ballot(v3 != 0);
      if (kWrite) {
        int64_t o = out + n + __popcll(m0 & lt) + __popcll(m1 & lt) + __popcll(m2 & lt) + __popcll(m3 & lt);
        if (v0) { col_out[o] = c0; cnt_out[o] = v0; o++; }
        if (v1) { col_out[o] = c0 + 1; cnt_out[o] = v1; o++; }
        if (v2) { col_out[o] = c0 + 2; cnt_out[o] = v2; o++; }
        if (v3) { col_out[o] = c0 + 3; cnt_out[o] = v3; }
      }
      n += __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
    };
    if (head) step(lane < head ? row[lane] : 0u, 0u, 0u, 0u, lane);
    const uint4 *rv = reinterpret_cast<const uint4 *>(row + head);
    for (int32_t g0 = 0; g0 < nvec; g0 += 64) {  // (uniform trip count: every lane takes part in the ballots)
      const int32_t g = g0 + lane;
      const uint4 x = g < nvec ? rv[g] : make_uint4(0u, 0u, 0u, 0u);
      step(x.x, x.y, x.z, x.w, head + g * 4);
    }
    if (tail0 < M) step(tail0 + lane < M ? row[tail0 + lane] : 0u, 0u, 0u, 0u, tail0 + lane);
    if (!kWrite && lane == 0) nnz_out[a] = n;
  }
}

// flag[a]: row a has entries; xflag[a] (world > 1): it has none here but the item has a row sum (its row lives
// on another rank)
__global__ void k_snap_flags(int32_t M, const int32_t *__restrict__ len, const int64_t *__restrict__ grs,
                             uint8_t *__restrict__ flag, uint8_t *__restrict__ xflag) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  const bool has = len[a] > 0;
  flag[a] = has ? 1 : 0;
  xflag[a] = (!has && grs[a] != 0) ? 1 : 0;
}

// the non-empty rows' packed offsets (rp: the prefix over all M rows; empty rows add nothing) and row sums
__global__ void k_snap_gather_rows(int64_t R, int32_t M, const int32_t *__restrict__ ids, const int64_t *__restrict__ rp,
                                   const int64_t *__restrict__ grs, int64_t *__restrict__ ptr_out,
                                   int64_t *__restrict__ sums_out) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r > R) return;
  if (r == R) {
    ptr_out[R] = rp[M];
    return;
  }
  const int32_t a = ids[r];
  ptr_out[r] = rp[a];
  sums_out[r] = grs[a];
}

__global__ void k_snap_gather_i64(int64_t n, const int32_t *__restrict__ ids, const int64_t *__restrict__ src,
                                  int64_t *__restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[ids[i]];
}

// List j = ptr[j + 1] - ptr[j] ids, at ptr[j] of the packed array and at aoff[j] of the arena; copied packed <- arena
// (kToPacked) or arena <- packed, in pieces of kListChunk ids, one wave per piece: piece c belongs to the list j
// with chunk_pre[j] <= c < chunk_pre[j + 1], so a long list is spread over many waves.
template <bool kToPacked>
__global__ __launch_bounds__(256) void k_snap_copy_lists(int64_t n_lists, int64_t n_chunks,
                                                         const int64_t *__restrict__ chunk_pre,
                                                         const int64_t *__restrict__ ptr, const int64_t *__restrict__ aoff,
                                                         const int32_t *__restrict__ src, int32_t *__restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t c = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    int64_t lo = 0, hi = n_lists;  // invariant: chunk_pre[lo] <= c < chunk_pre[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (chunk_pre[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t p = ptr[lo], n = ptr[lo + 1] - p, a = aoff[lo];
    const int64_t i0 = (c - chunk_pre[lo]) * kListChunk, i1 = min(n, i0 + kListChunk);
    for (int64_t i = i0 + lane; i < i1; i += 64) {
      if (kToPacked) dst[p + i] = src[a + i];
      else dst[a + i] = src[p + i];
    }
  }
}

// ---- sampled contexts (format 2) ------------------------------------------------------------------------------
// pack.  A sampled context's slabs keep entries whose count went back to 0 (not keys: DESIGN.md §5c "Global
// state"); the blob drops them.  live[e] = the live entries before packed entry e (an exclusive scan of
// cnt != 0 over the nnz entries and one closing element, so live[nnz] is their number).
struct ScanLiveU32 {
  const uint32_t *cnt;
  int64_t n;
  __device__ int64_t operator()(int64_t i) const { return i < n && cnt[i] != 0u ? 1 : 0; }
};

// the rows' offsets and lengths recounted over the live entries: rp_out[a] = live[rp[a]] for a in [0, M]
__global__ __launch_bounds__(256) void k_snap_live_rows(int32_t M, const int64_t *__restrict__ rp,
                                                        const int64_t *__restrict__ live, int64_t *__restrict__ rp_out,
                                                        int32_t *__restrict__ len_out) {
  const int64_t a = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (a > M) return;
  const int64_t b = live[rp[a]];
  rp_out[a] = b;
  if (a < M) len_out[a] = int32_t(live[rp[a + 1]] - b);
}

// the live entries to their places (column order within a row is kept: the scan is monotone)
__global__ __launch_bounds__(256) void k_snap_compact(int64_t nnz, const int64_t *__restrict__ live,
                                                      const int32_t *__restrict__ col, const uint32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ col_out, uint32_t *__restrict__ cnt_out) {
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < nnz; e += int64_t(gridDim.x) * 256) {
    const uint32_t c = cnt[e];
    if (c != 0u) {
      const int64_t o = live[e];
      col_out[o] = col[e];
      cnt_out[o] = c;
    }
  }
}

// the device sampler's item counters: flag[i] = count[i] != 0, then (after select_flagged) the selected items'
// counters as int16
__global__ __launch_bounds__(256) void k_snap_count_flags(int32_t M, const int32_t *__restrict__ count,
                                                          uint8_t *__restrict__ flag) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) flag[i] = count[i] != 0 ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_snap_gather_counts(int64_t n, const int32_t *__restrict__ ids,
                                                            const int32_t *__restrict__ count, int16_t *__restrict__ out) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k < n) out[k] = int16_t(count[ids[k]]);
}
// the device sampler's totals of the users in id order: out[j] = T[slots[j]]; a slot outside the per-slot state or
// a total below 1 sets `bit` (the host's tables and the device's state out of step; nothing is read out of range)
__global__ __launch_bounds__(256) void k_snap_gather_totals(int64_t n, const int32_t *__restrict__ slots,
                                                            const int32_t *__restrict__ T, int64_t slot_cap,
                                                            int32_t *__restrict__ out, unsigned int *err, unsigned int bit) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (j < n) {
    const int32_t slot = slots[j];
    int32_t t = 0;
    if (slot >= 0 && int64_t(slot) < slot_cap) t = T[slot];
    bad = t < 1;
    out[j] = t;
  }
  val_fold(bad, err, bit);
}

// section `kind` of the image from host memory (asynchronous: src outlives the caller's next synchronisation)
Status put(hipStream_t s, const BlobImage &v, int kind, const void *src) {
  if (v.bytes(kind) > 0) COOC_HIP_TRY(hipMemcpyAsync(v.raw(kind), src, size_t(v.bytes(kind)), hipMemcpyHostToDevice, s));
  return Status::Ok();
}

}  // namespace

Status launch_copy_lists(cooc_ctx &ctx, bool to_packed, const std::vector<int64_t> &chunk_pre,
                         const std::vector<int64_t> &aoff, const int64_t *d_ptr, const int32_t *src, int32_t *dst) {
  hipStream_t s = ctx.stream;
  const size_t n = aoff.size();
  Carve c;
  const auto pre = c.take<int64_t>(n + 1), off = c.take_last<int64_t>(n);
  COOC_TRY(ctx.snap_tmp2.reserve(c.end));
  int64_t *d_pre = pre.in(ctx.snap_tmp2), *d_aoff = off.in(ctx.snap_tmp2);
  COOC_HIP_TRY(hipMemcpyAsync(d_pre, chunk_pre.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(d_aoff, aoff.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
  const int64_t n_chunks = chunk_pre[n];
  if (to_packed) k_snap_copy_lists<true><<<wave_grid(n_chunks), 256, 0, s>>>(int64_t(n), n_chunks, d_pre, d_ptr, d_aoff, src, dst);
  else k_snap_copy_lists<false><<<wave_grid(n_chunks), 256, 0, s>>>(int64_t(n), n_chunks, d_pre, d_ptr, d_aoff, src, dst);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

SnapHeader Snapshotter::header_for(const cooc_ctx &ctx, const SnapCounts &c) {
  SnapHeader h;
  std::memset(&h, 0, sizeof(h));
  auto sec = [&](int kind) -> SnapSection & { return h.sec[kind - 1]; };
  sec(kSnapScalars).count = kSnapScalarWords;
  sec(kSnapUserIds).count = c.users;
  sec(kSnapHistPtr).count = c.users + 1;
  sec(kSnapHistItems).count = c.hist_items;
  sec(kSnapRowIds).count = sec(kSnapRowSums).count = c.rows;
  sec(kSnapRowPtr).count = c.rows + 1;
  sec(kSnapRowCols).count = sec(kSnapRowCnts).count = c.entries;
  sec(kSnapXsumIds).count = sec(kSnapXsumVals).count = c.xsums;
  sec(kSnapPendTs).count = c.pend_windows;
  sec(kSnapPendPtr).count = c.pend_windows + 1;
  sec(kSnapPendUsers).count = sec(kSnapPendItems).count = c.pend_records;
  const int32_t format = format_of(ctx);
  if (format == kSnapFormatSampled) {
    sec(kSnapSmpScalars).count = kSnapSmpScalarWords;
    sec(kSnapSmpItemIds).count = sec(kSnapSmpItemCnts).count = c.counted_items;
    sec(kSnapSmpUserIds).count = sec(kSnapSmpTotals).count = c.total_users;
  }
  snap_layout(&h, format);
  h.n_items = ctx.cfg.n_items;
  h.user_cut = ctx.cfg.user_cut;
  h.window_size_ms = ctx.cfg.window_size_ms;
  h.rank = ctx.comm ? ctx.comm->rank() : 0;
  h.world = ctx.comm ? ctx.comm->world() : 1;
  return h;
}

PendingWindows Snapshotter::flatten(const std::map<int64_t, Operator::Pending> &pending) {
  PendingWindows p;
  p.ptr.push_back(0);
  for (const auto &kv : pending) {  // (std::map: ascending maxTimestamp)
    p.ts.push_back(kv.first);
    p.users.insert(p.users.end(), kv.second.users.begin(), kv.second.users.end());
    p.items.insert(p.items.end(), kv.second.items.begin(), kv.second.items.end());
    p.ptr.push_back(int64_t(p.users.size()));
  }
  return p;
}

// ---- the tables of one prepare ----------------------------------------------------------------------------------
// Host: the users with a history in ascending id order (their histories' offsets in the blob and places in the
// arena) and the operator's buffered windows in timestamp order.  A sampled context's blob also names every user
// with a total (a superset: a user whose every record was rejected at the item cut has no history).  The host
// sampler's totals and counters are read here; the device sampler's are gathered on the device, where every slot
// has a total (a slot is made for a record of a finished window).
struct PackTables {
  std::vector<int32_t> user_ids;
  std::vector<int64_t> hist_ptr, aoff;
  std::vector<int32_t> tot_ids, tot_slots, totals;  // (totals, cnt_ids, cnts: host sampler only)
  std::vector<int32_t> cnt_ids;
  std::vector<int16_t> cnts;
  PendingWindows pend;
};

// Device (snap_tmp): M-sized arrays for the flags and selections over the items.  n_sel = {rows, rows of other
// ranks, counted items}.
struct PackScratch {
  int32_t *counted = nullptr;
  uint8_t *flag = nullptr, *xflag = nullptr;
  int32_t *ids = nullptr, *xids = nullptr, *n_sel = nullptr;
  char *sel = nullptr;
  int32_t *cids = nullptr;
  Status reserve(DevBuf &buf, int32_t M) {
    const size_t m = size_t(M);
    Carve c;
    const auto o_counted = c.take<int32_t>(m);
    const auto o_flag = c.take<uint8_t>(m), o_xflag = c.take<uint8_t>(m);
    const auto o_ids = c.take<int32_t>(m), o_xids = c.take<int32_t>(m), o_nsel = c.take<int32_t>(3);
    const auto o_sel = c.take<char>(select_tmp_bytes(M));
    const auto o_cids = c.take<int32_t>(m);
    COOC_TRY(buf.reserve(c.end));
    counted = o_counted.in(buf), flag = o_flag.in(buf), xflag = o_xflag.in(buf), ids = o_ids.in(buf);
    xids = o_xids.in(buf), n_sel = o_nsel.in(buf), sel = o_sel.in(buf), cids = o_cids.in(buf);
    return Status::Ok();
  }
};

// The global rows packed: the prefix rp over all M rows and the entries (nnz of them in the blob).  Sampled slabs:
// live = the live entries before each of the n_packed packed entries (dead ones included).  R rows have entries,
// X items have a row sum and their row on another rank.
struct PackedRows {
  const int64_t *rp = nullptr, *live = nullptr;
  int64_t nnz = 0, n_packed = 0, R = 0, X = 0;
};

PackTables Snapshotter::host_tables(const cooc_ctx &ctx) {
  const StreamState &st = ctx.stream_state;
  const bool sampled = st.sampled(), dev_sampled = st.dev_sampler_.enabled();
  PackTables t;
  std::vector<std::pair<int32_t, int32_t>> users, tot_users;  // (user id, slot): non-empty histories; totals
  auto add_user = [&](int32_t uid, int32_t slot) {
    if (st.h_len_[slot] > 0) users.emplace_back(uid, slot);
    if (sampled && (dev_sampled || st.sampler_.total(slot) > 0)) tot_users.emplace_back(uid, slot);
  };
  for (size_t u = 0; u < st.dense_slot_.size(); u++)
    if (st.dense_slot_[u] >= 0) add_user(int32_t(u), st.dense_slot_[u]);
  for (const auto &kv : st.slot_of_) add_user(kv.first, kv.second);
  std::sort(users.begin(), users.end());
  std::sort(tot_users.begin(), tot_users.end());
  const int64_t n_tot = int64_t(tot_users.size());
  t.tot_ids.resize(n_tot);
  t.tot_slots.resize(n_tot);
  for (int64_t j = 0; j < n_tot; j++) {
    t.tot_ids[j] = tot_users[j].first;
    t.tot_slots[j] = tot_users[j].second;
  }
  if (sampled && !dev_sampled) {
    t.totals.resize(n_tot);
    for (int64_t j = 0; j < n_tot; j++) t.totals[j] = st.sampler_.total(t.tot_slots[j]);
    for (int32_t i = 0; i < ctx.cfg.n_items; i++)
      if (st.sampler_.item_count(i) != 0) {
        t.cnt_ids.push_back(i);
        t.cnts.push_back(st.sampler_.item_count(i));
      }
  }
  const int64_t n_users = int64_t(users.size());
  t.user_ids.resize(n_users);
  t.hist_ptr.assign(n_users + 1, 0);
  t.aoff.resize(n_users);
  for (int64_t j = 0; j < n_users; j++) {
    t.user_ids[j] = users[j].first;
    t.aoff[j] = st.h_off_[users[j].second];
    t.hist_ptr[j + 1] = t.hist_ptr[j] + st.h_len_[users[j].second];
  }
  t.pend = flatten(ctx.op.pending_);
  return t;
}

Status Snapshotter::pack_global_rows(cooc_ctx &ctx, const PackScratch &sc, PackedRows *out) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  PackedRows &g = *out;
  const int32_t *lens = nullptr;
  if (st.sparse_global_) {  // (synchronises s)
    COOC_TRY(launch_pack_rows(s, M, st.gs_.base.as<int64_t>(), st.gs_.len.as<int32_t>(), st.gs_.col.as<int32_t>(),
                              st.gs_.cnt.as<uint32_t>(), ctx.snap_rp, ctx.snap_col, ctx.snap_cnt, st.d_scan_tmp_, &g.nnz));
    lens = st.gs_.len.as<int32_t>();
    if (st.sampled() && g.nnz > 0) {
      // entries whose count went back to 0 are no keys: flagged, scanned, and the rows recounted without them
      g.n_packed = g.nnz;
      Carve c;
      const auto o_rp = c.take<int64_t>(size_t(M) + 1);
      const auto o_len = c.take<int32_t>(size_t(M));
      const auto o_live = c.take_last<int64_t>(size_t(g.n_packed + 1));
      COOC_TRY(ctx.snap_live.reserve(c.end));
      COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(g.n_packed + 1)));
      int64_t *d_rp2 = o_rp.in(ctx.snap_live), *d_live = o_live.in(ctx.snap_live);
      int32_t *d_len2 = o_len.in(ctx.snap_live);
      int64_t serr = 0;
      COOC_TRY(launch_scan_ws<false>(ScanLiveU32{ctx.snap_cnt.as<uint32_t>(), g.n_packed}, d_live, g.n_packed + 1,
                                     st.d_scan_tmp_.as<unsigned long long>(), &serr, s));
      k_snap_live_rows<<<blocks_for(int64_t(M) + 1, 256), 256, 0, s>>>(M, ctx.snap_rp.as<int64_t>(), d_live, d_rp2, d_len2);
      COOC_HIP_TRY(hipGetLastError());
      COOC_HIP_TRY(hipMemcpyAsync(&g.nnz, d_live + g.n_packed, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if ((serr & 8) || g.nnz < 0 || g.nnz > g.n_packed)
        return Status{COOC_ERR_STATE, "internal bounds check failed (snapshot live entries)"};
      g.live = d_live;
      g.rp = d_rp2;
      lens = d_len2;
    }
  } else {
    COOC_TRY(ctx.snap_rp.reserve(sizeof(int64_t) * (size_t(M) + 1)));
    COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(M)));
    k_snap_dense_rows<false><<<wave_grid(M), 256, 0, s>>>(M, st.d_global_.as<uint32_t>(), nullptr, sc.counted, nullptr,
                                                           nullptr);
    COOC_HIP_TRY(hipGetLastError());
    int64_t *d_rp = ctx.snap_rp.as<int64_t>();
    COOC_HIP_TRY(hipMemsetAsync(d_rp, 0, sizeof(int64_t), s));
    int64_t serr = 0;
    COOC_TRY(launch_scan_ws<true>(ScanI32{sc.counted}, d_rp + 1, M, st.d_scan_tmp_.as<unsigned long long>(), &serr, s));
    COOC_HIP_TRY(hipMemcpyAsync(&g.nnz, d_rp + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (serr & 8) return Status{COOC_ERR_STATE, "internal bounds check failed (snapshot row prefix)"};
    lens = sc.counted;
  }
  if (!g.rp) g.rp = ctx.snap_rp.as<int64_t>();
  const bool multi = ctx.comm && ctx.comm->world() > 1;
  int32_t n_sel[2] = {0, 0};
  k_snap_flags<<<blocks_for(M, 256), 256, 0, s>>>(M, lens, st.d_grs_.as<int64_t>(), sc.flag, sc.xflag);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemsetAsync(sc.n_sel, 0, sizeof(int32_t) * 2, s));
  COOC_TRY(select_flagged(sc.flag, M, sc.ids, sc.n_sel, sc.sel, s));
  if (multi) COOC_TRY(select_flagged(sc.xflag, M, sc.xids, sc.n_sel + 1, sc.sel, s));
  COOC_HIP_TRY(hipMemcpyAsync(n_sel, sc.n_sel, sizeof(n_sel), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  g.R = n_sel[0];
  g.X = n_sel[1];
  return Status::Ok();
}

// the device sampler's counted items (the row flags are done with)
Status Snapshotter::count_sampler_items(cooc_ctx &ctx, const PackScratch &sc, int64_t *n_cnt) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  int32_t n_sel_c = 0;
  k_snap_count_flags<<<blocks_for(M, 256), 256, 0, s>>>(M, st.dev_sampler_.count_.as<int32_t>(), sc.flag);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemsetAsync(sc.n_sel + 2, 0, sizeof(int32_t), s));
  COOC_TRY(select_flagged(sc.flag, M, sc.cids, sc.n_sel + 2, sc.sel, s));
  COOC_HIP_TRY(hipMemcpyAsync(&n_sel_c, sc.n_sel + 2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (n_sel_c < 0 || n_sel_c > M) return Status{COOC_ERR_STATE, "internal bounds check failed (counted items)"};
  *n_cnt = n_sel_c;
  return Status::Ok();
}

// section 1: the accumulators, the operator's scalars and the running totals of d_scal_ (synchronises s)
Status Snapshotter::host_scalars(cooc_ctx &ctx, int64_t *scalars) {
  const StreamState &st = ctx.stream_state;
  const Operator &op = ctx.op;
  int64_t scal[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (st.global_ready_) COOC_HIP_TRY(hipMemcpyAsync(scal, st.d_scal_.p, sizeof(scal), hipMemcpyDeviceToHost, ctx.stream));
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  scalars[kScObservedExact] = st.observed_exact;
  scalars[kScObservedRef] = st.observed_ref;
  scalars[kScRowsumAcc] = st.rowsum_acc;
  scalars[kScRescoredItems] = st.rescored_items;
  scalars[kScLateElements] = op.late_elements;
  scalars[kScWatermark] = op.watermark;
  scalars[kScAgreed] = op.agreed_;
  scalars[kScRegather] = op.regather_ ? 1 : 0;
  scalars[kScScal2] = scal[2];
  scalars[kScScal3] = scal[3];
  return Status::Ok();
}

// The sampler's state: from the host sampler's vectors, or gathered from the device sampler's arrays.  smp (the
// caller's, kSnapSmpScalarWords zeros) is filled and uploaded.
Status Snapshotter::put_sampler_sections(cooc_ctx &ctx, const BlobImage &v, const PackTables &t, const PackScratch &sc,
                                         int64_t *smp) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int64_t n_cnt = v.count(kSnapSmpItemIds), n_tot = v.count(kSnapSmpUserIds);
  int64_t ctr[6] = {0, 0, 0, 0, 0, 0};
  COOC_TRY(st.sampling_counters(ctx, ctr));  // (synchronises s in device mode)
  smp[kSsItemCut] = st.sampler_.item_cut();
  smp[kSsSeed] = int64_t(st.sampler_.seed());
  smp[kSsRejected] = ctr[0];
  smp[kSsFills] = ctr[1];
  smp[kSsReplacements] = ctr[2];
  smp[kSsFeedbacks] = ctr[3];
  COOC_TRY(put(s, v, kSnapSmpScalars, smp));
  COOC_TRY(put(s, v, kSnapSmpUserIds, t.tot_ids.data()));
  if (!st.dev_sampler_.enabled()) {
    COOC_TRY(put(s, v, kSnapSmpItemIds, t.cnt_ids.data()));
    COOC_TRY(put(s, v, kSnapSmpItemCnts, t.cnts.data()));
    COOC_TRY(put(s, v, kSnapSmpTotals, t.totals.data()));
    COOC_HIP_TRY(hipStreamSynchronize(s));  // (the uploads read the caller's vectors)
    return Status::Ok();
  }
  if (n_cnt > 0) {
    COOC_HIP_TRY(hipMemcpyAsync(v.raw(kSnapSmpItemIds), sc.cids, sizeof(int32_t) * size_t(n_cnt), hipMemcpyDeviceToDevice, s));
    k_snap_gather_counts<<<blocks_for(n_cnt, 256), 256, 0, s>>>(n_cnt, sc.cids, st.dev_sampler_.count_.as<int32_t>(),
                                                                v.at<int16_t>(kSnapSmpItemCnts));
    COOC_HIP_TRY(hipGetLastError());
  }
  if (n_tot > 0) {
    // the (id-sorted user -> slot) table up, the totals gathered by slot; the error word follows the padded table
    // (4 n_tot is a multiple of 4, so it is inside the 256 B added)
    Carve c;
    const auto o_slots = c.take<int32_t>(size_t(n_tot));
    const auto o_terr = c.take_last<unsigned int>(1);
    COOC_TRY(ctx.snap_tmp2.reserve(sizeof(int32_t) * size_t(n_tot) + 256));
    int32_t *d_slots = o_slots.in(ctx.snap_tmp2);
    unsigned int *d_terr = o_terr.in(ctx.snap_tmp2);
    unsigned int terr = 0;
    COOC_HIP_TRY(hipMemcpyAsync(d_slots, t.tot_slots.data(), sizeof(int32_t) * size_t(n_tot), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemsetAsync(d_terr, 0, sizeof(unsigned int), s));
    k_snap_gather_totals<<<blocks_for(n_tot, 256), 256, 0, s>>>(n_tot, d_slots, st.dev_sampler_.total_.as<int32_t>(),
                                                                st.dev_sampler_.slot_cap_, v.at<int32_t>(kSnapSmpTotals),
                                                                d_terr, 1u);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemcpyAsync(&terr, d_terr, sizeof(terr), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (terr) return Status{COOC_ERR_STATE, "internal error: a user slot without a total on the device sampler"};
  }
  return Status::Ok();
}

// sections 5 - 11: the packed rows into the image
Status Snapshotter::put_row_sections(cooc_ctx &ctx, const BlobImage &v, const PackedRows &g, const PackScratch &sc) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  if (!st.global_ready_) {
    COOC_HIP_TRY(hipMemsetAsync(v.raw(kSnapRowPtr), 0, sizeof(int64_t), s));
    return Status::Ok();
  }
  const int64_t *grs = st.d_grs_.as<int64_t>();
  if (g.R > 0) COOC_HIP_TRY(hipMemcpyAsync(v.raw(kSnapRowIds), sc.ids, sizeof(int32_t) * size_t(g.R), hipMemcpyDeviceToDevice, s));
  k_snap_gather_rows<<<blocks_for(g.R + 1, 256), 256, 0, s>>>(g.R, M, sc.ids, g.rp, grs, v.at<int64_t>(kSnapRowPtr),
                                                               v.at<int64_t>(kSnapRowSums));
  COOC_HIP_TRY(hipGetLastError());
  if (g.nnz > 0) {
    int32_t *col = v.at<int32_t>(kSnapRowCols);
    uint32_t *cnt = v.at<uint32_t>(kSnapRowCnts);
    if (g.live) {
      k_snap_compact<<<std::min<unsigned>(blocks_for(g.n_packed, 256 * 4), 4096), 256, 0, s>>>(
          g.n_packed, g.live, ctx.snap_col.as<int32_t>(), ctx.snap_cnt.as<uint32_t>(), col, cnt);
      COOC_HIP_TRY(hipGetLastError());
    } else if (st.sparse_global_) {
      COOC_HIP_TRY(hipMemcpyAsync(col, ctx.snap_col.p, sizeof(int32_t) * size_t(g.nnz), hipMemcpyDeviceToDevice, s));
      COOC_HIP_TRY(hipMemcpyAsync(cnt, ctx.snap_cnt.p, sizeof(uint32_t) * size_t(g.nnz), hipMemcpyDeviceToDevice, s));
    } else {
      k_snap_dense_rows<true><<<wave_grid(M), 256, 0, s>>>(M, st.d_global_.as<uint32_t>(), g.rp, nullptr, col, cnt);
      COOC_HIP_TRY(hipGetLastError());
    }
  }
  if (g.X > 0) {
    COOC_HIP_TRY(hipMemcpyAsync(v.raw(kSnapXsumIds), sc.xids, sizeof(int32_t) * size_t(g.X), hipMemcpyDeviceToDevice, s));
    k_snap_gather_i64<<<blocks_for(g.X, 256), 256, 0, s>>>(g.X, sc.xids, grs, v.at<int64_t>(kSnapXsumVals));
    COOC_HIP_TRY(hipGetLastError());
  }
  return Status::Ok();
}

// the sections' checksums, then the sealed header at the image's start
Status Snapshotter::seal(cooc_ctx &ctx, SnapHeader *h) {
  hipStream_t s = ctx.stream;
  char *img = ctx.snap_img.as<char>();
  COOC_TRY(ctx.snap_sums.reserve(sizeof(unsigned long long) * kSnapSectionsMax + sizeof(unsigned int) * 2));
  COOC_TRY(launch_checksums(s, img, *h, ctx.snap_sums.as<unsigned long long>()));
  unsigned long long sums[kSnapSectionsMax];
  COOC_HIP_TRY(hipMemcpyAsync(sums, ctx.snap_sums.p, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < h->n_sections; k++) h->sec[k].sum = sums[k];
  snap_seal(h);
  COOC_HIP_TRY(hipMemcpyAsync(img, h, size_t(snap_header_bytes(h->n_sections)), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  return Status::Ok();
}

Status Snapshotter::prepare(cooc_ctx &ctx, cooc_snapshot_info *info) {
  StreamState &st = ctx.stream_state;
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  if (st.staged_)
    return Status{COOC_ERR_STATE, "window " + std::to_string(st.staged_ts_) + " is staged; finish it before a snapshot"};
  ctx.snapshot_release();
  hipStream_t s = ctx.stream;
  const bool sampled = st.sampled(), dev_sampled = st.dev_sampler_.enabled();
  if (dev_sampled && (!st.dev_sampler_.count_.p || !st.dev_sampler_.ctr_.p))
    return Status{COOC_ERR_STATE, "the device sampler's state was released and not re-created"};

  // ---- host tables; the global rows packed; the device sampler's counted items
  const PackTables t = host_tables(ctx);  // (lives to the end: the image's uploads read its vectors)
  PackScratch sc;
  PackedRows g;
  if (st.global_ready_ || dev_sampled) COOC_TRY(sc.reserve(ctx.snap_tmp, ctx.cfg.n_items));
  if (st.global_ready_) COOC_TRY(pack_global_rows(ctx, sc, &g));
  int64_t n_cnt = int64_t(t.cnt_ids.size());
  if (dev_sampled) COOC_TRY(count_sampler_items(ctx, sc, &n_cnt));

  // ---- the image's layout
  const int64_t n_users = int64_t(t.user_ids.size());
  SnapCounts c;
  c.users = n_users;
  c.hist_items = t.hist_ptr[n_users];
  c.rows = g.R;
  c.entries = g.nnz;
  c.xsums = g.X;
  c.pend_windows = int64_t(t.pend.ts.size());
  c.pend_records = int64_t(t.pend.users.size());
  c.counted_items = n_cnt;
  c.total_users = int64_t(t.tot_ids.size());
  SnapHeader h = header_for(ctx, c);
  COOC_TRY(ctx.snap_img.reserve(size_t(h.total_bytes)));
  const BlobImage v{&h, ctx.snap_img.as<char>()};
  for (int k = 1; k <= h.n_sections; k++)  // the pad of a section whose bytes are no multiple of 8
    if (v.bytes(k) & 7) COOC_HIP_TRY(hipMemsetAsync(v.raw(k) + snap_pad8(v.bytes(k)) - 8, 0, 8, s));

  // ---- host-side sections, the sampler's state (the two scalar arrays are uploaded from here)
  int64_t scalars[kSnapScalarWords] = {0}, smp[kSnapSmpScalarWords] = {0};
  COOC_TRY(host_scalars(ctx, scalars));
  COOC_TRY(put(s, v, kSnapScalars, scalars));
  COOC_TRY(put(s, v, kSnapUserIds, t.user_ids.data()));
  COOC_TRY(put(s, v, kSnapHistPtr, t.hist_ptr.data()));
  COOC_TRY(put(s, v, kSnapPendTs, t.pend.ts.data()));
  COOC_TRY(put(s, v, kSnapPendPtr, t.pend.ptr.data()));
  COOC_TRY(put(s, v, kSnapPendUsers, t.pend.users.data()));
  COOC_TRY(put(s, v, kSnapPendItems, t.pend.items.data()));
  if (sampled) COOC_TRY(put_sampler_sections(ctx, v, t, sc, smp));

  // ---- histories: arena -> back to back; the global rows; checksums, then the header
  const std::vector<int64_t> chunk_pre = chunk_prefix(t.hist_ptr);
  if (n_users > 0)
    COOC_TRY(launch_copy_lists(ctx, true, chunk_pre, t.aoff, v.at<int64_t>(kSnapHistPtr), st.arena_.as<int32_t>(),
                               v.at<int32_t>(kSnapHistItems)));
  COOC_TRY(put_row_sections(ctx, v, g, sc));
  COOC_TRY(seal(ctx, &h));
  // (the packed slab rows were only a stage on the way into the image)
  ctx.snap_col.release();
  ctx.snap_cnt.release();
  ctx.snap_live.release();
  ctx.snap_bytes = h.total_bytes;
  snap_info(h, info);
  return Status::Ok();
}

Status Snapshotter::copy(cooc_ctx &ctx, int64_t offset, int64_t n, uint8_t *out) {
  if (ctx.snap_bytes < 0) return Status{COOC_ERR_STATE, "no snapshot image: call cooc_snapshot_prepare first"};
  if (offset < 0 || n < 0 || offset > ctx.snap_bytes || n > ctx.snap_bytes - offset)
    return Status{COOC_ERR_ARG, "bytes [" + std::to_string(offset) + ", +" + std::to_string(n) + ") outside the " +
                                    std::to_string(ctx.snap_bytes) + " B snapshot image"};
  if (n == 0) return Status::Ok();
  if (!out) return Status{COOC_ERR_ARG, "out is NULL"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  COOC_HIP_TRY(hipMemcpy(out, ctx.snap_img.as<char>() + offset, size_t(n), hipMemcpyDeviceToHost));
  return Status::Ok();
}

}  // namespace cooc
