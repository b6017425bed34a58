// cooc_snapshot.hip — checkpoint and restore of the streaming state (cooc_snapshot_prepare .. cooc_restore_finish).
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
//            k_snap_copy_lists   history arena -> histories back to back (long lists in 2,048-id pieces)
//   restore  k_snap_val_*        the device validation pass over the untrusted contents, in two phases: a kernel
//                                indexes with an offset from the blob only after the offsets have passed
//            k_snap_scatter_*    packed rows -> the dense matrix or the row slabs; k_snap_copy_lists the other way
//   both     k_snap_checksum     per section, the sum over its 8-B words w_i of splitmix64(w_i ^ i)
//
// All of it is bandwidth-bound and runs on the context's stream.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "cooc_ctx.h"
#include "cooc_radix.h"
#include "cooc_snapshot.h"
#include "cooc_stream_kernels.h"

namespace cooc {
namespace {

inline unsigned blocks_for(int64_t n, int t) { return unsigned(std::max<int64_t>(1, (n + t - 1) / t)); }
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// ---- checksum -------------------------------------------------------------------------------------------------
struct SnapSpans {
  int64_t off[kSnapSections];    // in 8-B words from the image's start
  int64_t words[kSnapSections];
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

// sums[k] (device, kSnapSections words) = the checksum of section k of the image
Status launch_checksums(hipStream_t s, const void *img, const SnapHeader &h, unsigned long long *sums) {
  SnapSpans S;
  int64_t most = 1;
  for (int k = 0; k < kSnapSections; k++) {
    S.off[k] = h.sec[k].offset / 8;
    S.words[k] = snap_pad8(h.sec[k].bytes) / 8;
    most = std::max(most, S.words[k]);
  }
  COOC_HIP_TRY(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * kSnapSections, s));
  const dim3 grid(std::min<unsigned>(blocks_for(most, 256 * 8), 2048), kSnapSections);
  k_snap_checksum<<<grid, 256, 0, s>>>(static_cast<const uint64_t *>(img), S, sums);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

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
constexpr int64_t kListChunk = 2048;
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

// ---- validation of an untrusted blob's contents ---------------------------------------------------------------
// Every kernel ORs `bit` into *err when an element fails, one atomic per workgroup.  Phase A reads its arrays
// by position only; phase B (k_snap_val_rows) indexes with the row offsets and runs after they have passed.
__device__ inline void val_fold(bool bad, unsigned int *err, unsigned int bit) {
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0 && any) atomicOr(err, bit);
}

// ids strictly ascending; with range: inside [0, hi)
__global__ __launch_bounds__(256) void k_snap_val_ids(const int32_t *__restrict__ ids, int64_t n, bool range, int64_t hi,
                                                      unsigned int *err, unsigned int bit) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const int32_t v = ids[i];
    bad = (range && (v < 0 || int64_t(v) >= hi)) || (i > 0 && ids[i - 1] >= v);
  }
  val_fold(bad, err, bit);
}

// ptr[0, n]: starts at 0, strictly ascending (no empty list), ends at `end`
__global__ __launch_bounds__(256) void k_snap_val_ptr(const int64_t *__restrict__ ptr, int64_t n, int64_t end,
                                                      unsigned int *err, unsigned int bit) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (i <= n) {
    const int64_t v = ptr[i];
    bad = (i == 0 && v != 0) || (i == n && v != end) || (i < n && v >= ptr[i + 1]);
  }
  val_fold(bad, err, bit);
}

// v[i] inside [lo, hi)
__global__ __launch_bounds__(256) void k_snap_val_range(const uint32_t *__restrict__ v, int64_t n, uint32_t lo, uint64_t hi,
                                                        unsigned int *err, unsigned int bit) {
  bool bad = false;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    bad |= v[i] < lo || uint64_t(v[i]) >= hi;
  val_fold(bad, err, bit);
}

// one wave per row: columns strictly ascending, counts summing to the row sum
__global__ __launch_bounds__(256) void k_snap_val_rows(int64_t R, const int64_t *__restrict__ rp,
                                                       const int32_t *__restrict__ col, const uint32_t *__restrict__ cnt,
                                                       const int64_t *__restrict__ sums, unsigned int *err, unsigned int bit) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  bool bad = false;
  for (int64_t r = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; r < R; r += n_waves) {
    const int64_t b = rp[r], e = rp[r + 1];
    unsigned long long sum = 0;
    for (int64_t i = b + lane; i < e; i += 64) {
      if (i > b && col[i - 1] >= col[i]) bad = true;
      sum += cnt[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (int64_t(sum) != sums[r]) bad = true;
  }
  val_fold(bad, err, bit);
}

// ---- install --------------------------------------------------------------------------------------------------
// packed row r (item ids[r]): its row sum and, for the row slabs, its length
__global__ void k_snap_scatter_meta(int64_t R, const int32_t *__restrict__ ids, const int64_t *__restrict__ rp,
                                    const int64_t *__restrict__ sums, int64_t *__restrict__ grs, int32_t *__restrict__ len) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int32_t a = ids[r];
  grs[a] = sums[r];
  if (len) len[a] = int32_t(rp[r + 1] - rp[r]);
}

__global__ void k_snap_scatter_i64(int64_t n, const int32_t *__restrict__ ids, const int64_t *__restrict__ vals,
                                   int64_t *__restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[ids[i]] = vals[i];
}

// one wave per packed row into the (zeroed) dense matrix
__global__ __launch_bounds__(256) void k_snap_scatter_dense(int64_t R, int32_t M, const int32_t *__restrict__ ids,
                                                            const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                            const uint32_t *__restrict__ cnt, uint32_t *__restrict__ G) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t r = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; r < R; r += n_waves) {
    uint32_t *g = G + int64_t(ids[r]) * M;
    const int64_t e = rp[r + 1];
    for (int64_t i = rp[r] + lane; i < e; i += 64) g[col[i]] = cnt[i];
  }
}

inline unsigned wave_grid(int64_t n_waves) { return std::min<unsigned>(blocks_for(n_waves * 64, 256), 8192); }

// chunk_pre[j] = pieces of the lists before j (host), from the lists' offsets
std::vector<int64_t> chunk_prefix(const std::vector<int64_t> &ptr) {
  std::vector<int64_t> pre(ptr.size(), 0);
  for (size_t j = 0; j + 1 < ptr.size(); j++) pre[j + 1] = pre[j] + (ptr[j + 1] - ptr[j] + kListChunk - 1) / kListChunk;
  return pre;
}

}  // namespace

// The one place that reads and writes the private state of StreamState and Operator for a checkpoint.
struct Snapshotter {
  static Status prepare(cooc_ctx &ctx, cooc_snapshot_info *info);
  static Status copy(cooc_ctx &ctx, int64_t offset, int64_t n, uint8_t *out);
  static Status restore_begin(cooc_ctx &ctx, int64_t bytes);
  static Status restore_write(cooc_ctx &ctx, int64_t offset, int64_t n, const uint8_t *src);
  static Status restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info);

 private:
  static bool empty_state(const cooc_ctx &ctx);
  static void wipe(cooc_ctx &ctx);
  static Status validate_and_install(cooc_ctx &ctx, cooc_snapshot_info *info);
  static Status install(cooc_ctx &ctx, const SnapHeader &h, const std::vector<int64_t> &scalars,
                        const std::vector<int32_t> &user_ids, const std::vector<int64_t> &hist_ptr,
                        const std::vector<int64_t> &pend_ts, const std::vector<int64_t> &pend_ptr,
                        const std::vector<int32_t> &pend_users, const std::vector<int32_t> &pend_items);
};

Status Snapshotter::prepare(cooc_ctx &ctx, cooc_snapshot_info *info) {
  StreamState &st = ctx.stream_state;
  Operator &op = ctx.op;
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  if (st.staged_)
    return Status{COOC_ERR_STATE, "window " + std::to_string(st.staged_ts_) + " is staged; finish it before a snapshot"};
  ctx.snapshot_release();
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  const bool multi = ctx.comm && ctx.comm->world() > 1;

  // ---- host tables: the users in ascending id order, the operator's buffered windows in timestamp order
  std::vector<std::pair<int32_t, int32_t>> users;  // (user id, slot) of every non-empty history
  for (size_t u = 0; u < st.dense_slot_.size(); u++)
    if (st.dense_slot_[u] >= 0 && st.h_len_[st.dense_slot_[u]] > 0) users.emplace_back(int32_t(u), st.dense_slot_[u]);
  for (const auto &kv : st.slot_of_)
    if (st.h_len_[kv.second] > 0) users.emplace_back(kv.first, kv.second);
  std::sort(users.begin(), users.end());
  const int64_t n_users = int64_t(users.size());
  std::vector<int32_t> user_ids(n_users);
  std::vector<int64_t> hist_ptr(n_users + 1, 0), aoff(n_users);
  for (int64_t j = 0; j < n_users; j++) {
    user_ids[j] = users[j].first;
    aoff[j] = st.h_off_[users[j].second];
    hist_ptr[j + 1] = hist_ptr[j] + st.h_len_[users[j].second];
  }
  std::vector<int64_t> pend_ts, pend_ptr(1, 0);
  std::vector<int32_t> pend_users, pend_items;
  for (const auto &kv : op.pending_) {  // (std::map: ascending maxTimestamp)
    pend_ts.push_back(kv.first);
    pend_users.insert(pend_users.end(), kv.second.users.begin(), kv.second.users.end());
    pend_items.insert(pend_items.end(), kv.second.items.begin(), kv.second.items.end());
    pend_ptr.push_back(int64_t(pend_users.size()));
  }

  // ---- the global rows packed: the prefix rp over all M rows, the non-empty rows' ids, the other ranks' row sums
  int64_t nnz = 0;
  int32_t n_sel[2] = {0, 0};
  const size_t o_flag = al256(sizeof(int32_t) * size_t(M)), o_xflag = o_flag + al256(size_t(M));
  const size_t o_ids = o_xflag + al256(size_t(M)), o_xids = o_ids + al256(sizeof(int32_t) * size_t(M));
  const size_t o_nsel = o_xids + al256(sizeof(int32_t) * size_t(M)), o_sel = o_nsel + 256;
  char *tmp = nullptr;
  const int64_t *rp = nullptr;
  if (st.global_ready_) {
    COOC_TRY(ctx.snap_tmp.reserve(o_sel + select_tmp_bytes(M)));
    tmp = ctx.snap_tmp.as<char>();
    const int32_t *lens = nullptr;
    if (st.sparse_global_) {  // (synchronises s)
      COOC_TRY(launch_pack_rows(s, M, st.gs_.base.as<int64_t>(), st.gs_.len.as<int32_t>(), st.gs_.col.as<int32_t>(),
                                st.gs_.cnt.as<uint32_t>(), ctx.snap_rp, ctx.snap_col, ctx.snap_cnt, st.d_scan_tmp_, &nnz));
      lens = st.gs_.len.as<int32_t>();
    } else {
      COOC_TRY(ctx.snap_rp.reserve(sizeof(int64_t) * (size_t(M) + 1)));
      COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(M)));
      int32_t *counted = reinterpret_cast<int32_t *>(tmp);
      k_snap_dense_rows<false><<<wave_grid(M), 256, 0, s>>>(M, st.d_global_.as<uint32_t>(), nullptr, counted, nullptr,
                                                             nullptr);
      COOC_HIP_TRY(hipGetLastError());
      int64_t *d_rp = ctx.snap_rp.as<int64_t>();
      COOC_HIP_TRY(hipMemsetAsync(d_rp, 0, sizeof(int64_t), s));
      int64_t serr = 0;
      COOC_TRY(launch_scan_ws<true>(ScanI32{counted}, d_rp + 1, M, st.d_scan_tmp_.as<unsigned long long>(), &serr, s));
      COOC_HIP_TRY(hipMemcpyAsync(&nnz, d_rp + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (serr & 8) return Status{COOC_ERR_STATE, "internal bounds check failed (snapshot row prefix)"};
      lens = counted;
    }
    rp = ctx.snap_rp.as<int64_t>();
    uint8_t *flag = reinterpret_cast<uint8_t *>(tmp + o_flag), *xflag = reinterpret_cast<uint8_t *>(tmp + o_xflag);
    int32_t *d_nsel = reinterpret_cast<int32_t *>(tmp + o_nsel);
    k_snap_flags<<<blocks_for(M, 256), 256, 0, s>>>(M, lens, st.d_grs_.as<int64_t>(), flag, xflag);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemsetAsync(d_nsel, 0, sizeof(int32_t) * 2, s));
    COOC_TRY(select_flagged(flag, M, reinterpret_cast<int32_t *>(tmp + o_ids), d_nsel, tmp + o_sel, s));
    if (multi) COOC_TRY(select_flagged(xflag, M, reinterpret_cast<int32_t *>(tmp + o_xids), d_nsel + 1, tmp + o_sel, s));
    COOC_HIP_TRY(hipMemcpyAsync(n_sel, d_nsel, sizeof(n_sel), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }
  const int64_t R = n_sel[0], X = n_sel[1];

  // ---- the image's layout
  SnapHeader h;
  std::memset(&h, 0, sizeof(h));
  auto sec = [&](int kind) -> SnapSection & { return h.sec[kind - 1]; };
  sec(kSnapScalars).count = kSnapScalarWords;
  sec(kSnapUserIds).count = n_users;
  sec(kSnapHistPtr).count = n_users + 1;
  sec(kSnapHistItems).count = hist_ptr[n_users];
  sec(kSnapRowIds).count = R;
  sec(kSnapRowPtr).count = R + 1;
  sec(kSnapRowCols).count = sec(kSnapRowCnts).count = nnz;
  sec(kSnapRowSums).count = R;
  sec(kSnapXsumIds).count = sec(kSnapXsumVals).count = X;
  sec(kSnapPendTs).count = int64_t(pend_ts.size());
  sec(kSnapPendPtr).count = int64_t(pend_ptr.size());
  sec(kSnapPendUsers).count = sec(kSnapPendItems).count = int64_t(pend_users.size());
  snap_layout(&h);
  h.n_items = M;
  h.user_cut = ctx.cfg.user_cut;
  h.window_size_ms = ctx.cfg.window_size_ms;
  h.rank = ctx.comm ? ctx.comm->rank() : 0;
  h.world = ctx.comm ? ctx.comm->world() : 1;
  COOC_TRY(ctx.snap_img.reserve(size_t(h.total_bytes)));
  char *img = ctx.snap_img.as<char>();
  auto at = [&](int kind) { return img + sec(kind).offset; };
  for (int k = 1; k <= kSnapSections; k++)  // the pad of a section of an odd number of 4-B elements
    if (sec(k).bytes & 7) COOC_HIP_TRY(hipMemsetAsync(at(k) + snap_pad8(sec(k).bytes) - 8, 0, 8, s));
  auto put = [&](int kind, const void *src) -> Status {
    if (sec(kind).bytes > 0)
      COOC_HIP_TRY(hipMemcpyAsync(at(kind), src, size_t(sec(kind).bytes), hipMemcpyHostToDevice, s));
    return Status::Ok();
  };

  // ---- host-side sections
  int64_t scal[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (st.global_ready_) COOC_HIP_TRY(hipMemcpyAsync(scal, st.d_scal_.p, sizeof(scal), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  int64_t scalars[kSnapScalarWords] = {0};
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
  COOC_TRY(put(kSnapScalars, scalars));
  COOC_TRY(put(kSnapUserIds, user_ids.data()));
  COOC_TRY(put(kSnapHistPtr, hist_ptr.data()));
  COOC_TRY(put(kSnapPendTs, pend_ts.data()));
  COOC_TRY(put(kSnapPendPtr, pend_ptr.data()));
  COOC_TRY(put(kSnapPendUsers, pend_users.data()));
  COOC_TRY(put(kSnapPendItems, pend_items.data()));

  // ---- histories: arena -> back to back
  const std::vector<int64_t> chunk_pre = chunk_prefix(hist_ptr);
  if (n_users > 0) {
    const size_t o_aoff = al256(sizeof(int64_t) * size_t(n_users + 1));
    COOC_TRY(ctx.snap_tmp2.reserve(o_aoff + sizeof(int64_t) * size_t(n_users)));
    int64_t *d_pre = ctx.snap_tmp2.as<int64_t>();
    int64_t *d_aoff = reinterpret_cast<int64_t *>(ctx.snap_tmp2.as<char>() + o_aoff);
    COOC_HIP_TRY(hipMemcpyAsync(d_pre, chunk_pre.data(), sizeof(int64_t) * size_t(n_users + 1), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(d_aoff, aoff.data(), sizeof(int64_t) * size_t(n_users), hipMemcpyHostToDevice, s));
    k_snap_copy_lists<true><<<wave_grid(chunk_pre[n_users]), 256, 0, s>>>(
        n_users, chunk_pre[n_users], d_pre, reinterpret_cast<const int64_t *>(at(kSnapHistPtr)), d_aoff,
        st.arena_.as<int32_t>(), reinterpret_cast<int32_t *>(at(kSnapHistItems)));
    COOC_HIP_TRY(hipGetLastError());
  }

  // ---- global rows
  if (st.global_ready_) {
    const int32_t *ids = reinterpret_cast<const int32_t *>(tmp + o_ids), *xids = reinterpret_cast<const int32_t *>(tmp + o_xids);
    const int64_t *grs = st.d_grs_.as<int64_t>();
    if (R > 0) COOC_HIP_TRY(hipMemcpyAsync(at(kSnapRowIds), ids, sizeof(int32_t) * size_t(R), hipMemcpyDeviceToDevice, s));
    k_snap_gather_rows<<<blocks_for(R + 1, 256), 256, 0, s>>>(R, M, ids, rp, grs, reinterpret_cast<int64_t *>(at(kSnapRowPtr)),
                                                             reinterpret_cast<int64_t *>(at(kSnapRowSums)));
    COOC_HIP_TRY(hipGetLastError());
    if (nnz > 0) {
      if (st.sparse_global_) {
        COOC_HIP_TRY(hipMemcpyAsync(at(kSnapRowCols), ctx.snap_col.p, sizeof(int32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
        COOC_HIP_TRY(hipMemcpyAsync(at(kSnapRowCnts), ctx.snap_cnt.p, sizeof(uint32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
      } else {
        k_snap_dense_rows<true><<<wave_grid(M), 256, 0, s>>>(M, st.d_global_.as<uint32_t>(), rp, nullptr,
                                                              reinterpret_cast<int32_t *>(at(kSnapRowCols)),
                                                              reinterpret_cast<uint32_t *>(at(kSnapRowCnts)));
        COOC_HIP_TRY(hipGetLastError());
      }
    }
    if (X > 0) {
      COOC_HIP_TRY(hipMemcpyAsync(at(kSnapXsumIds), xids, sizeof(int32_t) * size_t(X), hipMemcpyDeviceToDevice, s));
      k_snap_gather_i64<<<blocks_for(X, 256), 256, 0, s>>>(X, xids, grs, reinterpret_cast<int64_t *>(at(kSnapXsumVals)));
      COOC_HIP_TRY(hipGetLastError());
    }
  } else {
    COOC_HIP_TRY(hipMemsetAsync(at(kSnapRowPtr), 0, sizeof(int64_t), s));
  }

  // ---- checksums, then the header
  COOC_TRY(ctx.snap_sums.reserve(sizeof(unsigned long long) * kSnapSections + sizeof(unsigned int) * 2));
  COOC_TRY(launch_checksums(s, img, h, ctx.snap_sums.as<unsigned long long>()));
  unsigned long long sums[kSnapSections];
  COOC_HIP_TRY(hipMemcpyAsync(sums, ctx.snap_sums.p, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < kSnapSections; k++) h.sec[k].sum = sums[k];
  snap_seal(&h);
  COOC_HIP_TRY(hipMemcpyAsync(img, &h, sizeof(h), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  // (the packed slab rows were only a stage on the way into the image)
  ctx.snap_col.release();
  ctx.snap_cnt.release();
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

bool Snapshotter::empty_state(const cooc_ctx &ctx) {
  const StreamState &st = ctx.stream_state;
  const Operator &op = ctx.op;
  return !st.staged_ && st.window_seq_ == 0 && st.h_off_.empty() && !st.global_ready_ && op.pending_.empty() &&
         op.watermark == INT64_MIN && op.late_elements == 0;
}

Status Snapshotter::restore_begin(cooc_ctx &ctx, int64_t bytes) {
  if (!empty_state(ctx))
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  if (bytes < kSnapHeaderBytes) return Status{COOC_ERR_ARG, "snapshot blob: shorter than its header"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  ctx.snapshot_release();
  ctx.restore_bytes = -1;
  COOC_TRY(ctx.restore_img.reserve(size_t(bytes)));
  COOC_HIP_TRY(hipMemsetAsync(ctx.restore_img.p, 0, size_t(bytes), ctx.stream));  // (ranges never written read as 0)
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  ctx.restore_bytes = bytes;
  return Status::Ok();
}

Status Snapshotter::restore_write(cooc_ctx &ctx, int64_t offset, int64_t n, const uint8_t *src) {
  if (ctx.restore_bytes < 0) return Status{COOC_ERR_STATE, "no restore in progress: call cooc_restore_begin first"};
  if (offset < 0 || n < 0 || offset > ctx.restore_bytes || n > ctx.restore_bytes - offset)
    return Status{COOC_ERR_ARG, "bytes [" + std::to_string(offset) + ", +" + std::to_string(n) + ") outside the " +
                                    std::to_string(ctx.restore_bytes) + " B announced"};
  if (n == 0) return Status::Ok();
  if (!src) return Status{COOC_ERR_ARG, "src is NULL"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  COOC_HIP_TRY(hipMemcpy(ctx.restore_img.as<char>() + offset, src, size_t(n), hipMemcpyHostToDevice));
  return Status::Ok();
}

// Back to a context without streaming state (a refused or failed restore leaves nothing behind).
void Snapshotter::wipe(cooc_ctx &ctx) {
  StreamState &st = ctx.stream_state;
  Operator &op = ctx.op;
  (void)hipStreamSynchronize(ctx.stream);
  st.release();
  st.slot_of_.clear();
  st.dense_slot_.clear();
  st.h_off_.clear();
  st.h_len_.clear();
  st.h_cap_.clear();
  st.staged_stamp_.clear();
  st.staged_pos_.clear();
  st.arena_used_ = 0;
  st.observed_exact = st.observed_ref = st.rowsum_acc = st.rescored_items = 0;
  st.have_window_ = st.delta_packed_ = false;
  op.pending_.clear();
  op.watermark = op.agreed_ = INT64_MIN;
  op.late_elements = 0;
  op.regather_ = false;
}

Status Snapshotter::restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info) {
  if (ctx.restore_bytes < 0) return Status{COOC_ERR_STATE, "no restore in progress: call cooc_restore_begin first"};
  if (!empty_state(ctx)) {
    ctx.restore_img.release();
    ctx.restore_bytes = -1;
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  }
  Status r = hipSetDevice(ctx.device) == hipSuccess ? validate_and_install(ctx, info) : Status{COOC_ERR_HIP, "hipSetDevice"};
  if (!r.ok()) wipe(ctx);
  (void)hipStreamSynchronize(ctx.stream);
  ctx.restore_img.release();
  ctx.restore_bytes = -1;
  return r;
}

Status Snapshotter::validate_and_install(cooc_ctx &ctx, cooc_snapshot_info *info) {
  hipStream_t s = ctx.stream;
  const char *img = ctx.restore_img.as<char>();
  // 1. header and directory (the host-only code of cooc_snapshot_inspect)
  uint8_t hdr[kSnapHeaderBytes];
  COOC_HIP_TRY(hipMemcpy(hdr, img, sizeof(hdr), hipMemcpyDeviceToHost));
  SnapHeader h;
  std::string why;
  if (snap_parse(hdr, ctx.restore_bytes, &h, &why) != COOC_OK) return Status{COOC_ERR_ARG, why};
  const int32_t M = ctx.cfg.n_items;
  if (h.n_items != M || h.window_size_ms != ctx.cfg.window_size_ms || h.user_cut != ctx.cfg.user_cut)
    return Status{COOC_ERR_ARG, "snapshot blob: taken with n_items " + std::to_string(h.n_items) + ", window " +
                                    std::to_string(h.window_size_ms) + " ms, user_cut " + std::to_string(h.user_cut) +
                                    "; this context has " + std::to_string(M) + ", " +
                                    std::to_string(ctx.cfg.window_size_ms) + " ms, " + std::to_string(ctx.cfg.user_cut)};
  const int32_t rank = ctx.comm ? ctx.comm->rank() : 0, world = ctx.comm ? ctx.comm->world() : 1;
  if (h.rank != rank || h.world != world)
    return Status{COOC_ERR_ARG, "snapshot blob: taken by rank " + std::to_string(h.rank) + " of " + std::to_string(h.world) +
                                    "; this context is rank " + std::to_string(rank) + " of " + std::to_string(world)};
  auto sec = [&](int kind) -> const SnapSection & { return h.sec[kind - 1]; };
  auto at = [&](int kind) { return img + sec(kind).offset; };
  const int64_t n_users = sec(kSnapUserIds).count, n_hist = sec(kSnapHistItems).count, R = sec(kSnapRowIds).count;
  const int64_t nnz = sec(kSnapRowCols).count, X = sec(kSnapXsumIds).count, P = sec(kSnapPendTs).count;
  const int64_t n_pend = sec(kSnapPendUsers).count;
  if (world == 1 && X > 0) return Status{COOC_ERR_ARG, "snapshot blob: row sums of other ranks without a communicator"};

  // 2. the sections' checksums
  COOC_TRY(ctx.snap_sums.reserve(sizeof(unsigned long long) * kSnapSections + sizeof(unsigned int) * 2));
  unsigned long long *d_sums = ctx.snap_sums.as<unsigned long long>();
  unsigned int *d_err = reinterpret_cast<unsigned int *>(d_sums + kSnapSections);
  COOC_TRY(launch_checksums(s, img, h, d_sums));
  unsigned long long sums[kSnapSections];
  COOC_HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < kSnapSections; k++)
    if (sums[k] != h.sec[k].sum)
      return Status{COOC_ERR_ARG, "snapshot blob: checksum mismatch in section " + std::to_string(k + 1)};

  // 3. the contents.  Phase A: every array by position (ids, offsets, ranges); phase B: the rows through their
  //    offsets, once those have passed.
  const int32_t *d_uids = reinterpret_cast<const int32_t *>(at(kSnapUserIds));
  const int64_t *d_hptr = reinterpret_cast<const int64_t *>(at(kSnapHistPtr));
  const int32_t *d_hist = reinterpret_cast<const int32_t *>(at(kSnapHistItems));
  const int32_t *d_rids = reinterpret_cast<const int32_t *>(at(kSnapRowIds));
  const int64_t *d_rptr = reinterpret_cast<const int64_t *>(at(kSnapRowPtr));
  const int32_t *d_col = reinterpret_cast<const int32_t *>(at(kSnapRowCols));
  const uint32_t *d_cnt = reinterpret_cast<const uint32_t *>(at(kSnapRowCnts));
  const int64_t *d_rsum = reinterpret_cast<const int64_t *>(at(kSnapRowSums));
  const int32_t *d_xids = reinterpret_cast<const int32_t *>(at(kSnapXsumIds));
  auto range_grid = [](int64_t n) { return std::min<unsigned>(blocks_for(n, 256 * 4), 4096); };
  COOC_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned int) * 2, s));
  k_snap_val_ids<<<blocks_for(n_users, 256), 256, 0, s>>>(d_uids, n_users, false, 0, d_err, 1u);
  k_snap_val_ptr<<<blocks_for(n_users + 1, 256), 256, 0, s>>>(d_hptr, n_users, n_hist, d_err, 2u);
  k_snap_val_range<<<range_grid(n_hist), 256, 0, s>>>(reinterpret_cast<const uint32_t *>(d_hist), n_hist, 0u, uint64_t(M),
                                                      d_err, 4u);
  k_snap_val_ids<<<blocks_for(R, 256), 256, 0, s>>>(d_rids, R, true, M, d_err, 8u);
  k_snap_val_ptr<<<blocks_for(R + 1, 256), 256, 0, s>>>(d_rptr, R, nnz, d_err, 16u);
  k_snap_val_range<<<range_grid(nnz), 256, 0, s>>>(reinterpret_cast<const uint32_t *>(d_col), nnz, 0u, uint64_t(M), d_err, 32u);
  k_snap_val_range<<<range_grid(nnz), 256, 0, s>>>(d_cnt, nnz, 1u, uint64_t(1) << 32, d_err, 64u);  // counts non-zero
  k_snap_val_ids<<<blocks_for(X, 256), 256, 0, s>>>(d_xids, X, true, M, d_err, 128u);
  COOC_HIP_TRY(hipGetLastError());
  unsigned int err[2] = {0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err[0])
    return Status{COOC_ERR_ARG, "snapshot blob: invalid contents (checks failed: " + std::to_string(err[0]) +
                                    "; 1 user ids, 2 history offsets, 4 history items, 8 row ids, 16 row offsets, "
                                    "32 columns, 64 counts, 128 row-sum ids)"};
  k_snap_val_rows<<<wave_grid(R), 256, 0, s>>>(R, d_rptr, d_col, d_cnt, d_rsum, d_err + 1, 1u);
  COOC_HIP_TRY(hipGetLastError());
  // the sections that become host state
  std::vector<int64_t> scalars(kSnapScalarWords), hist_ptr(n_users + 1), pend_ts(P), pend_ptr(P + 1);
  std::vector<int32_t> user_ids(n_users), pend_users(n_pend), pend_items(n_pend);
  auto get = [&](int kind, void *dst) -> Status {
    if (sec(kind).bytes > 0)
      COOC_HIP_TRY(hipMemcpyAsync(dst, at(kind), size_t(sec(kind).bytes), hipMemcpyDeviceToHost, s));
    return Status::Ok();
  };
  COOC_TRY(get(kSnapScalars, scalars.data()));
  COOC_TRY(get(kSnapUserIds, user_ids.data()));
  COOC_TRY(get(kSnapHistPtr, hist_ptr.data()));
  COOC_TRY(get(kSnapPendTs, pend_ts.data()));
  COOC_TRY(get(kSnapPendPtr, pend_ptr.data()));
  COOC_TRY(get(kSnapPendUsers, pend_users.data()));
  COOC_TRY(get(kSnapPendItems, pend_items.data()));
  COOC_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err[1])
    return Status{COOC_ERR_ARG, "snapshot blob: a global row's columns are not strictly ascending or its counts do "
                                "not sum to its row sum"};
  for (int64_t j = 0; j < n_users; j++)
    if (hist_ptr[j + 1] - hist_ptr[j] > int64_t(INT32_MAX))
      return Status{COOC_ERR_ARG, "snapshot blob: a user history longer than 2^31"};
  if (pend_ptr[0] != 0 || pend_ptr[P] != n_pend) return Status{COOC_ERR_ARG, "snapshot blob: bad pending offsets"};
  for (int64_t k = 0; k < P; k++)
    if (pend_ptr[k] >= pend_ptr[k + 1] || (k > 0 && pend_ts[k - 1] >= pend_ts[k]))
      return Status{COOC_ERR_ARG, "snapshot blob: pending windows out of order or empty"};
  for (int32_t it : pend_items)
    if (it < 0 || it >= M) return Status{COOC_ERR_ARG, "snapshot blob: a pending item outside [0, n_items)"};
  if (scalars[kScRegather] != 0 && scalars[kScRegather] != 1) return Status{COOC_ERR_ARG, "snapshot blob: bad scalar"};
  if (scalars[kScLateElements] < 0 || scalars[kScRescoredItems] < 0 || scalars[kScWatermark] < scalars[kScAgreed])
    return Status{COOC_ERR_ARG, "snapshot blob: bad scalar"};
  for (int k = kScScal3 + 1; k < kSnapScalarWords; k++)
    if (scalars[k] != 0) return Status{COOC_ERR_ARG, "snapshot blob: reserved scalar set"};

  // 4. everything passed
  COOC_TRY(install(ctx, h, scalars, user_ids, hist_ptr, pend_ts, pend_ptr, pend_users, pend_items));
  snap_info(h, info);
  return Status::Ok();
}

Status Snapshotter::install(cooc_ctx &ctx, const SnapHeader &h, const std::vector<int64_t> &scalars,
                            const std::vector<int32_t> &user_ids, const std::vector<int64_t> &hist_ptr,
                            const std::vector<int64_t> &pend_ts, const std::vector<int64_t> &pend_ptr,
                            const std::vector<int32_t> &pend_users, const std::vector<int32_t> &pend_items) {
  StreamState &st = ctx.stream_state;
  Operator &op = ctx.op;
  hipStream_t s = ctx.stream;
  const char *img = ctx.restore_img.as<char>();
  const int32_t M = ctx.cfg.n_items;
  auto sec = [&](int kind) -> const SnapSection & { return h.sec[kind - 1]; };
  auto at = [&](int kind) { return img + sec(kind).offset; };
  const int64_t n_users = sec(kSnapUserIds).count, R = sec(kSnapRowIds).count, nnz = sec(kSnapRowCols).count;
  const int64_t X = sec(kSnapXsumIds).count;

  // ---- global rows, row sums, running totals: in this context's representation (ensure_global chooses it)
  const bool any_global = R > 0 || X > 0 || scalars[kScScal2] != 0 || scalars[kScScal3] != 0;
  if (any_global) {
    COOC_TRY(st.ensure_global(ctx));  // (zeroed: the matrix or the slabs' base / len, the row sums, the totals)
    const int32_t *ids = reinterpret_cast<const int32_t *>(at(kSnapRowIds));
    const int64_t *rp = reinterpret_cast<const int64_t *>(at(kSnapRowPtr));
    const int32_t *col = reinterpret_cast<const int32_t *>(at(kSnapRowCols));
    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(at(kSnapRowCnts));
    int64_t *grs = st.d_grs_.as<int64_t>();
    if (R > 0) {
      k_snap_scatter_meta<<<blocks_for(R, 256), 256, 0, s>>>(R, ids, rp, reinterpret_cast<const int64_t *>(at(kSnapRowSums)),
                                                              grs, st.sparse_global_ ? st.gs_.len.as<int32_t>() : nullptr);
      COOC_HIP_TRY(hipGetLastError());
    }
    if (X > 0) {
      k_snap_scatter_i64<<<blocks_for(X, 256), 256, 0, s>>>(X, reinterpret_cast<const int32_t *>(at(kSnapXsumIds)),
                                                            reinterpret_cast<const int64_t *>(at(kSnapXsumVals)), grs);
      COOC_HIP_TRY(hipGetLastError());
    }
    if (st.sparse_global_) {
      // the slabs as compact_global leaves them: the rows back to back in row order (base = the prefix of len),
      // bump = live = the entries, and the growth slack launch_gs_merge's first window would otherwise compact for
      GlobalSparse &g = st.gs_;
      const int64_t cap = std::max<int64_t>(2 * nnz, int64_t(1) << 12);
      COOC_TRY(g.col.reserve(sizeof(int32_t) * size_t(cap)));
      COOC_TRY(g.cnt.reserve(sizeof(uint32_t) * size_t(cap)));
      COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(M)));
      int64_t serr = 0;
      COOC_TRY(launch_scan_ws<false>(ScanI32{g.len.as<int32_t>()}, g.base.as<int64_t>(), M,
                                     st.d_scan_tmp_.as<unsigned long long>(), &serr, s));
      if (nnz > 0) {
        COOC_HIP_TRY(hipMemcpyAsync(g.col.p, col, sizeof(int32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
        COOC_HIP_TRY(hipMemcpyAsync(g.cnt.p, cnt, sizeof(uint32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
      }
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (serr & 8) return Status{COOC_ERR_STATE, "internal bounds check failed (restored slab prefix)"};
      g.cap = cap;
      g.bump = g.live = nnz;
      g.compactions = 0;
    } else if (R > 0) {
      k_snap_scatter_dense<<<wave_grid(R), 256, 0, s>>>(R, M, ids, rp, col, cnt, st.d_global_.as<uint32_t>());
      COOC_HIP_TRY(hipGetLastError());
    }
    int64_t scal[8] = {0, 0, scalars[kScScal2], scalars[kScScal3], 0, 0, 0, 0};
    COOC_HIP_TRY(hipMemcpyAsync(st.d_scal_.p, scal, sizeof(scal), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }

  // ---- histories: a fresh arena, every list at finish()'s own first capacity; the slot tables in user order
  if (n_users > 0) {
    std::vector<int64_t> aoff(n_users);
    int64_t used = 0;
    for (int64_t j = 0; j < n_users; j++) {
      aoff[j] = used;
      used += std::max<int64_t>(16, hist_ptr[j + 1] - hist_ptr[j]);
    }
    st.arena_used_ = used;
    COOC_TRY(st.grow_arena(ctx, std::max<int64_t>(used, 1024)));
    const std::vector<int64_t> chunk_pre = chunk_prefix(hist_ptr);
    const size_t o_aoff = al256(sizeof(int64_t) * size_t(n_users + 1));
    COOC_TRY(ctx.snap_tmp2.reserve(o_aoff + sizeof(int64_t) * size_t(n_users)));
    int64_t *d_pre = ctx.snap_tmp2.as<int64_t>();
    int64_t *d_aoff = reinterpret_cast<int64_t *>(ctx.snap_tmp2.as<char>() + o_aoff);
    COOC_HIP_TRY(hipMemcpyAsync(d_pre, chunk_pre.data(), sizeof(int64_t) * size_t(n_users + 1), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(d_aoff, aoff.data(), sizeof(int64_t) * size_t(n_users), hipMemcpyHostToDevice, s));
    k_snap_copy_lists<false><<<wave_grid(chunk_pre[n_users]), 256, 0, s>>>(
        n_users, chunk_pre[n_users], d_pre, reinterpret_cast<const int64_t *>(at(kSnapHistPtr)), d_aoff,
        reinterpret_cast<const int32_t *>(at(kSnapHistItems)), st.arena_.as<int32_t>());
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipStreamSynchronize(s));
    for (int64_t j = 0; j < n_users; j++) {
      const int32_t slot = st.slot_for(user_ids[j]);  // (dense_slot_ / slot_of_, staged_stamp_, staged_pos_)
      const int64_t len = hist_ptr[j + 1] - hist_ptr[j];
      st.h_off_[slot] = aoff[j];
      st.h_len_[slot] = int32_t(len);
      st.h_cap_[slot] = int32_t(std::max<int64_t>(16, len));
    }
  }

  // ---- accumulators and the operator
  st.observed_exact = scalars[kScObservedExact];
  st.observed_ref = scalars[kScObservedRef];
  st.rowsum_acc = scalars[kScRowsumAcc];
  st.rescored_items = scalars[kScRescoredItems];
  op.late_elements = scalars[kScLateElements];
  op.watermark = scalars[kScWatermark];
  op.agreed_ = scalars[kScAgreed];
  op.regather_ = scalars[kScRegather] != 0;
  for (size_t k = 0; k < pend_ts.size(); k++) {
    Operator::Pending &p = op.pending_[pend_ts[k]];
    p.users.assign(pend_users.begin() + pend_ptr[k], pend_users.begin() + pend_ptr[k + 1]);
    p.items.assign(pend_items.begin() + pend_ptr[k], pend_items.begin() + pend_ptr[k + 1]);
  }
  return Status::Ok();
}

// ---- the context's entry points (cooc_capi.cpp) ---------------------------------------------------------------
Status snapshot_prepare(cooc_ctx &ctx, cooc_snapshot_info *info) { return Snapshotter::prepare(ctx, info); }
Status snapshot_copy(cooc_ctx &ctx, int64_t offset, int64_t n, uint8_t *out) { return Snapshotter::copy(ctx, offset, n, out); }
Status restore_begin(cooc_ctx &ctx, int64_t bytes) { return Snapshotter::restore_begin(ctx, bytes); }
Status restore_write(cooc_ctx &ctx, int64_t offset, int64_t n, const uint8_t *src) {
  return Snapshotter::restore_write(ctx, offset, n, src);
}
Status restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info) { return Snapshotter::restore_finish(ctx, info); }

}  // namespace cooc

void cooc_ctx::snapshot_release() {
  if (snap_bytes < 0 && !snap_img.p) return;
  (void)hipSetDevice(device);
  snap_img.release();
  snap_rp.release();
  snap_col.release();
  snap_cnt.release();
  snap_bytes = -1;
}
