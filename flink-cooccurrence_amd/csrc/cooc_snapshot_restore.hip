// cooc_snapshot_restore.hip — restore of the streaming state from one snapshot blob (cooc_restore_begin .. _finish;
// the blob: cooc_snapshot.h; how it is made: cooc_snapshot_pack.hip).
//
//   restore  k_snap_val_*        the device validation pass over the untrusted contents, in two phases: a kernel
//                                indexes with an offset from the blob only after the offsets have passed
//            k_snap_scatter_*    packed rows -> the dense matrix or the row slabs; k_snap_copy_lists (of the pack
//                                file) the other way, k_snap_checksum against the blob's own sums
//   sampled  a sampled context's blob is format 2: the same code with five more sections
//            k_snap_val_i16 / k_snap_val_totals   counters in 1..item_cut; every history's user has a total at
//                                least its length, and the length is at most user_cut
//            k_snap_scatter_counts / _totals / _lens   the device sampler's arrays from the blob
//
// validate leaves a context untouched; install runs only on contents that have passed, and a failure on the way
// wipes the context back to empty.  The restore from all parts of a checkpoint (cooc_snapshot_rescale.hip)
// validates every part with the same validate and installs with the same pieces.  All of it is bandwidth-bound and
// runs on the context's stream.
#include <cstring>

#include "cooc_radix.h"
#include "cooc_snapshot_impl.h"

namespace cooc {
namespace {

// ---- validation of an untrusted blob's contents ---------------------------------------------------------------
// Every kernel ORs `bit` into *err when an element fails, one atomic per workgroup (val_fold).  Phase A reads its
// arrays by position only; phase B (k_snap_val_rows) indexes with the row offsets and runs after they have passed.

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

// validate.  v[i] inside [lo, hi]
__global__ __launch_bounds__(256) void k_snap_val_i16(const int16_t *__restrict__ v, int64_t n, int32_t lo, int32_t hi,
                                                      unsigned int *err, unsigned int bit) {
  bool bad = false;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    bad |= int32_t(v[i]) < lo || int32_t(v[i]) > hi;
  val_fold(bad, err, bit);
}

// where id sits in the ascending ids[0, n), or -1 (every read is at a position below n)
__device__ inline int64_t snap_find(const int32_t *__restrict__ ids, int64_t n, int32_t id) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo < n && ids[lo] == id ? lo : -1;
}

// Every user with a history (uids[j], its length from hptr) against the users with a total (tids ascending, tot):
// the user is among them, its total is at least its history's length, and that length is at most user_cut.
// Reads by position only (the offsets enter as numbers, not as indices).
__global__ __launch_bounds__(256) void k_snap_val_totals(const int32_t *__restrict__ uids, int64_t n,
                                                         const int64_t *__restrict__ hptr,
                                                         const int32_t *__restrict__ tids, int64_t n_tot,
                                                         const int32_t *__restrict__ tot, int32_t user_cut,
                                                         unsigned int *err, unsigned int bit) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (j < n) {
    const int64_t len = hptr[j + 1] - hptr[j];
    const int64_t at = snap_find(tids, n_tot, uids[j]);
    bad = at < 0 || len > int64_t(user_cut) || int64_t(tot[at < 0 ? 0 : at]) < len;
  }
  val_fold(bad, err, bit);
}

// install (validated contents).  The device sampler's state from the blob: count[ids[k]] = cnts[k];
// T[slots[j]] = tot[j] for the users with a total (slots: the host's slot of each, in their order); L[slot] = the
// history's length for the users that have one.
__global__ __launch_bounds__(256) void k_snap_scatter_counts(int64_t n, const int32_t *__restrict__ ids,
                                                             const int16_t *__restrict__ cnts, int32_t *__restrict__ count) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k < n) count[ids[k]] = int32_t(cnts[k]);
}
__global__ __launch_bounds__(256) void k_snap_scatter_totals(int64_t n, const int32_t *__restrict__ slots,
                                                             const int32_t *__restrict__ tot, int64_t slot_cap,
                                                             int32_t *__restrict__ T) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= n) return;
  const int32_t slot = slots[j];
  if (slot >= 0 && int64_t(slot) < slot_cap) T[slot] = tot[j];
}
__global__ __launch_bounds__(256) void k_snap_scatter_lens(int64_t n, const int32_t *__restrict__ uids,
                                                           const int64_t *__restrict__ hptr,
                                                           const int32_t *__restrict__ tids, int64_t n_tot,
                                                           const int32_t *__restrict__ slots, int64_t slot_cap,
                                                           int32_t *__restrict__ L) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t at = snap_find(tids, n_tot, uids[j]);
  if (at < 0) return;
  const int32_t slot = slots[at];
  if (slot >= 0 && int64_t(slot) < slot_cap) L[slot] = int32_t(hptr[j + 1] - hptr[j]);
}

unsigned range_grid(int64_t n) { return std::min<unsigned>(blocks_for(n, 256 * 4), 4096); }

// Phase A: every array by position (ids, offsets, ranges), one bit of err[0] per check.  Format 2: the sampler's
// sections first (item_cut bounds the counters).
void launch_phase_a(hipStream_t s, const BlobView &v, int32_t M, int32_t item_cut, unsigned int *d_err) {
  const int64_t n_users = v.count(kSnapUserIds), n_hist = v.count(kSnapHistItems), R = v.count(kSnapRowIds);
  const int64_t nnz = v.count(kSnapRowCols), X = v.count(kSnapXsumIds);
  if (v.h->format == kSnapFormatSampled) {
    const int64_t n_cnt = v.count(kSnapSmpItemIds), n_tot = v.count(kSnapSmpUserIds);
    k_snap_val_ids<<<blocks_for(n_cnt, 256), 256, 0, s>>>(v.at<int32_t>(kSnapSmpItemIds), n_cnt, true, M, d_err, 256u);
    k_snap_val_i16<<<range_grid(n_cnt), 256, 0, s>>>(v.at<int16_t>(kSnapSmpItemCnts), n_cnt, 1, item_cut, d_err, 512u);
    k_snap_val_ids<<<blocks_for(n_tot, 256), 256, 0, s>>>(v.at<int32_t>(kSnapSmpUserIds), n_tot, false, 0, d_err, 1024u);
    k_snap_val_range<<<range_grid(n_tot), 256, 0, s>>>(v.at<uint32_t>(kSnapSmpTotals), n_tot, 1u, uint64_t(1) << 31, d_err,
                                                       2048u);
  }
  k_snap_val_ids<<<blocks_for(n_users, 256), 256, 0, s>>>(v.at<int32_t>(kSnapUserIds), n_users, false, 0, d_err, 1u);
  k_snap_val_ptr<<<blocks_for(n_users + 1, 256), 256, 0, s>>>(v.at<int64_t>(kSnapHistPtr), n_users, n_hist, d_err, 2u);
  k_snap_val_range<<<range_grid(n_hist), 256, 0, s>>>(v.at<uint32_t>(kSnapHistItems), n_hist, 0u, uint64_t(M), d_err, 4u);
  k_snap_val_ids<<<blocks_for(R, 256), 256, 0, s>>>(v.at<int32_t>(kSnapRowIds), R, true, M, d_err, 8u);
  k_snap_val_ptr<<<blocks_for(R + 1, 256), 256, 0, s>>>(v.at<int64_t>(kSnapRowPtr), R, nnz, d_err, 16u);
  k_snap_val_range<<<range_grid(nnz), 256, 0, s>>>(v.at<uint32_t>(kSnapRowCols), nnz, 0u, uint64_t(M), d_err, 32u);
  k_snap_val_range<<<range_grid(nnz), 256, 0, s>>>(v.at<uint32_t>(kSnapRowCnts), nnz, 1u, uint64_t(1) << 32, d_err,
                                                   64u);  // counts non-zero
  k_snap_val_ids<<<blocks_for(X, 256), 256, 0, s>>>(v.at<int32_t>(kSnapXsumIds), X, true, M, d_err, 128u);
}

// Phase B, once the offsets have passed: the rows through theirs (bit 1 of *d_err); format 2: the histories'
// users against the users with a total (bit 2; both id lists have passed)
void launch_phase_b(hipStream_t s, const BlobView &v, int32_t user_cut, unsigned int *d_err) {
  const int64_t R = v.count(kSnapRowIds), n_users = v.count(kSnapUserIds);
  k_snap_val_rows<<<wave_grid(R), 256, 0, s>>>(R, v.at<int64_t>(kSnapRowPtr), v.at<int32_t>(kSnapRowCols),
                                               v.at<uint32_t>(kSnapRowCnts), v.at<int64_t>(kSnapRowSums), d_err, 1u);
  if (v.h->format == kSnapFormatSampled)
    k_snap_val_totals<<<blocks_for(n_users, 256), 256, 0, s>>>(v.at<int32_t>(kSnapUserIds), n_users, v.at<int64_t>(kSnapHistPtr),
                                                               v.at<int32_t>(kSnapSmpUserIds), v.count(kSnapSmpUserIds),
                                                               v.at<int32_t>(kSnapSmpTotals), user_cut, d_err, 2u);
}

// the checks of the sections that became host state
Status check_host_sections(const Snapshotter::Parsed &p, int32_t M) {
  const std::vector<int64_t> &scalars = p.scalars, &hist_ptr = p.hist_ptr;
  const PendingWindows &pend = p.pend;
  const int64_t P = int64_t(pend.ts.size()), n_pend = int64_t(pend.users.size());
  for (size_t j = 0; j + 1 < hist_ptr.size(); j++)
    if (hist_ptr[j + 1] - hist_ptr[j] > int64_t(INT32_MAX))
      return Status{COOC_ERR_ARG, "snapshot blob: a user history longer than 2^31"};
  if (pend.ptr[0] != 0 || pend.ptr[P] != n_pend) return Status{COOC_ERR_ARG, "snapshot blob: bad pending offsets"};
  for (int64_t k = 0; k < P; k++)
    if (pend.ptr[k] >= pend.ptr[k + 1] || (k > 0 && pend.ts[k - 1] >= pend.ts[k]))
      return Status{COOC_ERR_ARG, "snapshot blob: pending windows out of order or empty"};
  for (int32_t it : pend.items)
    if (it < 0 || it >= M) return Status{COOC_ERR_ARG, "snapshot blob: a pending item outside [0, n_items)"};
  if (scalars[kScRegather] != 0 && scalars[kScRegather] != 1) return Status{COOC_ERR_ARG, "snapshot blob: bad scalar"};
  if (scalars[kScLateElements] < 0 || scalars[kScRescoredItems] < 0 || scalars[kScWatermark] < scalars[kScAgreed])
    return Status{COOC_ERR_ARG, "snapshot blob: bad scalar"};
  for (int k = kScScal3 + 1; k < kSnapScalarWords; k++)
    if (scalars[k] != 0) return Status{COOC_ERR_ARG, "snapshot blob: reserved scalar set"};
  return Status::Ok();
}

}  // namespace

bool Snapshotter::empty_state(const cooc_ctx &ctx) {
  const StreamState &st = ctx.stream_state;
  const Operator &op = ctx.op;
  return !st.staged_ && st.window_seq_ == 0 && st.h_off_.empty() && !st.global_ready_ && op.pending_.empty() &&
         op.watermark == INT64_MIN && op.late_elements == 0;
}

Status Snapshotter::restore_begin(cooc_ctx &ctx, int64_t bytes) {
  if (!empty_state(ctx))
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  if (bytes < snap_header_bytes(snap_sections_of(format_of(ctx))))
    return Status{COOC_ERR_ARG, "snapshot blob: shorter than its header"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  ctx.snapshot_release();
  ctx.restore_bytes = -1;
  ctx.restore_part_off.clear();
  ctx.restore_part_len.clear();
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
  if (st.sampled()) (void)reset_samplers(ctx);
}

// A sampled context's samplers back to what cooc_sampling_enable* left (StreamState::release has freed the device
// sampler's arrays; its cuts and seed stay).
Status Snapshotter::reset_samplers(cooc_ctx &ctx) {
  StreamState &st = ctx.stream_state;
  st.sampler_.reset();
  st.sm_seq_ = 0;
  if (st.dev_sampler_.enabled())
    COOC_TRY(st.dev_sampler_.enable(ctx.cfg.n_items, st.sampler_.item_cut(), ctx.cfg.user_cut, st.sampler_.seed(), ctx.stream));
  return Status::Ok();
}

Status Snapshotter::restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info) {
  if (ctx.restore_bytes < 0) return Status{COOC_ERR_STATE, "no restore in progress: call cooc_restore_begin first"};
  if (!empty_state(ctx)) {
    drop_restore(ctx);
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  }
  Status r{COOC_ERR_HIP, "hipSetDevice"};
  if (hipSetDevice(ctx.device) == hipSuccess) {
    Parsed p;
    r = validate(ctx, ctx.restore_img.as<char>(), ctx.restore_bytes, true, &p);
    if (r.ok()) r = install(ctx, ctx.restore_img.as<char>(), p);  // everything passed
    if (r.ok()) snap_info(p.h, info);
  }
  if (!r.ok()) wipe(ctx);
  (void)hipStreamSynchronize(ctx.stream);
  drop_restore(ctx);
  return r;
}

void Snapshotter::drop_restore(cooc_ctx &ctx) {
  ctx.restore_img.release();
  ctx.restore_bytes = -1;
  ctx.restore_part_off.clear();
  ctx.restore_part_len.clear();
}

// ---- validate -------------------------------------------------------------------------------------------------
// The whole validation of one untrusted blob of `bytes` bytes at img (device); own_rank: it must also have been
// taken by this context's (rank, world).
Status Snapshotter::validate(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, Parsed *out) {
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  // 1. header and directory; 2. the sections' checksums
  COOC_TRY(parse_header(ctx, img, bytes, own_rank, &out->h));
  const BlobView v{&out->h, img};
  Carve c;
  const auto o_sums = c.take_last<unsigned long long>(kSnapSectionsMax);
  const auto o_err = c.take_last<unsigned int>(2);
  COOC_TRY(ctx.snap_sums.reserve(c.end));
  COOC_TRY(check_checksums(ctx, v, o_sums.in(ctx.snap_sums)));
  // 3. the contents.  Phase A: every array by position (ids, offsets, ranges); phase B: the rows through their
  //    offsets, once those have passed.  Format 2: the sampler's scalars first (item_cut bounds the counters'
  //    check; the cuts and the seed are the context's own)
  const bool sampled = out->h.format == kSnapFormatSampled;
  if (sampled) COOC_TRY(check_sampler_scalars(ctx, v, out));
  unsigned int *d_err = o_err.in(ctx.snap_sums);
  COOC_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned int) * 2, s));
  launch_phase_a(s, v, M, sampled ? int32_t(out->smp_scalars[kSsItemCut]) : 0, d_err);
  COOC_HIP_TRY(hipGetLastError());
  unsigned int err[2] = {0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err[0])
    return Status{COOC_ERR_ARG, "snapshot blob: invalid contents (checks failed: " + std::to_string(err[0]) +
                                    "; 1 user ids, 2 history offsets, 4 history items, 8 row ids, 16 row offsets, "
                                    "32 columns, 64 counts, 128 row-sum ids, 256 counted items, 512 item counters, "
                                    "1024 users with a total, 2048 totals)"};
  launch_phase_b(s, v, ctx.cfg.user_cut, d_err + 1);
  COOC_HIP_TRY(hipGetLastError());
  COOC_TRY(download_host_sections(ctx, v, out));  // (asynchronous, beside phase B)
  COOC_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err[1] & 1u)
    return Status{COOC_ERR_ARG, "snapshot blob: a global row's columns are not strictly ascending or its counts do "
                                "not sum to its row sum"};
  if (err[1] & 2u)
    return Status{COOC_ERR_ARG, "snapshot blob: a user with a history has no total, a total below its history's "
                                "length, or a history longer than user_cut"};
  return check_host_sections(*out, M);
}

// header and directory (the host-only code of cooc_snapshot_inspect), then the configuration against the context's
Status Snapshotter::parse_header(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, SnapHeader *h) {
  const int32_t format = format_of(ctx);
  uint8_t hdr[sizeof(SnapHeader)];
  const int64_t hdr_bytes = snap_header_bytes(snap_sections_of(format));
  if (bytes < hdr_bytes) return Status{COOC_ERR_ARG, "snapshot blob: shorter than its header"};
  COOC_HIP_TRY(hipMemcpy(hdr, img, size_t(hdr_bytes), hipMemcpyDeviceToHost));
  std::string why;
  if (snap_parse(hdr, bytes, h, &why, format) != COOC_OK) return Status{COOC_ERR_ARG, why};
  const int32_t M = ctx.cfg.n_items;
  if (h->n_items != M || h->window_size_ms != ctx.cfg.window_size_ms || h->user_cut != ctx.cfg.user_cut)
    return Status{COOC_ERR_ARG, "snapshot blob: taken with n_items " + std::to_string(h->n_items) + ", window " +
                                    std::to_string(h->window_size_ms) + " ms, user_cut " + std::to_string(h->user_cut) +
                                    "; this context has " + std::to_string(M) + ", " +
                                    std::to_string(ctx.cfg.window_size_ms) + " ms, " + std::to_string(ctx.cfg.user_cut)};
  const int32_t rank = ctx.comm ? ctx.comm->rank() : 0, world = ctx.comm ? ctx.comm->world() : 1;
  if (own_rank && (h->rank != rank || h->world != world))
    return Status{COOC_ERR_ARG, "snapshot blob: taken by rank " + std::to_string(h->rank) + " of " + std::to_string(h->world) +
                                    "; this context is rank " + std::to_string(rank) + " of " + std::to_string(world)};
  if (h->world == 1 && h->sec[kSnapXsumIds - 1].count > 0)
    return Status{COOC_ERR_ARG, "snapshot blob: row sums of other ranks without a communicator"};
  return Status::Ok();
}

Status Snapshotter::check_checksums(cooc_ctx &ctx, const BlobView &v, unsigned long long *d_sums) {
  hipStream_t s = ctx.stream;
  COOC_TRY(launch_checksums(s, v.img, *v.h, d_sums));
  unsigned long long sums[kSnapSectionsMax];
  COOC_HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < v.h->n_sections; k++)
    if (sums[k] != v.h->sec[k].sum)
      return Status{COOC_ERR_ARG, "snapshot blob: checksum mismatch in section " + std::to_string(k + 1)};
  return Status::Ok();
}

Status Snapshotter::check_sampler_scalars(cooc_ctx &ctx, const BlobView &v, Parsed *out) {
  out->smp_scalars.assign(kSnapSmpScalarWords, 0);
  COOC_HIP_TRY(hipMemcpy(out->smp_scalars.data(), v.raw(kSnapSmpScalars), sizeof(int64_t) * kSnapSmpScalarWords,
                         hipMemcpyDeviceToHost));
  const int64_t *sc = out->smp_scalars.data();
  std::string why;
  if (snap_check_sampler_scalars(sc, &why) != COOC_OK) return Status{COOC_ERR_ARG, why};
  const Sampler &smp = ctx.stream_state.sampler_;
  if (sc[kSsItemCut] != smp.item_cut() || uint64_t(sc[kSsSeed]) != smp.seed())
    return Status{COOC_ERR_ARG, "snapshot blob: taken with item_cut " + std::to_string(sc[kSsItemCut]) + ", seed " +
                                    std::to_string(sc[kSsSeed]) + "; this context has " + std::to_string(smp.item_cut()) +
                                    ", " + std::to_string(int64_t(smp.seed()))};
  if (v.h->world != 1) return Status{COOC_ERR_ARG, "snapshot blob: a sampled context is single-subtask"};
  return Status::Ok();
}

// the sections that become host state, into *out (asynchronous: the caller synchronises before it reads them)
Status Snapshotter::download_host_sections(cooc_ctx &ctx, const BlobView &v, Parsed *out) {
  hipStream_t s = ctx.stream;
  const int64_t n_users = v.count(kSnapUserIds), P = v.count(kSnapPendTs), n_pend = v.count(kSnapPendUsers);
  out->scalars.assign(kSnapScalarWords, 0);
  out->hist_ptr.assign(n_users + 1, 0);
  out->user_ids.assign(n_users, 0);
  out->pend.ts.assign(P, 0);
  out->pend.ptr.assign(P + 1, 0);
  out->pend.users.assign(n_pend, 0);
  out->pend.items.assign(n_pend, 0);
  auto get = [&](int kind, void *dst) -> Status {
    if (v.bytes(kind) > 0) COOC_HIP_TRY(hipMemcpyAsync(dst, v.raw(kind), size_t(v.bytes(kind)), hipMemcpyDeviceToHost, s));
    return Status::Ok();
  };
  COOC_TRY(get(kSnapScalars, out->scalars.data()));
  COOC_TRY(get(kSnapUserIds, out->user_ids.data()));
  COOC_TRY(get(kSnapHistPtr, out->hist_ptr.data()));
  COOC_TRY(get(kSnapPendTs, out->pend.ts.data()));
  COOC_TRY(get(kSnapPendPtr, out->pend.ptr.data()));
  COOC_TRY(get(kSnapPendUsers, out->pend.users.data()));
  COOC_TRY(get(kSnapPendItems, out->pend.items.data()));
  if (v.h->format == kSnapFormatSampled) {
    const int64_t n_cnt = v.count(kSnapSmpItemIds), n_tot = v.count(kSnapSmpUserIds);
    out->tot_ids.assign(n_tot, 0);
    out->totals.assign(n_tot, 0);
    out->cnt_ids.assign(n_cnt, 0);
    out->cnts.assign(n_cnt, 0);
    COOC_TRY(get(kSnapSmpUserIds, out->tot_ids.data()));
    COOC_TRY(get(kSnapSmpTotals, out->totals.data()));
    COOC_TRY(get(kSnapSmpItemIds, out->cnt_ids.data()));
    COOC_TRY(get(kSnapSmpItemCnts, out->cnts.data()));
  }
  return Status::Ok();
}

// ---- the pieces of an install that the plain and the parts path share ------------------------------------------
// The slabs as compact_global leaves them, for the lengths already in gs_.len: the rows back to back in row order
// (base = the prefix of len), bump = live = the nnz entries, and the growth slack launch_gs_merge's first window
// would otherwise compact for.  The caller copies the entries in and synchronises.
Status Snapshotter::lay_out_slabs(cooc_ctx &ctx, int64_t nnz) {
  StreamState &st = ctx.stream_state;
  GlobalSparse &g = st.gs_;
  const int32_t M = ctx.cfg.n_items;
  const int64_t cap = std::max<int64_t>(2 * nnz, int64_t(1) << 12);
  COOC_TRY(g.col.reserve(sizeof(int32_t) * size_t(cap)));
  COOC_TRY(g.cnt.reserve(sizeof(uint32_t) * size_t(cap)));
  COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(M)));
  int64_t serr = 0;
  COOC_TRY(launch_scan_ws<false>(ScanI32{g.len.as<int32_t>()}, g.base.as<int64_t>(), M,
                                 st.d_scan_tmp_.as<unsigned long long>(), &serr, ctx.stream));
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  if (serr & 8) return Status{COOC_ERR_STATE, "internal bounds check failed (restored slab prefix)"};
  g.cap = cap;
  g.bump = g.live = nnz;
  g.compactions = 0;
  return Status::Ok();
}

// A fresh arena with every list at finish()'s own first capacity: aoff[j] = where list j starts
Status Snapshotter::lay_out_histories(cooc_ctx &ctx, const std::vector<int64_t> &lens, std::vector<int64_t> *aoff) {
  StreamState &st = ctx.stream_state;
  aoff->resize(lens.size());
  int64_t used = 0;
  for (size_t j = 0; j < lens.size(); j++) {
    (*aoff)[j] = used;
    used += std::max<int64_t>(16, lens[j]);
  }
  st.arena_used_ = used;
  return st.grow_arena(ctx, std::max<int64_t>(used, 1024));
}

// the slot tables in user order
void Snapshotter::set_slots(StreamState &st, const std::vector<int32_t> &user_ids, const std::vector<int64_t> &lens,
                            const std::vector<int64_t> &aoff) {
  for (size_t j = 0; j < user_ids.size(); j++) {
    const int32_t slot = st.slot_for(user_ids[j]);  // (dense_slot_ / slot_of_, staged_stamp_, staged_pos_)
    st.h_off_[slot] = aoff[j];
    st.h_len_[slot] = int32_t(lens[j]);
    st.h_cap_[slot] = int32_t(std::max<int64_t>(16, lens[j]));
  }
}

// the running totals of d_scal_ after a global install (synchronises s: the rows' copies are done with it)
Status Snapshotter::upload_running_totals(cooc_ctx &ctx, int64_t scal2, int64_t scal3) {
  int64_t scal[8] = {0, 0, scal2, scal3, 0, 0, 0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(ctx.stream_state.d_scal_.p, scal, sizeof(scal), hipMemcpyHostToDevice, ctx.stream));
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  return Status::Ok();
}

// accumulators and the operator
void Snapshotter::set_operator(cooc_ctx &ctx, const int64_t *scalars, const PendingWindows &pend) {
  StreamState &st = ctx.stream_state;
  Operator &op = ctx.op;
  st.observed_exact = scalars[kScObservedExact];
  st.observed_ref = scalars[kScObservedRef];
  st.rowsum_acc = scalars[kScRowsumAcc];
  st.rescored_items = scalars[kScRescoredItems];
  op.late_elements = scalars[kScLateElements];
  op.watermark = scalars[kScWatermark];
  op.agreed_ = scalars[kScAgreed];
  op.regather_ = scalars[kScRegather] != 0;
  for (size_t k = 0; k < pend.ts.size(); k++) {
    Operator::Pending &p = op.pending_[pend.ts[k]];
    p.users.assign(pend.users.begin() + pend.ptr[k], pend.users.begin() + pend.ptr[k + 1]);
    p.items.assign(pend.items.begin() + pend.ptr[k], pend.items.begin() + pend.ptr[k + 1]);
  }
}

// ---- install ----------------------------------------------------------------------------------------------------
// global rows, row sums, running totals: in this context's representation (ensure_global chooses it)
Status Snapshotter::install_rows(cooc_ctx &ctx, const BlobView &v, const Parsed &p) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  const int64_t R = v.count(kSnapRowIds), nnz = v.count(kSnapRowCols), X = v.count(kSnapXsumIds);
  COOC_TRY(st.ensure_global(ctx));  // (zeroed: the matrix or the slabs' base / len, the row sums, the totals)
  const int32_t *ids = v.at<int32_t>(kSnapRowIds);
  const int64_t *rp = v.at<int64_t>(kSnapRowPtr);
  const int32_t *col = v.at<int32_t>(kSnapRowCols);
  const uint32_t *cnt = v.at<uint32_t>(kSnapRowCnts);
  int64_t *grs = st.d_grs_.as<int64_t>();
  if (R > 0) {
    k_snap_scatter_meta<<<blocks_for(R, 256), 256, 0, s>>>(R, ids, rp, v.at<int64_t>(kSnapRowSums), grs,
                                                            st.sparse_global_ ? st.gs_.len.as<int32_t>() : nullptr);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (X > 0) {
    k_snap_scatter_i64<<<blocks_for(X, 256), 256, 0, s>>>(X, v.at<int32_t>(kSnapXsumIds), v.at<int64_t>(kSnapXsumVals), grs);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (st.sparse_global_) {
    COOC_TRY(lay_out_slabs(ctx, nnz));
    if (nnz > 0) {
      COOC_HIP_TRY(hipMemcpyAsync(st.gs_.col.p, col, sizeof(int32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
      COOC_HIP_TRY(hipMemcpyAsync(st.gs_.cnt.p, cnt, sizeof(uint32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
    }
  } else if (R > 0) {
    k_snap_scatter_dense<<<wave_grid(R), 256, 0, s>>>(R, M, ids, rp, col, cnt, st.d_global_.as<uint32_t>());
    COOC_HIP_TRY(hipGetLastError());
  }
  return upload_running_totals(ctx, p.scalars[kScScal2], p.scalars[kScScal3]);
}

Status Snapshotter::install(cooc_ctx &ctx, const char *img, const Parsed &p) {
  StreamState &st = ctx.stream_state;
  const BlobView v{&p.h, img};
  const std::vector<int64_t> &scalars = p.scalars, &hist_ptr = p.hist_ptr;
  const int64_t n_users = v.count(kSnapUserIds);
  const bool sampled = p.h.format == kSnapFormatSampled;
  if (v.count(kSnapRowIds) > 0 || v.count(kSnapXsumIds) > 0 || scalars[kScScal2] != 0 || scalars[kScScal3] != 0)
    COOC_TRY(install_rows(ctx, v, p));

  // ---- histories: a fresh arena, every list at finish()'s own first capacity; the slot tables in user order
  std::vector<int64_t> lens(n_users), aoff;
  if (n_users > 0) {
    for (int64_t j = 0; j < n_users; j++) lens[j] = hist_ptr[j + 1] - hist_ptr[j];
    COOC_TRY(lay_out_histories(ctx, lens, &aoff));
    const std::vector<int64_t> chunk_pre = chunk_prefix(hist_ptr);
    COOC_TRY(launch_copy_lists(ctx, false, chunk_pre, aoff, v.at<int64_t>(kSnapHistPtr), v.at<int32_t>(kSnapHistItems),
                               st.arena_.as<int32_t>()));
    COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));  // (the uploads read chunk_pre and aoff)
    // (format 2: the slot tables are made below, over every user with a total)
    if (!sampled) set_slots(st, p.user_ids, lens, aoff);
  }
  if (sampled) {
    // the slot tables in user order over every user with a total; those with a history (a subset, both lists
    // ascending) get it
    size_t j = 0;
    for (size_t t = 0; t < p.tot_ids.size(); t++) {
      const int32_t slot = st.slot_for(p.tot_ids[t]);
      if (j < p.user_ids.size() && p.user_ids[j] == p.tot_ids[t]) {
        st.h_off_[slot] = aoff[j];
        st.h_len_[slot] = int32_t(lens[j]);
        st.h_cap_[slot] = int32_t(std::max<int64_t>(16, lens[j]));
        j++;
      }
    }
    if (j != p.user_ids.size()) return Status{COOC_ERR_STATE, "internal error: a restored history without a total"};
    COOC_TRY(install_samplers(ctx, v, p));
  }
  set_operator(ctx, scalars.data(), p.pend);
  return Status::Ok();
}

// The samplers' state of a validated format-2 blob, after the slot tables: the host sampler's vectors, or the
// device sampler's arrays scattered on the device (its per-slot arrays grown to the restored slots first).
Status Snapshotter::install_samplers(cooc_ctx &ctx, const BlobView &v, const Parsed &p) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int64_t n_slots = int64_t(st.h_off_.size()), n_tot = int64_t(p.tot_ids.size()), n_cnt = int64_t(p.cnt_ids.size());
  const int64_t n_users = int64_t(p.user_ids.size());
  const int64_t *sc = p.smp_scalars.data();
  std::vector<int32_t> slots(n_tot);
  for (int64_t t = 0; t < n_tot; t++) slots[t] = st.find_slot(p.tot_ids[t]);
  if (!st.dev_sampler_.enabled()) {
    Sampler &m = st.sampler_;
    m.reset();
    for (int64_t k = 0; k < n_cnt; k++) m.item_count_[p.cnt_ids[k]] = p.cnts[k];
    m.len_.assign(n_slots, 0);
    m.total_.assign(n_slots, 0);
    m.stamp_.assign(n_slots, -1);
    m.pos_.assign(n_slots, 0);
    for (int64_t t = 0; t < n_tot; t++) {
      m.total_[slots[t]] = p.totals[t];
      m.len_[slots[t]] = st.h_len_[slots[t]];
    }
    m.rejected_ = sc[kSsRejected];
    m.fills_ = sc[kSsFills];
    m.replacements_ = sc[kSsReplacements];
    m.feedbacks_ = sc[kSsFeedbacks];
    m.n_users_ = n_users;
    return Status::Ok();
  }
  SampleStream &d = st.dev_sampler_;
  COOC_TRY(reset_samplers(ctx));  // (zeroed counters and per-slot arrays)
  COOC_TRY(d.grow_slots(n_slots, s));
  if (n_cnt > 0)
    k_snap_scatter_counts<<<blocks_for(n_cnt, 256), 256, 0, s>>>(n_cnt, v.at<int32_t>(kSnapSmpItemIds),
                                                                 v.at<int16_t>(kSnapSmpItemCnts), d.count_.as<int32_t>());
  if (n_tot > 0) {
    COOC_TRY(ctx.snap_tmp2.reserve(sizeof(int32_t) * size_t(n_tot)));
    int32_t *d_slots = ctx.snap_tmp2.as<int32_t>();
    COOC_HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), sizeof(int32_t) * size_t(n_tot), hipMemcpyHostToDevice, s));
    const int32_t *d_tids = v.at<int32_t>(kSnapSmpUserIds);
    k_snap_scatter_totals<<<blocks_for(n_tot, 256), 256, 0, s>>>(n_tot, d_slots, v.at<int32_t>(kSnapSmpTotals), d.slot_cap_,
                                                                 d.total_.as<int32_t>());
    if (n_users > 0)
      k_snap_scatter_lens<<<blocks_for(n_users, 256), 256, 0, s>>>(n_users, v.at<int32_t>(kSnapUserIds),
                                                                   v.at<int64_t>(kSnapHistPtr), d_tids, n_tot, d_slots,
                                                                   d.slot_cap_, d.len_.as<int32_t>());
  }
  COOC_HIP_TRY(hipGetLastError());
  // the decision counters: [0..3] saved, [4] the users with a reservoir; the rest is recomputed when read
  int64_t ctr[8] = {sc[kSsRejected], sc[kSsFills], sc[kSsReplacements], sc[kSsFeedbacks], n_users, 0, 0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(d.ctr_.p, ctr, sizeof(ctr), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));  // (the uploads read slots and ctr)
  return Status::Ok();
}

}  // namespace cooc

void cooc_ctx::snapshot_release() {
  if (snap_bytes < 0 && !snap_img.p) return;
  (void)hipSetDevice(device);
  snap_img.release();
  snap_rp.release();
  snap_col.release();
  snap_cnt.release();
  snap_live.release();
  snap_bytes = -1;
}
