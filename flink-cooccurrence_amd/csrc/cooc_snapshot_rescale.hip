// cooc_snapshot_rescale.hip — restore of a checkpoint into another parallelism (cooc_restore_begin_parts ..
// _finish_parts): ALL blobs of one checkpoint (one per old subtask) into this context's
// (rank, world).  All parts are resident on the device at once, so a restoring rank needs memory for the whole
// job's blobs next to its own share of the state.  Every part alone passes the validation of a plain restore
// (cooc_snapshot_restore.hip); then, across parts:
//
//   k_snap_keep_users + select_flagged        the users the route keeps, per part
//   k_snap_parts_rows / _xsums / k_snap_keep_rows   M-sized tables of the job's rows (owner part, offset, length,
//                       job-wide row sum), the cross-part checks, the rows this rank keeps
//   k_snap_copy_parts   kept rows / histories from the W_old images to the slabs / the arena (2,048 elements per
//                       wave, 16-B accesses where both sides sit alike)
//   k_snap_scatter_dense_parts   kept rows into the dense matrix
//
// All of it is bandwidth-bound and runs on the context's stream.
#include <cstring>
#include <utility>

#include "cooc_radix.h"
#include "cooc_snapshot_impl.h"

namespace cooc {
namespace {

// ---- rescaling: the parts of one checkpoint into another (rank, world) ------------------------------------------
// What the kernels below read of one validated part (device pointers into its image).
struct PartView {
  const int32_t *row_ids;
  const int64_t *row_ptr, *row_sums;
  const int32_t *xsum_ids;
  const int64_t *xsum_vals;
  const int32_t *col;
  const uint32_t *cnt;
  const int32_t *hist;
  int64_t R, X;
};

// Python's u % w (the result has the sign of w > 0)
__host__ __device__ inline int32_t floor_mod(int32_t u, int32_t w) {
  const int32_t m = u % w;
  return m < 0 ? m + w : m;
}

// flag[j]: the route keeps user ids[j] -- floor-mod(u, world) == rank, or bit u of bits[0, n_bits)
__global__ __launch_bounds__(256) void k_snap_keep_users(const int32_t *__restrict__ ids, int64_t n, int32_t kind,
                                                         int32_t world, int32_t rank, int64_t n_bits,
                                                         const uint64_t *__restrict__ bits, uint8_t *__restrict__ flag) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= n) return;
  const int32_t u = ids[j];
  bool keep;
  if (kind == COOC_ROUTE_MOD) keep = floor_mod(u, world) == rank;
  else keep = u >= 0 && int64_t(u) < n_bits && ((bits[u >> 6] >> (u & 63)) & 1ull) != 0;
  flag[j] = keep ? 1 : 0;
}

// The job's rows as M-sized tables, from the parts' own tables (blockIdx.y = the part r): owner[a] = r, the
// row's offset and length in r's columns / counts, and its row sum.  A row a of part r with a mod W != r fails
// (bit 1); the others' ids are distinct across parts, so every table cell has one writer.
__global__ __launch_bounds__(256) void k_snap_parts_rows(const PartView *__restrict__ P, int32_t W,
                                                         int32_t *__restrict__ owner, int64_t *__restrict__ off,
                                                         int32_t *__restrict__ len, int64_t *__restrict__ grs,
                                                         unsigned int *err) {
  const int32_t r = blockIdx.y;
  const PartView p = P[r];
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (j < p.R) {
    const int32_t a = p.row_ids[j];
    if (a % W != r) {
      bad = true;
    } else {
      const int64_t b = p.row_ptr[j];
      owner[a] = r;
      off[a] = b;
      len[a] = int32_t(p.row_ptr[j + 1] - b);
      grs[a] = p.row_sums[j];
    }
  }
  val_fold(bad, err, 1u);
}

// Part r's row sums of other ranks against the tables: each is a row of another part with that row sum (bit 2).
// Their number equals the other parts' rows (snap_check_parts) and their ids are distinct, so none is missing.
__global__ __launch_bounds__(256) void k_snap_parts_xsums(const PartView *__restrict__ P, int32_t W,
                                                          const int32_t *__restrict__ owner,
                                                          const int64_t *__restrict__ grs, unsigned int *err) {
  const int32_t r = blockIdx.y;
  const PartView p = P[r];
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (j < p.X) {
    const int32_t a = p.xsum_ids[j];
    bad = a % W == r || owner[a] < 0 || grs[a] != p.xsum_vals[j];
  }
  val_fold(bad, err, 2u);
}

// klen[a] = the length of row a when this context keeps it (a mod world == rank), else 0; tot[0] = kept rows,
// tot[1] = rows of other ranks (their row sums go into the next snapshot's sections 10 / 11), tot[2] = kept
// entries.  A grid-stride loop over at most 512 workgroups, one atomic per workgroup and total (the three totals
// are single addresses: an atomic per wave serialises at 1e6 items).
__global__ __launch_bounds__(256) void k_snap_keep_rows(int32_t M, int32_t world, int32_t rank,
                                                        const int32_t *__restrict__ owner,
                                                        const int32_t *__restrict__ len, int32_t *__restrict__ klen,
                                                        unsigned long long *__restrict__ tot) {
  __shared__ unsigned long long s_t[4][3];
  unsigned long long kept = 0, other = 0, e = 0;
  for (int64_t a = int64_t(blockIdx.x) * 256 + threadIdx.x; a < M; a += int64_t(gridDim.x) * 256) {
    const bool row = owner[a] >= 0, keep = row && a % world == rank;
    const int32_t n = keep ? len[a] : 0;
    klen[a] = n;
    kept += keep ? 1 : 0;
    other += (row && !keep) ? 1 : 0;
    e += unsigned(n);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kept += __shfl_xor(kept, o, 64);
    other += __shfl_xor(other, o, 64);
    e += __shfl_xor(e, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_t[threadIdx.x >> 6][0] = kept;
    s_t[threadIdx.x >> 6][1] = other;
    s_t[threadIdx.x >> 6][2] = e;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long t = s_t[0][threadIdx.x] + s_t[1][threadIdx.x] + s_t[2][threadIdx.x] + s_t[3][threadIdx.x];
    if (t) atomicAdd(&tot[threadIdx.x], t);
  }
}

// pieces of kListChunk entries of a list of len[i] entries
struct ScanChunksI32 {
  const int32_t *len;
  __device__ int64_t operator()(int64_t i) const { return (int64_t(len[i]) + kListChunk - 1) / kListChunk; }
};

// k_snap_copy_lists with the source chosen per list: list j is len[j] elements at soff[j] of src0[part[j]] (and of
// src1[part[j]] when kTwo: a row's columns and counts share their offsets) and goes to doff[j] of dst0 (dst1).
// Pieces of kListChunk elements, one wave per piece, piece c in the list j with pre[j] <= c < pre[j + 1] (lists
// without a piece, len 0, are never found).  A run starts 4-B aligned on both sides; where source and
// destination sit alike within 16 B it moves as up to 3 head words, 16-B groups and up to 3 tail words.
__device__ inline void copy_run(const uint32_t *__restrict__ sp, uint32_t *__restrict__ dp, int64_t n, int lane) {
  const unsigned ms = unsigned(reinterpret_cast<uintptr_t>(sp) >> 2) & 3u, md = unsigned(reinterpret_cast<uintptr_t>(dp) >> 2) & 3u;
  if (ms == md) {
    const int64_t head = min(n, int64_t((4u - ms) & 3u));
    if (lane < head) dp[lane] = sp[lane];
    const int64_t nvec = (n - head) >> 2, tail0 = head + nvec * 4;
    const uint4 *sv = reinterpret_cast<const uint4 *>(sp + head);
    uint4 *dv = reinterpret_cast<uint4 *>(dp + head);
    for (int64_t g = lane; g < nvec; g += 64) dv[g] = sv[g];
    if (tail0 + lane < n) dp[tail0 + lane] = sp[tail0 + lane];
  } else {
    for (int64_t i = lane; i < n; i += 64) dp[i] = sp[i];
  }
}
template <bool kTwo>
__global__ __launch_bounds__(256) void k_snap_copy_parts(int64_t n_lists, int64_t n_chunks, const int64_t *__restrict__ pre,
                                                         const int32_t *__restrict__ part, const int64_t *__restrict__ soff,
                                                         const int64_t *__restrict__ doff, const int32_t *__restrict__ len,
                                                         const uint32_t *const *__restrict__ src0,
                                                         const uint32_t *const *__restrict__ src1,
                                                         uint32_t *__restrict__ dst0, uint32_t *__restrict__ dst1) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t c = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    int64_t lo = 0, hi = n_lists;  // invariant: pre[lo] <= c < pre[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (pre[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t i0 = (c - pre[lo]) * kListChunk, n = min(int64_t(len[lo]) - i0, kListChunk);
    const int64_t so = soff[lo] + i0, d = doff[lo] + i0;
    const int32_t p = part[lo];
    copy_run(src0[p] + so, dst0 + d, n, lane);
    if (kTwo) copy_run(src1[p] + so, dst1 + d, n, lane);
  }
}

// k_snap_scatter_dense filtered and reading from the parts: one wave per kept row a (klen[a] > 0) into the
// (zeroed) dense matrix
__global__ __launch_bounds__(256) void k_snap_scatter_dense_parts(int32_t M, const PartView *__restrict__ P,
                                                                  const int32_t *__restrict__ owner,
                                                                  const int64_t *__restrict__ off,
                                                                  const int32_t *__restrict__ klen, uint32_t *__restrict__ G) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t a = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; a < M; a += n_waves) {
    const int32_t n = klen[a];
    if (n == 0) continue;
    const int32_t *col = P[owner[a]].col + off[a];
    const uint32_t *cnt = P[owner[a]].cnt + off[a];
    uint32_t *g = G + a * int64_t(M);
    for (int32_t i = lane; i < n; i += 64) g[col[i]] = cnt[i];
  }
}

// the route (NULL: COOC_ROUTE_MOD) checked, a bitmap cut to the int32 user ids
Status parse_route(const cooc_user_route *route, cooc_user_route *rt) {
  *rt = cooc_user_route{COOC_ROUTE_MOD, 0, 0, nullptr};
  if (route) *rt = *route;
  if (rt->kind != COOC_ROUTE_MOD && rt->kind != COOC_ROUTE_BITMAP) return Status{COOC_ERR_ARG, "user route: unknown kind"};
  if (rt->reserved != 0) return Status{COOC_ERR_ARG, "user route: reserved field set"};
  if (rt->kind == COOC_ROUTE_BITMAP && (rt->n_bits < 0 || (rt->n_bits > 0 && !rt->bits)))
    return Status{COOC_ERR_ARG, "user route: a bitmap of n_bits > 0 needs bits"};
  if (rt->kind == COOC_ROUTE_BITMAP) rt->n_bits = std::min<int64_t>(rt->n_bits, int64_t(1) << 31);  // (user ids are int32)
  return Status::Ok();
}

// the three totals of k_snap_keep_rows, then the cross-part checks' error word
struct PartsCtl {
  unsigned long long tot[3];
  unsigned int err;
};

}  // namespace

// The job under restore: the route into this context's (rank, world), every part validated alone (views[i] over
// parts[i].h and the part's image), the scalars merged across parts.
struct PartsJob {
  cooc_user_route rt;
  int32_t rank, world;
  std::vector<Snapshotter::Parsed> parts;
  std::vector<BlobView> views;
  int64_t merged[kSnapScalarWords];
  int64_t total_rows = 0, most_users = 0, most_rows = 0, most_x = 0;
  bool keeps(int32_t u) const {
    if (rt.kind == COOC_ROUTE_MOD) return floor_mod(u, world) == rank;
    return u >= 0 && int64_t(u) < rt.n_bits && ((rt.bits[u >> 6] >> (u & 63)) & 1ull) != 0;
  }
};

// The rows across parts as M-sized tables on the device (snap_tmp: no allocation per call once it has grown) --
// owner part, offset, length, job-wide row sum; klen / pre for the rows this rank keeps -- beside the parts' views
// and section pointers (src[0..2][i]: part i's columns, counts, history items).  The h_ vectors are what the
// uploads read: they live as long as the tables.
struct RowTables {
  int32_t *owner, *len, *klen;
  int64_t *off, *grs, *pre;
  PartsCtl *ctl;
  PartView *views;
  const uint32_t *const *src[3];
  unsigned long long *scan;
  std::vector<PartView> h_views;
  std::vector<const uint32_t *> h_src[3];
};

// a user of the job: where its history is (part, index there) and whether the route keeps it
struct KeptUser {
  int32_t user, part, idx, keep;
};

namespace {

// The tables filled by k_snap_parts_rows and checked by k_snap_parts_xsums (ctl->err; asynchronous)
Status build_row_tables(cooc_ctx &ctx, const PartsJob &job, RowTables *out) {
  hipStream_t s = ctx.stream;
  const size_t M = size_t(ctx.cfg.n_items), W = job.views.size();
  RowTables &t = *out;
  DevBuf &tbl = ctx.snap_tmp;
  Carve c;
  const auto o_owner = c.take<int32_t>(M), o_len = c.take<int32_t>(M), o_klen = c.take<int32_t>(M);
  const auto o_off = c.take<int64_t>(M), o_grs = c.take<int64_t>(M), o_pre = c.take<int64_t>(M + 1);
  const auto o_ctl = c.take<PartsCtl>(1);
  const auto o_views = c.take<PartView>(W);
  const Carved<const uint32_t *> o_src[3] = {c.take<const uint32_t *>(W), c.take<const uint32_t *>(W),
                                             c.take<const uint32_t *>(W)};
  const auto o_scan = c.take<unsigned long long>(scan_ws_bytes(int64_t(M)) / sizeof(unsigned long long));
  static_assert(sizeof(PartsCtl) <= 256, "the control block is one 256-B slot");
  COOC_TRY(tbl.reserve(c.end));
  t.owner = o_owner.in(tbl), t.len = o_len.in(tbl), t.klen = o_klen.in(tbl);
  t.off = o_off.in(tbl), t.grs = o_grs.in(tbl), t.pre = o_pre.in(tbl);
  t.ctl = o_ctl.in(tbl);
  t.views = o_views.in(tbl);
  t.scan = o_scan.in(tbl);
  t.h_views.resize(W);
  for (int k = 0; k < 3; k++) t.h_src[k].resize(W);
  for (size_t i = 0; i < W; i++) {
    const BlobView &b = job.views[i];
    PartView &v = t.h_views[i];
    v.row_ids = b.at<int32_t>(kSnapRowIds);
    v.row_ptr = b.at<int64_t>(kSnapRowPtr);
    v.row_sums = b.at<int64_t>(kSnapRowSums);
    v.xsum_ids = b.at<int32_t>(kSnapXsumIds);
    v.xsum_vals = b.at<int64_t>(kSnapXsumVals);
    v.col = b.at<int32_t>(kSnapRowCols);
    v.cnt = b.at<uint32_t>(kSnapRowCnts);
    v.hist = b.at<int32_t>(kSnapHistItems);
    v.R = b.count(kSnapRowIds);
    v.X = b.count(kSnapXsumIds);
    t.h_src[0][i] = b.at<uint32_t>(kSnapRowCols);
    t.h_src[1][i] = v.cnt;
    t.h_src[2][i] = b.at<uint32_t>(kSnapHistItems);
  }
  COOC_HIP_TRY(hipMemcpyAsync(t.views, t.h_views.data(), sizeof(PartView) * W, hipMemcpyHostToDevice, s));
  for (int k = 0; k < 3; k++) {
    const uint32_t **d = o_src[k].in(tbl);
    COOC_HIP_TRY(hipMemcpyAsync(d, t.h_src[k].data(), sizeof(void *) * W, hipMemcpyHostToDevice, s));
    t.src[k] = d;
  }
  COOC_HIP_TRY(hipMemsetAsync(t.owner, 0xFF, sizeof(int32_t) * M, s));  // -1: no part has the row
  COOC_HIP_TRY(hipMemsetAsync(t.len, 0, sizeof(int32_t) * M, s));
  COOC_HIP_TRY(hipMemsetAsync(t.off, 0, sizeof(int64_t) * M, s));
  COOC_HIP_TRY(hipMemsetAsync(t.grs, 0, sizeof(int64_t) * M, s));
  COOC_HIP_TRY(hipMemsetAsync(t.ctl, 0, 256, s));
  if (job.most_rows > 0)
    k_snap_parts_rows<<<dim3(blocks_for(job.most_rows, 256), unsigned(W)), 256, 0, s>>>(t.views, int32_t(W), t.owner, t.off,
                                                                                        t.len, t.grs, &t.ctl->err);
  if (job.most_x > 0)
    k_snap_parts_xsums<<<dim3(blocks_for(job.most_x, 256), unsigned(W)), 256, 0, s>>>(t.views, int32_t(W), t.owner, t.grs,
                                                                                      &t.ctl->err);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// The users the route keeps: flags per part on the device, select_flagged; the tables stay host state.  Every
// part's ids ascend, so the parts merge pairwise into the job's users in id order, and the kept ones come out in
// the order a plain restore installs them.
Status kept_users(cooc_ctx &ctx, const PartsJob &job, std::vector<KeptUser> *kept) {
  hipStream_t s = ctx.stream;
  const cooc_user_route &rt = job.rt;
  const int32_t W = int32_t(job.views.size());
  std::vector<std::vector<KeptUser>> runs(W);
  const size_t n_words = rt.kind == COOC_ROUTE_BITMAP ? size_t((rt.n_bits + 63) / 64) : 0;
  Carve c;
  const auto o_flag = c.take<uint8_t>(size_t(job.most_users));
  const auto o_idx = c.take<int32_t>(size_t(job.most_users)), o_n = c.take<int32_t>(1);
  const auto o_sel = c.take<char>(select_tmp_bytes(job.most_users));
  const auto o_bits = c.take_last<uint64_t>(n_words);
  COOC_TRY(ctx.snap_tmp2.reserve(c.end));
  const uint64_t *d_bits = nullptr;
  if (n_words > 0) {
    COOC_HIP_TRY(hipMemcpyAsync(o_bits.in(ctx.snap_tmp2), rt.bits, sizeof(uint64_t) * n_words, hipMemcpyHostToDevice, s));
    d_bits = o_bits.in(ctx.snap_tmp2);
  }
  uint8_t *d_flag = o_flag.in(ctx.snap_tmp2);
  int32_t *d_idx = o_idx.in(ctx.snap_tmp2), *d_n = o_n.in(ctx.snap_tmp2);
  char *d_sel = o_sel.in(ctx.snap_tmp2);
  std::vector<int32_t> idx;
  for (int32_t i = 0; i < W; i++) {
    const int64_t n = job.views[i].count(kSnapUserIds);
    if (n == 0) continue;
    k_snap_keep_users<<<blocks_for(n, 256), 256, 0, s>>>(job.views[i].at<int32_t>(kSnapUserIds), n, rt.kind, job.world,
                                                         job.rank, rt.n_bits, d_bits, d_flag);
    COOC_HIP_TRY(hipGetLastError());
    COOC_TRY(select_flagged(d_flag, n, d_idx, d_n, d_sel, s));
    int32_t n_kept = 0;
    COOC_HIP_TRY(hipMemcpyAsync(&n_kept, d_n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (n_kept < 0 || int64_t(n_kept) > n) return Status{COOC_ERR_STATE, "internal bounds check failed (kept users)"};
    idx.resize(size_t(n_kept));
    if (n_kept > 0) COOC_HIP_TRY(hipMemcpy(idx.data(), d_idx, sizeof(int32_t) * size_t(n_kept), hipMemcpyDeviceToHost));
    std::vector<KeptUser> &run = runs[i];
    run.resize(size_t(n));
    for (int64_t j = 0; j < n; j++) run[j] = KeptUser{job.parts[i].user_ids[j], i, int32_t(j), 0};
    for (int32_t j : idx) {
      if (j < 0 || int64_t(j) >= n) return Status{COOC_ERR_STATE, "internal bounds check failed (kept users)"};
      run[j].keep = 1;
    }
  }
  COOC_HIP_TRY(hipStreamSynchronize(s));  // (the bitmap's upload reads the caller's memory)
  while (runs.size() > 1) {
    std::vector<std::vector<KeptUser>> next;
    for (size_t i = 0; i + 1 < runs.size(); i += 2) {
      std::vector<KeptUser> m(runs[i].size() + runs[i + 1].size());
      std::merge(runs[i].begin(), runs[i].end(), runs[i + 1].begin(), runs[i + 1].end(), m.begin(),
                 [](const KeptUser &a, const KeptUser &b) { return a.user < b.user; });
      next.push_back(std::move(m));
    }
    if (runs.size() & 1) next.push_back(std::move(runs.back()));
    runs.swap(next);
  }
  // The one check that user ids are disjoint across parts: a part's own ids ascend strictly (validate), so a
  // duplicate is a user of two parts, and the merged run has the two side by side.
  for (size_t j = 0; j < runs[0].size(); j++) {
    if (j > 0 && runs[0][j - 1].user == runs[0][j].user)
      return Status{COOC_ERR_ARG, "snapshot parts: a user id in more than one part"};
    if (runs[0][j].keep) kept->push_back(runs[0][j]);
  }
  return Status::Ok();
}

}  // namespace

Status Snapshotter::restore_begin_parts(cooc_ctx &ctx, int32_t n_parts, const int64_t *bytes) {
  if (!empty_state(ctx))
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  // (the cross-part kernels take the part from blockIdx.y, at most 65,535; Flink's parallelism ends at 32,768)
  if (n_parts < 1 || n_parts > COOC_MAX_RESTORE_PARTS)
    return Status{COOC_ERR_ARG, "snapshot parts: n_parts outside [1, " + std::to_string(COOC_MAX_RESTORE_PARTS) + "]"};
  if (!bytes) return Status{COOC_ERR_ARG, "snapshot parts: bytes is NULL"};
  std::vector<int64_t> off(size_t(n_parts) + 1, 0), len(bytes, bytes + n_parts);
  for (int32_t i = 0; i < n_parts; i++) {
    if (len[i] < kSnapHeaderBytes) return Status{COOC_ERR_ARG, "snapshot parts: a part shorter than its header"};
    if (len[i] > (INT64_MAX >> 1) - off[i]) return Status{COOC_ERR_ARG, "snapshot parts: lengths overflow"};
    off[i + 1] = int64_t(al256(size_t(off[i] + len[i])));
  }
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  ctx.snapshot_release();
  drop_restore(ctx);
  COOC_TRY(ctx.restore_img.reserve(size_t(off[n_parts])));
  COOC_HIP_TRY(hipMemsetAsync(ctx.restore_img.p, 0, size_t(off[n_parts]), ctx.stream));  // (ranges never written read as 0)
  COOC_HIP_TRY(hipStreamSynchronize(ctx.stream));
  ctx.restore_part_off = std::move(off);
  ctx.restore_part_len = std::move(len);
  return Status::Ok();
}

Status Snapshotter::restore_write_part(cooc_ctx &ctx, int32_t part, int64_t offset, int64_t n, const uint8_t *src) {
  if (ctx.restore_part_len.empty())
    return Status{COOC_ERR_STATE, "no restore from parts in progress: call cooc_restore_begin_parts first"};
  if (part < 0 || size_t(part) >= ctx.restore_part_len.size()) return Status{COOC_ERR_ARG, "snapshot parts: no such part"};
  const int64_t len = ctx.restore_part_len[part];
  if (offset < 0 || n < 0 || offset > len || n > len - offset)
    return Status{COOC_ERR_ARG, "bytes [" + std::to_string(offset) + ", +" + std::to_string(n) + ") outside the " +
                                    std::to_string(len) + " B announced for part " + std::to_string(part)};
  if (n == 0) return Status::Ok();
  if (!src) return Status{COOC_ERR_ARG, "src is NULL"};
  COOC_HIP_TRY(hipSetDevice(ctx.device));
  COOC_HIP_TRY(hipMemcpy(ctx.restore_img.as<char>() + ctx.restore_part_off[part] + offset, src, size_t(n), hipMemcpyHostToDevice));
  return Status::Ok();
}

Status Snapshotter::restore_finish_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info) {
  if (ctx.restore_part_len.empty())
    return Status{COOC_ERR_STATE, "no restore from parts in progress: call cooc_restore_begin_parts first"};
  if (!empty_state(ctx)) {
    drop_restore(ctx);
    return Status{COOC_ERR_STATE, "a snapshot restores only into a context without streaming state"};
  }
  Status r = hipSetDevice(ctx.device) == hipSuccess ? validate_and_install_parts(ctx, route, info)
                                                    : Status{COOC_ERR_HIP, "hipSetDevice"};
  if (!r.ok()) wipe(ctx);
  (void)hipStreamSynchronize(ctx.stream);
  drop_restore(ctx);
  return r;
}

// Validation first, all of it; the installs run only on parts that have passed every check.
Status Snapshotter::validate_and_install_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info) {
  hipStream_t s = ctx.stream;
  PartsJob job;
  job.rank = ctx.comm ? ctx.comm->rank() : 0;
  job.world = ctx.comm ? ctx.comm->world() : 1;
  COOC_TRY(parse_route(route, &job.rt));
  COOC_TRY(validate_parts(ctx, &job));  // every part alone, then across parts from headers and scalars
  RowTables t;
  COOC_TRY(build_row_tables(ctx, job, &t));  // the rows across parts, checked on the device (asynchronous)
  std::vector<KeptUser> kept;
  COOC_TRY(kept_users(ctx, job, &kept));
  unsigned int err = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&err, &t.ctl->err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err)
    return Status{COOC_ERR_ARG, "snapshot parts: invalid across parts (checks failed: " + std::to_string(err) +
                                    "; 1 a row in a part that does not own it, 2 a part's row sums of other ranks are "
                                    "not the other parts' rows' sums)"};
  const PendingWindows pend = pending_union(job);

  // ---- everything passed: the rows, the histories, the accumulators (their sum on rank 0, 0 elsewhere), the operator
  unsigned long long tot[3] = {0, 0, 0};  // kept rows, rows of other ranks, kept entries
  if (job.total_rows > 0 || job.merged[kScScal2] != 0 || job.merged[kScScal3] != 0)
    COOC_TRY(install_rows_parts(ctx, job, t, tot));
  int64_t hist_items = 0;
  if (!kept.empty()) COOC_TRY(install_histories_parts(ctx, job, t, kept, &hist_items));
  int64_t *merged = job.merged;
  if (job.rank != 0) merged[kScObservedExact] = merged[kScRowsumAcc] = merged[kScRescoredItems] = merged[kScLateElements] = 0;
  if (job.world == 1) merged[kScAgreed] = INT64_MIN;
  set_operator(ctx, merged, pend);

  // ---- what cooc_snapshot_prepare would report right now
  SnapCounts c;
  c.users = int64_t(kept.size());
  c.hist_items = hist_items;
  c.rows = int64_t(tot[0]);
  c.entries = int64_t(tot[2]);
  c.xsums = job.world > 1 ? int64_t(tot[1]) : 0;
  c.pend_windows = int64_t(pend.ts.size());
  c.pend_records = int64_t(pend.users.size());
  snap_info(header_for(ctx, c), info);
  return Status::Ok();
}

// Every part alone: the whole validation of cooc_restore_finish but its (rank, world).  Then across parts, from
// headers and scalars (host-only: cooc_snapshot.cpp).
Status Snapshotter::validate_parts(cooc_ctx &ctx, PartsJob *job) {
  const int32_t M = ctx.cfg.n_items;
  const int32_t W = int32_t(ctx.restore_part_len.size());
  const char *img = ctx.restore_img.as<char>();
  job->parts.resize(W);
  std::vector<SnapPartHead> heads(W);
  for (int32_t i = 0; i < W; i++) {
    Parsed &p = job->parts[i];
    Status v = validate(ctx, img + ctx.restore_part_off[i], ctx.restore_part_len[i], false, &p);
    if (!v.ok()) return Status{v.code, "part " + std::to_string(i) + ": " + v.msg};
    heads[i].h = p.h;
    std::copy(p.scalars.begin(), p.scalars.end(), heads[i].scalars);
    heads[i].first_pending = p.pend.ts.empty() ? INT64_MAX : p.pend.ts[0];
    job->views.push_back(BlobView{&p.h, img + ctx.restore_part_off[i]});
  }
  std::string why;
  if (snap_check_parts(heads.data(), W, M, ctx.cfg.window_size_ms, ctx.cfg.user_cut, job->merged, &why) != COOC_OK)
    return Status{COOC_ERR_ARG, why};
  for (const BlobView &v : job->views) {
    job->total_rows += v.count(kSnapRowIds);
    job->most_users = std::max(job->most_users, v.count(kSnapUserIds));
    job->most_rows = std::max(job->most_rows, v.count(kSnapRowIds));
    job->most_x = std::max(job->most_x, v.count(kSnapXsumIds));
  }
  if (job->total_rows > M) return Status{COOC_ERR_ARG, "snapshot parts: more rows than items"};
  return Status::Ok();
}

// the pending windows' union: within a window the kept records of part 0, then part 1, ...
PendingWindows Snapshotter::pending_union(const PartsJob &job) {
  std::map<int64_t, Operator::Pending> pend;
  for (const Parsed &p : job.parts)
    for (size_t k = 0; k < p.pend.ts.size(); k++)
      for (int64_t e = p.pend.ptr[k]; e < p.pend.ptr[k + 1]; e++)
        if (job.keeps(p.pend.users[e])) {
          Operator::Pending &w = pend[p.pend.ts[k]];
          w.users.push_back(p.pend.users[e]);
          w.items.push_back(p.pend.items[e]);
        }
  return flatten(pend);
}

// The global rows a mod world == rank in this context's representation, every item's job-wide row sum, the
// job-wide totals; tot = kept rows, rows of other ranks, kept entries.
Status Snapshotter::install_rows_parts(cooc_ctx &ctx, const PartsJob &job, const RowTables &t, unsigned long long *tot) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  COOC_TRY(st.ensure_global(ctx));  // (zeroed)
  int32_t *klen = st.sparse_global_ ? st.gs_.len.as<int32_t>() : t.klen;
  k_snap_keep_rows<<<std::min<unsigned>(blocks_for(M, 256), 512), 256, 0, s>>>(M, job.world, job.rank, t.owner, t.len, klen,
                                                                               t.ctl->tot);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(st.d_grs_.p, t.grs, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(tot, t.ctl->tot, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  const int64_t nnz = int64_t(tot[2]);
  if (st.sparse_global_) {
    COOC_TRY(lay_out_slabs(ctx, nnz));
    if (nnz > 0) {
      int64_t n_chunks = 0, serr = 0;
      COOC_HIP_TRY(hipMemsetAsync(t.pre, 0, sizeof(int64_t), s));
      COOC_TRY(launch_scan_ws<true>(ScanChunksI32{klen}, t.pre + 1, M, t.scan, &serr, s));
      COOC_HIP_TRY(hipMemcpyAsync(&n_chunks, t.pre + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if ((serr & 8) || n_chunks < 1 || n_chunks > nnz)
        return Status{COOC_ERR_STATE, "internal bounds check failed (rescaled rows' pieces)"};
      k_snap_copy_parts<true><<<wave_grid(n_chunks), 256, 0, s>>>(M, n_chunks, t.pre, t.owner, t.off, st.gs_.base.as<int64_t>(),
                                                                  klen, t.src[0], t.src[1], st.gs_.col.as<uint32_t>(),
                                                                  st.gs_.cnt.as<uint32_t>());
      COOC_HIP_TRY(hipGetLastError());
    }
  } else if (nnz > 0) {
    k_snap_scatter_dense_parts<<<wave_grid(M), 256, 0, s>>>(M, t.views, t.owner, t.off, klen, st.d_global_.as<uint32_t>());
    COOC_HIP_TRY(hipGetLastError());
  }
  return upload_running_totals(ctx, job.merged[kScScal2], job.merged[kScScal3]);
}

// the kept histories, in user order, from whichever part holds them
Status Snapshotter::install_histories_parts(cooc_ctx &ctx, const PartsJob &job, const RowTables &t,
                                            const std::vector<KeptUser> &kept, int64_t *hist_items) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const size_t n = kept.size();
  std::vector<int32_t> user_ids(n), l_part(n), l_len(n);
  std::vector<int64_t> lens(n), aoff, l_soff(n), l_ptr(n + 1, 0);
  for (size_t j = 0; j < n; j++) {
    const std::vector<int64_t> &hp = job.parts[kept[j].part].hist_ptr;
    user_ids[j] = kept[j].user;
    l_part[j] = kept[j].part;
    l_soff[j] = hp[kept[j].idx];
    lens[j] = hp[kept[j].idx + 1] - hp[kept[j].idx];
    l_len[j] = int32_t(lens[j]);
    l_ptr[j + 1] = l_ptr[j] + lens[j];
  }
  *hist_items = l_ptr[n];
  COOC_TRY(lay_out_histories(ctx, lens, &aoff));
  const std::vector<int64_t> chunk_pre = chunk_prefix(l_ptr);
  Carve c;  // (the users' scratch is done with)
  const auto o_pre = c.take<int64_t>(n + 1), o_soff = c.take<int64_t>(n), o_doff = c.take<int64_t>(n);
  const auto o_part = c.take<int32_t>(n), o_hlen = c.take_last<int32_t>(n);
  DevBuf &b = ctx.snap_tmp2;
  COOC_TRY(b.reserve(c.end));
  COOC_HIP_TRY(hipMemcpyAsync(o_pre.in(b), chunk_pre.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(o_soff.in(b), l_soff.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(o_doff.in(b), aoff.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(o_part.in(b), l_part.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(o_hlen.in(b), l_len.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  k_snap_copy_parts<false><<<wave_grid(chunk_pre[n]), 256, 0, s>>>(int64_t(n), chunk_pre[n], o_pre.in(b), o_part.in(b),
                                                                   o_soff.in(b), o_doff.in(b), o_hlen.in(b), t.src[2], nullptr,
                                                                   st.arena_.as<uint32_t>(), nullptr);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipStreamSynchronize(s));  // (the uploads read this function's vectors)
  set_slots(st, user_ids, lens, aoff);
  return Status::Ok();
}

}  // namespace cooc
