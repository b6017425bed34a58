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
//   rescale  cooc_restore_begin_parts .. _finish_parts: ALL blobs of one checkpoint (one per old subtask) into
//            this context's (rank, world).  All parts are resident on the device at once, so a restoring rank
//            needs memory for the whole job's blobs next to its own share of the state.
//            k_snap_keep_users + select_flagged        the users the route keeps, per part
//            k_snap_parts_rows / _xsums / k_snap_keep_rows   M-sized tables of the job's rows (owner part, offset,
//                                length, job-wide row sum), the cross-part checks, the rows this rank keeps
//            k_snap_copy_parts   kept rows / histories from the W_old images to the slabs / the arena (2,048
//                                elements per wave, 16-B accesses where both sides sit alike)
//            k_snap_scatter_dense_parts   kept rows into the dense matrix
//   sampled  a sampled context's blob is format 2 (cooc_snapshot.h): the same code with five more sections
//            ScanLiveU32 + k_snap_live_rows + k_snap_compact   slab entries whose count went back to 0 dropped
//            k_snap_count_flags + select_flagged + k_snap_gather_counts / k_snap_gather_totals   the device
//                                sampler's non-zero item counters and the users' totals, in id order
//            k_snap_val_i16 / k_snap_val_totals   counters in 1..item_cut; every history's user has a total at
//                                least its length, and the length is at most user_cut
//            k_snap_scatter_counts / _totals / _lens   the device sampler's arrays from the blob
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

// sums[k] (device, kSnapSectionsMax words) = the checksum of section k of the image, k < h.n_sections
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

inline unsigned wave_grid(int64_t n_waves) { return std::min<unsigned>(blocks_for(n_waves * 64, 256), 8192); }

// chunk_pre[j] = pieces of the lists before j (host), from the lists' offsets
std::vector<int64_t> chunk_prefix(const std::vector<int64_t> &ptr) {
  std::vector<int64_t> pre(ptr.size(), 0);
  for (size_t j = 0; j + 1 < ptr.size(); j++) pre[j + 1] = pre[j] + (ptr[j + 1] - ptr[j] + kListChunk - 1) / kListChunk;
  return pre;
}

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

}  // namespace

// The one place that reads and writes the private state of StreamState and Operator for a checkpoint.
struct Snapshotter {
  static Status prepare(cooc_ctx &ctx, cooc_snapshot_info *info);
  static Status copy(cooc_ctx &ctx, int64_t offset, int64_t n, uint8_t *out);
  static Status restore_begin(cooc_ctx &ctx, int64_t bytes);
  static Status restore_write(cooc_ctx &ctx, int64_t offset, int64_t n, const uint8_t *src);
  static Status restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info);

  static Status restore_begin_parts(cooc_ctx &ctx, int32_t n_parts, const int64_t *bytes);
  static Status restore_write_part(cooc_ctx &ctx, int32_t part, int64_t offset, int64_t n, const uint8_t *src);
  static Status restore_finish_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info);

 private:
  // one validated blob: its header and the sections that become host state
  struct Parsed {
    SnapHeader h;
    std::vector<int64_t> scalars, hist_ptr, pend_ts, pend_ptr;
    std::vector<int32_t> user_ids, pend_users, pend_items;
    // format 2: the sampler's scalars, the users with a total and their totals, the counted items and counters
    std::vector<int64_t> smp_scalars;
    std::vector<int32_t> tot_ids, totals, cnt_ids;
    std::vector<int16_t> cnts;
  };
  // the blob format of this context: 2 when sampled, else 1
  static int32_t format_of(const cooc_ctx &ctx) { return ctx.stream_state.sampled() ? kSnapFormatSampled : kSnapFormat; }
  static Status reset_samplers(cooc_ctx &ctx);
  static Status install_samplers(cooc_ctx &ctx, const char *img, const Parsed &p);
  static bool empty_state(const cooc_ctx &ctx);
  static void wipe(cooc_ctx &ctx);
  static void drop_restore(cooc_ctx &ctx);
  static Status validate(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, Parsed *out);
  static Status install(cooc_ctx &ctx, const char *img, const Parsed &p);
  static Status validate_and_install_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info);
  // the pieces of an install that the plain and the parts path share
  static Status lay_out_slabs(cooc_ctx &ctx, int64_t nnz);
  static Status lay_out_histories(cooc_ctx &ctx, const std::vector<int64_t> &lens, std::vector<int64_t> *aoff);
  static void set_slots(StreamState &st, const std::vector<int32_t> &user_ids, const std::vector<int64_t> &lens,
                        const std::vector<int64_t> &aoff);
  static void set_operator(cooc_ctx &ctx, const int64_t *scalars, const std::vector<int64_t> &pend_ts,
                           const std::vector<int64_t> &pend_ptr, const std::vector<int32_t> &pend_users,
                           const std::vector<int32_t> &pend_items);
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
  // A sampled context's blob also names every user with a total (a superset: a user whose every record was
  // rejected at the item cut has no history).  The host sampler's totals are read here; the device sampler's are
  // gathered on the device below, where every slot has one (a slot is made for a record of a finished window).
  const bool sampled = st.sampled(), dev_sampled = st.dev_sampler_.enabled();
  const int32_t format = format_of(ctx);
  if (dev_sampled && (!st.dev_sampler_.count_.p || !st.dev_sampler_.ctr_.p))
    return Status{COOC_ERR_STATE, "the device sampler's state was released and not re-created"};
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
  std::vector<int32_t> tot_ids(n_tot), tot_slots(n_tot), totals;
  for (int64_t j = 0; j < n_tot; j++) {
    tot_ids[j] = tot_users[j].first;
    tot_slots[j] = tot_users[j].second;
  }
  std::vector<int32_t> cnt_ids;  // host sampler: the items with a counter, and the counters
  std::vector<int16_t> cnts;
  if (sampled && !dev_sampled) {
    totals.resize(n_tot);
    for (int64_t j = 0; j < n_tot; j++) totals[j] = st.sampler_.total(tot_slots[j]);
    for (int32_t i = 0; i < M; i++)
      if (st.sampler_.item_count(i) != 0) {
        cnt_ids.push_back(i);
        cnts.push_back(st.sampler_.item_count(i));
      }
  }
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
  const size_t o_cids = o_sel + al256(select_tmp_bytes(M)), o_tmp_end = o_cids + al256(sizeof(int32_t) * size_t(M));
  char *tmp = nullptr;
  const int64_t *rp = nullptr;
  const int64_t *live = nullptr;  // sampled slabs: the live entries before each packed entry
  int64_t n_packed = 0;           // ... and the packed entries, dead ones included
  if (st.global_ready_ || dev_sampled) {
    COOC_TRY(ctx.snap_tmp.reserve(o_tmp_end));
    tmp = ctx.snap_tmp.as<char>();
  }
  if (st.global_ready_) {
    const int32_t *lens = nullptr;
    if (st.sparse_global_) {  // (synchronises s)
      COOC_TRY(launch_pack_rows(s, M, st.gs_.base.as<int64_t>(), st.gs_.len.as<int32_t>(), st.gs_.col.as<int32_t>(),
                                st.gs_.cnt.as<uint32_t>(), ctx.snap_rp, ctx.snap_col, ctx.snap_cnt, st.d_scan_tmp_, &nnz));
      lens = st.gs_.len.as<int32_t>();
      if (sampled && nnz > 0) {
        // entries whose count went back to 0 are no keys: flagged, scanned, and the rows recounted without them
        n_packed = nnz;
        const size_t o_len = al256(sizeof(int64_t) * (size_t(M) + 1)), o_live = o_len + al256(sizeof(int32_t) * size_t(M));
        COOC_TRY(ctx.snap_live.reserve(o_live + sizeof(int64_t) * size_t(n_packed + 1)));
        COOC_TRY(st.d_scan_tmp_.reserve(scan_ws_bytes(n_packed + 1)));
        int64_t *d_rp2 = ctx.snap_live.as<int64_t>();
        int32_t *d_len2 = reinterpret_cast<int32_t *>(ctx.snap_live.as<char>() + o_len);
        int64_t *d_live = reinterpret_cast<int64_t *>(ctx.snap_live.as<char>() + o_live);
        int64_t serr = 0;
        COOC_TRY(launch_scan_ws<false>(ScanLiveU32{ctx.snap_cnt.as<uint32_t>(), n_packed}, d_live, n_packed + 1,
                                       st.d_scan_tmp_.as<unsigned long long>(), &serr, s));
        k_snap_live_rows<<<blocks_for(int64_t(M) + 1, 256), 256, 0, s>>>(M, ctx.snap_rp.as<int64_t>(), d_live, d_rp2, d_len2);
        COOC_HIP_TRY(hipGetLastError());
        COOC_HIP_TRY(hipMemcpyAsync(&nnz, d_live + n_packed, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        COOC_HIP_TRY(hipStreamSynchronize(s));
        if ((serr & 8) || nnz < 0 || nnz > n_packed)
          return Status{COOC_ERR_STATE, "internal bounds check failed (snapshot live entries)"};
        live = d_live;
        rp = d_rp2;
        lens = d_len2;
      }
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
    if (!rp) rp = ctx.snap_rp.as<int64_t>();
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
  // the device sampler's counted items (the row flags are done with)
  int64_t n_cnt = int64_t(cnt_ids.size());
  if (dev_sampled) {
    uint8_t *flag = reinterpret_cast<uint8_t *>(tmp + o_flag);
    int32_t *d_nsel = reinterpret_cast<int32_t *>(tmp + o_nsel);
    int32_t n_sel_c = 0;
    k_snap_count_flags<<<blocks_for(M, 256), 256, 0, s>>>(M, st.dev_sampler_.count_.as<int32_t>(), flag);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemsetAsync(d_nsel + 2, 0, sizeof(int32_t), s));
    COOC_TRY(select_flagged(flag, M, reinterpret_cast<int32_t *>(tmp + o_cids), d_nsel + 2, tmp + o_sel, s));
    COOC_HIP_TRY(hipMemcpyAsync(&n_sel_c, d_nsel + 2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (n_sel_c < 0 || n_sel_c > M) return Status{COOC_ERR_STATE, "internal bounds check failed (counted items)"};
    n_cnt = n_sel_c;
  }

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
  if (sampled) {
    sec(kSnapSmpScalars).count = kSnapSmpScalarWords;
    sec(kSnapSmpItemIds).count = sec(kSnapSmpItemCnts).count = n_cnt;
    sec(kSnapSmpUserIds).count = sec(kSnapSmpTotals).count = n_tot;
  }
  snap_layout(&h, format);
  h.n_items = M;
  h.user_cut = ctx.cfg.user_cut;
  h.window_size_ms = ctx.cfg.window_size_ms;
  h.rank = ctx.comm ? ctx.comm->rank() : 0;
  h.world = ctx.comm ? ctx.comm->world() : 1;
  COOC_TRY(ctx.snap_img.reserve(size_t(h.total_bytes)));
  char *img = ctx.snap_img.as<char>();
  auto at = [&](int kind) { return img + sec(kind).offset; };
  for (int k = 1; k <= h.n_sections; k++)  // the pad of a section whose bytes are no multiple of 8
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

  // ---- the sampler's state: from the host sampler's vectors, or gathered from the device sampler's arrays
  if (sampled) {
    int64_t ctr[6] = {0, 0, 0, 0, 0, 0};
    COOC_TRY(st.sampling_counters(ctx, ctr));  // (synchronises s in device mode)
    int64_t smp[kSnapSmpScalarWords] = {0};
    smp[kSsItemCut] = st.sampler_.item_cut();
    smp[kSsSeed] = int64_t(st.sampler_.seed());
    smp[kSsRejected] = ctr[0];
    smp[kSsFills] = ctr[1];
    smp[kSsReplacements] = ctr[2];
    smp[kSsFeedbacks] = ctr[3];
    COOC_TRY(put(kSnapSmpScalars, smp));
    COOC_TRY(put(kSnapSmpUserIds, tot_ids.data()));
    if (!dev_sampled) {
      COOC_TRY(put(kSnapSmpItemIds, cnt_ids.data()));
      COOC_TRY(put(kSnapSmpItemCnts, cnts.data()));
      COOC_TRY(put(kSnapSmpTotals, totals.data()));
      COOC_HIP_TRY(hipStreamSynchronize(s));  // (the uploads read this function's vectors)
    } else {
      const int32_t *cids = reinterpret_cast<const int32_t *>(tmp + o_cids);
      if (n_cnt > 0) {
        COOC_HIP_TRY(hipMemcpyAsync(at(kSnapSmpItemIds), cids, sizeof(int32_t) * size_t(n_cnt), hipMemcpyDeviceToDevice, s));
        k_snap_gather_counts<<<blocks_for(n_cnt, 256), 256, 0, s>>>(n_cnt, cids, st.dev_sampler_.count_.as<int32_t>(),
                                                                    reinterpret_cast<int16_t *>(at(kSnapSmpItemCnts)));
        COOC_HIP_TRY(hipGetLastError());
      }
      if (n_tot > 0) {
        // the (id-sorted user -> slot) table up, the totals gathered by slot
        COOC_TRY(ctx.snap_tmp2.reserve(sizeof(int32_t) * size_t(n_tot) + 256));
        int32_t *d_slots = ctx.snap_tmp2.as<int32_t>();
        unsigned int *d_terr = reinterpret_cast<unsigned int *>(ctx.snap_tmp2.as<char>() + al256(sizeof(int32_t) * size_t(n_tot)));
        unsigned int terr = 0;
        COOC_HIP_TRY(hipMemcpyAsync(d_slots, tot_slots.data(), sizeof(int32_t) * size_t(n_tot), hipMemcpyHostToDevice, s));
        COOC_HIP_TRY(hipMemsetAsync(d_terr, 0, sizeof(unsigned int), s));
        k_snap_gather_totals<<<blocks_for(n_tot, 256), 256, 0, s>>>(n_tot, d_slots, st.dev_sampler_.total_.as<int32_t>(),
                                                                    st.dev_sampler_.slot_cap_,
                                                                    reinterpret_cast<int32_t *>(at(kSnapSmpTotals)), d_terr, 1u);
        COOC_HIP_TRY(hipGetLastError());
        COOC_HIP_TRY(hipMemcpyAsync(&terr, d_terr, sizeof(terr), hipMemcpyDeviceToHost, s));
        COOC_HIP_TRY(hipStreamSynchronize(s));
        if (terr) return Status{COOC_ERR_STATE, "internal error: a user slot without a total on the device sampler"};
      }
    }
  }

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
      if (live) {
        k_snap_compact<<<std::min<unsigned>(blocks_for(n_packed, 256 * 4), 4096), 256, 0, s>>>(
            n_packed, live, ctx.snap_col.as<int32_t>(), ctx.snap_cnt.as<uint32_t>(),
            reinterpret_cast<int32_t *>(at(kSnapRowCols)), reinterpret_cast<uint32_t *>(at(kSnapRowCnts)));
        COOC_HIP_TRY(hipGetLastError());
      } else if (st.sparse_global_) {
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
  COOC_TRY(ctx.snap_sums.reserve(sizeof(unsigned long long) * kSnapSectionsMax + sizeof(unsigned int) * 2));
  COOC_TRY(launch_checksums(s, img, h, ctx.snap_sums.as<unsigned long long>()));
  unsigned long long sums[kSnapSectionsMax];
  COOC_HIP_TRY(hipMemcpyAsync(sums, ctx.snap_sums.p, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < h.n_sections; k++) h.sec[k].sum = sums[k];
  snap_seal(&h);
  COOC_HIP_TRY(hipMemcpyAsync(img, &h, size_t(snap_header_bytes(h.n_sections)), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
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

// The whole validation of one untrusted blob of `bytes` bytes at img (device); own_rank: it must also have been
// taken by this context's (rank, world).
Status Snapshotter::validate(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, Parsed *out) {
  hipStream_t s = ctx.stream;
  // 1. header and directory (the host-only code of cooc_snapshot_inspect)
  const int32_t format = format_of(ctx);
  const bool sampled = format == kSnapFormatSampled;
  uint8_t hdr[sizeof(SnapHeader)];
  const int64_t hdr_bytes = snap_header_bytes(snap_sections_of(format));
  if (bytes < hdr_bytes) return Status{COOC_ERR_ARG, "snapshot blob: shorter than its header"};
  COOC_HIP_TRY(hipMemcpy(hdr, img, size_t(hdr_bytes), hipMemcpyDeviceToHost));
  SnapHeader &h = out->h;
  std::string why;
  if (snap_parse(hdr, bytes, &h, &why, format) != COOC_OK) return Status{COOC_ERR_ARG, why};
  const int32_t M = ctx.cfg.n_items;
  if (h.n_items != M || h.window_size_ms != ctx.cfg.window_size_ms || h.user_cut != ctx.cfg.user_cut)
    return Status{COOC_ERR_ARG, "snapshot blob: taken with n_items " + std::to_string(h.n_items) + ", window " +
                                    std::to_string(h.window_size_ms) + " ms, user_cut " + std::to_string(h.user_cut) +
                                    "; this context has " + std::to_string(M) + ", " +
                                    std::to_string(ctx.cfg.window_size_ms) + " ms, " + std::to_string(ctx.cfg.user_cut)};
  const int32_t rank = ctx.comm ? ctx.comm->rank() : 0, world = ctx.comm ? ctx.comm->world() : 1;
  if (own_rank && (h.rank != rank || h.world != world))
    return Status{COOC_ERR_ARG, "snapshot blob: taken by rank " + std::to_string(h.rank) + " of " + std::to_string(h.world) +
                                    "; this context is rank " + std::to_string(rank) + " of " + std::to_string(world)};
  auto sec = [&](int kind) -> const SnapSection & { return h.sec[kind - 1]; };
  auto at = [&](int kind) { return img + sec(kind).offset; };
  const int64_t n_users = sec(kSnapUserIds).count, n_hist = sec(kSnapHistItems).count, R = sec(kSnapRowIds).count;
  const int64_t nnz = sec(kSnapRowCols).count, X = sec(kSnapXsumIds).count, P = sec(kSnapPendTs).count;
  const int64_t n_pend = sec(kSnapPendUsers).count;
  if (h.world == 1 && X > 0) return Status{COOC_ERR_ARG, "snapshot blob: row sums of other ranks without a communicator"};

  // 2. the sections' checksums
  COOC_TRY(ctx.snap_sums.reserve(sizeof(unsigned long long) * kSnapSectionsMax + sizeof(unsigned int) * 2));
  unsigned long long *d_sums = ctx.snap_sums.as<unsigned long long>();
  unsigned int *d_err = reinterpret_cast<unsigned int *>(d_sums + kSnapSectionsMax);
  COOC_TRY(launch_checksums(s, img, h, d_sums));
  unsigned long long sums[kSnapSectionsMax];
  COOC_HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < h.n_sections; k++)
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
  // format 2: the sampler's scalars first (item_cut bounds the counters' check; the cuts and the seed are the
  // context's own)
  const int64_t n_cnt = sampled ? sec(kSnapSmpItemIds).count : 0, n_tot = sampled ? sec(kSnapSmpUserIds).count : 0;
  if (sampled) {
    out->smp_scalars.assign(kSnapSmpScalarWords, 0);
    COOC_HIP_TRY(hipMemcpy(out->smp_scalars.data(), at(kSnapSmpScalars), sizeof(int64_t) * kSnapSmpScalarWords,
                           hipMemcpyDeviceToHost));
    const int64_t *sc = out->smp_scalars.data();
    if (snap_check_sampler_scalars(sc, &why) != COOC_OK) return Status{COOC_ERR_ARG, why};
    const Sampler &smp = ctx.stream_state.sampler_;
    if (sc[kSsItemCut] != smp.item_cut() || uint64_t(sc[kSsSeed]) != smp.seed())
      return Status{COOC_ERR_ARG, "snapshot blob: taken with item_cut " + std::to_string(sc[kSsItemCut]) + ", seed " +
                                      std::to_string(sc[kSsSeed]) + "; this context has " + std::to_string(smp.item_cut()) +
                                      ", " + std::to_string(int64_t(smp.seed()))};
    if (h.world != 1) return Status{COOC_ERR_ARG, "snapshot blob: a sampled context is single-subtask"};
  }
  COOC_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned int) * 2, s));
  if (sampled) {
    const int32_t *d_cids = reinterpret_cast<const int32_t *>(at(kSnapSmpItemIds));
    const int32_t *d_tids = reinterpret_cast<const int32_t *>(at(kSnapSmpUserIds));
    k_snap_val_ids<<<blocks_for(n_cnt, 256), 256, 0, s>>>(d_cids, n_cnt, true, M, d_err, 256u);
    k_snap_val_i16<<<range_grid(n_cnt), 256, 0, s>>>(reinterpret_cast<const int16_t *>(at(kSnapSmpItemCnts)), n_cnt, 1,
                                                     int32_t(out->smp_scalars[kSsItemCut]), d_err, 512u);
    k_snap_val_ids<<<blocks_for(n_tot, 256), 256, 0, s>>>(d_tids, n_tot, false, 0, d_err, 1024u);
    k_snap_val_range<<<range_grid(n_tot), 256, 0, s>>>(reinterpret_cast<const uint32_t *>(at(kSnapSmpTotals)), n_tot, 1u,
                                                       uint64_t(1) << 31, d_err, 2048u);
  }
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
                                    "32 columns, 64 counts, 128 row-sum ids, 256 counted items, 512 item counters, "
                                    "1024 users with a total, 2048 totals)"};
  k_snap_val_rows<<<wave_grid(R), 256, 0, s>>>(R, d_rptr, d_col, d_cnt, d_rsum, d_err + 1, 1u);
  if (sampled)  // the histories' users against the users with a total (both id lists have passed)
    k_snap_val_totals<<<blocks_for(n_users, 256), 256, 0, s>>>(d_uids, n_users, d_hptr,
                                                               reinterpret_cast<const int32_t *>(at(kSnapSmpUserIds)), n_tot,
                                                               reinterpret_cast<const int32_t *>(at(kSnapSmpTotals)),
                                                               ctx.cfg.user_cut, d_err + 1, 2u);
  COOC_HIP_TRY(hipGetLastError());
  // the sections that become host state
  std::vector<int64_t> &scalars = out->scalars, &hist_ptr = out->hist_ptr, &pend_ts = out->pend_ts, &pend_ptr = out->pend_ptr;
  std::vector<int32_t> &user_ids = out->user_ids, &pend_users = out->pend_users, &pend_items = out->pend_items;
  scalars.assign(kSnapScalarWords, 0);
  hist_ptr.assign(n_users + 1, 0);
  pend_ts.assign(P, 0);
  pend_ptr.assign(P + 1, 0);
  user_ids.assign(n_users, 0);
  pend_users.assign(n_pend, 0);
  pend_items.assign(n_pend, 0);
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
  if (sampled) {
    out->tot_ids.assign(n_tot, 0);
    out->totals.assign(n_tot, 0);
    out->cnt_ids.assign(n_cnt, 0);
    out->cnts.assign(n_cnt, 0);
    COOC_TRY(get(kSnapSmpUserIds, out->tot_ids.data()));
    COOC_TRY(get(kSnapSmpTotals, out->totals.data()));
    COOC_TRY(get(kSnapSmpItemIds, out->cnt_ids.data()));
    COOC_TRY(get(kSnapSmpItemCnts, out->cnts.data()));
  }
  COOC_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err[1] & 1u)
    return Status{COOC_ERR_ARG, "snapshot blob: a global row's columns are not strictly ascending or its counts do "
                                "not sum to its row sum"};
  if (err[1] & 2u)
    return Status{COOC_ERR_ARG, "snapshot blob: a user with a history has no total, a total below its history's "
                                "length, or a history longer than user_cut"};
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
  return Status::Ok();
}

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

// accumulators and the operator
void Snapshotter::set_operator(cooc_ctx &ctx, const int64_t *scalars, const std::vector<int64_t> &pend_ts,
                               const std::vector<int64_t> &pend_ptr, const std::vector<int32_t> &pend_users,
                               const std::vector<int32_t> &pend_items) {
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
  for (size_t k = 0; k < pend_ts.size(); k++) {
    Operator::Pending &p = op.pending_[pend_ts[k]];
    p.users.assign(pend_users.begin() + pend_ptr[k], pend_users.begin() + pend_ptr[k + 1]);
    p.items.assign(pend_items.begin() + pend_ptr[k], pend_items.begin() + pend_ptr[k + 1]);
  }
}

Status Snapshotter::install(cooc_ctx &ctx, const char *img, const Parsed &p) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const SnapHeader &h = p.h;
  const std::vector<int64_t> &scalars = p.scalars, &hist_ptr = p.hist_ptr;
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
      COOC_TRY(lay_out_slabs(ctx, nnz));
      if (nnz > 0) {
        COOC_HIP_TRY(hipMemcpyAsync(st.gs_.col.p, col, sizeof(int32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
        COOC_HIP_TRY(hipMemcpyAsync(st.gs_.cnt.p, cnt, sizeof(uint32_t) * size_t(nnz), hipMemcpyDeviceToDevice, s));
      }
    } else if (R > 0) {
      k_snap_scatter_dense<<<wave_grid(R), 256, 0, s>>>(R, M, ids, rp, col, cnt, st.d_global_.as<uint32_t>());
      COOC_HIP_TRY(hipGetLastError());
    }
    int64_t scal[8] = {0, 0, scalars[kScScal2], scalars[kScScal3], 0, 0, 0, 0};
    COOC_HIP_TRY(hipMemcpyAsync(st.d_scal_.p, scal, sizeof(scal), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }

  // ---- histories: a fresh arena, every list at finish()'s own first capacity; the slot tables in user order
  std::vector<int64_t> hist_lens, hist_aoff;
  if (n_users > 0) {
    std::vector<int64_t> lens(n_users), aoff;
    for (int64_t j = 0; j < n_users; j++) lens[j] = hist_ptr[j + 1] - hist_ptr[j];
    COOC_TRY(lay_out_histories(ctx, lens, &aoff));
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
    // (format 2: the slot tables are made below, over every user with a total)
    if (h.format != kSnapFormatSampled) set_slots(st, p.user_ids, lens, aoff);
    else hist_lens = std::move(lens), hist_aoff = std::move(aoff);
  }
  if (h.format == kSnapFormatSampled) {
    // the slot tables in user order over every user with a total; those with a history (a subset, both lists
    // ascending) get it
    size_t j = 0;
    for (size_t t = 0; t < p.tot_ids.size(); t++) {
      const int32_t slot = st.slot_for(p.tot_ids[t]);
      if (j < p.user_ids.size() && p.user_ids[j] == p.tot_ids[t]) {
        st.h_off_[slot] = hist_aoff[j];
        st.h_len_[slot] = int32_t(hist_lens[j]);
        st.h_cap_[slot] = int32_t(std::max<int64_t>(16, hist_lens[j]));
        j++;
      }
    }
    if (j != p.user_ids.size()) return Status{COOC_ERR_STATE, "internal error: a restored history without a total"};
    COOC_TRY(install_samplers(ctx, img, p));
  }
  set_operator(ctx, scalars.data(), p.pend_ts, p.pend_ptr, p.pend_users, p.pend_items);
  return Status::Ok();
}

// The samplers' state of a validated format-2 blob, after the slot tables: the host sampler's vectors, or the
// device sampler's arrays scattered on the device (its per-slot arrays grown to the restored slots first).
Status Snapshotter::install_samplers(cooc_ctx &ctx, const char *img, const Parsed &p) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const SnapHeader &h = p.h;
  auto sec = [&](int kind) -> const SnapSection & { return h.sec[kind - 1]; };
  auto at = [&](int kind) { return img + sec(kind).offset; };
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
    k_snap_scatter_counts<<<blocks_for(n_cnt, 256), 256, 0, s>>>(n_cnt, reinterpret_cast<const int32_t *>(at(kSnapSmpItemIds)),
                                                                 reinterpret_cast<const int16_t *>(at(kSnapSmpItemCnts)),
                                                                 d.count_.as<int32_t>());
  if (n_tot > 0) {
    COOC_TRY(ctx.snap_tmp2.reserve(sizeof(int32_t) * size_t(n_tot)));
    int32_t *d_slots = ctx.snap_tmp2.as<int32_t>();
    COOC_HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), sizeof(int32_t) * size_t(n_tot), hipMemcpyHostToDevice, s));
    const int32_t *d_tids = reinterpret_cast<const int32_t *>(at(kSnapSmpUserIds));
    k_snap_scatter_totals<<<blocks_for(n_tot, 256), 256, 0, s>>>(n_tot, d_slots, reinterpret_cast<const int32_t *>(at(kSnapSmpTotals)),
                                                                 d.slot_cap_, d.total_.as<int32_t>());
    if (n_users > 0)
      k_snap_scatter_lens<<<blocks_for(n_users, 256), 256, 0, s>>>(n_users, reinterpret_cast<const int32_t *>(at(kSnapUserIds)),
                                                                   reinterpret_cast<const int64_t *>(at(kSnapHistPtr)), d_tids,
                                                                   n_tot, d_slots, d.slot_cap_, d.len_.as<int32_t>());
  }
  COOC_HIP_TRY(hipGetLastError());
  // the decision counters: [0..3] saved, [4] the users with a reservoir; the rest is recomputed when read
  int64_t ctr[8] = {sc[kSsRejected], sc[kSsFills], sc[kSsReplacements], sc[kSsFeedbacks], n_users, 0, 0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(d.ctr_.p, ctr, sizeof(ctr), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  return Status::Ok();
}

// ---- rescaling --------------------------------------------------------------------------------------------------
// All parts are resident on the device at once (restore_img, each at a 256-B aligned offset): a restoring rank
// needs memory for the whole job's blobs next to its own share of the state.
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

Status Snapshotter::validate_and_install_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info) {
  StreamState &st = ctx.stream_state;
  hipStream_t s = ctx.stream;
  const int32_t M = ctx.cfg.n_items;
  const int32_t rank = ctx.comm ? ctx.comm->rank() : 0, world = ctx.comm ? ctx.comm->world() : 1;
  const int32_t W = int32_t(ctx.restore_part_len.size());
  const char *img = ctx.restore_img.as<char>();

  // ---- the route (NULL: COOC_ROUTE_MOD)
  cooc_user_route rt{COOC_ROUTE_MOD, 0, 0, nullptr};
  if (route) rt = *route;
  if (rt.kind != COOC_ROUTE_MOD && rt.kind != COOC_ROUTE_BITMAP) return Status{COOC_ERR_ARG, "user route: unknown kind"};
  if (rt.reserved != 0) return Status{COOC_ERR_ARG, "user route: reserved field set"};
  if (rt.kind == COOC_ROUTE_BITMAP && (rt.n_bits < 0 || (rt.n_bits > 0 && !rt.bits)))
    return Status{COOC_ERR_ARG, "user route: a bitmap of n_bits > 0 needs bits"};
  if (rt.kind == COOC_ROUTE_BITMAP) rt.n_bits = std::min<int64_t>(rt.n_bits, int64_t(1) << 31);  // (user ids are int32)
  auto keeps = [&](int32_t u) {
    if (rt.kind == COOC_ROUTE_MOD) return floor_mod(u, world) == rank;
    return u >= 0 && int64_t(u) < rt.n_bits && ((rt.bits[u >> 6] >> (u & 63)) & 1ull) != 0;
  };

  // ---- 1. every part alone: the whole validation of cooc_restore_finish but its (rank, world)
  std::vector<Parsed> parts(W);
  std::vector<SnapPartHead> heads(W);
  for (int32_t i = 0; i < W; i++) {
    Status v = validate(ctx, img + ctx.restore_part_off[i], ctx.restore_part_len[i], false, &parts[i]);
    if (!v.ok()) return Status{v.code, "part " + std::to_string(i) + ": " + v.msg};
    heads[i].h = parts[i].h;
    std::copy(parts[i].scalars.begin(), parts[i].scalars.end(), heads[i].scalars);
    heads[i].first_pending = parts[i].pend_ts.empty() ? INT64_MAX : parts[i].pend_ts[0];
  }
  // ---- 2. across parts, from headers and scalars (host-only: cooc_snapshot.cpp)
  int64_t merged[kSnapScalarWords];
  std::string why;
  if (snap_check_parts(heads.data(), W, M, ctx.cfg.window_size_ms, ctx.cfg.user_cut, merged, &why) != COOC_OK)
    return Status{COOC_ERR_ARG, why};
  auto cnt_of = [&](int32_t i, int kind) { return parts[i].h.sec[kind - 1].count; };
  auto at = [&](int32_t i, int kind) { return img + ctx.restore_part_off[i] + parts[i].h.sec[kind - 1].offset; };
  int64_t total_users = 0, total_rows = 0, most_users = 0, most_rows = 0, most_x = 0;
  for (int32_t i = 0; i < W; i++) {
    total_users += cnt_of(i, kSnapUserIds);
    total_rows += cnt_of(i, kSnapRowIds);
    most_users = std::max(most_users, cnt_of(i, kSnapUserIds));
    most_rows = std::max(most_rows, cnt_of(i, kSnapRowIds));
    most_x = std::max(most_x, cnt_of(i, kSnapXsumIds));
  }
  if (total_rows > M) return Status{COOC_ERR_ARG, "snapshot parts: more rows than items"};

  // ---- 3. user ids disjoint across parts (each part's are strictly ascending)
  if (W > 1) {
    std::vector<int32_t> all;
    all.reserve(size_t(total_users));
    for (const Parsed &p : parts) all.insert(all.end(), p.user_ids.begin(), p.user_ids.end());
    std::sort(all.begin(), all.end());
    if (std::adjacent_find(all.begin(), all.end()) != all.end())
      return Status{COOC_ERR_ARG, "snapshot parts: a user id in more than one part"};
  }

  // ---- 4. the rows across parts, on the device: M-sized tables (owner part, offset, length, job-wide row sum)
  DevBuf &tbl = ctx.snap_tmp;  // (the context's scratch: no allocation per call once it has grown)
  const size_t o_owner = 0, o_len = o_owner + al256(sizeof(int32_t) * size_t(M)), o_klen = o_len + al256(sizeof(int32_t) * size_t(M));
  const size_t o_off = o_klen + al256(sizeof(int32_t) * size_t(M)), o_grs = o_off + al256(sizeof(int64_t) * size_t(M));
  const size_t o_pre = o_grs + al256(sizeof(int64_t) * size_t(M)), o_tot = o_pre + al256(sizeof(int64_t) * (size_t(M) + 1));
  const size_t o_views = o_tot + 256, o_src = o_views + al256(sizeof(PartView) * size_t(W));
  const size_t o_scan = o_src + 3 * al256(sizeof(void *) * size_t(W)), o_end = o_scan + al256(scan_ws_bytes(M));
  COOC_TRY(tbl.reserve(o_end));
  char *t = tbl.as<char>();
  int32_t *d_owner = reinterpret_cast<int32_t *>(t + o_owner), *d_len = reinterpret_cast<int32_t *>(t + o_len);
  int32_t *d_klen = reinterpret_cast<int32_t *>(t + o_klen);
  int64_t *d_off = reinterpret_cast<int64_t *>(t + o_off), *d_grs = reinterpret_cast<int64_t *>(t + o_grs);
  int64_t *d_pre = reinterpret_cast<int64_t *>(t + o_pre);
  unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(t + o_tot);  // 3 totals, then the error word
  unsigned int *d_err = reinterpret_cast<unsigned int *>(d_tot + 3);
  PartView *d_views = reinterpret_cast<PartView *>(t + o_views);
  const size_t src_stride = al256(sizeof(void *) * size_t(W));
  auto d_src = [&](int k) { return reinterpret_cast<const uint32_t *const *>(t + o_src + k * src_stride); };
  std::vector<PartView> views(W);
  std::vector<const void *> src_tab[3] = {std::vector<const void *>(W), std::vector<const void *>(W), std::vector<const void *>(W)};
  for (int32_t i = 0; i < W; i++) {
    PartView &v = views[i];
    v.row_ids = reinterpret_cast<const int32_t *>(at(i, kSnapRowIds));
    v.row_ptr = reinterpret_cast<const int64_t *>(at(i, kSnapRowPtr));
    v.row_sums = reinterpret_cast<const int64_t *>(at(i, kSnapRowSums));
    v.xsum_ids = reinterpret_cast<const int32_t *>(at(i, kSnapXsumIds));
    v.xsum_vals = reinterpret_cast<const int64_t *>(at(i, kSnapXsumVals));
    v.col = reinterpret_cast<const int32_t *>(at(i, kSnapRowCols));
    v.cnt = reinterpret_cast<const uint32_t *>(at(i, kSnapRowCnts));
    v.hist = reinterpret_cast<const int32_t *>(at(i, kSnapHistItems));
    v.R = cnt_of(i, kSnapRowIds);
    v.X = cnt_of(i, kSnapXsumIds);
    src_tab[0][i] = v.col;
    src_tab[1][i] = v.cnt;
    src_tab[2][i] = v.hist;
  }
  COOC_HIP_TRY(hipMemcpyAsync(d_views, views.data(), sizeof(PartView) * size_t(W), hipMemcpyHostToDevice, s));
  for (int k = 0; k < 3; k++)
    COOC_HIP_TRY(hipMemcpyAsync(t + o_src + k * src_stride, src_tab[k].data(), sizeof(void *) * size_t(W), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemsetAsync(d_owner, 0xFF, sizeof(int32_t) * size_t(M), s));  // -1: no part has the row
  COOC_HIP_TRY(hipMemsetAsync(d_len, 0, sizeof(int32_t) * size_t(M), s));
  COOC_HIP_TRY(hipMemsetAsync(d_off, 0, sizeof(int64_t) * size_t(M), s));
  COOC_HIP_TRY(hipMemsetAsync(d_grs, 0, sizeof(int64_t) * size_t(M), s));
  COOC_HIP_TRY(hipMemsetAsync(d_tot, 0, 256, s));
  if (most_rows > 0)
    k_snap_parts_rows<<<dim3(blocks_for(most_rows, 256), unsigned(W)), 256, 0, s>>>(d_views, W, d_owner, d_off, d_len, d_grs, d_err);
  if (most_x > 0)
    k_snap_parts_xsums<<<dim3(blocks_for(most_x, 256), unsigned(W)), 256, 0, s>>>(d_views, W, d_owner, d_grs, d_err);
  COOC_HIP_TRY(hipGetLastError());

  // ---- 5. the users the route keeps: flags per part on the device, select_flagged; the tables stay host state.
  //         Every part's ids ascend, so the parts merge pairwise into the job's users in id order, and the kept
  //         ones come out in the order a plain restore installs them.
  struct User {
    int32_t user, part, idx, keep;
  };
  std::vector<std::vector<User>> runs(W);
  {
    const size_t n_words = rt.kind == COOC_ROUTE_BITMAP ? size_t((rt.n_bits + 63) / 64) : 0;
    const size_t o_idx = al256(size_t(most_users)), o_n = o_idx + al256(sizeof(int32_t) * size_t(most_users));
    const size_t o_sel = o_n + 256, o_bits = o_sel + al256(select_tmp_bytes(most_users));
    COOC_TRY(ctx.snap_tmp2.reserve(o_bits + sizeof(uint64_t) * n_words));
    char *ub = ctx.snap_tmp2.as<char>();
    const uint64_t *d_bits = nullptr;
    if (n_words > 0) {
      COOC_HIP_TRY(hipMemcpyAsync(ub + o_bits, rt.bits, sizeof(uint64_t) * n_words, hipMemcpyHostToDevice, s));
      d_bits = reinterpret_cast<const uint64_t *>(ub + o_bits);
    }
    uint8_t *d_flag = reinterpret_cast<uint8_t *>(ub);
    int32_t *d_idx = reinterpret_cast<int32_t *>(ub + o_idx), *d_n = reinterpret_cast<int32_t *>(ub + o_n);
    std::vector<int32_t> idx;
    for (int32_t i = 0; i < W; i++) {
      const int64_t n = cnt_of(i, kSnapUserIds);
      if (n == 0) continue;
      k_snap_keep_users<<<blocks_for(n, 256), 256, 0, s>>>(reinterpret_cast<const int32_t *>(at(i, kSnapUserIds)), n, rt.kind,
                                                           world, rank, rt.n_bits, d_bits, d_flag);
      COOC_HIP_TRY(hipGetLastError());
      COOC_TRY(select_flagged(d_flag, n, d_idx, d_n, ub + o_sel, s));
      int32_t n_kept = 0;
      COOC_HIP_TRY(hipMemcpyAsync(&n_kept, d_n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (n_kept < 0 || int64_t(n_kept) > n) return Status{COOC_ERR_STATE, "internal bounds check failed (kept users)"};
      idx.resize(size_t(n_kept));
      if (n_kept > 0) COOC_HIP_TRY(hipMemcpy(idx.data(), d_idx, sizeof(int32_t) * size_t(n_kept), hipMemcpyDeviceToHost));
      std::vector<User> &run = runs[i];
      run.resize(size_t(n));
      for (int64_t j = 0; j < n; j++) run[j] = User{parts[i].user_ids[j], i, int32_t(j), 0};
      for (int32_t j : idx) {
        if (j < 0 || int64_t(j) >= n) return Status{COOC_ERR_STATE, "internal bounds check failed (kept users)"};
        run[j].keep = 1;
      }
    }
    COOC_HIP_TRY(hipStreamSynchronize(s));  // (the bitmap's upload reads the caller's memory)
  }
  while (runs.size() > 1) {
    std::vector<std::vector<User>> next;
    for (size_t i = 0; i + 1 < runs.size(); i += 2) {
      std::vector<User> m(runs[i].size() + runs[i + 1].size());
      std::merge(runs[i].begin(), runs[i].end(), runs[i + 1].begin(), runs[i + 1].end(), m.begin(),
                 [](const User &a, const User &b) { return a.user < b.user; });
      next.push_back(std::move(m));
    }
    if (runs.size() & 1) next.push_back(std::move(runs.back()));
    runs.swap(next);
  }
  std::vector<User> kept;
  for (size_t j = 0; j < runs[0].size(); j++) {
    if (j > 0 && runs[0][j - 1].user == runs[0][j].user)
      return Status{COOC_ERR_ARG, "snapshot parts: a user id in more than one part"};
    if (runs[0][j].keep) kept.push_back(runs[0][j]);
  }
  runs.clear();
  unsigned int err = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (err)
    return Status{COOC_ERR_ARG, "snapshot parts: invalid across parts (checks failed: " + std::to_string(err) +
                                    "; 1 a row in a part that does not own it, 2 a part's row sums of other ranks are "
                                    "not the other parts' rows' sums)"};

  // ---- 6. the pending windows' union: within a window the kept records of part 0, then part 1, ...
  std::map<int64_t, std::pair<std::vector<int32_t>, std::vector<int32_t>>> pend;
  for (const Parsed &p : parts)
    for (size_t k = 0; k < p.pend_ts.size(); k++)
      for (int64_t e = p.pend_ptr[k]; e < p.pend_ptr[k + 1]; e++)
        if (keeps(p.pend_users[e])) {
          auto &w = pend[p.pend_ts[k]];
          w.first.push_back(p.pend_users[e]);
          w.second.push_back(p.pend_items[e]);
        }
  std::vector<int64_t> pend_ts, pend_ptr(1, 0);
  std::vector<int32_t> pend_users, pend_items;
  for (const auto &kv : pend) {
    pend_ts.push_back(kv.first);
    pend_users.insert(pend_users.end(), kv.second.first.begin(), kv.second.first.end());
    pend_items.insert(pend_items.end(), kv.second.second.begin(), kv.second.second.end());
    pend_ptr.push_back(int64_t(pend_users.size()));
  }

  // ---- 7. everything passed: the global rows a mod world == rank in this context's representation, every
  //         item's job-wide row sum, the job-wide totals
  unsigned long long tot[3] = {0, 0, 0};  // kept rows, rows of other ranks, kept entries
  if (total_rows > 0 || merged[kScScal2] != 0 || merged[kScScal3] != 0) {
    COOC_TRY(st.ensure_global(ctx));  // (zeroed)
    int32_t *klen = st.sparse_global_ ? st.gs_.len.as<int32_t>() : d_klen;
    k_snap_keep_rows<<<std::min<unsigned>(blocks_for(M, 256), 512), 256, 0, s>>>(M, world, rank, d_owner, d_len, klen, d_tot);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemcpyAsync(st.d_grs_.p, d_grs, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    const int64_t nnz = int64_t(tot[2]);
    if (st.sparse_global_) {
      COOC_TRY(lay_out_slabs(ctx, nnz));
      if (nnz > 0) {
        int64_t n_chunks = 0, serr = 0;
        COOC_HIP_TRY(hipMemsetAsync(d_pre, 0, sizeof(int64_t), s));
        COOC_TRY(launch_scan_ws<true>(ScanChunksI32{klen}, d_pre + 1, M, reinterpret_cast<unsigned long long *>(t + o_scan), &serr, s));
        COOC_HIP_TRY(hipMemcpyAsync(&n_chunks, d_pre + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        COOC_HIP_TRY(hipStreamSynchronize(s));
        if ((serr & 8) || n_chunks < 1 || n_chunks > nnz)
          return Status{COOC_ERR_STATE, "internal bounds check failed (rescaled rows' pieces)"};
        k_snap_copy_parts<true><<<wave_grid(n_chunks), 256, 0, s>>>(M, n_chunks, d_pre, d_owner, d_off, st.gs_.base.as<int64_t>(),
                                                                    klen, d_src(0), d_src(1), st.gs_.col.as<uint32_t>(),
                                                                    st.gs_.cnt.as<uint32_t>());
        COOC_HIP_TRY(hipGetLastError());
      }
    } else if (nnz > 0) {
      k_snap_scatter_dense_parts<<<wave_grid(M), 256, 0, s>>>(M, d_views, d_owner, d_off, klen, st.d_global_.as<uint32_t>());
      COOC_HIP_TRY(hipGetLastError());
    }
    int64_t scal[8] = {0, 0, merged[kScScal2], merged[kScScal3], 0, 0, 0, 0};
    COOC_HIP_TRY(hipMemcpyAsync(st.d_scal_.p, scal, sizeof(scal), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }

  // ---- 8. the kept histories, in user order, from whichever part holds them
  const int64_t n_kept = int64_t(kept.size());
  int64_t hist_items = 0;
  if (n_kept > 0) {
    std::vector<int32_t> user_ids(n_kept), l_part(n_kept), l_len(n_kept);
    std::vector<int64_t> lens(n_kept), aoff, l_soff(n_kept), l_ptr(n_kept + 1, 0);
    for (int64_t j = 0; j < n_kept; j++) {
      const std::vector<int64_t> &hp = parts[kept[j].part].hist_ptr;
      user_ids[j] = kept[j].user;
      l_part[j] = kept[j].part;
      l_soff[j] = hp[kept[j].idx];
      lens[j] = hp[kept[j].idx + 1] - hp[kept[j].idx];
      l_len[j] = int32_t(lens[j]);
      l_ptr[j + 1] = l_ptr[j] + lens[j];
    }
    hist_items = l_ptr[n_kept];
    COOC_TRY(lay_out_histories(ctx, lens, &aoff));
    const std::vector<int64_t> chunk_pre = chunk_prefix(l_ptr);
    const size_t o_soff = al256(sizeof(int64_t) * size_t(n_kept + 1)), o_doff = o_soff + al256(sizeof(int64_t) * size_t(n_kept));
    const size_t o_part = o_doff + al256(sizeof(int64_t) * size_t(n_kept)), o_hlen = o_part + al256(sizeof(int32_t) * size_t(n_kept));
    COOC_TRY(ctx.snap_tmp2.reserve(o_hlen + sizeof(int32_t) * size_t(n_kept)));  // (the users' scratch is done with)
    char *hp = ctx.snap_tmp2.as<char>();
    COOC_HIP_TRY(hipMemcpyAsync(hp, chunk_pre.data(), sizeof(int64_t) * size_t(n_kept + 1), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(hp + o_soff, l_soff.data(), sizeof(int64_t) * size_t(n_kept), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(hp + o_doff, aoff.data(), sizeof(int64_t) * size_t(n_kept), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(hp + o_part, l_part.data(), sizeof(int32_t) * size_t(n_kept), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipMemcpyAsync(hp + o_hlen, l_len.data(), sizeof(int32_t) * size_t(n_kept), hipMemcpyHostToDevice, s));
    k_snap_copy_parts<false><<<wave_grid(chunk_pre[n_kept]), 256, 0, s>>>(
        n_kept, chunk_pre[n_kept], reinterpret_cast<const int64_t *>(hp), reinterpret_cast<const int32_t *>(hp + o_part),
        reinterpret_cast<const int64_t *>(hp + o_soff), reinterpret_cast<const int64_t *>(hp + o_doff),
        reinterpret_cast<const int32_t *>(hp + o_hlen), d_src(2), nullptr, st.arena_.as<uint32_t>(), nullptr);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipStreamSynchronize(s));
    set_slots(st, user_ids, lens, aoff);
  }

  // ---- 9. accumulators (their sum on rank 0, 0 elsewhere) and the operator
  if (rank != 0) merged[kScObservedExact] = merged[kScRowsumAcc] = merged[kScRescoredItems] = merged[kScLateElements] = 0;
  if (world == 1) merged[kScAgreed] = INT64_MIN;
  set_operator(ctx, merged, pend_ts, pend_ptr, pend_users, pend_items);

  // ---- what cooc_snapshot_prepare would report right now
  SnapHeader h;
  std::memset(&h, 0, sizeof(h));
  auto sec = [&](int kind) -> SnapSection & { return h.sec[kind - 1]; };
  sec(kSnapScalars).count = kSnapScalarWords;
  sec(kSnapUserIds).count = n_kept;
  sec(kSnapHistPtr).count = n_kept + 1;
  sec(kSnapHistItems).count = hist_items;
  sec(kSnapRowIds).count = sec(kSnapRowSums).count = int64_t(tot[0]);
  sec(kSnapRowPtr).count = int64_t(tot[0]) + 1;
  sec(kSnapRowCols).count = sec(kSnapRowCnts).count = int64_t(tot[2]);
  sec(kSnapXsumIds).count = sec(kSnapXsumVals).count = world > 1 ? int64_t(tot[1]) : 0;
  sec(kSnapPendTs).count = int64_t(pend_ts.size());
  sec(kSnapPendPtr).count = int64_t(pend_ptr.size());
  sec(kSnapPendUsers).count = sec(kSnapPendItems).count = int64_t(pend_users.size());
  snap_layout(&h);
  h.rank = rank;
  h.world = world;
  snap_info(h, info);
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
Status restore_begin_parts(cooc_ctx &ctx, int32_t n_parts, const int64_t *bytes) {
  return Snapshotter::restore_begin_parts(ctx, n_parts, bytes);
}
Status restore_write_part(cooc_ctx &ctx, int32_t part, int64_t offset, int64_t n, const uint8_t *src) {
  return Snapshotter::restore_write_part(ctx, part, offset, n, src);
}
Status restore_finish_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info) {
  return Snapshotter::restore_finish_parts(ctx, route, info);
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
