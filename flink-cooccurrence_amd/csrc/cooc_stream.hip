// cooc_stream.hip — kernels of the resident streaming state.
//
//   k_relocate / k_append   per-user history arena (NonSampled...java:129-161: userHistory.add)
//   k_merge_global          global rows += window delta rows (ItemRowRescorer...java:171-177),
//                           global row sums += row-sum deltas and the rescorer's observed total
//                           += the int view of every delta (:144-156)
//   k_gs_*                  the same merge into sparse global rows (one sorted slab per row)
//
// The rescoring of the touched rows is in cooc_rescore.hip.
#include "cooc_stream_kernels.h"
#include "cooc_radix.h"

namespace cooc {
namespace {

inline unsigned blocks_for(int64_t n, int t) { return unsigned((n + t - 1) / t); }

__global__ void k_relocate(int64_t n, const int64_t *__restrict__ reloc, int32_t *__restrict__ arena) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t r = wave; r < n; r += n_waves) {
    const int64_t src = reloc[3 * r], dst = reloc[3 * r + 1], len = reloc[3 * r + 2];
    for (int64_t i = lane; i < len; i += 64) arena[dst + i] = arena[src + i];
  }
}

__global__ void k_append(int64_t n, const int64_t *__restrict__ new_ptr, const int64_t *__restrict__ new_dst,
                         const int32_t *__restrict__ new_items, int32_t *__restrict__ arena) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = wave; j < n; j += n_waves) {
    const int64_t s = new_ptr[j], e = new_ptr[j + 1], d = new_dst[j];
    for (int64_t i = s + lane; i < e; i += 64) arena[d + (i - s)] = new_items[i];
  }
}

// Contiguous copies of arena slabs: list j (len[j] ids at off[j]) to out[dst[j] ..).  One wave per list.
__global__ void k_gather_lists(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                               const int64_t *__restrict__ dst, const int32_t *__restrict__ arena,
                               int32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = wave; j < n; j += n_waves) {
    const int64_t s = off[j], d = dst[j];
    for (int64_t i = lane; i < len[j]; i += 64) out[d + i] = arena[s + i];
  }
}

// kMax cap (UserInteractionCounter...java:168): capped length min(n_u, cut) of every user at
// lens[u + 1]; an inclusive scan of lens[1..U] gives the capped offsets.
__global__ void k_cut_lens(int64_t U, const int64_t *__restrict__ up, int32_t cut, int64_t *__restrict__ lens) {
  const int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (u < U) lens[u + 1] = min(up[u + 1] - up[u], int64_t(cut));
}

// One wave per user copies its first (capped) items; the source rows are read coalesced.
__global__ void k_cut_copy(int64_t U, const int64_t *__restrict__ up, const int32_t *__restrict__ items,
                           const int64_t *__restrict__ cut_ptr, int32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t u = wave; u < U; u += n_waves) {
    const int64_t s = up[u], d = cut_ptr[u], n = cut_ptr[u + 1] - d;
    for (int64_t i = lane; i < n; i += 64) out[d + i] = items[s + i];
  }
}

// One wave per row with a non-empty delta; the int views of the row-sum deltas are summed per
// workgroup (one global atomic per workgroup, not per row).
__global__ __launch_bounds__(256) void k_merge_global(int32_t M, const int64_t *__restrict__ row_base,
                                                      const int32_t *__restrict__ row_nnz,
                                                      const int32_t *__restrict__ col, const uint32_t *__restrict__ cnt,
                                                      const int64_t *__restrict__ rowsum_delta,
                                                      uint32_t *__restrict__ G, int64_t *__restrict__ grs,
                                                      int64_t *__restrict__ scal) {
  __shared__ int64_t s_d32[4];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  int64_t d32 = 0;
  for (int64_t a = wave; a < M; a += n_waves) {
    const int32_t n = row_nnz[a];
    if (n == 0) continue;
    const int64_t b = row_base[a];
    if (G) {  // dense global rows (sparse ones are merged by k_gs_flags / k_gs_move_all / k_gs_insert)
      uint32_t *g = G + a * int64_t(M);
      for (int32_t i = lane; i < n; i += 64) g[col[b + i]] += cnt[b + i];  // unique (a, col) per window
    }
    if (lane == 0 && rowsum_delta) {
      const int64_t d = rowsum_delta[a];
      grs[a] += d;
      d32 += int64_t(int32_t(uint32_t(uint64_t(d))));  // RowSumAggregator's int value, ItemRowRescorer...java:154
    }
  }
  if (lane == 0) s_d32[threadIdx.x >> 6] = d32;
  __syncthreads();
  if (threadIdx.x == 0 && scal) {
    const int64_t t = s_d32[0] + s_d32[1] + s_d32[2] + s_d32[3];
    if (t) atomicAdd(reinterpret_cast<unsigned long long *>(scal + 1), (unsigned long long)t);
  }
}

__global__ void k_finish_scalars(int64_t *__restrict__ scal, int64_t observed_window) {
  scal[2] += scal[1];
  scal[3] += observed_window;
}

// ---- multi-GPU windows (p > 1 subtasks, the keyBy(item) of FlinkCooccurrences.java:152): after the owner
// merged its rows' partial deltas (Sharder::merge: rows a = part + r W), the M-row view of them, their merge
// into the resident rows, every item's all-reduced row-sum delta, and the packed copy-out.
__global__ void k_own_scatter(int32_t R, int32_t W, int32_t part, const int64_t *__restrict__ mbase,
                              const int32_t *__restrict__ mnnz, int64_t *__restrict__ base, int32_t *__restrict__ nnz) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t a = int64_t(part) + int64_t(r) * W;
  base[a] = mbase[r];
  nnz[a] = mnnz[r];
}

// every item's window row sum (all-reduced: the broadcast row-sum stream, :163) into the global row sums; scal[1]
// = the sum of their int views over ALL items (the rescorer's observed, :154), scal[4] = over the OWNED rows with
// a delta only (this subtask's RowSumProcessWindowRowSum accumulator, RowSumAggregator.java:50,67)
__global__ __launch_bounds__(256) void k_add_rowsums(int32_t M, const int64_t *__restrict__ rs, const int32_t *__restrict__ nnz,
                                                     int64_t *__restrict__ grs, int64_t *__restrict__ scal) {
  __shared__ int64_t s_all[4], s_own[4];
  int64_t all = 0, own = 0;
  for (int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; a < M; a += int64_t(gridDim.x) * blockDim.x) {
    const int64_t d = rs[a];
    if (d == 0) continue;
    grs[a] += d;
    const int64_t d32 = int64_t(int32_t(uint32_t(uint64_t(d))));
    all += d32;
    if (nnz[a] > 0) own += d32;
  }
  for (int o = 32; o > 0; o >>= 1) {
    all += __shfl_xor(all, o, 64);
    own += __shfl_xor(own, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_all[threadIdx.x >> 6] = all;
    s_own[threadIdx.x >> 6] = own;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t t = s_all[0] + s_all[1] + s_all[2] + s_all[3], u = s_own[0] + s_own[1] + s_own[2] + s_own[3];
    if (t) atomicAdd(reinterpret_cast<unsigned long long *>(scal + 1), (unsigned long long)t);
    if (u) atomicAdd(reinterpret_cast<unsigned long long *>(scal + 4), (unsigned long long)u);
  }
}

// one wave per row: the row's entries copied to its packed offset rp[a]
__global__ __launch_bounds__(256) void k_pack_rows(int32_t M, const int64_t *__restrict__ base, const int32_t *__restrict__ nnz,
                                                   const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                   const uint32_t *__restrict__ cnt, int32_t *__restrict__ out_col,
                                                   uint32_t *__restrict__ out_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t a = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; a < M; a += n_waves) {
    const int32_t n = nnz[a];
    const int64_t b = base[a], o = rp[a];
    for (int32_t i = lane; i < n; i += 64) {
      out_col[o + i] = col[b + i];
      out_cnt[o + i] = cnt[b + i];
    }
  }
}

struct ScanTouched {  // 1 for a row the window's delta touches
  const int32_t *row_nnz;
  __device__ int64_t operator()(int64_t a) const { return row_nnz[a] > 0 ? 1 : 0; }
};

// ---- sparse global rows (n_items >= 40,320): the rescorer's itemRows (ItemRowRescorer...java:35,
// 171-177) as one sorted slab per row, g_len[a] (column, count) entries at g_base[a] of an arena.  A
// window's packed delta rows (drp, dcol, dcnt; ascending columns) are merged into a new slab per
// touched row: a delta entry whose column is new takes a slot, one whose column exists adds to it.
__device__ inline int64_t lower_bound_col(const int32_t *__restrict__ c, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The row of packed delta entry e: the last a with drp[a] <= e (drp ascending, drp[M] = nnz).
__device__ inline int32_t gs_row_of(const int64_t *__restrict__ drp, int32_t M, int64_t e) {
  int32_t lo = 0, hi = M;  // invariant: drp[lo] <= e < drp[hi]
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (drp[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// Per delta entry (flat over the window's entries, whatever the row lengths): its column's position
// in the row's old slab (opos) and flag[e] = 1 when the column is new to the row.
__global__ __launch_bounds__(256) void k_gs_flags(int32_t M, int64_t nnz, const int64_t *__restrict__ drp,
                                                  const int32_t *__restrict__ dcol, const int64_t *__restrict__ gbase,
                                                  const int32_t *__restrict__ glen, const int32_t *__restrict__ gcol,
                                                  int32_t *__restrict__ flag, int64_t *__restrict__ opos) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int32_t a = gs_row_of(drp, M, e);
  const int32_t *old = gcol + gbase[a];
  const int64_t n_old = glen[a], c = dcol[e];
  const int64_t p = lower_bound_col(old, n_old, int32_t(c));
  opos[e] = p;
  flag[e] = (p < n_old && old[p] == c) ? 0 : 1;
}

// new slab of every touched row with new columns: old + new entries, bump-allocated; a row without new
// columns keeps its slab (-2: counts added in place); chunks[a] = its old entries in kGsChunk pieces
constexpr int64_t kGsChunk = 2048;
__global__ void k_gs_alloc(int32_t M, const int64_t *__restrict__ drp, const int64_t *__restrict__ newpre,
                           const int32_t *__restrict__ glen, int64_t *__restrict__ nbase,
                           unsigned long long *__restrict__ bump, int32_t *__restrict__ chunks) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  const int64_t d0 = drp[a], d1 = drp[a + 1];
  chunks[a] = 0;
  if (d0 == d1) {
    nbase[a] = -1;
    return;
  }
  const int64_t added = newpre[d1] - newpre[d0];
  if (added == 0) {  // no new column: the counts are added in place (the slab stays)
    nbase[a] = -2;
    return;
  }
  const int64_t need = int64_t(glen[a]) + added;
  nbase[a] = int64_t(atomicAdd(bump, (unsigned long long)need));
  chunks[a] = int32_t((glen[a] + kGsChunk - 1) / kGsChunk);
}

// The moved rows' old entries, kGsChunk per block (flat over the rows, so a long row is spread over
// many blocks): an old entry shifts right by the new columns below it and takes a matching delta's count.
__global__ __launch_bounds__(256) void k_gs_move_all(int32_t M, const int64_t *__restrict__ chunk_pre,
                                                 const int64_t *__restrict__ drp, const int32_t *__restrict__ dcol,
                                                 const uint32_t *__restrict__ dcnt, const int64_t *__restrict__ newpre,
                                                 const int64_t *__restrict__ nbase, const int64_t *__restrict__ gbase,
                                                 const int32_t *__restrict__ glen, int32_t *__restrict__ gcol,
                                                 uint32_t *__restrict__ gcnt) {
  const int64_t n_chunks = chunk_pre[M];
  for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    int32_t lo = 0, hi = M;  // the row: last a with chunk_pre[a] <= ch
    while (hi - lo > 1) {
      const int32_t mid = (lo + hi) >> 1;
      if (chunk_pre[mid] <= ch) lo = mid; else hi = mid;
    }
    const int32_t a = lo;
    const int64_t i0 = (ch - chunk_pre[a]) * kGsChunk, n_old = glen[a], i1 = min(n_old, i0 + kGsChunk);
    const int64_t nb = nbase[a], d0 = drp[a], d = drp[a + 1] - d0, ob = gbase[a];
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
      const int32_t c = gcol[ob + i];
      const int64_t p = lower_bound_col(dcol + d0, d, c);
      const uint32_t add = (p < d && dcol[d0 + p] == c) ? dcnt[d0 + p] : 0u;
      const int64_t pos = nb + i + (newpre[d0 + p] - newpre[d0]);
      gcol[pos] = c;
      gcnt[pos] = gcnt[ob + i] + add;
    }
  }
}

// Per delta entry: a new column lands after the old columns below it in the row's new slab; in a row
// without new columns the count is added where the column sits.
__global__ __launch_bounds__(256) void k_gs_insert(int32_t M, int64_t nnz, const int64_t *__restrict__ drp,
                                                   const int32_t *__restrict__ dcol, const uint32_t *__restrict__ dcnt,
                                                   const int64_t *__restrict__ newpre, const int32_t *__restrict__ flag,
                                                   const int64_t *__restrict__ opos, const int64_t *__restrict__ nbase,
                                                   const int64_t *__restrict__ gbase, int32_t *__restrict__ gcol,
                                                   uint32_t *__restrict__ gcnt) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int32_t a = gs_row_of(drp, M, e);
  const int64_t nb = nbase[a];
  if (nb == -2) {
    gcnt[gbase[a] + opos[e]] += dcnt[e];
  } else if (flag[e]) {
    const int64_t pos = nb + (newpre[e] - newpre[drp[a]]) + opos[e];
    gcol[pos] = dcol[e];
    gcnt[pos] = dcnt[e];
  }
}

__global__ void k_gs_commit(int32_t M, const int64_t *__restrict__ drp, const int64_t *__restrict__ newpre,
                            const int64_t *__restrict__ nbase, int64_t *__restrict__ gbase, int32_t *__restrict__ glen) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M || nbase[a] < 0) return;
  glen[a] += int32_t(newpre[drp[a + 1]] - newpre[drp[a]]);
  gbase[a] = nbase[a];
}

// compaction: every row's slab to a fresh arena at the prefix of the row lengths (one wave per row)
__global__ __launch_bounds__(256) void k_gs_compact(int32_t M, const int64_t *__restrict__ newbase,
                                                    int64_t *__restrict__ gbase, const int32_t *__restrict__ glen,
                                                    const int32_t *__restrict__ col_in, const uint32_t *__restrict__ cnt_in,
                                                    int32_t *__restrict__ col_out, uint32_t *__restrict__ cnt_out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t a = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6; a < M; a += n_waves) {
    const int64_t from = gbase[a], to = newbase[a], n = glen[a];
    for (int64_t i = lane; i < n; i += 64) {
      col_out[to + i] = col_in[from + i];
      cnt_out[to + i] = cnt_in[from + i];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) gbase[a] = to;
  }
}

}  // namespace

Status launch_relocate(hipStream_t s, int64_t n, const int64_t *reloc, int32_t *arena) {
  if (n > 0) k_relocate<<<std::min<unsigned>(blocks_for(n * 64, 256), 4096), 256, 0, s>>>(n, reloc, arena);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_gather_lists(hipStream_t s, int64_t n, const int64_t *off, const int32_t *len, const int64_t *dst,
                           const int32_t *arena, int32_t *out) {
  if (n > 0) k_gather_lists<<<std::min<unsigned>(blocks_for(n * 64, 256), 4096), 256, 0, s>>>(n, off, len, dst, arena, out);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_append(hipStream_t s, int64_t n, const int64_t *new_ptr, const int64_t *new_dst, const int32_t *items,
                     int32_t *arena) {
  if (n > 0) k_append<<<std::min<unsigned>(blocks_for(n * 64, 256), 4096), 256, 0, s>>>(n, new_ptr, new_dst, items, arena);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_merge_global(hipStream_t s, int32_t M, const int64_t *row_base, const int32_t *row_nnz,
                           const int32_t *col, const uint32_t *cnt, const int64_t *rowsum_delta, uint32_t *G,
                           int64_t *grs, int64_t *scal, int64_t observed_window) {
  COOC_HIP_TRY(hipMemsetAsync(scal + 1, 0, sizeof(int64_t), s));
  k_merge_global<<<std::min<unsigned>(blocks_for(int64_t(M) * 64, 256), 8192), 256, 0, s>>>(
      M, row_base, row_nnz, col, cnt, rowsum_delta, G, grs, scal);
  k_finish_scalars<<<1, 1, 0, s>>>(scal, observed_window);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_owned_view(hipStream_t s, int32_t M, int32_t W, int32_t part, int32_t R, const int64_t *mbase,
                         const int32_t *mnnz, int64_t *base, int32_t *nnz) {
  COOC_HIP_TRY(hipMemsetAsync(base, 0, sizeof(int64_t) * size_t(M), s));
  COOC_HIP_TRY(hipMemsetAsync(nnz, 0, sizeof(int32_t) * size_t(M), s));
  if (R > 0) k_own_scatter<<<blocks_for(R, 256), 256, 0, s>>>(R, W, part, mbase, mnnz, base, nnz);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_merge_owned(hipStream_t s, int32_t M, const int64_t *base, const int32_t *nnz, const int32_t *col,
                          const uint32_t *cnt, const int64_t *rs_all, uint32_t *G, int64_t *grs, int64_t *scal,
                          int64_t observed_window) {
  COOC_HIP_TRY(hipMemsetAsync(scal + 1, 0, sizeof(int64_t), s));
  COOC_HIP_TRY(hipMemsetAsync(scal + 4, 0, sizeof(int64_t), s));
  // the owned rows' entries into the dense global rows (k_merge_global with no row sums: zero deltas); G == NULL: a
  // large universe, whose sparse row slabs the caller merges (launch_gs_merge)
  if (G)
    k_merge_global<<<std::min<unsigned>(blocks_for(int64_t(M) * 64, 256), 8192), 256, 0, s>>>(
        M, base, nnz, col, cnt, nullptr, G, nullptr, nullptr);
  k_add_rowsums<<<std::min<unsigned>(blocks_for(M, 256), 1024), 256, 0, s>>>(M, rs_all, nnz, grs, scal);
  k_finish_scalars<<<1, 1, 0, s>>>(scal, observed_window);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_pack_rows(hipStream_t s, int32_t M, const int64_t *base, const int32_t *nnz, const int32_t *col,
                        const uint32_t *cnt, DevBuf &rp, DevBuf &out_col, DevBuf &out_cnt, DevBuf &tmp, int64_t *total) {
  COOC_TRY(rp.reserve(sizeof(int64_t) * (size_t(M) + 1)));
  int64_t *d_rp = rp.as<int64_t>();
  COOC_TRY(tmp.reserve(scan_ws_bytes(M)));
  COOC_HIP_TRY(hipMemsetAsync(d_rp, 0, sizeof(int64_t), s));
  int64_t serr = 0;
  COOC_TRY(launch_scan_ws<true>(ScanI32{nnz}, d_rp + 1, M, tmp.as<unsigned long long>(), &serr, s));
  COOC_HIP_TRY(hipMemcpyAsync(total, d_rp + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (serr & 8) return Status{2, "internal bounds check failed (row prefix)"};
  COOC_TRY(out_col.reserve(sizeof(int32_t) * size_t(*total + 1)));
  COOC_TRY(out_cnt.reserve(sizeof(uint32_t) * size_t(*total + 1)));
  k_pack_rows<<<std::min<unsigned>(blocks_for(int64_t(M) * 64, 256), 8192), 256, 0, s>>>(
      M, base, nnz, d_rp, col, cnt, out_col.as<int32_t>(), out_cnt.as<uint32_t>());
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_user_cut(hipStream_t s, int64_t n_users, const int64_t *up, const int32_t *items, int32_t cut,
                       int64_t *cut_ptr, int32_t *cut_items, DevBuf &tmp, int64_t *n_cut) {
  *n_cut = 0;
  if (n_users <= 0) {
    COOC_HIP_TRY(hipMemsetAsync(cut_ptr, 0, sizeof(int64_t), s));
    return Status::Ok();
  }
  // tmp = [capped lengths int64[n_users + 1] | scan workspace] (the scan is not in place)
  const size_t lens_bytes = (sizeof(int64_t) * size_t(n_users + 1) + 255) / 256 * 256;
  COOC_TRY(tmp.reserve(lens_bytes + scan_ws_bytes(n_users)));
  int64_t *lens = tmp.as<int64_t>();
  k_cut_lens<<<blocks_for(n_users, 256), 256, 0, s>>>(n_users, up, cut, lens);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemsetAsync(cut_ptr, 0, sizeof(int64_t), s));
  int64_t serr = 0;
  COOC_TRY(launch_scan_ws<true>(ScanI64{lens + 1}, cut_ptr + 1, n_users,
                                reinterpret_cast<unsigned long long *>(static_cast<char *>(tmp.p) + lens_bytes), &serr, s));
  const int64_t waves = std::min<int64_t>(n_users, int64_t(1) << 16);
  k_cut_copy<<<blocks_for(waves * 64, 256), 256, 0, s>>>(n_users, up, items, cut_ptr, cut_items);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(n_cut, cut_ptr + n_users, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (serr & 8) return Status{2, "internal bounds check failed (capped list prefix)"};
  return Status::Ok();
}

Status launch_touched(hipStream_t s, int32_t M, const int32_t *row_nnz, int32_t *touched, int64_t *n_touched,
                      DevBuf &tmp) {
  COOC_TRY(tmp.reserve(select_tmp_bytes(M)));
  return select_if(ScanTouched{row_nnz}, M, touched, n_touched, tmp.p, s);
}

Status launch_gs_merge(hipStream_t s, int32_t M, const int64_t *drp, const int32_t *dcol, const uint32_t *dcnt,
                       int64_t nnz, GlobalSparse &g, DevBuf &tmp, int64_t *new_cols) {
  // 1. per delta entry: its old-slab position and whether its column is new; the flags' prefix
  //    (newpre[nnz] = the window's new columns)
  COOC_TRY(g.flag.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(nnz, 1))));
  COOC_TRY(g.opos.reserve(sizeof(int64_t) * size_t(std::max<int64_t>(nnz, 1))));
  COOC_TRY(g.newpre.reserve(sizeof(int64_t) * size_t(nnz + 1)));
  COOC_TRY(g.nbase.reserve(sizeof(int64_t) * size_t(M)));
  COOC_TRY(g.chunk_pre.reserve(sizeof(int64_t) * size_t(M + 1) + sizeof(int32_t) * size_t(M)));
  int32_t *flag = g.flag.as<int32_t>();
  int64_t *newpre = g.newpre.as<int64_t>(), *opos = g.opos.as<int64_t>();
  int64_t *chunk_pre = g.chunk_pre.as<int64_t>();
  int32_t *chunks = reinterpret_cast<int32_t *>(chunk_pre + M + 1);
  COOC_HIP_TRY(hipMemsetAsync(newpre, 0, sizeof(int64_t), s));
  int64_t serr = 0, serr2 = 0;
  if (nnz > 0) {
    k_gs_flags<<<blocks_for(nnz, 256), 256, 0, s>>>(M, nnz, drp, dcol, g.base.as<int64_t>(), g.len.as<int32_t>(),
                                                  g.col.as<int32_t>(), flag, opos);
    COOC_TRY(tmp.reserve(scan_ws_bytes(nnz)));
    COOC_TRY(launch_scan_ws<true>(ScanI32{flag}, newpre + 1, nnz, tmp.as<unsigned long long>(), &serr, s));
  }
  COOC_HIP_TRY(hipMemcpyAsync(new_cols, newpre + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (serr & 8) return Status{2, "internal bounds check failed (new-column prefix)"};
  // 2. room for the moved rows' new slabs (at most live + nnz entries): compact, then grow
  const int64_t need = g.live + nnz;
  if (g.bump + need > g.cap) {
    COOC_TRY(compact_global(s, M, g, tmp, std::max<int64_t>(2 * (g.live + need), int64_t(1) << 12)));
  }
  COOC_TRY(g.bump_dev.reserve(sizeof(uint64_t)));
  COOC_HIP_TRY(hipMemcpyAsync(g.bump_dev.p, &g.bump, sizeof(int64_t), hipMemcpyHostToDevice, s));
  k_gs_alloc<<<blocks_for(M, 256), 256, 0, s>>>(M, drp, newpre, g.len.as<int32_t>(), g.nbase.as<int64_t>(),
                                                g.bump_dev.as<unsigned long long>(), chunks);
  // 3. the moved rows' old entries in kGsChunk pieces, then every delta entry
  COOC_HIP_TRY(hipMemsetAsync(chunk_pre, 0, sizeof(int64_t), s));
  COOC_TRY(tmp.reserve(scan_ws_bytes(M)));
  COOC_TRY(launch_scan_ws<true>(ScanI32{chunks}, chunk_pre + 1, M, tmp.as<unsigned long long>(), &serr2, s));
  // (the chunk total is not read back: a fixed grid strides over chunk_pre[M] chunks)
  k_gs_move_all<<<2048, 256, 0, s>>>(M, chunk_pre, drp, dcol, dcnt, newpre, g.nbase.as<int64_t>(), g.base.as<int64_t>(),
                                    g.len.as<int32_t>(), g.col.as<int32_t>(), g.cnt.as<uint32_t>());
  if (nnz > 0)
    k_gs_insert<<<blocks_for(nnz, 256), 256, 0, s>>>(M, nnz, drp, dcol, dcnt, newpre, flag, opos, g.nbase.as<int64_t>(),
                                                    g.base.as<int64_t>(), g.col.as<int32_t>(), g.cnt.as<uint32_t>());
  k_gs_commit<<<blocks_for(M, 256), 256, 0, s>>>(M, drp, newpre, g.nbase.as<int64_t>(), g.base.as<int64_t>(),
                                                 g.len.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  int64_t bump = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&bump, g.bump_dev.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (serr2 & 8) return Status{2, "internal bounds check failed (moved-chunk prefix)"};
  g.bump = bump;
  g.live += *new_cols;
  return Status::Ok();
}

Status compact_global(hipStream_t s, int32_t M, GlobalSparse &g, DevBuf &tmp, int64_t new_cap) {
  DevBuf col2, cnt2;
  COOC_TRY(col2.reserve(sizeof(int32_t) * size_t(new_cap)));
  COOC_TRY(cnt2.reserve(sizeof(uint32_t) * size_t(new_cap)));
  COOC_TRY(g.nbase.reserve(sizeof(int64_t) * size_t(M + 1)));
  int64_t *nb = g.nbase.as<int64_t>();
  COOC_HIP_TRY(hipMemsetAsync(nb, 0, sizeof(int64_t), s));
  COOC_TRY(tmp.reserve(scan_ws_bytes(M)));
  int64_t serr = 0;
  COOC_TRY(launch_scan_ws<true>(ScanI32{g.len.as<int32_t>()}, nb + 1, M, tmp.as<unsigned long long>(), &serr, s));
  if (g.col.p)
    k_gs_compact<<<std::min<unsigned>(blocks_for(int64_t(M) * 64, 256), 8192), 256, 0, s>>>(
        M, nb, g.base.as<int64_t>(), g.len.as<int32_t>(), g.col.as<int32_t>(), g.cnt.as<uint32_t>(), col2.as<int32_t>(),
        cnt2.as<uint32_t>());
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (serr & 8) return Status{2, "internal bounds check failed (row slab prefix)"};
  g.col = std::move(col2);
  g.cnt = std::move(cnt2);
  g.cap = new_cap;
  g.bump = g.live;
  g.compactions++;
  return Status::Ok();
}

}  // namespace cooc
