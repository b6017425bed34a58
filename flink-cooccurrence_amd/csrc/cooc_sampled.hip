// cooc_sampled.hip — device side of the sampled streaming mode (cooc_sampling_enable, include/cooc.h).
//
// A window of the sampled mode changes reservoir slots in place (UserInteractionCounter...java:206-240), so
// its delta is signed: the pairs of the reservoirs after the window that involve a changed slot, minus the
// pairs before it that did.  Both halves are "pairs whose later position is new" of a list, the rule the window
// counters already apply (cooc_device.h), once the list is reordered:
//
//   k_sm_lists   one wave per user with a changed slot: applies the replacements (in order, the last writer of
//                a slot wins) and the appends to the history arena, and writes the user's PLUS list (the
//                unchanged slots of the reservoir, then the changed slots' new values; old = #unchanged) and,
//                when a slot that existed before the window was replaced, its MINUS list (the same unchanged
//                slots, then those slots' old values; the same old).
//   k_sd_*       the two counted windows' packed rows (ascending columns) combined into the signed delta:
//                the union of the keys with plus - minus (two's complement in the uint32 counts) and the
//                row-sum differences.  Flag, scan, scatter, as the row-slab merge (k_gs_*, cooc_stream.hip).
#include "cooc_stream_kernels.h"
#include "cooc_scan.h"

namespace cooc {
namespace {

inline unsigned blocks_for(int64_t n, int t) { return unsigned((n + t - 1) / t); }

constexpr int kSmMarkWords = 1024;  // one bit per reservoir slot: user_cut <= 32,767 (a Java short)

// One wave (a 64-thread workgroup) per user.  err bit 0: a list position or slot outside its bounds (nothing is
// written there), bit 1: the host's count of unchanged slots differs from the marks'.
__global__ __launch_bounds__(64) void k_sm_lists(int64_t n, const SmUser *__restrict__ users,
                                                 const int32_t *__restrict__ app, const int32_t *__restrict__ rep,
                                                 int32_t *arena, int64_t arena_len, int32_t *__restrict__ lists,
                                                 int64_t lists_len, int32_t *__restrict__ err) {
  __shared__ uint32_t mark[kSmMarkWords];
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
    const SmUser u = users[j];
    const int32_t L = u.len_old, Lp = u.len_new, n_unch = u.n_unchanged;
    const bool minus = u.minus_dst >= 0;
    if (L < 0 || Lp < L || Lp > kSmMarkWords * 32 || u.arena_off < 0 || u.arena_off + Lp > arena_len ||
        u.plus_dst < 0 || u.plus_dst + Lp > lists_len || (minus && u.minus_dst + L > lists_len) || n_unch < 0 ||
        n_unch > L) {
      if (lane == 0) atomicOr(err, 1);
      continue;  // (uniform over the workgroup)
    }
    for (int32_t w = lane; w < (Lp + 31) >> 5; w += 64) mark[w] = 0u;
    __syncthreads();
    for (int32_t s = L + lane; s < Lp; s += 64) atomicOr(&mark[s >> 5], 1u << (s & 31));
    for (int32_t r = lane; r < u.n_rep; r += 64) {
      const int32_t s = rep[2 * (int64_t(u.rep_begin) + r)];
      if (s >= 0 && s < Lp) atomicOr(&mark[s >> 5], 1u << (s & 31));
      else atomicOr(err, 1);
    }
    __syncthreads();
    // the reservoir before the window: unchanged slots to both lists, replaced slots' old values to the minus list
    int32_t cu = 0, cc = 0;
    for (int32_t base = 0; base < L; base += 64) {
      const int32_t s = base + lane;
      const bool valid = s < L;
      const int32_t v = valid ? arena[u.arena_off + s] : 0;
      const bool ch = valid && ((mark[s >> 5] >> (s & 31)) & 1u);
      const bool un = valid && !ch;
      const unsigned long long bu = __ballot(un), bc = __ballot(ch);
      if (un) {
        const int32_t idx = cu + __popcll(bu & below);
        if (idx < n_unch) {
          lists[u.plus_dst + idx] = v;
          if (minus) lists[u.minus_dst + idx] = v;
        }
      }
      if (ch && minus) {
        const int32_t idx = n_unch + cc + __popcll(bc & below);
        if (idx < L) lists[u.minus_dst + idx] = v;
      }
      cu += __popcll(bu);
      cc += __popcll(bc);
    }
    if (lane == 0 && (cu != n_unch || (!minus && cc != 0))) atomicOr(err, 2);
    __syncthreads();
    // userHistory: the appends, then the replacements in arrival order (a slot may be filled and replaced, or
    // replaced twice, within the window)
    for (int32_t i = lane; i < Lp - L; i += 64) arena[u.arena_off + L + i] = app[int64_t(u.app_begin) + i];
    __threadfence();
    __syncthreads();
    if (lane == 0)
      for (int32_t r = 0; r < u.n_rep; r++) {
        const int32_t s = rep[2 * (int64_t(u.rep_begin) + r)];
        if (s >= 0 && s < Lp) arena[u.arena_off + s] = rep[2 * (int64_t(u.rep_begin) + r) + 1];
      }
    __threadfence();
    __syncthreads();
    // the changed slots' values after the window, in slot order, behind the unchanged ones
    int32_t c2 = 0;
    for (int32_t base = 0; base < Lp; base += 64) {
      const int32_t s = base + lane;
      const bool ch = s < Lp && ((mark[s >> 5] >> (s & 31)) & 1u);
      const unsigned long long bc = __ballot(ch);
      if (ch) {
        const int32_t v = __hip_atomic_load(arena + u.arena_off + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int32_t idx = n_unch + c2 + __popcll(bc & below);
        if (idx < Lp) lists[u.plus_dst + idx] = v;
        else atomicOr(err, 1);
      }
      c2 += __popcll(bc);
    }
    __syncthreads();  // (the marks are reused by the next user)
  }
}

// ---- the signed delta: plus rows (prp, pcol, pcnt) and minus rows (mrp, mcol, mcnt), both packed M-row CSRs
// with ascending columns.
constexpr int kSdBlock = 256;  // threads per workgroup of the flat per-entry kernels (one entry per thread)

__device__ inline int64_t sd_lower_bound(const int32_t *__restrict__ c, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the row of packed entry e: the last a with rp[a] <= e (rp ascending, rp[M] = the entries)
__device__ inline int32_t sd_row_of(const int64_t *__restrict__ rp, int32_t M, int64_t e) {
  int32_t lo = 0, hi = M;
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (rp[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// per minus entry: its column's position in the plus row (opos) and flag = 1 when the plus row lacks the column
__global__ __launch_bounds__(kSdBlock) void k_sd_flags(int32_t M, int64_t n_minus, const int64_t *__restrict__ mrp,
                                                       const int32_t *__restrict__ mcol, const int64_t *__restrict__ prp,
                                                       const int32_t *__restrict__ pcol, int32_t *__restrict__ flag,
                                                       int64_t *__restrict__ opos) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n_minus) return;
  const int32_t a = sd_row_of(mrp, M, e);
  const int64_t p0 = prp[a], np = prp[a + 1] - p0;
  const int32_t c = mcol[e];
  const int64_t p = sd_lower_bound(pcol + p0, np, c);
  opos[e] = p;
  flag[e] = (p < np && pcol[p0 + p] == c) ? 0 : 1;
}

// per row: entries of the union and the row-sum difference
__global__ __launch_bounds__(kSdBlock) void k_sd_rows(int32_t M, const int64_t *__restrict__ prp,
                                                      const int64_t *__restrict__ mrp, const int64_t *__restrict__ newpre,
                                                      const int64_t *__restrict__ prs, const int64_t *__restrict__ mrs,
                                                      int32_t *__restrict__ out_nnz, int64_t *__restrict__ out_rs) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  out_nnz[a] = int32_t((prp[a + 1] - prp[a]) + (newpre[mrp[a + 1]] - newpre[mrp[a]]));
  out_rs[a] = prs[a] - mrs[a];
}

// per plus entry: shifted right by the minus-only columns below it; a matching minus count is subtracted
__global__ __launch_bounds__(kSdBlock) void k_sd_plus(int32_t M, int64_t n_plus, const int64_t *__restrict__ prp,
                                                      const int32_t *__restrict__ pcol, const uint32_t *__restrict__ pcnt,
                                                      const int64_t *__restrict__ mrp, const int32_t *__restrict__ mcol,
                                                      const uint32_t *__restrict__ mcnt, const int64_t *__restrict__ newpre,
                                                      const int64_t *__restrict__ orp, int64_t n_out,
                                                      int32_t *__restrict__ ocol, uint32_t *__restrict__ ocnt,
                                                      int32_t *__restrict__ err) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n_plus) return;
  const int32_t a = sd_row_of(prp, M, e);
  const int64_t m0 = mrp[a], nm = mrp[a + 1] - m0;
  const int32_t c = pcol[e];
  const int64_t p = sd_lower_bound(mcol + m0, nm, c);
  const uint32_t sub = (p < nm && mcol[m0 + p] == c) ? mcnt[m0 + p] : 0u;
  const int64_t pos = orp[a] + (e - prp[a]) + (newpre[m0 + p] - newpre[m0]);
  if (pos < 0 || pos >= n_out) {
    atomicOr(err, 1);
    return;
  }
  ocol[pos] = c;
  ocnt[pos] = pcnt[e] - sub;  // modulo 2^32: the two's complement of a negative net
}

// per minus-only entry: behind the plus columns below it
__global__ __launch_bounds__(kSdBlock) void k_sd_minus(int32_t M, int64_t n_minus, const int64_t *__restrict__ mrp,
                                                       const int32_t *__restrict__ mcol, const uint32_t *__restrict__ mcnt,
                                                       const int64_t *__restrict__ newpre, const int32_t *__restrict__ flag,
                                                       const int64_t *__restrict__ opos, const int64_t *__restrict__ orp,
                                                       int64_t n_out, int32_t *__restrict__ ocol,
                                                       uint32_t *__restrict__ ocnt, int32_t *__restrict__ err) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n_minus || !flag[e]) return;
  const int32_t a = sd_row_of(mrp, M, e);
  const int64_t pos = orp[a] + opos[e] + (newpre[e] - newpre[mrp[a]]);
  if (pos < 0 || pos >= n_out) {
    atomicOr(err, 1);
    return;
  }
  ocol[pos] = mcol[e];
  ocnt[pos] = 0u - mcnt[e];
}

}  // namespace

Status launch_sm_lists(hipStream_t s, int64_t n, const SmUser *users, const int32_t *app, const int32_t *rep,
                       int32_t *arena, int64_t arena_len, int32_t *lists, int64_t lists_len, int32_t *err) {
  COOC_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  if (n > 0)
    k_sm_lists<<<unsigned(std::min<int64_t>(n, 1 << 16)), 64, 0, s>>>(n, users, app, rep, arena, arena_len, lists,
                                                                       lists_len, err);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_signed_delta(hipStream_t s, int32_t M, const int64_t *prp, const int32_t *pcol, const uint32_t *pcnt,
                           const int64_t *prs, int64_t n_plus, const int64_t *mrp, const int32_t *mcol,
                           const uint32_t *mcnt, const int64_t *mrs, int64_t n_minus, SignedDelta &d, DevBuf &tmp) {
  COOC_TRY(d.flag.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(n_minus, 1))));
  COOC_TRY(d.opos.reserve(sizeof(int64_t) * size_t(std::max<int64_t>(n_minus, 1))));
  COOC_TRY(d.newpre.reserve(sizeof(int64_t) * size_t(n_minus + 1)));
  COOC_TRY(d.rp.reserve(sizeof(int64_t) * (size_t(M) + 1)));
  COOC_TRY(d.nnz.reserve(sizeof(int32_t) * size_t(M)));
  COOC_TRY(d.rowsum.reserve(sizeof(int64_t) * size_t(M)));
  COOC_TRY(d.err.reserve(sizeof(int32_t)));
  int32_t *flag = d.flag.as<int32_t>();
  int64_t *newpre = d.newpre.as<int64_t>(), *opos = d.opos.as<int64_t>(), *orp = d.rp.as<int64_t>();
  COOC_HIP_TRY(hipMemsetAsync(newpre, 0, sizeof(int64_t), s));
  COOC_HIP_TRY(hipMemsetAsync(orp, 0, sizeof(int64_t), s));
  COOC_HIP_TRY(hipMemsetAsync(d.err.p, 0, sizeof(int32_t), s));
  int64_t serr = 0, serr2 = 0;
  if (n_minus > 0) {
    k_sd_flags<<<blocks_for(n_minus, kSdBlock), kSdBlock, 0, s>>>(M, n_minus, mrp, mcol, prp, pcol, flag, opos);
    COOC_TRY(tmp.reserve(scan_ws_bytes(n_minus)));
    COOC_TRY(launch_scan_ws<true>(ScanI32{flag}, newpre + 1, n_minus, tmp.as<unsigned long long>(), &serr, s));
  }
  k_sd_rows<<<blocks_for(M, kSdBlock), kSdBlock, 0, s>>>(M, prp, mrp, newpre, prs, mrs, d.nnz.as<int32_t>(),
                                                         d.rowsum.as<int64_t>());
  COOC_HIP_TRY(hipGetLastError());
  COOC_TRY(tmp.reserve(scan_ws_bytes(M)));
  COOC_TRY(launch_scan_ws<true>(ScanI32{d.nnz.as<int32_t>()}, orp + 1, M, tmp.as<unsigned long long>(), &serr2, s));
  int64_t n_out = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&n_out, orp + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if ((serr | serr2) & 8) return Status{2, "internal bounds check failed (signed delta prefix)"};
  if (n_out < 0 || n_out > n_plus + n_minus) return Status{2, "internal bounds check failed (signed delta size)"};
  COOC_TRY(d.col.reserve(sizeof(int32_t) * size_t(n_out + 1)));
  COOC_TRY(d.cnt.reserve(sizeof(uint32_t) * size_t(n_out + 1)));
  if (n_plus > 0)
    k_sd_plus<<<blocks_for(n_plus, kSdBlock), kSdBlock, 0, s>>>(M, n_plus, prp, pcol, pcnt, mrp, mcol, mcnt, newpre, orp,
                                                                n_out, d.col.as<int32_t>(), d.cnt.as<uint32_t>(),
                                                                d.err.as<int32_t>());
  if (n_minus > 0)
    k_sd_minus<<<blocks_for(n_minus, kSdBlock), kSdBlock, 0, s>>>(M, n_minus, mrp, mcol, mcnt, newpre, flag, opos, orp,
                                                                  n_out, d.col.as<int32_t>(), d.cnt.as<uint32_t>(),
                                                                  d.err.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  int32_t h_err = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&h_err, d.err.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (h_err) return Status{2, "internal bounds check failed (signed delta scatter)"};
  d.entries = n_out;
  return Status::Ok();
}

}  // namespace cooc
