// cooc_sparse_rows.hip — the rows of the large-universe path that are sorted instead of accumulated in LDS
// tables (the algorithm: cooc_sparse.hip's opening comment): the small rows (k_sp_small, a workgroup per row)
// and the tiny ones (k_sp_tiny, a wave per row) at the tail of the work queue, and the deferred rows
// (k_srb_row: the rows whose hash table overflowed in k_sp_main; all whole rows under COOC_FLAG_SORT_ROWS).
// A small or tiny row of column rank >= kTW is a mirror source like k_sp_main's rows: its runs at the split rows'
// columns also go to its record of mirrored cells (SpArgs.mrec; cooc_sparse.hip's opening comment).
#include "cooc_sparse.h"
#include <algorithm>
#include <cstdio>
#include <vector>

#ifdef COOC_SP_STATS
#define SRB_STAT(k, v) do { if (threadIdx.x == 0) atomicAdd(srb_st + (k), (unsigned long long)(v)); } while (0)
// k_sp_small's phase clocks and counts (sm_st: SpArgs.stats + kSmStatBase; NULL under k_srb_row's sorts)
#define SM_STAT(k, v) do { if (threadIdx.x == 0 && sm_st) atomicAdd(sm_st + (k), (unsigned long long)(v)); } while (0)
#define SM_ST(A) ((A).stats + kSmStatBase)
#else
#define SM_ST(A) nullptr
#define SRB_STAT(k, v) do {} while (0)
#define SM_STAT(k, v) do {} while (0)
#endif

namespace cooc {

namespace {

// One contribution's list -- n0 tile-0 ids of arena0 at s0 (a multiple of 8), then n1 other ids of arena1
// at s1 (a multiple of 4): the user's parts are 16-B aligned -- copied by one wave to d[0, n0 + n1): 16-B
// loads (8 or 4 ids), both parts' loads of a step issued before their stores.
__device__ inline void wave_copy_list(const uint16_t *__restrict__ a0, const uint32_t *__restrict__ a1, uint32_t s0,
                                      uint32_t n0, uint32_t s1, uint32_t n1, uint32_t *d, int lane) {
  const uint4 *p0 = reinterpret_cast<const uint4 *>(a0 + s0);
  const uint4 *p1 = reinterpret_cast<const uint4 *>(a1 + s1);
  const uint32_t g0 = (n0 + 7u) >> 3, g1 = (n1 + 3u) >> 2, g = max(g0, g1);
  for (uint32_t q = uint32_t(lane); q < g; q += 64u) {
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
    if (q < g0) v0 = p0[q];
    if (q < g1) v1 = p1[q];
    if (q < g0) {
      const uint32_t w[4] = {v0.x, v0.y, v0.z, v0.w};
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint32_t pos = 8u * q + uint32_t(i);
        if (pos < n0) d[pos] = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
      }
    }
    if (q < g1) {
      const uint32_t w[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t pos = 4u * q + uint32_t(i);
        if (pos < n1) d[n0 + pos] = w[i];
      }
    }
  }
}

__device__ inline void tiny_sync() {  // the wave's LDS writes visible to its other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- small rows: one 512-thread workgroup per row -----------------------------------------------------
// A whole row of kTinyW < W <= kSmallW pairs -- at C3 the half million rows of the Zipf tail, each one LDS
// hash chunk over every tile in k_sp_main (~20 us per chunk there, two chunks per CU) -- sorted instead: its
// lists gathered into 16 KB of LDS (a wave per contribution, coalesced), LSD-radix-sorted by the workgroup
// (7-bit digits, wave ballots rank equal digits), equal columns counted (the segmented reduce of the +1
// increments), the diagonal's self term removed, the entries written in column order from a
// per-workgroup output slab.  At 33 KB per workgroup a CU holds four rows in flight.
constexpr int kSmallThreads = 512, kSmallWaves = kSmallThreads / 64;  // (kSmallSlab: cooc_sparse.h)
constexpr int kRadixBits = 7;

// Stable LSD radix sort of k[0, n), n <= kSmallW, keys < 2^bits, kRadixBits per pass, ping-ponging between
// k and t; returns the buffer that holds the sorted keys.  Wave w owns positions [w P, (w + 1) P),
// P = 64 ceil(n / (64 kWaves)) <= kSmallW / kWaves, 64 at a time: a lane's rank among equal digits is the count of
// the lanes below it that hold its digit (wave_match, cooc_sparse.h) plus the wave's running count of the digit; one
// exclusive scan over (digit, wave) turns the counts into the scatter bases.  Four LDS accesses per key per pass.
// The counters h (u16, kRadixHist<kThreads> of them) are wave-major with a pad of two, h[w (kD + 2) + d]: the bank
// of a counter is w + d / 2, so within a wave the digit pairs {2j, 2j + 1} each have a bank of their own in the
// ranking and in the scatter, and the waves' rows start on different banks for the scan, which reads one digit
// across the waves.  A wave alone touches its row outside the scan, so it zeroes the row itself at the head of a
// pass (its own scatter of the pass before read the row last: LDS accesses of a wave stay in order) and a pass
// has three barriers.  On entry the workgroup is past a barrier behind the last write of k and the last use of h
// and s_wt; on return it is past a barrier behind the last write of the result.
template <int kThreads>
constexpr int kRadixHist = (kThreads / 64) * ((1 << kRadixBits) + 2);
template <int kThreads>
__device__ uint32_t *block_radix_sort(uint32_t *k, uint32_t *t, uint16_t *h, uint32_t *s_wt, uint32_t n, int bits,
                                      unsigned long long *sm_st = nullptr) {
  constexpr int kWaves = kThreads / 64, kE = kSmallW / kThreads, kD = 1 << kRadixBits, kRow = kD + 2;
  static_assert(kD * kWaves == 2 * kThreads, "two scan entries per thread");
  static_assert(kD == 128, "a lane zeroes one word (two counters) of its wave's row");
  // a wave ranks kE * 64 positions: the rank (< kE * 64 <= 512, 9 bits) and the digit (7 bits) fill all 16 bits,
  // so no 16-bit value is free to mark "no key" -- a position holds a key iff it is below n (checked by position
  // in the scatter; the former 0xffff marker was also digit 127 at rank 511, and that key was never scattered)
  static_assert(kE * 64 <= 512 && kRadixBits <= 7, "rank and digit pack into 16 bits");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint16_t *hw = h + wave * kRow;  // the wave's counters
  // the scan's two entries of thread tid: digit sd of waves sw and sw + 1 (digit-major over waves, as ever)
  const int sd = tid / (kWaves / 2), sw = 2 * (tid % (kWaves / 2));
  // wave w ranks the span [w P, (w + 1) P) ∩ [0, n): P the smallest multiple of 64 that covers n with every
  // wave (a row of 1,500 keys: 192 positions per wave, not 512 for the first three waves and none for the rest)
  const uint32_t P = ((n + uint32_t(kWaves * 64) - 1u) / uint32_t(kWaves * 64)) * 64u;
  const uint32_t base = uint32_t(wave) * P, lim = min(n, base + P);
  for (int sh = 0; sh < bits; sh += kRadixBits) {
    [[maybe_unused]] const unsigned long long c_0 = STAT_CLOCK();
    reinterpret_cast<uint32_t *>(hw)[lane] = 0u;
    tiny_sync();
    uint32_t pk[kE / 2];  // (digit << 9 | rank), two per register; meaningful only at positions below n
#pragma unroll
    for (int e = 0; e < kE / 2; e++) pk[e] = 0u;
#pragma unroll
    for (int e = 0; e < kE; e++) {
      const uint32_t p0 = base + uint32_t(e) * 64u;
      if (p0 >= lim) continue;  // (wave-uniform)
      const uint32_t p = p0 + uint32_t(lane);
      const bool v = p < lim;
      const uint32_t d = v ? (k[p] >> sh) & uint32_t(kD - 1) : 0u;
      const WaveMask m = wave_match<kRadixBits>(d, v);
      if (v) {
        uint16_t *hd = hw + d;
        const uint32_t old = *hd, below = m.below();
        const uint32_t x = (old + below) | (d << 9);
        pk[e / 2] = (e & 1) ? pk[e / 2] | (x << 16) : x;  // (the even step of a register comes first)
        if (below == 0u) *hd = uint16_t(old + m.count());  // the group's first lane
      }
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long c_1 = STAT_CLOCK();
    const uint32_t h0 = h[sw * kRow + sd], h1 = h[(sw + 1) * kRow + sd];
    const uint32_t inc = wave_incl_scan(h0 + h1);
    if (lane == 63) s_wt[wave] = inc;
    __syncthreads();
    uint32_t ex = inc - h0 - h1;
#pragma unroll
    for (int w = 0; w < kWaves; w++) ex += w < wave ? s_wt[w] : 0u;
    h[sw * kRow + sd] = uint16_t(ex);
    h[(sw + 1) * kRow + sd] = uint16_t(ex + h0);
    __syncthreads();
    [[maybe_unused]] const unsigned long long c_2 = STAT_CLOCK();
#pragma unroll
    for (int e = 0; e < kE; e++) {
      const uint32_t p = base + uint32_t(e) * 64u + uint32_t(lane);
      if (p >= lim) continue;
      const uint32_t x = (pk[e / 2] >> ((e & 1) * 16)) & 0xffffu, d = x >> 9;
      t[uint32_t(hw[d]) + (x & 511u)] = k[p];
    }
    __syncthreads();
    SM_STAT(2, c_1 - c_0);
    SM_STAT(3, c_2 - c_1);
    SM_STAT(4, STAT_CLOCK() - c_2);
    SM_STAT(12, 1);
    uint32_t *x = k;
    k = t;
    t = x;
  }
  return k;
}

// (the two key buffers, the padded counters, and 1 KB for the scalars)
static_assert(4 * (2 * (kSmallW + 1) * 4 + kRadixHist<kSmallThreads> * 2 + 1024) <= 160 * 1024, "four per CU");
__global__ __launch_bounds__(kSmallThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_sp_small(SpArgs A) {
  __shared__ uint32_t b0[kSmallW + 1], b1[kSmallW + 1];  // (+1: the run starts' end marker)
  __shared__ alignas(4) uint16_t s_h[kRadixHist<kSmallThreads>];  // (zeroed by the word)
  __shared__ uint32_t s_wt[kSmallWaves];
  __shared__ int64_t s_i, s_pos, s_cur, s_end;
  __shared__ unsigned long long s_sum;
  __shared__ int32_t s_drop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t first = A.tot->n_chunks - A.tot->n_tiny - A.tot->n_small, n_small = A.tot->n_small;
  const uint16_t *a0 = reinterpret_cast<const uint16_t *>(A.tarena0);
  const uint32_t *a1 = reinterpret_cast<const uint32_t *>(A.tarena);
  int bits = 1;
  while (bits < 32 && (uint32_t(A.M) - 1u) >> bits) bits++;
  unsigned long long *const sm_st = SM_ST(A);
  if (tid == 0) s_cur = s_end = 0;
  for (;;) {
    [[maybe_unused]] const unsigned long long c_0 = STAT_CLOCK();
    if (tid == 0) {
      s_i = int64_t(atomicAdd(reinterpret_cast<unsigned long long *>(&A.tot->small_ctr), 1ull));
      s_sum = 0ull;
      s_drop = -1;
    }
    __syncthreads();
    const int64_t i = uni(s_i);
    if (i >= n_small) break;
    if (!SP_CHECK(A, first + i >= 0 && first + i < A.tot->n_chunks)) break;
    const SpWork it = A.queue[first + i];
    const int32_t a = it.row;
    if (!SP_CHECK(A, a >= 0 && a < A.M && it.k0 >= 0 && it.k0 < it.k1 && it.k1 <= A.n_contrib)) continue;
    const uint32_t ra = uint32_t(sp_rank(A, a));
    // a mirror source (k_sp_main): the runs at the split rows' columns also go to the row's record of mirrored
    // cells (SpArgs.mrec)
    const bool msrc = A.mirror_hi > 0 && ra >= uint32_t(kTW);
    const int64_t k0 = it.k0, k1 = it.k1, e0 = A.epre[k0];
    const int64_t W64 = uni(int64_t(A.epre[k1] - e0));
    // the planner sends rows of kTinyW < W <= kSmallW pairs here; a larger W would overrun the LDS buffers
    // (as k_sp_tiny, the row is refused and the run fails its row-sum check instead)
    if (W64 > int64_t(kSmallW) || W64 <= 0) {
      if (tid == 0) {
        atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 2ull | 8ull);
        A.tot->bad_row = a;
        A.row_nnz[a] = 0;
      }
      __syncthreads();
      continue;
    }
    const uint32_t W = uint32_t(W64);
    const uint32_t self = uint32_t(A.spre ? A.spre[k1] - A.spre[k0] : k1 - k0);
    [[maybe_unused]] const unsigned long long c_1 = STAT_CLOCK();
    // 1. the lists at their prefix positions (epre), a wave per contribution: wave w's contributions are
    //    k0 + w + 8 j; lane j reads the j-th one's list bounds (all in one round of loads), then the wave
    //    copies the lists one after another (wave_copy_list)
    for (int64_t kb = k0 + wave; kb < k1; kb += int64_t(kSmallWaves) * 64) {
      const int64_t km = kb + int64_t(kSmallWaves) * lane;
      uint32_t m_s0 = 0, m_n0 = 0, m_s1 = 0, m_n1 = 0, m_d = 0;
      if (km < k1) {
        const uint32_t u = A.vals[km] & kListMask;
        const int4 r = sp_list_bounds(A, SP_CHECK(A, u < A.n_users) ? u : 0u);
        m_s0 = uint32_t(r.x);
        m_n0 = uint32_t(r.y) - m_s0;
        m_s1 = uint32_t(r.z);
        m_n1 = uint32_t(r.w) - m_s1;
        m_d = uint32_t(A.epre[km] - e0);
        // the list lands inside the row's W ids; its 16-B groups inside the arenas
        if (!SP_CHECK(A, m_d + m_n0 + m_n1 <= W && (int64_t(m_s0) + m_n0 + 7) / 8 <= A.n_groups0 &&
                             (int64_t(m_s1) + m_n1 + 3) / 4 <= A.n_groups))
          m_n0 = m_n1 = 0;
      }
      const int cnt = int(min<int64_t>(64, (k1 - kb + kSmallWaves - 1) / kSmallWaves));
      for (int j = 0; j < cnt; j++)
        wave_copy_list(a0, a1, uint32_t(__shfl(int(m_s0), j, 64)), uint32_t(__shfl(int(m_n0), j, 64)),
                       uint32_t(__shfl(int(m_s1), j, 64)), uint32_t(__shfl(int(m_n1), j, 64)),
                       b0 + uint32_t(__shfl(int(m_d), j, 64)), lane);
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long c_2 = STAT_CLOCK();
    // 2. radix sort
    const uint32_t *b = block_radix_sort<kSmallThreads>(b0, b1, s_h, s_wt, W, bits, sm_st);
    [[maybe_unused]] const unsigned long long c_3 = STAT_CLOCK();
    // 3. runs: the heads (a column's first position) among thread tid's kPer positions, ranked by a block
    //    scan; their positions go to the free buffer (st), then a thread per run
    uint32_t *st = (b == b0) ? b1 : b0;
    constexpr int kPer = kSmallW / kSmallThreads;
    uint32_t hm = 0;
#pragma unroll
    for (int e = 0; e < kPer; e++) {
      const uint32_t p = uint32_t(tid) * kPer + uint32_t(e);
      if (p < W && (p == 0 || b[p] != b[p - 1])) hm |= 1u << e;
    }
    const uint32_t inc = wave_incl_scan(uint32_t(__popc(hm)));
    if (lane == 63) s_wt[wave] = inc;
    __syncthreads();
    uint32_t r = inc - uint32_t(__popc(hm)), n_runs = 0;
#pragma unroll
    for (int w = 0; w < kSmallWaves; w++) {
      r += w < wave ? s_wt[w] : 0u;
      n_runs += s_wt[w];
    }
    n_runs = uni(n_runs);
#pragma unroll
    for (int e = 0; e < kPer; e++)
      if ((hm >> e) & 1u) st[r++] = uint32_t(tid) * kPer + uint32_t(e);
    if (tid == 0) st[n_runs] = W;
    __syncthreads();
    uint64_t sum = 0;
    for (uint32_t q = uint32_t(tid); q < n_runs; q += kSmallThreads) {
      const uint32_t p = st[q], c = st[q + 1] - p;
      sum += c;
      if (b[p] == ra && c == self) s_drop = int32_t(q);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0 && sum) atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();
    const int32_t drop = uni(s_drop);
    const uint32_t n_keep = n_runs - (drop >= 0 ? 1u : 0u);
    [[maybe_unused]] const unsigned long long c_4 = STAT_CLOCK();
    if (tid == 0) {
      s_pos = -1;
      if (s_cur + int64_t(n_keep) > s_end) {
        const int64_t take = max<int64_t>(kSmallSlab, int64_t(n_keep));
        const int64_t nb = int64_t(atomicAdd(A.bump, (unsigned long long)take));
        if (nb + take > A.cap) {
          atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 4ull);
          s_cur = s_end = 0;
        } else {
          s_cur = nb;
          s_end = nb + take;
        }
      }
      if (s_cur + int64_t(n_keep) <= s_end) {
        s_pos = s_cur;
        s_cur += n_keep;
      }
      A.row_base[a] = (n_keep && s_pos >= 0) ? s_pos : 0;
      A.row_nnz[a] = s_pos >= 0 ? int32_t(n_keep) : 0;
      // the row-sum check: the runs (self pairs included) add up to W
      if (s_sum != (unsigned long long)W) {
        atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 2ull);
        A.tot->bad_row = a;
      }
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long c_5 = STAT_CLOCK();
    const int64_t pos = uni(s_pos);
    if (pos >= 0 && SP_CHECK(A, pos + int64_t(n_keep) <= A.cap && n_runs <= W)) {
      for (uint32_t q = uint32_t(tid); q < n_runs; q += kSmallThreads) {
        if (int32_t(q) == drop) continue;
        const uint32_t p = st[q], c = st[q + 1] - p, key = b[p];
        const int64_t o = pos + q - (drop >= 0 && int32_t(q) > drop ? 1 : 0);
        A.col_out[o] = sp_col(A, key);
        A.cnt_out[o] = c - (key == ra ? self : 0u);
        if (msrc && key < uint32_t(A.mirror_hi)) {  // (key < kTW <= ra: never the diagonal)
          const int32_t sl = A.mslot[key];
          // (the row's record: its cells within a few neighbouring lines)
          if (sl >= 0) A.mrec[int64_t(ra - uint32_t(kTW)) * A.mrec_w + sl] = c;
        }
      }
    }
    __syncthreads();  // (b and the shared scalars are rewritten by the next row)
    SM_STAT(0, c_1 - c_0);  // dequeue and row header
    SM_STAT(1, c_2 - c_1);  // list gather
    SM_STAT(13, c_3 - c_2);  // the sort (block_radix_sort: 2 ranking, 3 scan, 4 scatter, 12 passes)
    SM_STAT(5, c_4 - c_3);  // runs
    SM_STAT(6, c_5 - c_4);  // reservation
    SM_STAT(7, STAT_CLOCK() - c_5);  // stores
    SM_STAT(8, 1);
    SM_STAT(9, W);
    SM_STAT(10, k1 - k0);
    SM_STAT(11, STAT_CLOCK() - c_0);
  }
}

// ---- tiny rows: one wave per row ------------------------------------------------------------------
// A whole row of at most kTinyW pairs (a streaming window's rows are mostly a few pairs each): its
// contributions' lists are gathered into a per-wave LDS buffer, sorted (bitonic, wave-synchronous),
// equal columns counted (the segmented reduce of the +1 increments), the diagonal's self term removed,
// and the entries written in column order from a per-wave output slab.  No workgroup barrier.
// (kTinyThreads, kTinyWaves, kTinySlab: cooc_sparse.h)

__global__ __launch_bounds__(kTinyThreads) void k_sp_tiny(SpArgs A) {
  __shared__ uint32_t buf[kTinyWaves][kTinyW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t *b = buf[wave];
  const int64_t first = A.tot->n_chunks - A.tot->n_tiny, n_tiny = A.tot->n_tiny;
  const uint16_t *a0 = reinterpret_cast<const uint16_t *>(A.tarena0);
  const uint32_t *a1 = reinterpret_cast<const uint32_t *>(A.tarena);
  int64_t slab_cur = 0, slab_end = 0;  // (wave-uniform)
  for (;;) {
    int64_t i = 0;
    if (lane == 0) i = int64_t(atomicAdd(reinterpret_cast<unsigned long long *>(&A.tot->tiny_ctr), 1ull));
    i = __shfl(i, 0, 64);
    if (i >= n_tiny) break;
    const SpWork it = A.queue[first + i];
    const int32_t a = it.row;
    const int64_t k0 = it.k0, k1 = it.k1;
    // 1. the contributions' lists (whole lists), 64 at a time, into b in list order
    uint32_t W = 0;
    for (int64_t c0 = k0; c0 < k1; c0 += 64) {
      uint32_t s0 = 0, n0 = 0, s1 = 0, n1 = 0;
      if (c0 + lane < k1) {
        const uint32_t u = A.vals[c0 + lane] & kListMask;
        const int4 r = sp_list_bounds(A, u);
        s0 = uint32_t(r.x);
        n0 = uint32_t(r.y) - s0;
        s1 = uint32_t(r.z);
        n1 = uint32_t(r.w) - s1;
      }
      const uint32_t len = n0 + n1, inc = wave_incl_scan(len);
      const uint32_t tot = __shfl(inc, 63, 64);
      if (W + tot > uint32_t(kTinyW)) {  // (cannot happen: the planner's W bounds it)
        if (lane == 0) atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 2ull);
        W = 0;
        break;
      }
      uint32_t *d = b + W + inc - len;
      for (uint32_t q = 0; q < n0; q++) d[q] = a0[s0 + q];
      for (uint32_t q = 0; q < n1; q++) d[n0 + q] = a1[s1 + q];
      W += tot;
    }
    // 2. bitonic sort of b[0, n2), padded with kSink
    uint32_t n2 = 1;
    while (n2 < W) n2 <<= 1;
    for (uint32_t q = W + lane; q < n2; q += 64) b[q] = kSink;
    tiny_sync();
    for (uint32_t k = 2; k <= n2; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t q = lane; q < n2 / 2; q += 64) {
          const uint32_t lo = 2 * q - (q & (j - 1)), hi = lo + j;  // pairs (lo, lo + j) with bit j of lo clear
          const uint32_t x = b[lo], y = b[hi];
          const bool up = (lo & k) == 0;
          if ((x > y) == up) {
            b[lo] = y;
            b[hi] = x;
          }
        }
        tiny_sync();
      }
    }
    // 3. run heads (a 256-bit mask in four ballots), counts, the diagonal's self term
    const uint32_t self = uint32_t(A.spre ? A.spre[k1] - A.spre[k0] : k1 - k0);
    const uint32_t ra = uint32_t(sp_rank(A, a));
    const bool msrc = A.mirror_hi > 0 && ra >= uint32_t(kTW);
    uint64_t hm[kTinyW / 64];
#pragma unroll
    for (int g = 0; g < kTinyW / 64; g++) {
      const uint32_t q = uint32_t(g * 64 + lane);
      const bool h = q < W && (q == 0 || b[q] != b[q - 1]);
      hm[g] = __ballot(h);
    }
    uint32_t my_cnt[kTinyW / 64], n_keep = 0;
    uint64_t keep[kTinyW / 64];
#pragma unroll
    for (int g = 0; g < kTinyW / 64; g++) {
      const uint32_t q = uint32_t(g * 64 + lane);
      uint32_t cnt = 0;
      if ((hm[g] >> lane) & 1ull) {
        uint32_t nx = W;  // the next head after q
        const uint64_t rest = lane < 63 ? hm[g] >> (lane + 1) << (lane + 1) : 0ull;
        if (rest) {
          nx = uint32_t(g * 64 + __ffsll((long long)rest) - 1);
        } else {
#pragma unroll
          for (int g2 = g + 1; g2 < kTinyW / 64; g2++)
            if (nx == W && hm[g2]) nx = uint32_t(g2 * 64 + __ffsll((long long)hm[g2]) - 1);
        }
        cnt = nx - q;
        if (b[q] == ra) cnt -= self;
      }
      my_cnt[g] = cnt;
      keep[g] = __ballot(cnt != 0u);
      n_keep += uint32_t(__popcll(keep[g]));
    }
    // 4. output: the wave's slab; row sum check (counts add up to W - self)
    if (slab_cur + n_keep > slab_end) {
      int64_t nb = 0;
      if (lane == 0) {
        const int64_t take = max<int64_t>(kTinySlab, n_keep);
        nb = int64_t(atomicAdd(A.bump, (unsigned long long)take));
        if (nb + take > A.cap) {
          atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 4ull);
          nb = -1;
        } else {
          nb = nb | (take << 40);  // (take <= 2^23, positions < 2^40)
        }
      }
      nb = __shfl(nb, 0, 64);
      if (nb < 0) break;
      slab_cur = nb & ((int64_t(1) << 40) - 1);
      slab_end = slab_cur + (nb >> 40);
    }
    const int64_t base = slab_cur;
    slab_cur += n_keep;
    uint64_t rsum = 0;
    uint32_t before = 0;
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int g = 0; g < kTinyW / 64; g++) {
      if (my_cnt[g]) {
        const int64_t pos = base + before + uint32_t(__popcll(keep[g] & lt));
        const uint32_t key = b[g * 64 + lane];
        A.col_out[pos] = sp_col(A, key);
        A.cnt_out[pos] = my_cnt[g];
        rsum += my_cnt[g];
        if (msrc && key < uint32_t(A.mirror_hi)) {  // a mirror source, as in k_sp_small
          const int32_t sl = A.mslot[key];
          if (sl >= 0) A.mrec[int64_t(ra - uint32_t(kTW)) * A.mrec_w + sl] = my_cnt[g];
        }
      }
      before += uint32_t(__popcll(keep[g]));
    }
    for (int o = 32; o > 0; o >>= 1) rsum += __shfl_xor(rsum, o, 64);
    if (lane == 0) {
      A.row_base[a] = n_keep ? base : 0;
      A.row_nnz[a] = int32_t(n_keep);
      if (rsum != uint64_t(A.rowsum[a])) {
        atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 2ull);
        A.tot->bad_row = a;
      }
    }
    tiny_sync();  // (b is rewritten by the next row)
  }
}

// ---- the sort path of the deferred rows (hash table overflow in k_sp_main; COOC_FLAG_SORT_ROWS: all) ------
// The overflow fallback of the per-row Int2ShortOpenHashMap (ItemRowAggregator.java:21-31) as an MSD radix
// sort by hand: one 1,024-thread workgroup per deferred row.
//  1. the first digit: the row's pairs are partitioned by column tile (kTW columns).  The tile histogram
//     comes from the users' tile tables (tb: a list is already grouped by tile); a wave per contribution
//     reserves its tile segments in the buckets and copies the list with 16-B loads, every id to the
//     bucket of its tile (its high bits) in the row's scratch range; no id is read twice;
//  2. every tile bucket, in column order, becomes (column, count) runs: consecutive buckets of <= kSrbSort
//     ids together are radix-sorted in LDS (block_radix_sort, by the offset in their tile range: two 7-bit
//     passes for one tile) and their runs counted (the segmented reduce of the +1 increments); a larger
//     bucket is counted in kTW LDS counters (a counting sort of the last digit) and compacted in column order.  The
//     runs are written to the front of the row's scratch range (behind the buckets already consumed); the
//     diagonal loses the row's self term (dropped at zero);
//  3. the runs are copied to an exactly sized output slice (relabelled columns mapped back), with the
//     row-sum check of the other paths.
// ~16 B of HBM traffic per pair (segment copy 4 + 4, bucket read 4, run copy) against ~40 for a device-wide
// radix sort of packed 8-B keys (the path this one replaced).
constexpr int kSrbThreads = 1024, kSrbWaves = kSrbThreads / 64, kSrbSort = kSmallW;
// buf: sort keys [0, kSrbSort], the other radix buffer from kSrbB, the radix histogram (u16) from kSrbH
// (kRadixHist: padded wave-major rows, an even count of u16)
constexpr int kSrbB = kSrbSort + 8, kSrbH = kSrbB + kSrbSort + 8, kSrbUsed = kSrbH + kRadixHist<kSrbThreads> / 2;
static_assert(kRadixHist<kSrbThreads> % 2 == 0 && kSrbUsed <= kTW, "the sort areas share the bucket's LDS counters");

__device__ inline uint32_t srb_block_excl_scan(uint32_t x, uint32_t *total, uint32_t *s_wt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(x);
  if (lane == 63) s_wt[wave] = inc;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kSrbWaves; w++) {
    const uint32_t v = s_wt[w];
    pre += w < wave ? v : 0u;
    tot += v;
  }
  __syncthreads();
  *total = uni(tot);
  return pre + inc - x;
}

__global__ __launch_bounds__(kSrbThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_srb_row(
    const int32_t *__restrict__ rows, int64_t n_rows, int64_t scr_stride, const int64_t *__restrict__ row_ptr,
    const uint32_t *__restrict__ vals, const int32_t *__restrict__ tb, const uint16_t *__restrict__ arena0,
    const uint32_t *__restrict__ arena1, int32_t T, int32_t Mc, uint32_t *__restrict__ scr_ids,
    uint32_t *__restrict__ scr_cnt, const int64_t *__restrict__ spre, const int64_t *__restrict__ rowsum,
    const int32_t *__restrict__ hot_col, const int32_t *__restrict__ pos_of, int32_t *__restrict__ col_out,
    uint32_t *__restrict__ cnt_out, unsigned long long *__restrict__ bump, int64_t cap,
    int64_t *__restrict__ row_base, int32_t *__restrict__ row_nnz, PlanTotals *__restrict__ tot,
    unsigned long long *__restrict__ srb_st) {
  __shared__ uint32_t buf[kTW];  // dense counters | sorted bucket keys [0, kSrbSort) + run starts above
  __shared__ uint32_t s_hist[kSpMaxTiles + 1], s_off[kSpMaxTiles + 1], s_cur[kSpMaxTiles + 1];
  __shared__ uint32_t s_wt[kSrbWaves];
  __shared__ int32_t s_wdst[kSrbWaves][kSpMaxTiles];  // per wave: a contribution's bucket positions by tile
  __shared__ uint32_t s_o;        // runs written so far (the row's entries)
  __shared__ int32_t s_drop;      // the bucket's run index of a diagonal that drops to zero (-1: none)
  __shared__ unsigned long long s_sum;
  __shared__ int64_t s_base, s_j, s_scur, s_send;  // the row's output base; the dequeued row; the output slab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's scratch range (every deferred row's pairs fit it); rows dequeued in deferral order
  const int64_t rb = int64_t(blockIdx.x) * scr_stride;
  for (int i = tid; i < kTW; i += kSrbThreads) buf[i] = 0u;
  if (tid == 0) s_scur = s_send = 0;
  bool dirty = false;  // the sort areas of buf hold keys (the counting path needs zero counters)
  for (;;) {
  if (tid == 0) s_j = int64_t(atomicAdd(reinterpret_cast<unsigned long long *>(&tot->srb_ctr), 1ull));
  if (tid <= kSpMaxTiles) {
    s_hist[tid] = 0u;
    s_cur[tid] = 0u;
  }
  if (tid == 0) {
    s_o = 0u;
    s_sum = 0ull;
  }
  __syncthreads();
  const int64_t j = uni(s_j);
  if (j >= n_rows) break;
  const int32_t a = rows[j];
  const uint32_t ra = uint32_t(relabel_pos(pos_of, uint32_t(a)));
  const int64_t k0 = row_ptr[a], k1 = row_ptr[a + 1];
  const uint32_t self = uint32_t(spre ? spre[k1] - spre[k0] : k1 - k0);
  const unsigned long long c_0 = STAT_CLOCK();
  SRB_STAT(5, 1);
  SRB_STAT(6, k1 - k0);
  // 1a. the tile histogram from the tile tables: a wave per contribution, lane t its tile t
  for (int64_t k = k0 + wave; k < k1; k += kSrbWaves) {
    const int32_t *tbu = tb + int64_t(vals[k] & kListMask) * (T + 2);
    if (lane < T) {
      const int32_t n_t = lane == 0 ? tbu[T + 1] - tbu[0] : tbu[lane + 1] - tbu[lane];
      if (n_t > 0) atomicAdd(&s_hist[lane], uint32_t(n_t));
    }
  }
  __syncthreads();
  if (wave == 0) {  // bucket starts: a wave scan of the T <= 64 tile counts
    const uint32_t h = lane < T ? s_hist[lane] : 0u, inc = wave_incl_scan(h);
    if (lane < T) s_off[lane] = inc - h;
    if (lane == T - 1) s_off[T] = inc;
  }
  __syncthreads();
  const unsigned long long c_1 = STAT_CLOCK();
  SRB_STAT(0, c_1 - c_0);
  // 1b. the partition, a wave per contribution: lane t reserves its tile's segment in bucket t; then the
  // wave copies the list with 16-B loads -- the tile-0 part (u16) to bucket 0, the other part (u32, tiles
  // in order) id by id to the bucket of the id's tile (the tile is the id's high bits)
  int32_t *wdst = s_wdst[wave];
  for (int64_t k = k0 + wave; k < k1; k += kSrbWaves) {
    const int32_t *tbu = tb + int64_t(vals[k] & kListMask) * (T + 2);
    const int32_t s0 = tbu[0], n0 = tbu[T + 1] - s0, s1 = tbu[1], n1 = tbu[T] - s1;
    if (lane < T) {
      const int32_t st = lane == 0 ? s0 : tbu[lane];
      const int32_t n_t = lane == 0 ? n0 : tbu[lane + 1] - st;
      const uint32_t d = n_t > 0 ? atomicAdd(&s_cur[lane], uint32_t(n_t)) : 0u;
      // bucket position of the part's position q: wdst[t] + q
      wdst[lane] = int32_t(s_off[lane] + d) - (lane == 0 ? 0 : st - s1);
    }
    tiny_sync();
    const uint4 *p0 = reinterpret_cast<const uint4 *>(arena0 + s0);
    const uint4 *p1 = reinterpret_cast<const uint4 *>(arena1 + s1);
    const uint32_t g0 = (uint32_t(n0) + 7u) >> 3, g1 = (uint32_t(n1) + 3u) >> 2, g = max(g0, g1);
    uint32_t *dst0 = scr_ids + rb + wdst[0];
    for (uint32_t q = uint32_t(lane); q < g; q += 64u) {
      uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
      if (q < g0) v0 = p0[q];
      if (q < g1) v1 = p1[q];
      if (q < g0) {
        const uint32_t w[4] = {v0.x, v0.y, v0.z, v0.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const uint32_t pos = 8u * q + uint32_t(i);
          if (pos < uint32_t(n0)) dst0[pos] = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
        }
      }
      if (q < g1) {
        const uint32_t w[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint32_t pos = 4u * q + uint32_t(i);
          if (pos < uint32_t(n1)) scr_ids[rb + wdst[w[i] >> kTShift] + int32_t(pos)] = w[i];
        }
      }
    }
    tiny_sync();  // (wdst is rewritten for the wave's next contribution)
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (the buckets are read back by other waves)
  const unsigned long long c_2 = STAT_CLOCK();
  SRB_STAT(1, c_2 - c_1);
  SRB_STAT(7, s_off[T]);
  // 2. the buckets in column order
  uint64_t sum = 0;
  for (int32_t t = 0; t < T;) {
    const uint32_t n = uni(s_hist[t]);
    if (n == 0) {
      t++;
      continue;
    }
    const uint32_t o = uni(s_o);
    const uint32_t c0 = uint32_t(t) * uint32_t(kTW);
    if (n <= uint32_t(kSrbSort)) {
      // a group: this bucket and the next ones while they fit kSrbSort ids together (contiguous in the
      // scratch), radix-sorted in LDS by their offset in the group's tile range, then its runs
      const unsigned long long c_g = STAT_CLOCK();
      uint32_t g = n;
      int32_t t1 = t + 1;
      while (t1 < T && g + uni(s_hist[t1]) <= uint32_t(kSrbSort)) g += uni(s_hist[t1++]);
      const uint32_t *src = scr_ids + rb + s_off[t];
      uint32_t *ka = buf, *kb = buf + kSrbB;
      {
        static_assert(kSrbSort == 4 * kSrbThreads, "four keys per thread");
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const uint32_t i = uint32_t(tid) + uint32_t(u) * kSrbThreads;
          v[u] = i < g ? src[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const uint32_t i = uint32_t(tid) + uint32_t(u) * kSrbThreads;
          if (i < g) ka[i] = v[u] - c0;
        }
      }
      __syncthreads();
      int bits = kTShift;
      while ((uint32_t(t1 - t) << kTShift) > (1u << bits)) bits++;
      const uint32_t *ks = block_radix_sort<kSrbThreads>(ka, kb, reinterpret_cast<uint16_t *>(buf + kSrbH), s_wt, g,
                                                         bits);
      uint32_t *st = ks == ka ? kb : ka;  // run starts in the free area (+1: the end marker)
      dirty = true;
      uint32_t hm = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t i = 4u * uint32_t(tid) + uint32_t(e);
        if (i < g && (i == 0 || ks[i] != ks[i - 1])) hm |= 1u << e;
      }
      uint32_t n_runs;
      const uint32_t r0 = srb_block_excl_scan(uint32_t(__popc(hm)), &n_runs, s_wt);
      if (tid == 0) s_drop = -1;
      {
        uint32_t r = r0;
#pragma unroll
        for (int e = 0; e < 4; e++)
          if ((hm >> e) & 1u) st[r++] = 4u * uint32_t(tid) + uint32_t(e);
      }
      if (tid == 0) st[n_runs] = g;
      __syncthreads();
      for (uint32_t r = tid; r < n_runs; r += kSrbThreads) {
        const uint32_t p = st[r], c = st[r + 1] - p;
        sum += c;
        if (ks[p] + c0 == ra && c == self) s_drop = int32_t(r);
      }
      __syncthreads();
      const int32_t drop = uni(s_drop);
      for (uint32_t r = tid; r < n_runs; r += kSrbThreads) {
        if (int32_t(r) == drop) continue;
        const uint32_t p = st[r], c = st[r + 1] - p, col = ks[p] + c0;
        const uint32_t q = o + r - (drop >= 0 && int32_t(r) > drop ? 1u : 0u);
        scr_ids[rb + q] = col;
        scr_cnt[rb + q] = c - (col == ra ? self : 0u);
      }
      if (tid == 0) s_o = o + n_runs - (drop >= 0 ? 1u : 0u);
      __syncthreads();
      SRB_STAT(2, STAT_CLOCK() - c_g);
      SRB_STAT(8, 1);
      t = t1;
    } else {
      // counting sort of the bucket's last digit: kTW LDS counters, then a column-order compaction
      const unsigned long long c_c = STAT_CLOCK();
      if (dirty) {
        for (uint32_t i = tid; i < uint32_t(kSrbUsed); i += kSrbThreads) buf[i] = 0u;
        dirty = false;
        __syncthreads();
      }
      const uint32_t *src = scr_ids + rb + s_off[t];
      const uint32_t w = uint32_t(min(int64_t(kTW), int64_t(Mc) - int64_t(c0)));
      for (uint32_t i0 = 0; i0 < n; i0 += 8u * kSrbThreads) {  // (8 loads in flight per thread)
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint32_t i = i0 + uint32_t(tid) + uint32_t(u) * kSrbThreads;
          v[u] = i < n ? src[i] : kSink;
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (v[u] != kSink) atomicAdd(&buf[v[u] - c0], 1u);
      }
      __syncthreads();
      if (tid == 0 && ra >= c0 && ra < c0 + w) buf[ra - c0] -= self;  // (the self pairs were counted too)
      __syncthreads();
      constexpr uint32_t per = uint32_t(kTW) / kSrbWaves;  // columns per wave (1,024)
      const uint32_t lo = min(w, uint32_t(wave) * per), hi = min(w, lo + per);
      uint32_t c = 0;
      for (uint32_t b = lo + lane; b < hi; b += 64) c += buf[b] != 0u;
      for (int x = 32; x > 0; x >>= 1) c += __shfl_xor(c, x, 64);
      uint32_t n_out;
      uint32_t off = srb_block_excl_scan(lane == 0 ? c : 0u, &n_out, s_wt);
      off = __shfl(off, 0, 64);
      const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
      for (uint32_t b0 = lo; b0 < hi; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        const uint32_t v = b < hi ? buf[b] : 0u;
        const uint64_t m = __ballot(v != 0u);
        if (v) {
          const uint32_t q = o + off + uint32_t(__popcll(m & lt));
          scr_ids[rb + q] = c0 + b;
          scr_cnt[rb + q] = v;
          sum += v;
          buf[b] = 0u;
        }
        off += uint32_t(__popcll(m));
      }
      if (tid == 0) {
        s_o = o + n_out;
        if (ra >= c0 && ra < c0 + w) sum += self;  // (sum counts the self pairs on both paths)
      }
      __syncthreads();
      SRB_STAT(3, STAT_CLOCK() - c_c);
      SRB_STAT(9, 1);
      t++;
    }
  }
  const unsigned long long c_3 = STAT_CLOCK();
  // 3. the exact output slice; the row-sum check
  for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x, 64);
  if (lane == 0 && sum) atomicAdd(&s_sum, (unsigned long long)sum);
  __syncthreads();
  const uint32_t d = s_o;
  if (tid == 0) {
    // the row's slice from the workgroup's output slab (a new slab of >= kSmallSlab entries when it is short)
    int64_t b = -1;
    if (s_scur + int64_t(d) > s_send) {
      const int64_t take = max<int64_t>(kSmallSlab, int64_t(d));
      const int64_t nb = int64_t(atomicAdd(bump, (unsigned long long)take));
      if (nb + take > cap) {
        atomicOr(reinterpret_cast<unsigned long long *>(&tot->err), 4ull);
        s_scur = s_send = 0;
      } else {
        s_scur = nb;
        s_send = nb + take;
      }
    }
    if (s_scur + int64_t(d) <= s_send) {
      b = s_scur;
      s_scur += d;
    }
    s_base = b;
    row_base[a] = (b < 0 || d == 0) ? 0 : b;
    row_nnz[a] = b < 0 ? 0 : int32_t(d);
    if (s_sum != (unsigned long long)(rowsum[a] + self)) {
      atomicOr(reinterpret_cast<unsigned long long *>(&tot->err), 2ull);
      tot->bad_row = a;
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int64_t base = s_base;
  (void)c_3;
  for (uint32_t i0 = 0; base >= 0 && i0 < d; i0 += 4u * kSrbThreads) {  // (4 entries' loads in flight per thread)
    uint32_t c[4], n[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t i = i0 + uint32_t(tid) + uint32_t(u) * kSrbThreads;
      c[u] = i < d ? scr_ids[rb + i] : 0u;
      n[u] = i < d ? scr_cnt[rb + i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t i = i0 + uint32_t(tid) + uint32_t(u) * kSrbThreads;
      if (i < d) {
        col_out[base + i] = relabel_col(hot_col, c[u]);
        cnt_out[base + i] = n[u];
      }
    }
  }
  SRB_STAT(4, STAT_CLOCK() - c_3);
  SRB_STAT(10, STAT_CLOCK() - c_0);
  __builtin_amdgcn_s_waitcnt(0);  // (the next row's partition rewrites the scratch these loads read)
  __syncthreads();
  }
}

__global__ void k_sr_pair_work(const int32_t *__restrict__ rows, int64_t n, const int64_t *__restrict__ row_w,
                               int64_t *__restrict__ out) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < n) out[j] = row_w[rows[j]];
}

}  // namespace

Status launch_sp_small(const SpArgs &A, int64_t grid, hipStream_t s) {
  k_sp_small<<<unsigned(grid), kSmallThreads, 0, s>>>(A);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status launch_sp_tiny(const SpArgs &A, int64_t grid, hipStream_t s) {
  k_sp_tiny<<<unsigned(grid), kTinyThreads, 0, s>>>(A);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// The deferred rows (k_sp_main: hash table overflow; COOC_FLAG_SORT_ROWS: every whole row) through k_srb_row:
// persistent workgroups (two per CU) take the rows in deferral order; each has a scratch range for the largest
// row's pairs as u32 ids + u32 run counts (a whole row has at most kSplitWork pairs).
Status Counter::run_deferred(int64_t n_def, int32_t T, const int64_t *row_ptr, const uint32_t *vals,
                             const int64_t *spre, int64_t cap, hipStream_t s) {
  const int32_t *rows = sp_defer_.as<int32_t>();
  // the rows' pair work (sp_roww_), to the host in deferral order
  COOC_TRY(sr_aux_.reserve(sizeof(int64_t) * size_t(n_def)));
  int64_t *d_w = sr_aux_.as<int64_t>();
  k_sr_pair_work<<<nblocks(n_def, 256), 256, 0, s>>>(rows, n_def, sp_roww_.as<int64_t>(), d_w);
  COOC_HIP_TRY(hipGetLastError());
  std::vector<int64_t> w(size_t(n_def), 0);
  COOC_HIP_TRY(hipMemcpyAsync(w.data(), d_w, sizeof(int64_t) * size_t(n_def), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  size_t f0 = 0, t0 = 0;
  COOC_HIP_TRY(hipMemGetInfo(&f0, &t0));
  int64_t max_w = 1;
  for (int64_t j = 0; j < n_def; j++) {
    max_w = std::max(max_w, w[size_t(j)]);
    last_deferred_pairs_ += w[size_t(j)];
  }
  const int64_t stride = (max_w + 63) & ~int64_t(63);
  int64_t grid = std::min<int64_t>(n_def, 2 * int64_t(n_cu_));
  grid = std::max<int64_t>(1, std::min<int64_t>(grid, int64_t(f0 / 2) / (8 * stride)));
  COOC_TRY(sr_keys_.reserve(sizeof(uint32_t) * size_t(2 * grid * stride)));
  uint32_t *ids = sr_keys_.as<uint32_t>(), *cn = ids + grid * stride;
  unsigned long long *srb_st = nullptr;
#ifdef COOC_SP_STATS
  static unsigned long long *d_srb = nullptr;
  if (!d_srb) COOC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_srb), 16 * 8));
  COOC_HIP_TRY(hipMemsetAsync(d_srb, 0, 16 * 8, s));
  srb_st = d_srb;
#endif
  PlanTotals *tot = tot_.as<PlanTotals>();
  COOC_HIP_TRY(hipMemsetAsync(&tot->srb_ctr, 0, sizeof(int64_t), s));
  k_srb_row<<<unsigned(grid), kSrbThreads, 0, s>>>(
      rows, n_def, stride, row_ptr, vals, sp_tb_.as<int32_t>(), sp_arena0_.as<uint16_t>(), sp_arena_.as<uint32_t>(), T,
      last_mc_, ids, cn, spre, rowsum_.as<int64_t>(), last_hot_col_, last_pos_of_, col_.as<int32_t>(),
      cnt_.as<uint32_t>(), bump_.as<unsigned long long>(), cap, row_base_.as<int64_t>(), row_nnz_.as<int32_t>(), tot,
      srb_st);
  COOC_HIP_TRY(hipGetLastError());
#ifdef COOC_SP_STATS
  {
    unsigned long long h[16];
    COOC_HIP_TRY(hipMemcpy(h, srb_st, sizeof(h), hipMemcpyDeviceToHost));
    const double r = h[5] ? double(h[5]) : 1.0;
    fprintf(stderr, "[srb stats] rows %llu contributions %llu pairs %llu | per row (us): hist %.1f partition %.1f "
            "sort groups %.1f (%llu) counting %.1f (%llu) output %.1f total %.1f\n", h[5], h[6], h[7], h[0] / 100.0 / r,
            h[1] / 100.0 / r, h[2] / 100.0 / r, h[8], h[3] / 100.0 / r, h[9], h[4] / 100.0 / r, h[10] / 100.0 / r);
  }
#endif
  return Status::Ok();
}

}  // namespace cooc
