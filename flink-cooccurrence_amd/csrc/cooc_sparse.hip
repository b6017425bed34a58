// cooc_sparse.hip — one window over empty histories for LARGE item universes (n_items >= 40,320,
// the C3 / C5 configs: 1e6 items), on gfx950.
//
// Same semantics as the batch path (cooc_count.hip): NonSampledUserInteractionCounter...java:113-165
// expanded from empty histories, reduced per row like ItemRowAggregator.java:26-31
// (Int2ShortOpenHashMap.addTo, exact uint32 here) and RowSumAggregator.java:25-27:
//   C[a, b] = sum_u #{ordered position pairs (p != q) : x_p = a, x_q = b},  rowsum[a] = sum_b C[a, b].
// A row a is the sum of the lists of the users that hold a (one "contribution" per interaction
// (u, a)), minus 1 at column a per contribution (the pair of a position with itself).
//
// At n_items = 1e6 a row cannot live in one LDS row (160 KB = 40K counters), and most rows are
// sparse: under Zipf(1) the row of an item of rank r holds ~W_1 / r pairs over up to 1e6 columns.
// The work unit is therefore a whole ROW, taken by one persistent workgroup per CU (heaviest rows
// first), which walks the row's column range as a sequence of CHUNKS and appends each chunk's
// entries, in column order, to the row's contiguous output (no gather pass):
//   * hash chunk  — a range of column tiles whose expected distinct keys fit an LDS open-addressing
//                   table (keys + counts, 1K..16K slots, the Int2ShortOpenHashMap of
//                   ItemRowAggregator.java:21-31 in LDS).  Sorted output without a sort: the keys'
//                   32-column blocks are ranked through a bitmap (L1) and per-block 32-bit masks, and
//                   an entry's slot is its block's base + the popcount of its mask below it.  A table
//                   that overflows (more distinct keys than expected) is redone with a 4x table, and
//                   at 16K slots as dense tiles.
//   * dense chunk — one column tile of 32,768 columns as uint32 LDS counters (one ds_add per pair),
//                   compacted in column order.
// The chunk plan of a row comes from its pair work W_a (exact) and the expected distinct keys per
// tile, E[d_t | W] = sum_{b in t} 1 - exp(-W f_b / N) (f_b = global frequency of b), tabulated per
// tile for W = 2^(k/2).  Per-user lists are regrouped by tile once (tb[u][t] = first position of
// tile t in u's list), so a tile range of a user's list is one contiguous segment.
// The few rows above kSplitWork pairs (the hottest items) are split into (row, tile, contribution
// range) work items that add into a dense uint32 staging row in HBM; a finalize kernel compacts
// each staging row (with the uint32 overflow check: sum of the counts == the closed-form row sum).
// When every split row's column lies in tile 0 (the usual case: they are the hottest items), their shares count
// tile 0 only and the cells above it are mirrored: C[a, b] = C[b, a], and row b's own tile-0 chunk has that
// count already, so it hands it over (SpArgs.mslot; ~15 tail ids walked per cell otherwise).  Row b owns one
// contiguous RECORD of those cells, one per split row (SpArgs.mrec: n_split cells padded to 64 B, ~1.1 KB at C3),
// so its stores stay within a few neighbouring lines -- a dense tile 0 writes the record whole, a thread per
// slot, coalesced -- and the staging rows shrink to their tile-0 heads.  The finalize transposes the records
// tile-wise, 64 source rows at a time through LDS (k_sp_tail_pass: a count pass, the head kernel's scan and
// single reservation per row, a write pass), so every entry lands where a full-width staging row put it.
//
// HBM layout: tarena uint32[N] (tile-grouped user lists), tb int32[U x (T+1)], contributions
// (item-sorted user indices) uint32[N], epre int64[N+1] (prefix of the contributions' list
// lengths), per-row plan (W, two 64-bit tile masks), output = padded CSR (row_base, row_nnz, col,
// cnt) over per-workgroup slabs of a bump-allocated region.
//
// Three files: cooc_sparse_plan.hip (the planner: relabel, regrouping, row plans, the queue), this one (the
// walk, the compactions, k_sp_main, the split rows' finalize and its transposing tail passes; Counter::run_sparse
// and one attempt of it) and
// cooc_sparse_rows.hip (the rows that are sorted instead: k_sp_small, k_sp_tiny, and k_srb_row for the rows whose
// hash table overflowed); what they share is in cooc_sparse.h.
#include "cooc_sparse.h"
#include <algorithm>
#include <cstdio>
#include <string>
#include <type_traits>

namespace cooc {

namespace {

constexpr int kMaxProbe = 64;                          // linear probes before an insert gives up
constexpr int kSpU = 4;                                // partner loads in flight per lane

// Block-wide exclusive scan (kWaves waves); *total = the block sum.  Two barriers.
template <int kWaves>
__device__ inline uint32_t block_excl_scan(uint32_t x, uint32_t *total, uint32_t *s_wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(x);
  if (lane == 63) s_wtot[wave] = inc;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const uint32_t v = s_wtot[w];
    pre += w < wave ? v : 0u;
    tot += v;
  }
  __syncthreads();
  *total = uni(tot);
  return pre + inc - x;
}

// ---- the accumulate kernel --------------------------------------------------------------------------
struct SpShared {
  uint32_t *R;       // [kTW] dense counters | hash keys [0, H) + counts [kHashMax, kHashMax + H)
  uint32_t *L1;      // [kL1Words] hash compaction: one bit per 32-column block
  uint32_t *L1pre;   // [kL1Words] its exclusive popcount prefix
  int32_t *gb;       // [kSpDb] a segment's first 16-B group - its virtual start
  uint32_t *info;    // [kSpDb] (its end - its first group's first position) << 2 | its first id's lane
  uint32_t *vst;     // [kSpDb + 1] virtual starts
  int32_t *qstart;   // [256] first segment of every walker
};

struct SpStatic {
  uint32_t wtot[kSpWaves];
  uint64_t red[kSpWaves];
  int32_t work;
  uint32_t flag;
  int64_t slab_cur, slab_end, row_begin, row_n, pos, copy_from, copy_n;
  int64_t saved_cur, saved_end;  // the workgroup's slab while a big row fills a region of its own
  uint32_t own;
  uint32_t bstart[kSpMaxTiles + 1]; // gather mode: bucket starts in the workgroup's scratch
  uint32_t bcur[kSpMaxTiles];       // ... and fill cursors
  uint64_t ovf;                     // tiles whose bucket overflowed (their chunks walk the lists)
  unsigned long long rsum;          // the current whole row's compacted counts, summed (row-sum check)
#ifdef COOC_SP_STATS
  unsigned long long st[64];
#endif
};

// Insert the (up to 4) partner ids of one 16-B group into the LDS table (keys store id + 1; 0 =
// empty), linear probing from a multiplicative hash.  The ids are probed in lockstep so that their
// LDS round trips overlap; each probe is one returning compare-and-swap (it claims an empty slot or
// returns the key that holds it) followed, on a hit, by a non-returning count add.  An id that finds
// no slot within kMaxProbe probes raises the overflow flag (the chunk is redone with a larger table);
// the planner sizes tables at <= 1/2 fill, so probe chains stay short.
__device__ inline void sp_hash_insert4(uint32_t *keys, uint32_t *cnts, const uint4 &v, uint32_t hshift, uint32_t hmask,
                                       SpStatic &S_) {
  uint32_t k[4] = {v.x + 1u, v.y + 1u, v.z + 1u, v.w + 1u};  // kSink + 1 == 0: a pad is never inserted
  uint32_t h[4];
#pragma unroll
  for (int i = 0; i < 4; i++) h[i] = (k[i] - 1u) * 0x9E3779B1u >> hshift;
#ifdef COOC_SP_STATS
  if (threadIdx.x == 0) S_.st[24] += (k[0] != 0u) + (k[1] != 0u) + (k[2] != 0u) + (k[3] != 0u);
#endif
  for (int p = 0; p < kMaxProbe; p++) {
#ifdef COOC_SP_STATS
    if (threadIdx.x == 0) S_.st[25] += 1;
#endif
    uint32_t cur[4];
#pragma unroll
    for (int i = 0; i < 4; i++) cur[i] = k[i] ? atomicCAS(keys + h[i], 0u, k[i]) : 0u;
    bool left = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (!k[i]) continue;
      if (cur[i] == 0u || cur[i] == k[i]) {
        atomicAdd(cnts + h[i], 1u);
        k[i] = 0u;
      } else {
        h[i] = (h[i] + 1u) & hmask;
        left = true;
      }
    }
    if (!left) return;
  }
  S_.flag = 1u;
}

// what a walk does with an id.  A batch's walk (sp_walk_batch) takes it as a template parameter, so its loop
// holds one apply body and no branch on the mode; sp_walk picks the instantiation once per batch (uniform)
constexpr int kWalkDense = 0;   // dense counters R[id - c0], c0 = the chunk's one tile
constexpr int kWalkHash = 1;    // hash insert
constexpr int kWalkGather = 2;  // tile 0 (arena0) dense, the other tiles (arena1) to their buckets
struct WalkOp {
  int mode;
  uint32_t hshift, hmask;  // hash mode: the table's size
  int64_t sbase;           // gather: the workgroup's scratch (16-B groups)
#ifdef COOC_SP_STATS
  bool split;     // a split share's walk: its tile-0 and tail list walks are clocked apart (st[56], st[57])
#endif
};

// Bits [kOff, kOff + kW) of w, as one v_bfe_u32 the compiler does not look into.  Written as shifts and a
// mask, an LDS word index is merged with its scaling into (w << a) & b, and the array's LDS base (a dynamic
// shared array's: not a constant the instruction's offset field could take) costs a v_add_u32 per id; behind
// the field extract the base rides on the scaling (v_lshl_add_u32).
template <int kOff, int kW>
__device__ inline uint32_t sp_bits(uint32_t w) {
  uint32_t r;
  asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(r) : "v"(w), "n"(kOff), "n"(kW));
  return r;
}

// The dense add of the id in bits [kSh, kSh + 16) of w (arena0's u16 ids; kSh = 0 also takes a whole u32 id)
// with addend bit (0 or 1: the id's bit of the lane mask), unconditionally: an id outside the segment adds 0.
// The counter is the id's low kTShift bits (c0 is a multiple of kTW, an id of the segment lies in
// [c0, c0 + kTW)), which also keeps a masked id's address (a neighbouring tile's id, a 0xFFFF.. pad) inside
// the counter array without a compare.
// u32 counters, or (mid shapes) u16 counters packed two per word: the odd column's addend is bit << 16.
template <class Sh, int kSh>
__device__ inline void sp_dense_add_bit(uint32_t *R, uint32_t w, uint32_t bit) {
  if (Sh::kU16)
    atomicAdd(&R[sp_bits<kSh + 1, kTShift - 1>(w)], bit << (((w >> kSh) & 1u) << 4));
  else
    atomicAdd(&R[sp_bits<kSh, kTShift>(w)], bit);
}

// One 16-B group of kIds partner ids (kIds = 4: u32 ids of arena1 or a gather bucket; 8: u16 tile-0 ids
// of arena0); m = the lanes (bits 0 .. kIds - 1) inside the walked segment, the others are ids of a
// neighbouring tile range or list (or end-of-list pads) and take no part.  Segments are exact and the pads lie
// outside every one, so the dense and gather modes go by m alone; the hash mode rewrites the masked ids to
// kSink, which its insert skips.  Gather mode: arena0 holds tile-0 ids only (the dense add), arena1 none of
// them (every id is appended to its tile's bucket, 4-B ids, packed).
template <class Sh, int kIds, int kMode>
__device__ inline void sp_apply_group(const SpArgs &A, const SpShared &L, SpStatic &S_, const WalkOp &op,
                                      const uint4 &v, uint32_t m) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if (kMode == kWalkHash) {
    uint32_t x[kIds];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (kIds == 4) {
        x[i] = w[i];
      } else {
        x[2 * i] = w[i] & 0xFFFFu;
        x[2 * i + 1] = w[i] >> 16;
      }
    }
#pragma unroll
    for (int i = 0; i < kIds; i++)
      if (!((m >> i) & 1u)) x[i] = kSink;
#pragma unroll
    for (int h = 0; h < kIds; h += 4)
      sp_hash_insert4(L.R, L.R + Sh::kHashMax, make_uint4(x[h], x[h + 1], x[h + 2], x[h + 3]), op.hshift, op.hmask, S_);
  } else if (kMode == kWalkGather && kIds == 4) {
    uint32_t *scr = reinterpret_cast<uint32_t *>(A.scratch + op.sbase);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (!((m >> i) & 1u)) continue;
      const uint32_t t = w[i] >> kTShift;  // (>= 1; bucket 0 has no room)
      const uint32_t slot = atomicAdd(&S_.bcur[t], 1u);
      if (slot < S_.bstart[t + 1] - S_.bstart[t]) scr[S_.bstart[t] + slot] = w[i];  // else the bucket overflowed
    }
  } else if (kIds == 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) sp_dense_add_bit<Sh, 0>(L.R, w[i], (m >> i) & 1u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      sp_dense_add_bit<Sh, 0>(L.R, w[i], (m >> (2 * i)) & 1u);
      sp_dense_add_bit<Sh, 16>(L.R, w[i], (m >> (2 * i + 1)) & 1u);
    }
  }
}

// One batch of segments: this thread's segment (tid < nb) is the ids at positions [s, e) of ar (16-B
// groups of kIds ids; a segment starts and ends anywhere inside a group).  The segments' group counts
// are block-scanned into virtual starts; walkers of S lanes (S from the mean segment length) own equal
// contiguous shares of the virtual range and step S groups at a time, kSpU loads in flight per lane,
// applying op to every id of the segment (lanes outside it masked).  Returns the batch's groups
// (uniform); ends with a barrier.
template <class Sh, int kIds, int kMode>
__device__ inline uint32_t sp_walk_batch(const SpArgs &A, const SpShared &L, SpStatic &S_, const uint4 *__restrict__ ar,
                                         int64_t nsrc, int nb, uint32_t s, uint32_t e, const WalkOp &op) {
  constexpr uint32_t kSh = kIds == 8 ? 3u : 2u, kLo = kIds - 1;
  const int tid = threadIdx.x;
  const unsigned long long c_b0 = STAT_CLOCK();
  const uint32_t len = (tid < nb && e > s) ? ((e + kLo) >> kSh) - (s >> kSh) : 0u;
  uint32_t total;
  const uint32_t ex = block_excl_scan<Sh::kWaves>(len, &total, S_.wtot);
  if (total == 0) return 0;  // uniform (scalar branch): no barrier is skipped by part of the block
  const uint32_t mean = total / uint32_t(nb);
#ifndef COOC_SP_SLONG
#define COOC_SP_SLONG 64u  // whole-wave walkers for long segments: 1.2% faster than 16 (profiles/r03/walker_ab)
#endif
#ifndef COOC_SP_SSHORT
#define COOC_SP_SSHORT 4u
#endif
#ifndef COOC_SP_STIER
#define COOC_SP_STIER 32  // segments of >= 32 groups: whole-wave walkers, >= 12: 16 lanes (profiles/r03/walker_ab)
#endif
  const uint32_t S = mean >= COOC_SP_STIER ? COOC_SP_SLONG : mean >= 12 ? 16u : COOC_SP_SSHORT;
  const uint32_t nW = uint32_t(Sh::kThreads) / S;
  if (tid < nb) {
    L.vst[tid] = ex;
    L.gb[tid] = int32_t(s >> kSh) - int32_t(ex);
    L.info[tid] = ((e - (s & ~kLo)) << 3) | (s & kLo);
    if (len) {
      const uint32_t q0 = uint32_t((uint64_t(ex) * nW + total - 1) / total);
      const uint32_t q1 = uint32_t((uint64_t(ex + len) * nW + total - 1) / total);
      for (uint32_t q = q0; q < q1 && q < nW; q++) L.qstart[q] = tid;
    }
  }
  if (tid == 0) L.vst[nb] = total;
  __syncthreads();
  const unsigned long long c_b1 = STAT_CLOCK();
  if (kMode == kWalkHash) STAT_ADD(16, c_b1 - c_b0);
  if (kMode == kWalkHash) STAT_ADD(18, total);
  const uint32_t q = uint32_t(tid) / S, ql = uint32_t(tid) % S;
  const uint32_t lo = uint32_t(uint64_t(total) * q / nW), hi = uint32_t(uint64_t(total) * (q + 1) / nW);
  uint32_t g = lo + ql;
  if (g < hi) {
    int32_t cur = L.qstart[q];
    uint32_t vs = L.vst[cur], next = L.vst[cur + 1], inf = L.info[cur];
    int32_t gb = L.gb[cur];
    // the group at virtual index gk of the current segment, and its in-segment lanes
    auto fetch = [&](uint32_t gk, uint4 &v, uint32_t &m) {
      while (gk >= next) {
        cur++;
        vs = next;
        next = L.vst[cur + 1];
        gb = L.gb[cur];
        inf = L.info[cur];
      }
      const int64_t gi = int64_t(gb) + int64_t(gk);
      const uint32_t qq = gk - vs;
      const uint32_t lo_l = qq ? 0u : (inf & 7u);
      const int32_t hi_l = min(int32_t(kIds), int32_t(inf >> 3) - int32_t(kIds) * int32_t(qq));
      m = ((1u << hi_l) - 1u) & ~((1u << lo_l) - 1u);
      v = SP_CHECK(A, gi >= 0 && gi < nsrc) ? ar[gi] : make_uint4(kSink, kSink, kSink, kSink);
    };
    uint4 v[kSpU] = {};
    uint32_t m = 0;  // 8 lane bits per group in flight
#ifdef COOC_SP_STATS
    const unsigned long long c_issue = STAT_CLOCK();
    bool first_seen = false;
#endif
#pragma unroll
    for (int k = 0; k < kSpU; k++) {
      const uint32_t gk = g + S * k;
      uint32_t mk = 0;
      if (gk < hi) fetch(gk, v[k], mk);
      m |= mk << (8 * k);
    }
    for (; g < hi; g += S * kSpU) {
      uint4 vn[kSpU] = {};
      uint32_t mn = 0;
#pragma unroll
      for (int k = 0; k < kSpU; k++) {
        const uint32_t gk = g + S * (kSpU + k);
        uint32_t mk = 0;
        if (gk < hi) fetch(gk, vn[k], mk);
        mn |= mk << (8 * k);
      }
#pragma unroll
      for (int k = 0; k < kSpU; k++) {
        const uint32_t mk = (m >> (8 * k)) & 255u;
        if (mk) sp_apply_group<Sh, kIds, kMode>(A, L, S_, op, v[k], mk);
#ifdef COOC_SP_STATS
        if (kMode == kWalkHash && k == 0 && !first_seen) {  // thread 0: the first group's data arrived and was applied
          first_seen = true;
          if (threadIdx.x == 0) {
            S_.st[54] += STAT_CLOCK() - c_issue;
            S_.st[55] += 1;
          }
        }
#endif
      }
#pragma unroll
      for (int k = 0; k < kSpU; k++) v[k] = vn[k];
      m = mn;
    }
  }
  __syncthreads();
  if (kMode == kWalkHash) STAT_ADD(17, STAT_CLOCK() - c_b1);
  return total;
}

// Walk the partner ids of contributions [k0, k1) restricted to tiles [t0, t1) (full: whole lists),
// applying op to every id: the tile-0 part of the lists from arena0 (u16, 8 ids per load), the rest from
// arena1 (u32), a batch of kSpDb contributions at a time.  bucket (gather mode's tile ranges): the one batch
// of the filled parts of tiles [t0, t1)'s buckets in the workgroup's scratch instead, k0 and k1 unused.
// Every batch walk of the kernel is instantiated here, once per id width and mode.  Returns the groups walked.
template <class Sh>
__device__ inline uint64_t sp_walk(const SpArgs &A, const SpShared &L, SpStatic &S_, int64_t k0, int64_t k1, int t0,
                                   int t1, bool full, bool bucket, const WalkOp &op) {
  uint64_t walked = 0;
  const int tid = threadIdx.x;
  const bool okt = SP_CHECK(A, t0 >= 0 && t1 <= A.T && t0 <= t1);
  const bool has0 = !bucket && (full || t0 == 0);    // (uniform)
  const int ta = full ? 1 : max(t0, 1), tz = full ? A.T : t1;
  const bool has1 = bucket || tz > ta;
  if (bucket) {
    k0 = 0;
    k1 = t1 - t0;
  }
  const uint4 *const ar1 = bucket ? A.scratch + op.sbase : A.tarena;
  const int64_t nsrc1 = bucket ? A.scr_cap : A.n_groups;
  // whole lists and tile-0 parts take their bounds from the compact records, read one batch ahead: batch
  // b0's records were loaded before batch b0 - kDb was walked, and its list indices a batch before that,
  // so only the first batch of a walk waits for its two dependent loads (a sub-range of the tail reads tb).
  // The read-ahead holds 5 VGPRs over the walk: the mid shapes have them, the big shape, at its 128 already,
  // would spill them (kAhead false: its records are loaded at the head of each batch)
  const bool rec = !bucket && A.tbc && (full || (t0 == 0 && !has1));  // (uniform)
  constexpr uint32_t kNoList = 0xFFFFFFFFu;
  auto list_of = [&](int64_t b) -> uint32_t {  // this thread's list of the batch at b
    if (b + tid >= k1 || !okt) return kNoList;
    const uint32_t u = SP_CHECK(A, b + tid < A.n_contrib) ? A.vals[b + tid] & kListMask : 0u;
    return SP_CHECK(A, u < A.n_users) ? u : 0u;
  };
  auto rec_of = [&](uint32_t u) -> int4 { return u != kNoList ? A.tbc[u] : make_int4(0, 0, 0, 0); };
  int4 rn = make_int4(0, 0, 0, 0);
  uint32_t un = kNoList;
  static_assert(Sh::kDb == Sh::kThreads, "a batch: one contribution per thread");
  if (rec && Sh::kAhead) {
    const uint32_t u0 = list_of(k0);
    un = list_of(k0 + Sh::kDb);
    rn = rec_of(u0);
  }
  for (int64_t b0 = k0; b0 < k1; b0 += Sh::kDb) {
    const int nb = int(min<int64_t>(Sh::kDb, k1 - b0));
    uint32_t s0 = 0, e0 = 0, s1 = 0, e1 = 0;
    STAT_ADD(19, op.mode == kWalkHash && !bucket ? 1 : 0);
    if (bucket) {
      if (tid < nb) {
        s1 = S_.bstart[t0 + tid];
        e1 = s1 + S_.bcur[t0 + tid];
      }
    } else if (rec) {
      if (!Sh::kAhead) rn = rec_of(list_of(b0));
      s0 = uint32_t(rn.x);
      e0 = uint32_t(rn.y);
      if (has1) {
        s1 = uint32_t(rn.z);
        e1 = uint32_t(rn.w);
      }
      if (Sh::kAhead) {
        rn = rec_of(un);  // (in flight over this batch's walk)
        un = list_of(b0 + 2 * Sh::kDb);
      }
    } else if (tid < nb && okt) {
      const uint32_t u = SP_CHECK(A, b0 + tid < A.n_contrib) ? A.vals[b0 + tid] & kListMask : 0u;
      const int32_t *tbu = A.tb + int64_t(SP_CHECK(A, u < A.n_users) ? u : 0u) * (A.T + 2);
      if (has0) {
        s0 = uint32_t(tbu[0]);
        e0 = uint32_t(tbu[A.T + 1]);
      }
      if (has1) {
        s1 = uint32_t(tbu[ta]);
        e1 = uint32_t(tbu[tz]);
      }
    }
    const unsigned long long c_w0 = STAT_CLOCK();
    if (has0) {  // (gather mode: arena0 is tile 0 only, the dense add)
      if (op.mode == kWalkHash)
        walked += sp_walk_batch<Sh, 8, kWalkHash>(A, L, S_, A.tarena0, A.n_groups0, nb, s0, e0, op);
      else
        walked += sp_walk_batch<Sh, 8, kWalkDense>(A, L, S_, A.tarena0, A.n_groups0, nb, s0, e0, op);
    }
    const unsigned long long c_w1 = STAT_CLOCK();
    if (has1) {
      if (op.mode == kWalkHash)
        walked += sp_walk_batch<Sh, 4, kWalkHash>(A, L, S_, ar1, nsrc1, nb, s1, e1, op);
      else if (op.mode == kWalkGather)
        walked += sp_walk_batch<Sh, 4, kWalkGather>(A, L, S_, ar1, nsrc1, nb, s1, e1, op);
      else
        walked += sp_walk_batch<Sh, 4, kWalkDense>(A, L, S_, ar1, nsrc1, nb, s1, e1, op);
    }
#ifdef COOC_SP_STATS
    if (op.split) {
      STAT_ADD(56, c_w1 - c_w0);
      STAT_ADD(57, STAT_CLOCK() - c_w1);
    }
#endif
    if (uni(S_.flag)) break;
  }
  return walked;
}

// Global stores of this workgroup made visible to its own later global loads.  __syncthreads() only
// drains LDS traffic (s_waitcnt lgkmcnt(0)), and the CU's vector L1 is write-through without
// keeping its lines in step with later stores: a line loaded earlier -- by this workgroup, or by the
// other workgroup resident on the CU reading its own data next to ours -- can still hold what the
// line had before.  So every wave waits for all its memory operations (s_waitcnt 0), the barrier,
// then the L1 is invalidated (agent-scope acquire: buffer_inv sc1) and the loads that follow read
// the XCD's L2, where the stores are.  Used where the kernel reads back what it wrote: a row moving
// to a new slab, the gather buckets.
__device__ inline void sp_global_sync() {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// Output space for n more entries of the current row (thread-uniform call).  Moves the row's
// entries so far to a new slab when the workgroup's slab is exhausted.  Returns the write position
// (-1 when the output region is exhausted: the host reruns with a larger region).
template <class Sh>
__device__ inline int64_t sp_reserve(const SpArgs &A, SpStatic &S_, int64_t n) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    S_.copy_n = 0;
    if (S_.slab_cur + n > S_.slab_end) {
      const int64_t need = S_.row_n + n;
      const int64_t take = max(A.slab, need + need / 2);  // a growing row moves O(log) times
      int64_t b = int64_t(atomicAdd(A.bump, (unsigned long long)take));
      if (b + take > A.cap) {
        atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 4ull);
        S_.pos = -1;
      } else {
        S_.copy_from = S_.row_begin;
        S_.copy_n = S_.row_n;
        S_.row_begin = b;
        S_.slab_cur = b + S_.row_n;
        S_.slab_end = b + take;
        S_.pos = S_.slab_cur;
        S_.slab_cur += n;
      }
    } else {
      S_.pos = S_.slab_cur;
      S_.slab_cur += n;
    }
    if (S_.pos >= 0) S_.row_n += n;
  }
  __syncthreads();
  const int64_t cn = uni(S_.copy_n);
  if (cn > 0) {  // the row's earlier entries follow it to the new slab (rare)
    sp_global_sync();  // they were just stored by other waves
    const int64_t from = S_.copy_from, to = S_.row_begin;
    for (int64_t i = tid; i < cn; i += Sh::kThreads) {
      if (SP_CHECK(A, to + i < A.cap && from + i < A.cap && from >= 0)) {
        A.col_out[to + i] = A.col_out[from + i];
        A.cnt_out[to + i] = A.cnt_out[from + i];
      }
    }
  }
  return uni(S_.pos);
}

// Column-order compaction of w dense counters (16-B aligned), appended to the row's output; the
// counters are left zero.  Waves own (64 kPer)-column-aligned ranges.  The count sweep reads kPer counters per
// lane (one 16-B LDS read: 4 u32 counters, or 8 u16 ones in the mid shape); the write sweep one LDS word per
// lane and sub-step, neighbouring lanes neighbouring columns (see there).
template <class Sh>
__device__ inline void sp_dense_compact(const SpArgs &A, const SpShared &L, SpStatic &S_, int32_t w, int32_t c0,
                                        uint64_t &rsum, uint32_t *mdst) {
  constexpr int kPer = Sh::kPer, kStep = 64 * kPer;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long c_d0 = STAT_CLOCK();
  uint32_t *row = L.R;
  // a mirror source's tile 0 (mdst = the row's record): its counts at the split rows' columns are those rows'
  // entries at column ra.  A short pass of its own ahead of the sweep (the counters are final, and cleared only
  // behind the sweep's first barrier), a thread per slot: the slot's column from srank (no dependent load in front
  // of the store), the whole record in a few coalesced stores, zero cells included (whole 64-B lines; the
  // finalize skips them as it skips the untouched ones)
  if (mdst) {
    for (int32_t sl = tid; sl < A.n_split; sl += Sh::kThreads) {
      const int32_t i = A.srank[sl];
      if (i < w) mdst[sl] = Sh::kU16 ? (row[i >> 1] >> ((i & 1) << 4)) & 0xFFFFu : row[i];
    }
  }
  const int32_t per = ((w + Sh::kWaves - 1) / Sh::kWaves + kStep - 1) & ~(kStep - 1);
  const int32_t lo = min(w, wave * per), hi = min(w, lo + per);
  const uint4 *row4 = reinterpret_cast<const uint4 *>(row);
  auto load = [&](int32_t b, uint32_t v[kPer]) {  // counters b .. b + kPer - 1 (b a multiple of kPer)
    if (b < hi) {
      const uint4 q = row4[b / kPer];
      const uint32_t ww[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        const uint32_t x = Sh::kU16 ? (ww[k >> 1] >> (16 * (k & 1))) & 0xFFFFu : ww[k & 3];
        v[k] = b + k < hi ? x : 0u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPer; k++) v[k] = 0u;
    }
  };
  uint32_t cnt = 0;
  for (int32_t b0 = lo; b0 < hi; b0 += kStep) {
    uint32_t v[kPer];
    load(b0 + kPer * lane, v);
#pragma unroll
    for (int k = 0; k < kPer; k++) cnt += v[k] != 0u;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) S_.wtot[wave] = cnt;
  __syncthreads();
  STAT_ADD(48, STAT_CLOCK() - c_d0);
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int wv = 0; wv < Sh::kWaves; wv++) {
    const uint32_t x = S_.wtot[wv];
    off += wv < wave ? x : 0u;
    tot += x;
  }
  // The write sweep takes a wave step's 64 kPer columns interleaved: in sub-step k lane l holds ONE LDS word, the
  // counter of column b0 + 64 k + l (u32) or the counters of columns b0 + 2 (64 k + l) and the next (u16), so
  // neighbouring lanes hold neighbouring columns, an entry's position is the step's offset + the ballot's bits
  // below the lane, and the active lanes of a store write one contiguous run (the lane-owns-kPer-columns
  // mapping of the count sweep left them 4 c bytes apart, c = the lane's non-zero count).  Entry order is
  // (wave range, step, sub-step, lane) = ascending column, every entry where the count sweep's mapping puts it.
  // After a relabel the output ids of tile 0 are hot_col[b]: the word's ids, one coalesced 4-B (u32) or 8-B
  // (u16) load per lane and sub-step, a whole step ahead (the first step's overlap the reservation); above tile 0
  // they are c0 + b - kTW.  The sweep exists once per case: a load's wait counts the stores issued since as well,
  // and behind exec-masked stores that count is unknown, so the id loads cost one full drain per step -- which
  // the sweep without them (kept ids, tiles above 0) does not pay
  const bool map = A.hot_col != nullptr && c0 == 0;
  constexpr int kW = Sh::kU16 ? 2 : 1, kSub = kPer / kW;  // columns per LDS word; sub-steps per step
  const int32_t cshift = c0 - (A.hot_col ? kTW : 0);
  uint32_t nxt[kSub][kW];
  auto colq = [&](int32_t b0, bool on) {  // the ids of the step at b0
#pragma unroll
    for (int k = 0; k < kSub; k++) {
      const int32_t b = b0 + kW * (64 * k + lane);
      if (Sh::kU16) {
        const uint2 t = (on && b < hi) ? *reinterpret_cast<const uint2 *>(A.hot_col + b) : make_uint2(0u, 0u);
        nxt[k][0] = t.x;
        nxt[k][kW - 1] = t.y;
      } else {
        nxt[k][0] = (on && b < hi) ? uint32_t(A.hot_col[b]) : 0u;
      }
    }
  };
  colq(lo, map);
  const int64_t base = sp_reserve<Sh>(A, S_, tot);  // (barrier: every wave has read wtot)
  STAT_ADD(49, STAT_CLOCK() - c_d0);
  off = uni(off);  // (the same in every lane of the wave: kept in a scalar register from here on)
  auto sweep = [&](auto mapped) {
    constexpr bool kMap = decltype(mapped)::value;
    for (int32_t b0 = lo; b0 < hi; b0 += kStep) {
      uint32_t word[kSub], ids[kSub][kW] = {};  // (ids: the mapped sweep only)
#pragma unroll
      for (int k = 0; k < kSub; k++) {
        const int32_t b = b0 + kW * (64 * k + lane);
        word[k] = b < hi ? row[b / kW] : 0u;
      }
      if constexpr (kMap) {
#pragma unroll
        for (int k = 0; k < kSub; k++)
#pragma unroll
          for (int j = 0; j < kW; j++) ids[k][j] = nxt[k][j];
        // the step's one drain, here for every lane: left to the first use, it would sit inside a sub-step's
        // exec-masked stores and be repeated in every sub-step after it (vmcnt 0; the other counters untouched)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        colq(b0 + kStep, true);
      }
#pragma unroll
      for (int k = 0; k < kSub; k++) {
        const int32_t b = b0 + kW * (64 * k + lane);
        // (a u16 word's odd column may lie past hi: masked as in the count sweep, though no id reaches it)
        const uint32_t x0 = Sh::kU16 ? word[k] & 0xFFFFu : word[k];
        const uint32_t x1 = (Sh::kU16 && b + 1 < hi) ? word[k] >> 16 : 0u;
        const uint64_t m0 = __ballot(x0 != 0u), m1 = Sh::kU16 ? __ballot(x1 != 0u) : 0ull;
        uint32_t pre = __builtin_amdgcn_mbcnt_hi(uint32_t(m0 >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m0), 0u));
        if (Sh::kU16) pre = __builtin_amdgcn_mbcnt_hi(uint32_t(m1 >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m1), pre));
        rsum += x0 + x1;
        if (word[k]) {
          // (the step's position is wave-uniform: scalar base + the lane's 32-bit offset, no 64-bit lane math)
          const int64_t pos = base + off;
          int32_t *const cp = A.col_out + pos;
          uint32_t *const np = A.cnt_out + pos;
          const uint32_t pre1 = pre + (x0 != 0u);
          if (base >= 0) {
            if (x0 && SP_CHECK(A, pos >= 0 && pos + pre < A.cap)) {
              cp[pre] = kMap ? int32_t(ids[k][0]) : cshift + b;
              np[pre] = x0;
            }
            if (Sh::kU16 && x1 && SP_CHECK(A, pos >= 0 && pos + pre1 < A.cap)) {
              cp[pre1] = kMap ? int32_t(ids[k][kW - 1]) : cshift + b + 1;
              np[pre1] = x1;
            }
          }
          row[b / kW] = 0u;
        }
        off += uint32_t(__popcll(m0)) + uint32_t(__popcll(m1));
      }
    }
  };
  if (map)
    sweep(std::true_type{});
  else
    sweep(std::false_type{});
  STAT_ADD(50, STAT_CLOCK() - c_d0);
  __syncthreads();
  STAT_ADD(51, STAT_CLOCK() - c_d0);
}

// Column-order compaction of the hash table (H slots) of the column range [c0, c1), appended to the
// row's output; leaves the table, L1 and the scratch it uses zero.  Entries are kept in registers
// (H / kThreads <= 16 per thread); their 32-column blocks are ranked through the L1 bitmap, every
// block gets a 32-bit column mask (in the keys area) and a base (prefix of mask popcounts, in the
// counts area); an entry goes to base + popcount(mask below its column).
template <class Sh>
__device__ inline void sp_hash_compact(const SpArgs &A, const SpShared &L, SpStatic &S_, int32_t H, int32_t c0,
                                       int32_t c1, uint64_t &rsum, uint32_t *mdst) {
  // (the thread index behind an opaque move: the LDS and store addresses the compaction derives from it are computed
  // here, per chunk, instead of being hoisted out of the workgroup loop and held in VGPRs over the whole kernel)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned long long c_h0 = STAT_CLOCK();
  // (mdst: a mirror source's chunk from tile 0 on -- the entries at the split rows' columns also go to the row's
  // record of mirrored cells, from the table sweep that both emission orders share)
  const uint32_t mhi = mdst ? uint32_t(A.mirror_hi) : 0u;
  uint32_t *keys = L.R, *cnts = L.R + Sh::kHashMax;
  const int per = H / Sh::kThreads;
  const int32_t nL1 = (c1 - c0 + 1023) >> 10;
  uint32_t ek[Sh::kHashMax / Sh::kThreads], ec[Sh::kHashMax / Sh::kThreads], er[Sh::kHashMax / Sh::kThreads];
  // the table swept 4 slots (16 B) per LDS access: thread tid takes slots 4 (tid + q kThreads) .. + 3
  (void)per;
#pragma unroll
  for (int q = 0; q < Sh::kHashMax / (4 * Sh::kThreads); q++) {
    const int j = 4 * (tid + q * Sh::kThreads);
    uint4 k4 = make_uint4(0u, 0u, 0u, 0u), v4 = k4;
    if (j < H) {
      k4 = *reinterpret_cast<const uint4 *>(keys + j);
      v4 = *reinterpret_cast<const uint4 *>(cnts + j);
      *reinterpret_cast<uint4 *>(keys + j) = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4 *>(cnts + j) = make_uint4(0u, 0u, 0u, 0u);
    }
    const uint32_t kk[4] = {k4.x, k4.y, k4.z, k4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = 4 * q + u;
      ek[i] = ~0u;
      ec[i] = 0u;
      er[i] = 0u;
      if (kk[u] && vv[u]) {
        const uint32_t col = kk[u] - 1u - uint32_t(c0);
        ek[i] = col;
        ec[i] = vv[u];
        rsum += vv[u];
        if (col < mhi) {
          const int32_t sl = A.mslot[col];
          if (sl >= 0) mdst[sl] = vv[u];  // (the record's cell)
        }
        if (Sh::kRank && !A.any_order) atomicOr(&L.L1[col >> 10], 1u << ((col >> 5) & 31u));
      }
    }
  }
  // COOC_FLAG_ANY_ORDER: the entries leave from the registers, in the order (wave, register index, lane).  No scan
  // over lanes and no staging in LDS: in sub-step i the wave takes the ballot of "register entry i is valid", an
  // entry's position is the wave's offset + the ballot's bits below its lane (v_mbcnt), the active lanes of a store
  // write one contiguous run, and the offset advances by the ballot's popcount (as sp_dense_compact's write sweep).
  const bool any = !Sh::kRank || A.any_order;
  constexpr int kE = Sh::kHashMax / Sh::kThreads;  // register entries per thread
  if (any) {  // the wave's entry count: kE ballots, their popcounts added in a scalar
    uint32_t wc = 0;
#pragma unroll
    for (int i = 0; i < kE; i++) wc += uint32_t(__popcll(__ballot(ek[i] != ~0u)));
    if ((tid & 63) == 0) S_.wtot[tid >> 6] = wc;
  }
  __syncthreads();  // the table is cleared (and: the L1 bits are set | the waves' counts are in wtot)
  STAT_ADD(46, STAT_CLOCK() - c_h0);
  if (any) {
    const int wave = tid >> 6;
    uint32_t off = 0, ne = 0;
#pragma unroll
    for (int wv = 0; wv < Sh::kWaves; wv++) {
      const uint32_t x = S_.wtot[wv];
      off += wv < wave ? x : 0u;
      ne += x;
    }
    ne = uni(ne);
    // after a relabel the ids of a chunk from tile 0 on are hot_col[column] below kTW and column - kTW above: looked
    // up in place (the entry's register takes the id), every load issued here, ahead of the reservation and of every
    // store -- an id loaded between exec-masked stores would be waited for with a full drain at each use.  The
    // write exists once per case behind one uniform branch, so the one without lookups has no load to wait for.
    const bool map = A.hot_col != nullptr && c0 == 0;
    if (map) {
#pragma unroll
      for (int i = 0; i < kE; i++) {
        const uint32_t c = ek[i];
        if (c != ~0u) ek[i] = c < uint32_t(kTW) ? uint32_t(A.hot_col[c]) : c - uint32_t(kTW);
      }
    }
    const unsigned long long c_a1 = STAT_CLOCK();
    STAT_ADD(20, c_a1 - c_h0);
    const int64_t base = sp_reserve<Sh>(A, S_, ne);  // (barrier: every wave has read wtot)
    const unsigned long long c_a2 = STAT_CLOCK();
    STAT_ADD(21, c_a2 - c_a1);
    off = uni(off);  // (the same in every lane of the wave: kept in a scalar register from here on)
    const uint32_t cshift = uint32_t(c0) - (A.hot_col ? uint32_t(kTW) : 0u);
    // the chunk's two output positions, in scalar registers of their own: read as fields of the kernel's argument
    // block in every sub-step, the block's spilled 16-register tuple was restored (14 v_readlane) in each of them
    // (named global: behind the opaque move the pointers' address space is no longer inferred, and the stores were flat)
    using gi32 = __attribute__((address_space(1))) int32_t;
    using gu32 = __attribute__((address_space(1))) uint32_t;
    gi32 *co = (gi32 *)(A.col_out + max<int64_t>(base, int64_t(0)));
    gu32 *cn = (gu32 *)(A.cnt_out + max<int64_t>(base, int64_t(0)));
    asm volatile("" : "+s"(co), "+s"(cn));
    auto write = [&](auto mapped) {
      constexpr bool kMap = decltype(mapped)::value;
      if constexpr (kMap) __builtin_amdgcn_s_waitcnt(0x0F70);  // the ids' one drain (vmcnt 0), here for every lane
#pragma unroll
      for (int i = 0; i < kE; i++) {
        const bool on = ek[i] != ~0u;
        const uint64_t m = __ballot(on);
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
        // (the sub-step's position is wave-uniform: scalar base + the lane's 32-bit offset, no 64-bit lane math)
        const int64_t pos = base + off;
        (void)pos;
        if (on && SP_CHECK(A, pos >= 0 && pos + pre < A.cap)) {
          (co + off)[pre] = int32_t(kMap ? ek[i] : cshift + ek[i]);
          (cn + off)[pre] = ec[i];
        }
        off += uint32_t(__popcll(m));
        // (the sub-steps stay apart in the schedule: each needs only its own offset and id at a time)
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (base >= 0) {  // (region exhausted: no stores, the host repeats the attempt)
      if (map)
        write(std::true_type{});
      else
        write(std::false_type{});
    }
    // No closing barrier: the table was cleared in the sweep (published by the barrier above) and nothing else in
    // LDS was written.  wtot is read between that barrier and sp_reserve's, pos behind sp_reserve's; both are next
    // written behind the barrier that opens the next chunk's walk (or ends the row), which every wave reaches
    // after its reads.
    STAT_ADD(22, STAT_CLOCK() - c_a2);
    STAT_ADD(23, ne);
    return;
  }
  if constexpr (Sh::kRank) {
  uint32_t nblk;
  {
    static_assert(Sh::kL1Words % Sh::kThreads == 0, "L1 words per thread");
    constexpr int kW = Sh::kL1Words / Sh::kThreads;  // consecutive L1 words per thread
    uint32_t pc[kW], x = 0;
#pragma unroll
    for (int i = 0; i < kW; i++) {
      pc[i] = kW * tid + i < nL1 ? uint32_t(__popc(L.L1[kW * tid + i])) : 0u;
      x += pc[i];
    }
    const uint32_t p = block_excl_scan<Sh::kWaves>(x, &nblk, S_.wtot);
    uint32_t run = p;
#pragma unroll
    for (int i = 0; i < kW; i++) {
      if (kW * tid + i < nL1) L.L1pre[kW * tid + i] = run;
      run += pc[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < Sh::kHashMax / Sh::kThreads; i++) {
    if (ek[i] == ~0u) continue;
    const uint32_t col = ek[i], wd = col >> 10, bit = (col >> 5) & 31u;
    const uint32_t r = L.L1pre[wd] + uint32_t(__popc(L.L1[wd] & ((1u << bit) - 1u)));
    er[i] = r;
    atomicOr(&keys[r], 1u << (col & 31u));
  }
  __syncthreads();
  STAT_ADD(47, STAT_CLOCK() - c_h0);
  const uint32_t pb = (nblk + Sh::kThreads - 1) / Sh::kThreads;
  const uint32_t r0 = min(nblk, uint32_t(tid) * pb), r1 = min(nblk, r0 + pb);
  uint32_t local = 0;
  for (uint32_t r = r0; r < r1; r++) local += uint32_t(__popc(keys[r]));
  uint32_t ne;
  uint32_t run = block_excl_scan<Sh::kWaves>(local, &ne, S_.wtot);
  for (uint32_t r = r0; r < r1; r++) {
    cnts[r] = run;
    run += uint32_t(__popc(keys[r]));
  }
  const unsigned long long c_h1 = STAT_CLOCK();
  STAT_ADD(20, c_h1 - c_h0);
  const int64_t base = sp_reserve<Sh>(A, S_, ne);  // (barrier: bases visible)
  const unsigned long long c_h2 = STAT_CLOCK();
  STAT_ADD(21, c_h2 - c_h1);
  if (base >= 0 && ne <= uint32_t(Sh::kWStage)) {
    // the chunk's entries land in LDS at their sorted positions (the free upper halves of the emptied key
    // and count areas), then leave in order: 16-B stores of whole column / count runs instead of one
    // scattered 4-B store per entry and array
    uint32_t *sc = keys + Sh::kWStage, *sn = cnts + Sh::kWStage;
    // (after a relabel a column maps back by a lookup in tile 0's 64 KB table, a subtraction above)
    const bool hot0 = A.hot_col && c0 < kTW;
    const uint32_t shift = A.hot_col ? uint32_t(kTW) : 0u;
#pragma unroll
    for (int i = 0; i < Sh::kHashMax / Sh::kThreads; i++) {
      if (ek[i] == ~0u) continue;
      const uint32_t col = ek[i], r = er[i];
      const uint32_t q = cnts[r] + uint32_t(__popc(keys[r] & ((1u << (col & 31u)) - 1u)));
      const uint32_t c = uint32_t(c0) + col;
      sc[q] = hot0 && c < uint32_t(kTW) ? uint32_t(A.hot_col[c]) : c - shift;
      sn[q] = ec[i];
    }
    __syncthreads();
    const uint32_t head = min(ne, uint32_t((4 - (base & 3)) & 3));  // entries before the first 16-B boundary
    const uint32_t body = (ne - head) >> 2;
    for (uint32_t j = tid; j < head; j += Sh::kThreads) {
      A.col_out[base + j] = int32_t(sc[j]);
      A.cnt_out[base + j] = sn[j];
    }
    int4 *co4 = reinterpret_cast<int4 *>(A.col_out + base + head);
    uint4 *cn4 = reinterpret_cast<uint4 *>(A.cnt_out + base + head);
    for (uint32_t j = tid; j < body; j += Sh::kThreads) {
      const uint32_t q = head + 4 * j;
      co4[j] = make_int4(int32_t(sc[q]), int32_t(sc[q + 1]), int32_t(sc[q + 2]), int32_t(sc[q + 3]));
      cn4[j] = make_uint4(sn[q], sn[q + 1], sn[q + 2], sn[q + 3]);
    }
    for (uint32_t q = head + 4 * body + tid; q < ne; q += Sh::kThreads) {
      A.col_out[base + q] = int32_t(sc[q]);
      A.cnt_out[base + q] = sn[q];
    }
    __syncthreads();
    for (uint32_t q = tid; q < ne; q += Sh::kThreads) {  // the areas go back to zero for the next chunk
      sc[q] = 0u;
      sn[q] = 0u;
    }
  } else if (base >= 0) {
#pragma unroll
    for (int i = 0; i < Sh::kHashMax / Sh::kThreads; i++) {
      if (ek[i] == ~0u) continue;
      const uint32_t col = ek[i], r = er[i];
      const int64_t pos = base + cnts[r] + uint32_t(__popc(keys[r] & ((1u << (col & 31u)) - 1u)));
      if (SP_CHECK(A, pos >= 0 && pos < A.cap)) {
        A.col_out[pos] = sp_col(A, uint32_t(c0) + col);
        A.cnt_out[pos] = ec[i];
      }
    }
  }
  __syncthreads();
  STAT_ADD(22, STAT_CLOCK() - c_h2);
  STAT_ADD(23, ne);
  for (uint32_t r = tid; r < nblk; r += Sh::kThreads) {
    keys[r] = 0u;
    cnts[r] = 0u;
  }
  for (int32_t i = tid; i < nL1; i += Sh::kThreads) L.L1[i] = 0u;
  __syncthreads();
  }  // (Sh::kRank)
}

// The workgroup loop.  A work item is a whole row (its chunks in column order, appended to the row's
// contiguous output) or a split row's (tile, contribution share), added into the staging row.  One
// code path for every chunk kind, so that the walk and the two compactions exist once.
// The shape (SpBig: 512 threads, two workgroups per CU; SpMid: 256 threads, three per CU; SpMidAny, the any-order
// runs' mid shape without the ranking bitmaps: four per CU) fixes the LDS layout; all keep 4 waves per SIMD
// (<= 128 VGPRs).  A launch takes the queue range [A.q_begin, A.q_end).
template <class Sh>
__global__ __launch_bounds__(Sh::kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_sp_main(SpArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ SpStatic S_;
  SpShared L;
  L.R = lds;
  L.L1 = Sh::kRank ? L.R + Sh::kRWords : nullptr;  // (a shape without column ranking has no bitmaps)
  L.L1pre = Sh::kRank ? L.L1 + Sh::kL1Words : nullptr;
  L.gb = reinterpret_cast<int32_t *>(L.R + Sh::kRWords + Sh::kBmWords);
  L.info = reinterpret_cast<uint32_t *>(L.gb + Sh::kDb);
  L.vst = L.info + Sh::kDb;
  L.qstart = reinterpret_cast<int32_t *>(L.vst + Sh::kDb + 4);
  const int tid = threadIdx.x;
  for (int32_t i = tid; i < Sh::kRWords + (Sh::kRank ? Sh::kL1Words : 0); i += Sh::kThreads) L.R[i] = 0u;
  if (tid == 0) {
    S_.slab_cur = S_.slab_end = 0;
    S_.flag = 0u;
  }
  // (the queue's tail: the mid rows (the mid shape's launch), the small rows (k_sp_small), the tiny ones (k_sp_tiny))
  const int64_t n_work = A.q_end - A.q_begin;
#ifdef COOC_SP_STATS
  if (threadIdx.x < 64) S_.st[threadIdx.x] = 0ull;
  const unsigned long long t_start = STAT_CLOCK();
#endif
  if (tid == 0) S_.work = atomicAdd(A.qctr, 1);
  __syncthreads();
  uint64_t rsum = 0;  // this thread's share of the current whole row's count sum
  for (;;) {
    const int32_t w = uni(S_.work);
    if (w >= n_work) break;
    // the next item is dequeued now and read at the end of this one (its latency hides behind the work)
    uint32_t next = 0;
    if (tid == 0) next = atomicAdd(A.qctr, 1);
    const SpWork it = A.queue[A.q_begin + w];
    const int32_t a = it.row;
    const int32_t ra = sp_rank(A, a);  // the row's own column (the self term), in column-rank space
    const bool split = it.kind == -2;  // a share of a split row's contributions, every tile, into staging
    const int64_t k0 = it.k0, k1 = it.k1;
    int t = 0;
    // (a mirrored split share: tile 0 only, a plain dense chunk; the other tiles come from the transposed rows)
    const int t_end = (split && A.mirror_hi > 0) ? 1 : A.T;
    // a whole row of column rank >= kTW is a mirror source: its tile-0 chunk also stores the split rows' cells
    // (mdst: the row's record)
    uint32_t *const mdst = (!split && A.mirror_hi > 0 && ra >= kTW) ? A.mrec + int64_t(ra - kTW) * A.mrec_w : nullptr;
    const uint64_t st = it.st, dn = it.dn, hz0 = it.hz[0], hz1 = it.hz[1];
    // gather mode (rows with many chunks, split shares): the lists are walked once; tile 0 is counted
    // on the way and every other tile's groups go to a bucket that its chunk then reads contiguously
    // (instead of one walk of every contribution per chunk).  Off when the tails exceed the scratch.
    bool gather = A.scr_cap > 0 && it.gslot >= 0;
    if (!split && tid == 0) {
      // a row expected to fill much of a slab gets a region of its own (est + 1/8), so it neither
      // moves nor strands the workgroup's slab; the slab is resumed after it
      const int64_t e = it.est;
      S_.own = 0u;
      if (e > A.slab / 4 && e + e / 8 > S_.slab_end - S_.slab_cur) {
        const int64_t take = e + e / 8 + 1024;
        const int64_t b = int64_t(atomicAdd(A.bump, (unsigned long long)take));
        if (b + take <= A.cap) {
          S_.saved_cur = S_.slab_cur;
          S_.saved_end = S_.slab_end;
          S_.own = 1u;
          S_.slab_cur = b;
          S_.slab_end = b + take;
        }
      }
      S_.row_begin = S_.slab_cur;
      S_.row_n = 0;
      S_.rsum = 0ull;
    }
    // the closed-form row sum this row's counts must add up to (read now, compared at the end)
    const int64_t rs_expect = (!split && tid == 0) ? A.rowsum[a] : 0;
    if (gather && tid < 64) {
      // bucket capacity of tile t >= 1 (in ids): the item's expected ids in tile t, Wi g_t, + 10% + 64.
      // A bucket that still overflows only sends its tile's chunk back to walking the lists.
      const float Wi = float(A.epre[k1] - A.epre[k0]);
      uint32_t cap = 0;
      if (tid >= 1 && tid < A.T) cap = (uint32_t(1.1f * Wi * A.gmass[tid]) + 64u + 3u) & ~3u;  // ids, 16-B aligned
      const uint32_t inc = wave_incl_scan(cap);
      if (tid < A.T) {
        S_.bstart[tid] = inc - cap;
        S_.bcur[tid] = 0u;
      }
      if (tid == A.T - 1) S_.bstart[A.T] = inc;
    }
    __syncthreads();
    gather = gather && uni(S_.bstart[A.T]) <= uint32_t(A.scr_cap) * 4u;
    const int dense_until = split ? t_end : -1;  // tiles below it go dense (split items)
    int32_t H = 0;                               // 0: table size from the estimate
    // a whole row whose hash table overflows (more distinct keys than the planner expected) is handed to
    // the sort path (k_srb_row, after this kernel) whole: its entries so far are dropped
    bool deferred = !split && A.sort_all;
    if (deferred) t = t_end;
    while (t < t_end) {
      // ---- this chunk: tiles [t, t1), dense or hash
      const bool dense = t < dense_until || ((dn >> t) & 1ull);
      int t1 = t + 1;
      if (!dense) {
        const uint64_t rest = t + 1 < 64 ? st >> (t + 1) : 0ull;
        t1 = rest ? min(t_end, t + __ffsll((long long)rest)) : t_end;
        if (H == 0) H = min(Sh::kHashMax, kHashMin << (((t < 32 ? hz0 : hz1) >> (2 * (t & 31))) & 3u));  // the planner's size
      }
      const int32_t c0 = t * kTW, c1 = min(A.M, t1 * kTW);
      WalkOp op;
      op.mode = dense ? kWalkDense : kWalkHash;
      const uint32_t lg = dense ? 0u : 31u - uint32_t(__clz(uint32_t(H)));
      op.hshift = 32u - lg;
      op.hmask = uint32_t(H) - 1u;
      if (tid == 0) {
        S_.flag = 0u;
      }
      __syncthreads();
      const unsigned long long c_walk = STAT_CLOCK();
      op.sbase = int64_t(blockIdx.x) * A.scr_cap;
#ifdef COOC_SP_STATS
      op.split = split;
#endif
      // tile 0 of a gather item (a dense chunk) counts tile 0 and sends the other tiles' groups to their
      // buckets; a later tile range of it walks the filled parts of its tiles' buckets (unless one of them
      // overflowed: then, as without gather mode, the lists over the chunk's tile range)
      const bool gwalk = gather && t == 0;
      const bool bucket = gather && !gwalk &&
                          !(uint64_t(uni(int64_t(S_.ovf))) & (((t1 < 64 ? (1ull << t1) : 0ull) - 1ull) & ~((1ull << t) - 1ull)));
      if (gwalk) op.mode = kWalkGather;
      const uint64_t walked = sp_walk<Sh>(A, L, S_, k0, k1, gwalk ? 0 : t, gwalk ? A.T : t1,
                                          gwalk || (!split && t == 0 && t1 == A.T), bucket, op);
      if (gwalk) {
        if (tid < 64) {
          const bool o = tid >= 1 && tid < A.T && S_.bcur[tid] > S_.bstart[tid + 1] - S_.bstart[tid];
          const uint64_t m = __ballot(o);
          if (tid == 0) S_.ovf = m;
        }
        sp_global_sync();  // the buckets are read back by other waves (and this item's lines are new)
      }
      if (bucket && split) STAT_ADD(58, STAT_CLOCK() - c_walk);  // a split share's bucket walks (tiles >= 1)
      const unsigned long long c_walked = STAT_CLOCK();
      STAT_ADD(split ? 4 : dense ? 0 : 1, c_walked - c_walk);
#ifdef COOC_SP_STATS
      // hash chunk classes: 0 = a light row (one hash chunk over every tile), 1 = a gathered tile range
      // (buckets), 2 = any other (walks the lists over its tile range)
      const int hcls = (!split && t == 0 && t1 == t_end) ? 0 : (gather && t > 0) ? 1 : 2;
      if (!dense && !split) {
        STAT_ADD(28 + 6 * hcls, 1);
        STAT_ADD(29 + 6 * hcls, c_walked - c_walk);
        STAT_ADD(31 + 6 * hcls, walked);
        STAT_ADD(33 + 6 * hcls, k1 - k0);
      }
#endif
      STAT_ADD(dense ? 9 : 10, walked);
      STAT_ADD(dense ? 5 : 6, 1);
      if (!dense && uni(S_.flag)) {
        STAT_ADD(7, 1);
        // overflow: clear the table (and the gather walk's state is this item's only); the row is deferred
        for (int32_t j = tid; j < H; j += Sh::kThreads) {
          L.R[j] = 0u;
          L.R[Sh::kHashMax + j] = 0u;
        }
        deferred = true;
        __syncthreads();  // every wave has read the flag and cleared its slots
        break;
      }
      // the -1 at column a per contribution whose walk includes its own position (whole rows)
      const uint32_t self = uint32_t(A.spre ? A.spre[k1] - A.spre[k0] : k1 - k0);
      if (split) {
        uint32_t *dst = A.staging + int64_t(A.split_slot[a]) * A.sstride + c0;
        if (!Sh::kU16) {  // (split rows are never mid rows)
          for (int32_t i = tid; i < c1 - c0; i += Sh::kThreads) {
            const uint32_t v = L.R[i];
            if (v) {
              atomicAdd(dst + i, v);
              L.R[i] = 0u;
            }
          }
        }
        __syncthreads();
        STAT_ADD(26, STAT_CLOCK() - c_walked);  // the share's flush of this tile into the staging row
      } else if (dense) {
        if (tid == 0 && ra >= c0 && ra < c1) {
          const uint32_t o = uint32_t(ra - c0);  // (the counter holds >= self: no borrow into the other u16)
          if (Sh::kU16)
            L.R[o >> 1] -= self << ((o & 1u) << 4);
          else
            L.R[o] -= self;
        }
        __syncthreads();
        sp_dense_compact<Sh>(A, L, S_, c1 - c0, c0, rsum, c0 == 0 ? mdst : nullptr);
        STAT_ADD(2, STAT_CLOCK() - c_walked);
      } else {
        if (tid == 0 && ra >= c0 && ra < c1) {
          uint32_t h = (uint32_t(ra) * 0x9E3779B1u) >> op.hshift;
          for (int p = 0; p < H; p++) {
            if (L.R[h] == uint32_t(ra) + 1u) {
              L.R[Sh::kHashMax + h] -= self;
              break;
            }
            h = (h + 1u) & op.hmask;
          }
        }
        __syncthreads();
        sp_hash_compact<Sh>(A, L, S_, H, c0, c1, rsum, c0 == 0 ? mdst : nullptr);
        STAT_ADD(3, STAT_CLOCK() - c_walked);
#ifdef COOC_SP_STATS
        STAT_ADD(30 + 6 * hcls, STAT_CLOCK() - c_walked);
        STAT_ADD(32 + 6 * hcls, uni(S_.row_n));
#endif
        STAT_ADD(14, H);
      }
      t = t1;
      H = 0;
    }
    STAT_ADD(split ? 12 : 11, 1);
    if (deferred) {
      STAT_ADD(8, 1);
      rsum = 0;
      if (tid == 0) {
        A.deferred[atomicAdd(reinterpret_cast<unsigned long long *>(&A.tot->n_deferred), 1ull)] = a;
        // the row's entries so far are abandoned: at the tail of the workgroup's slab they are handed back
        // (a row region of its own is restored below and its space stays unused)
        if (!S_.own) S_.slab_cur = S_.row_begin;
        S_.row_n = 0;
      }
    }
    if (!split) {  // the row-sum check: every count of the row, summed exactly (u64), == W_a - c_a
      for (int o = 32; o > 0; o >>= 1) rsum += __shfl_xor(rsum, o, 64);
      if ((tid & 63) == 0 && rsum) atomicAdd(&S_.rsum, (unsigned long long)rsum);
    }
    rsum = 0;
    if (!split && tid == 0) {
      A.row_base[a] = S_.row_n ? S_.row_begin : 0;
      A.row_nnz[a] = int32_t(S_.row_n);
      if (S_.own) {
        S_.slab_cur = S_.saved_cur;
        S_.slab_end = S_.saved_end;
      }
    }
    if (tid == 0) S_.work = next;
    __syncthreads();
    // a uint32 counter that wrapped, or any id lost or counted twice, breaks the sum
    if (!split && !deferred && tid == 0 && S_.rsum != (unsigned long long)rs_expect) {
      atomicOr(reinterpret_cast<unsigned long long *>(&A.tot->err), 2ull);
      A.tot->bad_row = a;
    }
  }
#ifdef COOC_SP_STATS
  if (tid == 0) {
    S_.st[13] = STAT_CLOCK() - t_start;
    for (int k = 0; k < 64; k++) atomicAdd(A.stats + k, S_.st[k]);
  }
#endif
}

// Split rows: the staging row (self term applied on the fly) compacted in column order into an
// exact-size region; the uint32 overflow check compares the count sum with the closed-form row sum.
// One 1,024-thread block per row; staging rows have a 16-B aligned stride, so in the first pass every lane reads
// kFinU x 4 counters (16-B loads) per step and the waves own 4,096-column-aligned ranges; the write pass reads
// one cell per lane and sub-step (see there).  M: the staging row's width -- every column, or, with the mirrored
// cells in records, the head's kTW; the kernel then also places the row's tail (tcnt, see below).
constexpr int kFinThreads = 1024, kFinWaves = kFinThreads / 64, kFinU = 4;
__global__ __launch_bounds__(kFinThreads) void k_sp_split_finalize(const int32_t *__restrict__ split_row,
                                                                    const uint32_t *__restrict__ staging, int64_t stride,
                                                                    int32_t M, const int64_t *__restrict__ row_ptr,
                                                                    const int64_t *__restrict__ rowsum,
                                                                    int32_t *__restrict__ col_out,
                                                                    uint32_t *__restrict__ cnt_out,
                                                                    unsigned long long *__restrict__ bump, int64_t cap,
                                                                    int64_t *__restrict__ row_base,
                                                                    int32_t *__restrict__ row_nnz,
                                                                    PlanTotals *__restrict__ tot,
                                                                    const int64_t *__restrict__ spre,
                                                                    const int32_t *__restrict__ hot_col,
                                                                    const int32_t *__restrict__ pos_of,
                                                                    uint32_t *__restrict__ tcnt, int32_t n_tiles,
                                                                    int32_t tw,
                                                                    const unsigned long long *__restrict__ tsum,
                                                                    int64_t *__restrict__ tbase) {
  __shared__ uint32_t s_w[kFinWaves], s_t[kFinWaves];
  __shared__ uint64_t s_red[kFinWaves];
  __shared__ int64_t s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t s = blockIdx.x;
  const int32_t a = split_row[s];
  const int32_t ra = relabel_pos(pos_of, uint32_t(a));  // staging rows are in relabelled column space
  const uint32_t self = uint32_t(spre ? spre[row_ptr[a + 1]] - spre[row_ptr[a]] : row_ptr[a + 1] - row_ptr[a]);
  const uint32_t *row = staging + int64_t(s) * stride;
  constexpr int32_t kStep = 64 * 4 * kFinU;  // columns per wave step
  const int32_t per = ((M + kFinWaves - 1) / kFinWaves + kStep - 1) / kStep * kStep;
  const int32_t lo = min(M, wave * per), hi = min(M, lo + per);
  auto load = [&](int32_t b, uint32_t v[4]) {
    if (b + 3 < hi) {
      const uint4 q = *reinterpret_cast<const uint4 *>(row + b);
      v[0] = q.x;
      v[1] = q.y;
      v[2] = q.z;
      v[3] = q.w;
    } else {
      for (int k = 0; k < 4; k++) v[k] = b + k < hi ? row[b + k] : 0u;
    }
    for (int k = 0; k < 4; k++)
      if (b + k == ra) v[k] -= self;
  };
  uint32_t cnt = 0;
  uint64_t sum = 0;
  for (int32_t b0 = lo; b0 < hi; b0 += kStep) {
    uint32_t v[kFinU][4];
#pragma unroll
    for (int u = 0; u < kFinU; u++) load(b0 + (u * 64 + lane) * 4, v[u]);
#pragma unroll
    for (int u = 0; u < kFinU; u++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        cnt += v[u][k] != 0u;
        sum += v[u][k];
      }
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) s_w[wave] = cnt;
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) s_red[wave] = sum;
  __syncthreads();
  uint32_t off = 0, tot_n = 0;
  uint64_t total_sum = 0;
  for (int w = 0; w < kFinWaves; w++) {
    off += w < wave ? s_w[w] : 0u;
    tot_n += s_w[w];
    total_sum += s_red[w];
  }
  // the row's tail in records (tcnt != NULL; M = kTW here, the head): k_sp_tail_pass left the non-zero cells of
  // every tile of kTailB source rows at tcnt[tile][s] and the cells' sum in tsum[s].  The counts become the tiles'
  // exclusive offsets within the tail, in place (a thread takes consecutive tiles; the strided cells of the
  // neighbouring slots' blocks share their lines in L2), and the one reservation below covers head and tail
  uint32_t tail_n = 0;
  if (tcnt) {
    const int32_t per_t = (n_tiles + kFinThreads - 1) / kFinThreads;
    const int32_t g0 = min(n_tiles, tid * per_t), g1 = min(n_tiles, g0 + per_t);
    uint32_t mine = 0;
    for (int32_t g = g0; g < g1; g++) mine += tcnt[int64_t(g) * tw + s];
    const uint32_t inc = wave_incl_scan(mine);
    if (lane == 63) s_t[wave] = inc;
    __syncthreads();
    uint32_t run = inc - mine;
    for (int w = 0; w < kFinWaves; w++) {
      run += w < wave ? s_t[w] : 0u;
      tail_n += s_t[w];
    }
    for (int32_t g = g0; g < g1; g++) {
      const uint32_t c = tcnt[int64_t(g) * tw + s];
      tcnt[int64_t(g) * tw + s] = run;
      run += c;
    }
  }
  if (tid == 0) {
    const uint32_t all_n = tot_n + tail_n;
    int64_t b = int64_t(atomicAdd(bump, (unsigned long long)all_n));
    if (b + int64_t(all_n) > cap) {
      atomicOr(reinterpret_cast<unsigned long long *>(&tot->err), 4ull);
      b = -1;
    }
    s_base = b;
    row_base[a] = b < 0 ? 0 : b;
    row_nnz[a] = int32_t(all_n);
    if (tcnt) {
      total_sum += tsum[s];
      tbase[s] = b < 0 ? -1 : b + int64_t(tot_n);  // the tail follows the head: ascending column rank
    }
    if (total_sum != uint64_t(rowsum[a])) atomicOr(reinterpret_cast<unsigned long long *>(&tot->err), 2ull);
  }
  __syncthreads();
  const int64_t base = s_base;
  if (base < 0) return;
  // the write pass takes a wave step's columns interleaved, one per lane and sub-step (column b0 + 64 j + lane):
  // an entry's position is the step's offset + the ballot's bits below the lane, and the active lanes of a
  // store write one contiguous run.  Ascending column, as the first pass's mapping: the same positions
  constexpr int kSub = kStep / 64;
  for (int32_t b0 = lo; b0 < hi; b0 += kStep) {
    uint32_t v[kSub];
#pragma unroll
    for (int j = 0; j < kSub; j++) {
      const int32_t b = b0 + 64 * j + lane;
      v[j] = b < hi ? row[b] : 0u;
      if (b == ra) v[j] -= self;
    }
#pragma unroll
    for (int j = 0; j < kSub; j++) {
      const int32_t b = b0 + 64 * j + lane;
      const uint64_t m = __ballot(v[j] != 0u);
      if (v[j]) {  // (the step's position is wave-uniform: scalar base + the lane's 32-bit offset)
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
        (col_out + (base + off))[pre] = relabel_col(hot_col, uint32_t(b));
        (cnt_out + (base + off))[pre] = v[j];
      }
      off += uint32_t(__popcll(m));
    }
  }
}

// Split rows' tails from the mirrored cells' records (SpArgs.mrec): rec[r][slot] = C[kTW + r, split_row[slot]] is
// split row slot's entry at column rank kTW + r.  The transpose is tile-wise: a tile of kTailB = 64 source rows x
// 64 slots is read row by row (a wave reads 256 contiguous bytes of one record: the records are read coalesced,
// every byte once per pass), staged in LDS (row pitch 65 words: conflict-free both ways) and taken out slot by
// slot, a lane per source row: the ballot of the non-zero cells ranks them, so a tile's entries of one slot are
// one contiguous ascending run.  Two passes around the head kernel (k_sp_split_finalize):
//   count (Write = false): tcnt[tile][slot] = the tile's non-zero cells of the slot (64-B stores), and the cells'
//                          sums, kept per workgroup in LDS over its tiles (kTailMaxSlots slots per sweep of the
//                          tiles: one sweep up to 1,024 split rows), added to tsum[slot] at the sweep's end;
//   write (Write = true):  the runs, at tbase[slot] + the tile's offset (tcnt after the head kernel's scan).
// A workgroup takes tiles blockIdx.x, + gridDim.x, ...; rows past rn and slots past tw read as zero.
constexpr int kTailThreads = 256, kTailWaves = kTailThreads / 64, kTailPer = kTailB / kTailWaves;
template <bool Write>
__global__ __launch_bounds__(kTailThreads) void k_sp_tail_pass(const uint32_t *__restrict__ rec, int32_t rn, int32_t tw,
                                                               int32_t n_split, int32_t n_tiles,
                                                               uint32_t *__restrict__ tcnt,
                                                               unsigned long long *__restrict__ tsum,
                                                               const int64_t *__restrict__ tbase,
                                                               int32_t *__restrict__ col_out,
                                                               uint32_t *__restrict__ cnt_out, int32_t col0) {
  __shared__ uint32_t tile[kTailB][65];
  __shared__ unsigned long long s_sum[Write ? 1 : kTailMaxSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t n_ch = (tw + 63) >> 6;
  // (the count pass sweeps the tiles once per kTailMaxSlots slots, whose sums it holds; the write pass once)
  const int32_t ch_sweep = Write ? n_ch : kTailMaxSlots / 64;
  for (int32_t ch0 = 0; ch0 < n_ch; ch0 += ch_sweep) {
  const int32_t ch1 = min(n_ch, ch0 + ch_sweep), s0 = ch0 * 64;
  if (!Write) {
    for (int32_t i = tid; i < kTailMaxSlots; i += kTailThreads) s_sum[i] = 0ull;
    __syncthreads();
  }
  for (int32_t g = blockIdx.x; g < n_tiles; g += gridDim.x) {
    const int32_t r0 = g * kTailB;
    for (int32_t ch = ch0; ch < ch1; ch++) {
      const int32_t sl = ch * 64 + lane;  // the load's slot; the wave's rows: r0 + kTailPer wave + j
      uint32_t v[kTailPer];
#pragma unroll
      for (int j = 0; j < kTailPer; j++) {
        const int32_t r = r0 + wave * kTailPer + j;
        v[j] = (r < rn && sl < tw) ? rec[int64_t(r) * tw + sl] : 0u;
      }
      // (write pass) the offsets of the wave's kTailPer slots, lane j its j-th: loaded next to the tile
      const int32_t so = ch * 64 + wave * kTailPer + lane;
      int64_t my_base = -1;
      if (Write && lane < kTailPer && so < n_split) {
        const int64_t tb = tbase[so];
        my_base = tb < 0 ? -1 : tb + int64_t(tcnt[int64_t(g) * tw + so]);
      }
      unsigned long long sm = 0ull;
#pragma unroll
      for (int j = 0; j < kTailPer; j++) {
        tile[wave * kTailPer + j][lane] = v[j];
        sm += v[j];
      }
      if (!Write && sm && sl < n_split) atomicAdd(&s_sum[sl - s0], sm);
      __syncthreads();
      uint32_t my_n = 0;
#pragma unroll
      for (int j = 0; j < kTailPer; j++) {
        const uint32_t x = tile[lane][wave * kTailPer + j];  // source row r0 + lane, the wave's j-th slot
        const uint64_t m = __ballot(x != 0u);
        if (Write) {
          const int64_t base = __shfl(my_base, j, 64);
          if (x && base >= 0) {  // (a non-zero cell's slot is below n_split: the pads stay as the memset left them)
            const uint32_t pre = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
            col_out[base + pre] = col0 + r0 + lane;
            cnt_out[base + pre] = x;
          }
        } else if (lane == j) {
          my_n = uint32_t(__popcll(m));
        }
      }
      if (!Write && lane < kTailPer && so < tw) tcnt[int64_t(g) * tw + so] = my_n;
      __syncthreads();  // (the tile is rewritten by the next step)
    }
  }
  if (!Write) {
    __syncthreads();
    for (int32_t i = tid; i < kTailMaxSlots && s0 + i < n_split; i += kTailThreads)
      if (s_sum[i]) atomicAdd(&tsum[s0 + i], s_sum[i]);
    __syncthreads();
  }
  }  // (slot sweep)
}

__global__ void k_sp_nnz_total(const int32_t *__restrict__ row_nnz, int32_t M, PlanTotals *__restrict__ tot) {
  __shared__ uint64_t s[4];
  uint64_t v = 0;
  for (int32_t a = blockIdx.x * 256 + threadIdx.x; a < M; a += gridDim.x * 256) v += uint64_t(row_nnz[a]);
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t t = s[0] + s[1] + s[2] + s[3];
    if (t) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->nnz_total), (unsigned long long)t);
  }
}

__global__ void k_sp_reset_run(PlanTotals *__restrict__ tot, int32_t *__restrict__ qctr,
                               unsigned long long *__restrict__ bump) {
  tot->err &= ~int64_t(6);  // the region (4) and row-sum (2) checks of the previous attempt
  tot->nnz_total = 0;
  tot->n_deferred = 0;
  tot->tiny_ctr = 0;
  tot->small_ctr = 0;
  qctr[0] = qctr[1] = 0;
  bump[0] = 0;
}

// ---- Counter::run_sparse (its planning phases: cooc_sparse_plan.hip; R: what the phases share, cooc_sparse.h) ----

// Gather scratch of a launch of g workgroups: a bucket region per workgroup for the largest expected tail
// (+25%), in 16-B groups; a work item whose exact tail is larger walks per chunk instead.  0 (no gather mode)
// when there is no tail or memory is short.
int64_t sp_scratch(int64_t max_tail, int64_t g, int32_t T, DevBuf &buf) {
  if (max_tail <= 0) return 0;
  const int64_t sc = std::min<int64_t>(kScrGroups, (max_tail + max_tail / 4 + 64 * T + 4096) / 4 + 1);
  const size_t need = sizeof(uint4) * size_t(g) * size_t(sc);
  size_t f0 = 0, t0 = 0;
  if (hipMemGetInfo(&f0, &t0) != hipSuccess) return 0;
  if (need > buf.cap && (need > (f0 + buf.cap) / 4 || !buf.reserve(need).ok())) return 0;
  return sc;
}

// The split rows' staging for R's layout (sized again when a mirrored attempt is repeated without mirroring).
// Row-major: n_split rows of sstride = Mc cells (16-B aligned).  Records (R.mstage): the rows' tile-0 heads, kTW
// cells each, then a record of mrec_w cells per column rank >= kTW; and the transposing finalize's scratch.
int64_t sp_tail_tiles(const SparseRun &R) { return R.mstage ? (int64_t(R.Mc) - kTW + kTailB - 1) / kTailB : 0; }
size_t sp_staging_cells(const SparseRun &R) {
  const size_t n = size_t(R.tot.n_split);
  return R.mstage ? n * size_t(kTW) + size_t(R.Mc - kTW) * size_t(R.mrec_w) : n * size_t(R.sstride);
}
Status sp_size_staging(SparseRun &R, DevBuf &staging, DevBuf &mtail) {
  R.sstride = R.mstage ? int64_t(kTW) : (int64_t(R.Mc) + 3) & ~int64_t(3);
  if (R.tot.n_split <= 0) return Status::Ok();
  COOC_TRY(staging.reserve(sizeof(uint32_t) * sp_staging_cells(R)));
  if (R.mstage)
    COOC_TRY(mtail.reserve(size_t(16) * size_t(R.tot.n_split) +
                           sizeof(uint32_t) * size_t(sp_tail_tiles(R)) * size_t(R.mrec_w)));
  return Status::Ok();
}

#ifdef COOC_SP_STATS
// the two k_sp_main launches' and k_sp_small's per-phase clocks and counts (64 words each), allocated once
unsigned long long *sp_stats_buf() {
  static unsigned long long *d_stats = nullptr;
  if (!d_stats) (void)hipMalloc(reinterpret_cast<void **>(&d_stats), kSpStatWords * 8);
  return d_stats;
}
#endif

}  // namespace

// The launches' grids, the staging rows, the gather scratch, 8. the output region and the kernels' arguments.
Status Counter::sparse_sizes(SparseRun &R) {
  const int32_t M = M_, T = R.T;
  const PlanTotals &t = R.tot;
  const int64_t n_split = t.n_split;
  COOC_TRY(sp_size_staging(R, staging_, sp_mtail_));  // (relabelled columns)
  // the two shapes' launches: the queue's big rows and split shares [0, n_big), then its mid rows
  const int64_t n_tiny = t.n_tiny, n_small = t.n_small, n_mid = t.n_mid;
  const int64_t n_big = t.n_chunks - n_tiny - n_small - n_mid;
  COOC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_main<SpBig>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SpBig::kLds));
  COOC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_main<SpMid>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SpMid::kLds));
  COOC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_main<SpMidAny>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SpMidAny::kLds));
  // any-order runs: the mid shape without the column ranking's bitmaps (COOC_SP_MID4=0: the ranking one)
  R.mid_any = any_order_ && !R.win && !mid4_off_;
  int per_cu = 1, per_cu_mid = 1;
  COOC_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sp_main<SpBig>, SpBig::kThreads, SpBig::kLds));
  if (R.mid_any)
    COOC_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_mid, k_sp_main<SpMidAny>, SpMidAny::kThreads,
                                                              SpMidAny::kLds));
  else
    COOC_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_mid, k_sp_main<SpMid>, SpMid::kThreads, SpMid::kLds));
  R.grid = std::min<int64_t>(std::max<int64_t>(n_big, 1), int64_t(n_cu_) * std::max(1, per_cu));
  R.grid_mid = std::min<int64_t>(std::max<int64_t>(n_mid, 1), int64_t(n_cu_) * std::max(1, per_cu_mid));
  // (mirrored split shares gather nothing: the big launch's scratch is sized by its whole rows alone)
  R.scr_cap = sp_scratch(R.mirror ? t.max_tail : std::max(t.max_tail, t.max_tail_split), R.grid, T, sp_scr_);
  R.scr_cap_mid = n_mid > 0 ? sp_scratch(t.max_tail_mid, R.grid_mid, T, sp_scr_mid_) : 0;
  R.n_gather = t.n_gather_rows + (R.mirror ? 0 : t.n_split_work);  // gather items (bound)
  // 8. output region: the expected entries plus slab slack, at most the exact bound
  size_t free_b = 0, total_b = 0;
  COOC_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  R.slab = std::max<int64_t>(int64_t(1) << 16, std::min<int64_t>(int64_t(1) << 22, t.est_nnz / (8 * R.grid)));
  R.grid_tiny = std::min<int64_t>((n_tiny + kTinyWaves - 1) / kTinyWaves, int64_t(n_cu_) * 8);
  R.grid_small = std::min<int64_t>(n_small, int64_t(n_cu_) * 4);
  R.slack = 2 * R.grid * R.slab + (n_mid ? 2 * R.grid_mid * R.slab : 0) + M +
            (n_tiny ? R.grid_tiny * kTinyWaves * kTinySlab : 0) + (n_small ? R.grid_small * kSmallSlab : 0) +
            2 * int64_t(n_cu_) * kSmallSlab;  // (+ k_srb_row)
  R.cap = std::min<int64_t>(t.cap_total + R.slack, t.est_nnz + t.est_nnz / 4 + R.slack);
  const int64_t budget = int64_t((free_b + col_.cap + cnt_.cap) / 10 * 8 / 8);
  R.cap = std::max<int64_t>(1, std::min(R.cap, budget));
  dense_mode_ = false;
  last_rows_ = M;
  COOC_TRY(bump_.reserve(sizeof(uint64_t) * 2));
  SpArgs &A = R.proto;
  A.queue = sp_queue_.as<SpWork>();
  A.tot = tot_.as<PlanTotals>();
  A.qctr = queue_.as<int32_t>();
  A.vals = vals_out_.as<uint32_t>();
  A.tb = sp_tb_.as<int32_t>();
  A.tbc = tbc_off_ ? nullptr : sp_tbc_.as<int4>();
  A.tarena = sp_arena_.as<uint4>();
  A.tarena0 = sp_arena0_.as<uint4>();
  A.epre = epre_.as<int64_t>();
  A.gmass = sp_est_.as<float>() + T * kEstK;
  A.split_slot = split_slot_.as<int32_t>();
  A.bump = bump_.as<unsigned long long>();
  A.slab = R.slab;
  A.row_base = row_base_.as<int64_t>();
  A.row_nnz = row_nnz_.as<int32_t>();
  A.M = R.Mc;  // (k_sp_main's column range)
  A.T = T;
  A.n_contrib = R.n_c;
  A.n_users = R.U;
  A.n_groups = R.n_groups1;
  A.n_groups0 = R.n_groups0;
  A.scratch = R.scr_cap ? sp_scr_.as<uint4>() : nullptr;
  A.scr_cap = (R.scr_cap && R.n_gather) ? R.scr_cap : 0;
  A.rowsum = rowsum_.as<int64_t>();
  A.spre = R.spre;
  COOC_TRY(sp_defer_.reserve(sizeof(int32_t) * size_t(M)));
  A.deferred = sp_defer_.as<int32_t>();
  A.sort_all = sort_rows_ ? 1 : 0;
  A.any_order = (any_order_ && !R.win) ? 1 : 0;
  A.hot_col = R.hot_col;
  A.pos_of = R.pos_of;
  A.mslot = R.mirror ? sp_mslot_.as<int32_t>() : nullptr;
  A.mirror_hi = R.mirror ? int32_t(std::min<int64_t>(t.split_rank_hi, kTW)) : 0;
  A.srank = R.mstage ? sp_srank_.as<int32_t>() : nullptr;  // (mrec itself: sparse_attempt, with staging)
  A.mrec_w = int32_t(R.mrec_w);
  A.n_split = int32_t(n_split);
  return Status::Ok();
}

// One attempt into a region of R.cap entries: the region and the counters reset, the four launches on the caller's
// stream (big, mid, small, tiny), the split rows' finalize, the totals (one sync).  *err: the run's error bits;
// *n_def: the whole rows it deferred to the sort path.
Status Counter::sparse_attempt(SparseRun &R, int64_t *err, int64_t *n_def) {
  hipStream_t s = R.s;
  const PlanTotals &t = R.tot;
  const int64_t n_split = t.n_split, n_tiny = t.n_tiny, n_small = t.n_small, n_mid = t.n_mid;
  const int64_t n_big = t.n_chunks - n_tiny - n_small - n_mid;
  PlanTotals *tot = tot_.as<PlanTotals>();
  COOC_TRY(col_.reserve(sizeof(int32_t) * size_t(R.cap + 1)));
  COOC_TRY(cnt_.reserve(sizeof(uint32_t) * size_t(R.cap + 1)));
  // (records: a source row without contributions writes none, and the hash and sorted sources only their
  // non-zero cells, so the records are cleared with the heads)
  if (n_split > 0) COOC_HIP_TRY(hipMemsetAsync(staging_.p, 0, sizeof(uint32_t) * sp_staging_cells(R), s));
  const int64_t n_tiles = sp_tail_tiles(R);
  unsigned long long *tsum = R.mstage ? sp_mtail_.as<unsigned long long>() : nullptr;
  int64_t *tbase = R.mstage ? sp_mtail_.as<int64_t>() + n_split : nullptr;
  uint32_t *tcnt = R.mstage ? reinterpret_cast<uint32_t *>(tbase + n_split) : nullptr;
  if (R.mstage) COOC_HIP_TRY(hipMemsetAsync(tsum, 0, sizeof(unsigned long long) * size_t(n_split), s));
  k_sp_reset_run<<<1, 1, 0, s>>>(tot, R.proto.qctr, bump_.as<unsigned long long>());
  SpArgs A = R.proto;
#ifdef COOC_SP_STATS
  A.stats = sp_stats_buf();
  (void)hipMemsetAsync(A.stats, 0, kSpStatWords * 8, s);
#endif
  A.staging = staging_.as<uint32_t>();
  A.sstride = R.sstride;
  A.mrec = R.mstage ? A.staging + n_split * int64_t(kTW) : nullptr;
  A.col_out = col_.as<int32_t>();
  A.cnt_out = cnt_.as<uint32_t>();
  A.cap = R.cap;
  if (R.timer && R.timer->enabled) COOC_HIP_TRY(hipEventRecord(R.timer->acc_begin, s));
  A.q_begin = 0;
  A.q_end = n_big;
  if (n_big > 0) {
    k_sp_main<SpBig><<<unsigned(R.grid), SpBig::kThreads, SpBig::kLds, s>>>(A);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (n_mid > 0) {  // the mid rows (after the big launch: it holds the heaviest rows)
    SpArgs B = A;
    B.qctr = A.qctr + 1;
    B.q_begin = n_big;
    B.q_end = n_big + n_mid;
    B.scratch = R.scr_cap_mid ? sp_scr_mid_.as<uint4>() : nullptr;
    B.scr_cap = (R.scr_cap_mid && R.n_gather) ? R.scr_cap_mid : 0;
#ifdef COOC_SP_STATS
    B.stats = A.stats + 64;
#endif
    if (R.mid_any)
      k_sp_main<SpMidAny><<<unsigned(R.grid_mid), SpMidAny::kThreads, SpMidAny::kLds, s>>>(B);
    else
      k_sp_main<SpMid><<<unsigned(R.grid_mid), SpMid::kThreads, SpMid::kLds, s>>>(B);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (n_small > 0) COOC_TRY(launch_sp_small(A, R.grid_small, s));
  if (n_tiny > 0) COOC_TRY(launch_sp_tiny(A, R.grid_tiny, s));
  // (after them: with mirroring the records take stores from the big, mid, small and tiny launches)
  // (records: the tails' count pass, the head kernel -- the rows' heads, kTW columns, and the one reservation per
  // row -- then the tails' write pass)
  if (n_split > 0) {
    const int32_t rn = R.Mc - kTW, tw = int32_t(R.mrec_w), col0 = R.hot_col ? 0 : kTW;
    const unsigned g_tail = unsigned(std::min<int64_t>(n_tiles, int64_t(n_cu_) * 8));
    if (R.mstage)
      k_sp_tail_pass<false><<<g_tail, kTailThreads, 0, s>>>(A.mrec, rn, tw, int32_t(n_split), int32_t(n_tiles), tcnt,
                                                           tsum, tbase, A.col_out, A.cnt_out, col0);
    k_sp_split_finalize<<<unsigned(n_split), kFinThreads, 0, s>>>(
        split_row_.as<int32_t>(), staging_.as<uint32_t>(), R.sstride, R.mstage ? kTW : R.Mc, row_ptr_.as<int64_t>(),
        rowsum_.as<int64_t>(), col_.as<int32_t>(), cnt_.as<uint32_t>(), bump_.as<unsigned long long>(), R.cap,
        row_base_.as<int64_t>(), row_nnz_.as<int32_t>(), tot, R.spre, R.hot_col, R.pos_of, tcnt, int32_t(n_tiles), tw,
        tsum, tbase);
    if (R.mstage)
      k_sp_tail_pass<true><<<g_tail, kTailThreads, 0, s>>>(A.mrec, rn, tw, int32_t(n_split), int32_t(n_tiles), tcnt,
                                                          tsum, tbase, A.col_out, A.cnt_out, col0);
    COOC_HIP_TRY(hipGetLastError());
  }
  // (the timed span: every counting kernel of the run -- k_sp_main, k_sp_small, k_sp_tiny, the split rows'
  // finalize -- so that moving rows between them cannot flatter the kernel time)
  if (R.timer && R.timer->enabled) COOC_HIP_TRY(hipEventRecord(R.timer->acc_end, s));
  COOC_HIP_TRY(hipMemcpyAsync(h_tot_, tot, sizeof(PlanTotals), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  *err = h_tot_->err;
  *n_def = h_tot_->n_deferred;
  // (COOC_FLAG_SORT_ROWS: every whole row is sorted -- the tiny and small rows by k_sp_tiny / k_sp_small, the
  // others by the sort path)
  last_deferred_ = *n_def + (sort_rows_ ? h_tot_->n_tiny + h_tot_->n_small : 0);
  last_deferred_pairs_ = sort_rows_ ? h_tot_->ts_pairs : 0;
  last_mirror_rows_ = R.mirror ? n_split : 0;
  return Status::Ok();
}

#ifdef COOC_SP_STATS
namespace {
// The per-phase clocks and counts of an attempt's two k_sp_main launches (stats build).
void sp_print_stats(const SparseRun &R, int attempt, int64_t err, int64_t mirror_rows) {
  const int64_t grid = R.grid, grid_mid = R.grid_mid;
  unsigned long long hh[kSpStatWords];
  (void)hipMemcpy(hh, sp_stats_buf(), sizeof(hh), hipMemcpyDeviceToHost);
  if (const unsigned long long *h = hh + kSmStatBase; h[8]) {  // k_sp_small (thread 0's clocks, 100 MHz)
    const double r = double(h[8]) * 100.0;
    fprintf(stderr, "[sp stats] small rows %llu keys %llu (%.0f per row) contributions %llu radix passes %llu | per row "
            "(us): total %.2f dequeue+header %.2f gather %.2f sort %.2f (ranking %.2f scan %.2f scatter %.2f) runs %.2f "
            "reservation %.2f stores %.2f\n", h[8], h[9], double(h[9]) / double(h[8]), h[10], h[12], h[11] / r, h[0] / r,
            h[1] / r, h[13] / r, h[2] / r, h[3] / r, h[4] / r, h[5] / r, h[6] / r, h[7] / r);
  }
  for (int shape = 0; shape < 2; shape++) {
    const unsigned long long *h = hh + 64 * shape;
    const double g = double(shape ? grid_mid : grid);
    if (shape && !R.tot.n_mid) break;
    fprintf(stderr, "[sp stats] %s shape (%lld WGs):\n", shape ? "mid" : "big", (long long)(shape ? grid_mid : grid));
    fprintf(stderr, "[sp stats] per WG (us): total %.0f walk dense %.0f walk hash %.0f split %.0f compact dense %.0f "
            "compact hash %.0f | chunks dense %llu hash %llu overflows %llu deferred rows %llu | pairs dense %.3g hash %.3g | "
            "rows %llu split items %llu | mean H %.0f | tail sizes %.0f\n",
            h[13] / 100.0 / g, h[0] / 100.0 / g, h[1] / 100.0 / g, h[4] / 100.0 / g, h[2] / 100.0 / g, h[3] / 100.0 / g,
            h[5], h[6], h[7], h[8], double(h[9]), double(h[10]), h[11], h[12], h[6] ? double(h[14]) / h[6] : 0.0,
            h[15] / 100.0 / g);
    fprintf(stderr, "[sp stats] hash detail per WG (us): walk scan %.0f walk loop %.0f | groups %.3g batches %llu | "
            "compact rank %.0f reserve %.0f write %.0f | entries %.3g\n", h[16] / 100.0 / g, h[17] / 100.0 / g,
            double(h[18]), h[19], h[20] / 100.0 / g, h[21] / 100.0 / g, h[22] / 100.0 / g, double(h[23]));
    fprintf(stderr, "[sp stats] split flush (staging atomics) per WG (us): %.0f\n", h[26] / 100.0 / g);
    fprintf(stderr, "[sp stats] split share phases per WG (us): tile-0 list walk %.0f, tail list walk %.0f, bucket "
            "walks (tiles >= 1) %.0f, staging flushes %.0f | mirrored split rows %lld\n", h[56] / 100.0 / g,
            h[57] / 100.0 / g, h[58] / 100.0 / g, h[26] / 100.0 / g, (long long)mirror_rows);
    fprintf(stderr, "[sp stats] hash compaction cumulative (us/WG): table+L1 %.0f, +masks %.0f | dense compaction "
            "cumulative (us/WG): count %.0f, +reserve %.0f, +writes %.0f, +barrier %.0f | hash walk: first group "
            "applied after %.2f us (thread 0, %llu walks)\n", h[46] / 100.0 / g, h[47] / 100.0 / g, h[48] / 100.0 / g,
            h[49] / 100.0 / g, h[50] / 100.0 / g, h[51] / 100.0 / g, h[55] ? h[54] / 100.0 / double(h[55]) : 0.0, h[55]);
    fprintf(stderr, "[sp stats] thread-0 sample: ids inserted %llu, probe rounds %llu (%.2f per group call)\n", h[24], h[25],
            h[24] ? double(h[25]) / double(h[24]) * 4.0 : 0.0);
    for (int c = 0; c < 3; c++) {
      const unsigned long long *q = h + 28 + 6 * c;
      fprintf(stderr, "[sp stats] hash class %s: chunks %llu, walk %.0f us/WG (%.2f us/chunk), compact %.0f us/WG "
              "(%.2f us/chunk), groups/chunk %.0f, row entries so far/chunk %.0f, contributions/chunk %.0f\n",
              c == 0 ? "light-row" : c == 1 ? "gathered" : "list-walk", q[0], q[1] / 100.0 / g,
              q[0] ? q[1] / 100.0 / double(q[0]) : 0.0, q[2] / 100.0 / g, q[0] ? q[2] / 100.0 / double(q[0]) : 0.0,
              q[0] ? double(q[3]) / q[0] : 0.0, q[0] ? double(q[4]) / q[0] : 0.0, q[0] ? double(q[5]) / q[0] : 0.0);
    }
  }
  fprintf(stderr, "[sp stats] attempt %d: cap %lld slab %lld grid %lld err %lld scr_cap %lld n_gather %lld\n", attempt,
          (long long)R.cap, (long long)R.slab, (long long)grid, (long long)err, (long long)R.proto.scr_cap,
          (long long)R.n_gather);
}
}  // namespace
#endif

Status Counter::run_sparse(int64_t U, const int64_t *up, const int32_t *items, int64_t n, hipStream_t s,
                           CountResult *out, KernelTimer *timer, const int32_t *owner, int32_t part,
                           const int64_t *freq, int64_t n_freq, const SparseWindow *win) {
  SparseRun R{};
  R.U = U;
  R.up = up;
  R.items = items;
  R.n = n;
  R.s = s;
  R.timer = timer;
  R.owner = owner;
  R.part = part;
  R.freq = freq;
  R.n_freq = n_freq;
  R.win = win;
  for (int64_t &v : last_plan_) v = 0;  // (cooc_last_batch_plan: no batch plan in this run)
  COOC_TRY(sparse_reserve(R));
  COOC_TRY(sparse_relabel(R));
  COOC_TRY(sparse_regroup(R));
  COOC_TRY(sparse_plan(R));
  COOC_TRY(sparse_sizes(R));
  // Attempts.  Two things repeat one:
  //  * a row was deferred while mirroring -- it leaves through the sort path, after the finalize and without
  //    mirroring, so the split rows would miss its cells (their row-sum check has fired).  Rare and exact: the
  //    queue is rebuilt without mirroring (the split shares walk their own tails) and the attempt repeated;
  //  * the region was exhausted below the exact bound (the expected key count was too low): it is grown to the
  //    bound, or to what memory allows, and the attempt repeated -- once.
  // (tests/test_gpu_region_grow.py reaches the grow, alone and ahead of the mirror repeat; cooc_last_attempts)
  int64_t err = 0;
  bool grown = false;
  last_attempts_ = 0;
  for (;;) {
    int64_t n_def = 0;
    last_attempts_++;
    last_region_entries_ = R.cap;
    COOC_TRY(sparse_attempt(R, &err, &n_def));
    if (R.mirror && n_def > 0 && !(err & 4)) {  // deferred while mirroring: repeat without
      R.mirror = false;
      R.mstage = false;  // (the staging rows are full-width again: sized for that layout)
      COOC_TRY(sp_size_staging(R, staging_, sp_mtail_));
      R.proto.srank = nullptr;
      COOC_TRY(sparse_queue(R));
      R.scr_cap = sp_scratch(std::max(R.tot.max_tail, R.tot.max_tail_split), R.grid, R.T, sp_scr_);
      R.n_gather = R.tot.n_gather_rows + R.tot.n_split_work;
      R.proto.scratch = R.scr_cap ? sp_scr_.as<uint4>() : nullptr;
      R.proto.scr_cap = (R.scr_cap && R.n_gather) ? R.scr_cap : 0;
      R.proto.mslot = nullptr;
      R.proto.mirror_hi = 0;
      continue;
    }
    if (n_def > 0 && !(err & 4)) {  // rows whose hash table overflowed (all whole rows: COOC_FLAG_SORT_ROWS)
      COOC_TRY(run_deferred(n_def, R.T, row_ptr_.as<int64_t>(), R.proto.vals, R.spre, R.cap, s));
      COOC_HIP_TRY(hipMemcpyAsync(&err, &tot_.as<PlanTotals>()->err, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
    }
    k_sp_nnz_total<<<std::min<unsigned>(nblocks(M_, 256), 64), 256, 0, s>>>(row_nnz_.as<int32_t>(), M_,
                                                                            tot_.as<PlanTotals>());
    COOC_HIP_TRY(hipGetLastError());
#ifdef COOC_SP_STATS
    sp_print_stats(R, grown ? 1 : 0, err, last_mirror_rows_);
#endif
    if (!(err & 4) || R.cap >= R.tot.cap_total + R.slack) break;
    // region exhausted below the exact bound: grow and repeat
    size_t f2 = 0, t2 = 0;
    COOC_HIP_TRY(hipMemGetInfo(&f2, &t2));
    const int64_t budget2 = int64_t((f2 + col_.cap + cnt_.cap) / 10 * 8 / 8);
    if (budget2 <= R.cap) break;
    R.cap = std::min<int64_t>(R.tot.cap_total + R.slack, budget2);
    // (exhausted after growing once: final.  The growth above stays ahead of this check, so the message below
    // names the region a further attempt would take)
    if (grown) break;
    grown = true;
  }
  if (err & 4)  // rows were cut short: never hand out a partial result
    return Status{4, "the output region (" + std::to_string(R.cap) + " entries) was exhausted"};
  out->row_base = row_base_.as<int64_t>();
  out->row_nnz = row_nnz_.as<int32_t>();
  out->col = col_.as<int32_t>();
  out->cnt = cnt_.as<uint32_t>();
  out->dense = nullptr;
  out->rowsum = rowsum_.as<int64_t>();
  out->rank_of = R.pos_of;
  out->unordered = R.proto.any_order != 0;
  out->work = R.tot.work_total;
  out->observed = R.tot.work_total - R.tot.self_total;  // ordered pairs of the counted rows
  out->nnz = -1;  // known after the stream drains: read_totals().nnz_total
  return Status::Ok();
}

}  // namespace cooc
