// cooc_sparse_plan.hip — the planner of the large-universe path (the algorithm: cooc_sparse.hip's opening
// comment): the optional column relabel, the users' lists regrouped by tile into the two arenas, the
// contributions sorted by row, the pair-work prefix, the expected distinct keys per tile, every row's chunk
// plan and the work queue -- the kernels, and the phases of Counter::run_sparse that launch them
// (sparse_reserve .. sparse_plan, sparse_queue).  Also the item-frequency histogram (launch_item_counts).
#include "cooc_sparse.h"
#include "cooc_scan.h"
#include "cooc_radix.h"
#include <algorithm>
#include <cstdio>
#include <string>

namespace cooc {

namespace {

constexpr uint64_t kGatherFlag = 1;                    // in a row plan's hz[0] (tile 0's code slot, tile 0 dense)
#ifndef COOC_SP_SPLIT_LG
#define COOC_SP_SPLIT_LG 23
#endif
#ifndef COOC_SP_GATHER_MIN
#define COOC_SP_GATHER_MIN 4  // rows of >= 4 chunks gather (A/B at round-4 HEAD: 125.2-125.5 vs 127.3-127.4 ms with 3)
#endif
constexpr int64_t kSplitWork = int64_t(1) << COOC_SP_SPLIT_LG;  // rows above this pair work are split
#ifndef COOC_SP_SUB_LG
#define COOC_SP_SUB_LG 24  // 2^24-pair shares: 1.4% faster than 2^23 on the 1/8 C3 shard (profiles/r03/sub_ab)
#endif
constexpr int64_t kSubWork = int64_t(1) << COOC_SP_SUB_LG;  // pairs per split work item (expected)
constexpr int kGatherMinChunks = COOC_SP_GATHER_MIN;   // rows with this many chunks gather their tails
#ifndef COOC_SP_FILL
#define COOC_SP_FILL 0.45f  // A/B at C3 (round 4, small rows in k_sp_small): 0.45 126.7, 0.5 126.9 (a row overflows), 0.375 130.3, 0.55 133 ms
#endif
#ifndef COOC_SP_DENSE
#define COOC_SP_DENSE 2.f
#endif
constexpr float kHashFill = COOC_SP_FILL * kHashMax;     // expected distinct keys per hash chunk
constexpr float kDensePairs = COOC_SP_DENSE * kTW;       // a tile with more expected pairs is dense
constexpr float kHashFillMid = COOC_SP_FILL * SpMid::kHashMax;
// a tile whose expected distinct keys exceed this is a dense chunk (its own tile of counters, compacted by a
// linear sweep) rather than part of a hash chunk (A/B knobs; default: the hash chunk's own capacity)
#ifndef COOC_SP_BIG_DENSE
#define COOC_SP_BIG_DENSE kHashFill
#endif
#ifndef COOC_SP_MID_DENSE
#define COOC_SP_MID_DENSE kHashFillMid
#endif
constexpr float kDenseKeys = COOC_SP_BIG_DENSE, kDenseKeysMid = COOC_SP_MID_DENSE;

// E[distinct keys of tile t | pair work W], interpolated in log2(W) between table points.
__device__ inline float est_distinct(const float *est, int t, int64_t W) {
  if (W <= 0) return 0.f;
  const float x = 2.f * log2f(float(W));
  int k = int(x);
  if (k >= kEstK - 1) return est[t * kEstK + kEstK - 1];
  const float f = x - float(k);
  const float lo = est[t * kEstK + k], hi = est[t * kEstK + k + 1];
  return lo + f * (hi - lo);
}

// Work items of a split row: shares of about kSubWork pairs whose expected tails (the pairs outside
// tile 0, mass 1 - g0) fit a gather scratch.
__device__ inline int32_t sp_split_shares(int64_t W, float g0) {
  const float tail = float(W) * fmaxf(0.f, 1.f - g0);
  return max(int32_t((W + kSubWork - 1) / kSubWork), int32_t(ceilf(tail / float(3 * kScrGroups))));
}

// ---- planner kernels ------------------------------------------------------------------------------
// Two arenas hold the users' lists, tile by tile: tile 0 (columns < 16,384: the Zipf head, ~70% of the
// ids) as u16 ids in arena0 (8 ids per 16-B load; at C3 the 1/8 shard's tile-0 part is ~180 MB and stays
// in the Infinity Cache), tiles >= 1 as u32 ids in arena1, ids of one tile contiguous, no padding between
// tiles.  tb[u] has T + 2 entries: tb[u][0] / tb[u][T + 1] = start / end of u's tile-0 ids in arena0
// (u16 positions), tb[u][t] (1 <= t <= T) = the arena1 position of tile t's first id (tb[u][T] = the end
// of u's list there).  A chunk reads a tile range of a list as the 16-B groups covering it and masks the
// ids outside it by position.
__device__ inline bool bit_of(const uint32_t *__restrict__ bits, uint32_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }

// An id's column after the relabel: a hot id's position in tile 0 (pos_of, gathered), any other id + kTW
// (arithmetic); without a relabel the id itself.
__device__ inline int32_t planner_rank(const int32_t *__restrict__ pos_of, const uint32_t *__restrict__ hotbm, uint32_t it) {
  if (!pos_of) return int32_t(it);
  return bit_of(hotbm, it) ? pos_of[it] : int32_t(it) + kTW;
}

// The arenas' user regions, packed and dense: one wave per user counts its tile-0 ids (ballots) and
// writes len[j] = round8(tile-0 ids) << 32 | round4(other ids); their inclusive prefix (one scan) gives
// every user's base in arena0 (high half) and arena1 (low half).
__global__ __launch_bounds__(256) void k_sp_tile_counts(int64_t U, const int64_t *__restrict__ up,
                                                        const int32_t *__restrict__ items, int32_t M,
                                                        uint64_t *__restrict__ len, const int32_t *__restrict__ owner,
                                                        int32_t part, int32_t *__restrict__ ownc,
                                                        const int32_t *__restrict__ rank_of,
                                                        const uint32_t *__restrict__ hotbm,
                                                        const uint32_t *__restrict__ minebm) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = gw; j < U; j += n_waves) {
    const int64_t s = up[j];
    const int32_t n = int32_t(up[j + 1] - s);
    int32_t n0 = 0, mine = 0;
    for (int32_t p0 = 0; p0 < n; p0 += 4 * 64) {
      int32_t it[4];
#pragma unroll
      for (int k = 0; k < 4; k++) it[k] = p0 + 64 * k + lane < n ? items[s + p0 + 64 * k + lane] : -1;
#pragma unroll
      for (int k = 0; k < 4; k++) {  // (an invalid id goes to tile 0 in k_sp_tile_lists, which reports it)
        const bool in = p0 + 64 * k + lane < n;
        const bool valid = uint32_t(it[k]) < uint32_t(M);
        // (tile 0: a hot id after a relabel -- a bit -- else an id below kTW)
        const bool t0 = !valid || (rank_of ? bit_of(hotbm, uint32_t(it[k])) : uint32_t(it[k]) < uint32_t(kTW));
        n0 += int32_t(__popcll(__ballot(in && t0)));
        if (owner) mine += int32_t(__popcll(__ballot(valid && bit_of(minebm, uint32_t(it[k])))));
      }
    }
    if (lane == 0) {
      len[j] = (uint64_t((n0 + 7) & ~7) << 32) | uint64_t((n - n0 + 3) & ~3);
      if (owner) ownc[j] = mine;
    }
  }
}

// One wave per user: validates the ids, emits the contributions (item, user) in CSR order for the item
// sort (the keyBy(itemA) regrouping, FlinkCooccurrences.java:152; owner != NULL: only counts the owned
// ones), counts the list by tile in LDS and writes the arenas: the user's tile-0 ids as u16 at its
// arena0 base (kSink16 pads to a multiple of 8), its other ids tile by tile as u32 at its arena1 base
// (kSink pads to a multiple of 4), bases from k_sp_tile_counts' prefix.  tb[j] gets the absolute
// offsets: [0] = base0, [t] = base1 + the ids of tiles 1..t-1, [T + 1] = base0 + the tile-0 ids.
// tbc[j] = {tb[j][0], tb[j][T + 1], tb[j][1], tb[j][T]}: the list's tile-0 range in arena0 and its whole
// tail range in arena1 as one 16-B record (16 B per list where a tb row is 4 (T + 2) B: the table of the
// walks that take whole lists or tile-0 parts stays in cache; a tile sub-range still reads tb).
constexpr int kTlR = 4;  // ids per lane held in registers across both passes (users of <= 256 ids)

__global__ __launch_bounds__(256) void k_sp_tile_lists(int64_t U, const int64_t *__restrict__ up,
                                                       const int32_t *__restrict__ items, int32_t M, int32_t T,
                                                       int32_t *__restrict__ tb, int4 *__restrict__ tbc,
                                                       uint16_t *__restrict__ arena0,
                                                       uint32_t *__restrict__ arena1, const uint64_t *__restrict__ pbase,
                                                       uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, const int32_t *__restrict__ owner,
                                                       int32_t part, const int64_t *__restrict__ ownoff,
                                                       PlanTotals *__restrict__ tot, const int32_t *__restrict__ rank_of,
                                                       const uint32_t *__restrict__ hotbm,
                                                       const uint32_t *__restrict__ minebm) {
  __shared__ int32_t cur[4][kSpMaxTiles + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t *c = cur[wave];
  const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  bool bad = false;
  int64_t s = 0, e = 0;
  if (gw < U) {
    s = up[gw];
    e = up[gw + 1];
  }
  for (int64_t j = gw; j < U; j += n_waves) {
    const int32_t n = int32_t(e - s);
    // the next user's bounds and this user's first kTlR * 64 ids: all loads in flight together
    int64_t sn = 0, en = 0;
    if (j + n_waves < U) {
      sn = up[j + n_waves];
      en = up[j + n_waves + 1];
    }
    int32_t r[kTlR];
#pragma unroll
    for (int k = 0; k < kTlR; k++) {
      const int32_t p = lane + 64 * k;
      r[k] = p < n ? items[s + p] : 0;
      if (uint32_t(r[k]) >= uint32_t(M)) bad = true;
    }
    for (int32_t t = lane; t <= T; t += 64) c[t] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    int32_t n0 = 0;  // (tile-0 ids, the Zipf head, counted by ballot: no same-address LDS atomics)
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    int64_t o = owner ? ownoff[j] : 0;  // (owned contributions: at ownoff[j], in list order)
    // it: the item id (contributions, owner map); rk: its column rank (tiles, arenas)
    auto count = [&](bool in, int32_t p, int32_t it, int32_t rk, bool valid) {
      n0 += __popcll(__ballot(in && (rk >> kTShift) == 0));
      if (in && (rk >> kTShift)) atomicAdd(&c[rk >> kTShift], 1);
      if (!owner) {
        if (keys && in) {  // (NULL: the contributions come from elsewhere, k_sp_window_contribs)
          keys[s + p] = uint32_t(it);
          vals[s + p] = uint32_t(j);
        }
      } else {
        const bool m = in && valid && bit_of(minebm, uint32_t(it));
        const uint64_t bal = __ballot(m);
        if (m && keys) {
          keys[o + __popcll(bal & lt)] = uint32_t(it);
          vals[o + __popcll(bal & lt)] = uint32_t(j);
        }
        o += __popcll(bal);
      }
    };
    bool valid[kTlR];
    int32_t rk[kTlR];
#pragma unroll
    for (int k = 0; k < kTlR; k++) {
      valid[k] = uint32_t(r[k]) < uint32_t(M);
      if (!valid[k]) r[k] = 0;
      rk[k] = lane + 64 * k < n ? planner_rank(rank_of, hotbm, uint32_t(r[k])) : r[k];
    }
#pragma unroll
    for (int k = 0; k < kTlR; k++) count(lane + 64 * k < n, lane + 64 * k, r[k], rk[k], valid[k]);
    for (int32_t p0 = 64 * kTlR; p0 < n; p0 += 64) {
      const int32_t p = p0 + lane;
      int32_t it = p < n ? items[s + p] : 0;
      const bool v = uint32_t(it) < uint32_t(M);
      if (!v) {
        bad = true;
        it = 0;
      }
      count(p < n, p, it, p < n ? planner_rank(rank_of, hotbm, uint32_t(it)) : it, v);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int32_t *tbj = tb + j * (T + 2);
    const int32_t n1 = n - n0;
    const uint64_t pb = pbase[j];
    const int64_t b0 = int64_t(pb >> 32), b1 = int64_t(pb & 0xFFFFFFFFull);
    // exclusive prefix of tiles 1..T's counts: tb and the tiles' cursors
    if (T < 64) {  // one wave scan, lane t = tile t
      const int32_t x = (lane >= 1 && lane <= T) ? c[lane] : 0;
      const int32_t ex = int32_t(wave_incl_scan(uint32_t(x))) - x;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (lane >= 1 && lane <= T) {
        tbj[lane] = int32_t(b1 + ex);  // (tile T is empty: tbj[T] = base1 + n1)
        c[lane] = ex;
      }
    } else if (lane == 0) {
      int32_t run = 0;
      for (int32_t t = 1; t <= T; t++) {
        const int32_t x = c[t];
        tbj[t] = int32_t(b1 + run);
        c[t] = run;
        run += x;
      }
    }
    if (lane == 0) {
      tbj[0] = int32_t(b0);
      tbj[T + 1] = int32_t(b0 + n0);
      tbc[j] = make_int4(int32_t(b0), int32_t(b0 + n0), int32_t(b1), int32_t(b1 + n1));  // (= tbj[0], [T + 1], [1], [T])
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint16_t *o0 = arena0 + b0;
    uint32_t *o1 = arena1 + b1;
    int32_t q0 = 0;  // the tile-0 cursor (wave-uniform): ballot ranks, in lane order
    auto place = [&](bool in, int32_t it) {
      const bool t0 = in && (it >> kTShift) == 0;
      const uint64_t b = __ballot(t0);
      if (t0) o0[q0 + int32_t(__popcll(b & lt))] = uint16_t(it);
      else if (in) o1[atomicAdd(&c[it >> kTShift], 1)] = uint32_t(it);
      q0 += int32_t(__popcll(b));
    };
#pragma unroll
    for (int k = 0; k < kTlR; k++) place(lane + 64 * k < n, rk[k]);
    for (int32_t p0 = 64 * kTlR; p0 < n; p0 += 64) {  // (long lists: L1 / L2 lines of the first pass)
      const int32_t p = p0 + lane;
      int32_t it = p < n ? items[s + p] : 0;
      if (uint32_t(it) >= uint32_t(M)) it = 0;
      place(p < n, p < n ? planner_rank(rank_of, hotbm, uint32_t(it)) : it);
    }
    if (lane < ((n0 + 7) & ~7) - n0) o0[n0 + lane] = uint16_t(kSink16);  // (<= 7 pads)
    if (lane < ((n1 + 3) & ~3) - n1) o1[n1 + lane] = kSink;              // (<= 3 pads)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    s = sn;
    e = en;
  }
  if (bad) atomicOr(reinterpret_cast<unsigned long long *>(&tot->err), 1ull);
}

// Streaming window (old / new positions, NonSampled...java:129-161): user j's two lists are A_j (the whole
// history after the window, at up2[2j]) and B_j (its new items, positions >= old[j], at up2[2j + 1]).
// Position p of A_j is a contribution of row x_p: a new position (p >= old[j]) walks A_j (every pair with
// it as the later one, the pair with itself removed: kSelfBit), an old one walks B_j (its pairs with the
// window's items).  Contribution p of user j lands at cbase[j] + p.  One wave per user.
__global__ __launch_bounds__(256) void k_sp_window_contribs(int64_t U, const int64_t *__restrict__ up2,
                                                           const int32_t *__restrict__ items,
                                                           const int32_t *__restrict__ old,
                                                           const int64_t *__restrict__ cbase,
                                                           uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = gw; j < U; j += n_waves) {
    const int64_t s = up2[2 * j];
    const int32_t n = int32_t(up2[2 * j + 1] - s), o = old[j];
    const int64_t c = cbase[j];
    for (int32_t p = lane; p < n; p += 64) {
      keys[c + p] = uint32_t(items[s + p]);
      vals[c + p] = p >= o ? (uint32_t(2 * j) | kSelfBit) : uint32_t(2 * j + 1);
    }
  }
}

// The (item, user) contributions of a batch in CSR order, for the item sort (the keyBy(itemA) regrouping,
// FlinkCooccurrences.java:152) ahead of the column relabel; an invalid id (k_sp_tile_lists reports it)
// becomes row 0.  One wave per user.
__global__ __launch_bounds__(256) void k_sp_contribs(int64_t U, const int64_t *__restrict__ up,
                                                     const int32_t *__restrict__ items, int32_t M,
                                                     uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = gw; j < U; j += n_waves) {
    const int64_t s = up[j], e = up[j + 1];
    for (int64_t p = s + lane; p < e; p += 64) {
      const int32_t it = items[p];
      keys[p] = uint32_t(it) < uint32_t(M) ? uint32_t(it) : 0u;
      vals[p] = uint32_t(j);
    }
  }
}

// Column relabel: the kTW most frequent items of the batch (its own frequencies -- the row lengths of the
// item-sorted contributions -- or the caller's global counts; ties: the smaller id first) become tile 0, in
// ascending id order; every other item keeps its id shifted one tile up.  So tile 0 (u16 arena, dense LDS
// tiles) holds the Zipf head whatever order the ids come in, and a column maps back to its item by a lookup
// in a 64 KB table (tile 0) or a subtraction (above).
__global__ void k_rank_keys(const int64_t *__restrict__ row_ptr, const int64_t *__restrict__ freq, int32_t M,
                            uint64_t *__restrict__ keys, int32_t *__restrict__ ids, uint8_t *__restrict__ hot) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  keys[a] = uint64_t(freq ? freq[a] : row_ptr[a + 1] - row_ptr[a]);
  ids[a] = a;
  hot[a] = 0;
}

__global__ void k_hot_mark(const int32_t *__restrict__ order, int32_t h, uint8_t *__restrict__ hot) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < h) hot[order[r]] = 1;
}

// how many of the hot items already have an id below kTW (the relabel is skipped when nearly all do)
__global__ void k_hot_overlap(const uint8_t *__restrict__ hot, int32_t n, int32_t *__restrict__ out) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t c = uint32_t(__popcll(__ballot(a < n && hot[a] != 0)));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, int32_t(c));
}

// Bitmaps over item ids for the planner's per-interaction passes: a 4-B gather per interaction into an
// M-entry table is one L2 request per lane (the passes over a whole 1e9-interaction log are bound by that
// request rate), a bit lookup into an M-bit table shares lines between the lanes (the hot ids' bits sit in
// few lines).  hot: the ids of tile 0 after a relabel; mine: the rows a part owns.
__global__ void k_bits_hot(const uint8_t *__restrict__ hot, int32_t M, uint32_t *__restrict__ bits) {
  const int32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= M) return;
  uint32_t v = 0;
  for (int b = 0; b < 32 && w * 32 + b < M; b++) v |= uint32_t(hot[w * 32 + b] != 0) << b;
  bits[w] = v;
}

__global__ void k_bits_owner(const int32_t *__restrict__ owner, int32_t part, int32_t M, uint32_t *__restrict__ bits) {
  const int32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= M) return;
  uint32_t v = 0;
  for (int b = 0; b < 32 && w * 32 + b < M; b++) v |= uint32_t(owner[w * 32 + b] == part) << b;
  bits[w] = v;
}

// pos_of (item -> column) and the frequencies in column order (the planner's per-tile estimate; the holes of
// the hot items above tile 0 count 0)
__global__ void k_relabel_pos(const uint8_t *__restrict__ hot, const uint64_t *__restrict__ freq_by_id, int32_t M,
                              int32_t *__restrict__ pos_of, int64_t *__restrict__ freq_col) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  const bool h = hot[a] != 0;
  if (!h) pos_of[a] = a + kTW;
  freq_col[kTW + a] = h ? 0 : int64_t(freq_by_id[a]);
}

__global__ void k_relabel_hot(const int32_t *__restrict__ hot_col, const uint64_t *__restrict__ freq_by_id,
                              int32_t *__restrict__ pos_of, int64_t *__restrict__ freq_col) {
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= kTW) return;
  const int32_t a = hot_col[c];
  pos_of[a] = c;
  freq_col[c] = int64_t(freq_by_id[a]);
}


__global__ void k_sp_row_ptr(const uint32_t *__restrict__ keys, int64_t n, int32_t M, int64_t *__restrict__ row_ptr) {
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a > M) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < uint32_t(a)) lo = mid + 1; else hi = mid;
  }
  row_ptr[a] = lo;
}

struct ScanUserLen {  // the pair work of contribution i (its list's length, from the u32 table), for launch_scan
  const uint32_t *vals;
  const uint32_t *len;
  __device__ int64_t operator()(int64_t i) const { return int64_t(len[vals[i] & kListMask]); }
};

// the lists' lengths as u32 (one 4-B gather per contribution in the pair-work prefix instead of two 8-B ones
// from the CSR pointers: a 5-MB table at the 1/8 C3 share)
__global__ void k_list_len32(int64_t U, const int64_t *__restrict__ up, uint32_t *__restrict__ len) {
  const int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (u < U) len[u] = uint32_t(up[u + 1] - up[u]);
}

struct ScanSelfFlag {  // SelfFlag of contribution i, for launch_scan
  const uint32_t *vals;
  __device__ int64_t operator()(int64_t i) const { return int64_t(vals[i] >> 31); }
};

// est[t][k] = sum over the columns b of tile t of 1 - exp(-2^(k/2) f_b / N); gmass[t] = tile t's
// share of the interactions.  One block per (tile, k).
__global__ __launch_bounds__(256) void k_sp_est(const int64_t *__restrict__ row_ptr, const int64_t *__restrict__ freq,
                                                int32_t M, int64_t n, float *__restrict__ est, float *__restrict__ gmass) {
  __shared__ double s_mass[4];
  __shared__ float s[4];
  const int t = blockIdx.x, k = blockIdx.y;
  const int32_t b0 = t * kTW, b1 = min(M, b0 + kTW);
  const float scale = exp2f(0.5f * float(k)) / float(n);
  float acc = 0.f;
  double mass = 0.0;
  for (int32_t b = b0 + threadIdx.x; b < b1; b += 256) {
    const int64_t fi = freq ? freq[b] : row_ptr[b + 1] - row_ptr[b];
    const float f = float(fi);
    mass += double(fi);
    if (f > 0.f) acc += -expm1f(-f * scale);
  }
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    mass += __shfl_xor(mass, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s[threadIdx.x >> 6] = acc;
    s_mass[threadIdx.x >> 6] = mass;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    est[t * kEstK + k] = s[0] + s[1] + s[2] + s[3];
    if (k == 0) gmass[t] = float((s_mass[0] + s_mass[1] + s_mass[2] + s_mass[3]) / double(n));
  }
}

// Per row: pair work W_a (exact), row sum W_a - c_a (closed form), and the chunk plan.
__global__ __launch_bounds__(256) void k_sp_plan(int32_t M, int32_t T, const int64_t *__restrict__ row_ptr,
                                                 const int64_t *__restrict__ epre, const float *__restrict__ est,
                                                 const float *__restrict__ gmass, int64_t *__restrict__ rowsum,
                                                 int64_t *__restrict__ row_w, uint64_t *__restrict__ pstart,
                                                 uint64_t *__restrict__ pdense, uint64_t *__restrict__ hz,
                                                 uint64_t *__restrict__ skey,
                                                 int32_t *__restrict__ order, int32_t *__restrict__ nwork,
                                                 int32_t *__restrict__ row_nnz, int64_t *__restrict__ row_base,
                                                 PlanTotals *__restrict__ tot, const int64_t *__restrict__ spre,
                                                 int32_t mid_on, const int32_t *__restrict__ pos_of) {
  __shared__ uint64_t s_red[4][4];
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t est_sum = 0, bound = 0, n_split = 0, split_work = 0, n_active = 0, max_tail = 0, n_gather = 0, n_tiny = 0,
           n_small = 0, ts_pairs = 0, n_mid = 0, max_tail_mid = 0, max_tail_split = 0, split_hi = 0;
  if (a < M) {
    const int64_t k0 = row_ptr[a], c = row_ptr[a + 1] - k0;
    const int64_t W = epre[k0 + c] - epre[k0];
    const int64_t self = spre ? spre[k0 + c] - spre[k0] : c;  // pairs of a position with itself
    rowsum[a] = W - self;
    row_w[a] = W;
    row_nnz[a] = 0;
    row_base[a] = 0;
    order[a] = a;
    skey[a] = uint64_t(W);
    uint64_t st = 0, dn = 0, h0 = 0, h1 = 0;
    int32_t nw = 0;
    if (c > 0) {
      n_active = 1;
      n_tiny = W <= kTinyW ? 1 : 0;  // (the W-descending queue puts them last)
      n_small = (W > kTinyW && W <= kSmallW) ? 1 : 0;  // (... just before the tiny ones)
      ts_pairs = (n_tiny || n_small) ? uint64_t(W) : 0u;
      // a mid row (k_sp_main's 256-thread shape): its chunks are planned for 4K-slot tables over <= 2^19 columns
      const bool mid = mid_on && !n_tiny && !n_small && W <= kMidW;
      n_mid = mid ? 1 : 0;
      const float hfill = mid ? kHashFillMid : kHashFill, dkeys = mid ? kDenseKeysMid : kDenseKeys;
      const int hmax = mid ? SpMid::kHashMax : kHashMax;
      const int hmaxtiles = mid ? SpMid::kHashMaxTiles : kHashMaxTiles;
      bound = uint64_t(min<int64_t>(W - self, M));
      float e_tot = 0.f;
      if (W > kSplitWork) {
        n_split = 1;
        for (int t = 0; t < T; t++) e_tot += est_distinct(est, t, W);
        nw = sp_split_shares(W, gmass[0]);
        split_work = uint64_t(nw);
        // (kept apart from the whole rows' tails: mirrored split shares gather nothing)
        max_tail_split = uint64_t(float(W) * fmaxf(0.f, 1.f - gmass[0]) / float(nw));
        split_hi = uint64_t(relabel_pos(pos_of, uint32_t(a))) + 1u;
      } else {
        float cur = 0.f;
        int n_in = 0, cs = -1;
        // a hash chunk's table: the smallest power of two >= SLACK * E[distinct] + 64 slots (kHashMin..kHashMax)
        auto close = [&]() {
          if (cs < 0) return;
          uint64_t code = 0;
#ifndef COOC_SP_HASH_SLACK
#define COOC_SP_HASH_SLACK 4.f  // table >= 4x the estimated distinct count (A/B)
#endif
          for (int H = kHashMin; H < hmax && float(H) < COOC_SP_HASH_SLACK * cur + 64.f; H <<= 1) code++;
          if (cs < 32) h0 |= code << (2 * cs); else h1 |= code << (2 * (cs - 32));
          cs = -1;
        };
        for (int t = 0; t < T; t++) {
          const float d = est_distinct(est, t, W);
          const float e = float(W) * gmass[t];
          e_tot += d;
          if (d > dkeys || e > kDensePairs) {
            close();
            st |= uint64_t(1) << t;
            dn |= uint64_t(1) << t;
          } else {
            if (cs < 0 || cur + d > hfill || n_in == hmaxtiles) {
              close();
              st |= uint64_t(1) << t;
              cs = t;
              cur = 0.f;
              n_in = 0;
            }
            cur += d;
            n_in++;
          }
        }
        close();
        if ((dn & 1ull) && __popcll(st) >= kGatherMinChunks) {  // gather mode (k_sp_main)
          // the flag: bit 0 of tile 0's hash-size code, unused when tile 0 is dense (every bit of dn is a
          // tile: a 64-tile universe, 1,032,193 to 1,048,576 columns, has one in bit 63)
          h0 |= kGatherFlag;
          max_tail = uint64_t(float(W) * fmaxf(0.f, 1.f - gmass[0]));
          if (mid) {
            max_tail_mid = max_tail;
            max_tail = 0;
          }
          n_gather = 1;
        }
      }
      est_sum = uint64_t(e_tot) + 1;
      row_nnz[a] = int32_t(min(est_sum, uint64_t(INT32_MAX)));  // carried to the queue record (k_sp_queue)
    }
    pstart[a] = st;
    pdense[a] = dn;
    hz[2 * a] = h0;
    hz[2 * a + 1] = h1;
    nwork[a] = nw;
  }
  uint64_t v[4] = {est_sum, bound, n_split, split_work};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = 0; i < 4; i++) {
    for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
    if (lane == 0) s_red[i][w] = v[i];
  }
  uint64_t act = n_active;
  for (int o = 32; o > 0; o >>= 1) {
    act += __shfl_xor(act, o, 64);
    n_tiny += __shfl_xor(n_tiny, o, 64);
    n_small += __shfl_xor(n_small, o, 64);
    n_mid += __shfl_xor(n_mid, o, 64);
    max_tail_mid = max(max_tail_mid, __shfl_xor(max_tail_mid, o, 64));
    ts_pairs += __shfl_xor(ts_pairs, o, 64);
    n_gather += __shfl_xor(n_gather, o, 64);
    max_tail = max(max_tail, __shfl_xor(max_tail, o, 64));
    max_tail_split = max(max_tail_split, __shfl_xor(max_tail_split, o, 64));
    split_hi = max(split_hi, __shfl_xor(split_hi, o, 64));
  }
  if (lane == 0 && split_hi) {
    atomicMax(reinterpret_cast<unsigned long long *>(&tot->max_tail_split), (unsigned long long)max_tail_split);
    atomicMax(reinterpret_cast<unsigned long long *>(&tot->split_rank_hi), (unsigned long long)split_hi);
  }
  if (lane == 0 && max_tail) atomicMax(reinterpret_cast<unsigned long long *>(&tot->max_tail), (unsigned long long)max_tail);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t r[4];
    for (int i = 0; i < 4; i++) r[i] = s_red[i][0] + s_red[i][1] + s_red[i][2] + s_red[i][3];
    if (r[0]) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->est_nnz), (unsigned long long)r[0]);
    if (r[1]) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->cap_total), (unsigned long long)r[1]);
    if (r[2]) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_split), (unsigned long long)r[2]);
    if (r[3]) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_split_work), (unsigned long long)r[3]);
  }
  if (lane == 0 && act) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_active), (unsigned long long)act);
  if (lane == 0 && n_tiny) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_tiny), (unsigned long long)n_tiny);
  if (lane == 0 && n_small) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_small), (unsigned long long)n_small);
  if (lane == 0 && n_mid) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_mid), (unsigned long long)n_mid);
  if (lane == 0 && max_tail_mid)
    atomicMax(reinterpret_cast<unsigned long long *>(&tot->max_tail_mid), (unsigned long long)max_tail_mid);
  if (lane == 0 && ts_pairs) atomicAdd(reinterpret_cast<unsigned long long *>(&tot->ts_pairs), (unsigned long long)ts_pairs);
  if (lane == 0 && n_gather)
    atomicAdd(reinterpret_cast<unsigned long long *>(&tot->n_gather_rows), (unsigned long long)n_gather);
}

__global__ void k_sp_gather_nwork(const int32_t *__restrict__ order, const int32_t *__restrict__ nwork, int32_t M,
                                  int32_t *__restrict__ out) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < M) out[r] = nwork[order[r]];
}

// Work queue: the split rows' shares (they are the heaviest rows, so the first n_split rows of the
// W-descending order), then every other row with contributions, heaviest first.  Gather items get a
// row of bucket starts (gslot).
__global__ void k_sp_queue(const int32_t *__restrict__ order, const uint64_t *__restrict__ skey,
                           const int32_t *__restrict__ wbase, const float *__restrict__ gmass,
                           const int64_t *__restrict__ row_ptr, const uint64_t *__restrict__ pstart,
                           const uint64_t *__restrict__ pdense, const uint64_t *__restrict__ hz, int32_t M, int32_t T,
                           PlanTotals *__restrict__ tot, SpWork *__restrict__ queue, int32_t *__restrict__ split_slot,
                           int32_t *__restrict__ split_row, const int32_t *__restrict__ row_nnz, int32_t mirror) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  const int64_t n_split = tot->n_split, n_split_work = tot->n_split_work;
  const int32_t a = order[r];
  const int64_t W = int64_t(skey[r]);
  if (W <= 0) return;
  const int64_t r0 = row_ptr[a], r1 = row_ptr[a + 1];
  unsigned long long *ng = reinterpret_cast<unsigned long long *>(&tot->n_gather);
  if (r < n_split) {
    split_slot[a] = r;
    split_row[r] = a;
    const int64_t q = wbase[r];
    const int32_t ns = sp_split_shares(W, gmass[0]);
    for (int32_t s = 0; s < ns; s++) {
      SpWork x{};
      x.k0 = r0 + (r1 - r0) * s / ns;
      x.k1 = r0 + (r1 - r0) * (s + 1) / ns;
      x.row = a;
      x.kind = -2;
      x.gslot = mirror ? -1 : int32_t(atomicAdd(ng, 1ull));  // (a mirrored share counts tile 0 only: no buckets)
      queue[q + s] = x;
    }
  } else {
    SpWork x{};
    x.k0 = r0;
    x.k1 = r1;
    x.st = pstart[a];
    x.dn = pdense[a];
    x.hz[0] = hz[2 * a];
    x.hz[1] = hz[2 * a + 1];
    x.row = a;
    x.kind = -1;
    x.gslot = ((x.dn & 1ull) && (x.hz[0] & kGatherFlag)) ? int32_t(atomicAdd(ng, 1ull)) : -1;
    x.est = row_nnz[a];
    queue[n_split_work + (r - n_split)] = x;
  }
}

// Mirroring: the staging slot of the split row at every column rank below kTW (mslot preset to -1), and every
// slot's column rank (srank, the inverse).
__global__ void k_sp_mirror_slots(const int32_t *__restrict__ split_row, int32_t n_split,
                                  const int32_t *__restrict__ pos_of, int32_t *__restrict__ mslot,
                                  int32_t *__restrict__ srank) {
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_split) return;
  const int32_t ra = relabel_pos(pos_of, uint32_t(split_row[r]));
  if (ra < kTW) mslot[ra] = r;
  srank[r] = ra;
}

__global__ void k_sp_totals(PlanTotals *__restrict__ tot, const int64_t *__restrict__ epre,
                            const int64_t *__restrict__ spre, int64_t n, int32_t *__restrict__ qctr) {
  tot->n_chunks = tot->n_split_work + (tot->n_active - tot->n_split);
  tot->work_total = epre[n];
  tot->self_total = spre ? spre[n] : n;
  qctr[0] = qctr[1] = 0;
}

int bits_for(int64_t v) {
  int b = 1;
  while ((int64_t(1) << b) < v) b++;
  return b;
}

// Item frequencies of a log (the multi-GPU owner map and the planner's column estimate).  Zipf logs put most
// interactions on a few items, whose global counters would serialise at L2 under per-interaction atomics;
// each workgroup therefore keeps the items it sees most in an LDS table (open addressing: an item claims a
// slot with a compare-and-swap, kHistProbe probes at most) and flushes it once; an item that finds no slot
// (the table is full of the workgroup's earlier items) goes to a global 64-bit atomic -- such items are rare
// in the workgroup's share, so their counters are not contended.  Whatever order the ids come in.
constexpr int kHistSlots = 8192, kHistProbe = 8, kHistThreads = 1024;
__global__ __launch_bounds__(kHistThreads) void k_item_counts(const int32_t *__restrict__ items, int64_t n, int32_t M,
                                                              unsigned long long *__restrict__ counts) {
  __shared__ uint32_t hk[kHistSlots], hc[kHistSlots];
  for (int i = threadIdx.x; i < kHistSlots; i += kHistThreads) {
    hk[i] = 0u;
    hc[i] = 0u;
  }
  __syncthreads();
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;  // a contiguous share per workgroup
  const int64_t i0 = int64_t(blockIdx.x) * per, i1 = min(n, i0 + per);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kHistThreads) {
    const uint32_t it = uint32_t(items[i]);
    if (it >= uint32_t(M)) continue;
    const uint32_t key = it + 1u;
    uint32_t h = (it * 0x9E3779B1u) >> (32 - 13);
    bool done = false;
    for (int p = 0; p < kHistProbe; p++) {
      const uint32_t cur = atomicCAS(hk + h, 0u, key);
      if (cur == 0u || cur == key) {
        atomicAdd(hc + h, 1u);
        done = true;
        break;
      }
      h = (h + 1u) & (kHistSlots - 1u);
    }
    if (!done) atomicAdd(counts + it, 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHistSlots; i += kHistThreads)
    if (hk[i]) atomicAdd(counts + (hk[i] - 1u), (unsigned long long)hc[i]);
}
}  // namespace

Status launch_item_counts(hipStream_t s, const int32_t *items, int64_t n, int32_t M, int64_t *counts) {
  COOC_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * size_t(M), s));
  if (n > 0) {
    int dev = 0, n_cu = 256;
    COOC_HIP_TRY(hipGetDevice(&dev));
    COOC_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t want = (n + 4095) / 4096;
    k_item_counts<<<unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu) * 2))), kHistThreads, 0, s>>>(
        items, n, M, reinterpret_cast<unsigned long long *>(counts));
    COOC_HIP_TRY(hipGetLastError());
  }
  return Status::Ok();
}

// ---- Counter::run_sparse, its planning phases (R: what they share, cooc_sparse.h) -----------------------------

// The checks of the call and the workspace every later phase takes for granted.
Status Counter::sparse_reserve(SparseRun &R) {
  const int32_t M = M_;
  const int64_t U = R.U, n = R.n;
  hipStream_t s = R.s;
  // column relabel (batch windows; not streaming ones, whose delta rows merge into column-ordered global
  // rows): the batch's kTW most frequent items -- its own frequencies, or the caller's global counts -- become
  // tile 0 and the rest move one tile up (k_relabel_*), so that the hot columns fill the u16 tile 0 and the
  // tiling works whatever order the ids come in.  Rows come out in that column order (CountResult.rank_of).
  // Mc: the columns of the relabelled space (M + kTW; holes where the hot items were).
  // (sparse_relabel drops the relabel again when the ids already put the hot items in tile 0)
  R.relabel = relabel_ && !R.win && M > kTW && int64_t(M) + kTW <= int64_t(kSpMaxTiles) * kTW;
  R.Mc = R.relabel ? M + kTW : M;
  R.T = int32_t((int64_t(R.Mc) + kTW - 1) / kTW);
  const int32_t T = R.T;
  if (T > kSpMaxTiles)
    return Status{1, "n_items > " + std::to_string(int64_t(kSpMaxTiles) * kTW) + " is not supported"};
  if (n > int64_t(INT32_MAX)) return Status{1, "more than 2^31 interactions in one window"};
  // (a contribution keeps its list index in bits 0..30, kSelfBit in bit 31)
  if (U > int64_t(kListMask)) return Status{1, "more than 2^31 - 1 user lists in one window"};
  const int64_t U1 = std::max<int64_t>(U, 1), n1 = std::max<int64_t>(n, 1);
  COOC_TRY(tot_.reserve(sizeof(PlanTotals)));
  COOC_TRY(queue_.reserve(sizeof(int32_t) * 4));
  COOC_TRY(keys_in_.reserve(sizeof(uint32_t) * (n1 + 1)));
  COOC_TRY(vals_in_.reserve(sizeof(uint32_t) * (n1 + 1)));
  COOC_TRY(keys_out_.reserve(sizeof(uint32_t) * (n1 + 1)));
  COOC_TRY(vals_out_.reserve(sizeof(uint32_t) * (n1 + 1)));
  R.n_groups0 = (n1 + 7 * U1) / 8 + 4;
  R.n_groups1 = (n1 + 3 * U1) / 4 + 4;
  COOC_TRY(sp_arena_.reserve(sizeof(uint4) * size_t(R.n_groups1)));   // arena1: lists padded to 4 ids
  COOC_TRY(sp_arena0_.reserve(sizeof(uint4) * size_t(R.n_groups0)));  // arena0: tile-0 ids padded to 8
  COOC_TRY(sp_pbase_.reserve(sizeof(uint64_t) * size_t(2 * U1 + 1)));  // packed region lengths, their prefix
  COOC_TRY(sp_ulen_.reserve(sizeof(uint32_t) * size_t(U1)));  // list lengths (u32) for the pair-work prefix
  COOC_TRY(sp_tb_.reserve(sizeof(int32_t) * size_t(U1) * size_t(T + 2)));
  COOC_TRY(sp_tbc_.reserve(sizeof(int4) * size_t(U1)));
  if (8 * R.n_groups0 > int64_t(INT32_MAX)) return Status{1, "more than 2^31 arena positions in one window"};
  COOC_TRY(epre_.reserve(sizeof(int64_t) * (n1 + 1)));
  COOC_TRY(row_ptr_.reserve(sizeof(int64_t) * (M + 1)));
  COOC_TRY(rowsum_.reserve(sizeof(int64_t) * M));
  COOC_TRY(row_base_.reserve(sizeof(int64_t) * (M + 1)));
  COOC_TRY(row_nnz_.reserve(sizeof(int32_t) * M));
  COOC_TRY(sp_roww_.reserve(sizeof(int64_t) * M));
  COOC_TRY(sp_pstart_.reserve(sizeof(uint64_t) * M));
  COOC_TRY(sp_pdense_.reserve(sizeof(uint64_t) * M));
  COOC_TRY(sp_hz_.reserve(sizeof(uint64_t) * 2 * M));
  COOC_TRY(order_keys_.reserve(sizeof(uint64_t) * 2 * M));
  COOC_TRY(order_.reserve(sizeof(int32_t) * 2 * M));
  COOC_TRY(row_nch_.reserve(sizeof(int32_t) * M));           // work items per row (split rows)
  COOC_TRY(ord_nch_.reserve(sizeof(int32_t) * M));           // ... in sorted order
  COOC_TRY(ord_cbase_.reserve(sizeof(int32_t) * (M + 1)));   // ... exclusive prefix
  COOC_TRY(sp_est_.reserve(sizeof(float) * (T * kEstK + T)));
  COOC_HIP_TRY(hipMemsetAsync(tot_.p, 0, sizeof(PlanTotals), s));
  COOC_HIP_TRY(hipMemsetAsync(epre_.p, 0, sizeof(int64_t), s));
  // the planner's sorts and its select (cooc_radix.h), and its prefix sums (cooc_scan.h): tile statuses for the
  // largest of them, reserved once up front
  COOC_TRY(sort_tmp_.reserve(std::max({radix_sort_tmp_bytes<uint32_t, uint32_t>(n1),
                                       radix_sort_tmp_bytes<uint64_t, int32_t>(M), select_tmp_bytes(M)})));
  COOC_TRY(scan_state_.reserve(
      sizeof(unsigned long long) *
      size_t(scan_state_words(std::max({n1, U1, int64_t(M), R.win ? R.win->n_contrib : int64_t(0)})))));
  if (U > 0) k_list_len32<<<nblocks(U, 256), 256, 0, s>>>(U, R.up, sp_ulen_.as<uint32_t>());
  return Status::Ok();
}

// 0. The column relabel: decides it (one sync) and builds its maps.
Status Counter::sparse_relabel(SparseRun &R) {
  const int32_t M = M_;
  const int64_t U = R.U, n = R.n;
  hipStream_t s = R.s;
  if (R.relabel) {
    uint32_t *keys_in = keys_in_.as<uint32_t>(), *vals_in = vals_in_.as<uint32_t>();
    uint32_t *keys = keys_out_.as<uint32_t>(), *vals = vals_out_.as<uint32_t>();
    int64_t *epre = epre_.as<int64_t>(), *row_ptr = row_ptr_.as<int64_t>();
    COOC_TRY(sp_rank_.reserve(sizeof(int32_t) * size_t(3 * M + kTW + 8) + size_t(M)));
    COOC_TRY(sp_rkeys_.reserve(sizeof(uint64_t) * size_t(2 * M) + sizeof(int64_t) * size_t(R.Mc)));
    R.pos_of = sp_rank_.as<int32_t>();
    R.hot_col = R.pos_of + M;
    int32_t *ids = R.hot_col + kTW, *order = ids + M, *n_sel = order + M;
    uint8_t *hot = reinterpret_cast<uint8_t *>(n_sel + 8);
    uint64_t *rk_in = sp_rkeys_.as<uint64_t>(), *rk_out = rk_in + M;
    int64_t *fc = reinterpret_cast<int64_t *>(rk_out + M);
    int64_t n_tot = n;
    if (!R.owner) {  // the log's own frequencies: the row lengths of the item-sorted contributions
      const int64_t waves = std::min<int64_t>(std::max<int64_t>(U, 1), 65536);
      if (U > 0) k_sp_contribs<<<nblocks(waves * 64, 256), 256, 0, s>>>(U, R.up, R.items, M, keys_in, vals_in);
      if (n > 0) {
        COOC_TRY(radix_sort_pairs(keys_in, vals_in, keys, vals, n, 0, bits_for(M), false, sort_tmp_.p, s));
        COOC_TRY(launch_scan<true>(ScanUserLen{vals, sp_ulen_.as<uint32_t>()}, epre + 1, n,
                                   scan_state_.as<unsigned long long>(), &tot_.as<PlanTotals>()->err, s));
      }
      k_sp_row_ptr<<<nblocks(int64_t(M) + 1, 256), 256, 0, s>>>(keys, n, M, row_ptr);
      R.sorted_early = true;
    } else {
      n_tot = R.n_freq;
    }
    k_rank_keys<<<nblocks(M, 256), 256, 0, s>>>(row_ptr, R.owner ? R.freq : nullptr, M, rk_in, ids, hot);
    const int fb = bits_for(std::max<int64_t>(n_tot, 1) + 1);
    COOC_TRY(radix_sort_pairs(rk_in, ids, rk_out, order, M, 0, fb, true, sort_tmp_.p, s));
    k_hot_mark<<<nblocks(kTW, 256), 256, 0, s>>>(order, kTW, hot);
    COOC_TRY(select_flagged(hot, M, R.hot_col, n_sel, sort_tmp_.p, s));  // kTW of them
    // ids that already put (nearly) every hot item in tile 0 keep their order: the relabel would only add
    // its lookups (an item-ranked log; measured 4 ms per C3 share)
    {
      int32_t *d_ov = n_sel + 4;
      COOC_HIP_TRY(hipMemsetAsync(d_ov, 0, sizeof(int32_t), s));
      k_hot_overlap<<<nblocks(kTW, 256), 256, 0, s>>>(hot, kTW, d_ov);
      int32_t ov = 0;
      COOC_HIP_TRY(hipMemcpyAsync(&ov, d_ov, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
#ifdef COOC_SP_STATS
      fprintf(stderr, "[sp] relabel: %d of the %d hot items have ids below %d -> %s\n", ov, kTW, kTW,
              ov >= kTW - kTW / 16 ? "kept ids" : "relabelled");
#endif
      if (ov >= kTW - kTW / 16) {
        R.relabel = false;
        R.Mc = M;
        R.T = int32_t((int64_t(R.Mc) + kTW - 1) / kTW);
        R.pos_of = R.hot_col = nullptr;
      }
    }
    if (R.relabel) {
      k_relabel_pos<<<nblocks(M, 256), 256, 0, s>>>(hot, rk_in, M, R.pos_of, fc);
      R.hot_u8 = hot;
      k_relabel_hot<<<nblocks(kTW, 256), 256, 0, s>>>(R.hot_col, rk_in, R.pos_of, fc);
      COOC_HIP_TRY(hipGetLastError());
      R.freq_col = fc;
    }
  }
  last_hot_col_ = R.hot_col;
  last_pos_of_ = R.pos_of;
  last_mc_ = R.Mc;
  return Status::Ok();
}

// 1. The users' lists regrouped by tile + the (item, user) contributions (owner != NULL: of this part's rows);
// 2. the contributions regrouped by row (the keyBy(itemA) of FlinkCooccurrences.java:152); 3. the row pointer;
// 4. the pair-work prefix (and a window's self-flag prefix).
Status Counter::sparse_regroup(SparseRun &R) {
  const int32_t M = M_, T = R.T;
  const int64_t U = R.U, n = R.n;
  const int32_t *owner = R.owner;
  hipStream_t s = R.s;
  const int64_t U1 = std::max<int64_t>(U, 1);
  const int64_t waves = std::min<int64_t>(std::max<int64_t>(U, 1), 65536);
  PlanTotals *tot = tot_.as<PlanTotals>();
  uint32_t *keys_in = keys_in_.as<uint32_t>(), *vals_in = vals_in_.as<uint32_t>();
  uint32_t *keys = keys_out_.as<uint32_t>(), *vals = vals_out_.as<uint32_t>();
  int64_t *epre = epre_.as<int64_t>();
  uint64_t *plen = sp_pbase_.as<uint64_t>(), *pbase = plen + U1;
  unsigned long long *scan_st = scan_state_.as<unsigned long long>();
  int64_t *scan_err = &tot->err;
  // the bitmaps of the user passes (hot ids after a relabel; the part's rows)
  const int64_t n_words = (int64_t(M) + 31) / 32;
  COOC_TRY(sp_bits_.reserve(sizeof(uint32_t) * size_t(2 * n_words + 2)));
  uint32_t *hotbm = R.relabel ? sp_bits_.as<uint32_t>() : nullptr;
  uint32_t *minebm = owner ? sp_bits_.as<uint32_t>() + n_words : nullptr;
  if (hotbm) k_bits_hot<<<nblocks(n_words, 256), 256, 0, s>>>(R.hot_u8, M, hotbm);
  if (minebm) k_bits_owner<<<nblocks(n_words, 256), 256, 0, s>>>(owner, R.part, M, minebm);
  if (owner) {
    COOC_TRY(sp_ownc_.reserve(sizeof(int32_t) * size_t(U1)));
    COOC_TRY(sp_ownoff_.reserve(sizeof(int64_t) * size_t(U1 + 1)));
  }
  COOC_HIP_TRY(hipMemsetAsync(pbase, 0, sizeof(uint64_t), s));
  if (U > 0) {
    k_sp_tile_counts<<<nblocks(waves * 64, 256), 256, 0, s>>>(U, R.up, R.items, M, plen, owner, R.part,
                                                             sp_ownc_.as<int32_t>(), R.pos_of, hotbm, minebm);
    COOC_TRY(launch_scan<true>(ScanU64{plen}, pbase + 1, U, scan_st, scan_err, s));
  }
  int64_t *ownoff = owner ? sp_ownoff_.as<int64_t>() : nullptr;
  if (owner) {  // owned contributions per user -> their offsets
    COOC_HIP_TRY(hipMemsetAsync(ownoff, 0, sizeof(int64_t), s));
    if (U > 0) {
      COOC_TRY(launch_scan<true>(ScanI32{sp_ownc_.as<int32_t>()}, ownoff + 1, U, scan_st, scan_err, s));
    }
  }
  if (U > 0) {
    k_sp_tile_lists<<<nblocks(waves * 64, 256), 256, 0, s>>>(
        U, R.up, R.items, M, T, sp_tb_.as<int32_t>(), sp_tbc_.as<int4>(), sp_arena0_.as<uint16_t>(),
        sp_arena_.as<uint32_t>(), pbase, (R.win || R.sorted_early) ? nullptr : keys_in, vals_in, owner, R.part, ownoff,
        tot, R.pos_of, hotbm, minebm);
    COOC_HIP_TRY(hipGetLastError());
  }
  R.n_c = n;
  if (R.win) {
    R.n_c = R.win->n_contrib;
    if (R.win->n_users > 0)
      k_sp_window_contribs<<<nblocks(std::min<int64_t>(R.win->n_users, 65536) * 64, 256), 256, 0, s>>>(
          R.win->n_users, R.up, R.items, R.win->old, R.win->cbase, keys_in, vals_in);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (owner) {
    COOC_HIP_TRY(hipMemcpyAsync(&R.n_c, ownoff + U, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }
  const int64_t n_c = R.n_c;
  if (n_c > 0 && !R.sorted_early) {
    COOC_TRY(radix_sort_pairs(keys_in, vals_in, keys, vals, n_c, 0, bits_for(M), false, sort_tmp_.p, s));
    COOC_TRY(launch_scan<true>(ScanUserLen{vals, sp_ulen_.as<uint32_t>()}, epre + 1, n_c, scan_st, scan_err, s));
  }
  if (R.win) {
    COOC_TRY(sp_spre_.reserve(sizeof(int64_t) * size_t(n_c + 2)));
    R.spre = sp_spre_.as<int64_t>();
    COOC_HIP_TRY(hipMemsetAsync(R.spre, 0, sizeof(int64_t), s));
    if (n_c > 0) {
      COOC_TRY(launch_scan<true>(ScanSelfFlag{vals}, R.spre + 1, n_c, scan_st, scan_err, s));
    }
  }
  if (!R.sorted_early) k_sp_row_ptr<<<nblocks(int64_t(M) + 1, 256), 256, 0, s>>>(keys, n_c, M, row_ptr_.as<int64_t>());
  return Status::Ok();
}

// The work queue: the split rows' shares, then every other row, heaviest first; the mirror slots when the split
// shares are mirrored.  Built again, without mirroring, when a mirrored attempt deferred a row (run_sparse).
Status Counter::sparse_queue(SparseRun &R) {
  const int32_t M = M_;
  hipStream_t s = R.s;
  PlanTotals *tot = tot_.as<PlanTotals>();
  const int64_t n_split = R.tot.n_split;
  COOC_HIP_TRY(hipMemsetAsync(&tot->n_gather, 0, sizeof(int64_t), s));
  k_sp_queue<<<nblocks(M, 256), 256, 0, s>>>(order_.as<int32_t>() + M, order_keys_.as<uint64_t>() + M,
                                            ord_cbase_.as<int32_t>(), sp_est_.as<float>() + R.T * kEstK,
                                            row_ptr_.as<int64_t>(), sp_pstart_.as<uint64_t>(),
                                            sp_pdense_.as<uint64_t>(), sp_hz_.as<uint64_t>(), M, R.T, tot,
                                            sp_queue_.as<SpWork>(), split_slot_.as<int32_t>(),
                                            split_row_.as<int32_t>(), row_nnz_.as<int32_t>(), R.mirror ? 1 : 0);
  COOC_HIP_TRY(hipGetLastError());
  if (R.mirror) {
    COOC_HIP_TRY(hipMemsetAsync(sp_mslot_.p, 0xff, sizeof(int32_t) * kTW, s));
    k_sp_mirror_slots<<<nblocks(n_split, 256), 256, 0, s>>>(split_row_.as<int32_t>(), int32_t(n_split), R.pos_of,
                                                           sp_mslot_.as<int32_t>(), sp_srank_.as<int32_t>());
    COOC_HIP_TRY(hipGetLastError());
  }
  return Status::Ok();
}

// 5. The expected distinct keys per tile; 6. every row's plan and the totals (one sync); 7. the rows ordered by
// pair work and the work queue.
Status Counter::sparse_plan(SparseRun &R) {
  const int32_t M = M_, T = R.T;
  hipStream_t s = R.s;
  PlanTotals *tot = tot_.as<PlanTotals>();
  int64_t *epre = epre_.as<int64_t>(), *row_ptr = row_ptr_.as<int64_t>();
  float *est = sp_est_.as<float>(), *gmass = est + T * kEstK;
  // column frequencies: of this log's interactions (owner == NULL), else the caller's global counts; in rank
  // order after a relabel
  const int64_t n_est = R.freq ? R.n_freq : R.win ? R.n_c : R.n;
  if (n_est > 0)
    k_sp_est<<<dim3(T, kEstK), 256, 0, s>>>(row_ptr, R.relabel ? R.freq_col : R.freq, R.Mc, n_est, est, gmass);
  else COOC_HIP_TRY(hipMemsetAsync(est, 0, sizeof(float) * (T * kEstK + T), s));
  k_sp_plan<<<nblocks(M, 256), 256, 0, s>>>(M, T, row_ptr, epre, est, gmass, rowsum_.as<int64_t>(),
                                            sp_roww_.as<int64_t>(), sp_pstart_.as<uint64_t>(),
                                            sp_pdense_.as<uint64_t>(), sp_hz_.as<uint64_t>(),
                                            order_keys_.as<uint64_t>(),
                                            order_.as<int32_t>(), row_nch_.as<int32_t>(), row_nnz_.as<int32_t>(),
                                            row_base_.as<int64_t>(), tot, R.spre, mid_off_ ? 0 : 1, R.pos_of);
  k_sp_totals<<<1, 1, 0, s>>>(tot, epre, R.spre, R.n_c, queue_.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(h_tot_, tot, sizeof(PlanTotals), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (h_tot_->err & 1) return Status{1, "item id outside [0, n_items)"};
  if (h_tot_->err & 8) return Status{2, "internal bounds check failed (planner prefix sum)"};
  R.tot = *h_tot_;  // (h_tot_ itself takes every attempt's totals)
  const int64_t n_split = R.tot.n_split;
  COOC_TRY(sp_queue_.reserve(sizeof(SpWork) * size_t(std::max<int64_t>(R.tot.n_chunks, 1))));
  COOC_TRY(split_row_.reserve(sizeof(int32_t) * std::max<int64_t>(n_split, 1)));
  COOC_TRY(split_slot_.reserve(sizeof(int32_t) * M));
  {
    // the keys are the rows' pair work, at most work_total: only its bits are sorted (C3's 1/8 share: 35 of 64,
    // five 8-bit passes instead of eight; the same order)
    const int wb = std::min(64, bits_for(R.tot.work_total + 1));
    COOC_TRY(radix_sort_pairs(order_keys_.as<uint64_t>(), order_.as<int32_t>(), order_keys_.as<uint64_t>() + M,
                              order_.as<int32_t>() + M, M, 0, wb, true, sort_tmp_.p, s));
    k_sp_gather_nwork<<<nblocks(M, 256), 256, 0, s>>>(order_.as<int32_t>() + M, row_nch_.as<int32_t>(), M,
                                                      ord_nch_.as<int32_t>());
    COOC_TRY(launch_scan<false>(ScanI32{ord_nch_.as<int32_t>()}, ord_cbase_.as<int32_t>(), M,
                                scan_state_.as<unsigned long long>(), &tot->err, s));
  }
  // Mirroring: a split row a whose column lies in tile 0 takes its cells above tile 0 from the entries C[b, a]
  // of the rows b there (C[a, b] = C[b, a] off the diagonal: both sides count the pairs of a and b in the same
  // lists -- also under user_cut, which cuts the lists before either side is counted), so its shares walk the
  // lists' tile-0 parts only.  Needs every row's own pass to see every list (no owner), the rows whole (no
  // window: a delta row is not symmetric) and the tile-0 chunks of k_sp_main / k_sp_small / k_sp_tiny as the
  // emitters (not COOC_FLAG_SORT_ROWS); a deferred row does not mirror, so a run that defers one is repeated
  // without (run_sparse).  COOC_SP_MIRROR=0: off (A/B).
  R.mirror = !mirror_off_ && !R.owner && !R.win && !sort_rows_ && n_split > 0 && R.tot.split_rank_hi <= kTW;
  if (R.mirror) COOC_TRY(sp_mslot_.reserve(sizeof(int32_t) * kTW));
  if (R.mirror) COOC_TRY(sp_srank_.reserve(sizeof(int32_t) * size_t(n_split)));
  // the mirrored cells' per-source-row records (cooc_sparse.h, SpArgs.mrec)
  R.mstage = R.mirror && R.Mc > kTW;
  R.mrec_w = (n_split + 15) & ~int64_t(15);
  return sparse_queue(R);
}

}  // namespace cooc
