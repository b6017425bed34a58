// cooc_sparse.h — what the three files of the large-universe path share (internal): cooc_sparse_plan.hip (the
// planner), cooc_sparse.hip (the row-per-workgroup accumulate kernel and Counter::run_sparse; the algorithm is
// described at its top) and cooc_sparse_rows.hip (the sorting kernels of the small, tiny and deferred rows).
#pragma once

#include "cooc_device.h"

#include <utility>

#ifdef COOC_SP_STATS
#define STAT_CLOCK() wall_clock64()
#define STAT_ADD(k, v) do { if (threadIdx.x == 0) S_.st[k] += (v); } while (0)  // LDS: keeps occupancy
// SpArgs.stats: 64 words per k_sp_main launch (big, mid), then k_sp_small's (cooc_sparse_rows.hip)
constexpr int kSmStatBase = 128, kSpStatWords = 192;
#else
#define STAT_CLOCK() 0ull
#define STAT_ADD(k, v) do {} while (0)
#endif

namespace cooc {

// One work item of k_sp_main, everything its start needs in one 64-B record (k_sp_queue).
struct SpWork {
  int64_t k0, k1;   // contribution range (row-sorted)
  uint64_t st, dn;  // chunk plan: bit t of st = a chunk starts at tile t, of dn = tile t is dense
  uint64_t hz[2];   // 2 bits per chunk-start tile: its hash table has kHashMin << code slots
  int32_t row;
  int32_t kind;     // -1: a whole row; -2: a share of a split row (every tile, into its staging row)
  int32_t gslot;    // >= 0: the item runs in gather mode (its tails go through buckets)
  int32_t est;      // a whole row's expected keys (planner estimate; sizes its output region)
};

struct SpArgs {
  const SpWork *queue;
  PlanTotals *tot;
  int32_t *qctr;            // this launch's work counter (k_sp_main: the queue range [q_begin, q_end))
  int64_t q_begin, q_end;
  const uint32_t *vals;     // contributions: user index, item-sorted
  const int32_t *tb;        // [U x (T + 2)] a user's tile-0 range in arena0, its tile starts in arena1
  const int4 *tbc;          // [U] a user's {tb[0], tb[T + 1], tb[1], tb[T]}: whole lists and tile-0 parts (NULL: from tb)
  const uint4 *tarena;      // arena1: the lists' ids of tiles >= 1 (u32), in 16-B groups
  const uint4 *tarena0;     // arena0: the lists' tile-0 ids (u16), in 16-B groups
  const int64_t *epre;      // [n_contrib + 1] prefix of the contributions' list lengths (pair work)
  const float *gmass;       // [T] share of the interactions in each tile
  uint32_t *staging;        // [n_split x sstride] (mirrored into records, mrec below: the rows' tile-0 heads alone)
  int64_t sstride;          // staging row stride: M rounded up to 4 (16-B aligned rows); kTW with records
  const int32_t *split_slot;
  int32_t *col_out;
  uint32_t *cnt_out;
  unsigned long long *bump;
  int64_t cap;
  int64_t slab;
  int64_t *row_base;
  int32_t *row_nnz;
  int32_t M, T;
  unsigned long long *stats;  // COOC_SP_STATS: per-phase clocks and counts
  int64_t n_contrib, n_users, n_groups, n_groups0;
  uint4 *scratch;           // gather mode: per-workgroup tail buckets, scr_cap groups each
  int64_t scr_cap;          // 0: gather mode off
  const int64_t *rowsum;    // [M] closed-form row sums W_a - c_a (k_sp_plan): every whole row is checked
  const int64_t *spre;      // streaming window: [n_contrib + 1] prefix of the kSelfBit flags; NULL: all set
  int32_t *deferred;        // [M] whole rows left to the sort path (k_srb_row, after this launch), tot->n_deferred of them
  int32_t sort_all;         // COOC_FLAG_SORT_ROWS: every whole row goes to that path (A/B and tests)
  int32_t any_order;        // COOC_FLAG_ANY_ORDER: hash chunks emitted as the waves hold them (no column ranking)
  // column relabel (batch windows, k_relabel_*): the kernels work in relabelled column space -- tile 0 holds
  // the batch's kTW most frequent items (hot_col[c], ascending ids), column c >= kTW the item c - kTW (its
  // own id shifted one tile up; the hot items leave holes there) -- and write the item ids to the output.
  // NULL: identity (streaming windows, and universes of at most one tile).
  const int32_t *hot_col;   // [kTW] column < kTW -> item id
  const int32_t *pos_of;    // [M] item id -> column
  // mirroring (every split row's column in tile 0; run_sparse): a split share counts tile 0 only.  Its row's
  // columns above tile 0 are the entries C[b, a] = C[a, b] of the rows b of column rank >= kTW, which those
  // rows' tile-0 chunks (dense, hash, or the sorted runs of the small and tiny rows) hand over (mrec below)
  const int32_t *mslot;     // [kTW] column rank -> staging slot of the split row there, -1 elsewhere
  int32_t mirror_hi;        // 1 + the largest split row's column rank; 0: mirroring off
  // the mirrored cells: the source row of column rank rb >= kTW owns the contiguous record mrec[(rb - kTW) *
  // mrec_w ...], whose cell `slot` is C[rb, split_row[slot]] -- a row's cells lie in a few neighbouring 64-B lines
  // (one line per split row, 4 MB apart, when they went into full-width staging rows) -- and staging holds the
  // split rows' tile-0 heads alone (sstride = kTW); the finalize transposes the records tile-wise (k_sp_tail_pass)
  uint32_t *mrec;           // [(Mc - kTW) x mrec_w] (NULL: no column above tile 0, no source)
  const int32_t *srank;     // [n_split] slot -> its split row's column rank (mslot's inverse)
  int32_t mrec_w;           // cells per record: n_split rounded up to 16 (64-B records)
  int32_t n_split;
};

// the transposing finalize: source rows per tile, and the slots whose cell sums a workgroup keeps in LDS at a
// time (8 KB; more split rows take further sweeps over the tiles)
constexpr int kTailB = 64, kTailMaxSlots = 1024;

// What the phases of Counter::run_sparse share: the call, then what each phase leaves for the later ones.
struct SparseRun {
  // the call (run_sparse's arguments)
  int64_t U;
  const int64_t *up;
  const int32_t *items;
  int64_t n;
  hipStream_t s;
  KernelTimer *timer;
  const int32_t *owner;
  int32_t part;
  const int64_t *freq;
  int64_t n_freq;
  const SparseWindow *win;
  // sparse_reserve: the column space -- the items' ids, or after a relabel Mc = n_items + kTW columns (holes
  // where the hot items were) -- in T tiles; the arenas' sizes in 16-B groups
  bool relabel;
  int32_t Mc, T;
  int64_t n_groups0, n_groups1;
  // sparse_relabel (which may drop the relabel again): the maps (NULL: identity), the hot ids' flags, the
  // frequencies in column order; sorted_early: the contributions are already sorted by row
  int32_t *hot_col, *pos_of;
  const uint8_t *hot_u8;
  const int64_t *freq_col;
  bool sorted_early;
  // sparse_regroup: the contributions (every interaction, or those of the owned rows, or a window's
  // positions) and, for a window, the prefix of their self flags in row order
  int64_t n_c;
  int64_t *spre;
  // sparse_plan: the host copy of the plan's totals; mirroring on (sparse_queue builds the queue for it), and
  // with it (mstage: when there are columns above tile 0) the mirrored cells' records, mrec_w cells each
  PlanTotals tot;
  bool mirror, mstage;
  int64_t mrec_w;
  // sparse_sizes: the launches' grids, the gather scratch per workgroup (16-B groups; 0: none) and the gather
  // items it serves, the staging stride, the output region (cap entries, handed out in slabs; slack: what the
  // slabs may strand) and the kernels' arguments but for the output region of an attempt
  int64_t grid, grid_mid, grid_small, grid_tiny;
  bool mid_any;
  int64_t scr_cap, scr_cap_mid, n_gather;
  int64_t sstride, slab, slack, cap;
  SpArgs proto;
};

// (internal linkage, as when the three files were one translation unit: each compiles its own copy of the
// constants and helpers below, and the kernels' code is what it was before the split)
namespace {

#ifndef COOC_SP_THREADS
#define COOC_SP_THREADS 512
#endif
#ifndef COOC_SP_TSHIFT
#define COOC_SP_TSHIFT 14
#endif
constexpr int kSpThreads = COOC_SP_THREADS;  // 512: two workgroups per CU
constexpr int kSpWaves = kSpThreads / 64;
constexpr int kTShift = COOC_SP_TSHIFT;
constexpr int kTW = 1 << kTShift;  // dense tile width (16384: 64 KB of uint32 LDS counters)
constexpr int kSpMaxTiles = 64;                        // per-row plans are 64-bit tile masks
constexpr int kHashMax = 8192;                       // slots: keys + counts = the dense tile's 128 KB
constexpr int kWStage = kHashMax / 2;                  // hash compaction: entries staged in LDS for 16-B stores
constexpr int kHashMin = 1024;                         // one slot per thread at least
constexpr int kHashMaxTiles = (1 << 20) / kTW;          // a hash chunk spans <= 2^20 columns ...
constexpr int kL1Words = kHashMaxTiles * kTW / 1024;   // ... so its block bitmap is <= 1024 words
constexpr int kSpDb = 512;                             // contribution descriptors per batch
constexpr int kEstK = 84;                              // estimate table: W_k = 2^(k/2), k < kEstK
constexpr int kTinyW = 256;                           // rows of at most this many pairs: one wave each (k_sp_tiny)
constexpr int kSmallW = 4096;                          // ... of at most this many: one 512-thread workgroup each (k_sp_small)
constexpr int64_t kScrGroups = int64_t(1) << 21;       // gather scratch per workgroup (16-B groups of 4 ids)
// the output slabs of the small and tiny rows' kernels (cooc_sparse_rows.hip; run_sparse sizes the region's slack by them)
constexpr int64_t kSmallSlab = 16384;  // output entries reserved per workgroup at a time (k_sp_small, k_srb_row)
constexpr int kTinyThreads = 256, kTinyWaves = kTinyThreads / 64;
constexpr int64_t kTinySlab = 4096;    // output entries reserved per wave at a time (k_sp_tiny)
constexpr int kSpLds = kTW * 4 + 2 * kL1Words * 4 + kSpDb * 8 + (kSpDb + 4) * 4 + kSpThreads;  // (gb + info: 8 B per descriptor)

// Two shapes of the accumulate kernel, one queue.  Rows of at most kMidW pairs ("mid rows": at C3 the half
// million rows of 4K..64K pairs, mostly one dense tile 0 plus a sparse tail) run with FOUR 256-thread
// workgroups per CU instead of two 512-thread ones: their chunks are short latency chains (walk, barrier,
// compaction), so more independent chunks per CU hide more of them.  The LDS budget (40 KB per workgroup)
// holds because a count never exceeds its row's pair work W <= 65,535: the dense tile's counters are u16,
// two per LDS word (a ds_add of 1 << 16 for the odd column never carries), and hash tables have 4K slots
// (chunks of half the expected keys) over column spans of at most 2^19 (a 512-word block bitmap).
#ifndef COOC_SP_MID_W
#define COOC_SP_MID_W 65535
#endif
constexpr int64_t kMidW = COOC_SP_MID_W;
static_assert(kMidW <= 65535, "mid rows count in u16");
template <int Threads, int HashMax, int L1Words, int Db, bool U16, bool Rank = true>
struct SpShape {
  static constexpr int kThreads = Threads, kWaves = Threads / 64;
  static constexpr int kHashMax = HashMax;            // hash slots: keys [0, H) + counts [HashMax, HashMax + H)
  static constexpr int kWStage = HashMax / 2;         // compaction staging (entries) in the emptied table
  static constexpr int kL1Words = L1Words;            // block bitmap words: chunk spans <= L1Words * 1024 columns
  static constexpr int kHashMaxTiles = L1Words * 1024 / kTW;
  static constexpr int kDb = Db;                      // contribution descriptors per walk batch
  static constexpr bool kU16 = U16;                   // dense counters: u16 pairs (true) or u32
  static constexpr int kPer = U16 ? 8 : 4;            // dense counters per 16-B LDS word
  static constexpr int kRWords = (U16 ? kTW / 2 : kTW) > 2 * HashMax ? (U16 ? kTW / 2 : kTW) : 2 * HashMax;
  static constexpr bool kRank = Rank;                 // false: any-order rows only (no column ranking, no block bitmaps)
  static constexpr int kBmWords = Rank ? 2 * L1Words : 0;  // L1 + L1pre
  // sp_walk reads the compact list bounds a batch ahead (5 VGPRs held over the walk): the mid shapes, 128 VGPRs
  // with it and no scratch; the big shape would spill them (scratch 12 -> 20 B per lane).  Reading the next
  // work item's first batch ahead as well (over the compactions) spilled 11-13 VGPRs in the mid shapes: not kept
  static constexpr bool kAhead = U16;
  static constexpr int kLds = kRWords * 4 + kBmWords * 4 + Db * 8 + (Db + 4) * 4 + Threads;
};
using SpBig = SpShape<kSpThreads, kHashMax, kL1Words, kSpDb, false>;
using SpMid = SpShape<256, 4096, 512, 256, true>;  // 40.9 KB of LDS: three per CU (four at 38.9 KB with 2^18-column spans measured slower: more chunks)
// the mid shape of COOC_FLAG_ANY_ORDER runs: hash chunks leave unranked, so the 4 KB of block bitmaps go and a
// FOURTH workgroup fits a CU's 160 KB (36.1 KB + the static part each), with the same tables and column spans
using SpMidAny = SpShape<256, 4096, 512, 256, true, false>;
static_assert(SpMidAny::kLds + 4096 == SpMid::kLds && 4 * (SpMidAny::kLds + 1024) <= 160 * 1024, "four per CU");
static_assert(SpBig::kLds == kSpLds, "the big shape is the original kernel");

// the arenas' pads (k_sp_tile_lists): no column, so every walk skips them
constexpr uint32_t kSink = 0xFFFFFFFFu;
constexpr uint32_t kSink16 = 0xFFFFu;  // (arena0 pads; never a tile-0 id)

// A contribution's value: the index of the list its row walks; in a streaming window (spre != NULL) with
// kSelfBit when the walk includes the contribution's own position (a new position walks its user's whole
// history, an old one only the window's new items, see k_sp_window_contribs).  In a one-window batch every
// walk includes it (no bit: the self count of a row is its contribution count).
constexpr uint32_t kSelfBit = 0x80000000u, kListMask = 0x7FFFFFFFu;

// the item of relabelled column r: a table lookup in tile 0 (64 KB, cache resident), arithmetic above it
__device__ inline int32_t relabel_col(const int32_t *hot_col, uint32_t r) {
  if (!hot_col) return int32_t(r);
  return r < uint32_t(kTW) ? hot_col[r] : int32_t(r) - kTW;
}
__device__ inline int32_t relabel_pos(const int32_t *pos_of, uint32_t a) { return pos_of ? pos_of[a] : int32_t(a); }
__device__ inline int32_t sp_col(const SpArgs &A, uint32_t r) { return relabel_col(A.hot_col, r); }
// list u's whole bounds {tile-0 start, end (arena0), tail start, end (arena1)}: one 16-B record, or four tb loads
__device__ inline int4 sp_list_bounds(const SpArgs &A, uint32_t u) {
  if (A.tbc) return A.tbc[u];
  const int32_t *tbu = A.tb + int64_t(u) * (A.T + 2);
  return make_int4(tbu[0], tbu[A.T + 1], tbu[1], tbu[A.T]);
}
__device__ inline int32_t sp_rank(const SpArgs &A, int32_t a) { return relabel_pos(A.pos_of, uint32_t(a)); }

// Bounds checks of the global index math (COOC_SP_CHECK builds, for fault hunting): a failed check sets err
// bit 8 (COOC_ERR_STATE "internal bounds check") and skips the access; release builds compile them out.
#ifdef COOC_SP_CHECK
#define SP_CHECK(A, cond) ((cond) ? true : (atomicOr(reinterpret_cast<unsigned long long *>(&(A).tot->err), 8ull), false))
#else
#define SP_CHECK(A, cond) true
#endif

// Values every thread of the workgroup holds identically (read from LDS after a barrier): made
// explicitly uniform so that the branches on them are scalar and no barrier sits in exec-masked code.
__device__ inline uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline int32_t uni(int32_t v) { return int32_t(__builtin_amdgcn_readfirstlane(uint32_t(v))); }
// (readfirstlane returns an int: each half goes through uint32_t, or a low half >= 2^31 would
// sign-extend over the high half -- output positions >= 2^31 came out negative and their rows unwritten)
__device__ inline int64_t uni(int64_t v) {
  const uint64_t u = uint64_t(v);
  const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(u >> 32)));
  const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(u)));
  return int64_t((uint64_t(hi) << 32) | uint64_t(lo));
}

__device__ inline uint32_t wave_incl_scan(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// The ranking primitive of block_radix_sort (cooc_sparse_rows.hip): for a lane of `valid`, the lanes of `valid`
// whose kBits-bit digit equals its own, as the two 32-bit halves of the wave's lane mask.  d must be 0 in the lanes
// outside `valid` (they then drop out of every bit's ballot by themselves).  Per digit bit: nb = -1 where the bit is
// set, else 0 (v_bfe_i32), the ballot of the set bits (one v_cmp into an SGPR pair), and half &= ~(ballot ^ nb) (one
// v_bitop3_b32 per half): four vector instructions per bit.
struct WaveMask {
  uint32_t lo, hi;
  // the mask's lanes below this one (v_mbcnt_lo / _hi), and all of them
  __device__ uint32_t below() const { return __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)); }
  __device__ uint32_t count() const { return uint32_t(__builtin_popcount(lo)) + uint32_t(__builtin_popcount(hi)); }
};
// One digit bit's step.  The sign-extended bit is one v_bfe_i32 the compiler does not look into (as sp_bits,
// cooc_sparse.hip: from the builtin it makes a shift for the compare and an arithmetic shift for the mask), and
// half & ~(ballot ^ nb) (truth table 0x90) is the builtin: written with operators, the chain is re-associated into
// shifts, xors and an or tree of half as many instructions again.
template <int kB>
__device__ inline void wave_match_bit(WaveMask &m, uint32_t d) {
  uint32_t nb;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(nb) : "v"(d), "n"(kB));
  const uint64_t bb = __ballot(nb != 0u);
  m.lo = __builtin_amdgcn_bitop3_b32(m.lo, uint32_t(bb), nb, 0x90);
  m.hi = __builtin_amdgcn_bitop3_b32(m.hi, uint32_t(bb >> 32), nb, 0x90);
}
template <int... kB>
__device__ inline void wave_match_bits(WaveMask &m, uint32_t d, std::integer_sequence<int, kB...>) {
  (wave_match_bit<kB>(m, d), ...);
}
template <int kBits>
__device__ inline WaveMask wave_match(uint32_t d, bool valid) {
  const uint64_t vm = __ballot(valid);
  WaveMask m{uint32_t(vm), uint32_t(vm >> 32)};
  wave_match_bits(m, d, std::make_integer_sequence<int, kBits>());
  return m;
}

inline unsigned nblocks(int64_t n, int t) { return unsigned((n + t - 1) / t); }

}  // namespace

// cooc_sparse_rows.hip: the small and tiny rows of A's queue (its tail: tot->n_small rows, then tot->n_tiny),
// launched on s with the grid run_sparse sized the output region's slack for
Status launch_sp_small(const SpArgs &A, int64_t grid, hipStream_t s);
Status launch_sp_tiny(const SpArgs &A, int64_t grid, hipStream_t s);

}  // namespace cooc
