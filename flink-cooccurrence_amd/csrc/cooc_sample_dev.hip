// cooc_sample_dev.hip — the sampled mode's decisions on the device (cooc_sample_device): the item cut, the
// per-user reservoir with its counter-based draw and the feedback of every window of a device-resident log, from
// empty state.  The same contract as the host sampler (cooc_sample.cpp, include/cooc.h "sampled mode"), restating
// ItemInteractionCounterTwoInputStreamOperator.java:119-143 (item cut), :94-116 (feedback) and
// UserInteractionCounterOneInputStreamOperator.java:145-257 (reservoir), written down data-parallel:
//
//   item cut   rho = the record's rank among the window's records of its item (arrival order):
//              sample = rho < item_cut - count[i], count[i] as at the window's start;
//   user stage j = its rank among the window's records of its user, s = the sampled ones among those before it:
//              total = T[u] + j + 1; a sampled record with L[u] + s < user_cut fills slot L[u] + s, any other
//              sampled record draws k = sample_draw(seed, u, total) and replaces slot k < user_cut or feeds its
//              item back;
//   slots      a slot written more than once keeps the writer that is last in arrival order: every writer raises
//              the slot's stamp to 1 + its index in the whole call (an integer max), then the writer whose stamp
//              stands stores its item.  The index grows across windows, so the stamps are never reset;
//   the end    count[i] += sampled - feedbacks, L[u] += fills, T[u] += records.
//
// rho and (j, s) come from two stable radix sorts of the window's (id, index) pairs (cooc_radix.h) over the bits
// the ids need, a prefix sum of the run heads (cooc_scan.h: the run's number, then its first position) and one
// of the sample flags in user order.  Integer adds and max are the only atomics, so a call's outputs do not depend
// on the order they land in.  Every window runs the same launches whatever its data; sample_window takes the
// carried state as arguments (SampleState).  The streaming mode's device sampler (cooc_sampling_enable_device,
// SampleStream at the end of this file) runs the same item stage and user order window by window on state it
// keeps for the life of a context, and emits its decisions instead of writing an arena.  With a communicator of
// world > 1 the window is the ranks' records in rank order: the ranks exchange their per-item histograms and their
// feedbacks each window (ItemCutExchange, in front of SampleStream below), the cut is taken at rho + the lower
// ranks' records and the replicated counters are committed from the job's totals.  cooc_sample_owned is the
// stateless pass in that form: sample_window_ranks (behind the exchange's kernels) runs sample_window's stages with
// the exchange in between, every rank on its own users' shard of a device-resident log; cooc_ctx::sample_log at the
// end of the file is the body of both stateless entry points.
#include <algorithm>
#include <climits>
#include <cstring>

#include "cooc_ctx.h"
#include "cooc_radix.h"
#include "cooc_scan.h"

namespace cooc {

namespace {

constexpr int kSmpThreads = 256;
// the call's device scalars: [0] rejected, [1] fills, [2] replacements, [3] feedbacks, [4] users with a
// reservoir, [5] sum of the item counters, [6] reservoir items, [7] the first record with an id out of range
constexpr int kSmpCtr = 8;

// State carried from window to window (device pointers).
struct SampleState {
  int32_t *count;       // [n_items] itemInteractions
  int32_t *len;         // [n_users] |H_u|
  int32_t *total;       // [n_users] userInteractionsTotal
  const int64_t *aoff;  // [n_users] where the user's reservoir starts in the arena
  int32_t *arena;       // the reservoirs, slot order
  uint32_t *stamp;      // per arena entry: 1 + the call-wide index of its last writer, 0 = never written
  int64_t *ctr;         // [kSmpCtr]
  const int32_t *ukey;  // [n_users] the draw's key of every user (cooc_sample_owned), NULL: the user's index
};

// The window's feedback list (cooc_sample_owned at world > 1): hdr[0] entries, hdr[1] error bits (1: a run outside
// the histogram list, 2: an entry outside the feedback list), one 8-byte word per entry as ItemCutExchange takes it.
struct SampleFeedback {
  int32_t *hdr;
  uint64_t *list;  // NULL: no list is kept
  int64_t cap;
};

// Scratch of one window of at most m_cap records.
struct SampleScratch {
  int64_t m_cap = 0;
  int32_t *iota = nullptr;   // [m_cap] 0, 1, ..
  uint32_t *key = nullptr;   // [m_cap] the sorted ids
  int32_t *val = nullptr;    // [m_cap] their records (index in the window)
  int32_t *run = nullptr;    // [m_cap] 1 + the number of the position's run
  int32_t *head = nullptr;   // [m_cap + 1] first position of every run, then m
  int32_t *ps = nullptr;     // [m_cap + 1] user order: sampled records before the position
  int32_t *dec = nullptr;    // [m_cap] user order: the arena entry the record writes, -1 = none
  uint8_t *samp = nullptr;   // [m_cap] arrival order: passed the item cut
  void *sort_tmp = nullptr;  // radix_sort_tmp_bytes<uint32_t, int32_t>(m_cap)
  unsigned long long *scan = nullptr;  // scan_state_words(m_cap + 1) words, then the scans' error word
};

inline size_t smp_al(size_t x) { return (x + 255) & ~size_t(255); }

inline int smp_bits(int64_t n) {  // bits of the ids [0, n)
  int b = 0;
  while ((int64_t(1) << b) < n) b++;
  return b;
}

// *c += the wave's lanes with f set (every lane of the wave calls it)
__device__ inline void smp_tally(bool f, int64_t *c) {
  const uint64_t m = __ballot(f);
  if (m != 0ull && (threadIdx.x & 63) == 0)
    atomicAdd(reinterpret_cast<unsigned long long *>(c), (unsigned long long)__popcll(m));
}

struct ScanSampled {  // the sample flags in sorted order, 0 at the closing element m
  const uint8_t *samp;
  const int32_t *val;
  int64_t m;
  __device__ int64_t operator()(int64_t i) const { return i < m ? int64_t(samp[val[i]]) : 0; }
};
struct ScanCapped {  // min(v[i], cap), 0 at the closing element n
  const int32_t *v;
  int32_t cap;
  int64_t n;
  __device__ int64_t operator()(int64_t i) const { return i < n ? int64_t(v[i] < cap ? v[i] : cap) : 0; }
};

__global__ void k_smp_iota(int32_t *__restrict__ out, int64_t n) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = int32_t(i);
}

// The first record whose user or item id is out of range (ctr[7], an unsigned min; all bits set: none).
__global__ void k_smp_check(const int32_t *__restrict__ users, const int32_t *__restrict__ items, int64_t n,
                            int32_t n_users, int32_t n_items, int64_t *__restrict__ ctr) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (uint32_t(users[i]) >= uint32_t(n_users) || uint32_t(items[i]) >= uint32_t(n_items))
    atomicMin(reinterpret_cast<unsigned long long *>(&ctr[7]), (unsigned long long)i);
}

__global__ void k_smp_user_records(const int32_t *__restrict__ users, int64_t n, int32_t *__restrict__ ucnt) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&ucnt[users[i]], 1);
}

// head[r] = the first position of run r, head[number of runs] = m (run: the inclusive prefix of the run heads)
__global__ void k_smp_runs(const uint32_t *__restrict__ key, const int32_t *__restrict__ run, int64_t m,
                           int32_t *__restrict__ head) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t r = run[p] - 1;
  if (p == 0 || key[p] != key[p - 1]) head[r] = int32_t(p);
  if (p == m - 1) head[r + 1] = int32_t(m);
}

// Item order.  1. the item cut: the first item_cut - count[i] records of item i in the window are sampled.
// kBase (world > 1): the window is the ranks' records in rank order, so base[r] records of run r's item on lower
// ranks stand before this rank's (ItemCutExchange::resolve; below 2^30, as rho).
template <bool kBase>
__global__ void k_smp_item_cut(const uint32_t *__restrict__ key, const int32_t *__restrict__ val,
                               const int32_t *__restrict__ run, const int32_t *__restrict__ head, int64_t m,
                               const int32_t *__restrict__ count, int32_t item_cut, uint8_t *__restrict__ samp,
                               int64_t *__restrict__ ctr, const int32_t *__restrict__ base) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool rejected = false;
  if (p < m) {
    const int32_t r = run[p] - 1;
    const int32_t rho = int32_t(p) - head[r] + (kBase ? base[r] : 0);
    const bool s = rho < item_cut - count[key[p]];
    samp[val[p]] = s ? 1 : 0;
    rejected = !s;
  }
  smp_tally(rejected, &ctr[0]);
}

// Item order, after every read of the window's cut: count[i] += the item's sampled records.
__global__ void k_smp_item_commit(const uint32_t *__restrict__ key, const int32_t *__restrict__ run,
                                  const int32_t *__restrict__ head, int64_t m, int32_t *__restrict__ count,
                                  int32_t item_cut) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t r = run[p] - 1;
  if (head[r] != int32_t(p)) return;
  const int32_t i = int32_t(key[p]), records = head[r + 1] - int32_t(p), room = item_cut - count[i];
  if (room > 0) count[i] += records < room ? records : room;
}

// User order.  2. the user stage: fill, replace or feed back; a writer raises its slot's stamp.
// kOwned (cooc_sample_owned): the draw is keyed by st.ukey[u] where the array is given, and with a feedback list
// every feedback's item is also appended to it, for the other ranks to subtract (any order: one add per wave
// reserves the wave's entries, a lane's place is its rank in the ballot; k_sst_decide's scheme).
template <bool kOwned>
__global__ void k_smp_decide(const uint32_t *__restrict__ key, const int32_t *__restrict__ val,
                             const int32_t *__restrict__ run, const int32_t *__restrict__ head,
                             const int32_t *__restrict__ ps, int64_t m, const int32_t *__restrict__ items,
                             const uint8_t *__restrict__ samp, SampleState st, uint32_t g0, int32_t user_cut,
                             uint64_t seed, int32_t *__restrict__ dec, SampleFeedback fb) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool fill = false, replace = false, feedback = false;
  int32_t fb_item = 0;
  if (p < m) {
    const int32_t u = int32_t(key[p]), rec = val[p];
    int64_t entry = -1;
    if (samp[rec]) {
      const int32_t start = head[run[p] - 1];
      const int32_t j = int32_t(p) - start, s = ps[p] - ps[start];
      const int64_t slot_fill = int64_t(st.len[u]) + s;
      if (slot_fill < user_cut) {
        fill = true;
        entry = st.aoff[u] + slot_fill;
      } else {
        const int32_t draw_key = kOwned && st.ukey ? st.ukey[u] : u;
        const int64_t k = sample_draw(seed, draw_key, st.total[u] + j + 1);
        if (k < user_cut) {
          replace = true;
          entry = st.aoff[u] + k;
        } else {
          feedback = true;
          fb_item = items[rec];
          atomicSub(&st.count[fb_item], 1);  // 3. the feedback (after k_smp_item_commit: never below 0)
        }
      }
      if (entry >= 0) atomicMax(&st.stamp[entry], g0 + uint32_t(rec) + 1u);
    }
    dec[p] = int32_t(entry);
  }
  if (kOwned && fb.list) {
    const uint64_t mask = __ballot(feedback);
    if (mask != 0ull) {
      const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)mask) - 1;
      int32_t at = 0;
      if (lane == leader) at = atomicAdd(&fb.hdr[0], __popcll(mask));
      at = __shfl(at, leader, 64);
      if (feedback) {
        const int64_t pos = int64_t(at) + __popcll(mask & ((1ull << lane) - 1ull));
        if (pos >= 0 && pos < fb.cap) fb.list[pos] = uint64_t(uint32_t(fb_item));
        else atomicOr(&fb.hdr[1], 2);
      }
    }
  }
  smp_tally(fill, &st.ctr[1]);
  smp_tally(replace, &st.ctr[2]);
  smp_tally(feedback, &st.ctr[3]);
}

// User order.  The slot's last writer stores its item; the run's first position commits L[u] and T[u].
__global__ void k_smp_apply(const uint32_t *__restrict__ key, const int32_t *__restrict__ val,
                            const int32_t *__restrict__ run, const int32_t *__restrict__ head,
                            const int32_t *__restrict__ ps, const int32_t *__restrict__ dec, int64_t m,
                            const int32_t *__restrict__ items, SampleState st, uint32_t g0, int32_t user_cut) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t rec = val[p], entry = dec[p];
  if (entry >= 0 && st.stamp[entry] == g0 + uint32_t(rec) + 1u) st.arena[entry] = items[rec];
  const int32_t r = run[p] - 1;
  if (head[r] != int32_t(p)) return;
  const int32_t u = int32_t(key[p]), end = head[r + 1];
  const int32_t sampled = ps[end] - ps[p], room = user_cut - st.len[u];
  if (room > 0) st.len[u] += sampled < room ? sampled : room;
  st.total[u] += end - int32_t(p);
}

__global__ void k_smp_users_out(const int32_t *__restrict__ len, const int32_t *__restrict__ total, int32_t n_users,
                                int32_t *__restrict__ d_total, int64_t *__restrict__ ctr) {
  const int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool has = false;
  if (u < n_users) {
    has = len[u] > 0;
    if (d_total) d_total[u] = total[u];
  }
  smp_tally(has, &ctr[4]);
}

__global__ void k_smp_items_out(const int32_t *__restrict__ count, int32_t n_items, int16_t *__restrict__ d_count,
                                int64_t *__restrict__ ctr) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t c = 0;
  if (i < n_items) {
    c = count[i];
    if (d_count) d_count[i] = int16_t(c);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c != 0)
    atomicAdd(reinterpret_cast<unsigned long long *>(&ctr[5]), (unsigned long long)c);
}

// One wave per user: its reservoir from the arena into the CSR.  Nothing is written when the CSR's capacity is
// below the reservoirs' size (res_ptr[n_users], also left in ctr[6]).
__global__ void k_smp_gather(const int32_t *__restrict__ len, const int64_t *__restrict__ aoff,
                             const int32_t *__restrict__ arena, const int64_t *__restrict__ res_ptr, int32_t n_users,
                             int64_t res_cap, int32_t *__restrict__ res_items, int64_t *__restrict__ ctr) {
  const int64_t need = res_ptr[n_users];
  const int64_t u = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (u == 0 && lane == 0) ctr[6] = need;
  if (u >= n_users || need > res_cap) return;
  const int32_t n = len[u];
  const int32_t *src = arena + aoff[u];
  int32_t *dst = res_items + res_ptr[u];
  for (int32_t k = lane; k < n; k += 64) dst[k] = src[k];
}

inline unsigned smp_grid(int64_t n) { return unsigned((n + kSmpThreads - 1) / kSmpThreads); }

// run[p] = 1 + the number of p's run of equal keys, head[r] = run r's first position (k_smp_runs)
Status smp_group(const SampleScratch &w, int64_t m, hipStream_t s) {
  int64_t *err = reinterpret_cast<int64_t *>(w.scan + scan_state_words(w.m_cap + 1));
  COOC_TRY(launch_scan<true>(ScanKeyHead<uint32_t>{w.key}, w.run, m, w.scan, err, s));
  k_smp_runs<<<smp_grid(m), kSmpThreads, 0, s>>>(w.key, w.run, m, w.head);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// the window's records grouped by item (stable: arrival order within a run): the per-item histogram as run heads
Status sample_item_order(const SampleScratch &w, const int32_t *items, int64_t m, int item_bits, hipStream_t s) {
  COOC_TRY((radix_sort_pairs<uint32_t, int32_t>(reinterpret_cast<const uint32_t *>(items), w.iota, w.key, w.val, m,
                                                0, item_bits, false, w.sort_tmp, s)));
  return smp_group(w, m, s);
}

// 1. by item: the cut, then the counters.  7 launches and memsets plus 4 per radix pass.
Status sample_item_stage(int32_t *count, int64_t *ctr, const SampleScratch &w, const int32_t *items, int64_t m,
                         int item_bits, int32_t item_cut, hipStream_t s) {
  const unsigned grid = smp_grid(m);
  COOC_TRY(sample_item_order(w, items, m, item_bits, s));
  k_smp_item_cut<false><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, m, count, item_cut, w.samp, ctr,
                                                     nullptr);
  k_smp_item_commit<<<grid, kSmpThreads, 0, s>>>(w.key, w.run, w.head, m, count, item_cut);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// 2. by user: the records grouped by their user key (stable: arrival order within a run), the sampled ones before
// every position (ps).  5 launches and memsets plus 4 per radix pass.
Status sample_user_order(const SampleScratch &w, const int32_t *users, int64_t m, int user_bits, hipStream_t s) {
  int64_t *err = reinterpret_cast<int64_t *>(w.scan + scan_state_words(w.m_cap + 1));
  COOC_TRY((radix_sort_pairs<uint32_t, int32_t>(reinterpret_cast<const uint32_t *>(users), w.iota, w.key, w.val, m,
                                                0, user_bits, false, w.sort_tmp, s)));
  COOC_TRY(smp_group(w, m, s));
  return launch_scan<false>(ScanSampled{w.samp, w.val, m}, w.ps, m + 1, w.scan, err, s);
}

// One window: m records (users, items) in arrival order, the first of them record g0 of the call, applied to the
// carried state.  14 launches and memsets plus 4 per radix pass, whatever the data.
Status sample_window(const SampleState &st, const SampleScratch &w, const int32_t *users, const int32_t *items,
                     int64_t m, int64_t g0, int item_bits, int user_bits, int32_t item_cut, int32_t user_cut,
                     uint64_t seed, hipStream_t s) {
  if (m <= 0) return Status::Ok();
  if (m > w.m_cap) return Status{COOC_ERR_STATE, "sample_window: a window above the scratch"};
  const unsigned grid = smp_grid(m);
  COOC_TRY(sample_item_stage(st.count, st.ctr, w, items, m, item_bits, item_cut, s));
  COOC_TRY(sample_user_order(w, users, m, user_bits, s));
  // the decisions, then the slots
  const SampleFeedback none{nullptr, nullptr, 0};
  if (st.ukey)
    k_smp_decide<true><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, m, items, w.samp, st,
                                                    uint32_t(g0), user_cut, seed, w.dec, none);
  else
    k_smp_decide<false><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, m, items, w.samp, st,
                                                     uint32_t(g0), user_cut, seed, w.dec, none);
  k_smp_apply<<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, w.dec, m, items, st, uint32_t(g0),
                                           user_cut);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// One window's scratch: smp_scratch_bytes(m_cap) bytes at p.  smp_scratch_carve sets the pointers and returns the
// first byte behind them; smp_scratch_init also clears the scans' error word and fills iota.
inline size_t smp_scratch_bytes(int64_t m_cap) {
  const size_t mi = smp_al(sizeof(int32_t) * size_t(m_cap)), mi1 = smp_al(sizeof(int32_t) * size_t(m_cap + 1));
  return 5 * mi + 2 * mi1 + smp_al(size_t(m_cap)) + smp_al(radix_sort_tmp_bytes<uint32_t, int32_t>(m_cap)) +
         smp_al(sizeof(unsigned long long) * size_t(scan_state_words(m_cap + 1) + 1));
}
inline char *smp_scratch_carve(SampleScratch &w, int64_t m_cap, char *p) {
  const size_t mi = smp_al(sizeof(int32_t) * size_t(m_cap)), mi1 = smp_al(sizeof(int32_t) * size_t(m_cap + 1));
  auto take = [&](size_t bytes) {
    char *q = p;
    p += bytes;
    return q;
  };
  w.m_cap = m_cap;
  w.iota = reinterpret_cast<int32_t *>(take(mi));
  w.key = reinterpret_cast<uint32_t *>(take(mi));
  w.val = reinterpret_cast<int32_t *>(take(mi));
  w.run = reinterpret_cast<int32_t *>(take(mi));
  w.dec = reinterpret_cast<int32_t *>(take(mi));
  w.head = reinterpret_cast<int32_t *>(take(mi1));
  w.ps = reinterpret_cast<int32_t *>(take(mi1));
  w.samp = reinterpret_cast<uint8_t *>(take(smp_al(size_t(m_cap))));
  w.sort_tmp = take(smp_al(radix_sort_tmp_bytes<uint32_t, int32_t>(m_cap)));
  w.scan = reinterpret_cast<unsigned long long *>(take(
      smp_al(sizeof(unsigned long long) * size_t(scan_state_words(m_cap + 1) + 1))));
  return p;
}
Status smp_scratch_init(SampleScratch &w, int64_t m_cap, char *p, hipStream_t s) {
  smp_scratch_carve(w, m_cap, p);
  COOC_HIP_TRY(hipMemsetAsync(w.scan + scan_state_words(m_cap + 1), 0, sizeof(int64_t), s));
  k_smp_iota<<<smp_grid(m_cap), kSmpThreads, 0, s>>>(w.iota, m_cap);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// ---- the streaming form (cooc_sampling_enable_device): the same item stage and user order over (slot, user id,
// item) records; the user stage emits its decisions instead of writing an arena, and three kernels turn them
// into what k_sm_lists reads (cooc_sampled.hip): the appended items and the (slot, item) replacements of every
// changed user, contiguous and in arrival order, and one SmChange per changed user.
//
//   k_sst_decide    user order: dec[p] = kSstFill, the replaced slot, or kSstNone; feedback decrements count[i].
//                   The draw is keyed by the record's user id, the state (L, T) by its slot.
//   scan            fr[p] = (fills << 32 | replacements) before position p, one 64-bit prefix sum
//   scan            dpre[p] = runs with a fill or a replacement that start before p
//   k_sst_scatter   app[fills before p] = item, rep[2 (replacements before p)] = (slot, item); a run's first
//                   position writes the user's SmChange at dpre[p] and commits L[slot] and T[slot]
//   k_sst_distinct  one wave per SmChange with replacements: the replaced slots below len_old marked in an LDS
//                   bitmap (one bit per reservoir slot, as k_sm_lists), their number into n_old_distinct
//
// Every index is checked against its capacity; a violation sets a bit of the header's err (nothing is written out
// of range) and the window fails.
constexpr int32_t kSstNone = -1, kSstFill = -2;
constexpr int kSstMarkWords = 1024;  // user_cut <= 32,767: one bit per reservoir slot, 4 KB

struct SstHeader {  // in front of the SmChange records, copied to the host with them
  int32_t n_changed;
  int32_t err;  // bit 0: a slot outside the per-slot state, 1: a list position, 2: a descriptor, 3: a replaced slot
  int32_t n_feedback;  // world > 1: the entries of the window's feedback list
  int32_t pad[5];
};
static_assert(sizeof(SstHeader) == sizeof(SmChange) && sizeof(SmChange) == 32, "header and records share a layout");

struct SstState {
  int32_t *count;  // [n_items]
  int32_t *len;    // [slot_cap] |H_u| by slot
  int32_t *total;  // [slot_cap] userInteractionsTotal by slot
  int64_t *ctr;    // [kSmpCtr]
  int64_t slot_cap;
};

struct ScanDecisions {  // (1 << 32) per fill, 1 per replacement, 0 at the closing element m
  const int32_t *dec;
  int64_t m;
  __device__ int64_t operator()(int64_t i) const {
    if (i >= m) return 0;
    const int32_t d = dec[i];
    return d == kSstFill ? (int64_t(1) << 32) : d >= 0 ? 1 : 0;
  }
};
struct ScanChangedHead {  // 1 at the first position of every run with a fill or a replacement
  const uint32_t *key;
  const int32_t *run, *head;
  const int64_t *fr;
  int64_t m;
  __device__ int64_t operator()(int64_t i) const {
    if (i >= m || !(i == 0 || key[i] != key[i - 1])) return 0;
    return fr[head[run[i]]] != fr[i] ? 1 : 0;
  }
};

__global__ void k_sst_decide(const uint32_t *__restrict__ key, const int32_t *__restrict__ val,
                             const int32_t *__restrict__ run, const int32_t *__restrict__ head,
                             const int32_t *__restrict__ ps, int64_t m, const int32_t *__restrict__ rec_users,
                             const int32_t *__restrict__ rec_items, const uint8_t *__restrict__ samp, SstState st,
                             int32_t user_cut, uint64_t seed, int32_t *__restrict__ dec,
                             SstHeader *__restrict__ hdr, uint64_t *__restrict__ fb, int64_t fb_cap) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool fill = false, replace = false, feedback = false;
  int32_t fb_item = 0;
  if (p < m) {
    const int64_t slot = int64_t(key[p]);
    const int32_t rec = val[p];
    int32_t d = kSstNone;
    if (slot >= st.slot_cap) {
      atomicOr(&hdr->err, 1);
    } else if (samp[rec]) {
      const int32_t start = head[run[p] - 1];
      const int32_t j = int32_t(p) - start, s = ps[p] - ps[start];
      if (int64_t(st.len[slot]) + s < user_cut) {
        fill = true;
        d = kSstFill;
      } else {
        const int64_t k = sample_draw(seed, rec_users[rec], st.total[slot] + j + 1);
        if (k < user_cut) {
          replace = true;
          d = int32_t(k);
        } else {
          feedback = true;
          fb_item = rec_items[rec];
          atomicSub(&st.count[fb_item], 1);  // 3. the feedback (after the window's commit: never below 0)
        }
      }
    }
    dec[p] = d;
  }
  if (fb) {  // world > 1: the item also goes to the window's feedback list, which the other ranks subtract (any
             // order: one add per wave reserves the wave's entries, a lane's place is its rank in the ballot)
    const uint64_t mask = __ballot(feedback);
    if (mask != 0ull) {
      const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)mask) - 1;
      int32_t at = 0;
      if (lane == leader) at = atomicAdd(&hdr->n_feedback, __popcll(mask));
      at = __shfl(at, leader, 64);
      if (feedback) {
        const int64_t pos = int64_t(at) + __popcll(mask & ((1ull << lane) - 1ull));
        if (pos < fb_cap) fb[pos] = uint64_t(uint32_t(fb_item));
        else atomicOr(&hdr->err, 2);
      }
    }
  }
  smp_tally(fill, &st.ctr[1]);
  smp_tally(replace, &st.ctr[2]);
  smp_tally(feedback, &st.ctr[3]);
}

__global__ void k_sst_scatter(const uint32_t *__restrict__ key, const int32_t *__restrict__ val,
                              const int32_t *__restrict__ run, const int32_t *__restrict__ head,
                              const int32_t *__restrict__ dec, const int64_t *__restrict__ fr,
                              const int32_t *__restrict__ dpre, int64_t m, const int32_t *__restrict__ rec_items,
                              SstState st, int64_t list_cap, int32_t *__restrict__ app, int32_t *__restrict__ rep,
                              SstHeader *__restrict__ hdr, SmChange *__restrict__ chg) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= m) return;
  if (p == 0) hdr->n_changed = dpre[m];
  const int32_t d = dec[p];
  const int64_t f = fr[p], fi = f >> 32, ri = f & 0xffffffffll;
  if (d == kSstFill) {
    if (fi < list_cap) app[fi] = rec_items[val[p]];
    else atomicOr(&hdr->err, 2);
  } else if (d >= 0) {
    if (ri < list_cap) {
      rep[2 * ri] = d;
      rep[2 * ri + 1] = rec_items[val[p]];
    } else {
      atomicOr(&hdr->err, 2);
    }
  }
  if (!(p == 0 || key[p] != key[p - 1])) return;
  // the run's first position: the user's record of changes, then L and T
  const int64_t slot = int64_t(key[p]);
  if (slot >= st.slot_cap) return;  // (k_sst_decide has set the error bit)
  const int32_t end = head[run[p]];
  const int64_t fe = fr[end];
  const int32_t fills = int32_t((fe >> 32) - fi), reps = int32_t((fe & 0xffffffffll) - ri);
  const int32_t L = st.len[slot];
  if (fills + reps > 0) {
    const int64_t j = dpre[p];
    if (j < list_cap) chg[j] = SmChange{int32_t(slot), L, fills, reps, 0, int32_t(fi), int32_t(ri), 0};
    else atomicOr(&hdr->err, 4);
  }
  if (fills > 0) {
    st.len[slot] = L + fills;
    if (L == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&st.ctr[4]), 1ull);
  }
  st.total[slot] += end - int32_t(p);
}

__global__ __launch_bounds__(64) void k_sst_distinct(SstHeader *__restrict__ hdr, SmChange *__restrict__ chg,
                                                     const int32_t *__restrict__ rep, int64_t list_cap) {
  __shared__ uint32_t mark[kSstMarkWords];
  const int lane = threadIdx.x;
  const int64_t n = hdr->n_changed < list_cap ? hdr->n_changed : list_cap;
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
    const SmChange c = chg[j];
    if (c.n_rep <= 0) continue;  // (uniform over the workgroup)
    if (c.len_old < 0 || c.len_old > kSstMarkWords * 32 || c.rep_begin < 0 ||
        int64_t(c.rep_begin) + c.n_rep > list_cap) {
      if (lane == 0) atomicOr(&hdr->err, 8);
      continue;
    }
    const int32_t words = (c.len_old + 31) >> 5;
    for (int32_t w = lane; w < words; w += 64) mark[w] = 0u;
    __syncthreads();
    for (int32_t r = lane; r < c.n_rep; r += 64) {
      const int32_t k = rep[2 * (int64_t(c.rep_begin) + r)];
      if (k >= 0 && k < c.len_old) atomicOr(&mark[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    int32_t cnt = 0;
    for (int32_t w = lane; w < words; w += 64) cnt += __popc(mark[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) chg[j].n_old_distinct = cnt;
    __syncthreads();  // (the marks are reused by the next user)
  }
}

// the window scratch of the streaming form behind SampleScratch's: fr, dpre, app, rep
struct SstScratch {
  SampleScratch w;
  int64_t *fr = nullptr;    // [m_cap + 1]
  int32_t *dpre = nullptr;  // [m_cap + 1]
  int32_t *app = nullptr;   // [m_cap]
  int32_t *rep = nullptr;   // [2 m_cap]
};
inline size_t sst_scratch_bytes(int64_t m_cap) {
  return smp_scratch_bytes(m_cap) + smp_al(sizeof(int64_t) * size_t(m_cap + 1)) +
         smp_al(sizeof(int32_t) * size_t(m_cap + 1)) + 3 * smp_al(sizeof(int32_t) * size_t(m_cap));
}
inline SstScratch sst_carve(int64_t m_cap, char *p) {  // (the pointers alone: smp_scratch_init has run at growth)
  SstScratch x;
  char *q = smp_scratch_carve(x.w, m_cap, p);
  x.fr = reinterpret_cast<int64_t *>(q);
  q += smp_al(sizeof(int64_t) * size_t(m_cap + 1));
  x.dpre = reinterpret_cast<int32_t *>(q);
  q += smp_al(sizeof(int32_t) * size_t(m_cap + 1));
  x.app = reinterpret_cast<int32_t *>(q);
  q += smp_al(sizeof(int32_t) * size_t(m_cap));
  x.rep = reinterpret_cast<int32_t *>(q);
  return x;
}

// ---- the item cut across ranks (ItemCutExchange): W lists of at most lmax words, rank q's at all + q * lmax, its
// length lens[q].  A histogram list holds (item << 32 | records) words sorted by item, every item once.
constexpr int32_t kIcxClamp = 1 << 30;  // sums of records are clamped here: above every item cut, rho + base fits

// the run heads of the by-item order as the rank's histogram list (run r's word at list[r])
__global__ void k_icx_pack(const uint32_t *__restrict__ key, const int32_t *__restrict__ run,
                           const int32_t *__restrict__ head, int64_t m, int64_t n_runs, uint64_t *__restrict__ list,
                           int32_t *__restrict__ err) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t r = run[p] - 1;
  if (head[r] != int32_t(p)) return;
  if (r < 0 || r >= n_runs) {
    atomicOr(err, 1);
    return;
  }
  list[r] = (uint64_t(key[p]) << 32) | uint64_t(uint32_t(head[r + 1] - int32_t(p)));
}

// the records of `item` in a sorted histogram list of n words (0: not listed)
__device__ inline int64_t icx_find(const uint64_t *__restrict__ list, int64_t n, uint32_t item) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (uint32_t(list[mid] >> 32) < item) lo = mid + 1; else hi = mid;
  }
  return lo < n && uint32_t(list[lo] >> 32) == item ? int64_t(uint32_t(list[lo])) : 0;
}

// One thread per slot (q, j) of the gathered histograms: the records of its item on the lower ranks (this rank's
// slots: the run's base) and, where no lower rank lists the item, the job's records of it (tot; -1 elsewhere, so
// every item of the union has one owner and the commit needs no atomics).
__global__ void k_icx_resolve(const uint64_t *__restrict__ all, const int64_t *__restrict__ lens, int32_t W,
                              int64_t lmax, int32_t rank, int32_t *__restrict__ base, int32_t *__restrict__ tot) {
  const int64_t slot = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (slot >= int64_t(W) * lmax) return;
  const int32_t q = int32_t(slot / lmax);
  const int64_t j = slot - int64_t(q) * lmax;
  if (j >= lens[q]) {
    tot[slot] = -1;
    return;
  }
  const uint64_t word = all[slot];
  const uint32_t item = uint32_t(word >> 32);
  int64_t lower = 0, sum = int64_t(uint32_t(word));
  for (int32_t o = 0; o < W; o++) {
    if (o == q) continue;
    const int64_t h = icx_find(all + int64_t(o) * lmax, lens[o] < lmax ? lens[o] : lmax, item);
    if (o < q) lower += h;
    sum += h;
  }
  if (q == rank) base[j] = int32_t(lower < kIcxClamp ? lower : kIcxClamp);
  tot[slot] = lower > 0 ? -1 : int32_t(sum < kIcxClamp ? sum : kIcxClamp);
}

// after every read of the window's cut: count[i] += the job's sampled records of i, by the item's one owner slot
__global__ void k_icx_commit(const uint64_t *__restrict__ all, const int32_t *__restrict__ tot, int64_t n_slots,
                             int32_t *__restrict__ count, int32_t n_items, int32_t item_cut,
                             int32_t *__restrict__ err) {
  const int64_t slot = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (slot >= n_slots) return;
  const int32_t t = tot[slot];
  if (t < 0) return;
  const uint32_t i = uint32_t(all[slot] >> 32);
  if (i >= uint32_t(n_items)) {
    atomicOr(err, 2);
    return;
  }
  const int32_t room = item_cut - count[i];
  if (room > 0) count[i] += t < room ? t : room;
}

// the gathered feedback lists: count[i] -= 1 per entry of every other rank (this rank's own were subtracted where
// they arose)
__global__ void k_icx_feedback(const uint64_t *__restrict__ all, const int64_t *__restrict__ lens, int32_t W,
                               int64_t lmax, int32_t rank, int32_t *__restrict__ count, int32_t n_items,
                               int32_t *__restrict__ err) {
  const int64_t slot = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (slot >= int64_t(W) * lmax) return;
  const int32_t q = int32_t(slot / lmax);
  if (q == rank || slot - int64_t(q) * lmax >= lens[q]) return;
  const uint64_t i = all[slot];
  if (i >= uint64_t(n_items)) {
    atomicOr(err, 2);
    return;
  }
  atomicSub(&count[i], 1);
}

// after resolve(): an item whose records over the ranks reached the clamp sets bit 4 of *err (tot is computed from
// the gathered lists alone, so every rank finds the same)
__global__ void k_icx_fits(const int32_t *__restrict__ tot, int64_t n_slots, int32_t *__restrict__ err) {
  const int64_t slot = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (slot < n_slots && tot[slot] >= kIcxClamp) atomicOr(err, 4);
}

// One window of cooc_sample_owned at world > 1: sample_window over the ranks' records in rank order.  A collective:
// every rank runs it for every window, also with m == 0 (the peers' sampled records and feedbacks still move the
// replicated counters).  Per window 2 to 4 all-gathers (ItemCutExchange::gather, twice: the lengths, then the
// lists unless every rank's is empty) and, beside sample_window's launches, k_icx_pack, k_icx_resolve, k_icx_fits,
// k_icx_commit in place of k_smp_item_commit and k_icx_feedback; two small reads of its own synchronise the stream
// (the number of runs, the feedback header), beside the exchange's three (two gathered length vectors, the error
// word).  lists: hdr (256 bytes), then m_cap histogram words, then m_cap feedbacks.
Status sample_window_ranks(const SampleState &st, const SampleScratch &w, const int32_t *users, const int32_t *items,
                           int64_t m, int64_t g0, int item_bits, int user_bits, int32_t n_items, int32_t item_cut,
                           int32_t user_cut, uint64_t seed, Comm &comm, ItemCutExchange &icx, char *lists,
                           hipStream_t s) {
  if (m > w.m_cap) return Status{COOC_ERR_STATE, "sample_window: a window above the scratch"};
  int32_t *hdr = reinterpret_cast<int32_t *>(lists);
  uint64_t *hist = reinterpret_cast<uint64_t *>(lists + 256), *fbl = hist + w.m_cap;
  const unsigned grid = smp_grid(m);
  COOC_HIP_TRY(hipMemsetAsync(hdr, 0, 2 * sizeof(int32_t), s));
  int32_t n_runs = 0;
  if (m > 0) {
    COOC_TRY(sample_item_order(w, items, m, item_bits, s));
    COOC_HIP_TRY(hipMemcpyAsync(&n_runs, w.run + (m - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (n_runs < 1 || n_runs > m) return Status{COOC_ERR_STATE, "internal error: the window's item runs out of range"};
    k_icx_pack<<<grid, kSmpThreads, 0, s>>>(w.key, w.run, w.head, m, n_runs, hist, &hdr[1]);
    COOC_HIP_TRY(hipGetLastError());
  }
  COOC_TRY(icx.gather(comm, s, hist, n_runs));
  COOC_TRY(icx.resolve(s));
  if (icx.lmax() > 0) {
    k_icx_fits<<<smp_grid(icx.slots()), kSmpThreads, 0, s>>>(icx.tot(), icx.slots(), &hdr[1]);
    COOC_HIP_TRY(hipGetLastError());
  }
  if (m > 0) {
    k_smp_item_cut<true><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, m, st.count, item_cut, w.samp,
                                                      st.ctr, icx.base());
    COOC_HIP_TRY(hipGetLastError());
  }
  COOC_TRY(icx.commit(s, st.count, n_items, item_cut));
  if (m > 0) {
    COOC_TRY(sample_user_order(w, users, m, user_bits, s));
    k_smp_decide<true><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, m, items, w.samp, st,
                                                    uint32_t(g0), user_cut, seed, w.dec,
                                                    SampleFeedback{hdr, fbl, m});
    k_smp_apply<<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, w.dec, m, items, st, uint32_t(g0),
                                             user_cut);
    COOC_HIP_TRY(hipGetLastError());
  }
  int32_t h[2] = {0, 0};
  COOC_HIP_TRY(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  Status local = Status::Ok();
  if (h[1] & 3) local = Status{COOC_ERR_STATE, "internal bounds check failed (owned sampler, " + std::to_string(h[1]) + ")"};
  else if (h[0] < 0 || h[0] > m) local = Status{COOC_ERR_STATE, "internal error: more feedbacks than the window has records"};
  // (the collective is made also by a rank whose window failed: its peers wait in it)
  COOC_TRY(icx.gather(comm, s, fbl, local.ok() ? h[0] : 0));
  COOC_TRY(icx.subtract_peers(s, st.count, n_items));
  COOC_TRY(local);
  if (h[1] & 4)  // (found from the gathered lists: the same verdict on every rank)
    return Status{COOC_ERR_ARG, "the job's records of one item in one window reach 2^30"};
  return Status::Ok();
}

// cooc_sample_owned's agreement, before any output is written or any other collective starts: the ranks all-gather
// (local status, n_windows, item_cut, user_cut, seed).  A rank whose own checks failed returns their status; if
// another rank failed, or the four values differ, every rank returns COOC_ERR_ARG and names the rank.
Status sample_agree(Comm &comm, DevBuf &buf, const Status &local, int32_t n_windows, int32_t item_cut,
                    int32_t user_cut, int64_t seed, hipStream_t s) {
  constexpr int kF = 5;
  const int32_t W = comm.world();
  const int64_t mine[kF] = {local.code, n_windows, item_cut, user_cut, seed};
  std::vector<int64_t> all(size_t(W) * kF, 0);
  auto exchange = [&]() -> Status {
    COOC_TRY(buf.reserve(sizeof(int64_t) * kF * size_t(W + 1)));
    int64_t *d = buf.as<int64_t>();
    COOC_HIP_TRY(hipMemcpyAsync(d + size_t(W) * kF, mine, sizeof(mine), hipMemcpyHostToDevice, s));
    COOC_TRY(comm.allgather(d + size_t(W) * kF, d, sizeof(mine), s));
    COOC_HIP_TRY(hipMemcpyAsync(all.data(), d, sizeof(mine) * size_t(W), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    return Status::Ok();
  };
  const Status x = exchange();
  if (!local.ok()) return local;
  COOC_TRY(x);
  for (int32_t q = 0; q < W; q++)
    if (all[size_t(q) * kF] != 0)
      return Status{COOC_ERR_ARG, "cooc_sample_owned: rank " + std::to_string(q) + " failed its checks (status " +
                                      std::to_string(all[size_t(q) * kF]) + "); no rank sampled"};
  for (int32_t q = 0; q < W; q++) {
    const int64_t *v = &all[size_t(q) * kF];
    if (std::memcmp(v + 1, &all[1], sizeof(int64_t) * (kF - 1)) == 0) continue;
    auto four = [](const int64_t *a) {
      return "n_windows " + std::to_string(a[1]) + ", item_cut " + std::to_string(a[2]) + ", user_cut " +
             std::to_string(a[3]) + ", seed " + std::to_string(a[4]);
    };
    return Status{COOC_ERR_ARG, "cooc_sample_owned: rank " + std::to_string(q) + " passed " + four(v) +
                                    ", rank 0 " + four(&all[0]) + "; no rank sampled"};
  }
  return Status::Ok();
}

// The first user whose draw key is negative (ctr[7], as k_smp_check).
__global__ void k_smp_check_keys(const int32_t *__restrict__ ukey, int32_t n_users, int64_t *__restrict__ ctr) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < n_users && ukey[j] < 0) atomicMin(reinterpret_cast<unsigned long long *>(&ctr[7]), (unsigned long long)j);
}

}  // namespace

int64_t ItemCutExchange::words() const {
  int64_t n = 0;
  for (int64_t v : lens_) n += v;
  return n;
}

Status ItemCutExchange::gather(Comm &c, hipStream_t s, const uint64_t *d_src, int64_t n) {
  const int32_t W = c.world();
  rank_ = c.rank();
  n_local_ = n;
  lens_.assign(size_t(W), 0);
  lmax_ = 0;
  COOC_TRY(dlens_.reserve(sizeof(int64_t) * size_t(W + 1)));
  COOC_TRY(err_.reserve(sizeof(int32_t)));
  int64_t *dl = dlens_.as<int64_t>();
  COOC_HIP_TRY(hipMemcpyAsync(dl + W, &n, sizeof(int64_t), hipMemcpyHostToDevice, s));
  COOC_TRY(c.allgather(dl + W, dl, sizeof(int64_t), s));
  COOC_HIP_TRY(hipMemcpyAsync(lens_.data(), dl, sizeof(int64_t) * size_t(W), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (lens_[size_t(rank_)] != n) return Status{COOC_ERR_STATE, "item-cut exchange: the gathered lengths disagree with this rank's"};
  for (int64_t v : lens_) {
    if (v < 0 || v >= (int64_t(1) << 29)) return Status{COOC_ERR_STATE, "item-cut exchange: a list length out of range"};
    lmax_ = std::max(lmax_, v);
  }
  if (lmax_ == 0) return Status::Ok();  // (every rank sees the same lengths: none of them gathers)
  COOC_TRY(send_.reserve(sizeof(uint64_t) * size_t(lmax_)));
  COOC_TRY(all_.reserve(sizeof(uint64_t) * size_t(lmax_) * size_t(W)));
  if (n < lmax_) COOC_HIP_TRY(hipMemsetAsync(send_.as<uint64_t>() + n, 0, sizeof(uint64_t) * size_t(lmax_ - n), s));
  if (n > 0) COOC_HIP_TRY(hipMemcpyAsync(send_.p, d_src, sizeof(uint64_t) * size_t(n), hipMemcpyDeviceToDevice, s));
  return c.allgather(send_.p, all_.p, int64_t(sizeof(uint64_t)) * lmax_, s);
}

Status ItemCutExchange::gather_host(Comm &c, hipStream_t s, const uint64_t *h_src, int64_t n) {
  COOC_TRY(base_.reserve(sizeof(uint64_t) * size_t(std::max<int64_t>(n, 1))));  // (staging: resolve() rewrites it)
  if (n > 0) COOC_HIP_TRY(hipMemcpyAsync(base_.p, h_src, sizeof(uint64_t) * size_t(n), hipMemcpyHostToDevice, s));
  return gather(c, s, base_.as<uint64_t>(), n);
}

Status ItemCutExchange::resolve(hipStream_t s) {
  if (lmax_ == 0) return Status::Ok();
  const int32_t W = int32_t(lens_.size());
  COOC_TRY(base_.reserve(sizeof(int32_t) * size_t(lmax_)));
  COOC_TRY(tot_.reserve(sizeof(int32_t) * size_t(slots())));
  k_icx_resolve<<<smp_grid(slots()), kSmpThreads, 0, s>>>(all_.as<uint64_t>(), dlens_.as<int64_t>(), W, lmax_, rank_,
                                                          base_.as<int32_t>(), tot_.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status ItemCutExchange::commit(hipStream_t s, int32_t *count, int32_t n_items, int32_t item_cut) {
  if (lmax_ == 0) return Status::Ok();
  if (!err_live_) COOC_HIP_TRY(hipMemsetAsync(err_.p, 0, sizeof(int32_t), s));
  err_live_ = true;
  k_icx_commit<<<smp_grid(slots()), kSmpThreads, 0, s>>>(all_.as<uint64_t>(), tot_.as<int32_t>(), slots(), count,
                                                         n_items, item_cut, err_.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status ItemCutExchange::subtract_peers(hipStream_t s, int32_t *count, int32_t n_items) {
  if (lmax_ > 0) {
    if (!err_live_) COOC_HIP_TRY(hipMemsetAsync(err_.p, 0, sizeof(int32_t), s));
    err_live_ = true;
    k_icx_feedback<<<smp_grid(slots()), kSmpThreads, 0, s>>>(all_.as<uint64_t>(), dlens_.as<int64_t>(),
                                                             int32_t(lens_.size()), lmax_, rank_, count, n_items,
                                                             err_.as<int32_t>());
    COOC_HIP_TRY(hipGetLastError());
  }
  if (!err_live_) return Status::Ok();
  err_live_ = false;
  int32_t h_err = 0;  // (the window's commit and this kernel share the word: one read per window)
  COOC_HIP_TRY(hipMemcpyAsync(&h_err, err_.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (h_err) return Status{COOC_ERR_STATE, "item-cut exchange: a peer's item outside [0, n_items)"};
  return Status::Ok();
}

Status ItemCutExchange::read_back(hipStream_t s, std::vector<uint64_t> *all, std::vector<int32_t> *base,
                                  std::vector<int32_t> *tot) {
  all->assign(size_t(slots()), 0);
  if (base) base->assign(size_t(n_local_), 0);
  if (tot) tot->assign(size_t(slots()), -1);
  if (lmax_ == 0) return Status::Ok();
  COOC_HIP_TRY(hipMemcpyAsync(all->data(), all_.p, sizeof(uint64_t) * size_t(slots()), hipMemcpyDeviceToHost, s));
  if (base && n_local_ > 0)
    COOC_HIP_TRY(hipMemcpyAsync(base->data(), base_.p, sizeof(int32_t) * size_t(n_local_), hipMemcpyDeviceToHost, s));
  if (tot) COOC_HIP_TRY(hipMemcpyAsync(tot->data(), tot_.p, sizeof(int32_t) * size_t(slots()), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  return Status::Ok();
}

Status SampleStream::enable(int32_t n_items, int32_t item_cut, int32_t user_cut, uint64_t seed, hipStream_t s) {
  COOC_TRY(count_.reserve(sizeof(int32_t) * size_t(n_items)));
  COOC_TRY(ctr_.reserve(sizeof(int64_t) * kSmpCtr));
  COOC_HIP_TRY(hipMemsetAsync(count_.p, 0, sizeof(int32_t) * size_t(n_items), s));
  COOC_HIP_TRY(hipMemsetAsync(ctr_.p, 0, sizeof(int64_t) * kSmpCtr, s));
  n_items_ = n_items;
  user_cut_ = user_cut;
  seed_ = seed;
  slot_cap_ = m_cap_ = 0;
  COOC_TRY(grow_slots(kSstSlots0, s));
  item_cut_ = item_cut;
  return Status::Ok();
}

// frees the device state; the sampler stays enabled with its cuts and seed (StreamState::release)
void SampleStream::release() {
  SampleStream fresh;
  fresh.n_items_ = n_items_;
  fresh.item_cut_ = item_cut_;
  fresh.user_cut_ = user_cut_;
  fresh.seed_ = seed_;
  *this = std::move(fresh);
}

// L and T for n_slots slots: contents preserved, the tail zeroed
Status SampleStream::grow_slots(int64_t n_slots, hipStream_t s) {
  if (n_slots <= slot_cap_) return Status::Ok();
  const int64_t cap = std::max<int64_t>(std::max<int64_t>(n_slots, 2 * slot_cap_), kSstSlots0);
  for (DevBuf *b : {&len_, &total_}) {
    DevBuf bigger;
    COOC_TRY(bigger.reserve(sizeof(int32_t) * size_t(cap)));
    hipError_t e = hipMemsetAsync(bigger.p, 0, sizeof(int32_t) * size_t(cap), s);
    if (e == hipSuccess && slot_cap_ > 0)
      e = hipMemcpyAsync(bigger.p, b->p, sizeof(int32_t) * size_t(slot_cap_), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return Status{3, std::string("SampleStream::grow_slots: ") + hipGetErrorString(e)};
    *b = std::move(bigger);
  }
  slot_cap_ = cap;
  return Status::Ok();
}

Status SampleStream::grow_window(int64_t m, hipStream_t s) {
  if (m <= m_cap_) return Status::Ok();
  const int64_t cap = std::max<int64_t>(std::max<int64_t>(m, 2 * m_cap_), 4096);
  COOC_HIP_TRY(hipStreamSynchronize(s));  // (nothing in flight reads the buffers that are replaced)
  m_cap_ = 0;
  COOC_TRY(win_.reserve(sst_scratch_bytes(cap)));
  COOC_TRY(rec_.reserve(sizeof(int32_t) * 3 * size_t(cap)));
  COOC_TRY(out_.reserve(sizeof(SmChange) * size_t(cap + 1)));
  SampleScratch w;
  COOC_TRY(smp_scratch_init(w, cap, win_.as<char>(), s));
  m_cap_ = cap;
  return Status::Ok();
}

Status SampleStream::window(hipStream_t s, int64_t n, const int32_t *rec3, int64_t n_slots, int64_t n_distinct,
                            std::vector<SmChange> *changed, Comm *comm, ItemCutExchange *icx) {
  changed->clear();
  const bool multi = comm && comm->world() > 1;
  if (n <= 0 && !multi) return Status::Ok();
  // (release() without a following enable(): a failed restore whose reset could not allocate)
  if (!count_.p || !ctr_.p) return Status{COOC_ERR_STATE, "the device sampler's state was released and not re-created"};
  // (fills << 32 must stay below the scan's 2^62, and 2 n entries of rep are indexed with an int32)
  if (n >= (int64_t(1) << 29)) return Status{COOC_ERR_ARG, "2^29 or more records in one sampled window"};
  if (multi && n <= 0) {  // no record here: the peers' sampled records and feedbacks still move every counter
    COOC_TRY(icx->gather(*comm, s, nullptr, 0));
    COOC_TRY(icx->resolve(s));
    COOC_TRY(icx->commit(s, count_.as<int32_t>(), n_items_, item_cut_));
    COOC_TRY(icx->gather(*comm, s, nullptr, 0));
    return icx->subtract_peers(s, count_.as<int32_t>(), n_items_);
  }
  COOC_TRY(grow_slots(n_slots, s));
  COOC_TRY(grow_window(n, s));
  const SstScratch x = sst_carve(m_cap_, win_.as<char>());
  const SampleScratch &w = x.w;
  app_ = x.app;
  rep_ = x.rep;
  int32_t *d_slots = rec_.as<int32_t>(), *d_users = d_slots + n, *d_items = d_users + n;
  SstHeader *hdr = out_.as<SstHeader>();
  SmChange *chg = out_.as<SmChange>() + 1;
  const SstState st{count_.as<int32_t>(), len_.as<int32_t>(), total_.as<int32_t>(), ctr_.as<int64_t>(), slot_cap_};
  int64_t *err = reinterpret_cast<int64_t *>(w.scan + scan_state_words(w.m_cap + 1));
  const unsigned grid = smp_grid(n);
  COOC_HIP_TRY(hipMemcpyAsync(d_slots, rec3, sizeof(int32_t) * 3 * size_t(n), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemsetAsync(hdr, 0, sizeof(SstHeader), s));
  uint64_t *fb = nullptr;
  if (!multi) {
    COOC_TRY(sample_item_stage(st.count, st.ctr, w, d_items, n, smp_bits(n_items_), item_cut_, s));
  } else {
    // the by-item order's runs are this rank's histogram: gathered, every run's base and every item's total found
    // in the peers' lists, the cut taken at rho + base, the counters committed over the gathered union
    COOC_TRY(sample_item_order(w, d_items, n, smp_bits(n_items_), s));
    int32_t n_runs = 0;
    COOC_HIP_TRY(hipMemcpyAsync(&n_runs, w.run + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (n_runs < 1 || n_runs > n) return Status{COOC_ERR_STATE, "internal error: the window's item runs out of range"};
    COOC_TRY(hist_.reserve(sizeof(uint64_t) * size_t(n_runs)));
    COOC_TRY(fb_.reserve(sizeof(uint64_t) * size_t(n)));
    fb = fb_.as<uint64_t>();
    k_icx_pack<<<grid, kSmpThreads, 0, s>>>(w.key, w.run, w.head, n, n_runs, hist_.as<uint64_t>(), &hdr->err);
    COOC_HIP_TRY(hipGetLastError());
    COOC_TRY(icx->gather(*comm, s, hist_.as<uint64_t>(), n_runs));
    COOC_TRY(icx->resolve(s));
    k_smp_item_cut<true><<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, n, st.count, item_cut_, w.samp,
                                                      st.ctr, icx->base());
    COOC_HIP_TRY(hipGetLastError());
    COOC_TRY(icx->commit(s, st.count, n_items_, item_cut_));
  }
  COOC_TRY(sample_user_order(w, d_slots, n, smp_bits(std::max<int64_t>(n_slots, 1)), s));
  k_sst_decide<<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.ps, n, d_users, d_items, w.samp, st,
                                            user_cut_, seed_, w.dec, hdr, fb, n);
  COOC_HIP_TRY(hipGetLastError());
  COOC_TRY(launch_scan<false>(ScanDecisions{w.dec, n}, x.fr, n + 1, w.scan, err, s));
  COOC_TRY(launch_scan<false>(ScanChangedHead{w.key, w.run, w.head, x.fr, n}, x.dpre, n + 1, w.scan, err, s));
  k_sst_scatter<<<grid, kSmpThreads, 0, s>>>(w.key, w.val, w.run, w.head, w.dec, x.fr, x.dpre, n, d_items, st, m_cap_,
                                             x.app, x.rep, hdr, chg);
  const int64_t bound = std::min<int64_t>(std::max<int64_t>(n_distinct, 1), n);
  k_sst_distinct<<<unsigned(std::min<int64_t>(bound, 1 << 16)), 64, 0, s>>>(hdr, chg, x.rep, m_cap_);
  COOC_HIP_TRY(hipGetLastError());
  // the one copy back: the header and the records of at most `bound` changed users
  changed->resize(size_t(bound) + 1);
  COOC_HIP_TRY(hipMemcpyAsync(changed->data(), hdr, sizeof(SmChange) * size_t(bound + 1), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  SstHeader h;
  std::memcpy(&h, changed->data(), sizeof(h));
  Status local = Status::Ok();
  if (h.err) local = Status{COOC_ERR_STATE, "internal bounds check failed (device sampler, " + std::to_string(h.err) + ")"};
  else if (h.n_changed < 0 || h.n_changed > bound)
    local = Status{COOC_ERR_STATE, "internal error: more changed users than the window has users"};
  else if (h.n_feedback < 0 || h.n_feedback > n)
    local = Status{COOC_ERR_STATE, "internal error: more feedbacks than the window has records"};
  if (multi) {  // (the collective is made also by a rank whose window failed: its peers wait in it)
    COOC_TRY(icx->gather(*comm, s, fb, local.ok() ? h.n_feedback : 0));
    COOC_TRY(icx->subtract_peers(s, st.count, n_items_));
  }
  COOC_TRY(local);
  changed->erase(changed->begin());
  changed->resize(size_t(h.n_changed));
  return Status::Ok();
}

Status SampleStream::counters(hipStream_t s, int64_t out[6]) {
  if (!count_.p || !ctr_.p) return Status{COOC_ERR_STATE, "the device sampler's state was released and not re-created"};
  int64_t *ctr = ctr_.as<int64_t>();
  COOC_HIP_TRY(hipMemsetAsync(&ctr[5], 0, sizeof(int64_t), s));
  k_smp_items_out<<<smp_grid(n_items_), kSmpThreads, 0, s>>>(count_.as<int32_t>(), n_items_, nullptr, ctr);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(out, ctr, sizeof(int64_t) * 6, hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  return Status::Ok();
}

Status SampleStream::total(hipStream_t s, int32_t slot, int32_t *total) {
  *total = 0;
  if (slot < 0 || slot >= slot_cap_) return Status::Ok();  // (a slot no finished window has seen)
  COOC_HIP_TRY(hipStreamSynchronize(s));
  COOC_HIP_TRY(hipMemcpy(total, total_.as<int32_t>() + slot, sizeof(int32_t), hipMemcpyDeviceToHost));
  return Status::Ok();
}

}  // namespace cooc

using cooc::Status;

Status cooc_ctx::sample_device(int64_t n, const int32_t *d_users, const int32_t *d_items, int32_t n_users,
                               int32_t n_windows, const int64_t *window_ptr, int32_t item_cut, int32_t user_cut,
                               int64_t seed, int64_t *d_res_ptr, int32_t *d_res_items, int64_t res_cap,
                               int32_t *d_total, int16_t *d_item_count, hipStream_t s, cooc_sample_info *info) {
  return sample_log(false, n, d_users, d_items, n_users, nullptr, n_windows, window_ptr, item_cut, user_cut, seed,
                    d_res_ptr, d_res_items, res_cap, d_total, d_item_count, s, info);
}

Status cooc_ctx::sample_owned(int64_t n, const int32_t *d_users, const int32_t *d_items, int32_t n_users,
                              const int32_t *d_user_key, int32_t n_windows, const int64_t *window_ptr,
                              int32_t item_cut, int32_t user_cut, int64_t seed, int64_t *d_res_ptr,
                              int32_t *d_res_items, int64_t res_cap, int32_t *d_total, int16_t *d_item_count,
                              hipStream_t s, cooc_sample_info *info) {
  return sample_log(true, n, d_users, d_items, n_users, d_user_key, n_windows, window_ptr, item_cut, user_cut, seed,
                    d_res_ptr, d_res_items, res_cap, d_total, d_item_count, s, info);
}

// Both entry points.  owned: the draw keyed by d_user_key, no user allowed where there is no record, and at world
// > 1 the windows over the ranks' records in rank order (sample_window_ranks) after the ranks agreed on the call.
Status cooc_ctx::sample_log(bool owned, int64_t n, const int32_t *d_users, const int32_t *d_items, int32_t n_users,
                            const int32_t *d_user_key, int32_t n_windows, const int64_t *window_ptr,
                            int32_t item_cut, int32_t user_cut, int64_t seed, int64_t *d_res_ptr,
                            int32_t *d_res_items, int64_t res_cap, int32_t *d_total, int16_t *d_item_count,
                            hipStream_t s, cooc_sample_info *info) {
  using namespace cooc;
  cooc_sample_info unread{};
  const bool no_info = info == nullptr;
  if (no_info) info = &unread;
  *info = cooc_sample_info{};
  const bool multi = owned && comm && comm->world() > 1;
  const int64_t one_window[2] = {0, n};
  int64_t m_max = 0;
  auto host_checks = [&]() -> Status {
    if (no_info) return Status{COOC_ERR_ARG, "cooc_sample_owned: info is NULL"};
    if (item_cut < 1 || item_cut > 32767)  // a Java short, ItemInteractionCounter...java:37
      return Status{COOC_ERR_ARG, std::to_string(item_cut) + " is not a valid itemCut"};
    if (user_cut < 1 || user_cut > 32767)  // UserInteractionCounter...java:54,76
      return Status{COOC_ERR_ARG, std::to_string(user_cut) + " is not a valid userCut"};
    if (n_users < 0 || (n_users == 0 && !(owned && n == 0)))  // (a rank of an owned job may hold no user)
      return Status{COOC_ERR_ARG, "n_users must be > 0"};
    if (n < 0 || n > int64_t(INT32_MAX))  // a user's total is a Java int
      return Status{COOC_ERR_ARG, "n_records must be in [0, 2^31 - 1]"};
    if (!d_res_ptr || res_cap < 0 || (res_cap > 0 && !d_res_items) || (n > 0 && (!d_users || !d_items)))
      return Status{COOC_ERR_ARG, std::string(owned ? "cooc_sample_owned" : "cooc_sample_device") +
                                      ": a required pointer is NULL"};
    if (!window_ptr) {
      if (n_windows != 1) return Status{COOC_ERR_ARG, "window_ptr == NULL needs n_windows == 1"};
      window_ptr = one_window;
    }
    if (n_windows < 1) return Status{COOC_ERR_ARG, "n_windows must be > 0"};
    if (window_ptr[0] != 0 || window_ptr[n_windows] != n)
      return Status{COOC_ERR_ARG, "window_ptr must start at 0 and end at n_records"};
    for (int32_t w = 0; w < n_windows; w++) {
      if (window_ptr[w + 1] < window_ptr[w]) return Status{COOC_ERR_ARG, "window_ptr must be non-decreasing"};
      m_max = std::max(m_max, window_ptr[w + 1] - window_ptr[w]);
    }
    // (one item's records on a rank stay below the exchange's clamp, so rho + base is an int32)
    if (multi && m_max >= (int64_t(1) << 30))
      return Status{COOC_ERR_ARG, "2^30 or more records in one window of a rank"};
    return Status::Ok();
  };
  Status local = host_checks();
  COOC_HIP_TRY(hipSetDevice(device));
  const int32_t M = cfg.n_items;
  const int64_t U = n_users;
  int64_t *ctr = nullptr, *aoff = nullptr, *scan_err = nullptr;
  int32_t *ucnt = nullptr;
  unsigned long long *scan = nullptr;
  SampleState st{};
  int64_t h_ctr[kSmpCtr] = {};

  // the call's state and the checks made on the device; nothing of the caller's is written
  auto prepare = [&]() -> Status {
    // the call's state: counters, L, T, the users' records, the arena offsets, the arena and its stamps
    const size_t scan_u = sizeof(unsigned long long) * size_t(scan_state_words(U + 1) + 1);
    const size_t o_ctr = 0, o_count = o_ctr + smp_al(sizeof(int64_t) * kSmpCtr);
    const size_t o_len = o_count + smp_al(sizeof(int32_t) * size_t(M)), o_total = o_len + smp_al(sizeof(int32_t) * U);
    const size_t o_ucnt = o_total + smp_al(sizeof(int32_t) * U), o_zero_end = o_ucnt + smp_al(sizeof(int32_t) * U);
    const size_t o_aoff = o_zero_end, o_scan = o_aoff + smp_al(sizeof(int64_t) * size_t(U + 1));
    const size_t o_stamp = o_scan + smp_al(scan_u), o_arena = o_stamp + smp_al(sizeof(uint32_t) * size_t(n));
    COOC_TRY(b_smp_state.reserve(o_arena + smp_al(sizeof(int32_t) * size_t(n))));
    char *base = b_smp_state.as<char>();
    ctr = reinterpret_cast<int64_t *>(base + o_ctr);
    ucnt = reinterpret_cast<int32_t *>(base + o_ucnt);
    aoff = reinterpret_cast<int64_t *>(base + o_aoff);
    scan = reinterpret_cast<unsigned long long *>(base + o_scan);
    scan_err = reinterpret_cast<int64_t *>(scan + scan_state_words(U + 1));
    st.count = reinterpret_cast<int32_t *>(base + o_count);
    st.len = reinterpret_cast<int32_t *>(base + o_len);
    st.total = reinterpret_cast<int32_t *>(base + o_total);
    st.aoff = aoff;
    st.stamp = reinterpret_cast<uint32_t *>(base + o_stamp);
    st.arena = reinterpret_cast<int32_t *>(base + o_arena);
    st.ctr = ctr;
    st.ukey = d_user_key;
    COOC_HIP_TRY(hipMemsetAsync(base, 0, o_zero_end, s));
    COOC_HIP_TRY(hipMemsetAsync(scan_err, 0, sizeof(int64_t), s));
    const int64_t none = -1;  // all bits set: above every index for the unsigned min
    if (d_user_key && U > 0) {
      COOC_HIP_TRY(hipMemsetAsync(&ctr[7], 0xff, sizeof(int64_t), s));
      k_smp_check_keys<<<smp_grid(U), kSmpThreads, 0, s>>>(d_user_key, n_users, ctr);
      COOC_HIP_TRY(hipGetLastError());
      COOC_HIP_TRY(hipMemcpyAsync(&h_ctr[7], &ctr[7], sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (h_ctr[7] != none) {
        int32_t bk = 0;
        COOC_HIP_TRY(hipMemcpy(&bk, d_user_key + h_ctr[7], sizeof(int32_t), hipMemcpyDeviceToHost));
        return Status{COOC_ERR_ARG, "user_key[" + std::to_string(h_ctr[7]) + "] = " + std::to_string(bk) +
                                        " is negative"};
      }
    }
    if (n > 0) {
      // ids out of range are found before anything is written
      COOC_HIP_TRY(hipMemsetAsync(&ctr[7], 0xff, sizeof(int64_t), s));
      k_smp_check<<<smp_grid(n), kSmpThreads, 0, s>>>(d_users, d_items, n, n_users, M, ctr);
      COOC_HIP_TRY(hipGetLastError());
      COOC_HIP_TRY(hipMemcpyAsync(&h_ctr[7], &ctr[7], sizeof(int64_t), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (h_ctr[7] != none) {
        int32_t bu = 0, bi = 0;
        COOC_HIP_TRY(hipMemcpy(&bu, d_users + h_ctr[7], sizeof(int32_t), hipMemcpyDeviceToHost));
        COOC_HIP_TRY(hipMemcpy(&bi, d_items + h_ctr[7], sizeof(int32_t), hipMemcpyDeviceToHost));
        return Status{COOC_ERR_ARG, "record " + std::to_string(h_ctr[7]) + ": user " + std::to_string(bu) + " (of " +
                                        std::to_string(n_users) + ") or item " + std::to_string(bi) + " (of " +
                                        std::to_string(M) + ") is out of range"};
      }
      // the arena: min(user_cut, the user's records in the call) entries per user, at most n in all
      COOC_HIP_TRY(hipMemsetAsync(st.stamp, 0, sizeof(uint32_t) * size_t(n), s));
      k_smp_user_records<<<smp_grid(n), kSmpThreads, 0, s>>>(d_users, n, ucnt);
      COOC_HIP_TRY(hipGetLastError());
    }
    return Status::Ok();
  };
  if (local.ok()) local = prepare();
  if (multi) COOC_TRY(sample_agree(*comm, b_smp_lists, local, n_windows, item_cut, user_cut, seed, s));
  COOC_TRY(local);
  COOC_TRY(launch_scan<false>(ScanCapped{ucnt, user_cut, U}, aoff, U + 1, scan, scan_err, s));

  if (m_max > 0 || multi) {
    SampleScratch w;
    if (m_max > 0) {
      COOC_TRY(b_smp_win.reserve(smp_scratch_bytes(m_max)));
      COOC_TRY(smp_scratch_init(w, m_max, b_smp_win.as<char>(), s));
    }
    // (the agreement's words have been read: its buffer now holds the windows' lists)
    if (multi) COOC_TRY(b_smp_lists.reserve(256 + 2 * sizeof(uint64_t) * size_t(m_max) + sizeof(int64_t) * 5 *
                                                      size_t(comm->world() + 1)));
    const int item_bits = smp_bits(M), user_bits = smp_bits(U);
    for (int32_t k = 0; k < n_windows; k++) {
      const int64_t g0 = window_ptr[k], m = window_ptr[k + 1] - g0;
      if (multi)
        COOC_TRY(sample_window_ranks(st, w, d_users + g0, d_items + g0, m, g0, item_bits, user_bits, M, item_cut,
                                     user_cut, uint64_t(seed), *comm, smp_icx, b_smp_lists.as<char>(), s));
      else
        COOC_TRY(sample_window(st, w, d_users + g0, d_items + g0, m, g0, item_bits, user_bits, item_cut, user_cut,
                               uint64_t(seed), s));
    }
  }

  // the outputs: the reservoirs' CSR, the totals, the item counters
  COOC_TRY(launch_scan<false>(ScanCapped{st.len, INT32_MAX, U}, d_res_ptr, U + 1, scan, scan_err, s));
  if (U > 0) k_smp_users_out<<<smp_grid(U), kSmpThreads, 0, s>>>(st.len, st.total, n_users, d_total, ctr);
  k_smp_items_out<<<smp_grid(M), kSmpThreads, 0, s>>>(st.count, M, d_item_count, ctr);
  if (U > 0)
    k_smp_gather<<<smp_grid(U * 64), kSmpThreads, 0, s>>>(st.len, aoff, st.arena, d_res_ptr, n_users, res_cap,
                                                           d_res_items, ctr);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(h_ctr, ctr, sizeof(int64_t) * 7, hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  info->rejected = h_ctr[0];
  info->fills = h_ctr[1];
  info->replacements = h_ctr[2];
  info->feedbacks = h_ctr[3];
  info->users = h_ctr[4];
  info->item_counter_sum = h_ctr[5];
  info->reservoir_items = h_ctr[6];
  if (h_ctr[6] > res_cap)
    return Status{COOC_ERR_ARG, "res_cap " + std::to_string(res_cap) + " is below the reservoirs' " +
                                    std::to_string(h_ctr[6]) + " items"};
  return Status::Ok();
}
