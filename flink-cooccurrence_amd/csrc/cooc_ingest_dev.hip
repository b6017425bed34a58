// cooc_ingest_dev.hip — the job's front end on the device: the text source's line splitter and what sits in front
// of every operator of the reference (the late drop of NonSampled...java:87-91, the TumblingEventTimeWindows
// assignment and keyBy(user)), for a log that is resident in device memory.
//
// cooc_parse_interactions_device (the semantics of cooc_ingest.cpp, byte for byte):
//   k_ing_count   per 4,096-byte tile, the '\n' bytes: 16-B loads, a 16-bit mask per thread, counts per tile
//   launch_scan   (cooc_scan.h) the tiles' prefix
//   k_ing_breaks  the same masks again, every '\n' offset stored at its rank (tile prefix + rank in the tile)
//   k_ing_parse   one thread per line; a workgroup's 256 lines are one contiguous byte range, staged in LDS with
//                 16-B loads when it fits, read from global memory otherwise (a line of any length parses)
// cooc_log_prepare_device:
//   k_lp_block_max, prefix_max   the largest timestamp of every watermark block and of the blocks before it
//   k_lp_check    late flags, the checks on kept records (first bad index by an integer min), window-end range
//   launch_scan   over the keep predicate: the compacted position of every kept record
//   k_lp_compact  (window ordinal, input index) of the kept records; k_lp_unsorted: already in firing order?
//   radix_sort_pairs (cooc_radix.h) by the ordinal's bits, stable: the firing order
//   k_lp_fire     items and sign-flipped user ids in firing order; radix_sort_pairs by user id: the CSR order
//   head flags + launch_scan: dense user indices, user_ptr, user_ids; window starts and ends
// Every atomic is an integer add, min, max or or: the outputs are bit-identical from call to call.
#include <algorithm>
#include <climits>
#include <string>

#include "cooc_ctx.h"
#include "cooc_radix.h"
#include "cooc_scan.h"
#include "cooc_window.h"

namespace cooc {

namespace {

constexpr int kIngThreads = 256, kIngChunk = 16, kIngTile = kIngThreads * kIngChunk;
constexpr int kIngLds = 16384;  // bytes of text one workgroup of k_ing_parse stages (64 per line)

inline size_t ing_al(size_t x) { return (x + 255) & ~size_t(255); }
inline unsigned ing_grid(int64_t n) { return unsigned((n + kIngThreads - 1) / kIngThreads); }

// The 16 bytes of chunk c of the text's 16-B-aligned grid: chunk c covers the text bytes [16 c - mis, 16 c - mis + 16)
// with mis = the text pointer's misalignment, so every whole chunk is one aligned 16-B load.  Bytes outside
// [0, n_bytes) read as 0 and are never loaded.
__device__ inline uint4 ing_load16(const char *__restrict__ text, int64_t n_bytes, int mis, int64_t c) {
  const int64_t b0 = c * kIngChunk - mis;
  if (b0 >= 0 && b0 + kIngChunk <= n_bytes) return *reinterpret_cast<const uint4 *>(text + b0);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int k = 0; k < kIngChunk; k++) {
    const int64_t b = b0 + k;
    if (b >= 0 && b < n_bytes) w[k >> 2] |= uint32_t(uint8_t(text[b])) << (8 * (k & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit k set: byte k of the word is '\n' (exact: no carries between the bytes)
__device__ inline uint32_t ing_nl_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;  // a zero byte where the text has '\n'
  const uint32_t y = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 in every zero byte
  return ((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u);
}
__device__ inline uint32_t ing_nl_mask(uint4 v) {
  return ing_nl_bits(v.x) | (ing_nl_bits(v.y) << 4) | (ing_nl_bits(v.z) << 8) | (ing_nl_bits(v.w) << 12);
}

// the workgroup's exclusive prefix of v over its 256 threads, and the total
__device__ inline int32_t ing_block_excl(int32_t v, int32_t *s_w, int32_t *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int32_t pre = inc - v, tot = 0;
#pragma unroll
  for (int w = 0; w < kIngThreads / 64; w++) {
    pre += w < wave ? s_w[w] : 0;
    tot += s_w[w];
  }
  *total = tot;
  return pre;
}

__global__ __launch_bounds__(kIngThreads) void k_ing_count(const char *__restrict__ text, int64_t n_bytes, int mis,
                                                          int32_t *__restrict__ counts,
                                                          unsigned long long *__restrict__ total) {
  __shared__ int32_t s_w[kIngThreads / 64];
  const int64_t c = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  const int32_t k = __popc(ing_nl_mask(ing_load16(text, n_bytes, mis, c)));
  int32_t tot;
  ing_block_excl(k, s_w, &tot);
  if (threadIdx.x == 0) {
    if (counts) counts[blockIdx.x] = tot;
    if (tot) atomicAdd(total, (unsigned long long)tot);
  }
}

// nl[r] = the offset of the r-th '\n', for r < nl_cap
__global__ __launch_bounds__(kIngThreads) void k_ing_breaks(const char *__restrict__ text, int64_t n_bytes, int mis,
                                                           const int32_t *__restrict__ tile_incl,
                                                           int32_t *__restrict__ nl, int64_t nl_cap) {
  __shared__ int32_t s_w[kIngThreads / 64];
  const int64_t c = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  uint32_t m = ing_nl_mask(ing_load16(text, n_bytes, mis, c));
  int32_t tot;
  int64_t r = int64_t(blockIdx.x ? tile_incl[blockIdx.x - 1] : 0) + ing_block_excl(__popc(m), s_w, &tot);
  const int64_t b0 = c * kIngChunk - mis;
  while (m) {
    const int k = __ffs(m) - 1;
    m &= m - 1;
    if (r < nl_cap) nl[r] = int32_t(b0 + k);
    r++;
  }
}

// Integer.valueOf / Long.valueOf over the field accumulated so far (cooc_ingest.cpp parse_int, one byte at a time)
struct IngField {
  uint64_t v = 0, lim = 0;
  int32_t n_digits = 0;
  bool neg = false, signed_ = false, bad = false;
  __device__ void begin(int64_t lo, int64_t hi) {
    v = 0, n_digits = 0, neg = false, signed_ = false, bad = false;
    lo_ = lo, hi_ = hi;
    lim = uint64_t(hi);
  }
  __device__ void byte(char ch) {
    if (bad) return;
    if (n_digits == 0 && !signed_ && (ch == '+' || ch == '-')) {
      signed_ = true;
      neg = ch == '-';
      // the magnitude accumulates unsigned: |Long.MIN_VALUE| fits in uint64
      lim = neg ? uint64_t(-(lo_ + 1)) + 1 : uint64_t(hi_);
      return;
    }
    if (ch < '0' || ch > '9') {
      bad = true;
      return;
    }
    const uint64_t d = uint64_t(ch - '0');
    if (v > (lim - d) / 10) {
      bad = true;
      return;
    }
    v = v * 10 + d;
    n_digits++;
  }
  __device__ bool ok() const { return !bad && n_digits > 0; }
  __device__ int64_t value() const { return neg ? int64_t(0) - int64_t(v - 1) - 1 : int64_t(v); }
  int64_t lo_ = 0, hi_ = 0;
};

// One line [s, e) of src (byte i of the text at src[i - bias]) -> (user, item, ts).  String.split(",") drops
// trailing empty fields only: "1,2,3,,," has three fields, "1,,3" an empty (invalid) second one, and whatever
// follows the third comma is ignored.
__device__ inline bool ing_parse_line(const char *src, int64_t bias, int64_t s, int64_t e, int32_t *u, int32_t *it,
                                      int64_t *ts) {
  IngField f;
  int fi = 0;
  f.begin(INT32_MIN, INT32_MAX);
  for (int64_t i = s; i <= e; i++) {
    const bool end = i == e;
    const char ch = end ? ',' : src[i - bias];
    if (ch != ',') {
      f.byte(ch);
      continue;
    }
    if (end && fi < 2) return false;  // fewer than three fields: split[2] -> ArrayIndexOutOfBoundsException
    if (!f.ok()) return false;
    if (fi == 0) {
      *u = int32_t(f.value());
      f.begin(INT32_MIN, INT32_MAX);
    } else if (fi == 1) {
      *it = int32_t(f.value());
      f.begin(INT64_MIN, INT64_MAX);
    } else {
      *ts = f.value();
      return true;
    }
    fi++;
  }
  return false;
}

__global__ __launch_bounds__(kIngThreads) void k_ing_parse(const char *__restrict__ text, int64_t n_bytes, int mis,
                                                          const int32_t *__restrict__ nl, int64_t n_nl,
                                                          int64_t n_lines, int32_t *__restrict__ users,
                                                          int32_t *__restrict__ items, int64_t *__restrict__ ts,
                                                          unsigned long long *__restrict__ bad) {
  __shared__ uint4 s_text[kIngLds / 16 + 1];
  __shared__ int64_t s_range[2];
  const int tid = threadIdx.x;
  const int64_t r = int64_t(blockIdx.x) * kIngThreads + tid;
  const bool live = r < n_lines;
  // line r: after the (r-1)-th '\n' up to the r-th, or up to the text's end for a last line without one
  const int64_t s = live ? (r ? int64_t(nl[r - 1]) + 1 : 0) : 0;
  const int64_t nle = live ? (r < n_nl ? int64_t(nl[r]) : n_bytes) : 0;
  int64_t e = nle;
  if (tid == 0) s_range[0] = s;
  if (live && (r == n_lines - 1 || tid == kIngThreads - 1)) s_range[1] = nle;
  __syncthreads();
  const int64_t g0 = s_range[0], g1 = s_range[1];  // the workgroup's bytes [g0, g1)
  const int64_t c0 = (g0 + mis) / kIngChunk, c1 = (g1 + mis + kIngChunk - 1) / kIngChunk;  // its chunks [c0, c1)
  const bool staged = c1 - c0 <= kIngLds / 16;
  if (staged) {
    for (int64_t c = c0 + tid; c < c1; c += kIngThreads) s_text[c - c0] = ing_load16(text, n_bytes, mis, c);
    __syncthreads();
  }
  if (!live) return;
  // byte i of the text: staged at s_text bytes [i - (16 c0 - mis)]
  const char *src = staged ? reinterpret_cast<const char *>(s_text) : text;
  const int64_t bias = staged ? c0 * kIngChunk - mis : 0;
  if (e > s && src[e - 1 - bias] == '\r') e--;  // TextInputFormat drops the '\r' of "\r\n"
  int32_t u = 0, it = 0;
  int64_t t = 0;
  if (ing_parse_line(src, bias, s, e, &u, &it, &t)) {
    users[r] = u;
    items[r] = it;
    ts[r] = t;
  } else {
    atomicMin(bad, (unsigned long long)r);
  }
}

// ---- log preparation ------------------------------------------------------------------------------------------

constexpr int kLpCtr = 8;  // [0] first bad record (unsigned min), [1] n_late, [2] smallest window end, [3] largest,
                           // [4] ordinals not in firing order, [5] or of (user key ^ the first), [6] [7] unused

__global__ __launch_bounds__(kIngThreads) void k_lp_fill(long long *__restrict__ p, int64_t n, long long v) {
  const int64_t i = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  if (i < n) p[i] = v;
}

// the largest timestamp of every block of W records (late ones included)
__global__ __launch_bounds__(kIngThreads) void k_lp_block_max(const int64_t *__restrict__ ts, int64_t n, int64_t W,
                                                             long long *__restrict__ bmax) {
  const int64_t i = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  const bool live = i < n;
  const int64_t b = live ? i / W : -1;
  long long v = live ? (long long)ts[i] : LLONG_MIN;
  // a wave inside one block (the usual case): one atomic
  const int64_t b0 = __shfl(b, 0, 64);
  if (__all(b == b0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long t = __shfl_xor(v, o, 64);
      v = t > v ? t : v;
    }
    if ((threadIdx.x & 63) == 0 && live) atomicMax(&bmax[b], v);
  } else if (live) {
    atomicMax(&bmax[b], v);
  }
}

// Exclusive prefix maximum (the identity is Long.MIN_VALUE), three launches: the tiles' maxima, their exclusive
// prefix in place by one workgroup, the tiles again with their carry.  cooc_scan.h sums; this is a max.
__global__ __launch_bounds__(kIngThreads) void k_pmax_tiles(const long long *__restrict__ in, int64_t n,
                                                           long long *__restrict__ tmax) {
  __shared__ long long s_w[kIngThreads / 64];
  const int64_t base = int64_t(blockIdx.x) * kIngTile;
  long long v = LLONG_MIN;
  for (int j = 0; j < kIngChunk; j++) {
    const int64_t i = base + j * kIngThreads + threadIdx.x;
    if (i < n) v = in[i] > v ? in[i] : v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kIngThreads / 64; w++) v = s_w[w] > v ? s_w[w] : v;
    tmax[blockIdx.x] = v;
  }
}

// the workgroup's exclusive prefix maximum of v over its 256 threads, and the maximum of all
__device__ inline long long lp_block_excl_max(long long v, long long *s_w, long long *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(inc, o, 64);
    if (lane >= o) inc = t > inc ? t : inc;
  }
  long long pre = __shfl_up(inc, 1, 64);
  if (lane == 0) pre = LLONG_MIN;
  __syncthreads();  // (s_w may still be read from the caller's last round)
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  long long tot = LLONG_MIN;
#pragma unroll
  for (int w = 0; w < kIngThreads / 64; w++) {
    if (w < wave) pre = s_w[w] > pre ? s_w[w] : pre;
    tot = s_w[w] > tot ? s_w[w] : tot;
  }
  *total = tot;
  return pre;
}

__global__ __launch_bounds__(kIngThreads) void k_pmax_carry(long long *__restrict__ tmax, int64_t n_tiles) {
  __shared__ long long s_w[kIngThreads / 64];
  long long carry = LLONG_MIN;
  for (int64_t base = 0; base < n_tiles; base += kIngThreads) {
    const int64_t i = base + threadIdx.x;
    const long long v = i < n_tiles ? tmax[i] : LLONG_MIN;
    long long tot;
    const long long pre = lp_block_excl_max(v, s_w, &tot);
    if (i < n_tiles) tmax[i] = pre > carry ? pre : carry;
    carry = tot > carry ? tot : carry;
  }
}

__global__ __launch_bounds__(kIngThreads) void k_pmax_apply(const long long *__restrict__ in, int64_t n,
                                                           const long long *__restrict__ tcarry,
                                                           long long *__restrict__ out) {
  __shared__ long long s_w[kIngThreads / 64];
  const int64_t b0 = int64_t(blockIdx.x) * kIngTile + int64_t(threadIdx.x) * kIngChunk;
  long long x[kIngChunk], run = LLONG_MIN;
#pragma unroll
  for (int k = 0; k < kIngChunk; k++) {
    x[k] = run;  // exclusive within the thread's run
    const long long v = b0 + k < n ? in[b0 + k] : LLONG_MIN;
    run = v > run ? v : run;
  }
  long long tot;
  long long pre = lp_block_excl_max(run, s_w, &tot);
  const long long c = tcarry[blockIdx.x];
  pre = c > pre ? c : pre;
#pragma unroll
  for (int k = 0; k < kIngChunk; k++)
    if (b0 + k < n) out[b0 + k] = x[k] > pre ? x[k] : pre;
}

// Record i is late iff ts[i] = Long.MIN_VALUE (the operator's initial watermark) or ts[i] < m_b, the largest
// timestamp of the blocks before its block b = i / W (the watermark m_b - 1 was emitted after block b - 1).
// mpre == NULL (W == 0, or a single block): no watermark before the end.
struct LpLate {
  const int64_t *ts;
  const long long *mpre;
  int64_t W;
  __device__ bool late(int64_t i) const {
    const int64_t t = ts[i];
    if (t == INT64_MIN) return true;
    return mpre != nullptr && t < int64_t(mpre[i / W]);
  }
  __device__ int64_t operator()(int64_t i) const { return late(i) ? 0 : 1; }  // the scan's input: kept
};

__global__ __launch_bounds__(kIngThreads) void k_lp_check(LpLate lt, const int32_t *__restrict__ items, int64_t n,
                                                         int32_t n_items, int64_t size, int64_t ts_lo, int64_t ts_hi,
                                                         long long *__restrict__ ctr) {
  const int64_t i = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  const bool live = i < n;
  const bool late = live && lt.late(i);
  const bool kept = live && !late;
  bool good = false;
  long long we = 0;
  if (kept) {
    const int64_t t = lt.ts[i];
    const int32_t it = items[i];
    good = it >= 0 && it < n_items && t >= ts_lo && t <= ts_hi;
    if (good)
      we = window_max_ts(t, size);
    else
      atomicMin(reinterpret_cast<unsigned long long *>(&ctr[0]), (unsigned long long)i);
  }
  const uint64_t m_late = __ballot(late), m_good = __ballot(good);
  long long lo = good ? we : LLONG_MAX, hi = good ? we : LLONG_MIN;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    if (m_late) atomicAdd(reinterpret_cast<unsigned long long *>(&ctr[1]), (unsigned long long)__popcll(m_late));
    if (m_good) {
      atomicMin(&ctr[2], lo);
      atomicMax(&ctr[3], hi);
    }
  }
}

// the kept records in arrival order: (window ordinal, input index)
__global__ __launch_bounds__(kIngThreads) void k_lp_compact(LpLate lt, int64_t n, const int32_t *__restrict__ pos,
                                                           int64_t size, int64_t we_min, uint64_t *__restrict__ okey,
                                                           int32_t *__restrict__ oidx) {
  const int64_t i = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  if (i >= n || lt.late(i)) return;
  const int64_t we = window_max_ts(lt.ts[i], size);
  okey[pos[i]] = (uint64_t(we) - uint64_t(we_min)) / uint64_t(size);
  oidx[pos[i]] = int32_t(i);
}

__global__ __launch_bounds__(kIngThreads) void k_lp_unsorted(const uint64_t *__restrict__ okey, int64_t n,
                                                            long long *__restrict__ ctr) {
  const int64_t j = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  const bool down = j > 0 && j < n && okey[j] < okey[j - 1];
  if (__ballot(down) && (threadIdx.x & 63) == 0) atomicOr(reinterpret_cast<unsigned long long *>(&ctr[4]), 1ull);
}

// firing order j: the record's item, its user id as an unsigned key (sign bit flipped: ascending as signed int32)
__global__ __launch_bounds__(kIngThreads) void k_lp_fire(const int32_t *__restrict__ sidx, int64_t n,
                                                        const int32_t *__restrict__ users,
                                                        const int32_t *__restrict__ items,
                                                        int32_t *__restrict__ rec_item, uint32_t *__restrict__ ukey,
                                                        int32_t *__restrict__ uval, long long *__restrict__ ctr) {
  const int64_t j = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  uint32_t diff = 0;
  if (j < n) {
    const int32_t i = sidx[j];
    const uint32_t k = uint32_t(users[i]) ^ 0x80000000u;
    if (rec_item) rec_item[j] = items[i];
    ukey[j] = k;
    uval[j] = int32_t(j);
    diff = k ^ (uint32_t(users[sidx[0]]) ^ 0x80000000u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) diff |= __shfl_xor(diff, o, 64);
  if ((threadIdx.x & 63) == 0 && diff) atomicOr(reinterpret_cast<unsigned long long *>(&ctr[5]), (unsigned long long)diff);
}

// CSR order k (by user, then firing order): the dense index of every user, its id and start, its items, and the
// index scattered back to the record's place in the firing order
__global__ __launch_bounds__(kIngThreads) void k_lp_users(const uint32_t *__restrict__ sukey,
                                                         const int32_t *__restrict__ suval,
                                                         const int32_t *__restrict__ uidx1, int64_t n,
                                                         const int32_t *__restrict__ sidx,
                                                         const int32_t *__restrict__ items,
                                                         int32_t *__restrict__ rec_user, int32_t *__restrict__ user_ids,
                                                         int64_t *__restrict__ user_ptr,
                                                         int32_t *__restrict__ user_items) {
  const int64_t k = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  if (k >= n) return;
  const int32_t d = uidx1[k] - 1, j = suval[k];
  if (k == 0 || sukey[k] != sukey[k - 1]) {
    if (user_ids) user_ids[d] = int32_t(sukey[k] ^ 0x80000000u);
    if (user_ptr) user_ptr[d] = k;
  }
  if (k == n - 1 && user_ptr) user_ptr[d + 1] = n;
  if (user_items) user_items[k] = items[sidx[j]];
  if (rec_user) rec_user[j] = d;
}

// firing order j: window w starts where the ordinal changes; its end is the smallest end + ordinal * size
__global__ __launch_bounds__(kIngThreads) void k_lp_windows(const uint64_t *__restrict__ skey,
                                                           const int32_t *__restrict__ widx1, int64_t n, int64_t size,
                                                           int64_t we_min, int64_t *__restrict__ wptr,
                                                           int64_t *__restrict__ wts) {
  const int64_t j = int64_t(blockIdx.x) * kIngThreads + threadIdx.x;
  if (j >= n) return;
  if (j == 0 || skey[j] != skey[j - 1]) {
    const int32_t w = widx1[j] - 1;
    wptr[w] = j;
    wts[w] = int64_t(uint64_t(we_min) + skey[j] * uint64_t(size));
  }
  if (j == n - 1) wptr[widx1[j]] = n;
}

Status prefix_max_exclusive(const long long *in, int64_t n, long long *out, long long *tiles, hipStream_t s) {
  if (n <= 0) return Status::Ok();
  const int64_t n_tiles = (n + kIngTile - 1) / kIngTile;
  k_pmax_tiles<<<unsigned(n_tiles), kIngThreads, 0, s>>>(in, n, tiles);
  k_pmax_carry<<<1, kIngThreads, 0, s>>>(tiles, n_tiles);
  k_pmax_apply<<<unsigned(n_tiles), kIngThreads, 0, s>>>(in, n, tiles, out);
  COOC_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

int bits_of(uint64_t v) {
  int b = 0;
  while (v) b++, v >>= 1;
  return b;
}

}  // namespace

}  // namespace cooc

using namespace cooc;

Status cooc_ctx::parse_device(const char *d_text, int64_t n_bytes, int64_t cap, int32_t *d_users, int32_t *d_items,
                              int64_t *d_ts, hipStream_t s, int64_t *n_records, int64_t *bad_line) {
  if (bad_line) *bad_line = -1;
  if (n_bytes < 0 || n_bytes >= (int64_t(1) << 31))
    return Status{COOC_ERR_ARG, "cooc_parse_interactions_device: n_bytes must be in [0, 2^31)"};
  if (!n_records || (n_bytes > 0 && !d_text))
    return Status{COOC_ERR_ARG, "cooc_parse_interactions_device: a required pointer is NULL"};
  const bool fill = d_users && d_items && d_ts;
  if (n_bytes == 0) {
    *n_records = 0;
    return Status::Ok();
  }
  COOC_HIP_TRY(hipSetDevice(device));
  const int mis = int(reinterpret_cast<uintptr_t>(d_text) & 15u);
  const int64_t n_chunks = (n_bytes + mis + kIngChunk - 1) / kIngChunk;
  const int64_t n_tiles = (n_chunks + kIngThreads - 1) / kIngThreads;
  // scratch: two words, the tiles' counts and their prefix, the scan's state (the '\n' offsets: b_ingest_aux)
  const size_t o_ctr = 0, o_counts = o_ctr + ing_al(2 * sizeof(int64_t));
  const size_t o_incl = o_counts + ing_al(sizeof(int32_t) * size_t(n_tiles));
  const size_t o_scan = o_incl + ing_al(sizeof(int32_t) * size_t(n_tiles));
  const size_t o_end = o_scan + ing_al(scan_ws_bytes(n_tiles));
  COOC_TRY(b_ingest.reserve(o_end));
  char *base = b_ingest.as<char>();
  unsigned long long *ctr = reinterpret_cast<unsigned long long *>(base + o_ctr);
  int32_t *counts = reinterpret_cast<int32_t *>(base + o_counts);
  COOC_HIP_TRY(hipMemsetAsync(&ctr[0], 0, sizeof(int64_t), s));
  COOC_HIP_TRY(hipMemsetAsync(&ctr[1], 0xff, sizeof(int64_t), s));  // above every index for the unsigned min
  k_ing_count<<<unsigned(n_tiles), kIngThreads, 0, s>>>(d_text, n_bytes, mis, fill ? counts : nullptr, &ctr[0]);
  COOC_HIP_TRY(hipGetLastError());
  int64_t n_nl = 0;
  char last = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&n_nl, &ctr[0], sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipMemcpyAsync(&last, d_text + n_bytes - 1, 1, hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  const int64_t n_lines = n_nl + (last != '\n' ? 1 : 0);  // a last line without '\n' is a record
  if (!fill) {
    *n_records = n_lines;
    return Status::Ok();
  }
  // the host parser stops at the first rejected line, or at line `cap` if none before it is rejected
  const int64_t n_parse = std::min(n_lines, std::max<int64_t>(cap, 0));
  int64_t h_bad = -1;
  if (n_parse > 0) {
    const int64_t nl_cap = std::min(n_nl, n_parse);
    COOC_TRY(b_ingest_aux.reserve(sizeof(int32_t) * size_t(nl_cap + 1)));
    int32_t *incl = reinterpret_cast<int32_t *>(base + o_incl);
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(base + o_scan);
    int32_t *nl = b_ingest_aux.as<int32_t>();
    int64_t scan_err = 0;
    COOC_TRY(launch_scan_ws<true>(ScanI32{counts}, incl, n_tiles, scan, &scan_err, s));
    if (nl_cap > 0) k_ing_breaks<<<unsigned(n_tiles), kIngThreads, 0, s>>>(d_text, n_bytes, mis, incl, nl, nl_cap);
    k_ing_parse<<<ing_grid(n_parse), kIngThreads, 0, s>>>(d_text, n_bytes, mis, nl, nl_cap, n_parse, d_users, d_items,
                                                          d_ts, &ctr[1]);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemcpyAsync(&h_bad, &ctr[1], sizeof(int64_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
  }
  if (h_bad != -1) {
    if (bad_line) *bad_line = h_bad;
    return Status{COOC_ERR_ARG, "line " + std::to_string(h_bad) + " is not 'user,item,timestamp'"};
  }
  if (n_lines > cap)
    return Status{COOC_ERR_ARG, "the text holds " + std::to_string(n_lines) + " records, more than the " +
                                    std::to_string(cap) + " given"};
  *n_records = n_lines;
  return Status::Ok();
}

Status cooc_ctx::log_prepare_device(int64_t n, const int32_t *d_users, const int32_t *d_items, const int64_t *d_ts,
                                    int64_t W, int32_t *d_rec_user, int32_t *d_rec_item, int32_t *d_user_ids,
                                    int64_t *d_user_ptr, int32_t *d_user_items, int64_t *window_ptr, int64_t *window_ts,
                                    int64_t cap_windows, hipStream_t s, cooc_log_info *info) {
  if (!info) return Status{COOC_ERR_ARG, "cooc_log_prepare_device: info is NULL"};
  *info = cooc_log_info{};
  info->bad_record = -1;
  if (n < 0 || n >= (int64_t(1) << 31))
    return Status{COOC_ERR_ARG, "cooc_log_prepare_device: n_records must be in [0, 2^31)"};
  if (W < 0) return Status{COOC_ERR_ARG, "cooc_log_prepare_device: records_per_watermark must be >= 0"};
  if (n > 0 && (!d_users || !d_items || !d_ts))
    return Status{COOC_ERR_ARG, "cooc_log_prepare_device: a required pointer is NULL"};
  COOC_HIP_TRY(hipSetDevice(device));
  static const int64_t zero = 0;
  const bool want_windows = window_ptr || window_ts;
  auto no_records = [&]() -> Status {  // no kept record: empty outputs
    if (d_user_ptr) COOC_HIP_TRY(hipMemcpyAsync(d_user_ptr, &zero, sizeof(int64_t), hipMemcpyHostToDevice, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    if (want_windows && cap_windows < 0) return Status{COOC_ERR_ARG, "cooc_log_prepare_device: cap_windows < 0"};
    if (window_ptr) window_ptr[0] = 0;
    return Status::Ok();
  };
  if (n == 0) return no_records();

  const int64_t size = cfg.window_size_ms;
  // the operator's window expression stays in range for ts in [MIN + 2 size, MAX - 2 size]
  const bool any_ts = size <= (INT64_MAX >> 2);
  const int64_t ts_lo = any_ts ? INT64_MIN + 2 * size : 1, ts_hi = any_ts ? INT64_MAX - 2 * size : 0;
  const int64_t nb = W > 0 ? (n + W - 1) / W : 0;  // watermark blocks
  const bool blocks = nb > 1;                      // (one block: no watermark before the end)
  const int64_t nb_tiles = blocks ? (nb + kIngTile - 1) / kIngTile : 0;

  // scratch, sized by n (the kept records are known only after the first pass)
  const size_t rdx = std::max(radix_sort_tmp_bytes<uint64_t, int32_t>(n), radix_sort_tmp_bytes<uint32_t, int32_t>(n));
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += ing_al(bytes);
    return at;
  };
  const size_t o_ctr = take(sizeof(int64_t) * kLpCtr), o_bmax = take(sizeof(int64_t) * size_t(nb)),
               o_mpre = take(sizeof(int64_t) * size_t(nb)), o_tiles = take(sizeof(int64_t) * size_t(nb_tiles)),
               o_pos = take(sizeof(int32_t) * size_t(n)), o_scan = take(scan_ws_bytes(n)),
               o_ckey = take(sizeof(uint64_t) * size_t(n)), o_cidx = take(sizeof(int32_t) * size_t(n)),
               o_skey = take(sizeof(uint64_t) * size_t(n)), o_sidx = take(sizeof(int32_t) * size_t(n)),
               o_ukey = take(sizeof(uint32_t) * size_t(n)),
               o_uval = take(sizeof(int32_t) * size_t(n)), o_sukey = take(sizeof(uint32_t) * size_t(n)),
               o_suval = take(sizeof(int32_t) * size_t(n)), o_rdx = take(rdx);
  COOC_TRY(b_ingest.reserve(o));
  char *base = b_ingest.as<char>();
  long long *ctr = reinterpret_cast<long long *>(base + o_ctr);
  long long *bmax = reinterpret_cast<long long *>(base + o_bmax), *mpre = reinterpret_cast<long long *>(base + o_mpre);
  long long *tiles = reinterpret_cast<long long *>(base + o_tiles);
  int32_t *pos = reinterpret_cast<int32_t *>(base + o_pos);
  unsigned long long *scan = reinterpret_cast<unsigned long long *>(base + o_scan);
  uint64_t *ckey = reinterpret_cast<uint64_t *>(base + o_ckey), *skey = reinterpret_cast<uint64_t *>(base + o_skey);
  int32_t *cidx = reinterpret_cast<int32_t *>(base + o_cidx), *sidx = reinterpret_cast<int32_t *>(base + o_sidx);
  uint32_t *ukey = reinterpret_cast<uint32_t *>(base + o_ukey), *sukey = reinterpret_cast<uint32_t *>(base + o_sukey);
  int32_t *uval = reinterpret_cast<int32_t *>(base + o_uval), *suval = reinterpret_cast<int32_t *>(base + o_suval);
  void *rdx_tmp = base + o_rdx;

  // 1. the blocks' maxima and their prefix maximum
  if (blocks) {
    k_lp_fill<<<ing_grid(nb), kIngThreads, 0, s>>>(bmax, nb, LLONG_MIN);  // (no byte pattern of a memset)
    k_lp_block_max<<<ing_grid(n), kIngThreads, 0, s>>>(d_ts, n, W, bmax);
    COOC_HIP_TRY(hipGetLastError());
    COOC_TRY(prefix_max_exclusive(bmax, nb, mpre, tiles, s));
  }
  const LpLate lt{d_ts, blocks ? mpre : nullptr, W};

  // 2. late records, the checks on the kept ones, the range of the window ends
  static const long long kCtrInit[kLpCtr] = {-1, 0, LLONG_MAX, LLONG_MIN, 0, 0, 0, 0};  // (outlives the copy)
  long long h_ctr[kLpCtr];
  COOC_HIP_TRY(hipMemcpyAsync(ctr, kCtrInit, sizeof(kCtrInit), hipMemcpyHostToDevice, s));
  k_lp_check<<<ing_grid(n), kIngThreads, 0, s>>>(lt, d_items, n, cfg.n_items, size, ts_lo, ts_hi, ctr);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  info->n_late = h_ctr[1];
  info->n_kept = n - h_ctr[1];
  if (h_ctr[0] != -1) {  // before any output is written
    info->bad_record = h_ctr[0];
    int32_t bi = 0;
    int64_t bt = 0;
    COOC_HIP_TRY(hipMemcpy(&bi, d_items + h_ctr[0], sizeof(int32_t), hipMemcpyDeviceToHost));
    COOC_HIP_TRY(hipMemcpy(&bt, d_ts + h_ctr[0], sizeof(int64_t), hipMemcpyDeviceToHost));
    if (bi < 0 || bi >= cfg.n_items)
      return Status{COOC_ERR_ARG, "record " + std::to_string(h_ctr[0]) + ": item " + std::to_string(bi) +
                                      " is outside [0, " + std::to_string(cfg.n_items) + ")"};
    return Status{COOC_ERR_ARG, "record " + std::to_string(h_ctr[0]) + ": timestamp " + std::to_string(bt) +
                                    " is within two window sizes of the end of the long range"};
  }
  const int64_t nk = info->n_kept;
  if (nk == 0) return no_records();
  const int64_t we_min = h_ctr[2], we_max = h_ctr[3];
  const uint64_t ord_max = (uint64_t(we_max) - uint64_t(we_min)) / uint64_t(size);

  // 3. compaction: the kept records' (window ordinal, input index) in arrival order
  int64_t scan_err = 0;
  COOC_TRY(launch_scan_ws<false>(lt, pos, n, scan, &scan_err, s));
  k_lp_compact<<<ing_grid(n), kIngThreads, 0, s>>>(lt, n, pos, size, we_min, ckey, cidx);
  // 4. the firing order: stable by ordinal, skipped when the log is already in it (the usual ascending log)
  k_lp_unsorted<<<ing_grid(nk), kIngThreads, 0, s>>>(ckey, nk, ctr);
  COOC_HIP_TRY(hipGetLastError());
  COOC_HIP_TRY(hipMemcpyAsync(&h_ctr[4], &ctr[4], sizeof(long long), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (h_ctr[4]) {
    COOC_TRY((radix_sort_pairs<uint64_t, int32_t>(ckey, cidx, skey, sidx, nk, 0, bits_of(ord_max), false, rdx_tmp, s)));
  } else {
    skey = ckey;
    sidx = cidx;
  }

  // the windows: head flags over the ordinals, their count, then the lists straight into the caller's arrays
  {
    int32_t *widx1 = pos;  // (the compaction's positions are consumed)
    COOC_TRY(launch_scan_ws<true>(ScanKeyHead<uint64_t>{skey}, widx1, nk, scan, &scan_err, s));
    int32_t n_win = 0;
    COOC_HIP_TRY(hipMemcpyAsync(&n_win, widx1 + (nk - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    info->n_windows = n_win;
    if (cap_windows >= n_win && want_windows) {
      COOC_TRY(b_ingest_aux.reserve(sizeof(int64_t) * size_t(2 * int64_t(n_win) + 1)));
      int64_t *wptr = b_ingest_aux.as<int64_t>(), *wts = wptr + n_win + 1;
      k_lp_windows<<<ing_grid(nk), kIngThreads, 0, s>>>(skey, widx1, nk, size, we_min, wptr, wts);
      COOC_HIP_TRY(hipGetLastError());
      if (window_ptr)
        COOC_HIP_TRY(hipMemcpyAsync(window_ptr, wptr, sizeof(int64_t) * size_t(n_win + 1), hipMemcpyDeviceToHost, s));
      if (window_ts)
        COOC_HIP_TRY(hipMemcpyAsync(window_ts, wts, sizeof(int64_t) * size_t(n_win), hipMemcpyDeviceToHost, s));
    }
  }

  // 5.-7. items in firing order; the users: stable by id, head flags, dense indices, the CSR, the scatter back
  {
    k_lp_fire<<<ing_grid(nk), kIngThreads, 0, s>>>(sidx, nk, d_users, d_items, d_rec_item, ukey, uval, ctr);
    COOC_HIP_TRY(hipGetLastError());
    COOC_HIP_TRY(hipMemcpyAsync(&h_ctr[5], &ctr[5], sizeof(long long), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    // bits above the highest one in which two ids differ do not order them
    COOC_TRY((radix_sort_pairs<uint32_t, int32_t>(ukey, uval, sukey, suval, nk, 0, bits_of(uint64_t(h_ctr[5])), false,
                                                  rdx_tmp, s)));
    int32_t *uidx1 = pos;
    COOC_TRY(launch_scan_ws<true>(ScanKeyHead<uint32_t>{sukey}, uidx1, nk, scan, &scan_err, s));
    k_lp_users<<<ing_grid(nk), kIngThreads, 0, s>>>(sukey, suval, uidx1, nk, sidx, d_items, d_rec_user, d_user_ids,
                                                    d_user_ptr, d_user_items);
    COOC_HIP_TRY(hipGetLastError());
    int32_t n_u = 0;
    COOC_HIP_TRY(hipMemcpyAsync(&n_u, uidx1 + (nk - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    info->n_users = n_u;
  }
  if (want_windows && cap_windows < info->n_windows)
    return Status{COOC_ERR_ARG, "the log has " + std::to_string(info->n_windows) + " windows, more than the " +
                                    std::to_string(cap_windows) + " given"};
  return Status::Ok();
}
