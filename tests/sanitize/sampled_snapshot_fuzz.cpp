// sampled_snapshot_fuzz.cpp — the parser of a sampled context's snapshot blob (cooc_sampling_snapshot_inspect, which
// is also the first check of cooc_sampling_restore_finish) under AddressSanitizer + UndefinedBehaviorSanitizer.
// tests/test_sampled_snapshot_cpu.py builds this with g++ -fsanitize=address,undefined against
// flink-cooccurrence_amd/csrc/cooc_snapshot.cpp (host-only: no HIP) and runs it as a child process.
//
// The blobs are laid out by hand here, from the format's description and not through the library's
// own writer: a 64-B header with the magic "COOCSMP2" and format 2, 20 directory entries of 40 B, then the
// sections back to back, each padded to 8 B; section 16 (the sampler's scalars) holds real words and a real
// checksum, the other sections junk that inspect never reads.  Valid blobs must inspect to their own numbers;
// every truncation, every single-bit flip of the header, the directory and section 16, random bytes, random section
// counts (laid out consistently, the header's checksum valid, so the count relations are what has to catch them),
// bad sampler scalars, and a format-1 blob must be COOC_ERR_ARG; the format-1 inspect must refuse the valid blobs.
// Every blob is handed over in a heap buffer of exactly its length, so a read past the end aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/cooc.h"

namespace {

constexpr int kSections = 20;
constexpr int64_t kHeader = 64 + 40 * kSections;
const int kElem[kSections] = {8, 4, 8, 4, 4, 8, 4, 4, 8, 4, 8, 8, 8, 4, 4, 8, 4, 2, 4, 4};

uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Blob {
  const char *magic = "COOCSMP2";
  int32_t format = 2, n_sections = kSections, n_items = 1000, user_cut = 4, rank = 0, world = 1;
  int64_t window_ms = 1000;
  int64_t count[kSections];
  int64_t smp[8] = {20, 0xC0FFEE, 3, 40, 5, 2, 0, 0};  // item_cut, seed, rejected, fills, replacements, feedbacks
};

void put32(std::vector<uint8_t> &b, size_t at, uint32_t v) {
  for (int i = 0; i < 4; i++) b[at + i] = uint8_t(v >> (8 * i));
}
void put64(std::vector<uint8_t> &b, size_t at, uint64_t v) {
  for (int i = 0; i < 8; i++) b[at + i] = uint8_t(v >> (8 * i));
}
uint64_t get64(const std::vector<uint8_t> &b, size_t at) {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v |= uint64_t(b[at + i]) << (8 * i);
  return v;
}

// counts: users, history items, rows, entries, pending windows, pending records, counted items, users with a total
Blob layout(int64_t users, int64_t hist, int64_t rows, int64_t entries, int64_t windows, int64_t records, int64_t counted,
            int64_t totals) {
  Blob B;
  const int64_t counts[kSections] = {16, users, users + 1, hist, rows, rows + 1, entries, entries, rows, 0, 0,
                                     windows, windows + 1, records, records, 8, counted, counted, totals, totals};
  for (int k = 0; k < kSections; k++) B.count[k] = counts[k];
  return B;
}

// the sections laid out from their counts, section 16 and its checksum real, the header sealed
std::vector<uint8_t> serialize(const Blob &B) {
  int64_t off[kSections], total = kHeader;
  for (int k = 0; k < kSections; k++) {
    off[k] = total;
    total += (B.count[k] * kElem[k] + 7) & ~int64_t(7);
  }
  std::vector<uint8_t> b(size_t(total), 0xA5);
  std::memcpy(b.data(), B.magic, 8);
  put32(b, 8, uint32_t(B.format));
  put32(b, 12, uint32_t(B.n_sections));
  put64(b, 16, uint64_t(total));
  put32(b, 24, uint32_t(B.n_items));
  put32(b, 28, uint32_t(B.user_cut));
  put64(b, 32, uint64_t(B.window_ms));
  put32(b, 40, uint32_t(B.rank));
  put32(b, 44, uint32_t(B.world));
  put64(b, 56, 0);
  uint64_t smp_sum = 0;
  if (B.count[15] == 8) {
    for (uint64_t i = 0; i < 8; i++) {
      put64(b, size_t(off[15]) + size_t(i) * 8, uint64_t(B.smp[i]));
      smp_sum += splitmix64(uint64_t(B.smp[i]) ^ i);
    }
  }
  for (int k = 0; k < kSections; k++) {
    const size_t at = 64 + size_t(k) * 40;
    put32(b, at, uint32_t(k + 1));
    put32(b, at + 4, uint32_t(kElem[k]));
    put64(b, at + 8, uint64_t(off[k]));
    put64(b, at + 16, uint64_t(B.count[k] * kElem[k]));
    put64(b, at + 24, uint64_t(B.count[k]));
    put64(b, at + 32, k == 15 ? smp_sum : 0x1234567800000000ull + uint64_t(k));
  }
  put64(b, 48, 0);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < uint64_t(kHeader / 8); i++) sum += splitmix64(get64(b, size_t(i) * 8) ^ i);
  put64(b, 48, sum);
  return b;
}

// through a heap copy of exactly n bytes
int inspect(const std::vector<uint8_t> &b, cooc_snapshot_info *info, cooc_sampling_snapshot_info *sinfo) {
  uint8_t *heap = b.empty() ? nullptr : new uint8_t[b.size()];
  if (heap) std::memcpy(heap, b.data(), b.size());
  const int st = cooc_sampling_snapshot_inspect(heap, int64_t(b.size()), info, sinfo);
  delete[] heap;
  return st;
}
int inspect_format1(const std::vector<uint8_t> &b, cooc_snapshot_info *info) {
  uint8_t *heap = b.empty() ? nullptr : new uint8_t[b.size()];
  if (heap) std::memcpy(heap, b.data(), b.size());
  const int st = cooc_snapshot_inspect(heap, int64_t(b.size()), info);
  delete[] heap;
  return st;
}

int n_fail = 0;
void expect(bool ok, const char *what, long long i) {
  if (ok) return;
  n_fail++;
  if (n_fail < 20) std::fprintf(stderr, "sampled_snapshot_fuzz: %s (case %lld)\n", what, i);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  auto u = [&](int64_t lo, int64_t hi) { return lo + int64_t(rng() % uint64_t(hi - lo + 1)); };
  cooc_snapshot_info info;
  cooc_sampling_snapshot_info sinfo;
  long long n_cases = 0;

  // ---- valid blobs inspect to their own numbers, and the format-1 inspect refuses them
  for (int c = 0; c < 200; c++) {
    const int64_t users = u(0, 30), hist = users + u(0, 50) * (users > 0), rows = u(0, 20), entries = rows + u(0, 60) * (rows > 0);
    const int64_t windows = u(0, 3), records = windows + u(0, 40) * (windows > 0), counted = u(0, 40), totals = users + u(0, 9);
    Blob B = layout(users, hist, rows, entries, windows, records, counted, totals);
    B.n_items = int32_t(u(40, 1 << 20));
    B.user_cut = int32_t(u(1, 32767));
    B.window_ms = u(1, 1 << 30);
    B.smp[0] = u(1, 32767);
    B.smp[1] = int64_t(rng());
    for (int k = 2; k < 6; k++) B.smp[k] = u(0, int64_t(1) << 40);
    const std::vector<uint8_t> b = serialize(B);
    const int st = inspect(b, &info, &sinfo);
    expect(st == COOC_OK, "a valid blob was refused", c);
    expect(info.bytes == int64_t(b.size()) && info.n_users == users && info.history_items == hist && info.global_rows == rows &&
               info.global_entries == entries && info.pending_windows == windows && info.pending_records == records &&
               info.format == 2 && info.rank == 0 && info.world == 1,
           "info differs from the blob", c);
    expect(sinfo.item_cut == B.smp[0] && sinfo.seed == B.smp[1] && sinfo.rejected == B.smp[2] && sinfo.fills == B.smp[3] &&
               sinfo.replacements == B.smp[4] && sinfo.feedbacks == B.smp[5] && sinfo.counted_items == counted &&
               sinfo.total_users == totals,
           "sinfo differs from the blob", c);
    expect(inspect_format1(b, &info) == COOC_ERR_ARG, "the format-1 inspect took a sampled blob", c);
    n_cases++;
  }

  const Blob good = layout(7, 40, 5, 33, 2, 9, 6, 9);
  const std::vector<uint8_t> gb = serialize(good);
  expect(inspect(gb, &info, &sinfo) == COOC_OK, "the base blob was refused", 0);

  // ---- every truncation, and a longer buffer
  for (size_t n = 0; n < gb.size(); n++) {
    std::vector<uint8_t> t(gb.begin(), gb.begin() + long(n));
    expect(inspect(t, &info, &sinfo) == COOC_ERR_ARG, "a truncated blob passed", (long long)n);
    n_cases++;
  }
  {
    std::vector<uint8_t> t = gb;
    t.push_back(0);
    expect(inspect(t, &info, &sinfo) == COOC_ERR_ARG, "a blob with a byte appended passed", 0);
  }

  // ---- every single-bit flip of the header, the directory and the sampler's scalars
  const int64_t smp_off = int64_t(get64(gb, 64 + 15 * 40 + 8));
  for (int64_t bit = 0; bit < (kHeader + 64) * 8; bit++) {
    std::vector<uint8_t> t = gb;
    const int64_t byte = bit >> 3;
    t[size_t(byte < kHeader ? byte : smp_off + (byte - kHeader))] ^= uint8_t(1u << (bit & 7));
    expect(inspect(t, &info, &sinfo) == COOC_ERR_ARG, "a flipped bit passed", bit);
    n_cases++;
  }

  // ---- random bytes, also behind a valid magic, version and section count
  for (int c = 0; c < 3000; c++) {
    std::vector<uint8_t> t(size_t(u(0, 2 * kHeader)));
    for (auto &x : t) x = uint8_t(rng());
    if ((c & 3) == 0 && t.size() >= 16) {
      std::memcpy(t.data(), "COOCSMP2", 8);
      put32(t, 8, 2);
      put32(t, 12, kSections);
    }
    expect(inspect(t, &info, &sinfo) == COOC_ERR_ARG, "random bytes passed", c);
    n_cases++;
  }

  // ---- random section counts, laid out consistently and sealed: OK exactly when every relation holds
  for (int c = 0; c < 4000; c++) {
    Blob B = good;
    const int n_edit = int(u(1, 3));
    for (int e = 0; e < n_edit; e++) B.count[u(0, kSections - 1)] = u(0, 12);
    const int64_t *n = B.count;
    const bool ok = n[0] == 16 && n[2] == n[1] + 1 && n[5] == n[4] + 1 && n[8] == n[4] && n[6] == n[7] && n[9] == n[10] &&
                    n[12] == n[11] + 1 && n[13] == n[14] && n[1] <= n[3] && n[4] <= n[6] && n[11] <= n[13] && n[9] == 0 &&
                    n[15] == 8 && n[16] == n[17] && n[18] == n[19] && n[18] >= n[1];
    if (n[9] != 0 && n[9] == n[10]) continue;  // (row sums of other ranks with world 1: left to the restore)
    const int st = inspect(serialize(B), &info, &sinfo);
    expect(st == (ok ? COOC_OK : COOC_ERR_ARG), ok ? "consistent counts were refused" : "unrelated section counts passed", c);
    n_cases++;
  }
  // each relation of the sampler's sections, one broken at a time
  {
    const int grow[] = {15, 16, 17, 18, 19};
    for (int k : grow) {
      Blob B = good;
      B.count[k] += 1;
      expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "a broken sampler relation passed", k);
      n_cases++;
    }
    Blob B = good;  // fewer users with a total than with a history
    B.count[18] = B.count[19] = good.count[1] - 1;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "fewer totals than histories passed", 0);
    B = good;  // more counted items than items
    B.n_items = 5;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "more counted items than items passed", 0);
  }

  // ---- the sampler's scalars
  {
    const int64_t bad_cut[] = {0, -1, 32768, int64_t(1) << 40};
    for (int64_t v : bad_cut) {
      Blob B = good;
      B.smp[0] = v;
      expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "a bad item_cut passed", (long long)v);
    }
    for (int k = 2; k < 6; k++) {
      Blob B = good;
      B.smp[k] = -1;
      expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "a negative counter passed", k);
    }
    for (int k = 6; k < 8; k++) {
      Blob B = good;
      B.smp[k] = 1;
      expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "a reserved scalar passed", k);
    }
    Blob B = good;  // any seed is fine
    B.smp[1] = INT64_MIN;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_OK, "a seed was refused", 0);
  }

  // ---- the header's fields, and the other format's identity
  {
    Blob B = good;
    B.magic = "COOCSNP1";
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "the format-1 magic passed", 0);
    B = good;
    B.format = 1;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "format 1 passed", 0);
    B = good;
    B.n_sections = 15;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "15 sections passed", 0);
    B = good;
    B.n_items = 0;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "n_items 0 passed", 0);
    B = good;
    B.window_ms = 0;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "window 0 passed", 0);
    B = good;
    B.rank = 1;
    expect(inspect(serialize(B), &info, &sinfo) == COOC_ERR_ARG, "rank >= world passed", 0);
  }

  // ---- NULL arguments
  expect(cooc_sampling_snapshot_inspect(nullptr, 0, &info, &sinfo) == COOC_ERR_ARG, "NULL bytes passed", 0);
  expect(cooc_sampling_snapshot_inspect(nullptr, int64_t(gb.size()), &info, &sinfo) == COOC_ERR_ARG, "NULL bytes with a length passed", 0);
  expect(cooc_sampling_snapshot_inspect(gb.data(), -1, &info, &sinfo) == COOC_ERR_ARG, "a negative length passed", 0);
  expect(cooc_sampling_snapshot_inspect(gb.data(), int64_t(gb.size()), nullptr, &sinfo) == COOC_ERR_ARG, "NULL info passed", 0);
  expect(cooc_sampling_snapshot_inspect(gb.data(), int64_t(gb.size()), &info, nullptr) == COOC_ERR_ARG, "NULL sinfo passed", 0);

  if (n_fail) {
    std::fprintf(stderr, "sampled_snapshot_fuzz: %d failures\n", n_fail);
    return 1;
  }
  std::printf("sampled_snapshot_fuzz ok: %lld cases\n", n_cases);
  return 0;
}
