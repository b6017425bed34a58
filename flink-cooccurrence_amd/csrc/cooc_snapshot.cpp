// cooc_snapshot.cpp — the snapshot blob's header and directory, of both formats: building them, and parsing them
// from untrusted bytes (cooc_snapshot_inspect / cooc_sampling_snapshot_inspect, and the first step of
// cooc_restore_finish / cooc_sampling_restore_finish), and the checks across the parts of
// one checkpoint that need only headers and scalars (cooc_restore_finish_parts).  Host-only: no HIP, no context;
// also built stand-alone under the host sanitizers (tests/sanitize/snapshot_fuzz.cpp, snapshot_parts_fuzz.cpp).
#include "cooc_snapshot.h"

#include <cstring>

namespace cooc {

// cooc_capi.cpp: the message behind cooc_last_error(NULL).  Weak: absent from a stand-alone build.
void snap_set_error(const std::string &msg) __attribute__((weak));

int32_t snap_elem_bytes(int32_t kind) {
  switch (kind) {
    case kSnapScalars: case kSnapHistPtr: case kSnapRowPtr: case kSnapRowSums: case kSnapXsumVals: case kSnapPendTs:
    case kSnapPendPtr: case kSnapSmpScalars:
      return 8;
    case kSnapUserIds: case kSnapHistItems: case kSnapRowIds: case kSnapRowCols: case kSnapRowCnts: case kSnapXsumIds:
    case kSnapPendUsers: case kSnapPendItems: case kSnapSmpItemIds: case kSnapSmpUserIds: case kSnapSmpTotals:
      return 4;
    case kSnapSmpItemCnts:
      return 2;
    default:
      return 0;
  }
}

void snap_layout(SnapHeader *h, int32_t format) {
  const int n_sections = snap_sections_of(format);
  int64_t off = snap_header_bytes(n_sections);
  for (int i = 0; i < n_sections; i++) {
    SnapSection &s = h->sec[i];
    s.kind = i + 1;
    s.elem = snap_elem_bytes(s.kind);
    s.bytes = s.count * s.elem;
    s.offset = off;
    off += snap_pad8(s.bytes);
  }
  for (int i = n_sections; i < kSnapSectionsMax; i++) h->sec[i] = SnapSection{};
  h->magic = snap_magic_of(format);
  h->format = format;
  h->n_sections = n_sections;
  h->total_bytes = off;
  h->reserved = 0;
}

// over the header and the n_sections directory entries the blob holds (the caller has checked n_sections)
static uint64_t header_sum(const SnapHeader &h) {
  SnapHeader t = h;
  t.header_sum = 0;
  uint64_t w[sizeof(SnapHeader) / 8];
  std::memcpy(w, &t, sizeof(w));
  uint64_t sum = 0;
  for (uint64_t i = 0; i < uint64_t(snap_header_bytes(h.n_sections) / 8); i++) sum += snap_splitmix64(w[i] ^ i);
  return sum;
}

void snap_seal(SnapHeader *h) { h->header_sum = header_sum(*h); }

int snap_parse(const uint8_t *p, int64_t n_bytes, SnapHeader *h, std::string *why, int32_t format) {
  const int n_sections = snap_sections_of(format);
  const int64_t header_bytes = snap_header_bytes(n_sections);
  auto bad = [&](const char *m) {
    if (why) *why = std::string("snapshot blob: ") + m;
    return int(COOC_ERR_ARG);
  };
  if (!p || n_bytes < header_bytes) return bad("shorter than its header");
  std::memset(h, 0, sizeof(*h));
  std::memcpy(h, p, size_t(header_bytes));
  if (h->magic != snap_magic_of(format)) return bad("bad magic");
  if (h->format != format) return bad("unknown format version");
  if (h->n_sections != n_sections) return bad("unexpected section count");
  if (h->header_sum != header_sum(*h)) return bad("header checksum mismatch");
  if (h->total_bytes != n_bytes) return bad("its length is not the length it announces");
  if (h->reserved != 0) return bad("reserved field set");
  if (h->n_items < 1 || h->user_cut < 0 || h->user_cut > 32767 || h->window_size_ms < 1)
    return bad("bad configuration fields");
  if (h->world < 1 || h->rank < 0 || h->rank >= h->world) return bad("bad rank / world");
  int64_t off = header_bytes;
  for (int i = 0; i < n_sections; i++) {
    const SnapSection &s = h->sec[i];
    if (s.kind != i + 1 || s.elem != snap_elem_bytes(i + 1)) return bad("unexpected section kind");
    if (s.count < 0 || s.count > n_bytes / s.elem) return bad("section count out of range");  // (so count * elem fits)
    if (s.bytes != s.count * s.elem) return bad("section bytes are not count x element size");
    // sections back to back in directory order: aligned, inside the blob, no overlap, no gap
    if (s.offset != off) return bad("section offset out of place");
    const int64_t padded = snap_pad8(s.bytes);
    if (padded > n_bytes - off) return bad("section runs past the end");
    off += padded;
  }
  if (off != n_bytes) return bad("sections do not fill the blob");
  auto cnt = [&](int kind) { return h->sec[kind - 1].count; };
  if (cnt(kSnapScalars) != kSnapScalarWords) return bad("bad scalar section");
  if (cnt(kSnapHistPtr) != cnt(kSnapUserIds) + 1) return bad("history offsets do not match the users");
  if (cnt(kSnapRowPtr) != cnt(kSnapRowIds) + 1 || cnt(kSnapRowSums) != cnt(kSnapRowIds))
    return bad("row offsets / sums do not match the rows");
  if (cnt(kSnapRowCols) != cnt(kSnapRowCnts)) return bad("columns and counts differ in number");
  if (cnt(kSnapXsumIds) != cnt(kSnapXsumVals)) return bad("row-sum ids and values differ in number");
  if (cnt(kSnapPendPtr) != cnt(kSnapPendTs) + 1) return bad("pending offsets do not match the windows");
  if (cnt(kSnapPendUsers) != cnt(kSnapPendItems)) return bad("pending users and items differ in number");
  if (cnt(kSnapUserIds) > cnt(kSnapHistItems)) return bad("more users than history items");  // (no empty history)
  if (cnt(kSnapRowIds) > h->n_items || cnt(kSnapXsumIds) > h->n_items || cnt(kSnapRowIds) > cnt(kSnapRowCols))
    return bad("more rows than items or entries");
  if (cnt(kSnapPendTs) > cnt(kSnapPendUsers)) return bad("more pending windows than records");
  if (format == kSnapFormatSampled) {
    if (cnt(kSnapSmpScalars) != kSnapSmpScalarWords) return bad("bad sampler scalar section");
    if (cnt(kSnapSmpItemIds) != cnt(kSnapSmpItemCnts)) return bad("counted items and counters differ in number");
    if (cnt(kSnapSmpUserIds) != cnt(kSnapSmpTotals)) return bad("users with a total and totals differ in number");
    if (cnt(kSnapSmpUserIds) < cnt(kSnapUserIds)) return bad("more users with a history than with a total");
    if (cnt(kSnapSmpItemIds) > h->n_items) return bad("more counted items than items");
  }
  return COOC_OK;
}

int snap_check_sampler_scalars(const int64_t *sc, std::string *why) {
  auto bad = [&](const char *m) {
    if (why) *why = std::string("snapshot blob: ") + m;
    return int(COOC_ERR_ARG);
  };
  if (sc[kSsItemCut] < 1 || sc[kSsItemCut] > 32767) return bad("item_cut outside [1, 32767]");
  for (int k = kSsRejected; k <= kSsFeedbacks; k++)
    if (sc[k] < 0) return bad("a negative decision counter");
  for (int k = kSsFeedbacks + 1; k < kSnapSmpScalarWords; k++)
    if (sc[k] != 0) return bad("reserved sampler scalar set");
  return COOC_OK;
}

void snap_sampling_info(const SnapHeader &h, const int64_t *sc, cooc_sampling_snapshot_info *sinfo) {
  std::memset(sinfo, 0, sizeof(*sinfo));
  sinfo->item_cut = int32_t(sc[kSsItemCut]);
  sinfo->seed = sc[kSsSeed];
  sinfo->rejected = sc[kSsRejected];
  sinfo->fills = sc[kSsFills];
  sinfo->replacements = sc[kSsReplacements];
  sinfo->feedbacks = sc[kSsFeedbacks];
  sinfo->counted_items = h.sec[kSnapSmpItemIds - 1].count;
  sinfo->total_users = h.sec[kSnapSmpUserIds - 1].count;
}

void snap_info(const SnapHeader &h, cooc_snapshot_info *info) {
  std::memset(info, 0, sizeof(*info));
  info->bytes = h.total_bytes;
  info->n_users = h.sec[kSnapUserIds - 1].count;
  info->history_items = h.sec[kSnapHistItems - 1].count;
  info->global_rows = h.sec[kSnapRowIds - 1].count;
  info->global_entries = h.sec[kSnapRowCols - 1].count;
  info->pending_windows = h.sec[kSnapPendTs - 1].count;
  info->pending_records = h.sec[kSnapPendUsers - 1].count;
  info->format = h.format;
  info->rank = h.rank;
  info->world = h.world;
}

int snap_check_parts(const SnapPartHead *parts, int64_t n_parts, int32_t n_items, int64_t window_size_ms,
                     int32_t user_cut, int64_t *merged, std::string *why) {
  auto bad = [&](int64_t i, const char *m) {
    if (why) *why = "snapshot parts: part " + std::to_string(i) + ": " + m;
    return int(COOC_ERR_ARG);
  };
  if (!parts || !merged || n_parts < 1 || n_parts > int64_t(INT32_MAX)) {
    if (why) *why = "snapshot parts: the number of parts must be in [1, 2^31)";
    return int(COOC_ERR_ARG);
  }
  static const int kJobWide[] = {kScObservedRef, kScScal2, kScScal3};
  static const int kAdditive[] = {kScObservedExact, kScRowsumAcc, kScRescoredItems, kScLateElements};
  const int64_t *s0 = parts[0].scalars;
  for (int k = 0; k < kSnapScalarWords; k++) merged[k] = 0;
  for (int64_t i = 0; i < n_parts; i++) {
    const SnapHeader &h = parts[i].h;
    const int64_t *sc = parts[i].scalars;
    if (h.n_items != n_items || h.window_size_ms != window_size_ms || h.user_cut != user_cut)
      return bad(i, "taken with another n_items, window size or user_cut");
    if (int64_t(h.world) != n_parts) return bad(i, "its world is not the number of parts");
    if (int64_t(h.rank) != i) return bad(i, "not taken by the rank of its position");
    for (int k : kJobWide)
      if (sc[k] != s0[k]) return bad(i, "a job-wide total differs from part 0's");
    if (sc[kScRegather] != 0) return bad(i, "taken with a collective step outstanding");
    if (parts[i].first_pending <= sc[kScWatermark]) return bad(i, "a window pending at or below its watermark");
    if (n_parts > 1 && (sc[kScWatermark] != s0[kScWatermark] || sc[kScAgreed] != sc[kScWatermark]))
      return bad(i, "its watermark is not the job's agreed one");
    for (int k : kAdditive)
      if (__builtin_add_overflow(merged[k], sc[k], &merged[k])) return bad(i, "an accumulator's sum overflows");
  }
  // a part's row sums of other ranks are as many as the other parts' rows (their contents: the device pass)
  int64_t rows = 0;
  for (int64_t i = 0; i < n_parts; i++) {
    const int64_t r = parts[i].h.sec[kSnapRowIds - 1].count;
    if (r < 0 || r > n_items) return bad(i, "more rows than items");  // (so the sum fits: n_parts, n_items < 2^31)
    rows += r;
  }
  for (int64_t i = 0; i < n_parts; i++)
    if (parts[i].h.sec[kSnapXsumIds - 1].count != rows - parts[i].h.sec[kSnapRowIds - 1].count)
      return bad(i, "its row sums of other ranks are not as many as the other parts' rows");
  for (int k : kJobWide) merged[k] = s0[k];
  merged[kScWatermark] = merged[kScAgreed] = s0[kScWatermark];
  return COOC_OK;
}

}  // namespace cooc

extern "C" int cooc_snapshot_inspect(const uint8_t *bytes, int64_t n_bytes, cooc_snapshot_info *info) {
  std::string why;
  try {
    if (!info) {
      why = "cooc_snapshot_inspect: info is NULL";
    } else {
      cooc::SnapHeader h;
      if (cooc::snap_parse(bytes, n_bytes, &h, &why) == COOC_OK) {
        cooc::snap_info(h, info);
        return COOC_OK;
      }
    }
    if (cooc::snap_set_error) cooc::snap_set_error(why);
  } catch (...) {  // (std::string allocation: no exception crosses the C-ABI)
  }
  return COOC_ERR_ARG;
}

// The sampled format's header and directory, then its sampler scalars (section 16: inside the blob once the
// directory has passed), their checksum and their host checks.
extern "C" int cooc_sampling_snapshot_inspect(const uint8_t *bytes, int64_t n_bytes, cooc_snapshot_info *info,
                                              cooc_sampling_snapshot_info *sinfo) {
  std::string why;
  try {
    if (!info || !sinfo) {
      why = "cooc_sampling_snapshot_inspect: info or sinfo is NULL";
    } else {
      cooc::SnapHeader h;
      if (cooc::snap_parse(bytes, n_bytes, &h, &why, cooc::kSnapFormatSampled) == COOC_OK) {
        const cooc::SnapSection &sec = h.sec[cooc::kSnapSmpScalars - 1];
        int64_t sc[cooc::kSnapSmpScalarWords];
        std::memcpy(sc, bytes + sec.offset, sizeof(sc));
        uint64_t sum = 0;
        for (uint64_t i = 0; i < uint64_t(cooc::kSnapSmpScalarWords); i++) sum += cooc::snap_splitmix64(uint64_t(sc[i]) ^ i);
        if (sum != sec.sum) {
          why = "snapshot blob: checksum mismatch in section " + std::to_string(int(cooc::kSnapSmpScalars));
        } else if (cooc::snap_check_sampler_scalars(sc, &why) == COOC_OK) {
          cooc::snap_info(h, info);
          cooc::snap_sampling_info(h, sc, sinfo);
          return COOC_OK;
        }
      }
    }
    if (cooc::snap_set_error) cooc::snap_set_error(why);
  } catch (...) {  // (std::string allocation: no exception crosses the C-ABI)
  }
  return COOC_ERR_ARG;
}
