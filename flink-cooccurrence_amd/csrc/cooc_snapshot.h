// cooc_snapshot.h — layout of the snapshot blob (cooc_snapshot_prepare .. cooc_restore_finish),
// shared by the host-only header code (cooc_snapshot.cpp: no HIP, also built stand-alone under the host
// sanitizers) and the device side (cooc_snapshot_pack.hip, _restore.hip, _rescale.hip; cooc_snapshot_impl.h).
//
//   [header: 64 B][directory: n_sections x 40 B][sections, in directory order, each 8-B aligned, zero-padded]
//
// Little-endian.  The blob is canonical: the sections follow the directory back to back in kind order, so two
// contexts in the same logical state give the same bytes.
//
// Two formats share the container.  Format 1 ("COOCSNP1", 15 sections) is the unsampled streaming state.  Format 2
// ("COOCSMP2", 20 sections: the 15 of format 1 with their meaning, then the sampler's state) is a sampled
// context's (cooc_sampling_snapshot_prepare ..).  The two magics differ in two bytes by two bits each, so no
// single-bit flip turns one into the other, and each family of entry points rejects the other's blobs.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/cooc.h"

namespace cooc {

constexpr uint64_t kSnapMagic = 0x31504e53434f4f43ull;  // "COOCSNP1"
constexpr int32_t kSnapFormat = 1;
constexpr uint64_t kSnapMagicSampled = 0x32504d53434f4f43ull;  // "COOCSMP2"
constexpr int32_t kSnapFormatSampled = 2;

enum SnapKind : int32_t {
  kSnapScalars = 1,   // int64[kSnapScalarWords]: see SnapScalar
  kSnapUserIds,       // int32[n_users]: users with a resident history, ascending
  kSnapHistPtr,       // int64[n_users + 1]: their histories' offsets in kSnapHistItems
  kSnapHistItems,     // int32[history_items]: the histories back to back, each in arrival order
  kSnapRowIds,        // int32[global_rows]: items with a non-empty global row, ascending
  kSnapRowPtr,        // int64[global_rows + 1]
  kSnapRowCols,       // int32[global_entries]: ascending within a row
  kSnapRowCnts,       // uint32[global_entries]: exact counts (> 0)
  kSnapRowSums,       // int64[global_rows]: the rows' global row sums
  kSnapXsumIds,       // int32[n]: world > 1 only -- items whose row lives on another rank (ascending) ...
  kSnapXsumVals,      // int64[n]: ... and their (job-wide, non-zero) row sums
  kSnapPendTs,        // int64[pending_windows]: maxTimestamp of the operator's buffered windows, ascending
  kSnapPendPtr,       // int64[pending_windows + 1]: their records' offsets
  kSnapPendUsers,     // int32[pending_records]: the records in arrival order
  kSnapPendItems,     // int32[pending_records]
  kSnapKindEnd,
  // format 2 only: the sampler's state (cooc_sample.h).  The feedback queue is not state (it is applied at the end
  // of the window it arose in, and no snapshot is taken while a window is staged); stamps, window numbers and the
  // slot numbering are layout.
  kSnapSmpScalars = kSnapKindEnd,  // int64[kSnapSmpScalarWords]: see SnapSmpScalar
  kSnapSmpItemIds,    // int32[n]: items whose counter is non-zero, ascending
  kSnapSmpItemCnts,   // int16[n]: their counters, each in 1..item_cut
  kSnapSmpUserIds,    // int32[n]: users with userInteractionsTotal > 0, ascending: a superset of kSnapUserIds (a
                      // user whose every record was rejected at the item cut has a total and no reservoir)
  kSnapSmpTotals,     // int32[n]: their totals, each >= 1 and >= the user's history length
  kSnapSampledKindEnd
};
constexpr int kSnapSections = kSnapKindEnd - 1;
constexpr int kSnapSectionsSampled = kSnapSampledKindEnd - 1;
constexpr int kSnapSectionsMax = kSnapSectionsSampled;

enum SnapScalar : int {
  kScObservedExact = 0,
  kScObservedRef,
  kScRowsumAcc,
  kScRescoredItems,
  kScLateElements,
  kScWatermark,
  kScAgreed,
  kScRegather,
  kScScal2,  // d_scal_[2]: the rescorer's observed total (cumulative, read by the next window's rescoring)
  kScScal3,  // d_scal_[3]: the exact observed total (cumulative)
  kSnapScalarWords = 16  // (the rest zero)
};

enum SnapSmpScalar : int {
  kSsItemCut = 0,
  kSsSeed,
  kSsRejected,
  kSsFills,
  kSsReplacements,
  kSsFeedbacks,
  kSnapSmpScalarWords = 8  // (the rest zero)
};

struct SnapSection {
  int32_t kind;
  int32_t elem;     // bytes per element
  int64_t offset;   // from the start of the blob, a multiple of 8
  int64_t bytes;    // count * elem (the section occupies bytes rounded up to 8, the pad zero)
  int64_t count;
  uint64_t sum;     // sum over the section's 8-B words w_i of splitmix64(w_i ^ i), mod 2^64
};
static_assert(sizeof(SnapSection) == 40, "directory entry");

struct SnapHeader {
  uint64_t magic;
  int32_t format, n_sections;
  int64_t total_bytes;
  int32_t n_items, user_cut;
  int64_t window_size_ms;
  int32_t rank, world;
  uint64_t header_sum;  // the same sum over the header and directory words, this word taken as 0
  uint64_t reserved;
  SnapSection sec[kSnapSectionsMax];  // a blob holds the first n_sections of them
};
constexpr int64_t snap_header_bytes(int n_sections) { return 64 + int64_t(n_sections) * 40; }
constexpr int64_t kSnapHeaderBytes = snap_header_bytes(kSnapSections);
constexpr int64_t kSnapSampledHeaderBytes = snap_header_bytes(kSnapSectionsSampled);
static_assert(sizeof(SnapHeader) == snap_header_bytes(kSnapSectionsMax), "header + directory");
static_assert(kSnapHeaderBytes == COOC_SNAPSHOT_HEADER_BYTES, "include/cooc.h names the header's size");
static_assert(kSnapSampledHeaderBytes == COOC_SAMPLED_SNAPSHOT_HEADER_BYTES, "include/cooc.h names the header's size");
constexpr int snap_sections_of(int32_t format) { return format == kSnapFormatSampled ? kSnapSectionsSampled : kSnapSections; }
constexpr uint64_t snap_magic_of(int32_t format) { return format == kSnapFormatSampled ? kSnapMagicSampled : kSnapMagic; }

#if defined(__HIPCC__)
#define COOC_SNAP_HD __host__ __device__
#else
#define COOC_SNAP_HD
#endif
// the splitmix64 of cooc_verify_batch (include/cooc.h)
COOC_SNAP_HD inline uint64_t snap_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

inline int64_t snap_pad8(int64_t b) { return (b + 7) & ~int64_t(7); }
int32_t snap_elem_bytes(int32_t kind);
// Offsets and total of a blob of the given format from the sections' counts (kind, elem, bytes filled in), then
// the header's own checksum (after the sections' sums are set).
void snap_layout(SnapHeader *h, int32_t format = kSnapFormat);
void snap_seal(SnapHeader *h);
// The header and directory of a blob of n_bytes (untrusted) that must be of the given format: COOC_OK and *h (the
// directory entries past the format's own zero), or COOC_ERR_ARG and *why.  Reads at most the format's header
// bytes of p.
int snap_parse(const uint8_t *p, int64_t n_bytes, SnapHeader *h, std::string *why, int32_t format = kSnapFormat);
void snap_info(const SnapHeader &h, cooc_snapshot_info *info);
// Format 2: the host checks of the sampler's scalars (item_cut in 1..32767, counters >= 0, the zero words zero),
// and what cooc_sampling_snapshot_inspect reports of them and of the directory.
int snap_check_sampler_scalars(const int64_t *sc, std::string *why);
void snap_sampling_info(const SnapHeader &h, const int64_t *sc, cooc_sampling_snapshot_info *sinfo);

// Rescaling (cooc_restore_finish_parts): what the cross-part checks need of one part, each part having passed
// snap_parse and the host checks of its scalars and pending windows.
struct SnapPartHead {
  SnapHeader h;
  int64_t scalars[kSnapScalarWords];
  int64_t first_pending;  // the lowest maxTimestamp of its pending windows; INT64_MAX without one
};
// The checks across the parts of one checkpoint that need only headers and scalars: part i taken by rank i of
// n_parts with the configuration given, the job-wide scalars (kScObservedRef, kScScal2, kScScal3) equal, no
// collective step outstanding (kScRegather 0), no window pending at or below the part's watermark, with
// n_parts > 1 one watermark that is also every part's agreed one, and accumulators whose sums fit int64.
// COOC_OK and merged[] (the scalars of new rank 0: the accumulators summed, kScAgreed = the watermark,
// kScRegather 0), or COOC_ERR_ARG and *why.
int snap_check_parts(const SnapPartHead *parts, int64_t n_parts, int32_t n_items, int64_t window_size_ms,
                     int32_t user_cut, int64_t *merged, std::string *why);

}  // namespace cooc
