// cooc_snapshot_impl.h — what the three device files of the checkpoint code share (private to them and to
// cooc_capi.cpp, which calls the Snapshotter's entry points):
//
//   cooc_snapshot_pack.hip      cooc_snapshot_prepare / _copy: the streaming state into one blob
//   cooc_snapshot_restore.hip   cooc_restore_begin .. _finish: one untrusted blob validated and installed
//   cooc_snapshot_rescale.hip   cooc_restore_begin_parts .. _finish_parts: all blobs of one checkpoint into another
//                               (rank, world)
//
// The blob's layout and its host-only header code are cooc_snapshot.h / cooc_snapshot.cpp.
#pragma once

#include <algorithm>
#include <cassert>
#include <map>
#include <type_traits>
#include <vector>

#include "cooc_ctx.h"
#include "cooc_snapshot.h"

namespace cooc {

inline unsigned blocks_for(int64_t n, int t) { return unsigned(std::max<int64_t>(1, (n + t - 1) / t)); }
inline unsigned wave_grid(int64_t n_waves) { return std::min<unsigned>(blocks_for(n_waves * 64, 256), 8192); }
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// ---- one typed view of a blob -----------------------------------------------------------------------------------
// A blob's header (host) and its image (device; Img = char while cooc_snapshot_prepare writes it).  Sections are
// named by their 1-based kind; at<T> is the section's array, T being its element type (cooc_snapshot.h), which
// is held against the directory entry.
template <class Img>
struct BlobViewT {
  const SnapHeader *h;
  Img *img;
  int64_t count(int kind) const { return h->sec[kind - 1].count; }
  int64_t bytes(int kind) const { return h->sec[kind - 1].bytes; }
  Img *raw(int kind) const { return img + h->sec[kind - 1].offset; }
  template <class T>
  auto at(int kind) const {
    using P = std::conditional_t<std::is_const<Img>::value, const T, T>;
    assert(int32_t(sizeof(T)) == h->sec[kind - 1].elem && "a snapshot section read as another element type");
    return reinterpret_cast<P *>(raw(kind));
  }
};
using BlobView = BlobViewT<const char>;
using BlobImage = BlobViewT<char>;

// ---- one way to carve scratch -----------------------------------------------------------------------------------
// Arrays back to back in one DevBuf, each starting 256-B aligned: take<T>(n) is the next array's place and
// `end` the bytes to reserve.  take_last leaves the layout's last array unpadded.
template <class T>
struct Carved {
  size_t off;
  T *in(const DevBuf &b) const { return reinterpret_cast<T *>(b.as<char>() + off); }
};
struct Carve {
  size_t end = 0;
  template <class T>
  Carved<T> take(size_t n) {
    const Carved<T> c{end};
    end += al256(sizeof(T) * n);
    return c;
  }
  template <class T>
  Carved<T> take_last(size_t n) {
    const Carved<T> c{end};
    end += sizeof(T) * n;
    return c;
  }
};

// ---- lists copied in pieces ---------------------------------------------------------------------------------------
// k_snap_copy_lists and k_snap_copy_parts move a list in pieces of kListChunk ids, one wave per piece.
constexpr int64_t kListChunk = 2048;
// chunk_pre[j] = pieces of the lists before j (host), from the lists' offsets
inline std::vector<int64_t> chunk_prefix(const std::vector<int64_t> &ptr) {
  std::vector<int64_t> pre(ptr.size(), 0);
  for (size_t j = 0; j + 1 < ptr.size(); j++) pre[j + 1] = pre[j] + (ptr[j + 1] - ptr[j] + kListChunk - 1) / kListChunk;
  return pre;
}

#if defined(__HIPCC__)
// Every checking kernel ORs `bit` into *err when an element fails, one atomic per workgroup.
__device__ inline void val_fold(bool bad, unsigned int *err, unsigned int bit) {
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0 && any) atomicOr(err, bit);
}
#endif

// ---- launch helpers that more than one file calls (cooc_snapshot_pack.hip) ----------------------------------------
// sums[k] (device, kSnapSectionsMax words) = the checksum of section k of the image, k < h.n_sections
Status launch_checksums(hipStream_t s, const void *img, const SnapHeader &h, unsigned long long *sums);
// The histories between a blob (d_ptr: their offsets on the device, n = aoff.size() lists back to back) and the
// arena (list j at aoff[j]): dst <- src, arena -> blob when to_packed, else blob -> arena.  chunk_pre =
// chunk_prefix of the offsets.  Both vectors are uploaded asynchronously into snap_tmp2: they must outlive the
// caller's next synchronisation of the stream.
Status launch_copy_lists(cooc_ctx &ctx, bool to_packed, const std::vector<int64_t> &chunk_pre,
                         const std::vector<int64_t> &aoff, const int64_t *d_ptr, const int32_t *src, int32_t *dst);

// the operator's buffered windows flattened in timestamp order: window k is ts[k], records [ptr[k], ptr[k + 1])
struct PendingWindows {
  std::vector<int64_t> ts, ptr;
  std::vector<int32_t> users, items;
};

// what a blob's directory is laid out from (the sampler's two only in format 2)
struct SnapCounts {
  int64_t users = 0, hist_items = 0, rows = 0, entries = 0, xsums = 0, pend_windows = 0, pend_records = 0;
  int64_t counted_items = 0, total_users = 0;
};

// the steps' own tables (defined by the file that uses them)
struct PackTables;
struct PackScratch;
struct PackedRows;
struct PartsJob;
struct RowTables;
struct KeptUser;

// The one place that reads and writes the private state of StreamState and Operator for a checkpoint.
struct Snapshotter {
  // ---- cooc_snapshot_pack.hip
  static Status prepare(cooc_ctx &ctx, cooc_snapshot_info *info);
  static Status copy(cooc_ctx &ctx, int64_t offset, int64_t n, uint8_t *out);
  // ---- cooc_snapshot_restore.hip
  static Status restore_begin(cooc_ctx &ctx, int64_t bytes);
  static Status restore_write(cooc_ctx &ctx, int64_t offset, int64_t n, const uint8_t *src);
  static Status restore_finish(cooc_ctx &ctx, cooc_snapshot_info *info);
  // ---- cooc_snapshot_rescale.hip
  static Status restore_begin_parts(cooc_ctx &ctx, int32_t n_parts, const int64_t *bytes);
  static Status restore_write_part(cooc_ctx &ctx, int32_t part, int64_t offset, int64_t n, const uint8_t *src);
  static Status restore_finish_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info);

  // one validated blob: its header and the sections that become host state
  struct Parsed {
    SnapHeader h;
    std::vector<int64_t> scalars, hist_ptr;
    std::vector<int32_t> user_ids;
    PendingWindows pend;
    // format 2: the sampler's scalars, the users with a total and their totals, the counted items and counters
    std::vector<int64_t> smp_scalars;
    std::vector<int32_t> tot_ids, totals, cnt_ids;
    std::vector<int16_t> cnts;
  };

 private:
  // the blob format of this context: 2 when sampled, else 1
  static int32_t format_of(const cooc_ctx &ctx) { return ctx.stream_state.sampled() ? kSnapFormatSampled : kSnapFormat; }
  // The header of the blob that cooc_snapshot_prepare makes of this context with these counts: the directory laid
  // out, the configuration and (rank, world) set; sums and seal are the caller's.
  static SnapHeader header_for(const cooc_ctx &ctx, const SnapCounts &c);
  static PendingWindows flatten(const std::map<int64_t, Operator::Pending> &pending);

  // ---- the steps of prepare (cooc_snapshot_pack.hip)
  static PackTables host_tables(const cooc_ctx &ctx);
  static Status pack_global_rows(cooc_ctx &ctx, const PackScratch &sc, PackedRows *out);
  static Status count_sampler_items(cooc_ctx &ctx, const PackScratch &sc, int64_t *n_cnt);
  static Status host_scalars(cooc_ctx &ctx, int64_t *scalars);
  static Status put_sampler_sections(cooc_ctx &ctx, const BlobImage &v, const PackTables &t, const PackScratch &sc,
                                     int64_t *smp);
  static Status put_row_sections(cooc_ctx &ctx, const BlobImage &v, const PackedRows &g, const PackScratch &sc);
  static Status seal(cooc_ctx &ctx, SnapHeader *h);

  // ---- restore (cooc_snapshot_restore.hip); the parts path validates every part with validate and installs with
  //      the pieces below
  static bool empty_state(const cooc_ctx &ctx);
  static void wipe(cooc_ctx &ctx);
  static void drop_restore(cooc_ctx &ctx);
  static Status reset_samplers(cooc_ctx &ctx);
  static Status validate(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, Parsed *out);
  static Status parse_header(cooc_ctx &ctx, const char *img, int64_t bytes, bool own_rank, SnapHeader *h);
  static Status check_checksums(cooc_ctx &ctx, const BlobView &v, unsigned long long *d_sums);
  static Status check_sampler_scalars(cooc_ctx &ctx, const BlobView &v, Parsed *out);
  static Status download_host_sections(cooc_ctx &ctx, const BlobView &v, Parsed *out);
  static Status install(cooc_ctx &ctx, const char *img, const Parsed &p);
  static Status install_rows(cooc_ctx &ctx, const BlobView &v, const Parsed &p);
  static Status install_samplers(cooc_ctx &ctx, const BlobView &v, const Parsed &p);
  static Status lay_out_slabs(cooc_ctx &ctx, int64_t nnz);
  static Status lay_out_histories(cooc_ctx &ctx, const std::vector<int64_t> &lens, std::vector<int64_t> *aoff);
  static void set_slots(StreamState &st, const std::vector<int32_t> &user_ids, const std::vector<int64_t> &lens,
                        const std::vector<int64_t> &aoff);
  static Status upload_running_totals(cooc_ctx &ctx, int64_t scal2, int64_t scal3);
  static void set_operator(cooc_ctx &ctx, const int64_t *scalars, const PendingWindows &pend);

  // ---- the steps of restore_finish_parts (cooc_snapshot_rescale.hip)
  static Status validate_and_install_parts(cooc_ctx &ctx, const cooc_user_route *route, cooc_snapshot_info *info);
  static Status validate_parts(cooc_ctx &ctx, PartsJob *job);
  static PendingWindows pending_union(const PartsJob &job);
  static Status install_rows_parts(cooc_ctx &ctx, const PartsJob &job, const RowTables &t, unsigned long long *tot);
  static Status install_histories_parts(cooc_ctx &ctx, const PartsJob &job, const RowTables &t,
                                        const std::vector<KeptUser> &kept, int64_t *hist_items);
};

}  // namespace cooc
