// cooc_owned.hip — one window of the multi-GPU job inside the library (cooc_count_owned, cooc_topk_owned): the
// reference's keyBy(user) / keyBy(ItemCooccurrences::getItem) / broadcast() exchanges
// (FlinkCooccurrences.java:70,152,163) as collectives of the context's communicator (cooc_comm.h: RCCL over
// xGMI, or caller operations).  n_items >= 40,320: the histories all-gathered around the owned-rows count of
// cooc_sparse.hip (count_owned).  Below: the pair records routed to the rows' owners, a mod world, around the
// batch planner's shard_plan / shard_count (count_owned_records).
#include <algorithm>
#include <vector>

#include "cooc_comm.h"
#include "cooc_ctx.h"
#include "cooc_radix.h"
#include "cooc_stream_kernels.h"

using cooc::Status;

namespace {

constexpr int32_t kSnakeHead = 4096;  // rows placed greedily (sharding.snake_owner's head)

__global__ void k_iota(int32_t *v, int32_t n) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// owner[order[i]]: the head's greedy ranks, then the snake over the ranks sorted by load
__global__ void k_owner_assign(const int32_t *__restrict__ order, int32_t M, int32_t h,
                               const int32_t *__restrict__ head_owner, const int32_t *__restrict__ rank_by_load,
                               int32_t world, int32_t *__restrict__ owner) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  int32_t o;
  if (i < h) {
    o = head_owner[i];
  } else {
    const int64_t pos = int64_t(i) - h, lap = pos / world, r = pos % world;
    o = rank_by_load[(lap & 1) == 0 ? r : world - 1 - r];
  }
  owner[order[i]] = o;
}

__global__ void k_lengths(const int64_t *__restrict__ up, int64_t U, int64_t *__restrict__ lens) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < U) lens[j] = up[j + 1] - up[j];
}

// The owned rows of the records exchange as item-indexed views: item a = part + r * W takes row r of the compact
// R-row result (its col / cnt are shared, not copied), every other item is empty at a valid base; and the owner map
// a mod W.
__global__ void k_own_expand(int32_t M, int32_t W, int32_t part, const int64_t *__restrict__ c_base,
                             const int32_t *__restrict__ c_nnz, const int64_t *__restrict__ c_rowsum,
                             int64_t *__restrict__ row_base, int32_t *__restrict__ row_nnz,
                             int64_t *__restrict__ rowsum, int32_t *__restrict__ owner) {
  const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= M) return;
  const int32_t o = a % W, r = a / W;
  const int32_t n = o == part ? c_nnz[r] : 0;
  row_base[a] = n > 0 ? c_base[r] : 0;
  row_nnz[a] = n;
  rowsum[a] = o == part ? c_rowsum[r] : 0;
  owner[a] = o;
}

__global__ void k_own_widen(const int32_t *__restrict__ v, int32_t n, int64_t *__restrict__ out) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = int64_t(v[i]);
}

__global__ void k_own_fill_u16(uint16_t *__restrict__ p, int64_t n, uint16_t v) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// the first interaction whose item lies outside [0, M) (*first starts at ~0)
__global__ void k_own_first_bad(const int32_t *__restrict__ items, int64_t n, int32_t M,
                                unsigned long long *__restrict__ first) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n && (items[i] < 0 || items[i] >= M)) atomicMin(first, (unsigned long long)i);
}

inline unsigned nblk(int64_t n, int t) { return unsigned(std::max<int64_t>(1, (n + t - 1) / t)); }

}  // namespace

Status cooc_ctx::count_owned(int64_t n_users, const int64_t *d_up, const int32_t *d_items, int64_t n, hipStream_t s,
                             cooc_owned_info *info, cooc_device_result *out) {
  if (!comm) return Status{COOC_ERR_STATE, "cooc_count_owned needs a communicator (cooc_comm_init)"};
  if (counter.batch_ok()) return count_owned_records(n_users, d_up, d_items, n, s, info, out, Status::Ok());
  COOC_HIP_TRY(hipSetDevice(device));
  cooc::Comm &C = *comm;
  const int32_t M = cfg.n_items, W = C.world(), me = C.rank();
  // (1) global item frequencies
  COOC_TRY(own_counts.reserve(sizeof(int64_t) * size_t(M)));
  int64_t *counts = own_counts.as<int64_t>();
  COOC_TRY(cooc::launch_item_counts(s, d_items, n, M, counts));
  COOC_TRY(C.allreduce_sum_i64(counts, M, s));
  // (2) owner map: rows by descending frequency (a stable radix sort: ties keep the smaller id first).  A count
  // is at most the job's interactions, fewer than 2^31 (checked below, once the sizes are gathered and before
  // the order is used): 31 key bits
  COOC_TRY(own_sort.reserve(sizeof(int64_t) * size_t(M) + 2 * sizeof(int32_t) * size_t(M)));
  uint64_t *skeys = own_sort.as<uint64_t>();
  int32_t *ids = reinterpret_cast<int32_t *>(skeys + M), *order = ids + M;
  k_iota<<<nblk(M, 256), 256, 0, s>>>(ids, M);
  COOC_TRY(own_tmp.reserve(cooc::radix_sort_tmp_bytes<uint64_t, int32_t>(M)));
  COOC_TRY((cooc::radix_sort_pairs<uint64_t, int32_t>(reinterpret_cast<const uint64_t *>(counts), ids, skeys, order, M,
                                                      0, 31, true, own_tmp.p, s)));
  const int32_t h = std::min(kSnakeHead, M);
  std::vector<int64_t> head_counts(size_t(h) + 1);
  COOC_HIP_TRY(hipMemcpyAsync(head_counts.data(), skeys, sizeof(int64_t) * size_t(h), hipMemcpyDeviceToHost, s));
  // sizes of every rank's part, gathered in the same sync
  COOC_TRY(own_sizes.reserve(sizeof(int64_t) * size_t(2 + 2 * W)));
  int64_t *d_sz = own_sizes.as<int64_t>();
  const int64_t my_sz[2] = {n_users, n};
  COOC_HIP_TRY(hipMemcpyAsync(d_sz, my_sz, sizeof(my_sz), hipMemcpyHostToDevice, s));
  COOC_TRY(C.allgather(d_sz, d_sz + 2, 2 * sizeof(int64_t), s));
  std::vector<int64_t> sz(static_cast<size_t>(2 * W));
  COOC_HIP_TRY(hipMemcpyAsync(sz.data(), d_sz + 2, sizeof(int64_t) * size_t(2 * W), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  std::vector<int32_t> head_owner(size_t(h) + 1);
  std::vector<int32_t> rank_by_load(static_cast<size_t>(W));
  cooc::snake_head(head_counts.data(), h, W, head_owner.data(), rank_by_load.data());
  COOC_TRY(own_owner.reserve(sizeof(int32_t) * (size_t(M) + size_t(h) + size_t(W))));
  int32_t *owner = own_owner.as<int32_t>(), *d_head = owner + M, *d_rbl = d_head + h;
  COOC_HIP_TRY(hipMemcpyAsync(d_head, head_owner.data(), sizeof(int32_t) * size_t(h), hipMemcpyHostToDevice, s));
  COOC_HIP_TRY(hipMemcpyAsync(d_rbl, rank_by_load.data(), sizeof(int32_t) * size_t(W), hipMemcpyHostToDevice, s));
  k_owner_assign<<<nblk(M, 256), 256, 0, s>>>(order, M, h, d_head, d_rbl, W, owner);
  COOC_HIP_TRY(hipGetLastError());
  // (3) the histories, all-gathered into one compact CSR (parts in rank order)
  int64_t U_all = 0, N_all = 0;
  const size_t Wn = static_cast<size_t>(W);
  std::vector<int64_t> u_off(Wn), n_off(Wn), u_bytes(Wn), n_bytes(Wn);
  for (int32_t r = 0; r < W; r++) {
    u_off[size_t(r)] = U_all * int64_t(sizeof(int64_t));
    n_off[size_t(r)] = N_all * int64_t(sizeof(int32_t));
    u_bytes[size_t(r)] = sz[size_t(2 * r)] * int64_t(sizeof(int64_t));
    n_bytes[size_t(r)] = sz[size_t(2 * r + 1)] * int64_t(sizeof(int32_t));
    U_all += sz[size_t(2 * r)];
    N_all += sz[size_t(2 * r + 1)];
  }
  if (sz[size_t(2 * me)] != n_users || sz[size_t(2 * me + 1)] != n)
    return Status{COOC_ERR_STATE, "cooc_count_owned: the gathered sizes disagree with this rank's part"};
  if (N_all > int64_t(INT32_MAX)) return Status{COOC_ERR_ARG, "more than 2^31 interactions in one window"};
  COOC_TRY(own_lens.reserve(sizeof(int64_t) * size_t(std::max<int64_t>(1, n_users + U_all))));
  int64_t *lens = own_lens.as<int64_t>(), *lens_all = lens + n_users;
  COOC_TRY(own_up.reserve(sizeof(int64_t) * size_t(U_all + 1)));
  COOC_TRY(own_items.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(1, N_all))));
  int64_t *up_all = own_up.as<int64_t>();
  int32_t *it_all = own_items.as<int32_t>();
  if (n_users > 0) k_lengths<<<nblk(n_users, 256), 256, 0, s>>>(d_up, n_users, lens);
  const std::vector<int64_t> zero(Wn, 0), my_u(Wn, n_users * int64_t(sizeof(int64_t))),
      my_n(Wn, n * int64_t(sizeof(int32_t)));
  // every rank sends its whole part to every peer (send offsets all 0); the parts land compact, in rank order
  COOC_TRY(C.alltoallv(lens, zero.data(), my_u.data(), lens_all, u_off.data(), u_bytes.data(), s));
  COOC_TRY(C.alltoallv(d_items, zero.data(), my_n.data(), it_all, n_off.data(), n_bytes.data(), s));
  COOC_HIP_TRY(hipMemsetAsync(up_all, 0, sizeof(int64_t), s));
  // the gathered lengths' prefix (cooc_scan.h; own_tmp holds the tile statuses and, after them, the error word)
  const int64_t scan_words = cooc::scan_state_words(std::max<int64_t>(U_all, 1));
  COOC_TRY(own_tmp.reserve(sizeof(unsigned long long) * size_t(scan_words + 1)));
  int64_t *scan_err = reinterpret_cast<int64_t *>(own_tmp.as<unsigned long long>() + scan_words);
  COOC_HIP_TRY(hipMemsetAsync(scan_err, 0, sizeof(int64_t), s));
  COOC_TRY(cooc::launch_scan<true>(cooc::ScanI64{lens_all}, up_all + 1, U_all, own_tmp.as<unsigned long long>(), scan_err, s));
  int64_t h_scan_err = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&h_scan_err, scan_err, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  // (4) the owned rows over every user
  COOC_TRY(count_device_owned(U_all, up_all, it_all, N_all, owner, me, counts, N_all, s, out));
  // (5) the job's ordered pairs
  COOC_TRY(own_obs.reserve(sizeof(int64_t)));
  int64_t obs = out->observed;
  COOC_HIP_TRY(hipMemcpyAsync(own_obs.p, &obs, sizeof(int64_t), hipMemcpyHostToDevice, s));
  COOC_TRY(C.allreduce_sum_i64(own_obs.as<int64_t>(), 1, s));
  int64_t obs_all = 0;
  COOC_HIP_TRY(hipMemcpyAsync(&obs_all, own_obs.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  COOC_HIP_TRY(hipStreamSynchronize(s));
  if (h_scan_err & 8) return Status{COOC_ERR_STATE, "internal bounds check failed (gathered history prefix)"};
  info->part = me;
  info->n_parts = W;
  info->observed = obs_all;
  info->local_observed = out->observed;
  info->n_users_all = U_all;
  info->n_interactions_all = N_all;
  info->gathered_bytes = int64_t(sizeof(int32_t)) * (N_all - n) + int64_t(sizeof(int64_t)) * (U_all - n_users);
  info->owner = owner;
  info->item_counts = counts;
  return Status::Ok();
}

// One window below 40,320 items (sharding.count_records inside the library).  Every rank plans its own users'
// records (shard_plan), the ranks agree on one record each before any payload moves, then the u16 arenas are
// all-gathered and the row counts and 8-B descriptors go to the rows' owners (a mod world), which count complete rows
// (shard_count, always a padded CSR) and install them as the batch result through item-indexed views.
Status cooc_ctx::count_owned_records(int64_t n_users, const int64_t *d_up, const int32_t *d_items, int64_t n,
                                     hipStream_t s, cooc_owned_info *info, cooc_device_result *out,
                                     const Status &pre) {
  if (!comm) return Status{COOC_ERR_STATE, "cooc_count_owned needs a communicator (cooc_comm_init)"};
  COOC_HIP_TRY(hipSetDevice(device));
  cooc::Comm &C = *comm;
  const int32_t M = cfg.n_items, W = C.world(), me = C.rank();
  const size_t Wn = static_cast<size_t>(W);
  have_batch = false;
  batch_topk = 0;
  // (1) the local plan.  The agreement's record: status, users, interactions after the cut, arena ids, ordered
  // pairs, then the descriptors bound for every owner
  constexpr int kH = 5;
  const size_t F = kH + Wn;
  std::vector<int64_t> mine(F, 0);
  int64_t n_cut = n;
  auto plan = [&]() -> Status {
    COOC_TRY(pre);
    if (n_users < 0 || n < 0 || (n_users == 0 && n > 0) || (n_users > 0 && (!d_up || (n > 0 && !d_items))))
      return Status{COOC_ERR_ARG, "bad CSR arguments"};
    if (n_users > 0) COOC_TRY(apply_user_cut(n_users, &d_up, &d_items, &n_cut, s));
    const int64_t cap = (n_cut + 7 * std::max<int64_t>(n_users, 1) + 16 + 7) / 8 * 8;
    COOC_TRY(rec_desc.reserve(sizeof(uint64_t) * size_t(n_cut + 1)));
    COOC_TRY(rec_rc.reserve(sizeof(int32_t) * size_t(M)));
    COOC_TRY(rec_arena.reserve(sizeof(uint16_t) * size_t(cap)));
    const Status st = counter.shard_plan(n_users, d_up, d_items, n_cut, W, s, rec_desc.as<uint64_t>(),
                                         rec_rc.as<int32_t>(), rec_arena.as<uint16_t>(), cap, &mine[kH], &mine[3],
                                         &mine[4]);
    if (st.code == COOC_ERR_ARG && n_cut > 0) {  // an item id out of range: the message names the first one
      COOC_TRY(rec_agree.reserve(sizeof(int64_t)));
      unsigned long long *d_first = rec_agree.as<unsigned long long>(), first = 0;
      COOC_HIP_TRY(hipMemsetAsync(d_first, 0xff, sizeof(first), s));
      k_own_first_bad<<<nblk(n_cut, 256), 256, 0, s>>>(d_items, n_cut, M, d_first);
      COOC_HIP_TRY(hipGetLastError());
      COOC_HIP_TRY(hipMemcpyAsync(&first, d_first, sizeof(first), hipMemcpyDeviceToHost, s));
      COOC_HIP_TRY(hipStreamSynchronize(s));
      if (first < (unsigned long long)n_cut) {
        int32_t id = 0;
        COOC_HIP_TRY(hipMemcpy(&id, d_items + first, sizeof(id), hipMemcpyDeviceToHost));
        return Status{COOC_ERR_ARG, "cooc_count_owned: interaction " + std::to_string(first) + ": item " +
                                        std::to_string(id) + " (of " + std::to_string(M) + ")"};
      }
    }
    COOC_TRY(st);
    mine[1] = n_users;
    mine[2] = n_cut;
    return Status::Ok();
  };
  const Status local = plan();
  mine[0] = local.code;
  if (!local.ok()) std::fill(mine.begin() + 1, mine.end(), 0);
  // (2) the agreement, before any payload moves (cooc_sample_owned's scheme): one all-gather of the records
  std::vector<int64_t> all(F * Wn, 0);
  auto exchange = [&]() -> Status {
    COOC_TRY(rec_agree.reserve(sizeof(int64_t) * F * (Wn + 1)));
    int64_t *d = rec_agree.as<int64_t>();
    COOC_HIP_TRY(hipMemcpyAsync(d + F * Wn, mine.data(), sizeof(int64_t) * F, hipMemcpyHostToDevice, s));
    COOC_TRY(C.allgather(d + F * Wn, d, int64_t(sizeof(int64_t) * F), s));
    COOC_HIP_TRY(hipMemcpyAsync(all.data(), d, sizeof(int64_t) * F * Wn, hipMemcpyDeviceToHost, s));
    COOC_HIP_TRY(hipStreamSynchronize(s));
    return Status::Ok();
  };
  const Status x = exchange();
  if (!local.ok()) return local;
  COOC_TRY(x);
  for (int32_t q = 0; q < W; q++)
    if (all[size_t(q) * F] != 0)
      return Status{COOC_ERR_ARG, "cooc_count_owned: rank " + std::to_string(q) + " failed its checks (status " +
                                      std::to_string(all[size_t(q) * F]) + "); no rank counted"};
  if (!std::equal(mine.begin(), mine.end(), all.begin() + size_t(me) * F))
    return Status{COOC_ERR_STATE, "cooc_count_owned: the gathered records disagree with this rank's plan"};
  auto send = [&](int32_t src, int32_t o) { return all[size_t(src) * F + kH + size_t(o)]; };
  int64_t U_all = 0, N_all = 0, obs_all = 0, ids_max = 0, n_recv = 0;
  for (int32_t q = 0; q < W; q++) {
    const int64_t *v = &all[size_t(q) * F];
    U_all += v[1], N_all += v[2], obs_all += v[4];
    ids_max = std::max(ids_max, v[3]);
  }
  // (shard_count takes fewer than 2^31 descriptors per owner: checked on the gathered matrix, so all ranks fail alike)
  for (int32_t o = 0; o < W; o++) {
    int64_t col = 0;
    for (int32_t q = 0; q < W; q++) col += send(q, o);
    if (col > int64_t(INT32_MAX))
      return Status{COOC_ERR_ARG, "cooc_count_owned: " + std::to_string(col) + " pair records for the rows of rank " +
                                      std::to_string(o) + ", more than 2^31 - 1; no rank counted"};
    if (o == me) n_recv = col;
  }
  // (7) the job's item frequencies: the planner's local row counts widened, all-reduced (before shard_count
  // reuses the planner's array)
  COOC_TRY(own_counts.reserve(sizeof(int64_t) * size_t(M)));
  int64_t *counts = own_counts.as<int64_t>();
  k_own_widen<<<nblk(M, 256), 256, 0, s>>>(counter.plan_row_counts(), M, counts);
  COOC_HIP_TRY(hipGetLastError());
  COOC_TRY(C.allreduce_sum_i64(counts, M, s));
  // (3) the arenas, one slot of `stride` ids per rank: the largest rank's ids and one pad group (a 16-B load that
  // starts at a list's last group never leaves its slot).  This rank's ids are copied into the send slot behind the
  // gathered ones and padded there with the sink id M: the stride is known only after the plan
  const int64_t stride = ids_max + 8, my_ids = mine[3];
  COOC_TRY(rec_arena_all.reserve(sizeof(uint16_t) * size_t(stride) * (Wn + 1)));
  uint16_t *arena_all = rec_arena_all.as<uint16_t>(), *slot = arena_all + size_t(stride) * Wn;
  if (my_ids > 0)
    COOC_HIP_TRY(hipMemcpyAsync(slot, rec_arena.p, sizeof(uint16_t) * size_t(my_ids), hipMemcpyDeviceToDevice, s));
  k_own_fill_u16<<<nblk(stride - my_ids, 256), 256, 0, s>>>(slot + my_ids, stride - my_ids, uint16_t(M));
  COOC_HIP_TRY(hipGetLastError());
  COOC_TRY(C.allgather(slot, arena_all, stride * int64_t(sizeof(uint16_t)), s));
  // (4) row counts and descriptors to their owners; every size from the gathered matrix
  auto rows_of = [&](int32_t o) { return o < M ? (M - o + W - 1) / W : 0; };
  const int32_t R = rows_of(me);
  std::vector<int64_t> so(Wn), sb(Wn), ro(Wn), rb(Wn);
  int64_t rows_before = 0;
  for (int32_t o = 0; o < W; o++) {
    so[size_t(o)] = rows_before * int64_t(sizeof(int32_t));
    sb[size_t(o)] = int64_t(rows_of(o)) * int64_t(sizeof(int32_t));
    ro[size_t(o)] = int64_t(o) * R * int64_t(sizeof(int32_t));
    rb[size_t(o)] = int64_t(R) * int64_t(sizeof(int32_t));
    rows_before += rows_of(o);
  }
  COOC_TRY(rec_rrc.reserve(sizeof(int32_t) * size_t(std::max<int64_t>(1, int64_t(W) * R))));
  COOC_TRY(C.alltoallv(rec_rc.p, so.data(), sb.data(), rec_rrc.p, ro.data(), rb.data(), s));
  int64_t sent = 0, got = 0;
  for (int32_t o = 0; o < W; o++) {
    so[size_t(o)] = sent * int64_t(sizeof(uint64_t));
    sb[size_t(o)] = send(me, o) * int64_t(sizeof(uint64_t));
    ro[size_t(o)] = got * int64_t(sizeof(uint64_t));
    rb[size_t(o)] = send(o, me) * int64_t(sizeof(uint64_t));
    sent += send(me, o);
    got += send(o, me);
  }
  COOC_TRY(rec_rdesc.reserve(sizeof(uint64_t) * size_t(std::max<int64_t>(1, n_recv))));
  COOC_TRY(C.alltoallv(rec_desc.p, so.data(), sb.data(), rec_rdesc.p, ro.data(), rb.data(), s));
  // (5) the owned rows, complete, as a padded CSR of R rows
  cooc::CountResult r;
  COOC_TRY(counter.shard_count(W, me, rec_rrc.as<int32_t>(), rec_rdesc.as<uint64_t>(), n_recv, arena_all, stride, s, &r,
                               timer.enabled ? &timer : nullptr, true));
  // (6) the item-indexed views and the owner map
  COOC_TRY(rec_base.reserve(sizeof(int64_t) * size_t(M)));
  COOC_TRY(rec_nnz.reserve(sizeof(int32_t) * size_t(M)));
  COOC_TRY(rec_rs.reserve(sizeof(int64_t) * size_t(M)));
  COOC_TRY(own_owner.reserve(sizeof(int32_t) * size_t(M)));
  k_own_expand<<<nblk(M, 256), 256, 0, s>>>(M, W, me, r.row_base, r.row_nnz, r.rowsum, rec_base.as<int64_t>(),
                                            rec_nnz.as<int32_t>(), rec_rs.as<int64_t>(), own_owner.as<int32_t>());
  COOC_HIP_TRY(hipGetLastError());
  // (8) the batch result: the counter's totals and error bits, then the views in place of its R-row arrays
  COOC_TRY(finish_batch(r, s, out));
  out->row_base = batch_result.row_base = rec_base.as<int64_t>();
  out->row_nnz = batch_result.row_nnz = rec_nnz.as<int32_t>();
  out->rowsum = batch_result.rowsum = rec_rs.as<int64_t>();
  batch_expanded = true;
  batch_owned = true;
  // (9) (the owned rows' pairs are their row sums' total: every received record adds its list less itself)
  info->part = me;
  info->n_parts = W;
  info->observed = obs_all;
  info->local_observed = out->observed;
  info->n_users_all = U_all;
  info->n_interactions_all = N_all;
  info->gathered_bytes = int64_t(W - 1) * (stride * int64_t(sizeof(uint16_t)) + int64_t(R) * int64_t(sizeof(int32_t))) +
                         (n_recv - send(me, me)) * int64_t(sizeof(uint64_t));
  info->owner = own_owner.as<int32_t>();
  info->item_counts = counts;
  return Status::Ok();
}

Status cooc_ctx::topk_owned(int32_t topk, int32_t flags, int32_t *d_sizes, int32_t *d_values, double *d_scores,
                            int64_t *d_rowsum_global, hipStream_t s) {
  if (!comm) return Status{COOC_ERR_STATE, "cooc_topk_owned needs a communicator (cooc_comm_init)"};
  if (!have_batch) return Status{COOC_ERR_STATE, "no cooc_count_owned result on this context"};
  COOC_HIP_TRY(hipSetDevice(device));
  const int32_t M = cfg.n_items;
  COOC_TRY(own_rowsum.reserve(sizeof(int64_t) * size_t(M)));
  int64_t *rs = own_rowsum.as<int64_t>();
  COOC_HIP_TRY(hipMemcpyAsync(rs, batch_result.rowsum, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
  COOC_TRY(comm->allreduce_sum_i64(rs, M, s));
  if (d_rowsum_global)
    COOC_HIP_TRY(hipMemcpyAsync(d_rowsum_global, rs, sizeof(int64_t) * size_t(M), hipMemcpyDeviceToDevice, s));
  return topk_batch_device(topk, flags, rs, d_sizes, d_values, d_scores, s);
}
