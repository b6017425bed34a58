"""Host-side mirror of the reference's operator interface over the C-ABI.

The reference (Java, Flink 1.3.2) cannot be built here, so the host side above the C-ABI mirrors its
operator surface with the same names, argument meaning and error behaviour:

* ``NonSampledUserInteractionCounterOneInputStreamOperator`` —
  NonSampledUserInteractionCounterOneInputStreamOperator.java:31-178 (constructor ``(windowSize,
  windowUnit)`` :61, ``processElement`` :84-110, ``onEventTime`` :113-165) fused with the two window
  aggregators it feeds (ItemRowAggregator.java:15-57, RowSumAggregator.java:15-72) and the rescorer
  (ItemRowRescorerTwoInputStreamOperator.java:22-246, constructor ``(short topK)`` :51-56).
  ``process_watermark`` returns the fired windows' outputs: per-window delta rows (the
  ``Tuple2<Integer, Int2ShortOpenHashMap>`` records), row-sum updates (``Tuple2<Integer,Integer>``)
  and the top-k queues (``Tuple2<Integer, IntDoublePriorityQueue>``).
* ``CooccurrenceCore`` — one C-ABI context: the stateless one-window batch (``count``,
  ``count_device``) and the streaming window API (``submit_batch`` / ``finish_window``).

Every compute call goes through libcooc_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (CoocCommOps, CoocConfig, CoocDeviceResult, CoocOwnedInfo, CoocWindowInfo, check, f64p, i16p, i32p,
                   i64p, u32p)

# Configuration.java:160-182 window units -> milliseconds (Time.of(size, unit).toMilliseconds())
_UNIT_MS = {"MILLISECONDS": 1, "SECONDS": 1000, "MINUTES": 60_000, "HOURS": 3_600_000, "DAYS": 86_400_000}


def window_size_ms(size: int, unit: str = "MILLISECONDS") -> int:
    u = unit.upper()
    if u not in _UNIT_MS:
        raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"Unrecognized window unit {unit}")  # :176-177
    return int(size) * _UNIT_MS[u]


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(t) if a is not None else None


def _stream_arg(stream, tensor):
    """The HIP stream a device-tensor entry point runs on: the caller's, else torch's current stream
    on the tensor's device, so that the library's kernels are ordered after the work that produced
    the inputs and before the work that consumes the outputs (cooc.h, stream contract)."""
    if stream is not None:
        return ctypes.c_void_p(int(stream))
    import torch

    if getattr(tensor, "is_cuda", False):
        return ctypes.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)
    return None


def _as_i64(v: int) -> int:
    """A seed given as an unsigned 64-bit value, as the signed int64 of the C-ABI."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


@dataclass
class BatchResult:
    """C of one window over empty histories, as a packed CSR over all n_items rows."""
    row_ptr: np.ndarray   # int64 [M+1]
    cols: np.ndarray      # int32 [nnz], ascending within a row
    cnt: np.ndarray       # uint32 [nnz] exact
    cnt16: np.ndarray     # int16 [nnz]   Int2ShortOpenHashMap view
    rowsum: np.ndarray    # int64 [M] exact
    rowsum32: np.ndarray  # int32 [M]     Java int view
    observed: int         # sum_u n_u (n_u - 1)


@dataclass
class WindowResult:
    """One fired window's observable outputs (same layout as oracle.WindowOutput)."""
    ts: int
    rows: np.ndarray
    row_ptr: np.ndarray
    cols: np.ndarray
    exact: np.ndarray
    v16: np.ndarray
    rs_items: np.ndarray
    rs_exact: np.ndarray
    rs_v32: np.ndarray
    observed: int
    topk_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    topk_sizes: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    topk_values: np.ndarray = field(default_factory=lambda: np.zeros((0, 0), np.int32))
    topk_scores: np.ndarray = field(default_factory=lambda: np.zeros((0, 0), np.float64))


@dataclass
class PreparedLog:
    """A log after the late drop, grouped by window and by user (cooc_log_prepare_device).  Device tensors trimmed to
    the kept records / users; the window lists on the host."""
    rec_user: object      # int32 [n_kept] dense user index of every kept record, in firing order
    rec_item: object      # int32 [n_kept] its item
    user_ids: object      # int32 [n_users] the id of every dense index, ascending
    user_ptr: object      # int64 [n_users + 1] } every user's kept items in firing order: a CSR for count_device
    user_items: object    # int32 [n_kept]      }
    window_ptr: np.ndarray  # int64 [n_windows + 1] into rec_user / rec_item
    window_ts: np.ndarray   # int64 [n_windows] the windows' maxTimestamp, ascending
    info: dict


class CooccurrenceCore:
    """One context of the C-ABI (one Flink subtask)."""

    def __init__(self, n_items: int, topk: int = 0, window_size_ms: int = 1000, device: int = -1,
                 exact_scores: bool = False, output: str = "auto", planner: str = "auto", user_cut: int = 0,
                 devices=None, subtask: int = 0, column_order: bool = False, any_order: bool = False,
                 item_cut: int = 0, sample_seed: int = 0, sample_on: str = "host"):
        """output: layout of count_device results: "auto", "csr" (padded CSR) or "dense" (n_items^2).
        planner: "auto" (the batch planner below 40,320 items, the large-universe planner above), "large"
        (the large-universe planner at any n_items; "general" is an alias) or "sort" (large, with every
        whole row through the sort + segmented-reduce path: packed 64-bit pair keys, radix sort, runs).
        user_cut: kMax, 0 = off; else only the first user_cut interactions of every user are expanded
        (UserInteractionCounter...java:168-205, the deterministic branch; later ones are dropped).
        item_cut: fMax, 0 = off; else the sampled streaming mode (cooc_sampling_enable): the item cut, user_cut
        as the size of a per-user reservoir, retractions when a slot is replaced; sample_seed seeds its
        counter-based draw.  Window counts are then signed (WindowResult.exact may be 0 or negative).
        sample_on: where the sampled mode decides a window's records: "host" (cooc_sampling_enable, record by
        record on the calling thread) or "device" (cooc_sampling_enable_device: the item counters, reservoir
        lengths and totals live on the GPU); the outputs are identical.
        column_order: COOC_FLAG_COLUMN_ORDER (device rows of the large-universe path in id order instead of the
        renumbered order: the batch's 16,384 most frequent items first, in id order, then the rest in id order;
        the renumbering is skipped when 15/16 of those hot items already have ids below 16,384).
        any_order: COOC_FLAG_ANY_ORDER (large-universe batch rows in no particular order: the LDS hash chunks skip
        their column ranking; host copies still come out sorted)."""
        L = _lib.load()
        flags = _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0
        if output not in ("auto", "csr", "dense"):
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"unknown output layout {output!r}")
        flags |= {"auto": 0, "csr": _lib.COOC_FLAG_OUTPUT_CSR, "dense": _lib.COOC_FLAG_OUTPUT_DENSE}[output]
        if planner not in ("auto", "general", "large", "sort"):
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"unknown planner {planner!r}")
        if sample_on not in ("host", "device"):
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"unknown sample_on {sample_on!r}")
        flags |= _lib.COOC_FLAG_GENERAL_PLANNER if planner != "auto" else 0
        flags |= _lib.COOC_FLAG_SORT_ROWS if planner == "sort" else 0
        flags |= _lib.COOC_FLAG_COLUMN_ORDER if column_order else 0
        flags |= _lib.COOC_FLAG_ANY_ORDER if any_order else 0
        cfg = CoocConfig(device, n_items, topk, flags, window_size_ms, user_cut, 0)
        h = ctypes.c_void_p()
        if devices is None:
            check(L.cooc_create(ctypes.byref(cfg), ctypes.byref(h)), None)
        else:  # create(cfg{devices[]}): this subtask's GPU is devices[subtask % len(devices)]
            devs = np.ascontiguousarray(devices, np.int32)
            check(L.cooc_create_on(ctypes.byref(cfg), _p(devs, i32p), len(devs), int(subtask), ctypes.byref(h)), None)
        self._h = h
        self.n_items = n_items
        self.topk = topk
        self.device = int(device) if devices is None else int(np.asarray(devices)[subtask % len(devices)])
        self.comm_world = 0  # > 0 once comm_init / comm_init_ops joined a communicator
        self.general_planner = planner != "auto"  # every window through the large-universe planner
        self.sampled = False
        if item_cut:
            try:
                enable = L.cooc_sampling_enable_device if sample_on == "device" else L.cooc_sampling_enable
                check(enable(self._h, int(item_cut), ctypes.c_int64(_as_i64(sample_seed))), self._h)
            except Exception:
                self.close()
                raise
            self.sampled = True

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().cooc_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- stateless one-window batch -------------------------------------------------------------
    def count_device(self, user_ptr, items, stream=None) -> CoocDeviceResult:
        """user_ptr: int64 device tensor [U+1] (user_ptr[0] == 0); items: int32 device tensor."""
        res = CoocDeviceResult()
        n_users = int(user_ptr.numel()) - 1
        check(_lib.load().cooc_count_device(self._h, n_users, ctypes.c_void_p(user_ptr.data_ptr()),
                                            ctypes.c_void_p(items.data_ptr()), int(items.numel()),
                                            _stream_arg(stream, items), ctypes.byref(res)), self._h)
        return res

    def item_counts(self, items, out=None, stream=None):
        """Item frequencies of a device int32 tensor -> int64 device tensor [n_items] (cooc_item_counts)."""
        import torch

        if out is None:
            out = torch.empty(self.n_items, dtype=torch.int64, device=items.device)
        check(_lib.load().cooc_item_counts(self._h, ctypes.c_void_p(items.data_ptr()) if items.numel() else None,
                                           int(items.numel()), ctypes.c_void_p(out.data_ptr()),
                                           _stream_arg(stream, out)), self._h)
        return out

    def count_device_owned(self, user_ptr, items, owner, part: int, item_counts, n_total: int,
                           stream=None) -> CoocDeviceResult:
        """Rows a with owner[a] == part over every user given (multi-GPU, n_items >= 40,320).
        owner: int32 device tensor [n_items]; item_counts: int64 device tensor [n_items] of the
        global log (n_total interactions)."""
        res = CoocDeviceResult()
        n_users = int(user_ptr.numel()) - 1
        check(_lib.load().cooc_count_device_owned(
            self._h, n_users, ctypes.c_void_p(user_ptr.data_ptr()), ctypes.c_void_p(items.data_ptr()),
            int(items.numel()), ctypes.c_void_p(owner.data_ptr()), int(part), ctypes.c_void_p(item_counts.data_ptr()),
            int(n_total), _stream_arg(stream, items), ctypes.byref(res)), self._h)
        return res

    def count(self, user_ptr, items) -> BatchResult:
        up = np.ascontiguousarray(user_ptr, np.int64)
        it = np.ascontiguousarray(items, np.int32)
        info = CoocWindowInfo()
        L = _lib.load()
        check(L.cooc_count_host(self._h, len(up) - 1, _p(up, i64p), _p(it, i32p), ctypes.byref(info)), self._h)
        return self.copy_batch(info.nnz, info.observed)

    def copy_batch(self, nnz: int, observed: int) -> BatchResult:
        M = self.n_items
        rp = np.zeros(M + 1, np.int64)
        cols = np.zeros(nnz, np.int32)
        cnt = np.zeros(nnz, np.uint32)
        cnt16 = np.zeros(nnz, np.int16)
        rs = np.zeros(M, np.int64)
        rs32 = np.zeros(M, np.int32)
        check(_lib.load().cooc_copy_batch(self._h, _p(rp, i64p), _p(cols, i32p), _p(cnt, u32p), _p(cnt16, i16p),
                                          _p(rs, i64p), _p(rs32, i32p)), self._h)
        return BatchResult(rp, cols, cnt, cnt16, rs, rs32, int(observed))

    def column_order(self) -> np.ndarray:
        """cooc_copy_column_order: the position of every column in the last batch's device row order (its
        top-k iteration order): the descending-frequency rank after the large-universe relabel, else the
        column id."""
        out = np.zeros(self.n_items, np.int32)
        check(_lib.load().cooc_copy_column_order(self._h, _p(out, i32p)), self._h)
        return out

    def topk_batch(self, topk: int, exact_scores: bool = False, stream=None):
        """LLR top-k of every row of the last batch -> (sizes [M], values [M, k], scores [M, k])."""
        L = _lib.load()
        check(L.cooc_topk_batch(self._h, topk, _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0,
                                None if stream is None else ctypes.c_void_p(int(stream))), self._h)
        M = self.n_items
        sizes = np.zeros(M, np.int32)
        vals = np.zeros((M, topk), np.int32)
        scores = np.zeros((M, topk), np.float64)
        check(L.cooc_copy_topk_batch(self._h, _p(sizes, i32p), _p(vals, i32p), _p(scores, f64p)), self._h)
        return sizes, vals, scores

    def topk_batch_device(self, topk: int, sizes, values, scores, rowsum_global=None, exact_scores: bool = False,
                          stream=None) -> None:
        """LLR top-k of every row of the last batch into device tensors (sizes int32 [M], values int32
        [M, k], scores float64 [M, k]) on torch's current stream.  rowsum_global (int64 device [M]):
        the all-reduced row sums of a multi-GPU run (rows not owned here come out with size 0)."""
        check(_lib.load().cooc_topk_batch_device(
            self._h, topk, _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0,
            None if rowsum_global is None else ctypes.c_void_p(rowsum_global.data_ptr()),
            ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
            _stream_arg(stream, sizes)), self._h)

    def llr(self, k4) -> np.ndarray:
        """LogLikelihood.logLikelihoodRatio of each (k11, k12, k21, k22) row, on the device."""
        k = np.ascontiguousarray(k4, np.int64).reshape(-1, 4)
        out = np.zeros(len(k), np.float64)
        check(_lib.load().cooc_llr(self._h, len(k), _p(k, i64p), _p(out, f64p)), self._h)
        return out

    def topk_items(self, items, k: int, exact_scores: bool = False):
        """topk(handle, items[], k) of SURVEY §8(b): the top-k of the given rows of the last batch ->
        (sizes [n], values [n, k], scores [n, k]), heap layout as topk_batch."""
        its = np.ascontiguousarray(items, np.int32)
        n = len(its)
        sizes = np.zeros(n, np.int32)
        vals = np.zeros((n, k), np.int32)
        scores = np.zeros((n, k), np.float64)
        check(_lib.load().cooc_topk_items(self._h, k, _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0, n,
                                          _p(its, i32p), _p(sizes, i32p), _p(vals, i32p), _p(scores, f64p)), self._h)
        return sizes, vals, scores

    # ---- sharding layer (owner-partitioned exchange of partial rows) -----------------------------
    def partition_plan(self, n_parts: int) -> np.ndarray:
        out = np.zeros(n_parts, np.int64)
        check(_lib.load().cooc_partition_plan(self._h, n_parts, _p(out, i64p)), self._h)
        return out

    def partition_pack(self, n_parts: int, row_nnz, entries, stream=None) -> None:
        """row_nnz: int32 device tensor [n_items]; entries: int64 device tensor [sum of the plan]."""
        check(_lib.load().cooc_partition_pack(self._h, n_parts, ctypes.c_void_p(row_nnz.data_ptr()),
                                              ctypes.c_void_p(entries.data_ptr()) if entries.numel() else None,
                                              _stream_arg(stream, row_nnz)), self._h)

    def copy_rowsum_device(self, rowsum, stream=None) -> None:
        check(_lib.load().cooc_copy_rowsum_device(self._h, ctypes.c_void_p(rowsum.data_ptr()),
                                                  _stream_arg(stream, rowsum)),
              self._h)

    def merge_partitions(self, n_parts: int, part: int, recv_row_nnz, recv_entries, rowsum_global=None,
                         stream=None, signed_nets: bool = False) -> CoocDeviceResult:
        """Owner `part`: the n_parts sources' partial rows (source-major device tensors; recv_entries may be None
        when every row is empty) merged into rows part + r * n_parts.  signed_nets: the counts are a sampled
        window's nets (cooc_selftest_merge, flags 1)."""
        res = CoocDeviceResult()
        L = _lib.load()
        args = (self._h, n_parts, part, ctypes.c_void_p(recv_row_nnz.data_ptr()),
                ctypes.c_void_p(recv_entries.data_ptr()) if recv_entries is not None and recv_entries.numel() else None,
                None if rowsum_global is None else ctypes.c_void_p(rowsum_global.data_ptr()))
        tail = (_stream_arg(stream, recv_row_nnz), ctypes.byref(res))
        check(L.cooc_selftest_merge(*args, 1, *tail) if signed_nets else L.cooc_merge_partitions(*args, *tail),
              self._h)
        return res

    # ---- sharded records (multi-GPU owner routing of pair records) -------------------------------
    @staticmethod
    def shard_arena_cap(n_users: int, n_interactions: int) -> int:
        """u16 arena ids cooc_shard_plan needs for a part (a multiple of 8)."""
        return (n_interactions + 7 * max(n_users, 1) + 16 + 7) // 8 * 8

    def shard_plan(self, user_ptr, items, n_parts: int, desc, row_counts, arena, stream=None):
        """This part's users -> desc (int64 device [n_interactions]), row_counts (int32 device
        [n_items], owner-major), arena (int16 device [>= shard_arena_cap]).  Returns (descriptors per
        owner (np.int64 [n_parts]), arena ids used, this part's ordered pairs)."""
        send = np.zeros(n_parts, np.int64)
        info = np.zeros(2, np.int64)
        n_users = int(user_ptr.numel()) - 1
        check(_lib.load().cooc_shard_plan(
            self._h, n_users, ctypes.c_void_p(user_ptr.data_ptr()), ctypes.c_void_p(items.data_ptr()),
            int(items.numel()), n_parts, ctypes.c_void_p(desc.data_ptr()) if desc.numel() else None,
            ctypes.c_void_p(row_counts.data_ptr()), ctypes.c_void_p(arena.data_ptr()), int(arena.numel()),
            _stream_arg(stream, items), _p(send, i64p), _p(info, i64p)), self._h)
        return send, int(info[0]), int(info[1])

    def shard_count(self, n_parts: int, part: int, recv_row_counts, recv_desc, arena_all, arena_stride: int,
                    stream=None) -> CoocDeviceResult:
        """Owner `part`: complete rows part + r * n_parts from every source's records."""
        res = CoocDeviceResult()
        check(_lib.load().cooc_shard_count(
            self._h, n_parts, part, ctypes.c_void_p(recv_row_counts.data_ptr()),
            ctypes.c_void_p(recv_desc.data_ptr()) if recv_desc.numel() else None, int(recv_desc.numel()),
            ctypes.c_void_p(arena_all.data_ptr()), int(arena_stride),
            _stream_arg(stream, recv_row_counts), ctypes.byref(res)), self._h)
        return res

    def verify_batch(self, symmetry: bool = False, row_checksum=None, stream=None) -> dict:
        """cooc_verify_batch over the last count_device result: the reference's DEVELOPMENT_MODE row-sum
        check (ItemRowRescorer...java:183-193) and the CSR contract's checks, on the device.
        row_checksum: optional uint64-sized device tensor [n_items] (torch.int64 is fine) that receives
        every row's fingerprint (sum of splitmix64(col << 32 ^ count); oracle.row_checksums restates it)."""
        out = np.zeros(8, np.int64)
        flags = _lib.COOC_VERIFY_SYMMETRY if symmetry else 0
        cs = ctypes.c_void_p(row_checksum.data_ptr()) if row_checksum is not None else None
        check(_lib.load().cooc_verify_batch(self._h, flags, cs, _p(out, i64p), self._stream(stream)), self._h)
        return {"sum_counts": int(out[0]), "sum_rowsums": int(out[1]), "entries": int(out[2]),
                "rows_bad_sum": int(out[3]), "rows_bad_entries": int(out[4]),
                "asymmetric_entries": None if out[5] < 0 else int(out[5])}

    def _stream(self, stream):
        """An explicit stream as given; else torch's current stream on this context's device (the null
        stream without a GPU)."""
        if stream is not None:
            return ctypes.c_void_p(int(stream))
        try:
            import torch

            if torch.cuda.is_available():
                dev = self.device if self.device >= 0 else torch.cuda.current_device()
                return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        except ImportError:
            pass
        return None

    # ---- communicator: the RCCL sharding layer inside the library -------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """cooc_comm_unique_id: rank 0's communicator id (128 opaque bytes) for cooc_comm_init."""
        buf = (ctypes.c_uint8 * _lib.COOC_COMM_ID_BYTES)()
        check(_lib.load().cooc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), None)
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """Join the RCCL communicator `unique_id` as `rank` of `world` (one context per GPU process)."""
        buf = (ctypes.c_uint8 * _lib.COOC_COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(_lib.load().cooc_comm_init(self._h, ctypes.cast(buf, ctypes.c_void_p), int(rank), int(world)), self._h)
        self.comm_world = int(world)

    def comm_init_ops(self, rank: int, world: int, ops: CoocCommOps) -> None:
        """The library's exchange over caller collectives (cooc_comm_ops); `ops` must stay alive as long
        as the context (the context keeps a reference)."""
        check(_lib.load().cooc_comm_init_ops(self._h, int(rank), int(world), ctypes.byref(ops), None), self._h)
        self._comm_ops = ops
        self.comm_world = int(world)

    def count_owned_host(self, user_ptr, items):
        """cooc_count_owned_host: count_owned from host arrays (a JVM subtask's buffered shard); the owned
        rows become this context's batch result.  Returns (BatchResult of the owned rows, CoocOwnedInfo)."""
        up = np.ascontiguousarray(user_ptr, np.int64)
        it = np.ascontiguousarray(items, np.int32)
        info, winfo = CoocOwnedInfo(), CoocWindowInfo()
        L = _lib.load()
        check(L.cooc_count_owned_host(self._h, len(up) - 1, _p(up, i64p), _p(it, i32p), ctypes.byref(info),
                                      ctypes.byref(winfo)), self._h)
        return self.copy_batch(winfo.nnz, winfo.observed), info

    def count_owned_host_info(self, user_ptr, items):
        """cooc_count_owned_host without copying the owned rows out: (CoocWindowInfo, CoocOwnedInfo); the rows
        then stream out with copy_batch_row_ptr / copy_batch_range (what the JVM operators do)."""
        up = np.ascontiguousarray(user_ptr, np.int64)
        it = np.ascontiguousarray(items, np.int32)
        info, winfo = CoocOwnedInfo(), CoocWindowInfo()
        check(_lib.load().cooc_count_owned_host(self._h, len(up) - 1, _p(up, i64p), _p(it, i32p), ctypes.byref(info),
                                                ctypes.byref(winfo)), self._h)
        return winfo, info

    def copy_batch_row_ptr(self):
        """(row_ptr int64[M + 1], rowsum int64[M], rowsum32 int32[M]) of the last batch (cooc_copy_batch with
        the entry arrays NULL)."""
        M = self.n_items
        rp, rs, rs32 = np.zeros(M + 1, np.int64), np.zeros(M, np.int64), np.zeros(M, np.int32)
        check(_lib.load().cooc_copy_batch(self._h, _p(rp, i64p), None, None, None, _p(rs, i64p), _p(rs32, i32p)),
              self._h)
        return rp, rs, rs32

    def copy_batch_range(self, r0: int, r1: int, cap: int):
        """cooc_copy_batch_range: (cols int32, cnt uint32, cnt16 int16) of rows [r0, r1), at most cap entries."""
        cols, cnt, cnt16 = np.zeros(cap, np.int32), np.zeros(cap, np.uint32), np.zeros(cap, np.int16)
        check(_lib.load().cooc_copy_batch_range(self._h, int(r0), int(r1), int(cap), _p(cols, i32p), _p(cnt, u32p),
                                                _p(cnt16, i16p)), self._h)
        return cols, cnt, cnt16

    def topk_owned_host(self, topk: int, exact_scores: bool = False) -> None:
        """cooc_topk_owned_host: the owned rows' heaps into the context's buffers (copy_topk_range reads them)."""
        check(_lib.load().cooc_topk_owned_host(self._h, int(topk), _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0),
              self._h)

    def copy_topk_range(self, r0: int, r1: int, topk: int):
        """cooc_copy_topk_batch_range: (sizes [n], values [n, k], scores [n, k]) of rows [r0, r1)."""
        n = int(r1) - int(r0)
        sizes, vals, scores = np.zeros(n, np.int32), np.zeros((n, topk), np.int32), np.zeros((n, topk), np.float64)
        check(_lib.load().cooc_copy_topk_batch_range(self._h, int(r0), int(r1), int(topk), _p(sizes, i32p),
                                                     _p(vals, i32p), _p(scores, f64p)), self._h)
        return sizes, vals, scores

    def comm_allgather_i64(self, value: int) -> np.ndarray:
        """cooc_comm_allgather_i64: every rank's value, in rank order."""
        out = np.zeros(self.comm_world, np.int64)
        check(_lib.load().cooc_comm_allgather_i64(self._h, int(value), _p(out, i64p)), self._h)
        return out

    def count_owned(self, user_ptr, items, stream=None):
        """cooc_count_owned: this rank's users -> the rows it owns over the whole job's users (item
        counts all-reduced, owner map, histories all-gathered, owned rows counted, pairs all-reduced),
        all inside the library.  Returns (CoocDeviceResult, CoocOwnedInfo)."""
        res, info = CoocDeviceResult(), CoocOwnedInfo()
        n_users = int(user_ptr.numel()) - 1
        check(_lib.load().cooc_count_owned(self._h, n_users, ctypes.c_void_p(user_ptr.data_ptr()),
                                           ctypes.c_void_p(items.data_ptr()) if items.numel() else None,
                                           int(items.numel()), _stream_arg(stream, user_ptr), ctypes.byref(info),
                                           ctypes.byref(res)), self._h)
        return res, info

    def topk_owned(self, topk: int, sizes, values, scores, rowsum_global=None, exact_scores: bool = False,
                   stream=None) -> None:
        """cooc_topk_owned: the owned rows' row sums all-reduced, then their LLR top-k into device tensors."""
        check(_lib.load().cooc_topk_owned(
            self._h, int(topk), _lib.COOC_FLAG_EXACT_SCORES if exact_scores else 0, ctypes.c_void_p(sizes.data_ptr()),
            ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
            None if rowsum_global is None else ctypes.c_void_p(rowsum_global.data_ptr()), _stream_arg(stream, sizes)),
            self._h)

    @staticmethod
    def snake_owner(counts, world: int, head: int = 4096) -> np.ndarray:
        """cooc_snake_owner (host): the owner map cooc_count_owned builds, from host item counts."""
        c = np.ascontiguousarray(counts, np.int64)
        out = np.zeros(len(c), np.int32)
        check(_lib.load().cooc_snake_owner(_p(c, i64p), len(c), int(world), int(head), _p(out, i32p)), None)
        return out

    def set_kernel_timing(self, enable: bool = True) -> None:
        check(_lib.load().cooc_set_kernel_timing(self._h, 1 if enable else 0), self._h)

    def last_sort_rows(self) -> tuple:
        """(rows, ordered pairs) the last large-universe count sent through the sort + segmented-reduce
        path (rows whose LDS hash table overflowed, or every whole row with planner="sort")."""
        rows, pairs = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.load().cooc_last_sort_rows(self._h, ctypes.byref(rows), ctypes.byref(pairs)), self._h)
        return rows.value, pairs.value

    def last_mirror_rows(self) -> int:
        """Split rows whose columns above the first tile the last large-universe count took from the other
        rows' entries (the matrix is symmetric) instead of walking them; 0 when that was off."""
        rows = ctypes.c_int64()
        check(_lib.load().cooc_last_mirror_rows(self._h, ctypes.byref(rows)), self._h)
        return rows.value

    def last_attempts(self) -> tuple:
        """(attempts, region entries) of the last large-universe count: 1 attempt normally, 2 after the output
        region was grown to the exact bound or after a mirrored attempt was repeated without mirroring, 3 after
        both; and the entries of the region the last attempt filled."""
        attempts, entries = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.load().cooc_last_attempts(self._h, ctypes.byref(attempts), ctypes.byref(entries)), self._h)
        return attempts.value, entries.value

    def last_batch_plan(self) -> tuple:
        """(B, db, n_chunks, n_split, dense, max_len, n_long, 0) of the last run of the batch planner
        (n_items < 40,320): partition blocks of the histogram / scatter passes, descriptors per batch of the
        accumulate kernel, chunks, split rows, 1 for the dense layout, the longest list and the lists longer than
        2,048 ids.  Zeros before any such run and after a large-universe run."""
        v = (ctypes.c_int64 * 8)()
        check(_lib.load().cooc_last_batch_plan(self._h, v), self._h)
        return tuple(int(x) for x in v)

    def global_slab_stats(self) -> tuple:
        """(cap, bump, live, compactions) of the sparse global rows' arena (n_items >= 40,320): capacity in
        entries, the bump pointer, the live entries (the sum of the row lengths) and the compactions since the
        state was created or restored, the first window's included.  Zeros with the dense global matrix."""
        v = [ctypes.c_int64() for _ in range(4)]
        check(_lib.load().cooc_global_slab_stats(self._h, *[ctypes.byref(x) for x in v]), self._h)
        return tuple(x.value for x in v)

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float()
        check(_lib.load().cooc_last_kernel_ms(self._h, ctypes.byref(ms)), self._h)
        return ms.value

    # ---- streaming windows ----------------------------------------------------------------------
    def submit_batch(self, window_ts: int, user_ids, user_ptr, items) -> None:
        uid = np.ascontiguousarray(user_ids, np.int32)
        up = np.ascontiguousarray(user_ptr, np.int64)
        it = np.ascontiguousarray(items, np.int32)
        check(_lib.load().cooc_submit_batch(self._h, window_ts, len(uid), _p(uid, i32p), _p(up, i64p),
                                            _p(it, i32p)), self._h)

    def finish_window(self, window_ts: int) -> WindowResult:
        return self._window(self.finish_window_info(window_ts))

    def finish_window_info(self, window_ts: int) -> CoocWindowInfo:
        """Process the staged window; its outputs stay on the device until window_result()."""
        info = CoocWindowInfo()
        check(_lib.load().cooc_finish_window(self._h, window_ts, ctypes.byref(info)), self._h)
        return info

    def window_result(self, info: CoocWindowInfo) -> WindowResult:
        return self._window(info)

    def _window(self, info: CoocWindowInfo) -> WindowResult:
        L = _lib.load()
        R, nnz = info.n_rows, info.nnz
        rows = np.zeros(R, np.int32)
        rp = np.zeros(R + 1, np.int64)
        cols = np.zeros(nnz, np.int32)
        cnt = np.zeros(nnz, np.uint32)
        cnt16 = np.zeros(nnz, np.int16)
        check(L.cooc_copy_window_delta(self._h, _p(rows, i32p), _p(rp, i64p), _p(cols, i32p), _p(cnt, u32p),
                                       _p(cnt16, i16p)), self._h)
        rs_items = np.zeros(R, np.int32)
        rs = np.zeros(R, np.int64)
        rs32 = np.zeros(R, np.int32)
        check(L.cooc_copy_window_rowsums(self._h, _p(rs_items, i32p), _p(rs, i64p), _p(rs32, i32p)), self._h)
        # (sampled mode: the counts are signed nets, two's complement in the uint32 buffer)
        exact = cnt.view(np.int32).astype(np.int64) if self.sampled else cnt.astype(np.int64)
        w = WindowResult(info.ts, rows, rp, cols, exact, cnt16, rs_items, rs, rs32, info.observed)
        if info.topk > 0:
            k = info.topk
            tr = np.zeros(info.n_topk, np.int32)
            ts = np.zeros(info.n_topk, np.int32)
            tv = np.zeros((info.n_topk, k), np.int32)
            tsc = np.zeros((info.n_topk, k), np.float64)
            if info.n_topk:
                check(L.cooc_copy_window_topk(self._h, _p(tr, i32p), _p(ts, i32p), _p(tv, i32p), _p(tsc, f64p)),
                      self._h)
            w.topk_rows, w.topk_sizes, w.topk_values, w.topk_scores = tr, ts, tv, tsc
        return w

    def global_rowsums(self):
        M = self.n_items
        ex = np.zeros(M, np.int64)
        v32 = np.zeros(M, np.int32)
        check(_lib.load().cooc_global_rowsums(self._h, _p(ex, i64p), _p(v32, i32p)), self._h)
        return ex, v32

    def global_observed(self):
        ex = ctypes.c_int64()
        ref = ctypes.c_int64()
        check(_lib.load().cooc_global_observed(self._h, ctypes.byref(ex), ctypes.byref(ref)), self._h)
        return ex.value, ref.value

    def global_row(self, item: int):
        L = _lib.load()
        n = ctypes.c_int64()
        check(L.cooc_global_row_nnz(self._h, item, ctypes.byref(n)), self._h)
        cols = np.zeros(n.value, np.int32)
        cnt = np.zeros(n.value, np.uint32)
        cnt16 = np.zeros(n.value, np.int16)
        check(L.cooc_global_row(self._h, item, _p(cols, i32p), _p(cnt, u32p), _p(cnt16, i16p)), self._h)
        return cols, cnt, cnt16

    # ---- sampled mode ---------------------------------------------------------------------------
    def sampling_enable(self, item_cut: int, seed: int = 0, on: str = "host") -> None:
        """cooc_sampling_enable (on="host") / cooc_sampling_enable_device (on="device") on a context built with
        user_cut > 0 and without item_cut, which has no streaming state yet.  The call a multi-GPU job makes after
        comm_init / comm_init_ops: a sampled context refuses to join a communicator, one that has joined accepts
        sampling (include/cooc.h, sampled mode at world > 1)."""
        if on not in ("host", "device"):
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"unknown sample_on {on!r}")
        L = _lib.load()
        enable = L.cooc_sampling_enable_device if on == "device" else L.cooc_sampling_enable
        check(enable(self._h, int(item_cut), ctypes.c_int64(_as_i64(seed))), self._h)
        self.sampled = True

    def user_history(self, user: int):
        """(items, total): the user's resident history in slot order (the reservoir in the sampled mode) and its
        userInteractionsTotal (outside the sampled mode: the history's length)."""
        L = _lib.load()
        n = ctypes.c_int32()
        total = ctypes.c_int32()
        check(L.cooc_copy_user_history(self._h, int(user), 0, None, ctypes.byref(n), ctypes.byref(total)), self._h)
        items = np.zeros(n.value, np.int32)
        if n.value:
            check(L.cooc_copy_user_history(self._h, int(user), n.value, _p(items, i32p), None, None), self._h)
        return items, total.value

    def last_window_runs(self) -> int:
        """Runs of the window counter in the last sampled window: 0 empty, 1 plus lists only, 2 with the minus run."""
        n = ctypes.c_int64()
        check(_lib.load().cooc_last_window_runs(self._h, ctypes.byref(n)), self._h)
        return n.value

    def sampling_counters(self) -> dict:
        a = np.zeros(6, np.int64)
        check(_lib.load().cooc_sampling_counters(self._h, _p(a, i64p)), self._h)
        names = ("item_cut_rejections", "fills", "replacements", "feedbacks", "users", "item_counter_sum")
        return {k: int(v) for k, v in zip(names, a)}

    def sample_device(self, users, items, n_users: int, item_cut: int, user_cut: int, seed: int = 0, window_ptr=None,
                      stream=None, *, res_cap=None):
        """cooc_sample_device: the sampled mode's item cut, reservoirs and feedback over a device-resident log, from
        empty state.  users, items: int32 device tensors of the records in arrival order (users: dense indices
        [0, n_users)); window_ptr: host int64 [n_windows + 1] (None: one window).  Returns (res_ptr int64
        [n_users + 1], res_items int32, total int32 [n_users], item_count int16 [n_items], info dict) as device
        tensors; (res_ptr, res_items) is a CSR for count_device.  res_items is allocated at
        min(n_records, n_users * user_cut) (res_cap: another capacity) and trimmed; the call's info, also of a
        failed call, stays in last_sample_info."""
        return self._sample(False, users, items, n_users, None, item_cut, user_cut, seed, window_ptr, stream, res_cap)

    def sample_owned(self, users, items, n_users: int, user_key, item_cut: int, user_cut: int, seed: int = 0,
                     window_ptr=None, stream=None, *, res_cap=None):
        """cooc_sample_owned: sample_device over the context's communicator, a collective.  users, items: this
        rank's own users' records (users: local dense indices [0, n_users); n_users == 0 without records is allowed);
        user_key: int32 device tensor [n_users] of the users' job-wide ids, which key the draw (None: the index);
        window_ptr: over this rank's records, the same number of windows on every rank.  Returns sample_device's
        tuple: (res_ptr, res_items) is the rank's local CSR, an input of count_owned; total is local, item_count
        replicated; info counts this rank's decisions, item_counter_sum the job's.  Without a communicator, or at
        world 1, no collective is called.  If any rank's arguments fail, every rank raises
        IllegalArgumentException."""
        return self._sample(True, users, items, n_users, user_key, item_cut, user_cut, seed, window_ptr, stream,
                            res_cap)

    def _sample(self, owned, users, items, n_users, user_key, item_cut, user_cut, seed, window_ptr, stream, res_cap):
        import torch

        n = int(users.numel())
        if int(items.numel()) != n:
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, "users and items differ in length")
        if user_key is not None and int(user_key.numel()) != max(int(n_users), 0):
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, "user_key must hold n_users keys")
        dev = users.device
        wp = None if window_ptr is None else np.ascontiguousarray(window_ptr, np.int64)
        n_windows = 1 if wp is None else len(wp) - 1
        cap = min(n, max(int(n_users), 0) * max(int(user_cut), 0)) if res_cap is None else int(res_cap)
        res_ptr = torch.empty(max(int(n_users), 0) + 1, dtype=torch.int64, device=dev)
        res_items = torch.empty(max(cap, 0), dtype=torch.int32, device=dev)
        total = torch.empty(max(int(n_users), 0), dtype=torch.int32, device=dev)
        item_count = torch.empty(self.n_items, dtype=torch.int16, device=dev)
        info = _lib.CoocSampleInfo()
        self.last_sample_info = None
        L = _lib.load()
        head = (self._h, n, ctypes.c_void_p(users.data_ptr()) if n else None,
                ctypes.c_void_p(items.data_ptr()) if n else None, int(n_users))
        if owned:
            head += (ctypes.c_void_p(user_key.data_ptr()) if user_key is not None and user_key.numel() else None,)
        st = (L.cooc_sample_owned if owned else L.cooc_sample_device)(
            *head, n_windows, _p(wp, i64p), int(item_cut),
            int(user_cut), ctypes.c_int64(_as_i64(seed)), ctypes.c_void_p(res_ptr.data_ptr()),
            ctypes.c_void_p(res_items.data_ptr()) if cap > 0 else None, cap, ctypes.c_void_p(total.data_ptr()),
            ctypes.c_void_p(item_count.data_ptr()), _stream_arg(stream, users), ctypes.byref(info))
        self.last_sample_info = info.as_dict()
        check(st, self._h)
        return res_ptr, res_items[:info.reservoir_items], total, item_count, self.last_sample_info

    # ---- device ingest -------------------------------------------------------------------------
    def parse_interactions_device(self, text, stream=None):
        """cooc_parse_interactions_device: parse_interactions for a text on the GPU.  text: a torch.uint8 device
        tensor, or bytes (copied to the context's device).  Returns (users int32, items int32, ts int64) device
        tensors; a rejected line raises IllegalArgumentException naming its 0-based index."""
        import torch

        if isinstance(text, (bytes, bytearray, memoryview)):
            host = torch.frombuffer(bytearray(text), dtype=torch.uint8) if len(text) else torch.empty(0, dtype=torch.uint8)
            text = host.to(torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device()))
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous():
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, "text must be a contiguous torch.uint8 device tensor")
        L = _lib.load()
        nb = int(text.numel())
        tp = ctypes.c_void_p(text.data_ptr()) if nb else None
        sa = _stream_arg(stream, text)
        n, bad = ctypes.c_int64(), ctypes.c_int64(-1)
        check(L.cooc_parse_interactions_device(self._h, tp, nb, 0, None, None, None, sa, ctypes.byref(n),
                                               ctypes.byref(bad)), self._h)
        users = torch.empty(n.value, dtype=torch.int32, device=text.device)
        items = torch.empty(n.value, dtype=torch.int32, device=text.device)
        ts = torch.empty(n.value, dtype=torch.int64, device=text.device)
        check(L.cooc_parse_interactions_device(self._h, tp, nb, n.value, ctypes.c_void_p(users.data_ptr()),
                                               ctypes.c_void_p(items.data_ptr()), ctypes.c_void_p(ts.data_ptr()), sa,
                                               ctypes.byref(n), ctypes.byref(bad)), self._h)
        return users, items, ts

    def prepare_log(self, users, items, ts, records_per_watermark: int = 100_000, stream=None) -> "PreparedLog":
        """cooc_log_prepare_device: the late drop, the tumbling-window assignment and keyBy(user) of a log in arrival
        order (int32, int32, int64 device tensors), as the operator holds it after run_text_source's feed with the
        same records_per_watermark.  Returns a PreparedLog; the window lists are fetched with the two-phase call
        when the log has more windows than the first call allows for.  The call's info, also of a failed call,
        stays in last_log_info."""
        import torch

        n = int(users.numel())
        if int(items.numel()) != n or int(ts.numel()) != n:
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, "users, items and ts differ in length")
        dev = users.device
        rec_user = torch.empty(n, dtype=torch.int32, device=dev)
        rec_item = torch.empty(n, dtype=torch.int32, device=dev)
        user_ids = torch.empty(n, dtype=torch.int32, device=dev)
        user_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        user_items = torch.empty(n, dtype=torch.int32, device=dev)
        info = _lib.CoocLogInfo()
        self.last_log_info = None
        L = _lib.load()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
        cap = 1024
        while True:
            wp, wt = np.zeros(cap + 1, np.int64), np.zeros(cap, np.int64)
            st = L.cooc_log_prepare_device(self._h, n, ptr(users), ptr(items), ptr(ts), int(records_per_watermark),
                                           ptr(rec_user), ptr(rec_item), ptr(user_ids),
                                           ctypes.c_void_p(user_ptr.data_ptr()), ptr(user_items), _p(wp, i64p),
                                           _p(wt, i64p), cap, _stream_arg(stream, users), ctypes.byref(info))
            self.last_log_info = info.as_dict()
            if st == _lib.COOC_ERR_ARG and info.bad_record < 0 and info.n_windows > cap:
                cap = int(info.n_windows)  # the need, as reported: the second phase
                continue
            check(st, self._h)
            break
        nk, nu, nw = int(info.n_kept), int(info.n_users), int(info.n_windows)
        return PreparedLog(rec_user[:nk], rec_item[:nk], user_ids[:nu], user_ptr[:nu + 1], user_items[:nk],
                           wp[:nw + 1].copy(), wt[:nw].copy(), self.last_log_info)

    # ---- checkpoints ----------------------------------------------------------------------------
    SNAPSHOT_RANGE = 1 << 30  # bytes per cooc_snapshot_copy / cooc_restore_write call

    def snapshot(self, range_bytes: int = SNAPSHOT_RANGE) -> bytes:
        """The streaming state as one canonical blob (cooc_snapshot_prepare, copies in ranges of at most
        range_bytes, cooc_snapshot_release); its cooc_snapshot_info is kept as a dict in last_snapshot_info.
        IllegalStateException while a window staged by submit_batch is unfinished, and on a sampled context
        (item_cut > 0): that one is checkpointed with snapshot_sampled() / restore_sampled()."""
        return self._snapshot(_lib.load().cooc_snapshot_prepare, range_bytes)

    def snapshot_sampled(self, range_bytes: int = SNAPSHOT_RANGE) -> bytes:
        """snapshot() of a sampled context, decided on the host or the device (cooc_sampling_snapshot_prepare): the
        format-2 blob, which also holds the item counters, the users' totals and the decision counters.  The same
        logical state gives the same bytes in either mode and either representation of the global rows.
        IllegalStateException on an unsampled context or while a window is staged."""
        return self._snapshot(_lib.load().cooc_sampling_snapshot_prepare, range_bytes)

    def _snapshot(self, prepare, range_bytes: int) -> bytes:
        L = _lib.load()
        info = _lib.CoocSnapshotInfo()
        check(prepare(self._h, ctypes.byref(info)), self._h)
        try:
            out = np.empty(info.bytes, np.uint8)
            for off in range(0, info.bytes, int(range_bytes)):
                n = min(int(range_bytes), info.bytes - off)
                check(L.cooc_snapshot_copy(self._h, off, n, ctypes.c_void_p(out.ctypes.data + off)), self._h)
        finally:
            check(L.cooc_snapshot_release(self._h), self._h)
        self.last_snapshot_info = info.as_dict()
        return out.tobytes()

    def restore(self, blob: bytes, range_bytes: int = SNAPSHOT_RANGE) -> dict:
        """Install a blob of snapshot() into this context, which must have no streaming state
        (IllegalStateException otherwise).  The blob is validated first; a blob that fails, or one taken with
        another n_items / window / user_cut / (rank, world), is IllegalArgumentException and leaves the context
        empty and usable.  Returns the blob's cooc_snapshot_info as a dict.  A sampled context refuses
        (IllegalStateException): it restores a blob of snapshot_sampled() with restore_sampled()."""
        L = _lib.load()
        return self._restore(L.cooc_restore_begin, L.cooc_restore_write, L.cooc_restore_finish, blob, range_bytes)

    def restore_sampled(self, blob: bytes, range_bytes: int = SNAPSHOT_RANGE) -> dict:
        """Install a blob of snapshot_sampled() into this sampled context (either mode), which must have no
        streaming state (IllegalStateException otherwise, also on an unsampled context).  A blob that fails the
        validation, a format-1 blob of snapshot(), or one taken with another n_items / window / user_cut /
        item_cut / seed is IllegalArgumentException and leaves the context empty, sampled and usable."""
        L = _lib.load()
        return self._restore(L.cooc_sampling_restore_begin, L.cooc_sampling_restore_write,
                             L.cooc_sampling_restore_finish, blob, range_bytes)

    def _restore(self, begin, write, finish, blob: bytes, range_bytes: int) -> dict:
        buf = np.frombuffer(blob, np.uint8)
        check(begin(self._h, len(buf)), self._h)
        for off in range(0, len(buf), int(range_bytes)):
            n = min(int(range_bytes), len(buf) - off)
            check(write(self._h, off, n, ctypes.c_void_p(buf.ctypes.data + off)), self._h)
        info = _lib.CoocSnapshotInfo()
        check(finish(self._h, ctypes.byref(info)), self._h)
        return info.as_dict()

    def restore_parts(self, blobs, route=None, range_bytes: int = SNAPSHOT_RANGE) -> dict:
        """Rescaling: install ALL blobs of one checkpoint of a job (blobs[i] taken by rank i of len(blobs)) into
        this context's own (rank, world), which may differ from the job's (cooc_restore_begin_parts, _write_part,
        _finish_parts; join the communicator first).  route says which users this context keeps: None keeps u with
        u % world == rank; a numpy bool / uint8 array over user ids keeps u iff 0 <= u < len(route) and route[u]
        (the caller sees to it that every user is kept by exactly one subtask); a _lib.CoocUserRoute goes to the
        library as it is.  Everything is validated first: IllegalArgumentException leaves the context empty and
        usable.  Returns the cooc_snapshot_info of the installed state as a dict."""
        L = _lib.load()
        bufs = [np.frombuffer(b, np.uint8) for b in blobs]
        sizes = np.array([len(b) for b in bufs], np.int64)
        words = None
        if route is None:
            rt = _lib.CoocUserRoute(_lib.COOC_ROUTE_MOD, 0, 0, None)
        elif isinstance(route, _lib.CoocUserRoute):
            rt = route
        else:
            keep = np.ascontiguousarray(route).astype(bool)
            packed = np.packbits(keep, bitorder="little")
            words = np.zeros((len(keep) + 63) // 64 * 8 + 8, np.uint8)
            words[:len(packed)] = packed
            rt = _lib.CoocUserRoute(_lib.COOC_ROUTE_BITMAP, 0, len(keep), ctypes.c_void_p(words.ctypes.data))
        check(L.cooc_restore_begin_parts(self._h, len(bufs), _p(sizes, i64p)), self._h)
        for i, buf in enumerate(bufs):
            for off in range(0, len(buf), int(range_bytes)):
                n = min(int(range_bytes), len(buf) - off)
                check(L.cooc_restore_write_part(self._h, i, off, n, ctypes.c_void_p(buf.ctypes.data + off)), self._h)
        info = _lib.CoocSnapshotInfo()
        check(L.cooc_restore_finish_parts(self._h, ctypes.byref(rt), ctypes.byref(info)), self._h)
        return info.as_dict()

    @staticmethod
    def snapshot_info(blob: bytes) -> dict:
        """cooc_snapshot_inspect: header and directory of a blob, on the host (no context, no device)."""
        buf = np.frombuffer(blob, np.uint8) if len(blob) else np.zeros(1, np.uint8)
        info = _lib.CoocSnapshotInfo()
        check(_lib.load().cooc_snapshot_inspect(ctypes.c_void_p(buf.ctypes.data), len(blob), ctypes.byref(info)), None)
        return info.as_dict()

    @staticmethod
    def sampled_snapshot_info(blob: bytes) -> dict:
        """cooc_sampling_snapshot_inspect: header, directory and sampler scalars of a snapshot_sampled() blob, on
        the host: the fields of snapshot_info() and item_cut, seed, the four decision counters, counted_items
        (items with a non-zero counter) and total_users (users with a total)."""
        buf = np.frombuffer(blob, np.uint8) if len(blob) else np.zeros(1, np.uint8)
        info, sinfo = _lib.CoocSnapshotInfo(), _lib.CoocSamplingSnapshotInfo()
        check(_lib.load().cooc_sampling_snapshot_inspect(ctypes.c_void_p(buf.ctypes.data), len(blob), ctypes.byref(info),
                                                         ctypes.byref(sinfo)), None)
        return {**info.as_dict(), **sinfo.as_dict()}

    # ---- operator mirror ------------------------------------------------------------------------
    def op_process_elements(self, users, items, ts) -> int:
        u = np.ascontiguousarray(users, np.int32)
        i = np.ascontiguousarray(items, np.int32)
        t = np.ascontiguousarray(ts, np.int64)
        late = ctypes.c_int64()
        check(_lib.load().cooc_op_process_elements(self._h, len(u), _p(u, i32p), _p(i, i32p), _p(t, i64p),
                                                   ctypes.byref(late)), self._h)
        return late.value

    def op_process_watermark(self, watermark: int) -> list[WindowResult]:
        out = []
        L = _lib.load()
        while True:
            fired = ctypes.c_int32()
            info = CoocWindowInfo()
            check(L.cooc_op_process_watermark(self._h, watermark, ctypes.byref(fired), ctypes.byref(info)), self._h)
            if not fired.value:
                return out
            out.append(self._window(info))

    def op_counters(self) -> dict:
        a = np.zeros(5, np.int64)
        check(_lib.load().cooc_op_counters(self._h, _p(a, i64p)), self._h)
        return {
            "UserInteractionCounterLateElements": int(a[0]),
            "UserInteractionCounterObservedCooccurrences": int(a[1]),
            "RowSumProcessWindowRowSum": int(a[2]),
            "ItemRowRescorerRescoredItems": int(a[3]),
            "rescorer_observed": int(a[4]),
        }


class NonSampledUserInteractionCounterOneInputStreamOperator:
    """Drop-in for the `--skip-cuts` operator chain (FlinkCooccurrences.java:65-74,135-167).

    ``NonSampledUserInteractionCounterOneInputStreamOperator(windowSize, windowUnit)`` plus the
    rescorer's ``topK`` (ItemRowRescorerTwoInputStreamOperator(short topK), :51-56) and the item-id
    universe the device tables are sized for.
    """

    ITEM_TAG = "itemCooccurrences"  # NonSampled...java:41-42
    ROW_SUM_TAG = "rowSums"         # NonSampled...java:45-46

    def __init__(self, window_size: int, window_unit: str = "MILLISECONDS", *, n_items: int, top_k: int = 10,
                 device: int = -1, exact_scores: bool = False, planner: str = "auto", user_cut: int = 0,
                 item_cut: int = 0, sample_seed: int = 0, sample_on: str = "host"):
        """user_cut (kMax, 0 = off): expand only the first user_cut interactions of every user
        (UserInteractionCounter...java:168-205 without its random reservoir branch).  item_cut (fMax) > 0: the
        sampled mode, with user_cut as the reservoir size, decided on sample_on = "host" or "device"
        (CooccurrenceCore)."""
        if top_k <= 0:  # ItemRowRescorer...java:52-54
            raise _lib.IllegalArgumentException(_lib.COOC_ERR_ARG, f"{top_k} is <= 0")
        self.core = CooccurrenceCore(n_items, top_k, window_size_ms(window_size, window_unit), device, exact_scores,
                                     planner=planner, user_cut=user_cut, item_cut=item_cut, sample_seed=sample_seed,
                                     sample_on=sample_on)

    def process_element(self, user: int, item: int, timestamp: int) -> bool:
        """Returns True when the record was late and dropped (NonSampled...java:89-91)."""
        return self.core.op_process_elements([user], [item], [timestamp]) == 1

    def process_elements(self, users, items, timestamps) -> int:
        return self.core.op_process_elements(users, items, timestamps)

    def process_watermark(self, watermark: int) -> list[WindowResult]:
        return self.core.op_process_watermark(watermark)

    def accumulators(self) -> dict:
        return self.core.op_counters()

    def user_history(self, user: int):
        return self.core.user_history(user)

    def sampling_counters(self) -> dict:
        return self.core.sampling_counters()

    def sampling_enable(self, item_cut: int, seed: int = 0, on: str = "host") -> None:
        """The sampled mode of a multi-GPU job: built with user_cut and without item_cut, joined to its communicator
        (sharding.init_comm_torch_ops(op.core), core.comm_init), then sampled (CooccurrenceCore.sampling_enable)."""
        self.core.sampling_enable(item_cut, seed, on)

    # snapshotState / initializeState: the operator's whole state (histories, global rows and row sums, the
    # accumulators, the watermark and the buffered windows) as one blob.  A sampled operator (item_cut > 0) goes
    # through the _sampled calls: its blob also holds the item counters, the totals and the decision counters.
    def snapshot(self) -> bytes:
        return self.core.snapshot()

    def restore(self, blob: bytes) -> dict:
        return self.core.restore(blob)

    def snapshot_sampled(self) -> bytes:
        return self.core.snapshot_sampled()

    def restore_sampled(self, blob: bytes) -> dict:
        return self.core.restore_sampled(blob)

    @staticmethod
    def sampled_snapshot_info(blob: bytes) -> dict:
        return CooccurrenceCore.sampled_snapshot_info(blob)

    # a restart at another parallelism: all blobs of the old job's checkpoint (union list state)
    def restore_parts(self, blobs, route=None, range_bytes: int = CooccurrenceCore.SNAPSHOT_RANGE) -> dict:
        return self.core.restore_parts(blobs, route, range_bytes)

    @staticmethod
    def snapshot_info(blob: bytes) -> dict:
        return CooccurrenceCore.snapshot_info(blob)

    def close(self):
        self.core.close()


# ---- ItemCooccurrences wire codec (ItemCooccurrences.java:113-147) --------------------------------
def encode_item_cooccurrences(items, increments, rec_ptr, others, ks=None) -> bytes:
    """Records (item, increment, others[rec_ptr[r]:rec_ptr[r+1]]) in the Kryo wire format of
    ItemCooccurrences.Serializer.write; ks[r] != -1 skips slot k of record r (:124-131)."""
    it = np.ascontiguousarray(items, np.int32)
    inc = np.ascontiguousarray(increments, np.int16)
    rp = np.ascontiguousarray(rec_ptr, np.int64)
    ot = np.ascontiguousarray(others, np.int32)
    kk = None if ks is None else np.ascontiguousarray(ks, np.int32)
    L = _lib.load()
    n = ctypes.c_int64()
    args = (len(it), _p(it, i32p), _p(inc, i16p), None if kk is None else _p(kk, i32p), _p(rp, i64p), _p(ot, i32p))
    check(L.cooc_records_encode(*args, None, 0, ctypes.byref(n)), None)
    out = np.zeros(max(n.value, 1), np.uint8)
    check(L.cooc_records_encode(*args, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)), None)
    return out[: n.value].tobytes()


def decode_item_cooccurrences(data: bytes):
    """ItemCooccurrences.Serializer.read over a byte stream of records -> (items int32,
    increments int16, rec_ptr int64, others int32)."""
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    L = _lib.load()
    nr, no = ctypes.c_int64(), ctypes.c_int64()
    bp = buf.ctypes.data_as(ctypes.c_void_p)
    check(L.cooc_records_decode(bp, len(data), ctypes.byref(nr), ctypes.byref(no), None, None, None, None), None)
    items = np.zeros(nr.value, np.int32)
    inc = np.zeros(nr.value, np.int16)
    rp = np.zeros(nr.value + 1, np.int64)
    ot = np.zeros(no.value, np.int32)
    check(L.cooc_records_decode(bp, len(data), ctypes.byref(nr), ctypes.byref(no), _p(items, i32p), _p(inc, i16p),
                                _p(rp, i64p), _p(ot, i32p)), None)
    return items, inc, rp, ot


# ---- text ingest (FlinkCooccurrences.java:55-61,207-229) -------------------------------------------
def parse_interactions(data: bytes):
    """'\\n'-delimited "user,item,timestamp" lines -> (users int32, items int32, ts int64), with the
    reference's InteractionLineSplitter semantics; a rejected line raises IllegalArgumentException
    naming its 0-based index."""
    L = _lib.load()
    n, bad = ctypes.c_int64(), ctypes.c_int64()
    check(L.cooc_parse_interactions(data, len(data), 0, None, None, None, ctypes.byref(n), ctypes.byref(bad)), None)
    users = np.zeros(n.value, np.int32)
    items = np.zeros(n.value, np.int32)
    ts = np.zeros(n.value, np.int64)
    st = L.cooc_parse_interactions(data, len(data), n.value, _p(users, i32p), _p(items, i32p), _p(ts, i64p),
                                   ctypes.byref(n), ctypes.byref(bad))
    if st != _lib.COOC_OK:
        raise _lib.IllegalArgumentException(st, f"line {bad.value} is not 'user,item,timestamp'")
    return users, items, ts


def run_text_source(op, data: bytes, records_per_watermark: int = 100_000) -> list:
    """Drive an operator from the job's text input: records in file order, and after every
    records_per_watermark records the AscendingTimestampExtractor watermark (largest timestamp so far
    - 1, FlinkCooccurrences.java:221-229); Long.MAX_VALUE at the end of the input (PROCESS_ONCE)."""
    users, items, ts = parse_interactions(data)
    out, hi = [], None
    for lo in range(0, len(users), records_per_watermark):
        sl = slice(lo, lo + records_per_watermark)
        op.process_elements(users[sl], items[sl], ts[sl])
        m = int(ts[sl].max())
        hi = m if hi is None else max(hi, m)
        out += op.process_watermark(hi - 1)
    out += op.process_watermark(2**63 - 1)
    return out
