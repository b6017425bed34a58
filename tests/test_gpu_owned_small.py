"""cooc_count_owned / cooc_topk_owned below 40,320 items in one process: a world-1 communicator whose operations
only copy this rank's buffers to themselves (cooc_comm_ops) runs the whole records exchange -- local plan,
agreement, arena all-gather, row counts and descriptors to their owner, owner count, expansion to item-indexed
views -- and owns every row, so the result must equal cooc_count_device's row for row and cooc_topk_owned's heaps
cooc_topk_batch's.  Also pinned here, with no communicator: the rescoring path the owners take
(cooc_topk_batch_device with external row sums over a batch-planner CSR, columns ascending, no column order), and
sharding.count_owned's refusal of a small universe without a library communicator.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (at collection, before any test opens the GPU through the library: torch.cuda finds it)

import _owned_small as osm
from test_multiproc_gpu import _d2h, _rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _self_copy_ops(_lib):
    """cooc_comm_ops of a one-rank world: the sum over one rank is the value, the gather and the exchange copy this
    rank's bytes to their place, on the stream given"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    calls = {"allreduce": 0, "allgather": 0, "alltoallv": 0}

    def copy(dst, src, n, stream):
        return hip.hipMemcpyAsync(dst, src, n, 3, stream) if n else 0

    def allreduce(_user, _buf, _n, _stream):
        calls["allreduce"] += 1
        return 0

    def allgather(_user, d_send, d_recv, nbytes, stream):
        calls["allgather"] += 1
        return copy(d_recv, d_send, nbytes, stream)

    def alltoallv(_user, d_send, send_off, send_bytes, d_recv, recv_off, recv_bytes, stream):
        calls["alltoallv"] += 1
        assert send_bytes[0] == recv_bytes[0]
        return copy((d_recv or 0) + recv_off[0], (d_send or 0) + send_off[0], send_bytes[0], stream)

    return _lib.CoocCommOps(_lib.ALLREDUCE_FN(allreduce), _lib.ALLGATHER_FN(allgather),
                            _lib.ALLTOALLV_FN(alltoallv)), calls


def _topk_device(core, torch, M, rowsum_global=None):
    dev = torch.device("cuda", 0)
    sizes = torch.empty(M, dtype=torch.int32, device=dev)
    vals = torch.zeros((M, osm.TOPK), dtype=torch.int32, device=dev)
    scores = torch.zeros((M, osm.TOPK), dtype=torch.float64, device=dev)
    core.topk_batch_device(osm.TOPK, sizes, vals, scores, rowsum_global=rowsum_global)
    torch.cuda.current_stream().synchronize()
    return sizes.cpu().numpy(), vals.cpu().numpy(), scores.cpu().numpy()


def _same_heaps(got, want):
    assert np.array_equal(got[0], want[0])
    for a in np.flatnonzero(want[0]):
        n = int(want[0][a])
        assert np.array_equal(got[1][a, :n], want[1][a, :n]), f"row {a}: heap values"
        assert np.array_equal(got[2][a, :n], want[2][a, :n], equal_nan=True), f"row {a}: scores"


def test_world1_count_owned_equals_count_device(pkg, torch_cuda):
    torch = torch_cuda
    from flink_cooccurrence_amd import _lib

    up, it, M = osm.log_a()
    dev = torch.device("cuda", 0)
    up_d, it_d = torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev)
    with pkg.CooccurrenceCore(n_items=M, device=0, output="csr") as core:
        whole = core.count_device(up_d, it_d)
        torch.cuda.current_stream().synchronize()
        w = _rows(whole, M)
        w_nnz, w_obs = int(whole.nnz), int(whole.observed)
        w_tk = core.topk_batch(osm.TOPK)
    ops, calls = _self_copy_ops(_lib)
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        core.comm_init_ops(0, 1, ops)
        res, info = core.count_owned(up_d, it_d)
        torch.cuda.current_stream().synchronize()
        assert calls == {"allreduce": 1, "allgather": 2, "alltoallv": 2}  # the agreement and the arenas; counts, records
        assert res.n_items == M and not res.dense and int(res.nnz) == w_nnz
        lens = np.diff(up)
        assert info.part == 0 and info.n_parts == 1 and info.gathered_bytes == 0
        assert info.observed == info.local_observed == int(res.observed) == w_obs == int(np.sum(lens * (lens - 1)))
        assert info.n_users_all == len(lens) and info.n_interactions_all == len(it)
        assert np.all(_d2h(info.owner, M, np.int32) == 0)
        assert np.array_equal(_d2h(info.item_counts, M, np.int64), np.bincount(it, minlength=M))
        for x, y in zip(_rows(res, M), w):
            assert np.array_equal(x, y)
        rs = torch.empty(M, dtype=torch.int64, device=dev)
        sizes = torch.empty(M, dtype=torch.int32, device=dev)
        vals = torch.zeros((M, osm.TOPK), dtype=torch.int32, device=dev)
        scores = torch.zeros((M, osm.TOPK), dtype=torch.float64, device=dev)
        core.topk_owned(osm.TOPK, sizes, vals, scores, rowsum_global=rs)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(rs.cpu().numpy(), w[3])
        _same_heaps((sizes.cpu().numpy(), vals.cpu().numpy(), scores.cpu().numpy()), w_tk)
        v = core.verify_batch()
        assert v["rows_bad_sum"] == 0 and v["rows_bad_entries"] == 0 and v["entries"] == w_nnz


def test_rescoring_a_small_csr_against_external_row_sums(pkg, torch_cuda):
    """no communicator: cooc_topk_batch_device over a small-universe CSR result, once with rowsum_global = the
    result's own row sums (the owners' path: the two passes, ascending columns, no column order) and once with
    rowsum_global = None; the heaps must be the same, bit for bit"""
    torch = torch_cuda
    up, it, M = osm.log_a()
    dev = torch.device("cuda", 0)
    with pkg.CooccurrenceCore(n_items=M, device=0, output="csr") as core:
        res = core.count_device(torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
        torch.cuda.current_stream().synchronize()
        assert not res.dense
        own = torch.empty(M, dtype=torch.int64, device=dev)
        core.copy_rowsum_device(own)
        plain = _topk_device(core, torch, M)
        external = _topk_device(core, torch, M, rowsum_global=own)
    assert plain[0].max() == osm.TOPK and np.count_nonzero(plain[0]) > 100
    _same_heaps(external, plain)


def test_count_owned_without_a_library_communicator_names_init_comm(pkg, torch_cuda):
    torch = torch_cuda
    from flink_cooccurrence_amd import sharding

    up, it, M = osm.log_a()
    dev = torch.device("cuda", 0)
    with pkg.CooccurrenceCore(n_items=M, device=0) as core:
        with pytest.raises(RuntimeError, match=r"init_comm .*init_comm_torch_ops"):
            sharding.count_owned(core, torch.from_numpy(up).to(dev), torch.from_numpy(it).to(dev))
