"""A numpy model of the owner-partitioned exchange of partial rows (cooc_shard.hip: k_permute_nnz, k_pack_entries,
k_pack_entries_dense and the two merges behind Sharder::merge), written from the contract in include/cooc.h and not
from what the library returns:

  owner(a)       = a mod n                           row a's owner among n parts
  rows_owned     = the a = p, p + n, p + 2 n, .. < M
  perm_index(a)  = (rows of the owners before owner(a)) + a div n      owner-major, then ascending row
  an entry       = col << 32 | cnt                   cnt a uint32, a signed net in two's complement
  a merged count = the sources' counts summed modulo 2^32
  a merged key   = unsigned: its summed count is nonzero; signed nets: any source sent it (also at net 0)
  a row sum      = unsigned: the merged counts summed; signed nets: summed after sign extension from 32 bits

The merge has two implementations behind one call: one dense LDS row per owned row while 4 M bytes (signed nets:
plus 4 ceil(M / 32) of touched bits) fit DENSE_MAX_BYTES, else a sort by (owned row << 32 | col) over kb key bits
and a sum by key.  merge_path and sort_key_bits restate that choice for the tests' shape claims.
"""
from collections import namedtuple

import numpy as np

DENSE_MAX_BYTES = 160 * 1024 - 1024   # kMergeDenseMaxBytes
MERGE_WAVES = 16                      # k_merge_rows, k_pack_entries_dense: 1024 threads

Packed = namedtuple("Packed", "row_nnz part_entries entries")
Merged = namedtuple("Merged", "row_ptr cols cnt rowsum")   # a CSR over the owned rows


def rows_owned(M, n, p):
    return len(range(p, M, n))


def perm_index(a, M, n):
    a = np.asarray(a, np.int64)
    owned = np.array([rows_owned(M, n, o) for o in range(min(n, M + 1))], np.int64)
    before = np.concatenate([[0], np.cumsum(owned)])
    return before[a % n] + a // n


def pack(row_ptr, cols, cnt, M, n):
    """A sorted CSR of M rows -> (row lengths in (owner, row) order, entries per owner, packed entries in that
    order)."""
    rp = np.asarray(row_ptr, np.int64)
    nnz = np.diff(rp)
    order = np.concatenate([np.arange(o, M, n, dtype=np.int64) for o in range(n)]) if M else np.zeros(0, np.int64)
    e = np.asarray(cols).astype(np.uint64) << np.uint64(32)
    e |= np.asarray(cnt).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    idx = np.repeat(rp[order], nnz[order]) + _ramp(nnz[order])
    part = np.zeros(n, np.int64)
    np.add.at(part, order % n, nnz[order])
    return Packed(nnz[order].astype(np.int32), part, e[idx])


def _ramp(lens):
    """0 .. l - 1 for every l of lens, concatenated."""
    lens = np.asarray(lens, np.int64)
    return np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)


def sorted_keys(M, n, part, recv_nnz, recv_entries):
    """The received entries as the sorted merge sees them: their keys (owned row << 32 | col) in ascending order,
    equal keys in source order, and the counts in that order."""
    R = rows_owned(M, n, part)
    nnz = np.asarray(recv_nnz, np.int64)
    assert len(nnz) == n * R
    e = np.zeros(0, np.uint64) if recv_entries is None else np.asarray(recv_entries).view(np.uint64)
    assert len(e) == int(nnz.sum())
    r = np.repeat(np.arange(n * R, dtype=np.int64) % max(R, 1), nnz).astype(np.uint64)
    key = (r << np.uint64(32)) | (e >> np.uint64(32))
    order = np.argsort(key, kind="stable")
    return key[order], e[order] & np.uint64(0xFFFFFFFF)


def merge(M, n, part, recv_nnz, recv_entries, signed):
    """recv_nnz int32 [n * R] and recv_entries uint64, both source-major -> Merged over the R owned rows."""
    R = rows_owned(M, n, part)
    key, val = sorted_keys(M, n, part, recv_nnz, recv_entries)
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    ukey = key[first]
    usum = (np.add.reduceat(val, first) if len(key) else val) & np.uint64(0xFFFFFFFF)
    if not signed:
        keep = usum != 0
        ukey, usum = ukey[keep], usum[keep]
    urow = (ukey >> np.uint64(32)).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(urow, minlength=R))]).astype(np.int64)
    cnt = usum.astype(np.uint32)
    summand = cnt.view(np.int32).astype(np.int64) if signed else cnt.astype(np.int64)
    rowsum = np.zeros(R, np.int64)
    np.add.at(rowsum, urow, summand)
    return Merged(row_ptr, (ukey & np.uint64(0xFFFFFFFF)).astype(np.int32), cnt, rowsum)


def merge_path(M, signed):
    """"dense" or "sorted": which implementation a context of M items merges with."""
    lds = 4 * M + (4 * ((M + 31) // 32) if signed else 0)
    return "sorted" if lds > DENSE_MAX_BYTES else "dense"


def sort_key_bits(R):
    """Key bits the sorted merge has to sort by: 32 of the column and those of the owned row indices 0 .. R - 1
    (one at the least)."""
    return 32 + max(1, int(R - 1).bit_length())


def wave_ranges(M):
    """The column ranges [lo, hi) of the 16 waves of the dense merge's compaction (empty ones included)."""
    per = (-(-M // MERGE_WAVES) + 63) & ~63
    return [(min(M, w * per), min(M, (w + 1) * per)) for w in range(MERGE_WAVES)]
