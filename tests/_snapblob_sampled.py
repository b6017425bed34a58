"""The sampled context's snapshot blob (format 2) restated in numpy: the container of _snapblob.py
(64-byte header, 40-byte directory entries, sections back to back in kind order, each 8-byte aligned and
zero-padded, splitmix checksums) with a magic of its own and 20 sections: the 15 of format 1, then the sampler's
scalars, the counted items and their int16 counters, the users with a total and their totals.  No library code is
involved: the tests build and take apart blobs from the format's description alone.  build() lays out whatever
sections it is given and seals them, so a blob whose sections break a relation or hold a bad value still carries
valid checksums, and the check under test is what has to refuse it."""
import struct

import numpy as np

import _snapblob as f1

HEADER, ENTRY, N_SECTIONS = 64, 40, 20
HEADER_BYTES = HEADER + ENTRY * N_SECTIONS  # 864
MAGIC, FORMAT = 0x32504D53434F4F43, 2  # "COOCSMP2"
SMP_SCALARS, SMP_ITEM_IDS, SMP_ITEM_CNTS, SMP_USER_IDS, SMP_TOTALS = range(16, 21)
DTYPES = dict(f1.DTYPES)
DTYPES.update({SMP_SCALARS: "<i8", SMP_ITEM_IDS: "<i4", SMP_ITEM_CNTS: "<i2", SMP_USER_IDS: "<i4", SMP_TOTALS: "<i4"})
# the sampler scalar section's words
ITEM_CUT, SEED, REJECTED, FILLS, REPLACEMENTS, FEEDBACKS = range(6)
SMP_SCALAR_WORDS = 8

checksum = f1.checksum


def parse(blob: bytes):
    """-> (fields, sections) as _snapblob.parse, for a format-2 blob"""
    magic, fmt, n_sec, total, n_items, user_cut, window, rank, world, _, reserved = struct.unpack_from("<QiiqiiqiiQQ", blob, 0)
    assert (magic, fmt, n_sec, total, reserved) == (MAGIC, FORMAT, N_SECTIONS, len(blob), 0)
    fields = dict(n_items=n_items, user_cut=user_cut, window_size_ms=window, rank=rank, world=world)
    sections = {}
    for k in range(N_SECTIONS):
        kind, elem, off, nbytes, count, _ = struct.unpack_from("<iiqqqQ", blob, HEADER + ENTRY * k)
        assert kind == k + 1 and elem == np.dtype(DTYPES[kind]).itemsize and nbytes == count * elem
        sections[kind] = np.frombuffer(blob, DTYPES[kind], count, off).copy()
    return fields, sections


def build(fields, sections, *, magic=MAGIC, fmt=FORMAT) -> bytes:
    """The canonical blob of these header fields and 20 sections, checksummed, the header sealed last."""
    body, entries, off = [], [], HEADER_BYTES
    for kind in range(1, N_SECTIONS + 1):
        a = np.ascontiguousarray(sections[kind], DTYPES[kind])
        raw = a.tobytes()
        raw += bytes(-len(raw) % 8)
        entries.append((kind, a.dtype.itemsize, off, a.nbytes, len(a), checksum(raw)))
        body.append(raw)
        off += len(raw)
    head = bytearray(HEADER_BYTES)
    struct.pack_into("<QiiqiiqiiQQ", head, 0, magic, fmt, N_SECTIONS, off, fields["n_items"], fields["user_cut"],
                     fields["window_size_ms"], fields["rank"], fields["world"], 0, 0)
    for k, e in enumerate(entries):
        struct.pack_into("<iiqqqQ", head, HEADER + ENTRY * k, *e)
    struct.pack_into("<Q", head, 48, checksum(bytes(head)))
    return bytes(head) + b"".join(body)


def empty_sections(item_cut: int, seed: int):
    s = f1.empty_sections()
    for k in (SMP_ITEM_IDS, SMP_ITEM_CNTS, SMP_USER_IDS, SMP_TOTALS):
        s[k] = np.zeros(0, DTYPES[k])
    s[SMP_SCALARS] = np.zeros(SMP_SCALAR_WORDS, "<i8")
    s[SMP_SCALARS][ITEM_CUT] = item_cut
    s[SMP_SCALARS][SEED] = np.array(seed & (2**64 - 1), np.uint64).astype(np.int64)
    return s


def example(n_items=50, user_cut=4, item_cut=20, seed=0xC0FFEE, window_size_ms=1000):
    """A small consistent state written down by hand: three users with a total (7 has no history), two global rows,
    three counted items, one pending window."""
    fields = dict(n_items=n_items, user_cut=user_cut, window_size_ms=window_size_ms, rank=0, world=1)
    s = empty_sections(item_cut, seed)
    s[f1.USER_IDS] = np.array([3, 9], "<i4")
    s[f1.HIST_PTR] = np.array([0, 2, 3], "<i8")
    s[f1.HIST_ITEMS] = np.array([1, 2, 5], "<i4")
    s[f1.ROW_IDS] = np.array([1, 2], "<i4")
    s[f1.ROW_PTR] = np.array([0, 1, 2], "<i8")
    s[f1.ROW_COLS] = np.array([2, 1], "<i4")
    s[f1.ROW_CNTS] = np.array([1, 1], "<u4")
    s[f1.ROW_SUMS] = np.array([1, 1], "<i8")
    s[f1.PEND_TS] = np.array([4999], "<i8")
    s[f1.PEND_PTR] = np.array([0, 2], "<i8")
    s[f1.PEND_USERS] = np.array([3, 11], "<i4")
    s[f1.PEND_ITEMS] = np.array([4, 4], "<i4")
    s[f1.SCALARS][f1.WATERMARK] = 3999
    s[f1.SCALARS][f1.OBSERVED_EXACT] = 2
    s[f1.SCALARS][f1.OBSERVED_REF] = 2
    s[f1.SCALARS][f1.SCAL2] = 2
    s[f1.SCALARS][f1.SCAL3] = 2
    s[SMP_SCALARS][REJECTED] = 2
    s[SMP_SCALARS][FILLS] = 3
    s[SMP_ITEM_IDS] = np.array([1, 2, 5], "<i4")
    s[SMP_ITEM_CNTS] = np.array([1, 1, 1], "<i2")
    s[SMP_USER_IDS] = np.array([3, 7, 9], "<i4")
    s[SMP_TOTALS] = np.array([2, 2, 1], "<i4")
    return fields, s
