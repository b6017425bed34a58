"""cooc_parse_interactions_device == cooc_parse_interactions, byte for byte: the same arrays on valid texts, the
same status and bad line on every dictated reject (fixtures: tests/_log_model.py, checked on the CPU by
tests/test_ingest_device_cpu.py)."""
import ctypes

import numpy as np
import pytest

import _log_model as lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """torch's runtime comes up before the library's first context, as in the other device-tensor tests"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def core(pkg, torch_cuda):
    with pkg.CooccurrenceCore(n_items=300) as c:
        yield c


def _raw(core, text: bytes, cap=None, fill=True, offset=0):
    """One C call on `text` placed `offset` bytes into a device buffer -> (status, n_records, bad_line, arrays)"""
    import torch

    from flink_cooccurrence_amd import _lib

    dev = torch.device("cuda:0")
    buf = torch.zeros(len(text) + offset + 1, dtype=torch.uint8, device=dev)
    if text:
        buf[offset:offset + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    n_host = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    cap = n_host if cap is None else cap
    users = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev)
    items = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev)
    ts = torch.full((max(cap, 1),), -7, dtype=torch.int64, device=dev)
    n, bad = ctypes.c_int64(-5), ctypes.c_int64(-5)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if fill else None  # noqa: E731
    st = _lib.load().cooc_parse_interactions_device(
        core._h, ctypes.c_void_p(buf.data_ptr() + offset) if text else None, len(text), cap, p(users), p(items),
        p(ts), None, ctypes.byref(n), ctypes.byref(bad))
    torch.cuda.synchronize()
    return st, n.value, bad.value, (users.cpu().numpy(), items.cpu().numpy(), ts.cpu().numpy())


def _host(pkg, text):
    from flink_cooccurrence_amd import _lib
    from flink_cooccurrence_amd.core import _p

    L = _lib.load()
    n, bad = ctypes.c_int64(-5), ctypes.c_int64(-5)
    cap = text.count(b"\n") + 1
    u, i, t = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
    st = L.cooc_parse_interactions(text, len(text), cap, _p(u, _lib.i32p), _p(i, _lib.i32p), _p(t, _lib.i64p),
                                   ctypes.byref(n), ctypes.byref(bad))
    return st, n.value, bad.value, (u, i, t)


@pytest.mark.parametrize("which", ["cycling", "special", "long_line"])
def test_valid_text_equals_host(pkg, core, which):
    text = {"cycling": lm.cycling_text(), "special": lm.SPECIAL_TEXT, "long_line": lm.LONG_LINE_TEXT}[which]
    hs, hn, hb, harr = _host(pkg, text)
    assert hs == 0 and hb == -1
    for offset in (0, 5):  # a text that starts off the 16-B grid parses the same
        st, n, bad, arr = _raw(core, text, offset=offset)
        assert (st, n, bad) == (0, hn, -1)
        for g, h in zip(arr, harr):
            assert np.array_equal(g[:n], h[:hn])
    # count-only mode, and a capacity one short
    assert _raw(core, text, fill=False)[:3] == (0, hn, -1)
    st, _, bad, _ = _raw(core, text, cap=hn - 1)
    assert st == 1 and bad == -1
    # the Python surface: device tensors from a device tensor and from bytes
    got = core.parse_interactions_device(text)
    assert [str(x.dtype) for x in got] == ["torch.int32", "torch.int32", "torch.int64"] and got[0].is_cuda
    for g, h in zip(got, harr):
        assert np.array_equal(g.cpu().numpy(), h[:hn])


def test_empty_and_lone_newline(pkg, core):
    from flink_cooccurrence_amd import _lib

    assert _raw(core, b"")[:3] == (0, 0, -1)
    assert _raw(core, b"", fill=False)[:3] == (0, 0, -1)
    assert _host(pkg, b"\n")[0] == 1 and _host(pkg, b"\n")[2] == 0
    st, _, bad, _ = _raw(core, b"\n")
    assert (st, bad) == (1, 0)  # one empty line, bad line 0
    assert _raw(core, b"\n", fill=False)[:2] == (0, 1)
    assert [x.numel() for x in core.parse_interactions_device(b"")] == [0, 0, 0]
    with pytest.raises(_lib.IllegalArgumentException, match="line 0 "):
        core.parse_interactions_device(b"\n")
    assert _raw(core, b"1,2,3")[:3] == (0, 1, -1)  # the context stays usable


@pytest.mark.parametrize("name", sorted(lm.REJECTS))
def test_rejects_equal_host(pkg, core, name):
    for at in (0, lm.N_VALID // 2, lm.N_VALID - 1):
        text = lm.reject_text(lm.REJECTS[name], at)
        hs, _, hb, _ = _host(pkg, text)
        st, _, bad, _ = _raw(core, text)
        assert (hs, hb) == (1, at) and (st, bad) == (hs, hb)
    # two rejects in one text: the smaller index
    text = lm.reject_text(lm.REJECTS[name], 6, lm.REJECTS["letter"], 2)
    assert _host(pkg, text)[2] == 2 and _raw(core, text)[2] == 2
    # a reject below the capacity wins over the capacity; above it, the capacity is the error
    assert _raw(core, lm.reject_text(lm.REJECTS[name], 2), cap=4)[2] == 2
    st, _, bad, _ = _raw(core, lm.reject_text(lm.REJECTS[name], 6), cap=4)
    assert (st, bad) == (1, -1)


def test_two_calls_are_bit_identical(core):
    text = lm.cycling_text()
    a, b = _raw(core, text), _raw(core, text)
    assert a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
