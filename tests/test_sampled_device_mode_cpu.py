"""cooc_sampling_enable_device without a GPU: the entry point is declared in the header, exported and bound like
cooc_sampling_enable, the additive entry point leaves the ABI version alone, and CooccurrenceCore validates
sample_on before it touches the library."""
import ctypes
import inspect

import pytest


def test_symbol_binding_and_abi(pkg):
    L = pkg.load_library()
    assert "cooc_sampling_enable_device" in pkg.header_symbols()
    assert L.cooc_sampling_enable_device.argtypes == L.cooc_sampling_enable.argtypes
    assert L.cooc_sampling_enable_device.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64]
    assert L.cooc_sampling_enable_device.restype is ctypes.c_int
    assert L.cooc_abi_version() == 7
    assert L.cooc_sampling_enable_device(None, 5, 1) != 0  # a NULL context is an argument error, not a crash


def test_sample_on_keyword(pkg):
    from flink_cooccurrence_amd._lib import IllegalArgumentException

    assert inspect.signature(pkg.CooccurrenceCore.__init__).parameters["sample_on"].default == "host"
    with pytest.raises(IllegalArgumentException, match="sample_on"):
        pkg.CooccurrenceCore(n_items=16, user_cut=3, item_cut=5, sample_on="bogus")
    with pytest.raises(IllegalArgumentException, match="sample_on"):  # also when the sampled mode is off
        pkg.CooccurrenceCore(n_items=16, sample_on="gpu")
    ops = [c for _, c in inspect.getmembers(pkg, inspect.isclass)
           if "sample_seed" in inspect.signature(c.__init__).parameters]
    assert len(ops) >= 2  # the core and the operator mirror that forwards to it
    assert all(inspect.signature(c.__init__).parameters["sample_on"].default == "host" for c in ops)
