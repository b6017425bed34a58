"""cooc_sample_device without a GPU: the symbol is declared and exported, its info struct is the header's 64 bytes,
the binding carries it, and the additive entry point leaves the ABI version alone."""
import ctypes


def test_symbol_struct_and_abi(pkg):
    from flink_cooccurrence_amd import _lib

    L = pkg.load_library()
    assert "cooc_sample_device" in pkg.header_symbols()
    assert getattr(L, "cooc_sample_device").argtypes is not None
    assert len(L.cooc_sample_device.argtypes) == 17
    assert ctypes.sizeof(_lib.CoocSampleInfo) == 64
    assert [n for n, _ in _lib.CoocSampleInfo._fields_] == [
        "rejected", "fills", "replacements", "feedbacks", "users", "item_counter_sum", "reservoir_items", "reserved"]
    assert L.cooc_abi_version() == 7
    assert hasattr(pkg.CooccurrenceCore, "sample_device")


def test_header_documents_the_struct(pkg):
    """the header's struct has the binding's eight int64 fields, in order"""
    import re

    from flink_cooccurrence_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct cooc_sample_info \{(.*?)\} cooc_sample_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int64_t\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.CoocSampleInfo._fields_]
