"""CPU-only: the ctypes declarations of page documents (mgx_document_request, mgx_document_entry, mgx_document_view in
mygram_db_amd/_capi.py) against include/mygram_gpu.h, by the method of test_capi_structs_cpu.py: equal field names, order
and sizes; and the constants both sides and the planner state."""
import ctypes as C
import re

import test_capi_structs_cpu as base
from pkg import mg

STRUCTS = {"mgx_document_request": "DocumentRequest", "mgx_document_entry": "DocumentEntry",
           "mgx_document_view": "DocumentView", "mgx_document_record_header": "DocumentRecordHeader"}
NAMES = ["mgx_index_attach_primary_key_bytes", "mgx_index_max_primary_key_bytes", "mgx_batch_set_documents",
         "mgx_batch_defer_documents", "mgx_batch_fetch_documents", "mgx_documents_gather"]


def test_document_structs_match_the_header():
    src = base._header()
    for cname, pyname in STRUCTS.items():
        want = base._fields(src, cname)
        cls = getattr(mg._capi, pyname)
        got = [(f[0], C.sizeof(f[1])) for f in cls._fields_]
        assert got == want, cname
    assert C.sizeof(mg._capi.DocumentRequest) == 16 and C.sizeof(mg._capi.DocumentEntry) == 32
    assert C.sizeof(mg._capi.DocumentView) == 16 and C.sizeof(mg._capi.DocumentRecordHeader) == 16


def test_document_constants_match_the_header():
    src = base._header()
    cap = mg._capi
    assert int(re.search(r"#define MGX_DOC_MAX_COLUMNS (\d+)u", src).group(1)) == cap.DOC_MAX_COLUMNS == 32
    assert int(re.search(r"#define MGX_DOC_MAX_LIMIT (\d+)u", src).group(1)) == cap.DOC_MAX_LIMIT == 1024
    assert "#define MGX_DOC_ARENA_CAP (256ull << 20)" in src and cap.DOC_ARENA_CAP == 256 << 20
    assert int(re.search(r"#define MGX_DOC_NO_COLUMN (0x[0-9A-F]+)u", src).group(1), 16) == cap.DOC_NO_COLUMN == 0xFFFFFFFF
    flags = {n: int(re.search(r"#define MGX_DOC_%s (\d+)u" % n, src).group(1)) for n in ("FOUND", "HAS_KEY", "MAPPED")}
    assert (flags["FOUND"], flags["HAS_KEY"], flags["MAPPED"]) == (cap.DOC_FOUND, cap.DOC_HAS_KEY, cap.DOC_MAPPED) == (1, 2, 4)
    # the planner's own constants are the header's
    hpp = open(base.os.path.join(base.ROOT, "mygram-db_amd", "csrc", "mgx_documents.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kMaxColumns = (\d+);", hpp).group(1)) == 32
    assert int(re.search(r"constexpr uint32_t kMaxLimit = (\d+);", hpp).group(1)) == 1024
    assert "constexpr uint64_t kArenaCap = 256ull << 20;" in hpp
    assert "constexpr uint32_t kFound = 1u, kHasKey = 2u, kMapped = 4u;" in hpp


def test_document_entry_points_are_declared_on_both_sides():
    src = base._header()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in mg._capi.EXPORTS, name


def test_abi_version_is_unchanged():
    assert mg._capi.ABI_VERSION == 5
    assert int(re.search(r"#define MGX_ABI_VERSION (\d+)U", base._header()).group(1)) == 5
