"""CPU-only: the ctypes declarations of FACET in a batch (mgx_facet_request, mgx_facet_entry, mgx_facet_view in
mygram_db_amd/_capi.py) against include/mygram_gpu.h, by the method of test_capi_structs_cpu.py: equal field names, order
and sizes; and the constants both sides state."""
import ctypes as C
import re

import test_capi_structs_cpu as base
from pkg import mg

STRUCTS = {"mgx_facet_request": "FacetRequest", "mgx_facet_entry": "FacetEntry", "mgx_facet_view": "FacetView"}


def test_facet_structs_match_the_header():
    src = base._header()
    for cname, pyname in STRUCTS.items():
        want = base._fields(src, cname)
        cls = getattr(mg._capi, pyname)
        got = [(f[0], C.sizeof(f[1])) for f in cls._fields_]
        assert got == want, cname
    assert C.sizeof(mg._capi.FacetRequest) == 16 and C.sizeof(mg._capi.FacetEntry) == 24 and C.sizeof(mg._capi.FacetView) == 16


def test_facet_constants_match_the_header():
    src = base._header()
    assert int(re.search(r"#define MGX_FACET_MAX_COLUMNS (\d+)u", src).group(1)) == mg._capi.FACET_MAX_COLUMNS == 8
    assert 256 << 20 == mg._capi.FACET_ARENA_CAP and "#define MGX_FACET_ARENA_CAP (256ull << 20)" in src
    bins = int(re.search(r"#define MGX_FACET_LDS_BINS (\d+)u", src).group(1))
    assert bins == mg._capi.FACET_LDS_BINS
    # the planner's own constants are the header's
    hpp = open(base.os.path.join(base.ROOT, "mygram-db_amd", "csrc", "mgx_facet.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kLdsBins = (\d+);", hpp).group(1)) == bins
    assert int(re.search(r"constexpr uint32_t kMaxColumns = (\d+);", hpp).group(1)) == 8
    assert "constexpr uint64_t kArenaCap = 256ull << 20;" in hpp
    assert bins * 4 * 2 <= 160 * 1024  # two workgroups' histograms fit a CU's LDS


def test_abi_version_is_unchanged():
    assert mg._capi.ABI_VERSION == 5
