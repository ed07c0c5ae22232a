"""CPU-only: the ctypes declarations of the C ABI's structs (mygram_db_amd/_capi.py) against include/mygram_gpu.h —
field names, order and sizes of every struct both sides declare, mgx_query and mgx_condition among them, and the ABI
version. (ctypes lays a Structure out with the platform's natural alignment, as the C compiler does: equal names, order
and field sizes mean equal offsets.)"""
import ctypes as C
import os
import re

from pkg import ROOT, mg

STRUCTS = {"mgx_build_params": "BuildParams", "mgx_mgix_info": "MgixInfo", "mgx_columns_view": "ColumnsView",
           "mgx_index_desc": "IndexDesc", "mgx_term": "Term", "mgx_filter": "Filter", "mgx_condition": "Condition",
           "mgx_query": "Query", "mgx_dump_view": "DumpView", "mgx_dump_filter_column": "DumpFilterColumn",
           "mgx_filter_column_desc": "FilterColumnDesc", "mgx_expr_token": "ExprToken", "mgx_query_result": "QueryResult",
           "mgx_result_view": "ResultView", "mgx_highlight_request": "HighlightRequest",
           "mgx_highlight_entry": "HighlightEntry", "mgx_highlight_view": "HighlightView"}
SIZES = {"uint8_t": 1, "uint32_t": 4, "int32_t": 4, "int": 4, "uint64_t": 8, "double": 8, "size_t": C.sizeof(C.c_size_t)}


def _header():
    src = open(os.path.join(ROOT, "include", "mygram_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _fields(src, name):
    """[(field, size in bytes)] of `typedef struct name { ... } name;`"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(?:const )?(?:struct )?(\w+)\s*(.*)", decl)
        ctype, rest = m.group(1), m.group(2)
        for part in rest.split(","):
            part = part.strip()
            arr = re.search(r"\[(\d+)\]", part)
            field = re.sub(r"\[.*\]", "", part).replace("const", "").replace("*", "").strip()
            if "*" in part:
                size = C.sizeof(C.c_void_p)
            elif ctype in STRUCTS:
                size = C.sizeof(getattr(mg._capi, STRUCTS[ctype]))
            else:
                size = (SIZES[ctype] if ctype != "char" else 1) * (int(arr.group(1)) if arr else 1)
            out.append((field, size))
    return out


def test_abi_version_matches_the_header():
    m = re.search(r"#define MGX_ABI_VERSION (\d+)U", _header())
    assert int(m.group(1)) == mg._capi.ABI_VERSION == 5


def test_ctypes_structs_match_the_header():
    src = _header()
    for cname, pyname in STRUCTS.items():
        want = _fields(src, cname)
        cls = getattr(mg._capi, pyname)
        got = [(f[0], C.sizeof(f[1])) for f in cls._fields_]
        assert got == want, cname


def test_query_carries_conditions_last():
    q = mg._capi.Query
    assert [f[0] for f in q._fields_][-2:] == ["conditions", "n_conditions"]
    assert q.conditions.offset == (q.fuzzy_verify_distance.offset + 4 + 7) // 8 * 8  # (appended: earlier fields keep their place)
    assert q.conditions.size == C.sizeof(C.c_void_p)
    cond = mg._capi.Condition
    assert C.sizeof(cond) == 40
    assert [(f, getattr(cond, f).offset) for f, _ in cond._fields_] == [
        ("column_id", 0), ("op", 4), ("literal_bits", 8), ("eq_epsilon", 16), ("null_matches", 24), ("never_matches", 28),
        ("negate", 32), ("reserved", 36)]
    cap = re.search(r"#define MGX_CONDITION_ARENA_MAX_BYTES \(1ull << (\d+)\)", _header())
    assert 1 << int(cap.group(1)) == mg._capi.CONDITION_ARENA_MAX_BYTES
