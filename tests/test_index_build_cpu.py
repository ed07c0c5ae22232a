"""CPU-only: the host side of mgx_index_build_device. Every refusal that needs no device answers without one, with its own
code and with both outputs NULL; a valid request without a device is the library's "no CPU fallback" error. The plain
arithmetic of the resident ending (mygram-db_amd/csrc/mgx_build.hpp: PlanResident) is checked by
tests/cpp/resident_plan_check.cpp, a stand-alone program built here with g++ and -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pkg import ROOT, mg

K = mg._capi
INVALID, OUT_OF_RANGE, NOT_IMPLEMENTED, INTERNAL = 2, 3, 4, 5


def _params(ngram=2, kanji=0, cross=1, size=None, version=None):
    return K.BuildParams(C.sizeof(K.BuildParams) if size is None else size, K.ABI_VERSION if version is None else version,
                         ngram, kanji, cross, 0)


def _desc(device=0, tile_shift=0, attach_text=1, size=None, version=None):
    return K.IndexBuildDesc(C.sizeof(K.IndexBuildDesc) if size is None else size,
                            K.ABI_VERSION if version is None else version, device, tile_shift, 0.0, attach_text, 0)


def _corpus(texts=("abc", "bcd")):
    c = mg.Corpus.from_texts(list(texts))
    return c, c.text_bytes.ctypes.data, c.text_off.ctypes.data


def _call(params, desc, text_bytes, text_off, first, n_docs, outs=(True, True)):
    L = K.load()
    ch, ih = C.c_void_p(0x1234), C.c_void_p(0x5678)
    rc = L.mgx_index_build_device(C.byref(params) if params is not None else None, C.byref(desc) if desc is not None else None,
                                  text_bytes, text_off, first, n_docs, C.byref(ch) if outs[0] else None,
                                  C.byref(ih) if outs[1] else None)
    msg = L.mgx_last_error().decode()
    if rc != 0:  # on any failure both outputs are NULL
        assert (ch.value is None or not outs[0]) and (ih.value is None or not outs[1]), (rc, msg)
    return rc, msg, ch, ih


def test_exports_declared_and_the_descriptor_layout():
    L = K.load()
    src = open(os.path.join(ROOT, "include", "mygram_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("mgx_index_build_device", 8), ("mgx_index_read_postings", 6)):
        assert name in K.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
        assert len(getattr(L, name).argtypes) == n_args
    assert L.mgx_abi_version() == 5
    # struct_size, version, device, tile_shift | dense_threshold | attach_text, reserved
    assert C.sizeof(K.IndexBuildDesc) == 32
    assert K.IndexBuildDesc.dense_threshold.offset == 16 and K.IndexBuildDesc.attach_text.offset == 24
    assert re.search(r"typedef struct mgx_index_build_desc \{[^}]*uint32_t attach_text;[^}]*uint32_t reserved;[^}]*\}", src)


def test_null_arguments_and_bad_structs_are_invalid_arguments():
    c, tb, to = _corpus()
    for args in ((None, _desc(), tb, to, 1, 2), (_params(), None, tb, to, 1, 2), (_params(), _desc(), tb, None, 1, 2),
                 (_params(), _desc(), None, to, 1, 2)):
        rc, msg, _, _ = _call(*args)
        assert rc == INVALID and "mgx_index_build_device: null argument" in msg, (rc, msg)
    for outs in ((False, True), (True, False)):
        rc, msg, _, _ = _call(_params(), _desc(), tb, to, 1, 2, outs=outs)
        assert rc == INVALID and "null argument" in msg
    for p, d in ((_params(size=4), _desc()), (_params(version=K.ABI_VERSION + 1), _desc()), (_params(), _desc(size=8)),
                 (_params(), _desc(version=K.ABI_VERSION - 1))):
        rc, msg, _, _ = _call(p, d, tb, to, 1, 2)
        assert rc == INVALID and "bad struct_size/version" in msg, (rc, msg)


def test_the_refusals_of_the_device_column_builder_keep_their_codes_and_order():
    c, tb, to = _corpus()
    rc, msg, _, _ = _call(_params(ngram=4), _desc(), tb, to, 2**32 - 2, 2)  # doc ids before the n-gram limit
    assert rc == OUT_OF_RANGE and "doc ids exceed uint32" in msg
    for ngram, kanji in ((4, 0), (2, 4), (7, 7)):
        rc, msg, _, _ = _call(_params(ngram=ngram, kanji=kanji), _desc(), tb, to, 1, 2)
        assert rc == NOT_IMPLEMENTED and "3 code points" in msg, (rc, msg)
    off = np.asarray([0, 5, 3], dtype=np.uint64)
    rc, msg, _, _ = _call(_params(), _desc(), tb, off.ctypes.data, 1, 2)
    assert rc == INVALID and "text_off descends" in msg
    # each answers what mgx_columns_build_device answers for the same arguments
    L = K.load()
    h = C.c_void_p()
    for p, o, first in ((_params(ngram=4), to, 2**32 - 2), (_params(ngram=4), to, 1), (_params(), off.ctypes.data, 1)):
        want = L.mgx_columns_build_device(C.byref(p), tb, o, first, 2, 0, C.byref(h))
        rc, _, _, _ = _call(p, _desc(), tb, o, first, 2)
        assert rc == want and want != 0


def test_what_mgx_index_create_refuses_for_the_host_columns_is_refused_alike():
    L = K.load()
    c, tb, to = _corpus()
    host = mg.Columns(c, 1, 2, 0, True)
    v = host.view

    def create(tile_shift, cols_view):
        d = K.IndexDesc(C.sizeof(K.IndexDesc), K.ABI_VERSION, 0, tile_shift, cols_view.first_doc_id, cols_view.n_docs,
                        cols_view.n_grams, cols_view.offsets, cols_view.docids, cols_view.tf, cols_view.doc_len, 0.0,
                        cols_view.tf_overflow_pos, cols_view.tf_overflow_val, cols_view.n_tf_overflow)
        h = C.c_void_p()
        return L.mgx_index_create(C.byref(d), C.byref(h))

    for shift in (13, 15, 1):
        want = create(shift, v)
        rc, msg, _, _ = _call(_params(), _desc(tile_shift=shift), tb, to, 1, 2)
        assert rc == want == NOT_IMPLEMENTED and "tile_shift" in msg, (rc, want, msg)
    e, etb, eto = _corpus([])
    empty = mg.Columns(e, 1, 2, 0, True)
    want = create(0, empty.view)
    rc, msg, _, _ = _call(_params(), _desc(), etb, eto, 1, 0)
    assert rc == want == OUT_OF_RANGE and "n_docs" in msg, (rc, want, msg)


def test_a_valid_request_without_a_device_has_no_cpu_fallback():
    L = K.load()
    if L.mgx_device_count() > 0:
        pytest.skip("a device is present")
    c, tb, to = _corpus()
    for attach in (0, 1):
        rc, msg, ch, ih = _call(_params(), _desc(attach_text=attach), tb, to, 1, 2)
        assert rc == INTERNAL and "no HIP device available" in msg and "no CPU fallback" in msg
        assert ch.value is None and ih.value is None
    rc, msg, _, _ = _call(_params(), _desc(device=-1), tb, to, 1, 2)  # (the device ordinal is checked against a device count)
    assert rc == INTERNAL and "no CPU fallback" in msg
    with pytest.raises(K.MgxError) as e:
        mg.DeviceIndex.build_resident(c, 1, 2, 0, True)
    assert e.value.code == INTERNAL
    with pytest.raises(K.MgxError) as e:
        mg.Index(corpus=c, build_device=0, resident=True)
    assert e.value.code == INTERNAL


def test_read_postings_null_arguments():
    L = K.load()
    n = C.c_uint64(7)
    assert L.mgx_index_read_postings(None, 0, None, None, 0, C.byref(n)) == INVALID
    assert "mgx_index_read_postings: null argument" in L.mgx_last_error().decode()


def test_python_and_shim_layers_carry_the_mode():
    import inspect
    from mygram_db_amd import _shim_capi as S
    assert inspect.signature(mg.Index.__init__).parameters["resident"].default is False
    assert callable(mg.DeviceIndex.read_postings) and callable(mg.DeviceIndex.build_resident)
    for name in ("mgxs_table_set_build_mode", "mgxs_table_build_counters"):
        assert name in S.EXPORTS and hasattr(S.load(), name)
    assert S.load().mgxs_table_set_build_mode(None, 2) == INVALID
    assert S.load().mgxs_table_build_counters(None, None, None, None) == INVALID
    assert (S.Table.BUILD_HOST, S.Table.BUILD_DEVICE_COLUMNS, S.Table.BUILD_DEVICE_RESIDENT) == (0, 1, 2)
    with pytest.raises(ValueError):
        mg.Index(texts=["abc"], resident=True)  # resident needs the device that builds


def test_the_resident_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "resident_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "resident_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("resident plan ok: ")
    assert int(r.stdout.split()[3]) > 10_000
