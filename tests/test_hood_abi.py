"""The C entries of the hood-rows block (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument
check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("wgnn_hood_rows_count", "wgnn_hood_rows_fill")
BITS = ("BAD_INDEX", "BAD_ROWPTR", "BAD_COL", "BAD_SIZE")


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1])
    for bit in BITS + ("MAX_MEMBERS", "MAX_SLAB_GENES"):
        assert int(re.search(r"#define\s+WGNN_HOOD_%s\s+(\d+)" % bit, text).group(1)) == getattr(_lib, "HOOD_" + bit)
    bits = {getattr(_lib, "HOOD_" + bit) for bit in BITS}
    assert bits == {1, 2, 4, 8} and _lib.HOOD_MAX_MEMBERS == 256 and _lib.HOOD_MAX_SLAB_GENES == 16384
    assert {bit for bit, _ in ops._HOOD_STATUS} == bits and all(text for _, text in ops._HOOD_STATUS)      # a text per bit
    assert api.SMOOTH_MAX_NEIGHBORS == _lib.HOOD_MAX_MEMBERS - 1 and api.SMOOTH_CHUNK_BYTES == 256 << 20
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.hood_rows is ops.hood_rows and sda.Smoothed is api.Smoothed and {"hood_rows", "Smoothed"} <= set(sda.__all__)
    assert callable(sda.ResidentPredictor.smooth) and callable(sda.ResidentPredictor.smooth_file) and callable(api._neighbor_lists)
    from scdeepsort_amd import build
    assert "wgnn_hood.hip" in [p.name for p in build.SRC]
    code = lambda name: re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / name).read_text())
    src = code("wgnn_hood.hip")
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in src and "asm" not in src      # lognorm() is shared, plain C++
    assert '#include "wgnn_build_rows.h"' in src and "raise_lds" in src
    assert code("wgnn_align_rows.h").count("log1p") == 1


def _buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 2048 * i)


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _buffers()

    def run(fill, rowptr=at(0), col=at(1), cnt=at(2), n_rows=4, nnz=10, lib_=at(3), hood_ptr=at(4), members=at(5), n_units=3,
            n_members=7, n_genes=20, scale=1e4, threshold=0.0, slab=0, n_out=at(6), out_rowptr=at(8), out_col=at(9),
            out_val=at(10), out_cnt=at(11), status=at(12), flags=0):
        head = (rowptr, col, cnt, n_rows, nnz, lib_, hood_ptr, members, n_units, n_members, n_genes, scale, threshold, slab)
        if fill:
            return lib.wgnn_hood_rows_fill(*head, out_rowptr, out_col, out_val, out_cnt, status, flags, None)
        return lib.wgnn_hood_rows_count(*head, n_out, status, flags, None)

    def fails(code, word, only=None, **kw):
        for fill in (False, True) if only is None else (only,):
            assert run(fill, **kw) == code, (fill, kw)
            msg = lib.wgnn_last_error_string(code)
            assert (b"wgnn_hood_rows_fill" if fill else b"wgnn_hood_rows_count") in msg and word in msg, (kw, msg)

    fails(-1, b"status", status=None)
    fails(-1, b"hood_ptr is required", hood_ptr=None)
    fails(-1, b"members is required", members=None)
    for name in ("rowptr", "lib_"):
        fails(-1, b"rowptr and lib are required", **{name: None})
    fails(-1, b"col and cnt", col=None)
    fails(-1, b"col and cnt", cnt=None)
    fails(-1, b"n_out", only=False, n_out=None)
    fails(-1, b"out_rowptr", only=True, out_rowptr=None)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"n_units", n_units=-1)
    fails(-1, b"n_units", n_units=2 ** 31)
    fails(-1, b"n_members", n_members=-1)
    fails(-1, b"n_genes", n_genes=-1)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", threshold=thr)
    fails(-1, b"slab_genes", slab=-1)
    fails(-1, b"LDS", slab=16385)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    for name in ("lib_", "hood_ptr"):
        fails(-2, b"8-byte", **{name: at(3) + 4})
    fails(-2, b"8-byte", only=True, out_rowptr=at(8) + 4)
    fails(-2, b"8-byte", only=True, out_cnt=at(11) + 4)
    fails(-2, b"rowptr", rowptr=at(0) + 4, flags=16)
    fails(-2, b"rowptr", rowptr=at(0) + 2)
    fails(-2, b"4-byte", cnt=at(2) + 1)
    fails(-2, b"4-byte", col=at(1) + 2)
    fails(-2, b"4-byte", members=at(5) + 2)
    fails(-2, b"4-byte", only=False, n_out=at(6) + 2)
    fails(-2, b"4-byte", only=True, out_col=at(9) + 2)
    fails(-2, b"4-byte", only=True, out_val=at(10) + 2)
    fails(-2, b"4-byte", status=at(12) + 2)
    # no unit is a no-op, with or without operands and rows; the limits themselves pass
    for fill in (False, True):
        assert run(fill, n_units=0) == 0 and run(fill, n_units=0, n_rows=0, nnz=0, n_members=0, flags=16) == 0
        assert run(fill, n_units=0, rowptr=None, col=None, cnt=None, lib_=None, hood_ptr=None, members=None, n_out=None,
                   out_rowptr=None, out_col=None, out_val=None, out_cnt=None) == 0
        assert run(fill, n_units=0, slab=16384, n_genes=0, n_rows=2 ** 31 - 1, n_members=2 ** 40) == 0


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    rp, col, cnt = torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32), torch.ones(2)
    lib = torch.ones(2, dtype=torch.int64)
    ptr, members = torch.tensor([0, 2], dtype=torch.int64), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.hood_rows(rp, col, cnt, lib, ptr, members, 5)
