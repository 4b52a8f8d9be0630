"""The C entries of the pool-rows block (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument
check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("wgnn_pool_rows_accumulate", "wgnn_pool_rows_count", "wgnn_pool_rows_fill")


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1])
    for bit in ("BAD_INDEX", "BAD_ROWPTR", "BAD_COL", "MAX_CELLS_PER_UNIT", "MAX_SLAB_GENES"):
        assert int(re.search(r"#define\s+WGNN_POOL_%s\s+(\d+)" % bit, text).group(1)) == getattr(_lib, "POOL_" + bit)
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.pool_rows is ops.pool_rows
    from scdeepsort_amd import build
    assert "wgnn_pool.hip" in [p.name for p in build.SRC]
    code = lambda name: re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / name).read_text())
    src = code("wgnn_pool.hip")
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in src and "asm" not in src      # lognorm() is shared, plain C++
    # ONE definition of the transform: the float form calls the double form, nobody restates it
    rows = code("wgnn_align_rows.h")
    assert rows.count("log1p") == 1 and "return lognorm((double)x, total, scale)" in rows
    assert "log1p" not in code("wgnn_align_merge.hip") and "log1p" not in code("wgnn_pairs.hip")


def _buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 2048 * i)


def test_accumulate_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _buffers()

    def run(rowptr=at(0), col=at(1), cnt=at(2), n_rows=4, nnz=10, group_ptr=at(3), members=at(4), n_groups=3, n_genes=20,
            acc=at(5), ld_acc=20, cells=0, slab=0, status=at(6), flags=0):
        return lib.wgnn_pool_rows_accumulate(rowptr, col, cnt, n_rows, nnz, group_ptr, members, n_groups, n_genes, acc, ld_acc,
                                             cells, slab, status, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_pool_rows_accumulate" in msg and word in msg, (kw, msg)

    fails(-1, b"status", status=None)
    for name in ("rowptr", "group_ptr", "members"):
        fails(-1, b"required", **{name: None})
    fails(-1, b"col and cnt", col=None)
    fails(-1, b"col and cnt", cnt=None)
    fails(-1, b"acc is required", acc=None)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"n_groups", n_groups=-1)
    fails(-1, b"n_groups", n_groups=2 ** 31)
    fails(-1, b"n_genes", n_genes=-1, ld_acc=0)
    fails(-1, b"ld_acc", ld_acc=19)
    fails(-1, b"cells_per_unit", cells=-1)
    fails(-1, b"cells_per_unit", cells=257)
    fails(-1, b"slab_genes", slab=-1)
    fails(-1, b"LDS", slab=16385)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    fails(-2, b"group_ptr", group_ptr=at(3) + 4)
    fails(-2, b"acc", acc=at(5) + 4)
    fails(-2, b"rowptr", rowptr=at(0) + 4, flags=16)
    fails(-2, b"rowptr", rowptr=at(0) + 2)
    fails(-2, b"4-byte", members=at(4) + 2)
    fails(-2, b"4-byte", cnt=at(2) + 1)
    fails(-2, b"4-byte", status=at(6) + 2)
    # nothing to do is a no-op, with or without operands; the limits themselves pass
    assert run(n_groups=0) == 0 and run(n_rows=0, nnz=0, flags=16) == 0 and run(n_genes=0, ld_acc=0) == 0
    assert run(n_groups=0, rowptr=None, col=None, cnt=None, group_ptr=None, members=None, acc=None) == 0
    assert run(n_groups=0, cells=256, slab=16384) == 0


def test_finish_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _buffers()

    def run(fill, acc=at(0), ld_acc=20, total=at(1), n_groups=3, n_genes=20, scale=1e4, threshold=0.0, n_out=at(2),
            out_rowptr=at(3), out_col=at(4), out_val=at(5), out_cnt=at(6), status=at(7)):
        head = (acc, ld_acc, total, n_groups, n_genes, scale, threshold)
        if fill:
            return lib.wgnn_pool_rows_fill(*head, out_rowptr, out_col, out_val, out_cnt, status, None)
        return lib.wgnn_pool_rows_count(*head, n_out, status, None)

    def fails(code, word, only=None, **kw):
        for fill in (False, True) if only is None else (only,):
            assert run(fill, **kw) == code, (fill, kw)
            msg = lib.wgnn_last_error_string(code)
            assert (b"wgnn_pool_rows_fill" if fill else b"wgnn_pool_rows_count") in msg and word in msg, (kw, msg)

    fails(-1, b"status", status=None)
    fails(-1, b"total", total=None)
    fails(-1, b"acc", acc=None)
    fails(-1, b"n_out", only=False, n_out=None)
    fails(-1, b"out_rowptr", only=True, out_rowptr=None)
    fails(-1, b"n_groups", n_groups=-1)
    fails(-1, b"n_groups", n_groups=2 ** 31)
    fails(-1, b"n_genes", n_genes=-1, ld_acc=0)
    fails(-1, b"ld_acc", ld_acc=19)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", threshold=thr)
    fails(-2, b"8-byte", acc=at(0) + 4)
    fails(-2, b"8-byte", total=at(1) + 4)
    fails(-2, b"8-byte", only=True, out_rowptr=at(3) + 4)
    fails(-2, b"8-byte", only=True, out_cnt=at(6) + 4)
    fails(-2, b"4-byte", only=False, n_out=at(2) + 2)
    fails(-2, b"4-byte", only=True, out_val=at(5) + 2)
    fails(-2, b"4-byte", status=at(7) + 1)
    assert run(False, n_groups=0) == 0 and run(True, n_groups=0) == 0
    assert run(False, n_groups=0, acc=None, total=None, n_out=None) == 0
    assert run(True, n_groups=0, out_cnt=None, out_rowptr=None) == 0


def test_ops_refuses_cpu_tensors():
    rp, col, cnt = torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32), torch.ones(2)
    lib, group = torch.ones(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(sda.WgnnError):
        sda.pool_rows(rp, col, cnt, lib, group, 1)
