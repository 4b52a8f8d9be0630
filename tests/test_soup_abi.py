"""The C entries of the soup-rows block (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument
check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("wgnn_soup_rows_count", "wgnn_soup_rows_fill")


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1])
    for bit in ("BAD_ROWPTR", "BAD_COL", "BAD_ADD", "MAX_SLAB_GENES"):
        assert int(re.search(r"#define\s+WGNN_SOUP_%s\s+(\d+)" % bit, text).group(1)) == getattr(_lib, "SOUP_" + bit)
    assert len({_lib.SOUP_BAD_ROWPTR, _lib.SOUP_BAD_COL, _lib.SOUP_BAD_ADD}) == 3
    assert {bit for bit, _ in ops._SOUP_STATUS} == {_lib.SOUP_BAD_ROWPTR, _lib.SOUP_BAD_COL, _lib.SOUP_BAD_ADD}      # a text per bit
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.soup_rows is ops.soup_rows and sda.Ambient is api.Ambient and {"soup_rows", "Ambient"} <= set(sda.__all__)
    assert callable(sda.ResidentPredictor.ambient) and callable(sda.ResidentPredictor.ambient_file)
    from scdeepsort_amd import build
    assert "wgnn_soup.hip" in [p.name for p in build.SRC]
    code = lambda name: re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / name).read_text())
    src = code("wgnn_soup.hip")
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in src and "asm" not in src      # lognorm() is shared, plain C++
    assert code("wgnn_align_rows.h").count("log1p") == 1
    assert "0x94D049BB133111EBull" in src and "0xA0761D6478BD642Full" in src                       # K_SOUP, K_READ


def _buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 2048 * i)


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _buffers()

    def run(fill, rowptr=at(0), col=at(1), cnt=at(2), n_rows=4, nnz=10, lib_=at(3), n_add=at(4), cdf=at(5), n_genes=20, n_draws=3,
            row0=0, draw0=0, seed=1, scale=1e4, threshold=0.0, slab=0, n_out=at(6), soup_mapped=at(7), out_rowptr=at(8),
            out_col=at(9), out_val=at(10), out_cnt=at(11), status=at(12), flags=0):
        head = (rowptr, col, cnt, n_rows, nnz, lib_, n_add, cdf, n_genes, n_draws, row0, draw0, seed, scale, threshold, slab)
        if fill:
            return lib.wgnn_soup_rows_fill(*head, out_rowptr, out_col, out_val, out_cnt, status, flags, None)
        return lib.wgnn_soup_rows_count(*head, n_out, soup_mapped, status, flags, None)

    def fails(code, word, only=None, **kw):
        for fill in (False, True) if only is None else (only,):
            assert run(fill, **kw) == code, (fill, kw)
            msg = lib.wgnn_last_error_string(code)
            assert (b"wgnn_soup_rows_fill" if fill else b"wgnn_soup_rows_count") in msg and word in msg, (kw, msg)

    fails(-1, b"status", status=None)
    for name in ("rowptr", "lib_", "n_add", "cdf"):
        fails(-1, b"required", **{name: None})
    fails(-1, b"col and cnt", col=None)
    fails(-1, b"col and cnt", cnt=None)
    fails(-1, b"n_out", only=False, n_out=None)
    fails(-1, b"out_rowptr", only=True, out_rowptr=None)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"n_genes", n_genes=-1)
    fails(-1, b"n_genes", n_genes=2 ** 31 - 1)
    fails(-1, b"n_draws", n_draws=0)
    fails(-1, b"n_draws", n_draws=-2)
    fails(-1, b"n_rows * n_draws", n_rows=2 ** 30, n_draws=2)
    fails(-1, b"row0", row0=-1)
    fails(-1, b"draw0", draw0=-1)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", threshold=thr)
    fails(-1, b"slab_genes", slab=-1)
    fails(-1, b"LDS", slab=16385)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    for name in ("lib_", "n_add", "cdf"):
        fails(-2, b"8-byte", **{name: at(3) + 4})
    fails(-2, b"8-byte", only=True, out_rowptr=at(8) + 4)
    fails(-2, b"8-byte", only=True, out_cnt=at(11) + 4)
    fails(-2, b"rowptr", rowptr=at(0) + 4, flags=16)
    fails(-2, b"rowptr", rowptr=at(0) + 2)
    fails(-2, b"4-byte", cnt=at(2) + 1)
    fails(-2, b"4-byte", col=at(1) + 2)
    fails(-2, b"4-byte", only=False, n_out=at(6) + 2)
    fails(-2, b"4-byte", only=False, soup_mapped=at(7) + 2)
    fails(-2, b"4-byte", only=True, out_val=at(10) + 2)
    fails(-2, b"4-byte", status=at(12) + 2)
    # nothing to do is a no-op, with or without operands; the limits themselves pass
    for fill in (False, True):
        assert run(fill, n_rows=0) == 0 and run(fill, n_rows=0, nnz=0, flags=16) == 0
        assert run(fill, n_rows=0, rowptr=None, col=None, cnt=None, lib_=None, n_add=None, cdf=None, n_out=None, soup_mapped=None,
                   out_rowptr=None, out_col=None, out_val=None, out_cnt=None) == 0
        assert run(fill, n_rows=0, slab=16384, n_genes=0, n_draws=2 ** 31 - 1) == 0


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    rp, col, cnt = torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32), torch.ones(2)
    lib, n_add = torch.ones(2, dtype=torch.int64), torch.ones(2, dtype=torch.int64)
    cdf = torch.tensor([0, 1, 2], dtype=torch.int64)
    with pytest.raises(sda.WgnnError):
        sda.soup_rows(rp, col, cnt, lib, n_add, cdf, 2, scale=1e4, threshold=0.0)
    with pytest.raises(TypeError):                                     # scale and threshold have no default
        sda.soup_rows(rp, col, cnt, lib, n_add, cdf, 2)


def test_rho_levels():
    assert api._rho_levels(0.1) == (0.1,) and api._rho_levels((0.2, 0.05, 0.2, 0)) == (0.0, 0.05, 0.2)
    for bad in ((), 1.0, -0.1, float("nan"), (0.1, 1.5)):
        with pytest.raises(ValueError):
            api._rho_levels(bad)
