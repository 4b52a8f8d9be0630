"""``wgnn_rank_sets_rows`` (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument check returns
its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_rank_sets_rows"


def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text) and hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % NAME, text, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES[NAME][1]) == 14
    assert lib.wgnn_version() == 206                                   # an additive export
    assert sda.rank_sets_rows is ops.rank_sets_rows and sda.SignatureScores is sda.api.SignatureScores
    assert sda.read_gmt is sda.api.read_gmt and ops.SETS_PER_LAUNCH == 64
    from scdeepsort_amd import build
    assert "wgnn_signatures.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_signatures.hip").read_text())
    assert "asm" not in src and "atomic" not in src and "float" in src and "double" not in src     # plain C++, integers only


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(rowptr=at(0), col=at(1), val=at(2), n_rows=4, n_genes=100, member=at(3), n_sets=3, max_rank=1500, rank2_sum=at(4),
            ld_sum=3, present=at(5), ld_present=3, flags=0):
        return lib.wgnn_rank_sets_rows(rowptr, col, val, n_rows, n_genes, member, n_sets, max_rank, rank2_sum, ld_sum, present,
                                       ld_present, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_rank_sets_rows" in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for name in ("rowptr", "col", "val"):
        fails(-1, b"required", **{name: None})
    fails(-1, b"member", member=None)
    fails(-1, b"rank2_sum", rank2_sum=None)
    fails(-1, b"present", present=None)
    for n in (0, -1, 65):
        fails(-1, b"n_sets", n_sets=n, ld_sum=65, ld_present=65)
    for r in (0, -1, 2 ** 30 + 1):
        fails(-1, b"max_rank", max_rank=r)
    for g in (0, -5):
        fails(-1, b"n_genes", n_genes=g)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"ld_sum", ld_sum=2)
    fails(-1, b"ld_present", ld_present=2)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    # WGNN_ERR_ALIGNMENT
    fails(-2, b"8-byte", member=at(3) + 4)
    fails(-2, b"8-byte", rank2_sum=at(4) + 4)
    fails(-2, b"rowptr", rowptr=at(0) + 4, flags=16)
    fails(-2, b"rowptr", rowptr=at(0) + 2)
    fails(-2, b"4-byte", present=at(5) + 2)
    fails(-2, b"4-byte", col=at(1) + 1)
    fails(-2, b"4-byte", val=at(2) + 2)
    # an empty batch is a no-op; the limits themselves pass the checks
    assert run(n_rows=0) == 0 and run(n_rows=0, flags=16) == 0
    assert run(n_rows=0, n_sets=64, ld_sum=64, ld_present=64, max_rank=2 ** 30, n_genes=2 ** 31 - 1) == 0
    assert run(n_rows=0, n_sets=1, ld_sum=1, ld_present=1, max_rank=1, n_genes=1) == 0


def test_ops_refuses_cpu_tensors():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(sda.WgnnError):
        sda.rank_sets_rows(rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, dtype=torch.int64), 2, 10, 3)
