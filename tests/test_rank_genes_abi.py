"""``wgnn_rank_genes_groups`` (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument check returns
its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_rank_genes_groups"


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name, n in ((NAME, 17), (NAME + "_workspace", 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.rank_genes_groups is ops.rank_genes_groups and sda.GeneRanks is sda.api.GeneRanks
    assert hasattr(sda.ResidentPredictor, "rank_genes") and hasattr(sda.ResidentPredictor, "rank_genes_file")
    assert ops.RANK_GENES_MAX_ROWS == 2 ** 20 and ops.RANK_GENES_MAX_GROUPS == 4096
    from scdeepsort_amd import build
    assert "wgnn_rank_genes.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_rank_genes.hip").read_text())
    assert "asm" not in src and "float" in src and "double" not in src              # plain C++, integers only


def test_workspace_size_and_its_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    ask = lambda *a: lib.wgnn_rank_genes_groups_workspace(*a, C.addressof(nb))
    assert ask(1000, 5000, 16, 300) == 0 and 0 < nb.value <= 32 * 300          # per gene, nothing per entry or per cell
    small = nb.value
    assert ask(2 ** 20, 2 ** 31 - 1, 4096, 300) == 0 and nb.value == small
    assert ask(0, 0, 1, 1) == 0 and nb.value > 0
    for bad, word in (((2 ** 20 + 1, 0, 1, 1), b"n_rows"), ((-1, 0, 1, 1), b"n_rows"), ((1, -1, 1, 1), b"nnz"),
                      ((1, 2 ** 31, 1, 1), b"nnz"), ((1, 0, 0, 1), b"n_groups"), ((1, 0, 4097, 1), b"n_groups"),
                      ((1, 0, 1, 0), b"n_genes")):
        assert ask(*bad) == -1
        msg = lib.wgnn_last_error_string(-1)
        assert b"wgnn_rank_genes_groups_workspace" in msg and word in msg, (bad, msg)
    assert lib.wgnn_rank_genes_groups_workspace(1, 0, 1, 1, None) == -1


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i
    need = C.c_int64()
    assert lib.wgnn_rank_genes_groups_workspace(4, 0, 3, 100, C.addressof(need)) == 0

    def run(t_rowptr=at(0), t_cell=at(1), t_val=at(2), group=at(3), group_size=at(4), n_rows=4, n_groups=3, n_genes=100,
            rank2_sum=at(5), ld_sum=100, count=at(6), ld_count=100, tie_sum=at(7), workspace=at(8), workspace_bytes=need.value,
            flags=0):
        return lib.wgnn_rank_genes_groups(t_rowptr, t_cell, t_val, group, group_size, n_rows, n_groups, n_genes, rank2_sum,
                                          ld_sum, count, ld_count, tie_sum, workspace, workspace_bytes, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_rank_genes_groups" in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for name in ("rank2_sum", "count", "tie_sum", "t_rowptr", "group_size", "t_cell", "t_val", "group"):
        fails(-1, b"required", **{name: None})
    for n in (-1, 2 ** 20 + 1, 2 ** 31):
        fails(-1, b"n_rows", n_rows=n)
    for k in (0, -1, 4097):
        fails(-1, b"n_groups", n_groups=k)
    for g in (0, -5):
        fails(-1, b"n_genes", n_genes=g)
    fails(-1, b"ld_sum", ld_sum=99)
    fails(-1, b"ld_count", ld_count=99)
    for f in (1, 16, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    # WGNN_ERR_WORKSPACE (-4)
    fails(-4, b"workspace", workspace_bytes=need.value - 1)
    fails(-4, b"workspace", workspace_bytes=-1)
    fails(-4, b"workspace", workspace=None)
    # WGNN_ERR_ALIGNMENT
    for name, i in (("rank2_sum", 5), ("tie_sum", 7), ("group_size", 4), ("workspace", 8)):
        fails(-2, b"8-byte", **{name: at(i) + 4})
    for name, i in (("t_rowptr", 0), ("t_cell", 1), ("t_val", 2), ("group", 3), ("count", 6)):
        fails(-2, b"4-byte", **{name: at(i) + 2})


def test_ops_refuses_cpu_tensors():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(sda.WgnnError):
        sda.rank_genes_groups(rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(1, dtype=torch.int32), 2, 3)
