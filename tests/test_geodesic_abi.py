"""``wgnn_geodesic_round`` (``include/wgnn.h``) without a GPU: declared, bound and exported, every argument check returns its code
before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check - and the kernel keeps
everything in registers: no scratch, no spill, no LDS.  tests/test_gpu_geodesic_rows.py runs it."""
import ctypes as C
import dataclasses
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_geodesic.hip"
ENTRY, N_ARGS = "wgnn_geodesic_round", 14


def test_symbol_is_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\b%s\s*\(" % ENTRY, text) and hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES
    n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % ENTRY, text, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES[ENTRY][1]) == N_ARGS
    assert lib.wgnn_version() == 206                                   # an additive export
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (define("WGNN_GEODESIC_UNSORTED"), define("WGNN_GEODESIC_BAD_COL"), define("WGNN_GEODESIC_BAD_ROWPTR"),
            define("WGNN_GEODESIC_BAD_LENGTH")) == (_lib.GEODESIC_UNSORTED, _lib.GEODESIC_BAD_COL, _lib.GEODESIC_BAD_ROWPTR,
                                                    _lib.GEODESIC_BAD_LENGTH) == (1, 2, 4, 8)
    assert define("WGNN_GEODESIC_LANES") == _lib.GEODESIC_LANES == 16 and define("WGNN_GEODESIC_MAX_BLOCKS") == _lib.GEODESIC_MAX_BLOCKS
    assert [bit for bit, _ in ops._GEODESIC_STATUS] == [1, 2, 4, 8]
    from scdeepsort_amd import build
    assert "wgnn_geodesic.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and "__shared__" not in src and not re.search(r"\bfmaf?\b", src)       # plain C++, one add
    assert "fp contract(off)" in src


def test_the_public_names():
    for name in ("distance_graph", "geodesic_rows", "group_edges"):
        assert getattr(sda, name) is getattr(ops, name) and name in sda.__all__
    assert ops.DistanceGraph._fields == ("rowptr", "col", "length")
    assert ops.GeodesicRows._fields == ("dist", "pred", "rounds", "converged", "reached")
    assert ops.GroupEdges._fields == ("edges", "size")
    for name in ("Pseudotime", "Abstraction"):
        assert name in sda.__all__ and dataclasses.is_dataclass(getattr(sda, name))
    for method in ("pseudotime", "pseudotime_file", "paga", "paga_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert {"distance", "pseudotime", "pred", "root", "reached", "rounds", "converged", "k", "space", "metric", "label",
            "max_prob"} <= {f.name for f in dataclasses.fields(sda.Pseudotime)}
    assert {"edges", "size", "out_edges", "connectivities", "expected", "group_names", "n_skipped"} <= \
        {f.name for f in dataclasses.fields(sda.Abstraction)}
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*(from|import)\b.*\b(api|ops)\b", tables_src, flags=re.M)    # neither the predictor nor the ops


def test_the_kernel_compiles_without_scratch_spills_or_lds(tmp_path):
    """The compiler's own resource remarks for gfx950."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_geodesic.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 1 and "geodesic_round_kernel" in names[0]
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert figures("ScratchSize [bytes/lane]") == [0] and figures("VGPRs Spill") == [0] and figures("SGPRs Spill") == [0]
    assert figures("LDS Size [bytes/block]") == [0]
    assert figures("VGPRs")[0] <= 64                                    # eight waves per SIMD


def _host_buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 4096 * i)


def test_argument_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(rowptr=at(0), col=at(1), length=at(2), n=10, nnz=20, dist_in=at(3), pred_in=at(4), dist_out=at(5), pred_out=at(6),
            changed=at(7), status=at(8), grid_blocks=0, flags=0):
        return lib.wgnn_geodesic_round(rowptr, col, length, n, nnz, dist_in, pred_in, dist_out, pred_out, changed, status,
                                       grid_blocks, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert ENTRY.encode() in msg and word in msg, (kw, msg)

    for operand in ("rowptr", "col", "length", "dist_in", "pred_in", "dist_out", "pred_out", "changed", "status"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    for g in (-1, 8193):
        fails(-1, b"grid_blocks", grid_blocks=g)
    for f in (1, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    fails(-1, b"other buffers", dist_out=at(3))                         # a round reads the state before it: no in-place update
    fails(-1, b"other buffers", pred_out=at(4))
    for operand, i in (("rowptr", 0), ("changed", 7), ("status", 8)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("length", 2), ("dist_in", 3), ("pred_in", 4), ("dist_out", 5), ("pred_out", 6)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert run(n=0) == 0 and run(n=0, nnz=0, grid_blocks=8192) == 0     # nothing to do: no launch


def test_ops_refuse_cpu_tensors():
    rowptr, col = torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.geodesic_rows(rowptr, col, torch.zeros(0), 0)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.distance_graph(torch.zeros((4, 2), dtype=torch.int64), torch.zeros((4, 2)))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.group_edges(torch.zeros((4, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 2)
