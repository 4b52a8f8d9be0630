"""The ``wgnn_leiden_*`` entries (``include/wgnn.h``) without a GPU: declared, bound and exported, every argument check returns its
code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check - and the kernels are
integer code that keeps everything in registers and uses the Louvain sweep's LDS tables.  tests/test_gpu_leiden_rows.py runs
them."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_leiden.hip"
ENTRIES = (("wgnn_leiden_boundary", 12), ("wgnn_leiden_refine_sweep", 28), ("wgnn_leiden_accept", 8))
KERNELS = ("refine_wave_kernel", "refine_heavy_kernel", "boundary_kernel", "accept_kernel")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    assert int(re.search(r"#define\s+WGNN_LEIDEN_BAD_PARTITION\s+(\d+)", text).group(1)) == _lib.LEIDEN_BAD_PARTITION == 64
    louvain_bits = (_lib.LOUVAIN_UNSORTED, _lib.LOUVAIN_BAD_COL, _lib.LOUVAIN_BAD_ROWPTR, _lib.LOUVAIN_NO_SCRATCH,
                    _lib.LOUVAIN_BAD_LABEL, _lib.LOUVAIN_BAD_WEIGHT)
    assert not any(bit & _lib.LEIDEN_BAD_PARTITION for bit in louvain_bits)      # one status word: the bits are reused, one added
    assert sda.leiden_graph is ops.leiden_graph and "leiden_graph" in sda.__all__
    assert ops.LeidenRows._fields == ops.LouvainRows._fields[:2] + ("refined_labels",) + ops.LouvainRows._fields[2:]
    for method in ("leiden", "leiden_file"):
        assert hasattr(sda.ResidentPredictor, method)
    import dataclasses
    fields = {f.name: f for f in dataclasses.fields(sda.Communities)}
    assert fields["method"].default == "louvain"
    from scdeepsort_amd import build
    assert "wgnn_leiden.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and not re.search(r"\b(float|double|fmaf?)\b", src)      # integers only, plain C++


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel of wgnn_leiden.hip keeps everything in registers, and its LDS
    tables are the Louvain sweep's."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_leiden.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == len(KERNELS)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    n = len(KERNELS)
    assert figures("ScratchSize [bytes/lane]") == [0] * n and figures("VGPRs Spill") == [0] * n and figures("SGPRs Spill") == [0] * n
    lds = dict(zip(names, figures("LDS Size [bytes/block]")))
    assert [v for k, v in lds.items() if "refine_wave_kernel" in k] == [256 * 8]
    assert all(4096 * 8 <= v <= 4096 * 8 + 64 for k, v in lds.items() if "refine_heavy_kernel" in k)
    assert [v for k, v in lds.items() if "boundary_kernel" in k] == [0]


def _host_buffers():
    buf = (C.c_double * 16384)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 4096 * i)


def _fails(lib, name, run):
    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert name.encode() in msg and word in msg, (kw, msg)
    return fails


def test_boundary_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, P=at(3), ref=at(4), ext=at(5), kinP=at(6), stats=at(7), flags=0):
        return lib.wgnn_leiden_boundary(rowptr, col, w, n, nnz, P, ref, ext, kinP, stats, flags, None)

    fails = _fails(lib, "wgnn_leiden_boundary", run)
    for operand in ("rowptr", "col", "w", "P", "ref", "ext", "stats"):  # kinP is optional
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    for f in (1, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for operand, i in (("rowptr", 0), ("ext", 5), ("kinP", 6), ("stats", 7)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("w", 2), ("P", 3), ("ref", 4)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert run(n=0) == 0 and run(n=0, kinP=None) == 0


def test_refine_sweep_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, P=at(3), ref=at(4), deg=at(5), totP=at(6), tot=at(7), size=at(8),
            ext=at(9), kinP=at(10), m_den=40, num=1, sweep=0, heavy=at(11), n_heavy=2, wave_rows=128, block_rows=2048, prop=at(12),
            gain=at(13), stats=at(14), workspace=at(15), workspace_bytes=4096, scratch_blocks=1, flags=0):
        return lib.wgnn_leiden_refine_sweep(rowptr, col, w, n, nnz, P, ref, deg, totP, tot, size, ext, kinP, m_den, num, sweep, heavy,
                                            n_heavy, wave_rows, block_rows, prop, gain, stats, workspace, workspace_bytes,
                                            scratch_blocks, flags, None)

    fails = _fails(lib, "wgnn_leiden_refine_sweep", run)
    for operand in ("rowptr", "col", "w", "P", "ref", "deg", "totP", "tot", "size", "ext", "kinP", "prop", "gain", "stats"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-5)
    for kw in (dict(m_den=0), dict(num=0), dict(num=-3)):
        fails(-1, b"positive", **kw)
    fails(-1, b"sweep", sweep=-1)
    fails(-1, b"n_heavy", n_heavy=-1)
    fails(-1, b"heavy", heavy=None)
    for s in (-1, 257):
        fails(-1, b"scratch_blocks", scratch_blocks=s)
    for f in (1, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for r in (-1, 129):
        fails(-3, b"wave_rows", wave_rows=r)
    for r in (-1, 2049):
        fails(-3, b"block_rows", block_rows=r)
    for operand, i in (("rowptr", 0), ("deg", 5), ("totP", 6), ("tot", 7), ("ext", 9), ("kinP", 10), ("gain", 13), ("stats", 14)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("w", 2), ("P", 3), ("ref", 4), ("size", 8), ("prop", 12), ("heavy", 11), ("workspace", 15)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    fails(-4, b"workspace", workspace_bytes=10 * 4 - 1)                 # one scratch block of 10 int32
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)
    assert run(n=0) == 0


def test_accept_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(ref=at(0), prop=at(1), n=10, nxt=at(2), gain=at(3), stats=at(4), flags=0):
        return lib.wgnn_leiden_accept(ref, prop, n, nxt, gain, stats, flags, None)

    fails = _fails(lib, "wgnn_leiden_accept", run)
    for operand in ("ref", "prop", "nxt", "gain", "stats"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"flag", flags=4)
    for operand, i in (("gain", 3), ("stats", 4)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("ref", 0), ("prop", 1), ("nxt", 2)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})


def test_ops_refuse_cpu_tensors():
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.leiden_graph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
