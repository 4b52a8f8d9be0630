"""``wgnn_snn_weights`` and the ``wgnn_louvain_*`` entries (``include/wgnn.h``) without a GPU: declared, bound and exported, every
argument check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the
check - and the kernels are integer code that keeps everything in registers.  What only the entries of a graph can show (unsorted
rows, columns out of range) is a status bit of ``wgnn_louvain_modularity``: its values are pinned here, tests/test_gpu_louvain_rows.py
raises them on the device."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_louvain.hip"
ENTRIES = (("wgnn_snn_weights", 10), ("wgnn_louvain_sweep_workspace_bytes", 3), ("wgnn_louvain_sweep", 24),
           ("wgnn_louvain_apply", 9), ("wgnn_louvain_modularity", 10))
KERNELS = ("snn_weights_kernel", "sweep_wave_kernel", "sweep_heavy_kernel", "apply_kernel", "inside_kernel", "tot2_kernel")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    for name, value in (("WGNN_SNN_IDX_I64", _lib.SNN_IDX_I64), ("WGNN_LOUVAIN_UNSORTED", _lib.LOUVAIN_UNSORTED),
                        ("WGNN_LOUVAIN_BAD_COL", _lib.LOUVAIN_BAD_COL), ("WGNN_LOUVAIN_BAD_ROWPTR", _lib.LOUVAIN_BAD_ROWPTR),
                        ("WGNN_LOUVAIN_NO_SCRATCH", _lib.LOUVAIN_NO_SCRATCH), ("WGNN_LOUVAIN_BAD_LABEL", _lib.LOUVAIN_BAD_LABEL),
                        ("WGNN_LOUVAIN_BAD_WEIGHT", _lib.LOUVAIN_BAD_WEIGHT)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value
    assert (_lib.LOUVAIN_UNSORTED, _lib.LOUVAIN_BAD_COL, _lib.LOUVAIN_BAD_ROWPTR) == (1, 2, 4)
    for name in ("snn_graph", "louvain_graph"):
        assert getattr(sda, name) is getattr(ops, name)
    assert sda.Communities is sda.api.Communities and sda.api.CommunitiesSummary is sda.tables.CommunitiesSummary
    for method in ("louvain", "louvain_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert (ops.SNN_MAX_K, ops.LOUVAIN_WAVE_ROWS, ops.LOUVAIN_BLOCK_ROWS) == (64, 128, 2048)
    from scdeepsort_amd import build
    assert "wgnn_louvain.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and not re.search(r"\b(float|double|fmaf?)\b", src)      # integers only, plain C++
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*from\s+\.?(api|ops)\b|^\s*from\s+\.\s+import\s+.*\b(api|ops)\b|^\s*import\s+.*\b(api|ops)\b",
                         tables_src, flags=re.M)


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel of wgnn_louvain.hip keeps everything in registers, and the
    LDS tables are the sizes the header states."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_louvain.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == len(KERNELS)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    n = len(KERNELS)
    assert figures("ScratchSize [bytes/lane]") == [0] * n and figures("VGPRs Spill") == [0] * n and figures("SGPRs Spill") == [0] * n
    lds = dict(zip(names, figures("LDS Size [bytes/block]")))
    assert [v for k, v in lds.items() if "sweep_wave_kernel" in k] == [256 * 8]
    assert all(4096 * 8 <= v <= 4096 * 8 + 64 for k, v in lds.items() if "sweep_heavy_kernel" in k)


def test_workspace_sizes_and_their_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    size = lambda *a: lib.wgnn_louvain_sweep_workspace_bytes(*a, C.addressof(nb))
    assert size(0, 0) == 0 and nb.value == 0
    assert size(1000, 0) == 0 and nb.value == 0                        # no long row: no scratch
    assert size(1000, 3) == 0 and nb.value == 3 * 1000 * 4
    assert size(2 ** 31 - 1, 256) == 0 and nb.value == (2 ** 31 - 1) * 4 * 256
    for bad, word in (((-1, 1), b"n must"), ((2 ** 31, 1), b"n must"), ((10, -1), b"scratch_blocks"), ((10, 257), b"scratch_blocks")):
        assert size(*bad) == -1, bad
        msg = lib.wgnn_last_error_string(-1)
        assert b"wgnn_louvain_sweep_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_louvain_sweep_workspace_bytes(1, 1, None) == -1


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


def test_snn_weights_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(idx=at(0), ld_idx=8, n=10, k=8, rowptr=at(1), col=at(2), nnz=20, w=at(3), flags=0):
        return lib.wgnn_snn_weights(idx, ld_idx, n, k, rowptr, col, nnz, w, flags, None)

    fails = _fails(lib, "wgnn_snn_weights", run)
    for operand in ("idx", "rowptr", "col", "w"):                       # WGNN_ERR_BAD_ARG: null pointers, negative sizes
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"ld_idx", ld_idx=7)
    for f in (1, 16, 512, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for k in (0, -1, 65, 1000):                                         # WGNN_ERR_UNSUPPORTED: k > 64
        fails(-3, b"k must", k=k, ld_idx=1000)
    fails(-2, b"8-byte", rowptr=at(1) + 4)                              # WGNN_ERR_ALIGNMENT
    fails(-2, b"8-byte", idx=at(0) + 4, flags=_lib.SNN_IDX_I64)
    for operand, i in (("idx", 0), ("col", 2), ("w", 3)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert run(n=0) == 0 and run(nnz=0) == 0                            # nothing to do: no launch


def test_sweep_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, comm=at(3), deg=at(4), tot=at(5), size=at(6), m_den=40, num=1, sweep=0,
            heavy=at(7), n_heavy=2, wave_rows=128, block_rows=2048, nxt=at(8), gain=at(9), stats=at(10), workspace=at(11),
            workspace_bytes=4096, scratch_blocks=1, flags=0):
        return lib.wgnn_louvain_sweep(rowptr, col, w, n, nnz, comm, deg, tot, size, m_den, num, sweep, heavy, n_heavy, wave_rows,
                                      block_rows, nxt, gain, stats, workspace, workspace_bytes, scratch_blocks, flags, None)

    fails = _fails(lib, "wgnn_louvain_sweep", run)
    for operand in ("rowptr", "col", "w", "comm", "deg", "tot", "size", "nxt", "gain", "stats"):
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
    for operand, i in (("rowptr", 0), ("deg", 4), ("tot", 5), ("gain", 9), ("stats", 10)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("w", 2), ("comm", 3), ("size", 6), ("nxt", 8), ("heavy", 7), ("workspace", 11)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    fails(-4, b"workspace", workspace_bytes=10 * 4 - 1)                 # one scratch block of 10 int32
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)
    assert run(n=0) == 0


def test_apply_and_modularity_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def apply(old_label=at(0), label=at(1), deg=at(2), n=10, tot=at(3), size=at(4), stats=at(5), flags=0):
        return lib.wgnn_louvain_apply(old_label, label, deg, n, tot, size, stats, flags, None)

    fails = _fails(lib, "wgnn_louvain_apply", apply)
    for operand in ("label", "deg", "tot", "size", "stats"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"flag", flags=1)
    for operand, i in (("deg", 2), ("tot", 3), ("stats", 5)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("old_label", 0), ("label", 1), ("size", 4)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})

    def modularity(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, label=at(3), tot=at(4), stats=at(5), flags=0):
        return lib.wgnn_louvain_modularity(rowptr, col, w, n, nnz, label, tot, stats, flags, None)

    fails = _fails(lib, "wgnn_louvain_modularity", modularity)
    for operand in ("rowptr", "col", "w", "label", "tot", "stats"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"flag", flags=2)
    for operand, i in (("rowptr", 0), ("tot", 4), ("stats", 5)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("w", 2), ("label", 3)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert modularity(n=0) == 0


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    idx = torch.zeros((5, 3), dtype=torch.int64)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.snn_graph(idx)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.louvain_graph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    from fractions import Fraction
    assert ops.louvain_resolution(0.8) == Fraction(4, 5) and ops.louvain_resolution(2) == 2
    for bad in (0, -1, 1e-9, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            ops.louvain_resolution(bad)
