"""``wgnn_kmeans_seed`` / ``wgnn_group_rows_reduce`` and their workspace entries (``include/wgnn.h``) without a GPU: declared, bound
and exported, every argument check returns its code before any launch - host memory stands in for the operands,
``wgnn_last_error_string`` names the check - and the kernels keep everything in registers."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_kmeans.hip"
ENTRIES = (("wgnn_kmeans_seed", 12), ("wgnn_kmeans_seed_workspace_bytes", 3), ("wgnn_group_rows_reduce", 16),
           ("wgnn_group_rows_reduce_workspace", 4))


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    for name in ("kmeans_seed", "group_rows_reduce", "kmeans_rows"):
        assert getattr(sda, name) is getattr(ops, name)
    assert sda.KMeans is sda.api.KMeans and sda.api.KMeansSummary is sda.tables.KMeansSummary
    for method in ("kmeans", "kmeans_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert ops.KMEANS_MAX_K == 4096
    from scdeepsort_amd import build
    assert "wgnn_kmeans.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and "fmaf(" in src and not re.search(r"\batomic\w*\s*\(", src)       # plain C++, no atomic at all
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*from\s+\.?(api|ops)\b|^\s*from\s+\.\s+import\s+.*\b(api|ops)\b|^\s*import\s+.*\b(api|ops)\b",
                         tables_src, flags=re.M)


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel of wgnn_kmeans.hip keeps everything in registers."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_kmeans.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 4
    for kernel in ("seed_pass_kernel", "seed_pick_kernel", "rows_chunk_kernel", "rows_finish_kernel"):
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert figures("ScratchSize [bytes/lane]") == [0] * 4 and figures("VGPRs Spill") == [0] * 4 and figures("SGPRs Spill") == [0] * 4


def test_workspace_sizes_and_their_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    seed = lambda *a: lib.wgnn_kmeans_seed_workspace_bytes(*a, C.addressof(nb))
    assert seed(1, 1) == 0 and nb.value == 8 + 4                       # one chunk sum, one row mark
    assert seed(256, 4096) == 0 and nb.value == 8 + 256 * 4
    assert seed(257, 3) == 0 and nb.value == 2 * 8 + 257 * 4
    assert seed(100_000, 1000) == 0 and nb.value == 391 * 8 + 100_000 * 4
    for bad, code, word in (((0, 1), -1, b"n_rows"), ((-1, 1), -1, b"n_rows"), ((2 ** 31, 1), -1, b"n_rows"),
                            ((10, 0), -3, b"K must"), ((10, -1), -3, b"K must"), ((10, 4097), -3, b"K must")):
        assert seed(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_kmeans_seed_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_kmeans_seed_workspace_bytes(1, 1, None) == -1

    rows = lambda *a: lib.wgnn_group_rows_reduce_workspace(*a, C.addressof(nb))
    assert rows(0, 1, 1) == 0 and nb.value == 16                       # one slot: a double and an int32, to a multiple of 8
    assert rows(300, 7, 20) == 0 and nb.value == 1808                  # 11 slots of 20 doubles and an int32: 1804, rounded up
    assert rows(100_000, 1024, 200) == 0 and nb.value == (100_000 // 64 + 1024) * (200 * 8 + 4) and nb.value % 8 == 0
    for bad, code, word in (((-1, 1, 1), -1, b"n_rows"), ((2 ** 31, 1, 1), -1, b"n_rows"), ((1, 0, 1), -1, b"n_groups"),
                            ((1, -3, 1), -1, b"n_groups"), ((1, 1, 0), -1, b"D must"), ((1, 1, 65537), -3, b"65536")):
        assert rows(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_group_rows_reduce_workspace" in msg and word in msg, (bad, msg)
    assert lib.wgnn_group_rows_reduce_workspace(1, 1, 1, None) == -1


def _host_buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 4096 * i)


def test_seed_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()
    name = "wgnn_kmeans_seed"

    def run(X=at(0), ld_x=8, n_rows=10, D=8, K=3, seed=0, seed_row=at(1), min_d2=at(2), workspace=at(3), workspace_bytes=4096,
            flags=0):
        return lib.wgnn_kmeans_seed(X, ld_x, n_rows, D, K, seed, seed_row, min_d2, workspace, workspace_bytes, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert name.encode() in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for n in (0, -1, 2 ** 31):
        fails(-1, b"n_rows", n_rows=n)
    for f in (1, 16, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for operand in ("X", "seed_row", "min_d2"):
        fails(-1, b"required", **{operand: None})
    # WGNN_ERR_UNSUPPORTED
    for K in (0, -1, 4097):
        fails(-3, b"K must", K=K)
    for D in (0, 3, 1028, 2048):
        fails(-3, b"D must be in", D=D, ld_x=4096)
    # WGNN_ERR_ALIGNMENT
    for D in (5, 6, 1023):
        fails(-2, b"multiple of 4", D=D, ld_x=4096)
    for ld in (4, 9, 10):
        fails(-2, b"ld_x", ld_x=ld)
    fails(-2, b"16-byte", X=at(0) + 8)
    for operand, i in (("seed_row", 1), ("min_d2", 2)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    fails(-2, b"8-byte", workspace=at(3) + 4)
    # WGNN_ERR_WORKSPACE: 10 rows need one chunk sum and ten marks
    fails(-4, b"workspace", workspace_bytes=8 + 40 - 1)
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)


def test_reduce_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()
    name = "wgnn_group_rows_reduce"

    def run(X=at(0), ld_x=8, order=at(1), seg_ptr=at(2), n_rows=10, n_groups=3, D=8, total=at(3), ld_sum=8, count=at(4),
            mean=at(5), ld_mean=8, workspace=at(6), workspace_bytes=4096, flags=0):
        return lib.wgnn_group_rows_reduce(X, ld_x, order, seg_ptr, n_rows, n_groups, D, total, ld_sum, count, mean, ld_mean,
                                          workspace, workspace_bytes, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert name.encode() in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for operand in ("total", "count", "seg_ptr"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n_rows", n_rows=n)
    for k in (0, -2):
        fails(-1, b"n_groups", n_groups=k)
    for D in (0, -4):
        fails(-1, b"D must", D=D)
    for f in (1, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    fails(-1, b"ld_x", ld_x=7)
    fails(-1, b"ld_sum", ld_sum=7)
    fails(-1, b"ld_mean", ld_mean=7)
    assert run(mean=None, ld_mean=0, workspace_bytes=0) == -4          # without a mean its stride is not looked at
    # WGNN_ERR_UNSUPPORTED
    fails(-3, b"65536", D=65537, ld_x=2 ** 20, ld_sum=2 ** 20, ld_mean=2 ** 20)
    # WGNN_ERR_ALIGNMENT
    for operand, i in (("total", 3), ("count", 4), ("seg_ptr", 2)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("X", 0), ("order", 1), ("mean", 5)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    fails(-2, b"8-byte", workspace=at(6) + 4)
    # WGNN_ERR_WORKSPACE: 10 rows in 3 groups are 3 slots of 8 doubles and an int32
    fails(-4, b"workspace", workspace_bytes=3 * (8 * 8 + 4) - 1)
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(5, 8)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.kmeans_seed(x, 2)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.group_rows_reduce(x, torch.zeros(5, dtype=torch.int64), 2)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.kmeans_rows(x, 2)
