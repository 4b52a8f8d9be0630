"""``wgnn_knn_segments`` / ``wgnn_knn_segments_workspace_bytes`` (``include/wgnn.h``) without a GPU: declared, bound and exported,
and every argument check returns its code before any launch - host memory stands in for the operands,
``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_knn_segments"
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_knn_segments.hip"
SHARED = (SOURCE.with_name("wgnn_pair_tile.h"), SOURCE.with_name("wgnn_topk_select.h"))      # the pair tile (it holds the chain), the selection


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name, n in ((NAME, 22), ("wgnn_knn_segments_workspace_bytes", 6)):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    defined = {k: int(v) for k, v in re.findall(r"#define WGNN_KNN_SEGMENTS_(\w+)\s+(\d+)", header)}
    assert defined == dict(MAX_SEGS=_lib.KNN_SEGMENTS_MAX_SEGS, MAX_LIST=_lib.KNN_SEGMENTS_MAX_LIST,
                           BAD_ORDER=_lib.KNN_SEGMENTS_BAD_ORDER) == dict(MAX_SEGS=64, MAX_LIST=64, BAD_ORDER=1)
    assert (ops.KNN_SEGMENTS_MAX_SEGS, ops.KNN_SEGMENTS_MAX_LIST) == (64, 64)
    assert sda.knn_segments is ops.knn_segments and sda.BatchGraph is sda.api.BatchGraph and issubclass(sda.BatchGraph, sda.NeighborGraph)
    for method in ("bbknn", "bbknn_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert hasattr(sda.NeighborGraph, "lisi")
    from scdeepsort_amd import build
    assert SOURCE.name in [p.name for p in build.SRC]
    raw = SOURCE.read_text()
    assert all('#include "%s"' % h.name in raw for h in SHARED) and "fmaf(" not in raw          # the shared tile and selection, no copy
    code = lambda path: re.sub(r"//.*", "", path.read_text())
    src = "".join(code(path) for path in (SOURCE,) + SHARED)
    assert "asm" not in src and "double" not in src and "fmaf(" in code(SHARED[0])    # plain C++, the chain in explicit fmaf
    atomics = re.findall(r"atomic\w*\s*\(\s*(&\s*)?a\.(\w+)", src)                    # atomics on a global operand:
    assert atomics and all(field == "status" for _, field in atomics)                # the status word, nothing else


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: both kernels of wgnn_knn_segments.hip keep everything in registers."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_knn_segments.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 2 and any("knn_segments_kernel" in n for n in names) and any("knn_segments_merge" in n for n in names)
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert figures("ScratchSize [bytes/lane]") == [0, 0] and figures("VGPRs Spill") == [0, 0] and figures("SGPRs Spill") == [0, 0]
    assert max(figures("VGPRs")) <= 96                                 # five workgroups per CU: what the staging size is chosen for


def test_workspace_size_and_its_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    ask = lambda *a: lib.wgnn_knn_segments_workspace_bytes(*a, C.addressof(nb))
    # n_segs * splits lists of k keys per query, whatever the sizes: the second kernel always runs
    assert ask(1000, 5000, 1, 15, 1) == 0 and nb.value == 1000 * 15 * 8
    assert ask(1000, 5000, 4, 3, 1) == 0 and nb.value == 4 * 1000 * 3 * 8
    assert ask(1000, 5000, 4, 3, 7) == 0 and nb.value == 4 * 7 * 1000 * 3 * 8
    assert ask(1000, 5000, 4, 3, 64) == 0 and nb.value == 64 * 1000 * 3 * 8        # lowered to 64 // n_segs sub-ranges
    assert ask(1000, 5000, 64, 1, 2) == 0 and nb.value == 64 * 1000 * 8
    assert ask(100, 5000, 3, 3, 7) == 0 and nb.value == 3 * 7 * 100 * 3 * 8        # a query sub-range of the rows
    assert ask(197, 197, 3, 3, 0) == 0 and nb.value == 3 * 197 * 3 * 8             # a segment of about one tile: nothing to split
    for n, S in ((2000, 4), (20_000, 16), (100_000, 4)):                           # chosen from the sizes: whole lists of 1 .. 64 units
        assert ask(n, n, S, 3, 0) == 0 and nb.value % (S * n * 3 * 8) == 0 and 1 <= nb.value // (S * n * 3 * 8) <= 64 // S
    assert ask(2000, 2000, 4, 3, 0) == 0 and nb.value // (4 * 2000 * 3 * 8) == 4   # 8 tiles of a mean segment: two each
    assert ask(10_000_000, 10_000_000, 4, 3, 0) == 0 and nb.value == 4 * 10_000_000 * 3 * 8     # query tiles enough on their own
    assert ask(0, 0, 1, 1, 0) == 0 and nb.value == 0
    for bad, code, word in (((-1, 1, 1, 1, 0), -1, b"n_q"), ((2 ** 31, 1, 1, 1, 0), -1, b"n_q"), ((1, -1, 1, 1, 0), -1, b"n_rows"),
                            ((1, 2 ** 31, 1, 1, 0), -1, b"n_rows"), ((1, 1, 1, 0, 0), -3, b"k must"), ((1, 1, 1, 65, 0), -3, b"k must"),
                            ((1, 1, 0, 1, 0), -3, b"n_segs must"), ((1, 1, 65, 1, 0), -3, b"n_segs must"),
                            ((1, 1, 5, 13, 0), -3, b"n_segs * k"), ((1, 1, 64, 2, 0), -3, b"n_segs * k"),
                            ((1, 1, 1, 1, -1), -1, b"n_splits"), ((1, 1, 1, 1, 65), -1, b"n_splits")):
        assert ask(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_knn_segments_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_knn_segments_workspace_bytes(1, 1, 1, 1, 0, None) == -1


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 5120)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(X=at(0), ld_x=8, n_rows=10, D=8, order=at(1), seg_ptr=at(2), n_segs=2, k=3, q_first=0, n_q=4, n_splits=1,
            idx=at(3), d2=at(4), ld_out=6, merged_idx=at(5), merged_d2=at(6), ld_merged=6, status=at(7), workspace=at(8),
            workspace_bytes=4096, flags=0):
        return lib.wgnn_knn_segments(X, ld_x, n_rows, D, order, seg_ptr, n_segs, k, q_first, n_q, n_splits, idx, d2, ld_out,
                                     merged_idx, merged_d2, ld_merged, status, workspace, workspace_bytes, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert NAME.encode() in msg and word in msg, (kw, msg)

    # n_q == 0: nothing to do, whatever the pointers - but the sizes are still checked
    assert run(n_q=0) == 0 and run(n_q=0, q_first=10) == 0
    assert run(n_q=0, X=None, order=None, seg_ptr=None, idx=None, d2=None, status=None, workspace=None) == 0
    fails(-3, b"k must", n_q=0, k=0)
    # WGNN_ERR_BAD_ARG
    for n in (-1, 2 ** 31):
        fails(-1, b"n_q", n_q=n)
        fails(-1, b"n_rows", n_rows=n)
    for s in (-1, 65):
        fails(-1, b"n_splits", n_splits=s)
    for f in (1, 16, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    fails(-1, b"ld_out", ld_out=5)
    fails(-1, b"ld_merged", ld_merged=5)
    assert run(n_q=0, merged_idx=None, merged_d2=None, ld_merged=0) == 0          # the merged list is optional ...
    fails(-1, b"come together", merged_idx=None)                                   # ... as a pair
    fails(-1, b"come together", merged_d2=None)
    for first in (-1, 7, 2 ** 40):                                                 # 7 + 4 queries > 10 rows
        fails(-1, b"q_first", q_first=first)
    fails(-1, b"q_first", n_rows=3)
    assert run(q_first=6, n_q=0) == 0
    for name in ("X", "order", "seg_ptr", "idx", "d2", "status"):
        fails(-1, b"required", **{name: None})
    # WGNN_ERR_UNSUPPORTED
    for k in (0, -1, 65):
        fails(-3, b"k must", k=k, ld_out=256, ld_merged=256)
    for n_segs in (0, -1, 65):
        fails(-3, b"n_segs must", n_segs=n_segs, k=1, ld_out=256, ld_merged=256)
    for n_segs, k in ((2, 33), (5, 13), (64, 2), (22, 3)):
        fails(-3, b"n_segs * k", n_segs=n_segs, k=k, ld_out=256, ld_merged=256)
    for D in (0, 3, 1028, 2048):
        fails(-3, b"D must be in", D=D, ld_x=4096)
    # WGNN_ERR_ALIGNMENT
    for D in (5, 6, 1023):
        fails(-2, b"multiple of 4", D=D, ld_x=4096)
    for ld in (4, 9, 10):
        fails(-2, b"ld_x", ld_x=ld)
    fails(-2, b"16-byte", X=at(0) + 8)
    fails(-2, b"8-byte", seg_ptr=at(2) + 4)
    for name, i in (("order", 1), ("idx", 3), ("d2", 4), ("merged_idx", 5), ("merged_d2", 6), ("status", 7)):
        fails(-2, b"4-byte", **{name: at(i) + 2})
    fails(-2, b"8-byte", workspace=at(8) + 4)
    # WGNN_ERR_WORKSPACE: 2 segments x 1 sub-range x 4 queries x 3 keys of 8 bytes
    fails(-4, b"workspace", workspace_bytes=2 * 4 * 3 * 8 - 1)
    fails(-4, b"workspace", n_splits=2, workspace_bytes=2 * 2 * 4 * 3 * 8 - 1)
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)


def test_ops_refuses_cpu_tensors():
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.knn_segments(torch.zeros(5, 8), torch.zeros(5, dtype=torch.int64), 1, 3)
