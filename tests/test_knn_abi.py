"""``wgnn_knn_rows`` / ``wgnn_knn_workspace_bytes`` (``include/wgnn.h``) without a GPU: declared, bound and exported, and every
argument check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names
the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_knn_rows"
CSRC = ROOT / "scdeepsort_amd" / "csrc"
SHARED = ("wgnn_pair_tile.h", "wgnn_topk_select.h")                    # the pair tile (it holds the chain) and the top-k selection
code = lambda name: re.sub(r"//.*", "", (CSRC / name).read_text())     # a file of csrc without its comments


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name, n in ((NAME, 17), ("wgnn_knn_workspace_bytes", 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.knn_rows is ops.knn_rows and sda.NeighborGraph is sda.api.NeighborGraph
    for method in ("embed", "knn", "knn_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert (ops.KNN_MAX_K, ops.KNN_MAX_D, ops.KNN_MAX_SPLITS) == (64, 1024, 64)
    from scdeepsort_amd import build
    assert "wgnn_knn.hip" in [p.name for p in build.SRC]
    raw = (CSRC / "wgnn_knn.hip").read_text()
    assert all('#include "%s"' % h in raw for h in SHARED) and "fmaf(" not in raw      # the shared tile and selection, no copy of them
    src = "".join(code(name) for name in ("wgnn_knn.hip",) + SHARED)
    assert "asm" not in src and "double" not in src and "fmaf(" in code(SHARED[0])    # plain C++, the chain in explicit fmaf
    assert not re.search(r"atomic\w*\s*\(\s*(&\s*)?a\.", src)                         # no atomic on a global operand


def test_the_shared_tile_keeps_the_resources_the_timings_stand_on(tmp_path):
    """The compiler's resource remarks for the three kernels built on csrc/wgnn_pair_tile.h: the occupancy each was measured
    at, nothing in scratch, and the silhouette kernel's static LDS (the two slab buffers and its 64 group ids)."""
    import subprocess
    from scdeepsort_amd import build
    for name, kernel, occupancy, lds in (("wgnn_knn", "knn_kernel", 4, None), ("wgnn_knn_segments", "knn_segments_kernel", 5, None),
                                         ("wgnn_silhouette", "sil_kernel", 4, 17664)):
        r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                            str(CSRC / (name + ".hip")), "-o", str(tmp_path / (name + ".s"))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blocks = [b for b in r.stderr.split("Function Name: ")[1:] if kernel in b.split()[0]]
        assert len(blocks) == 1, (name, kernel)
        figure = lambda what: int(re.search(r"%s: (\d+)" % re.escape(what), blocks[0]).group(1))
        assert figure("Occupancy [waves/SIMD]") == occupancy, (kernel, figure("Occupancy [waves/SIMD]"))
        assert (figure("ScratchSize [bytes/lane]"), figure("VGPRs Spill"), figure("SGPRs Spill")) == (0, 0, 0), kernel
        assert lds is None or figure("LDS Size [bytes/block]") == lds, kernel


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: both kernels of wgnn_knn.hip keep everything in registers."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(ROOT / "scdeepsort_amd" / "csrc" / "wgnn_knn.hip"), "-o", str(tmp_path / "wgnn_knn.s")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 2 and any("knn_kernel" in n for n in names) and any("knn_merge" in n for n in names)
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert figures("ScratchSize [bytes/lane]") == [0, 0] and figures("VGPRs Spill") == [0, 0] and figures("SGPRs Spill") == [0, 0]


def test_workspace_size_and_its_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    ask = lambda *a: lib.wgnn_knn_workspace_bytes(*a, C.addressof(nb))
    assert ask(1000, 5000, 15, 1) == 0 and nb.value == 0               # one range: nothing to merge
    assert ask(1000, 5000, 15, 3) == 0 and nb.value == 3 * 1000 * 15 * 8
    assert ask(1000, 5000, 64, 64) == 0 and nb.value == 64 * 1000 * 64 * 8
    assert ask(100, 64, 15, 0) == 0 and nb.value == 0                  # one candidate tile: nothing to split
    for n in (200, 2000, 100_000):                                     # chosen from the sizes: whole lists of some 2..64 splits
        assert ask(n, n, 15, 0) == 0 and nb.value % (n * 15 * 8) == 0 and 2 <= nb.value // (n * 15 * 8) <= 64
    assert ask(10_000_000, 10_000_000, 15, 0) == 0 and nb.value == 0   # query tiles enough on their own
    assert ask(0, 0, 1, 0) == 0 and nb.value == 0
    for bad, code, word in (((-1, 1, 1, 0), -1, b"n_q"), ((2 ** 31, 1, 1, 0), -1, b"n_q"), ((1, -1, 1, 0), -1, b"n_c"),
                            ((1, 2 ** 31, 1, 0), -1, b"n_c"), ((1, 1, 0, 0), -3, b"k must"), ((1, 1, 65, 0), -3, b"k must"),
                            ((1, 1, 1, -1), -1, b"n_splits"), ((1, 1, 1, 65), -1, b"n_splits")):
        assert ask(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_knn_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_knn_workspace_bytes(1, 1, 1, 0, None) == -1


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(Q=at(0), ld_q=8, n_q=4, X=at(1), ld_x=8, n_c=10, D=8, k=3, self_offset=0, n_splits=1, idx=at(2), d2=at(3), ld_out=3,
            workspace=at(4), workspace_bytes=4096, flags=0):
        return lib.wgnn_knn_rows(Q, ld_q, n_q, X, ld_x, n_c, D, k, self_offset, n_splits, idx, d2, ld_out, workspace,
                                 workspace_bytes, flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert NAME.encode() in msg and word in msg, (kw, msg)

    # n_q == 0: nothing to do, whatever the pointers - but the sizes are still checked
    assert run(n_q=0, self_offset=-1) == 0 and run(n_q=0, Q=None, idx=None, d2=None, X=None, workspace=None) == 0
    fails(-3, b"k must", n_q=0, k=0)
    # WGNN_ERR_BAD_ARG
    for n in (-1, 2 ** 31):
        fails(-1, b"n_q", n_q=n)
        fails(-1, b"n_c", n_c=n)
    for s in (-1, 65):
        fails(-1, b"n_splits", n_splits=s)
    for f in (1, 16, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    fails(-1, b"ld_out", ld_out=2)
    for off in (-2, 7, 2 ** 40):                                       # 7 + 4 queries > 10 candidates
        fails(-1, b"self_offset", self_offset=off)
    assert run(self_offset=6, n_q=0) == 0 and run(self_offset=-1, n_q=0, n_c=0) == 0
    fails(-1, b"self_offset", self_offset=0, n_c=3)
    for name in ("Q", "X", "idx", "d2"):
        fails(-1, b"required", **{name: None})
    # WGNN_ERR_UNSUPPORTED
    for k in (0, -1, 65):
        fails(-3, b"k must", k=k, ld_out=128)
    for D in (0, 3, 1028, 2048):
        fails(-3, b"D must be in", D=D, ld_q=4096, ld_x=4096)
    # WGNN_ERR_ALIGNMENT
    for D in (5, 6, 1023):
        fails(-2, b"multiple of 4", D=D, ld_q=4096, ld_x=4096)
    for kw in (dict(ld_q=4), dict(ld_x=4), dict(ld_q=9), dict(ld_x=10)):
        fails(-2, b"ld_q and ld_x", **kw)
    for name, i in (("Q", 0), ("X", 1)):
        fails(-2, b"16-byte", **{name: at(i) + 8})
    for name, i in (("idx", 2), ("d2", 3)):
        fails(-2, b"4-byte", **{name: at(i) + 2})
    fails(-2, b"8-byte", n_splits=2, workspace=at(4) + 4)
    # WGNN_ERR_WORKSPACE: two ranges need 2 * 4 * 3 * 8 bytes
    fails(-4, b"workspace", n_splits=2, workspace_bytes=2 * 4 * 3 * 8 - 1)
    fails(-4, b"workspace", n_splits=2, workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.knn_rows(torch.zeros(5, 8), 3)
