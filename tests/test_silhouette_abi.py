"""``wgnn_silhouette_rows`` and its workspace entry (``include/wgnn.h``) without a GPU: declared, bound and exported, every argument
check returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check -
and the kernels keep everything in registers."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_silhouette.hip"
TILE = SOURCE.with_name("wgnn_pair_tile.h")                            # the pair tile it shares with the kNN kernels: it holds the chain
ENTRIES = (("wgnn_silhouette_rows", 15), ("wgnn_silhouette_workspace_bytes", 4))


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    assert sda.silhouette_rows is ops.silhouette_rows
    assert sda.Silhouette is sda.api.Silhouette is sda.tables.Silhouette and sda.api.SilhouetteSummary is sda.tables.SilhouetteSummary
    for method in ("silhouette", "silhouette_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert ops.SILHOUETTE_MAX_GROUPS == 4096 and ops.SILHOUETTE_MAX_SPLITS == 64
    from scdeepsort_amd import build
    assert "wgnn_silhouette.hip" in [p.name for p in build.SRC]
    raw = SOURCE.read_text()
    assert '#include "%s"' % TILE.name in raw and "fmaf(" not in raw   # the shared pair tile, no copy of its chain
    tile = re.sub(r"//.*", "", TILE.read_text())
    src = re.sub(r"//.*", "", raw) + tile
    assert "asm" not in src and "fmaf(" in tile and "sqrtf(" in src and not re.search(r"\batomic\w*\s*\(", src)
    assert "double" not in tile                                        # fp64 is this file's partial sums, never the chain
    assert "__fsqrt_rn" not in src                                     # the bare hardware square root is not correctly rounded
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*from\s+\.?(api|ops)\b|^\s*from\s+\.\s+import\s+.*\b(api|ops)\b|^\s*import\s+.*\b(api|ops)\b",
                         tables_src, flags=re.M)


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel of wgnn_silhouette.hip keeps everything in registers."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_silhouette.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 3
    for kernel in ("sil_kernel", "sil_plan", "sil_merge"):
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert figures("ScratchSize [bytes/lane]") == [0] * 3 and figures("VGPRs Spill") == [0] * 3 and figures("SGPRs Spill") == [0] * 3
    assert max(figures("LDS Size [bytes/block]")) <= 64 * 1024         # the default LDS suffices: nothing to raise


def test_workspace_sizes_and_their_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    size = lambda *a: lib.wgnn_silhouette_workspace_bytes(*a, C.addressof(nb))
    # one split needs no workspace; s splits hold s + 1 bounds and 20 bytes per split and row, to a multiple of 8
    assert size(0, 1, 0) == 0 and nb.value == 0
    assert size(197, 7, 1) == 0 and nb.value == 0
    assert size(197, 7, 2) == 0 and nb.value == 3 * 8 + 2 * 197 * 20
    assert size(197, 7, 5) == 0 and nb.value == (6 * 8 + 5 * 197 * 20 + 7) // 8 * 8 and nb.value % 8 == 0
    assert size(1, 4096, 64) == 0 and nb.value == 65 * 8 + 64 * 20
    # n_splits = 0: about 4096 workgroups, at least two of the n / 64 candidate tiles and one group per split, at most 64
    assert size(197, 7, 0) == 0 and nb.value == 3 * 8 + 2 * 197 * 20              # 4 query tiles: 2 splits
    assert size(2000, 16, 0) == 0 and nb.value == 17 * 8 + 16 * 2000 * 20          # 32 query tiles: 16 splits
    assert size(2000, 3, 0) == 0 and nb.value == 4 * 8 + 3 * 2000 * 20             # ... but never more than groups
    assert size(20_000, 1024, 0) == 0 and nb.value == 15 * 8 + 14 * 20_000 * 20    # 313 query tiles: ceil(4096 / 313) = 14
    assert size(100_000, 16, 0) == 0 and nb.value == 4 * 8 + 3 * 100_000 * 20
    assert size(1_000_000, 16, 0) == 0 and nb.value == 0                           # enough query tiles alone
    assert size(64, 4, 0) == 0 and nb.value == 0                                   # one query tile, one candidate tile at least
    for bad, code, word in (((-1, 1, 0), -1, b"n must"), ((2 ** 31, 1, 0), -1, b"n must"), ((10, 1, -1), -1, b"n_splits"),
                            ((10, 1, 65), -1, b"n_splits"), ((10, 0, 0), -3, b"K must"), ((10, -2, 0), -3, b"K must"),
                            ((10, 4097, 0), -3, b"K must")):
        assert size(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_silhouette_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_silhouette_workspace_bytes(1, 1, 0, None) == -1


def _host_buffers():
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 4096 * i)


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()
    name = "wgnn_silhouette_rows"

    def run(X=at(0), ld_x=8, n=10, D=8, seg_ptr=at(1), K=3, n_splits=1, a=at(2), b=at(3), s=at(4), nearest=at(5),
            workspace=at(6), workspace_bytes=4096, flags=0):
        return lib.wgnn_silhouette_rows(X, ld_x, n, D, seg_ptr, K, n_splits, a, b, s, nearest, workspace, workspace_bytes,
                                        flags, None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert name.encode() in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    for splits in (-1, 65):
        fails(-1, b"n_splits", n_splits=splits)
    for f in (1, 16, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for operand in ("X", "seg_ptr", "a", "b", "s", "nearest"):
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
    for operand, i in (("seg_ptr", 1), ("a", 2), ("b", 3), ("s", 4)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"4-byte", nearest=at(5) + 2)
    fails(-2, b"8-byte", n_splits=2, workspace=at(6) + 4)
    # WGNN_ERR_WORKSPACE: 10 rows in 2 splits are 3 bounds and 2 x 10 x 20 bytes
    fails(-4, b"workspace", n_splits=2, workspace_bytes=3 * 8 + 400 - 1)
    fails(-4, b"workspace", n_splits=2, workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)
    # an empty batch needs no operand and launches nothing
    assert run(n=0, X=None, seg_ptr=None, a=None, b=None, s=None, nearest=None, workspace=None, workspace_bytes=0) == 0


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(5, 8)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.silhouette_rows(x, torch.zeros(5, dtype=torch.int64), 2)
