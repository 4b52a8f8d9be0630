"""The ``wgnn_harmony_*`` / ``wgnn_weighted_group_reduce`` entries and their workspace queries (``include/wgnn.h``) without a GPU:
declared, bound and exported, every argument check returns its code before any launch - host memory stands in for the operands,
``wgnn_last_error_string`` names the check - and the kernels keep everything in registers."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_harmony.hip"
ENTRIES = (("wgnn_harmony_scores", 13), ("wgnn_harmony_assign_workspace_bytes", 5), ("wgnn_harmony_assign_block", 14),
           ("wgnn_harmony_fold", 16), ("wgnn_weighted_group_reduce_workspace_bytes", 5), ("wgnn_weighted_group_reduce", 16),
           ("wgnn_harmony_objective_workspace_bytes", 2), ("wgnn_harmony_objective", 15), ("wgnn_harmony_apply", 14))
KERNELS = ("scores_kernel", "assign_kernel", "fold_kernel", "wgr_chunk_kernel", "wgr_finish_kernel", "objective_chunk_kernel",
           "objective_finish_kernel", "apply_kernel")


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    for name in ("harmony_scores", "harmony_assign_block", "harmony_fold", "weighted_group_reduce", "harmony_objective",
                 "harmony_apply", "harmony_rows"):
        assert getattr(sda, name) is getattr(ops, name)
    assert (ops.HARMONY_MAX_K, ops.HARMONY_MAX_BATCHES, ops.HARMONY_MAX_D, ops.HARMONY_MAX_BLOCKS) == (256, 64, 1024, 64)
    header = (ROOT / "include" / "wgnn.h").read_text()
    for macro, value in (("WGNN_HARMONY_MAX_K", _lib.HARMONY_MAX_K), ("WGNN_HARMONY_MAX_BATCHES", _lib.HARMONY_MAX_BATCHES),
                         ("WGNN_HARMONY_MAX_D", _lib.HARMONY_MAX_D), ("WGNN_HARMONY_MAX_BLOCKS", _lib.HARMONY_MAX_BLOCKS),
                         ("WGNN_HARMONY_T_CHUNK", _lib.HARMONY_T_CHUNK), ("WGNN_HARMONY_W_CHUNK", _lib.HARMONY_W_CHUNK),
                         ("WGNN_HARMONY_OBJ_CHUNK", _lib.HARMONY_OBJ_CHUNK)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == value
    from scdeepsort_amd import build
    assert "wgnn_harmony.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and not re.search(r"\batomic\w*\s*\(", src, flags=re.I)      # plain C++, no atomic at all
    assert "#pragma clang fp contract(off)" in src and not re.search(r"\bfmaf?\s*\(", src)
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*from\s+\.?(api|ops)\b|^\s*from\s+\.\s+import\s+.*\b(api|ops)\b|^\s*import\s+.*\b(api|ops)\b",
                         tables_src, flags=re.M)


def test_the_reference_shares_the_chunks():
    import harmony_reference as hr
    assert (hr.T_CHUNK, hr.W_CHUNK, hr.OBJ_CHUNK) == (_lib.HARMONY_T_CHUNK, _lib.HARMONY_W_CHUNK, _lib.HARMONY_OBJ_CHUNK)


def test_the_kernels_compile_without_scratch(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel of wgnn_harmony.hip keeps everything in registers."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_harmony.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == len(KERNELS)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    zeros = [0] * len(KERNELS)
    assert figures("ScratchSize [bytes/lane]") == zeros and figures("VGPRs Spill") == zeros and figures("SGPRs Spill") == zeros
    assert max(figures("LDS Size [bytes/block]")) <= 64 * 1024


def test_workspace_sizes_and_their_checks():
    lib = _lib.lib()
    nb = C.c_int64(-1)
    assign = lambda *a: lib.wgnn_harmony_assign_workspace_bytes(*a, C.addressof(nb))
    assert assign(1, 1, 1, 1) == 0 and nb.value == 8                   # one chunk, one entry
    assert assign(19, 7, 3, 20) == 0 and nb.value == 7 * 3 * 8         # block 0 holds one cell
    assert assign(1000, 100, 4, 20) == 0 and nb.value == 1 * 100 * 4 * 8       # 50 members: one chunk of 64
    assert assign(100_000, 256, 64, 1) == 0 and nb.value == 1563 * 256 * 64 * 8
    for bad, code, word in (((0, 1, 1, 1), -1, b"n_rows"), ((2 ** 31, 1, 1, 1), -1, b"n_rows"), ((10, 0, 1, 1), -3, b"K must"),
                            ((10, 257, 1, 1), -3, b"K must"), ((10, 1, 0, 1), -3, b"S must"), ((10, 1, 65, 1), -3, b"S must"),
                            ((10, 1, 1, 0), -3, b"n_blocks"), ((10, 1, 1, 65), -3, b"n_blocks")):
        assert assign(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_harmony_assign_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_harmony_assign_workspace_bytes(1, 1, 1, 1, None) == -1

    wgr = lambda *a: lib.wgnn_weighted_group_reduce_workspace_bytes(*a, C.addressof(nb))
    assert wgr(1, 1, 1, 1) == 0 and nb.value == 1 * 1 * 2 * 8          # one slot: a moment and a weight
    assert wgr(1000, 7, 3, 8) == 0 and nb.value == (3 + 3) * 7 * 9 * 8
    assert wgr(100_000, 100, 16, 200) == 0 and nb.value == (390 + 16) * 100 * 201 * 8
    for bad, code, word in (((0, 1, 1, 1), -1, b"n_rows"), ((1, 257, 1, 1), -3, b"K must"), ((1, 1, 65, 1), -3, b"S must"),
                            ((1, 1, 1, 0), -3, b"D must"), ((1, 1, 1, 1025), -3, b"D must")):
        assert wgr(*bad) == code, bad
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_weighted_group_reduce_workspace_bytes" in msg and word in msg, (bad, msg)
    assert lib.wgnn_weighted_group_reduce_workspace_bytes(1, 1, 1, 1, None) == -1

    obj = lambda n: lib.wgnn_harmony_objective_workspace_bytes(n, C.addressof(nb))
    assert obj(1) == 0 and nb.value == 24 and obj(256) == 0 and nb.value == 24 and obj(257) == 0 and nb.value == 48
    assert obj(0) == -1 and obj(2 ** 31) == -1 and lib.wgnn_harmony_objective_workspace_bytes(1, None) == -1


def _host_buffers():
    buf = (C.c_double * 16384)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 4096 * i)


def _checker(name, run):
    lib = _lib.lib()

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert name.encode() in msg and word in msg, (kw, msg)
    return fails


def _common(fails, *, has_s=True, has_d=False, has_blocks=False, has_grid=False):
    for n in (0, -1, 2 ** 31):
        fails(-1, b"n_rows", n_rows=n)
    for K in (0, -1, 257):
        fails(-3, b"K must", K=K)
    if has_s:
        for S in (0, 65):
            fails(-3, b"S must", S=S)
    if has_d:
        for D in (0, -4, 1025):
            fails(-3, b"D must", D=D)
    if has_blocks:
        for nb in (0, 65):
            fails(-3, b"n_blocks", n_blocks=nb)
    if has_grid:
        for g in (-1, 65537):
            fails(-1, b"grid_blocks", grid_blocks=g)
    for f in (1, 256, 2 ** 31):
        fails(-1, b"flag", flags=f)


def test_scores_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(U=at(0), ld_u=8, Y=at(1), ld_y=8, n_rows=10, D=8, K=3, sigma=0.1, dot=at(2), dist=at(3), e=at(4), flags=0):
        return lib.wgnn_harmony_scores(U, ld_u, Y, ld_y, n_rows, D, K, sigma, dot, dist, e, flags, None)

    fails = _checker("wgnn_harmony_scores", run)
    _common(fails, has_s=False, has_d=True)
    for s in (0.0, -1.0, float("inf"), float("nan")):
        fails(-1, b"sigma", sigma=s)
    for operand in ("U", "Y", "dist", "e"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"ld_u", ld_u=7)
    fails(-1, b"ld_u", ld_y=7)
    for operand, i in (("U", 0), ("Y", 1), ("dot", 2), ("dist", 3), ("e", 4)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})


def test_assign_and_fold_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(e=at(0), batch=at(1), pen=at(2), n_rows=10, K=3, S=2, n_blocks=4, q=0, R=at(3), workspace=at(4), workspace_bytes=4096,
            grid_blocks=0, flags=0):
        return lib.wgnn_harmony_assign_block(e, batch, pen, n_rows, K, S, n_blocks, q, R, workspace, workspace_bytes, grid_blocks,
                                             flags, None)

    fails = _checker("wgnn_harmony_assign_block", run)
    _common(fails, has_blocks=True, has_grid=True)
    for q in (-1, 4):
        fails(-1, b"q must", q=q)
    for operand in ("e", "batch", "R"):
        fails(-1, b"required", **{operand: None})
    for operand, i in (("e", 0), ("pen", 2), ("R", 3)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"4-byte", batch=at(1) + 2)
    fails(-2, b"8-byte", workspace=at(4) + 4)
    fails(-4, b"workspace", workspace_bytes=3 * 2 * 8 - 1)             # 10 rows in 4 blocks: one chunk of a [3, 2] table
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)

    def run(workspace=at(4), workspace_bytes=4096, n_rows=10, T=at(0), Pr=at(1), theta=at(2), K=3, S=2, n_blocks=4, q_store=0,
            q_skip=1, O=at(3), E=at(5), pen=at(6), flags=0):
        return lib.wgnn_harmony_fold(workspace, workspace_bytes, n_rows, T, Pr, theta, K, S, n_blocks, q_store, q_skip, O, E, pen,
                                     flags, None)

    fails = _checker("wgnn_harmony_fold", run)
    _common(fails, has_blocks=True)
    for kw in (dict(q_store=-2), dict(q_store=4), dict(q_skip=-2), dict(q_skip=4)):
        fails(-1, b"q_store", **kw)
    for operand in ("T", "Pr", "O", "E"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"theta", theta=None)
    for operand, i in (("T", 0), ("Pr", 1), ("theta", 2), ("O", 3), ("E", 5), ("pen", 6)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-4, b"workspace", workspace_bytes=3 * 2 * 8 - 1)
    fails(-4, b"workspace", workspace=None)
    fails(-2, b"8-byte", workspace=at(4) + 4)


def test_reduce_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(X=at(0), ld_x=8, R=at(1), order=at(2), seg_ptr=at(3), n_rows=10, D=8, K=3, S=2, M=at(4), n=at(5), workspace=at(6),
            workspace_bytes=4096, grid_blocks=0, flags=0):
        return lib.wgnn_weighted_group_reduce(X, ld_x, R, order, seg_ptr, n_rows, D, K, S, M, n, workspace, workspace_bytes,
                                              grid_blocks, flags, None)

    fails = _checker("wgnn_weighted_group_reduce", run)
    _common(fails, has_d=True, has_grid=True)
    for operand in ("X", "R", "order", "seg_ptr", "M", "n"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"ld_x", ld_x=7)
    for operand, i in (("X", 0), ("R", 1), ("seg_ptr", 3), ("M", 4), ("n", 5)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"4-byte", order=at(2) + 2)
    fails(-2, b"8-byte", workspace=at(6) + 4)
    fails(-4, b"workspace", workspace_bytes=2 * 3 * 9 * 8 - 1)         # 10 rows in 2 groups: 2 slots of [3, 8 + 1]
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)


def test_objective_and_apply_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def run(R=at(0), dist=at(1), batch=at(2), O=at(3), E=at(4), theta=at(5), n_rows=10, K=3, S=2, sigma=0.1, out=at(6),
            workspace=at(7), workspace_bytes=4096, flags=0):
        return lib.wgnn_harmony_objective(R, dist, batch, O, E, theta, n_rows, K, S, sigma, out, workspace, workspace_bytes, flags,
                                          None)

    fails = _checker("wgnn_harmony_objective", run)
    _common(fails)
    for s in (0.0, -1.0, float("inf"), float("nan")):
        fails(-1, b"sigma", sigma=s)
    for operand in ("R", "dist", "batch", "O", "E", "theta", "out"):
        fails(-1, b"required", **{operand: None})
    for operand, i in (("R", 0), ("dist", 1), ("O", 3), ("E", 4), ("theta", 5), ("out", 6)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"4-byte", batch=at(2) + 2)
    fails(-2, b"8-byte", workspace=at(7) + 4)
    fails(-4, b"workspace", workspace_bytes=23)
    fails(-4, b"workspace", workspace=None)
    fails(-4, b"workspace", workspace_bytes=-1)

    def run(Z0=at(0), ld_z=8, R=at(1), W=at(2), batch=at(3), n_rows=10, D=8, K=3, S=2, Zc=at(4), U=at(5), grid_blocks=0, flags=0):
        return lib.wgnn_harmony_apply(Z0, ld_z, R, W, batch, n_rows, D, K, S, Zc, U, grid_blocks, flags, None)

    fails = _checker("wgnn_harmony_apply", run)
    _common(fails, has_d=True, has_grid=True)
    for operand in ("Z0", "U"):
        fails(-1, b"required", **{operand: None})
    for operand in ("W", "batch", "Zc"):
        fails(-1, b"with R", **{operand: None})
    fails(-1, b"ld_z", ld_z=7)
    for operand, i in (("Z0", 0), ("R", 1), ("W", 2), ("Zc", 4), ("U", 5)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"4-byte", batch=at(3) + 2)


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(5, 8, dtype=torch.float64)
    b = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.harmony_scores(x, x, 0.1)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.harmony_assign_block(x, b, 1, 2, 0, x.clone())
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.weighted_group_reduce(x, x, None, 1)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.harmony_apply(x)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.harmony_rows(torch.ones(5, 8), b.long(), 2, n_clusters=2)
