"""The ``wgnn_diffusion_*`` / ``wgnn_lanczos_*`` / ``wgnn_basis_combine`` entries (``include/wgnn.h``) without a GPU: declared, bound
and exported, the constants equal the header's, every argument check returns its code before any launch - host memory stands in
for the operands, ``wgnn_last_error_string`` names the check - and the kernels need no scratch and spill nothing.
tests/test_gpu_diffusion_rows.py runs them."""
import ctypes as C
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_diffusion.hip"
ENTRIES = {"wgnn_diffusion_degree": 11, "wgnn_diffusion_weights": 12, "wgnn_lanczos_init": 8, "wgnn_lanczos_apply": 12,
           "wgnn_lanczos_dots_workspace_bytes": 2, "wgnn_lanczos_dots": 14, "wgnn_lanczos_update": 10, "wgnn_lanczos_scale": 8,
           "wgnn_basis_combine": 11, "wgnn_diffusion_distance": 10}


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for entry, n_args in ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % entry, text) and hasattr(lib, entry) and entry in _lib.SIGNATURES, entry
        declared = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1).split(","))
        assert declared == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert lib.wgnn_version() == 206                                   # additive exports
    define = lambda name: re.search(r"#define\s+%s\s+(\S+)" % name, text).group(1)
    assert [int(define("WGNN_DIFFUSION_" + n)) for n in ("UNSORTED", "BAD_COL", "BAD_ROWPTR", "BAD_WEIGHT")] == \
        [_lib.DIFFUSION_UNSORTED, _lib.DIFFUSION_BAD_COL, _lib.DIFFUSION_BAD_ROWPTR, _lib.DIFFUSION_BAD_WEIGHT] == [1, 2, 4, 8]
    assert [bit for bit, _ in ops._DIFFUSION_STATUS] == [1, 2, 4, 8]
    assert int(define("WGNN_DIFFUSION_LANES")) == _lib.DIFFUSION_LANES == ops.DIFFUSION_LANES == 16
    assert int(define("WGNN_DIFFUSION_MAX_BLOCKS")) == _lib.DIFFUSION_MAX_BLOCKS == 8192
    assert int(define("WGNN_DIFFUSION_MAX_COMPS")) == _lib.DIFFUSION_MAX_COMPS == ops.DIFFUSION_MAX_COMPS == 64
    assert int(define("WGNN_LANCZOS_CHUNK")) == _lib.LANCZOS_CHUNK == ops.LANCZOS_CHUNK == 256
    assert int(define("WGNN_LANCZOS_MAX_STEPS")) == _lib.LANCZOS_MAX_STEPS == ops.LANCZOS_MAX_STEPS == 1024
    assert int(define("WGNN_LANCZOS_NORM")) == _lib.LANCZOS_NORM == 256
    assert float.fromhex(define("WGNN_LANCZOS_BREAKDOWN")) == _lib.LANCZOS_BREAKDOWN == ops.LANCZOS_BREAKDOWN == 2.0 ** -26
    from scdeepsort_amd import build
    assert "wgnn_diffusion.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and not re.search(r"\bfmaf?\b", src) and "fp contract(off)" in src      # plain C++, nothing fused
    assert re.findall(r"atomic\w+", src) == ["atomicOr"]               # the status word alone


def test_the_public_names():
    for name in ("graph_components", "diffusion_operator", "lanczos_graph", "lanczos_ritz", "basis_combine", "diffusion_distance"):
        assert getattr(sda, name) is getattr(ops, name) and name in sda.__all__
    assert ops.DiffusionOperator._fields == ("t", "q", "z")
    assert ops.LanczosRows._fields == ("V", "alpha", "beta", "n_run", "breakdown", "n_cells")
    assert (ops.lanczos_steps(9999), ops.lanczos_steps(10000)) == (128, 256)
    for name in ("DiffusionMap", "DiffusionPseudotime"):
        assert name in sda.__all__ and dataclasses.is_dataclass(getattr(sda, name))
    for method in ("diffmap", "diffmap_file", "dpt", "dpt_file"):
        assert hasattr(sda.ResidentPredictor, method)
    assert {"coords", "eigenvalues", "residual", "converged", "n_steps", "breakdown", "in_component", "n_components", "seed", "label",
            "max_prob"} <= {f.name for f in dataclasses.fields(sda.DiffusionMap)}
    assert {"distance", "pseudotime", "roots", "n_dcs", "label", "max_prob"} <= {f.name for f in dataclasses.fields(sda.DiffusionPseudotime)}
    for method in ("by_type", "by_group", "frame", "pseudotime_frame", "summary"):
        assert hasattr(sda.DiffusionPseudotime, method)
    assert sda.DiffusionPseudotime.by_group is sda.Pseudotime.by_group  # shared code, not a copy
    tables_src = (ROOT / "scdeepsort_amd" / "tables.py").read_text()
    assert not re.search(r"^\s*(from|import)\b.*\b(api|ops)\b", tables_src, flags=re.M)    # neither the predictor nor the ops


def test_the_kernels_compile_without_scratch_or_spills(tmp_path):
    """The compiler's own resource remarks for gfx950."""
    import subprocess
    from scdeepsort_amd import build
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(tmp_path / "wgnn_diffusion.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 10
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    assert set(figures("ScratchSize [bytes/lane]")) == {0} and set(figures("VGPRs Spill")) == {0} and set(figures("SGPRs Spill")) == {0}
    assert max(figures("VGPRs")) <= 64                                  # eight waves per SIMD
    lds = dict(zip(names, figures("LDS Size [bytes/block]")))
    assert [v for k, v in lds.items() if "dots_kernel" in k] == [16 * 256 * 8] and sum(lds.values()) == 16 * 256 * 8


def test_the_ritz_step_on_the_host():
    theta, S, res = ops.lanczos_ritz([2.0, 2.0, 2.0], torch.tensor([1.0, 1.0, 0.5], dtype=torch.float64), 3)
    want = 2.0 + np.sqrt(2.0) * np.array([1.0, 0.0, -1.0])
    np.testing.assert_allclose(theta, want, atol=1e-14)
    np.testing.assert_allclose(res, np.abs(0.5 * S[2]), atol=0)
    assert S.shape == (3, 3) and ops.lanczos_ritz([], [], 0)[1].shape == (0, 0)
    assert ops.lanczos_ritz([1.0, 5.0], [0.0, 0.0], 2)[0].tolist() == [5.0, 1.0]      # descending
    with pytest.raises(ValueError):
        ops.lanczos_ritz([1.0], [1.0], 2)


def _host_buffers():
    buf = (C.c_double * 16384)()
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, (lambda i: base + 8192 * i)


def _fails(lib, entry, run):
    def fails(code, word, **kw):
        assert run(**kw) == code, (entry, kw)
        msg = lib.wgnn_last_error_string(code)
        assert entry.encode() in msg and word in msg, (kw, msg)
    return fails


def test_graph_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def degree(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, q=at(3), out=at(4), status=at(5), grid_blocks=0, flags=0):
        return lib.wgnn_diffusion_degree(rowptr, col, w, n, nnz, q, out, status, grid_blocks, flags, None)

    def weights(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, q=at(3), z=at(4), t=at(5), status=at(6), grid_blocks=0, flags=0):
        return lib.wgnn_diffusion_weights(rowptr, col, w, n, nnz, q, z, t, status, grid_blocks, flags, None)

    def apply(rowptr=at(0), col=at(1), t=at(2), n=10, nnz=20, x=at(3), y=at(4), halt=at(5), status=at(6), grid_blocks=0, flags=0):
        return lib.wgnn_lanczos_apply(rowptr, col, t, n, nnz, x, y, halt, status, grid_blocks, flags, None)

    for entry, run, required, wide, narrow, alias in (
            ("wgnn_diffusion_degree", degree, ("rowptr", "col", "w", "out", "status"), ("rowptr", "q", "out", "status"), ("col", "w"),
             dict(out=at(3))),
            ("wgnn_diffusion_weights", weights, ("rowptr", "col", "w", "q", "z", "t", "status"), ("rowptr", "q", "z", "t", "status"),
             ("col", "w"), dict(t=at(4))),
            ("wgnn_lanczos_apply", apply, ("rowptr", "col", "t", "x", "y", "status"), ("rowptr", "t", "x", "y", "halt", "status"),
             ("col",), dict(y=at(3)))):
        fails = _fails(lib, entry, run)
        for operand in required:
            fails(-1, b"required", **{operand: None})
        for n in (-1, 2 ** 31):
            fails(-1, b"n must", n=n)
        fails(-1, b"nnz", nnz=-1)
        for g in (-1, 8193):
            fails(-1, b"grid_blocks", grid_blocks=g)
        for f in (1, 256, 2 ** 31):
            fails(-1, b"flag", flags=f)
        fails(-1, b"another buffer", **alias)
        for operand in wide:
            fails(-2, b"8-byte", **{operand: at(7) + 4})
        for operand in narrow:
            fails(-2, b"4-byte", **{operand: at(7) + 2})
        assert run(n=0) == 0 and run(n=0, nnz=0, grid_blocks=8192) == 0  # nothing to do: no launch
    assert degree(q=None, n=0) == 0 and apply(halt=None, n=0) == 0      # the optional operands


def test_vector_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()
    V, n = at(0), 8                                                     # a basis of up to 8 rows x 8 values in at(0)

    def init(z=at(1), mask=at(2), n=n, seed=0, w0=at(3), w1=at(4), flags=0):
        return lib.wgnn_lanczos_init(z, mask, n, seed, w0, w1, flags, None)

    def dots(V=V, ld=n, n_rows=3, w=at(1), n=n, c=at(2), keep=at(3), halt=at(4), tag=1, workspace=at(5), workspace_bytes=8192,
             grid_blocks=0, flags=0):
        return lib.wgnn_lanczos_dots(V, ld, n_rows, w, n, c, keep, halt, tag, workspace, workspace_bytes, grid_blocks, flags, None)

    def update(V=V, ld=n, n_rows=3, c=at(1), w=at(2), n=n, halt=at(3), grid_blocks=0, flags=0):
        return lib.wgnn_lanczos_update(V, ld, n_rows, c, w, n, halt, grid_blocks, flags, None)

    def scale(w=at(1), beta=at(2), v=at(3), n=n, halt=at(4), grid_blocks=0, flags=0):
        return lib.wgnn_lanczos_scale(w, beta, v, n, halt, grid_blocks, flags, None)

    def combine(V=V, ld=n, m=3, S=at(1), lds=2, n_cols=2, Y=at(2), ldy=3, n=n, flags=0):
        return lib.wgnn_basis_combine(V, ld, m, S, lds, n_cols, Y, ldy, n, flags, None)

    def distance(Y=at(1), ldy=4, n=n, g=at(2), n_dcs=3, roots=at(3), n_roots=1, d=at(4), flags=0):
        return lib.wgnn_diffusion_distance(Y, ldy, n, g, n_dcs, roots, n_roots, d, flags, None)

    fails = _fails(lib, "wgnn_lanczos_init", init)
    for operand in ("z", "mask", "w0", "w1"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"three buffers", w1=at(3))
    fails(-1, b"three buffers", w0=at(1))
    fails(-1, b"n must", n=-1)
    fails(-1, b"flag", flags=1)
    for operand in ("z", "w0", "w1"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert init(n=0) == 0

    fails = _fails(lib, "wgnn_lanczos_dots", dots)
    for operand in ("w", "c", "workspace"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"V is required", V=None)
    fails(-1, b"a norm takes", flags=_lib.LANCZOS_NORM)                 # with a V
    fails(-1, b"a norm takes", flags=_lib.LANCZOS_NORM, V=None, n_rows=2)
    for rows in (0, 1026):
        fails(-1, b"n_rows", n_rows=rows)
    fails(-1, b"ld < n", ld=n - 1)
    fails(-1, b"tag", tag=0)
    fails(-1, b"flag", flags=1)
    for g in (-1, 8193):
        fails(-1, b"grid_blocks", grid_blocks=g)
    fails(-4, b"workspace", workspace_bytes=3 * 8 - 1)
    fails(-1, b"overlap", c=at(1))                                      # c is w
    fails(-1, b"overlap", c=V + 8 * 5)                                  # c inside V
    fails(-1, b"overlap", w=at(5) + 64)                                 # w inside the workspace
    fails(-1, b"overlap", workspace=V + 64)
    for operand in ("V", "w", "c", "keep", "halt", "workspace"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert dots(n=0) == 0 and dots(n=0, V=None, flags=_lib.LANCZOS_NORM, n_rows=1, keep=None, halt=None) == 0
    assert lib.wgnn_lanczos_dots_workspace_bytes(257, 3) == 2 * 3 * 8 and lib.wgnn_lanczos_dots_workspace_bytes(256, 1) == 8

    fails = _fails(lib, "wgnn_lanczos_update", update)
    for operand in ("V", "c", "w"):
        fails(-1, b"required", **{operand: None})
    for rows in (0, 1026):
        fails(-1, b"n_rows", n_rows=rows)
    fails(-1, b"ld < n", ld=n - 1)
    fails(-1, b"overlap", w=V + 8 * n)                                  # w is row 1 of V
    fails(-1, b"overlap", c=V)
    fails(-1, b"overlap", c=at(2))                                      # c is w
    fails(-1, b"flag", flags=256)
    for operand in ("V", "c", "w", "halt"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert update(n=0) == 0 and update(w=V + 8 * 3 * n, n=0) == 0       # the row behind the last one read is free

    fails = _fails(lib, "wgnn_lanczos_scale", scale)
    for operand in ("w", "beta", "v"):
        fails(-1, b"required", **{operand: None})
    fails(-1, b"three buffers", v=at(1))
    fails(-1, b"three buffers", beta=at(3))
    fails(-1, b"flag", flags=1)
    for operand in ("w", "beta", "v", "halt"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert scale(n=0) == 0

    fails = _fails(lib, "wgnn_basis_combine", combine)
    for operand in ("V", "S", "Y"):
        fails(-1, b"required", **{operand: None})
    for m in (-1, 1025):
        fails(-1, b"m must", m=m)
    for cols in (-1, 64):
        fails(-1, b"n_cols", n_cols=cols, ldy=100, lds=100)
    fails(-1, b"ldy", ldy=2)
    fails(-1, b"lds", lds=1)
    fails(-1, b"ld < n", ld=n - 1)
    fails(-1, b"overlap", Y=V + 8 * 2 * n)
    fails(-1, b"overlap", Y=at(1))
    for operand in ("V", "S", "Y"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert combine(n=0) == 0 and combine(n=0, S=None, n_cols=0, lds=0, ldy=1) == 0

    fails = _fails(lib, "wgnn_diffusion_distance", distance)
    for operand in ("Y", "g", "roots", "d"):
        fails(-1, b"required", **{operand: None})
    for dcs in (1, 65):
        fails(-1, b"n_dcs", n_dcs=dcs, ldy=100)
    fails(-1, b"ldy", ldy=2)
    fails(-1, b"n_roots", n_roots=0)
    fails(-1, b"another buffer", d=at(1))
    fails(-1, b"flag", flags=1)
    for operand in ("Y", "g", "roots", "d"):
        fails(-2, b"8-byte", **{operand: at(6) + 4})
    assert distance(n=0) == 0


def test_ops_refuse_cpu_tensors():
    rowptr, col = torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.graph_components(rowptr, col)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.diffusion_operator(rowptr, col, torch.zeros(0))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.lanczos_graph(rowptr, col, torch.zeros(0, dtype=torch.float64), torch.zeros(5, dtype=torch.float64), torch.ones(5, dtype=torch.bool))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.basis_combine(torch.zeros((2, 5), dtype=torch.float64), np.zeros((1, 1)))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.diffusion_distance(torch.zeros((5, 3), dtype=torch.float64), np.zeros(3), 0)
