"""``wgnn_fuzzy_rows``, ``wgnn_fuzzy_union``, ``wgnn_layout_init`` and ``wgnn_layout_epoch`` (``include/wgnn.h``) without a GPU:
declared, bound and exported, every argument check returns its code before any launch - host memory stands in for the operands,
``wgnn_last_error_string`` names the check - and the kernels keep everything in registers, with no atomics and no LDS."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "scdeepsort_amd" / "csrc" / "wgnn_umap.hip"
ENTRIES = (("wgnn_fuzzy_rows", 12), ("wgnn_fuzzy_union", 11), ("wgnn_layout_init", 5), ("wgnn_layout_epoch", 19))
KERNELS = ("fuzzy_rows_kernel", "fuzzy_union_kernel", "layout_init_kernel", "layout_epoch_kernel")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name, n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.SIGNATURES
        n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) == n
    assert lib.wgnn_version() == 206                                   # additive exports
    for name, value in (("WGNN_FUZZY_IDX_I64", _lib.FUZZY_IDX_I64), ("WGNN_LAYOUT_LANES", _lib.LAYOUT_LANES),
                        ("WGNN_LAYOUT_MAX_EPOCHS", _lib.LAYOUT_MAX_EPOCHS), ("WGNN_LAYOUT_MAX_NEG", _lib.LAYOUT_MAX_NEG)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value
    assert (_lib.LAYOUT_LANES, _lib.FUZZY_MAX_K, ops.FUZZY_MAX_K, ops.LAYOUT_LANES) == (16, 64, 64, 16)
    # the float and double arguments travel as such
    assert _lib.SIGNATURES["wgnn_fuzzy_rows"][1][6] is C.c_double
    assert [i for i, t in enumerate(_lib.SIGNATURES["wgnn_layout_epoch"][1]) if t is C.c_float] == [5, 10, 11, 12, 13]
    for name in ("fuzzy_graph", "layout_graph", "layout_curve"):
        assert getattr(sda, name) is getattr(ops, name)
    assert sda.Layout is sda.api.Layout and sda.api.LayoutSummary is sda.tables.LayoutSummary
    for method in ("umap", "umap_file"):
        assert hasattr(sda.ResidentPredictor, method)
    from scdeepsort_amd import build
    assert "wgnn_umap.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", SOURCE.read_text())
    assert "asm" not in src and "atomic" not in src and "__shared__" not in src and "fmaf" not in src
    assert "#pragma clang fp contract(off)" in src                      # every operation of the contract is rounded on its own


def test_the_kernels_compile_without_scratch_and_fused_multiply_adds(tmp_path):
    """The compiler's own resource remarks for gfx950: every kernel keeps everything in registers and uses no LDS; and the only
    float32 fused multiply-adds in the assembly are those of the correctly rounded divisions and of sqrtf."""
    import subprocess
    from scdeepsort_amd import build
    out = tmp_path / "wgnn_umap.s"
    r = subprocess.run([build.hipcc(), *build.FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(SOURCE), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == len(KERNELS)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel
    figures = lambda what: [int(v) for v in re.findall(r"%s: (\d+)" % re.escape(what), r.stderr)]
    n = len(KERNELS)
    assert figures("ScratchSize [bytes/lane]") == [0] * n and figures("VGPRs Spill") == [0] * n and figures("SGPRs Spill") == [0] * n
    assert figures("LDS Size [bytes/block]") == [0] * n
    asm = out.read_text()
    body = asm[asm.index("layout_epoch_kernel"):]
    # r, the attraction's two quotients and the repulsion's one: four divisions of five fused steps each, and nothing else fused
    assert len(re.findall(r"\bv_div_fixup_f32\b", body)) == 4
    assert len(re.findall(r"\bv_(fma|fmac|mad|mac)_f32", body)) == 4 * 5


def test_curve_and_epoch_defaults():
    a, b = ops.layout_curve()
    assert abs(a - 1.5769) < 1e-3 and abs(b - 0.8951) < 1e-3          # umap-learn's values for min_dist 0.1, spread 1
    assert (round(a, 3), round(b, 3)) == (ops.LAYOUT_A, ops.LAYOUT_B)
    a2, b2 = ops.layout_curve(0.5, 1.0)
    assert a2 < a and b2 > b                                            # a wider plateau: a flatter, later drop
    for bad in ((-0.1, 1.0), (2.0, 1.0), (0.1, 0.0), (0.1, float("inf"))):
        with pytest.raises(ValueError):
            ops.layout_curve(*bad)
    assert ops.layout_epochs(9999) == 500 and ops.layout_epochs(10000) == 200


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


def test_fuzzy_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def rows(idx=at(0), ld_idx=8, d2=at(1), ld_d2=8, n=10, k=8, target=3.17, rho=at(2), sigma=at(3), member=at(4), flags=0):
        return lib.wgnn_fuzzy_rows(idx, ld_idx, d2, ld_d2, n, k, target, rho, sigma, member, flags, None)

    fails = _fails(lib, "wgnn_fuzzy_rows", rows)
    for operand in ("idx", "d2", "rho", "sigma", "member"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    for kw in (dict(ld_idx=7), dict(ld_d2=7)):
        fails(-1, b"ld_idx", **kw)
    for target in (0.0, -1.0, float("inf"), float("nan")):
        fails(-1, b"target", target=target)
    for f in (1, 16, 512, 2 ** 31):
        fails(-1, b"flag", flags=f)
    for k in (0, -1, 65, 1000):
        fails(-3, b"k must", k=k, ld_idx=1000, ld_d2=1000)
    for operand, i in (("rho", 2), ("sigma", 3)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    fails(-2, b"8-byte", idx=at(0) + 4, flags=_lib.FUZZY_IDX_I64)
    for operand, i in (("idx", 0), ("d2", 1), ("member", 4)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert rows(n=0) == 0

    def union(idx=at(0), ld_idx=8, member=at(1), n=10, k=8, rowptr=at(2), col=at(3), nnz=20, w=at(4), flags=0):
        return lib.wgnn_fuzzy_union(idx, ld_idx, member, n, k, rowptr, col, nnz, w, flags, None)

    fails = _fails(lib, "wgnn_fuzzy_union", union)
    for operand in ("idx", "member", "rowptr", "col", "w"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"ld_idx", ld_idx=7)
    fails(-1, b"flag", flags=1)
    for k in (0, 65):
        fails(-3, b"k must", k=k, ld_idx=1000)
    fails(-2, b"8-byte", rowptr=at(2) + 4)
    fails(-2, b"8-byte", idx=at(0) + 4, flags=_lib.FUZZY_IDX_I64)
    for operand, i in (("idx", 0), ("member", 1), ("col", 3), ("w", 4)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert union(n=0) == 0 and union(nnz=0) == 0


def test_layout_errors_return_before_any_launch():
    lib = _lib.lib()
    buf, at = _host_buffers()

    def init(y=at(0), n=10, seed=0, flags=0):
        return lib.wgnn_layout_init(y, n, seed, flags, None)

    fails = _fails(lib, "wgnn_layout_init", init)
    fails(-1, b"required", y=None)
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"flag", flags=1)
    fails(-2, b"4-byte", y=at(0) + 2)
    assert init(n=0) == 0

    def epoch(rowptr=at(0), col=at(1), w=at(2), n=10, nnz=20, wmax=1.0, y_in=at(3), y_out=at(4), epoch=0, n_epochs=10, a=1.5, b=0.9,
              gamma=1.0, alpha=1.0, n_neg=5, seed=0, fired=at(5), flags=0):
        return lib.wgnn_layout_epoch(rowptr, col, w, n, nnz, wmax, y_in, y_out, epoch, n_epochs, a, b, gamma, alpha, n_neg, seed,
                                     fired, flags, None)

    fails = _fails(lib, "wgnn_layout_epoch", epoch)
    for operand in ("rowptr", "col", "w", "y_in", "y_out"):
        fails(-1, b"required", **{operand: None})
    for n in (-1, 2 ** 31):
        fails(-1, b"n must", n=n)
    fails(-1, b"nnz", nnz=-1)
    fails(-1, b"another buffer", y_out=at(3))
    for kw in (dict(n_epochs=0), dict(n_epochs=10001)):
        fails(-1, b"n_epochs", **kw)
    for kw in (dict(epoch=-1), dict(epoch=10)):
        fails(-1, b"epoch must", **kw)
    for n_neg in (-1, 65):
        fails(-1, b"n_neg", n_neg=n_neg)
    for wmax in (0.0, -1.0, float("inf"), float("nan")):
        fails(-1, b"wmax", wmax=wmax)
    for name in ("a", "b", "gamma", "alpha"):
        for value in (float("inf"), float("nan")):
            fails(-1, b"finite", **{name: value})
    fails(-1, b"flag", flags=1)
    for operand, i in (("rowptr", 0), ("y_in", 3), ("y_out", 4), ("fired", 5)):
        fails(-2, b"8-byte", **{operand: at(i) + 4})
    for operand, i in (("col", 1), ("w", 2)):
        fails(-2, b"4-byte", **{operand: at(i) + 2})
    assert epoch(n=0) == 0
    assert epoch(n=0, fired=None) == 0                                  # fired is optional


def test_ops_refuse_cpu_tensors():
    idx, d2 = torch.zeros((5, 3), dtype=torch.int64), torch.zeros((5, 3))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.fuzzy_graph(idx, d2)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.layout_graph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), "hash")
