"""``wgnn_predict_rows_panels`` (``include/wgnn.h``) without a GPU: declared, bound and exported, and every argument check
returns its code before any launch - host memory stands in for the operands, ``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_predict_rows_panels"


def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text) and hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % NAME, text, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES[NAME][1]) == 31
    assert lib.wgnn_version() == 206                                   # an additive export
    assert sda.predict_rows_panels is ops.predict_rows_panels and sda.PanelCalls is sda.api.PanelCalls
    from scdeepsort_amd import build
    assert "wgnn_panels.hip" in [p.name for p in build.SRC]
    src = re.sub(r"//.*", "", (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_panels.hip").read_text())
    assert '#include "wgnn_align_rows.h"' in src and "log1p" not in src and "asm" not in src      # lognorm() is shared, plain C++
    assert "lognorm(" in src


def test_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) // 16 * 16
    at = lambda i: base + 4096 * i

    def run(rowptr=at(0), col=at(1), raw=at(2), n_rows=4, table=at(3), H=8, ld=8, alpha=at(4), bias=at(5), self_rows=None,
            member=at(6), n_panels=3, lib_=None, ld_lib=3, scale=1e4, threshold=0.0, out=at(7), ld_out=None, head=False, b_head=at(9),
            n_classes=5, w_head=at(8), logits=None, ld_logits=5, label=at(10), max_prob=at(11), entries=None, flags=0):
        w = w_head if head else None
        return lib.wgnn_predict_rows_panels(rowptr, col, raw, n_rows, table, ld, 100, H, alpha, bias, self_rows, ld,
                                            member, n_panels, lib_, ld_lib, scale, threshold, None if head else out,
                                            ld if ld_out is None else ld_out, w, b_head if head else None, n_classes if head else 0, 0.1,
                                            logits, ld_logits, label if head else None, max_prob if head else None, entries, flags,
                                            None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert b"wgnn_predict_rows_panels" in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG
    for name in ("rowptr", "col", "raw", "table", "alpha", "bias"):
        fails(-1, b"required", **{name: None})
    fails(-1, b"member", member=None)
    fails(-1, b"member", member=None, head=True)
    for n in (0, -1, 65):
        fails(-1, b"n_panels", n_panels=n)
    fails(-1, b"2^31", n_rows=2 ** 26, n_panels=32)
    fails(-1, b"n_rows", n_rows=2 ** 31)
    fails(-1, b"n_rows", n_rows=-1)
    fails(-1, b"ld_lib", lib_=at(12), ld_lib=2)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        fails(-1, b"scale", lib_=at(12), scale=scale)
    for thr in (-0.5, float("nan")):
        fails(-1, b"threshold", lib_=at(12), threshold=thr)
    assert run(n_rows=0, scale=0.0, threshold=-1.0, ld_lib=0) == 0    # without lib those three are not read
    fails(-1, b"label", head=True, label=None)
    fails(-1, b"max_prob", head=True, max_prob=None)
    fails(-1, b"b_head", head=True, b_head=None)
    fails(-1, b"n_classes", head=True, n_classes=0)
    fails(-1, b"ld_logits", head=True, logits=at(13), ld_logits=4)
    fails(-1, b"out", out=None)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=1)
    fails(-1, b"WGNN_FLAG_ROWPTR_I64", flags=16 | 256)
    # WGNN_ERR_ALIGNMENT
    fails(-2, b"multiple of 4", H=10, ld=12)
    fails(-2, b"ld_table", ld=6)
    fails(-2, b"16-byte", table=at(3) + 4)
    fails(-2, b"16-byte", bias=at(5) + 8)
    fails(-2, b"self_rows", self_rows=at(13) + 4)
    fails(-2, b"8-byte", member=at(6) + 4)
    fails(-2, b"8-byte", lib_=at(12) + 4)
    fails(-2, b"entries", entries=at(13) + 2)
    fails(-2, b"ld_out", out=at(7) + 4)
    fails(-2, b"ld_out", ld_out=4)
    fails(-2, b"w_head", head=True, w_head=at(8) + 8)
    fails(-2, b"4-byte", head=True, label=at(10) + 2)
    fails(-2, b"4-byte", head=True, max_prob=at(11) + 1)
    # WGNN_ERR_UNSUPPORTED
    fails(-3, b"256", H=260, ld=260)
    fails(-3, b"64 KiB", head=True, H=256, ld=256, n_classes=65)
    # an empty batch is a no-op in every mode; the limits themselves pass the checks
    assert run(n_rows=0) == 0 and run(n_rows=0, head=True, flags=16) == 0 and run(n_rows=0, lib_=at(12)) == 0
    assert run(n_rows=0, n_panels=64, head=True, H=256, ld=256, n_classes=64, logits=at(13), ld_logits=64, entries=at(14)) == 0


def test_ops_refuses_cpu_tensors():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    args = (rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, 8), torch.ones(5), torch.zeros(8))
    with pytest.raises(sda.WgnnError):
        sda.predict_rows_panels(*args, torch.zeros(3, dtype=torch.int64), 2)
