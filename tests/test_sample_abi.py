"""``wgnn_sample_rows`` (K5, ``include/wgnn.h``) without a GPU: declared, bound and exported, its draw law written down in the
header, and every refusal returns its code before any launch - host memory stands in for the operands,
``wgnn_last_error_string`` names the check."""
import ctypes as C
import re
import types
from pathlib import Path

import pytest
import torch

from scdeepsort_amd import _lib, sampler

ROOT = Path(__file__).resolve().parent.parent
NAME = "wgnn_sample_rows"
POINTERS = ("rowptr", "col", "val", "step", "out_col", "out_val", "out_cnt", "out_self", "out_inv")      # required; row_ids is not


def test_symbol_is_declared_bound_and_exported():
    raw = (ROOT / "include" / "wgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text) and hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    n_args = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % NAME, text, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES[NAME][1]) == 15
    assert lib.wgnn_version() == 206
    from scdeepsort_amd import build
    assert "wgnn_sample.hip" in [p.name for p in build.SRC]
    assert not any("fast-math" in f or f in ("-Ofast", "-ffp-contract=fast") for f in build.FLAGS)     # out_inv: a rounded division


def test_the_header_and_the_kernel_name_the_constants_of_the_restatement():
    import sample_reference as R
    block = (ROOT / "include" / "wgnn.h").read_text().split("K5  seeded neighbour subsampling")[1].split("int wgnn_sample_rows")[0]
    src = (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_sample.hip").read_text()
    for name in ("K_STEP", "K_STREAM", "K_ROW", "K_DRAW"):
        word = "0x%016X" % getattr(R, name)
        assert "%s = %s" % (name, word) in block and word + "ull" in src, name
    assert len({R.K_STEP, R.K_STREAM, R.K_ROW, R.K_DRAW}) == 4


def test_refusals_return_before_any_launch():
    lib = _lib.lib()
    buf = (C.c_double * 4096)()
    at = lambda i: C.addressof(buf) + 2048 * i
    given = dict(zip(POINTERS, (at(i) for i in range(len(POINTERS)))))

    def run(n_rows=4, k=3, row_ids=None, seed=7, stream_id=0, **kw):
        p = {**given, **kw}
        return lib.wgnn_sample_rows(p["rowptr"], p["col"], p["val"], row_ids, n_rows, k, seed, p["step"], stream_id,
                                    p["out_col"], p["out_val"], p["out_cnt"], p["out_self"], p["out_inv"], None)

    def fails(code, word, **kw):
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code)
        assert NAME.encode() in msg and word in msg, (kw, msg)

    # WGNN_ERR_BAD_ARG: the pointers first, whatever the sizes
    for name in POINTERS:
        fails(-1, b"required", **{name: None})
        fails(-1, b"required", n_rows=0, **{name: None})
        fails(-1, b"required", k=257, **{name: None})
    for n in (-1, -2 ** 40):
        fails(-1, b"n_rows", n_rows=n)
        fails(-1, b"n_rows", n_rows=n, k=257)
    for k in (0, -1, -2 ** 31):
        fails(-1, b"k must be positive", k=k)
        fails(-1, b"k must be positive", k=k, n_rows=0)
    # WGNN_ERR_UNSUPPORTED
    for k in (257, 258, 2 ** 31 - 1):
        fails(-3, b"k must be <= 256", k=k)
        fails(-3, b"k must be <= 256", k=k, n_rows=0)
    # nothing to do: OK, with or without row_ids, at the largest k, for any key - and nothing was written
    assert run(n_rows=0) == 0 and run(n_rows=0, k=256, row_ids=at(9)) == 0
    assert run(n_rows=0, k=1, seed=2 ** 64 - 1, stream_id=-1) == 0
    assert not any(buf)


def test_a_new_call_forgets_the_last_detail():
    lib = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    bad = lambda: lib.wgnn_sample_rows(p, p, p, None, 0, 0, 7, p, 0, p, p, p, p, p, None)
    good = lambda: lib.wgnn_sample_rows(p, p, p, None, 0, 1, 7, p, 0, p, p, p, p, p, None)
    assert bad() == -1 and NAME.encode() in lib.wgnn_last_error_string(-1)
    assert NAME.encode() not in lib.wgnn_last_error_string(-1)         # handed out once
    assert bad() == -1 and good() == 0
    assert NAME.encode() not in lib.wgnn_last_error_string(-1)         # cleared by the call that succeeded


@pytest.mark.parametrize("longest,k", [(256, 257), (256, 10 ** 6), (5000, 257)])
def test_sample_block_static_refuses_more_than_256_draws(longest, k):
    csr = types.SimpleNamespace(device=torch.device("cpu"), max_row_nnz=longest)
    with pytest.raises(_lib.WgnnError, match="at most 256"):
        sampler.sample_block_static(csr, None, k, sampler.DeviceSampler(1, "cpu"), 0)
