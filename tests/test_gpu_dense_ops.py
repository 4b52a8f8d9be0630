"""The dense half of a layer and the training glue - ``wgnn_linear_fwd[_ex]`` (``linear_mfma_f32<TX, DUAL, MI>``),
``wgnn_linear_wgrad`` (``wgrad_mfma_f32`` + ``wgrad_reduce``), ``wgnn_agg_bwd_prepare`` (``agg_bwd_prepare`` + ``fold_rows``) and
``wgnn_ce_sum_fwd_bwd`` (``ce_sum_rows`` + ``fold_scalar``) - against the fp64 reference ``oracle/dense_half.py``, called through
the C ABI (``_lib.call``): the ``ops`` wrappers cannot reach most of the options below.

Three groups:

* **exact** - operands on a dyadic lattice (exact in fp16 too) or saturated cross-entropy rows: the kernels must equal the fp64
  reference BIT FOR BIT (``torch.equal``).  The case tables are ``oracle.dense_half.*_EXACT_CASES``; that the demand is fair for
  every tuple (``sum|terms| / unit < 2**24``, an fp32 evaluation in random order gives the same bits, no case passes by vacuity)
  is checked without a GPU in ``tests/test_dense_half_reference.py``, and asserted again here on the reference of each case.
* **float** - standard-normal operands, tolerance per element ``float_bound(abs_sum, n_terms)`` from the reference, no constant in
  the test (unsaturated cross-entropy keeps the project's 2e-6: ``expf`` / ``logf`` accuracy is the device library's).  Every case
  prints its worst ``err / bound``.
* **error returns** that launch nothing.

Every output is an inner view of a larger SENTINEL-filled tensor - guard rows before and after, guard columns through
``ld > width`` - and the sentinels are checked after each call; the scratch workspaces carry guards as well.  Outputs start
filled with FILL, so an element the kernel skipped fails the comparison.

Option -> test:

    all eight linear_mfma_f32 instantiations, tile 64 / 128 / auto ..... test_linear_fwd_exact (9 shapes each)
    bias NULL, ReLU, ld_x > K, ld_w > K, ld_out > N, ld_out_scaled != ld_out, out == NULL ... test_linear_fwd_exact
    M == 0, wgnn_linear_fwd == _ex ...................................... test_linear_fwd_empty_and_plain_entry
    wgrad: caller-chosen n_slabs, accumulate, ld_g / ld_x / ld_dw ....... test_linear_wgrad_exact
    agg_bwd_prepare: R > 8192 (grid-stride), D up to 1024, modes, out / inv_deg NULL, each output alone, ld > D
                                                                          test_agg_bwd_prepare_exact, _empty
    ce: ld_logits / ld_dlogits > C, dlogits NULL, -100 rows, a label out of range ... test_ce_sum_exact, _bad_label
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_backward_ops as GB
from oracle import agg_backward as AB
from oracle import dense_half as DH
from scdeepsort_amd import _lib
from scdeepsort_amd.graph import _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, FILL = GB.SENTINEL, -777.0
FORCE_TILE = {64: 1 << 16, 128: 1 << 17, "auto": 0}          # wgnn_linear_fwd_ex's tile-height switches (wgnn_linear.hip)
OK, BAD_ARG, ALIGNMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -4


# ---- helpers -------------------------------------------------------------------------------------------------------------
def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype)


def guarded(inner, pad_cols=0):
    """A device tensor ([n, D] or [n]) copied into a larger SENTINEL-filled one: guard row(s) / elements on each side and
    ``pad_cols`` guard columns left and right (ld = D + 2 * pad_cols).  Returns (whole, view)."""
    if inner.dim() == 1:
        whole = torch.full((inner.shape[0] + 8,), SENTINEL, device=DEV, dtype=inner.dtype)
        view = whole[4:4 + inner.shape[0]]
    else:
        n, D = inner.shape
        whole = torch.full((n + 2, D + 2 * pad_cols), SENTINEL, device=DEV, dtype=inner.dtype)
        view = whole[1:n + 1, pad_cols:pad_cols + D]
    view.copy_(inner)
    return whole, view


def fresh(*shape, pad_cols=0):
    """A guarded output that holds FILL (what no kernel result here equals)."""
    return guarded(torch.full(shape, FILL, device=DEV), pad_cols)


def wide(x, on):
    """An INPUT with ld = width + 8 inside SENTINEL columns (a kernel that reads past the width computes with 12345)."""
    return guarded(x, 4)[1] if on else x


def call(name, *args):
    d = torch.device(DEV)
    return _lib.call(d, name, *args, _stream(d))


def intact(*pairs):
    torch.cuda.synchronize()
    return all(GB.guards_intact(whole, view) for whole, view in pairs)


RATIOS = {}


def record_ratio(entry, what, got, want64, bound):
    r = AB.worst_ratio(got.detach().cpu().numpy(), want64, bound)
    RATIOS[entry] = max(RATIOS.get(entry, 0.0), r)
    print(f"RATIO entry={entry} output={what} err/bound={r:.4f} worst_so_far={RATIOS[entry]:.4f}")
    return r


# ---- wgnn_linear_fwd_ex -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lin_operands(M, N, K):
    L = DH.lattice_linear(M, N, K, DH.case_seed("lin", M, N, K))
    return L, dict(f32=dev(L["x"]), f16=dev(L["x"], torch.float16), w=dev(L["w"]), bias=dev(L["bias"]), rs=dev(L["row_scale"]))


def linear_ex(x, w, bias, out, rs, out2, M, N, K, flags):
    return call("wgnn_linear_fwd_ex", _ptr(x), _lib.F16 if x.dtype == torch.float16 else _lib.F32, x.stride(0) if M else K, _ptr(w),
                w.stride(0), _ptr(bias), _ptr(out), out.stride(0) if out is not None else 0, _ptr(rs), _ptr(out2),
                out2.stride(0) if out2 is not None else 0, M, N, K, flags)


@pytest.mark.parametrize("case", DH.LINEAR_EXACT_CASES, ids=DH.lin_id)
def test_linear_fwd_exact(case):
    dt, dual, tile, M, N, K, bias, relu, ldx, ldw, ldo, null_out = case
    L, T = lin_operands(M, N, K)
    ref = DH.linear_fwd(L["x"], L["w"], L["bias"] if bias else None, relu, L["row_scale"] if dual else None)
    assert DH.linear_budget(ref, L["row_scale"] if dual else None) < 24
    x, w = wide(T[dt], ldx), wide(T["w"], ldw)
    o = None if null_out else fresh(M, N, pad_cols=3 if ldo else 0)
    o2 = fresh(M, N, pad_cols=5 if ldo else 0) if dual else None
    rc = linear_ex(x, w, T["bias"] if bias else None, o and o[1], T["rs"] if dual else None, o2 and o2[1], M, N, K,
                   (_lib.FLAG_RELU if relu else 0) | FORCE_TILE[tile])
    assert rc == OK
    assert intact(*[p for p in (o, o2) if p])
    if o:
        GB.assert_exact(o[1], ref["out"], "out")
    if dual:
        GB.assert_exact(o2[1], ref["out_scaled"], "out_scaled")
        if o:
            assert torch.equal(o2[1], T["rs"][:, None] * o[1])


def test_linear_fwd_empty_and_plain_entry():
    """M == 0 returns WGNN_OK and touches nothing; wgnn_linear_fwd gives the bits of wgnn_linear_fwd_ex."""
    M, N, K = 129, 33, 52
    L, T = lin_operands(M, N, K)
    o, o2 = fresh(M, N, pad_cols=3), fresh(M, N, pad_cols=5)
    assert linear_ex(T["f32"], T["w"], T["bias"], o[1], T["rs"], o2[1], 0, N, K, _lib.FLAG_RELU) == OK
    torch.cuda.synchronize()
    assert bool((o[1] == FILL).all()) and bool((o2[1] == FILL).all()) and intact(o, o2)
    assert linear_ex(T["f32"], T["w"], T["bias"], o[1], None, None, M, N, K, _lib.FLAG_RELU) == OK
    p = fresh(M, N, pad_cols=3)
    x = wide(T["f32"], True)
    assert call("wgnn_linear_fwd", _ptr(x), x.stride(0), _ptr(T["w"]), K, _ptr(T["bias"]), _ptr(p[1]), p[1].stride(0), M, N, K,
                _lib.FLAG_RELU) == OK
    assert intact(o, p) and torch.equal(o[1], p[1])
    GB.assert_exact(p[1], DH.linear_fwd(L["x"], L["w"], L["bias"], True)["out"], "wgnn_linear_fwd")


@pytest.mark.parametrize("M,N,K,dt", DH.LINEAR_FLOAT_CASES)
def test_linear_fwd_float(M, N, K, dt):
    gen = torch.Generator(device=DEV).manual_seed(DH.case_seed("flin", M, N, K))
    x = torch.randn(M, K, generator=gen, device=DEV)
    w, b, rs = torch.randn(N, K, generator=gen, device=DEV), torch.randn(N, generator=gen, device=DEV), torch.rand(M, generator=gen, device=DEV) + 0.5
    if dt == "f16":
        x = x.half()
    ref = DH.linear_fwd(x.float().cpu().numpy(), w.cpu().numpy(), b.cpu().numpy())        # on the fp16-rounded inputs
    bound = AB.float_bound(ref["abs_sum"], K + 1)
    for tile in (64, 128, "auto"):
        o, o2 = fresh(M, N, pad_cols=3), fresh(M, N, pad_cols=5)
        assert linear_ex(x, w, b, o[1], rs, o2[1], M, N, K, FORCE_TILE[tile]) == OK
        assert intact(o, o2)
        assert record_ratio("linear_fwd", f"out[{dt},tile{tile}]", o[1], ref["out"], bound) <= 1
        assert torch.equal(o2[1], rs[:, None] * o[1])


# ---- wgnn_linear_wgrad --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wg_operands(M, N, K):
    L = DH.lattice_wgrad(M, N, K, DH.case_seed("wg", M, N, K))
    return L, dict(g=dev(L["g"]), x=dev(L["x"]), prior=dev(L["prior"]))


def wgrad_slabs(M, N, K, kind):
    if kind == "ws":
        ns, nb = C.c_int64(), C.c_int64()
        assert _lib.lib().wgnn_linear_wgrad_workspace(M, N, K, C.addressof(ns), C.addressof(nb)) == OK
        assert nb.value == ns.value * N * K * 4
        return int(ns.value)
    return M // 16 + 3 if kind == "over" else kind


def wgrad(g, x, prior, M, N, K, n_slabs, lddw):
    """One call on fresh guarded buffers; returns the dW view after checking every guard (the workspace's too)."""
    dw = guarded(prior, 4 if lddw else 0) if prior is not None else fresh(N, K, pad_cols=4 if lddw else 0)
    ws = fresh(n_slabs * N * K)
    assert call("wgnn_linear_wgrad", _ptr(g), g.stride(0), _ptr(x), x.stride(0), _ptr(dw[1]), dw[1].stride(0), M, N, K,
                1 if prior is not None else 0, _ptr(ws[1]), n_slabs) == OK
    assert intact(dw, ws)
    return dw[1]


@pytest.mark.parametrize("case", DH.WGRAD_EXACT_CASES, ids=DH.wg_id)
def test_linear_wgrad_exact(case):
    M, N, K, kind, acc, ldg, ldx, lddw = case
    L, T = wg_operands(M, N, K)
    ref = DH.linear_wgrad(L["g"], L["x"], L["prior"] if acc else None)
    assert DH.wgrad_budget(ref) < 24
    n_slabs = wgrad_slabs(M, N, K, kind)
    g, x = wide(T["g"], ldg), wide(T["x"], ldx)
    first = wgrad(g, x, T["prior"] if acc else None, M, N, K, n_slabs, lddw)
    GB.assert_exact(first, ref["dW"], f"dW (n_slabs {n_slabs})")
    assert torch.equal(first, wgrad(g, x, T["prior"] if acc else None, M, N, K, n_slabs, lddw))      # a second launch: same bits


@pytest.mark.parametrize("M,N,K", DH.WGRAD_FLOAT_CASES)
def test_linear_wgrad_float(M, N, K):
    gen = torch.Generator(device=DEV).manual_seed(DH.case_seed("fwg", M, N, K))
    g, x = torch.randn(M, N, generator=gen, device=DEV), torch.randn(M, K, generator=gen, device=DEV)
    ref = DH.linear_wgrad(g.cpu().numpy(), x.cpu().numpy())
    for kind in ("ws", 3, "over"):
        n_slabs = wgrad_slabs(M, N, K, kind)
        got = wgrad(wide(g, True), x, None, M, N, K, n_slabs, True)
        assert record_ratio("linear_wgrad", f"dW[slabs {n_slabs}]", got, ref["dW"], AB.float_bound(ref["abs_sum"], M + n_slabs)) <= 1


# ---- wgnn_agg_bwd_prepare ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def prep_operands(R, D):
    L = DH.lattice_prepare(R, D, DH.case_seed("prep", R, D))
    return L, {k: dev(L[k]) for k in ("gout", "out", "h_self", "neigh_sum", "inv_deg", "alpha")}


def prepare(T, R, D, mode, has_out, has_inv, wanted, ld):
    """One call; ``T``: device operands.  Returns {name: view} of the wanted outputs after checking every guard."""
    gout, out, h_self = wide(T["gout"], ld), wide(T["out"], ld) if has_out else None, wide(T["h_self"], ld)
    bufs = dict(g_scaled=fresh(R, D), dh_self=fresh(R, D, pad_cols=4 if ld else 0), dalpha_row=fresh(R), dself_row=fresh(R),
                dbias=fresh(D))
    p = {k: (bufs[k][1] if k in wanted else None) for k in bufs}
    nf = C.c_int64()
    assert _lib.lib().wgnn_agg_bwd_prepare_workspace(R, D, C.addressof(nf)) == OK
    assert nf.value == min(2048, max(1, -(-R // 4))) * D
    ws = fresh(int(nf.value))
    self_idx = R if mode == "genes" else R + 1
    rc = call("wgnn_agg_bwd_prepare", _ptr(gout), gout.stride(0), _ptr(out), out.stride(0) if has_out else 0,
              _ptr(T["inv_deg"]) if has_inv else None, _ptr(T["alpha"]), DH.MODE[mode], self_idx, _ptr(p["g_scaled"]),
              _ptr(h_self), h_self.stride(0), _ptr(p["dh_self"]), bufs["dh_self"][1].stride(0), _ptr(T["neigh_sum"]),
              _ptr(p["dalpha_row"]), _ptr(p["dself_row"]), _ptr(p["dbias"]), R, D, _ptr(ws[1]), int(nf.value))
    assert rc == OK
    assert intact(ws, *bufs.values())
    for k in bufs:                                             # an output that was not asked for is not written
        if k not in wanted:
            assert bool((bufs[k][1] == FILL).all()), k
    return {k: bufs[k][1] for k in wanted}


def prepare_ref(L, mode, has_out, has_inv):
    R = L["gout"].shape[0]
    return DH.bwd_prepare(L["gout"], L["out"] if has_out else None, L["inv_deg"] if has_inv else None, L["alpha"], DH.MODE[mode],
                          R if mode == "genes" else R + 1, L["h_self"], L["neigh_sum"])


@pytest.mark.parametrize("case", DH.PREPARE_EXACT_CASES, ids=DH.prep_id)
def test_agg_bwd_prepare_exact(case):
    R, D, mode, has_out, has_inv, outputs, ld = case
    L, T = prep_operands(R, D)
    ref = prepare_ref(L, mode, has_out, has_inv)
    assert max(DH.prepare_budget(ref).values()) < 24
    got = prepare(T, R, D, mode, has_out, has_inv, DH.PREP_OUTPUTS[outputs], ld)
    for k, v in got.items():
        GB.assert_exact(v, ref[k], k)


def test_agg_bwd_prepare_empty():
    """R == 0: dbias is zeros, nothing else is touched."""
    D = 260
    T = {k: torch.zeros(4, D, device=DEV) for k in ("gout", "out", "h_self", "neigh_sum")}
    T.update(inv_deg=torch.ones(4, device=DEV), alpha=torch.ones(6, device=DEV))
    got = prepare(T, 0, D, "genes", True, True, ("dbias",), False)
    assert bool((got["dbias"] == 0).all())


@pytest.mark.parametrize("R,D,mode", DH.PREPARE_FLOAT_CASES)
def test_agg_bwd_prepare_float(R, D, mode):
    gen = torch.Generator(device=DEV).manual_seed(DH.case_seed("fprep", R, D))
    T = {k: torch.randn(R, D, generator=gen, device=DEV) for k in ("gout", "out", "h_self", "neigh_sum")}
    T.update(inv_deg=torch.rand(R, generator=gen, device=DEV) * 0.95 + 0.05, alpha=torch.rand(R + 2, generator=gen, device=DEV) + 0.5)
    ref = prepare_ref({k: v.cpu().numpy() for k, v in T.items()}, mode, True, True)
    got = prepare(T, R, D, mode, True, True, DH.PREP_OUTPUTS["all"], True)
    assert record_ratio("agg_bwd_prepare", "dalpha_row", got["dalpha_row"], ref["dalpha_row"], AB.float_bound(ref["abs_dalpha_row"], D)) <= 1
    assert record_ratio("agg_bwd_prepare", "dself_row", got["dself_row"], ref["dself_row"], AB.float_bound(ref["abs_dself_row"], D)) <= 1
    assert record_ratio("agg_bwd_prepare", "dbias", got["dbias"], ref["dbias"], AB.float_bound(ref["abs_dbias"], R)) <= 1
    # elementwise outputs: at most two roundings of two or three factors (K_ROUND allows eight)
    for k in ("g_scaled", "dh_self"):
        assert record_ratio("agg_bwd_prepare", k, got[k], ref[k], AB.float_bound(np.abs(ref[k]), 0)) <= 1


# ---- wgnn_ce_sum_fwd_bwd ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ce_operands(n, Cn):
    S = DH.saturated_ce(n, Cn, DH.case_seed("ce", n, Cn))
    return S, dev(S["logits"]), dev(S["labels"], torch.int64)


def ce(logits, labels, n, Cn, want_d=True, ldd=False):
    """One call on fresh guarded buffers; returns (loss tensor [1], dlogits view | None)."""
    nf = C.c_int64()
    assert _lib.lib().wgnn_ce_sum_workspace(n, C.addressof(nf)) == OK
    ws, loss = fresh(int(nf.value)), fresh(1)
    d = fresh(n, Cn, pad_cols=2 if ldd else 0) if want_d else None
    assert call("wgnn_ce_sum_fwd_bwd", _ptr(logits), logits.stride(0), _ptr(labels), n, Cn, _ptr(loss[1]), _ptr(d and d[1]),
                d[1].stride(0) if d else 0, _ptr(ws[1]), int(nf.value)) == OK
    assert intact(ws, loss, *([d] if d else []))
    return loss[1], d and d[1]


@pytest.mark.parametrize("case", DH.CE_EXACT_CASES, ids=DH.ce_id)
def test_ce_sum_exact(case):
    n, Cn, ldx, ldd = case
    S, x, y = ce_operands(n, Cn)
    assert DH.ce_budget(S) < 24
    x = guarded(x, 3)[1] if ldx else x
    loss, d = ce(x, y, n, Cn, True, ldd)
    assert loss.item() == S["loss"]
    GB.assert_exact(d, S["dlogits"], "dlogits")
    assert torch.equal(ce(x, y, n, Cn, False)[0], loss)        # dlogits == NULL: the same loss bits


def test_ce_sum_bad_label_is_nan_in_its_row_only():
    n, Cn = 257, 5
    S, x, y = ce_operands(n, Cn)
    bad = y.clone()
    assert bad[100].item() != DH.IGNORE_INDEX
    bad[100] = Cn + 5
    loss, d = ce(x, bad, n, Cn, True, True)
    assert torch.isnan(loss).item() and torch.isnan(d[100]).all()
    keep = torch.arange(n, device=DEV) != 100
    GB.assert_exact(d[keep], S["dlogits"][keep.cpu().numpy()], "the other rows")


@pytest.mark.parametrize("n,Cn", DH.CE_FLOAT_CASES)
def test_ce_sum_float(n, Cn):
    """Unsaturated logits: the project's existing tolerance (test_cross_entropy_sum_kernel_matches_torch); the measured distance
    from fp64 is printed."""
    gen = torch.Generator(device=DEV).manual_seed(n + Cn)
    x = 3.0 * torch.randn(n, Cn, generator=gen, device=DEV)
    y = torch.randint(0, Cn, (n,), generator=gen, device=DEV)
    ref = DH.ce_sum(x.cpu().numpy(), y.cpu().numpy())
    loss, d = ce(guarded(x, 3)[1], y, n, Cn, True, True)
    e_loss = abs(loss.item() - ref["loss"])
    e_d = float(np.abs(d.cpu().numpy().astype(np.float64) - ref["dlogits"]).max())
    print(f"CE n={n} C={Cn} loss_err={e_loss:.3e} rel={e_loss / abs(ref['loss']):.3e} dlogits_max_err={e_d:.3e}")
    assert e_loss < 2e-6 * max(1.0, abs(ref["loss"])) * max(1.0, n ** 0.5 / 30)
    assert e_d <= 2e-6


# ---- error returns that launch nothing ----------------------------------------------------------------------------------------------
def test_error_returns():
    """Real, generously sized allocations behind every pointer: a missing check would compute garbage, not fault."""
    big = torch.zeros(4, 64 * 2048, device=DEV)               # inputs | outputs | second output | workspace
    half = torch.zeros(64 * 64, device=DEV, dtype=torch.float16)
    p, q, q2, wsp = (_ptr(big[i]) for i in range(4))
    off4 = _ptr(big[0, 1:])                                    # 4-byte aligned only

    def lin(x=p, dt=_lib.F32, ld_x=8, w=p, ld_w=8, out=q, rs=None, o2=None, K=8, flags=0):
        return call("wgnn_linear_fwd_ex", x, dt, ld_x, w, ld_w, None, out, 8, rs, o2, 8, 4, 8, K, flags)
    assert lin() == OK
    assert lin(K=6) == ALIGNMENT and lin(ld_x=6) == ALIGNMENT and lin(ld_w=6) == ALIGNMENT
    assert lin(ld_x=4) == BAD_ARG and lin(ld_w=4) == BAD_ARG
    assert lin(out=None) == BAD_ARG                            # both outputs NULL
    assert lin(rs=p) == BAD_ARG and lin(o2=q2) == BAD_ARG      # row_scale and out_scaled come together
    assert lin(rs=p, o2=q2) == OK and lin(rs=p, o2=q2, out=None) == OK
    assert lin(w=off4) == ALIGNMENT and lin(x=off4) == ALIGNMENT
    assert lin(x=_ptr(half[1:]), dt=_lib.F16) == ALIGNMENT and lin(x=_ptr(half[4:]), dt=_lib.F16) == OK     # f16 rows: 8 bytes
    assert lin(flags=2) == BAD_ARG

    def wg(ws=wsp, n_slabs=1, ld_dw=8, N=8, g=p):
        return call("wgnn_linear_wgrad", g, 8, p, 8, q, ld_dw, 16, N, 8, 0, ws, n_slabs)
    assert wg() == OK
    assert wg(n_slabs=0) == WORKSPACE and wg(n_slabs=-3) == WORKSPACE and wg(ws=None) == WORKSPACE
    assert wg(ld_dw=4) == BAD_ARG and wg(N=6) == ALIGNMENT and wg(g=off4) == ALIGNMENT

    def prep(D=8, neigh=p, dalpha=q, h_self=p, dself=q2, ws=wsp, ws_floats=2048 * 8, mode=2, alpha=None, ld=8):
        return call("wgnn_agg_bwd_prepare", p, ld, None, 0, None, alpha, mode, 0, None, h_self, ld, None, ld, neigh, dalpha, dself,
                    _ptr(big[1, 4096:]), 4, D, ws, ws_floats)
    assert prep() == OK
    assert prep(D=1028, ld=1028) == UNSUPPORTED and prep(D=6) == ALIGNMENT
    assert prep(neigh=None) == BAD_ARG                         # dalpha_row without neigh_sum
    assert prep(h_self=None) == BAD_ARG                        # dself_row without h_self
    assert prep(neigh=None, dalpha=None) == OK
    assert prep(mode=0) == BAD_ARG and prep(mode=3) == BAD_ARG
    assert prep(ws=None) == WORKSPACE and prep(ws_floats=7) == WORKSPACE

    lab = torch.zeros(64, device=DEV, dtype=torch.int64)

    def cee(ld=8, ld_d=8, d=q, ws=wsp, ws_floats=4, Cn=8):
        return call("wgnn_ce_sum_fwd_bwd", p, ld, _ptr(lab), 16, Cn, q2, d, ld_d, ws, ws_floats)
    assert cee() == OK
    assert cee(ld=7) == BAD_ARG and cee(ld_d=7) == BAD_ARG and cee(ld_d=0, d=None) == OK and cee(Cn=0) == BAD_ARG
    assert cee(ws=None) == WORKSPACE and cee(ws_floats=1) == WORKSPACE
    torch.cuda.synchronize()
