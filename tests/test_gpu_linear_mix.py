"""``wgnn_linear_mix_fwd`` (the fp32 MFMA GEMM with its A operand formed in the loader, include/wgnn.h) against the fp64
reference of ``linear_mix_reference.py``.

* exact group: on the dyadic lattice the kernel's outputs equal the fp64 reference BIT FOR BIT (``torch.equal``) - every M x K x N
  of the table at both forced tile heights, with / without bias and ReLU, ``out`` only / ``out_scaled`` only / both, packed
  operands and ``ld > K`` / ``ld_out > N``; fp16-stored ``x2`` on a subset.  Every output is an inner view of a NaN-filled
  tensor (guard rows above and below, guard columns when ``ld_out > N``) and the guards are checked after the call.
* float group: operands the package builds (a graph's cached feature sum, ``mix_coeffs``, random features / weights) within
  ``(K + 8) * 2^-24 * sum|terms|`` per element - K accumulations, the loader's two roundings, the bias, and slack for the
  epilogue's scale.
* ``mix_coeffs`` equals its two products bit for bit; argument refusals of the entry.
"""
import numpy as np
import pytest
import torch

import linear_mix_reference as LM
from conftest import small_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def wide(t, on):
    """``t`` as an inner view of a wider NaN-filled table (leading dimension = width + 8), or ``t`` itself."""
    if not on:
        return t
    whole = torch.full((t.shape[0] + 2, t.shape[1] + 8), float("nan"), dtype=t.dtype, device=t.device)
    whole[1:-1, 4:-4] = t
    return whole[1:-1, 4:-4]


def guarded_out(M, N, ld):
    whole = torch.full((M + 2, N + (8 if ld else 0)), float("nan"), dtype=torch.float32, device=DEV)
    return whole, (whole[1:-1, 4:-4] if ld else whole[1:-1])


def guards_intact(whole, view, ld):
    mask = torch.ones_like(whole, dtype=torch.bool)
    (mask[1:-1, 4:-4] if ld else mask[1:-1]).fill_(False)
    return bool(torch.isnan(whole[mask]).all()) and not bool(torch.isnan(view).any())


def run_case(ops, L, T, tile, M, K, N, bias, relu, outputs, ld, x2_half=False):
    x2 = T["x2"].half() if x2_half else T["x2"]
    o_whole, o = guarded_out(M, N, ld) if outputs != "scaled" else (None, None)
    s_whole, s = guarded_out(M, N, ld) if outputs != "out" else (None, None)
    res = ops.linear_mix_fwd(wide(T["x1"], ld), T["c1"], wide(x2, ld), T["c2"], wide(T["w"], ld), T["bias"] if bias else None,
                             relu=relu, row_scale=T["row_scale"] if outputs != "out" else None, want_out=outputs != "scaled",
                             tile_rows=tile, out=o, out_scaled=s)
    ref = LM.reference(L["x1"], L["c1"], L["x2"], L["c2"], L["w"], L["bias"] if bias else None, relu, L["row_scale"])
    if outputs != "scaled":
        got = res if outputs == "out" else res[0]
        assert got.data_ptr() == o.data_ptr() and guards_intact(o_whole, o, ld)
        assert torch.equal(got, dev32(ref["out"])) and LM.same_bits(got.cpu().numpy(), ref["out"])
    if outputs != "out":
        assert res[1].data_ptr() == s.data_ptr() and guards_intact(s_whole, s, ld)
        assert torch.equal(res[1], dev32(ref["out_scaled"])) and LM.same_bits(res[1].cpu().numpy(), ref["out_scaled"])
        if outputs == "scaled":
            assert res[0] is None


@pytest.mark.parametrize("tile,M", [(t, m) for t in LM.MIX_TILES for m in LM.MIX_M])
def test_exact_on_the_lattice(tile, M):
    from scdeepsort_amd import ops
    rows = [c for c in LM.EXACT_CASES if c[0] == tile and c[1] == M]
    assert len(rows) == len(LM.MIX_K) * len(LM.MIX_N)
    for (_, _, K, N, bias, relu, outputs, ld) in rows:
        L = LM.lattice(M, K, N, LM.case_seed("mix", M, K, N))
        T = {k: dev32(v) for k, v in L.items()}
        run_case(ops, L, T, tile, M, K, N, bias, relu, outputs, ld)
        if N in (1, 129) or K == 20:                                   # the __half loader of x2 on a subset
            run_case(ops, L, T, tile, M, K, N, bias, relu, outputs, ld, x2_half=True)


def test_automatic_tile_height_and_many_row_tiles():
    """No forced tile height (the entry picks 64 or 128 rows by how the tiles fill the chip), more row tiles than one round of
    workgroups would need at small sizes, ragged in M, N and K."""
    from scdeepsort_amd import ops
    M, K, N = 1031, 20, 129
    L = LM.lattice(M, K, N, LM.case_seed("mix", M, K, N))
    T = {k: dev32(v) for k, v in L.items()}
    run_case(ops, L, T, None, M, K, N, True, True, "both", True)


def test_float_operands_built_by_the_package_stay_in_the_bound():
    import scdeepsort_amd as sda
    from scdeepsort_amd import ops
    case = small_case(cells=300, genes=200, dim=64, seed=5)
    g = sda.CellGeneGraph.from_expression(case["expr"], case["support_mask"], device=DEV)
    G, K = case["G"], case["dim"]
    feats = torch.from_numpy(case["feats"]).to(DEV)
    h_g, h_c = feats[:G], feats[G:]
    S = g.feature_sum(h_c)
    assert S.shape == (G, K) and S.dtype == torch.float32
    alpha = torch.from_numpy(np.random.default_rng(6).uniform(0.5, 1.5, G + 2).astype(np.float32)).to(DEV)
    c1, c2 = ops.mix_coeffs(alpha, G, g.gc.inv_deg)
    assert torch.equal(c1, alpha[:G] * g.gc.inv_deg) and torch.equal(c2, alpha[G] * g.gc.inv_deg)
    rng = np.random.default_rng(7)
    for N in (16, 256):
        W, b = dev32(rng.standard_normal((N, K)) / np.sqrt(K)), dev32(rng.standard_normal(N))
        out, scaled = ops.linear_mix_fwd(S, c1, h_g, c2, W, b, relu=False, row_scale=alpha[:G])
        ref = LM.reference(*(t.double().cpu().numpy() for t in (S, c1, h_g, c2, W, b)), relu=False,
                           row_scale=alpha[:G].double().cpu().numpy())
        bound = (K + 8) * 2.0 ** -24 * ref["abs_sum"]
        err = np.abs(out.double().cpu().numpy() - ref["out"])
        err_s = np.abs(scaled.double().cpu().numpy() - ref["out_scaled"])
        print(f"N={N}: worst |err| / bound = {float((err / bound).max()):.4f} (out), "
              f"{float((err_s / (alpha[:G].double().cpu().numpy()[:, None] * bound)).max()):.4f} (scaled)")
        assert (err <= bound).all() and err.max() > 0
        assert (err_s <= alpha[:G].double().cpu().numpy()[:, None] * bound).all()
        relu_out = ops.linear_mix_fwd(S, c1, h_g, c2, W, b, relu=True)
        assert torch.equal(relu_out, torch.relu(out))


def test_refusals():
    from scdeepsort_amd import ops
    from scdeepsort_amd._lib import WgnnError
    x = torch.zeros(8, 8, device=DEV)
    c = torch.ones(8, device=DEV)
    w = torch.zeros(4, 8, device=DEV)
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x, c, x[:, :4], c, w)                      # x1 and x2 disagree
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x, c[:4], x, c, w)                         # a coefficient per row
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x, c, x, c, w, want_out=False)             # no output left
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x[:, :6], c, x[:, :6], c, w[:, :6])        # K % 4
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x, c, x, c, w, out=torch.zeros(8, 3, device=DEV))      # an output table narrower than N
    with pytest.raises(WgnnError):
        ops.linear_mix_fwd(x.cpu(), c, x, c, w)                       # no CPU fallback
    assert ops.linear_mix_fwd(x[:0], c[:0], x[:0], c[:0], w).shape == (0, 4)
