"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical inputs.
Tolerance: 1e-4 absolute on O(1) fp32 values (BASELINE.json north_star); index/plan work is exact."""
import json

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from conftest import GOLDEN, load_golden, small_case
from oracle import wgnn_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"


def dev(x, dtype=torch.float32):
    return torch.as_tensor(x, dtype=dtype, device=DEV)


def make_model(sd, dim, hidden, n_classes, n_layers, G, order="auto"):
    m = sda.GNN(dim, hidden, n_classes, n_layers, G, activation=F.relu).to(DEV)
    m.load_state_dict(sd)
    m.order = order
    return m.eval()


def test_library_loaded_and_gpu_present():
    assert torch.cuda.is_available()
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    from scdeepsort_amd import _lib
    assert _lib.lib().wgnn_version() >= _lib.ABI_MIN and _lib.lib().wgnn_version() // 100 == _lib.ABI_MAJOR


def test_kat_2x2_on_gpu():
    kat = json.loads((GOLDEN / "kat_2x2.json").read_text())
    expr = sp.csr_matrix(np.array(kat["expr_rows"], dtype=np.float32))
    g = sda.CellGeneGraph.from_expression(expr, device=DEV)
    # K4 normalisation, hand-derived values
    np.testing.assert_allclose(g.cg.val.cpu().numpy(), [0.5, 1.5, 1.0], rtol=1e-6)         # into c0: g0,g1 ; into c1: g0
    np.testing.assert_allclose(g.gc.val.cpu().numpy(), [2 / 3, 4 / 3, 1.0], rtol=1e-6)     # into g0: c0,c1 ; into g1: c0
    np.testing.assert_allclose(g.cg.inv_deg.cpu().numpy(), [1 / 3, 1 / 2], rtol=1e-6)
    alpha = dev(kat["alpha"])
    x = torch.zeros(4, 4, device=DEV); x[:, 0] = dev(kat["features"])                       # D padded to 4
    zc = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, 3, x[:2], x[2:])
    zg = sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, 2, x[2:], x[:2])
    got = torch.cat([zg[:, 0], zc[:, 0]]).cpu().numpy()
    np.testing.assert_allclose(got, [kat["neigh"][k] for k in ("g0", "g1", "c0", "c1")], rtol=1e-6)
    assert torch.all(zc[:, 1:] == 0)


@pytest.mark.parametrize("D", [4, 8, 24, 32, 64, 100, 128, 256, 400, 1024])
@pytest.mark.parametrize("mode", ["cells", "genes"])
def test_aggregate_widths_and_modes(D, mode):
    c = small_case(cells=200, genes=150, dim=D, seed=D, density=0.3)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV, chunk=32)   # forces long-row splitting
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]
    alpha = np.random.default_rng(1).uniform(0.5, 1.5, G + 2).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    if mode == "cells":
        out = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc))
        np.testing.assert_allclose(out.cpu().numpy(), zc, atol=TOL)
        assert g.cg.plan.n_long > 0
    else:
        out = sda.agg_fwd(g.gc, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg))
        np.testing.assert_allclose(out.cpu().numpy(), zg, atol=TOL)


def test_fused_bias_relu_and_flags():
    c = small_case(seed=11, dim=32)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(2)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32); bias = rng.standard_normal(32).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, _ = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    out = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), bias=dev(bias), relu=True)
    np.testing.assert_allclose(out.cpu().numpy(), np.maximum(zc + bias, 0), atol=TOL)
    # NO_ALPHA + NO_MEAN + no self = plain A @ H (multi-GPU partial sums; cell-feature build)
    raw = sda.agg_fwd(g.cg, None, sda.NO_ALPHA, 0, dev(Hg), None, no_mean=True)
    np.testing.assert_allclose(raw.cpu().numpy(), cg.A_cg.astype(np.float64) @ Hg.astype(np.float64), atol=2e-4, rtol=1e-5)


def test_seed_subset_and_order():
    """row_ids = the seed list of a NodeFlow batch: arbitrary order, repeats allowed (predict.py:75-76)."""
    c = small_case(seed=12, dim=64)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV, chunk=16)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; alpha = np.random.default_rng(3).uniform(0.5, 1.5, G + 2).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, _ = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    ids = torch.tensor([5, 3, 90, 3, 0, 95], device=DEV)
    out = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), row_ids=ids)
    np.testing.assert_allclose(out.cpu().numpy(), zc[ids.cpu().numpy()], atol=TOL)
    out2 = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc)[ids], row_ids=ids, self_compact=True)
    assert torch.equal(out, out2)
    empty = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), row_ids=ids[:0])
    assert empty.shape == (0, 64)


def test_fp16_feature_storage_fp32_accumulate():
    c = small_case(seed=13, dim=128)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; alpha = np.random.default_rng(4).uniform(0.5, 1.5, G + 2).astype(np.float32)
    f16 = c["feats"].astype(np.float16)
    zc, _ = O.csr_aggregate(cg, alpha, f16[:G].astype(np.float64), f16[G:].astype(np.float64))   # same rounded inputs
    out = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(f16[:G], torch.float16), dev(f16[G:], torch.float16),
                      out_dtype=torch.float32)
    np.testing.assert_allclose(out.cpu().numpy(), zc, atol=TOL)
    out16 = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(f16[:G], torch.float16), dev(f16[G:], torch.float16))
    assert out16.dtype == torch.float16
    np.testing.assert_allclose(out16.float().cpu().numpy(), zc, atol=2e-3)


@pytest.mark.parametrize("name", ["testis199", "pancreas11"])
@pytest.mark.parametrize("order", ["project_first", "aggregate_first"])
def test_golden_forward(name, order):
    c = load_golden(name)
    z = c["z"]
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(c["sd"], int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), c["n_layers"], c["G"], order)
    with torch.no_grad():
        logits = m(g, dev(c["feats"])).cpu().numpy()
        emb = m.embed(g, dev(c["feats"])).cpu().numpy()
    np.testing.assert_allclose(logits, z["logits_f64"], atol=TOL)
    np.testing.assert_allclose(logits, z["logits_f32"], atol=TOL)
    np.testing.assert_allclose(emb, z["hidden_last_f32"], atol=TOL)


def test_forward_seeds_match_nodeflow_batches():
    c = small_case(seed=14)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=5)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, c["dim"], c["hidden"], c["n_classes"], 2, c["G"])
    rng = np.random.default_rng(1)
    seeds = rng.permutation(np.arange(c["G"], c["G"] + c["C"]))[:40]
    want = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), seeds, 2).numpy()
    with torch.no_grad():
        got = m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(got, want, atol=TOL)


@pytest.mark.parametrize("save_sum", [True, False])
@pytest.mark.parametrize("n_layers,order", [(1, "auto"), (2, "project_first"), (2, "aggregate_first")])
def test_training_gradients_match_autograd_oracle(n_layers, order, save_sum, monkeypatch):
    """loss = CE_sum on a seed batch; grads of every parameter incl. alpha (train.py:34-36,80-84).  `save_sum`: the gene
    rows' alpha gradient from the neighbour sums saved by the forward (default) or from a K3 pass over the edges."""
    from scdeepsort_amd import ops
    monkeypatch.setattr(ops, "SAVE_NEIGH_SUM", save_sum)
    c = small_case(cells=80, genes=48, dim=16, hidden=12, n_classes=4, seed=15, test_cells=0)
    sd = O.init_params(16, 12, 4, n_layers, 48, seed=6)
    rg = O.build_reference_graph(c["expr"])
    seeds = np.array([48 + i for i in (0, 5, 9, 33, 70, 3)])        # includes the empty cell (row 3)
    labels = torch.tensor([0, 1, 2, 3, 1, 0])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, n_layers)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV, chunk=8)
    m = make_model(sd, 16, 12, 4, n_layers, 48, order)
    logits = m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds).to(DEV))
    l = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
    l.backward()
    assert l.item() == pytest.approx(float(loss), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=k)


def test_golden_gradients():
    c = load_golden("testis199"); z = c["z"]
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(c["sd"], int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), c["n_layers"], c["G"])
    logits = m(g, dev(c["feats"]), seeds=torch.from_numpy(z["seeds"]).to(DEV))
    l = F.cross_entropy(logits, torch.from_numpy(z["labels"]).to(DEV), reduction="sum")
    l.backward()
    assert l.item() == pytest.approx(float(z["loss"]), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), c["grads"][k], atol=2e-4, rtol=1e-3, err_msg=k)


def test_normalize_rows_matches_reference_formula():
    rng = np.random.default_rng(7)
    nnz = np.array([0, 1, 5, 64, 65, 1000, 3])
    rowptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int32)
    raw = rng.uniform(0.5, 7.0, rowptr[-1]).astype(np.float32)
    from scdeepsort_amd.graph import _normalize_on_device
    val, inv = _normalize_on_device(dev(rowptr, torch.int32), dev(raw))
    want = np.empty_like(raw)
    for r in range(len(nnz)):
        seg = raw[rowptr[r]:rowptr[r + 1]]
        if len(seg):
            want[rowptr[r]:rowptr[r + 1]] = (np.float32(len(seg)) * seg) / np.float32(seg.astype(np.float64).sum())
    np.testing.assert_allclose(val.cpu().numpy(), want, rtol=2e-6)
    np.testing.assert_allclose(inv.cpu().numpy(), 1.0 / (nnz + 1), rtol=1e-7)


def test_full_size_properties_cfg2():
    """At BASELINE cfg2 size: oracle parity on a row sample + size-independent properties
    (linearity in h, seed-subset == full, determinism)."""
    from scdeepsort_amd import synthetic as S
    cfg = S.CONFIGS["cfg2"]
    rp, col, val = S.synth_expression(cfg.cells, cfg.genes, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, cfg.genes)
    G, C = cfg.genes, cfg.cells
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    h1 = S.synth_features(G + C, cfg.hidden, device=DEV); h2 = S.synth_features(G + C, cfg.hidden, seed=5, device=DEV)
    f = lambda h: sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, h[:G], h[G:])
    fg = lambda h: sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, G, h[G:], h[:G])
    z1, z2, z3 = f(h1), f(h2), f(2 * h1 - 0.5 * h2)
    assert (2 * z1 - 0.5 * z2 - z3).abs().max().item() < 1e-4
    y1, y2, y3 = fg(h1), fg(h2), fg(2 * h1 - 0.5 * h2)
    assert (2 * y1 - 0.5 * y2 - y3).abs().max().item() < 1e-4
    assert torch.equal(z1, f(h1)) and torch.equal(y1, fg(h1))                    # deterministic (no atomics)
    ids = torch.randperm(C, device=DEV)[:777]
    sub = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, h1[:G], h1[G:], row_ids=ids)
    # since round 4 a cfg2-size full pass runs LDS-streamed (ops.TILED_MIN_WORK): the seeds' rows (row-wave kernel) agree with
    # it to rounding, and bit for bit with the row-wave kernel's own full pass
    from scdeepsort_amd import ops
    assert ops.tiled_kernel_serves(g.cg, cfg.hidden)
    assert (sub - z1[ids]).abs().max().item() < 1e-5
    saved, ops.TILED_MIN_WORK = ops.TILED_MIN_WORK, None
    try:
        assert torch.equal(sub, f(h1)[ids])
    finally:
        ops.TILED_MIN_WORK = saved
    # oracle on the same graph (CPU, seconds at this size)
    expr = S.to_scipy(rp, col, val, G)
    cg = O.build_csr_graph(expr)
    zc, zg = O.csr_aggregate(cg, alpha.cpu().numpy(), h1[:G].cpu().numpy().astype(np.float64), h1[G:].cpu().numpy().astype(np.float64))
    np.testing.assert_allclose(z1.cpu().numpy(), zc, atol=TOL)
    np.testing.assert_allclose(y1.cpu().numpy(), zg, atol=TOL)
    np.testing.assert_allclose(g.cg.val.cpu().numpy(), cg.A_cg.data, rtol=3e-6)
    np.testing.assert_allclose(g.gc.val.cpu().numpy(), cg.A_gc.data, rtol=3e-6)


def test_full_size_properties_cfg3():
    """At BASELINE cfg3 size (the bench workload, LDS-streamed kernel): size-independent properties -
    linearity in h, determinism, a row sample against the row-wave kernel, and a "checksum of checksums":
    with h = 1 every output element must equal (sum_j w_j*alpha[k_j] + alpha_self) / (deg+1), computed here with
    plain torch scatter-adds over the CSR."""
    from scdeepsort_amd import ops, synthetic as S
    cfg = S.CONFIGS["cfg3"]
    G, C, H = cfg.genes, cfg.cells, cfg.hidden
    rp, col, val = S.synth_expression(C, G, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    del rp, col, val
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg1, hc1 = S.synth_features(G, H, device=DEV), S.synth_features(C, H, seed=3, device=DEV)
    hg2, hc2 = S.synth_features(G, H, seed=5, device=DEV), S.synth_features(C, H, seed=6, device=DEV)
    ops.PROFILE = []
    f = lambda a, b: sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, a, b)
    fg = lambda a, b: sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, G, b, a)
    z1, z2, z3 = f(hg1, hc1), f(hg2, hc2), f(2 * hg1 - 0.5 * hg2, 2 * hc1 - 0.5 * hc2)
    y1, y2, y3 = fg(hg1, hc1), fg(hg2, hc2), fg(2 * hg1 - 0.5 * hg2, 2 * hc1 - 0.5 * hc2)
    kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
    ops.PROFILE = None
    assert kernels == {"agg_tiled_flat4"}
    assert (2 * z1 - 0.5 * z2 - z3).abs().max().item() < 1e-4
    assert (2 * y1 - 0.5 * y2 - y3).abs().max().item() < 1e-4
    assert torch.equal(z1, f(hg1, hc1)) and torch.equal(y1, fg(hg1, hc1))          # deterministic (no atomics)
    ids = torch.randperm(C, device=DEV)[:1000]
    sub = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg1, hc1, row_ids=ids)    # row-wave kernel (K1)
    assert (sub - z1[ids]).abs().max().item() < 1e-4
    gids = torch.randperm(G, device=DEV)[:1000]
    subg = sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, G, hc1, hg1, row_ids=gids)
    assert (subg - y1[gids]).abs().max().item() < 1e-4
    # independent formulation at full size: torch's CSR SpMM (hipSPARSE) + elementwise epilogue, fp32
    A_cg = torch.sparse_csr_tensor(g.cg.rowptr.long(), g.cg.col.long(), g.cg.val, size=(C, G))
    ref_c = (torch.sparse.mm(A_cg, alpha[:G, None] * hg1) + alpha[G + 1] * hc1) * g.cg.inv_deg[:, None]
    assert (ref_c - z1).abs().max().item() < 1e-4
    A_gc = torch.sparse_csr_tensor(g.gc.rowptr.long(), g.gc.col.long(), g.gc.val, size=(G, C))
    ref_g = (alpha[:G, None] * torch.sparse.mm(A_gc, hc1) + alpha[G] * hg1) * g.gc.inv_deg[:, None]
    assert (ref_g - y1).abs().max().item() < 1e-4
    del A_cg, A_gc, ref_c, ref_g
    # checksum: constant features
    ones_g, ones_c = torch.ones(G, H, device=DEV), torch.ones(C, H, device=DEV)
    zc, zg = f(ones_g, ones_c), fg(ones_g, ones_c)
    a64 = alpha.double()
    row_c = torch.repeat_interleave(torch.arange(C, device=DEV), (g.cg.rowptr[1:] - g.cg.rowptr[:-1]).long())
    want_c = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, row_c, g.cg.val.double() * a64[g.cg.col.long()])
    want_c = (want_c + a64[G + 1]) * g.cg.inv_deg.double()
    row_g = torch.repeat_interleave(torch.arange(G, device=DEV), (g.gc.rowptr[1:] - g.gc.rowptr[:-1]).long())
    want_g = torch.zeros(G, dtype=torch.float64, device=DEV).index_add_(0, row_g, g.gc.val.double())
    want_g = (a64[:G] * want_g + a64[G]) * g.gc.inv_deg.double()
    assert (zc.double() - want_c[:, None]).abs().max().item() < 1e-4
    assert (zg.double() - want_g[:, None]).abs().max().item() < 1e-4
    # the normalisation itself: every non-empty row's weights sum to its in-degree (preprocess_internal.py:17-23)
    deg_c = (g.cg.rowptr[1:] - g.cg.rowptr[:-1]).double()
    sum_c = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, row_c, g.cg.val.double())
    assert (sum_c - deg_c).abs().max().item() < 1e-2 and ((sum_c - deg_c).abs() / deg_c.clamp(min=1)).max().item() < 1e-5


# ---- LDS-streamed (tiled) kernel: same outputs as the oracle, every geometry -------------------
@pytest.mark.parametrize("D", [4, 64, 128, 200, 252, 256])
@pytest.mark.parametrize("geom", [(None, 1), (3, 1), (2, 4), (5, 7)])
@pytest.mark.parametrize("direction", ["cells", "genes"])
@pytest.mark.parametrize("kb", [64, 78])
def test_tiled_kernel_matches_oracle(D, geom, direction, kb):
    """The hand-scheduled tile kernel (agg_tiled_flat4) at every width it serves natively: D = 256 and narrower rows
    (reference default hidden_dim = 200, train.py:137; D/4 lanes in the DMA, 1 KiB LDS slots), all tile geometries."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops
    c = small_case(cells=700, genes=333, dim=D, seed=D + 7, density=0.25, test_cells=50)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(5)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32); bias = rng.standard_normal(D).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    if direction == "cells":
        tp = build_tile_plan(g.cg, *geom, block_rows=kb)
        out = ops.agg_fwd_tiled(g.cg, tp, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), bias=dev(bias), relu=True)
        want = np.maximum(zc + bias, 0)
    else:
        tp = build_tile_plan(g.gc, *geom, block_rows=kb)
        out = ops.agg_fwd_tiled(g.gc, tp, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg), bias=dev(bias), relu=True)
        want = np.maximum(zg + bias, 0)
    assert tp.n_col_splits == geom[1]
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)


@pytest.mark.parametrize("kb", [16, 17, 19, 23, 31])
@pytest.mark.parametrize("direction", ["cells", "genes"])
def test_flat_kernel_many_blocks(kb, direction):
    """D = 256 with short LDS blocks: 40-125 source blocks per tile, so the six-block steady-state loop of
    agg_tiled_flat4 and every tail length (blocks mod 6) run; chunks longer than 64 entries (hub genes) too."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops
    c = small_case(cells=1500, genes=700, dim=256, seed=kb, density=0.12, test_cells=30)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(kb)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    ops.PROFILE = []
    if direction == "cells":
        tp = build_tile_plan(g.cg, 6, 1, block_rows=kb)
        out = ops.agg_fwd_tiled(g.cg, tp, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc))
        want = zc
    else:
        tp = build_tile_plan(g.gc, 3, 2, block_rows=kb)
        out = ops.agg_fwd_tiled(g.gc, tp, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg))
        want = zg
    kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
    ops.PROFILE = None
    assert kernels == {"agg_tiled_flat4"}
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)


@pytest.mark.parametrize("D", [64, 200, 256])
def test_generic_tile_kernel_still_matches(D):
    """agg_tiled (compiler-scheduled, kept for A/B timing behind debug flag bit 19) against the flat kernel: same bits
    are not required (different summation order), same result to 1e-4 is."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops
    c = small_case(cells=500, genes=260, dim=D, seed=D, density=0.2, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    G = c["G"]
    alpha = dev(np.random.default_rng(1).uniform(0.5, 1.5, G + 2).astype(np.float32))
    Hg, Hc = dev(c["feats"][:G]), dev(c["feats"][G:])
    tp = build_tile_plan(g.cg, 3, 2, block_rows=64)
    flat = ops.agg_fwd_tiled(g.cg, tp, alpha, sda.SRC_IS_GENE, G + 1, Hg, Hc)
    ops.DEBUG_FLAGS = 1 << 19
    try:
        gen = ops.agg_fwd_tiled(g.cg, tp, alpha, sda.SRC_IS_GENE, G + 1, Hg, Hc)
    finally:
        ops.DEBUG_FLAGS = 0
    np.testing.assert_allclose(gen.cpu().numpy(), flat.cpu().numpy(), atol=2e-5)


def test_tiled_plan_covers_every_edge_once():
    from scdeepsort_amd.graph import build_tile_plan
    c = small_case(cells=600, genes=300, seed=3, density=0.2)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    for csr, geom in ((g.cg, (4, 1)), (g.gc, (3, 5))):
        tp = build_tile_plan(csr, *geom)
        from scdeepsort_amd.graph import TILE_PAD_FLAG
        real = (tp.entries[:, 0] & TILE_PAD_FLAG) == 0               # zero-weight fillers keep shared pairs at even offsets
        assert int(real.sum()) == csr.nnz and (tp.entries[~real, 1] == 0).all()
        seg = tp.seg_ptr.cpu().numpy()
        assert seg[0] == 0 and seg[-1] == tp.entries.shape[0] and (np.diff(seg) >= 0).all()
        # weights multiset preserved (bit-exact), every row appears in exactly one (row-)tile per column split
        assert torch.equal(torch.sort(tp.entries[real, 1]).values, torch.sort(csr.val.view(torch.int32)).values)
        # tiles of one column split share a source range (tile_hdr); their launch order is XCD-aware (graph._flat_tile_index)
        begins = tp.hdr[:, 0].cpu().numpy()
        split_of = np.searchsorted(np.unique(begins), begins)
        assert len(np.unique(begins)) == geom[1] and (np.bincount(split_of) == tp.n_row_tiles).all()
        all_slots = tp.items[:, :, 0].cpu().numpy()
        first = None
        for k in range(geom[1]):
            s = all_slots[split_of == k].reshape(-1); s = s[s >= 0]
            # every row at least once per column split; hub rows several times (virtual rows, see build_tile_plan)
            assert sorted(set(s.tolist())) == list(range(csr.n_rows))
            first = np.bincount(s, minlength=csr.n_rows) if first is None else first
            assert np.array_equal(np.bincount(s, minlength=csr.n_rows), first)
        # partial-sum slots: a permutation of 0..n_partials-1 over all items that have one
        ps = tp.items[:, :, 3].reshape(-1); ps = ps[ps >= 0].cpu().numpy()
        assert sorted(ps.tolist()) == list(range(tp.n_partials))


def test_tiled_dispatch_is_used_for_large_passes_and_matches_rowwave():
    from scdeepsort_amd import ops, synthetic as S
    rp, col, val = S.synth_expression(30000, 3000, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, 3000)
    alpha = torch.rand(3002, device=DEV) + 0.5
    hg = S.synth_features(3000, 256, device=DEV); hc = S.synth_features(30000, 256, seed=9, device=DEV)
    old = ops.TILED_MIN_WORK
    try:
        ops.TILED_MIN_WORK = None
        a1 = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, 3001, hg, hc); b1 = sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, 3000, hc, hg)
        ops.TILED_MIN_WORK = 1
        a2 = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, 3001, hg, hc); b2 = sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, 3000, hc, hg)
    finally:
        ops.TILED_MIN_WORK = old
    assert g.cg._tile_plan is not None and g.gc._tile_plan is not None
    assert (a1 - a2).abs().max().item() < 2e-5 and (b1 - b2).abs().max().item() < 2e-5


def test_simulated_two_shards_match_unsharded():
    """Cell-axis sharding with the HIP operators: two shards on one GPU, partial gene sums added by hand
    where RCCL would all-reduce them, must equal the unsharded forward."""
    from scdeepsort_amd import synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    from scdeepsort_amd.dist import shard_range
    G, C, Din, H = 300, 1000, 40, 32
    rp, col, val = S.synth_expression(C, G, 0.08, device=DEV)
    torch.manual_seed(0)
    m = sda.GNN(Din, H, 5, 2, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, Din, device=DEV)
    full = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    with torch.no_grad():
        want = m(full, feats)
        shards = []
        for r in range(2):
            lo, hi = shard_range(C, r, 2)
            b, e = int(rp[lo]), int(rp[hi])
            shards.append((lo, hi, (rp[lo:hi + 1] - rp[lo]).clone(), col[b:e].clone(), val[b:e].clone()))
        stats = [ShardedWgnn.gene_stats(c_, v_, G) for _, _, _, c_, v_ in shards]
        g_deg, g_sum = stats[0][0] + stats[1][0], stats[0][1] + stats[1][1]
        eng = [ShardedWgnn.build(m, r_, c_, v_, G, global_stats=(g_deg, g_sum)) for _, _, r_, c_, v_ in shards]
        assert all(e.world == 2 for e in eng)
        # the cells<-genes pass that runs next to the in-flight all-reduce leaves the communicator its CUs (one-round tile
        # geometry within 256 - COMM_CUS, only inside LocalOps.overlapped()); everything else keeps the whole chip
        assert all(e.overlap_cu_budget == 224 and e.graph.cg.cu_budget == 256 and e.graph.gc.cu_budget == 256 for e in eng)
        with eng[0]._ops().overlapped():
            assert eng[0].graph.cg.cu_budget == 224 and eng[0].graph.cg.tile_plan(78).n_tiles <= 224
        assert eng[0].graph.cg.cu_budget == 256
        W1, b1 = m.layers[0].fc_neigh.weight, m.layers[0].fc_neigh.bias
        W2, b2 = m.layers[1].fc_neigh.weight, m.layers[1].fc_neigh.bias
        h_g = feats[:G]
        p_g = F.linear(h_g, W1)
        p_c = [F.linear(feats[G + lo:G + hi], W1) for lo, hi, *_ in shards]
        new_c = [e._ops().cells_layer(p_g, pc, b1, True) for e, pc in zip(eng, p_c)]
        total = sum(e._ops().genes_partial(pc) for e, pc in zip(eng, p_c))          # <- the all-reduce
        h_g1 = eng[0]._ops().genes_finish(total, p_g, b1, True)
        p_g2 = F.linear(h_g1, W2)
        out = [e._ops().cells_layer(p_g2, F.linear(nc, W2), b2, True) for e, nc in zip(eng, new_c)]
        got = torch.cat([m.linear(o) for o in out])
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=2e-5)
    # world == 1 engine is the plain model
    e1 = ShardedWgnn.build(m, rp, col, val, G)
    assert e1.overlap_cu_budget == 256 and e1._ops().overlapped is None
    with torch.no_grad():
        assert torch.equal(e1.forward(feats[:G], feats[G:]), want)


def test_budgeted_tile_geometry_matches_full_chip_geometry():
    """The N = 8 shard of the cfg3 job (12 500 cells x 20 000 genes): the cells<-genes pass on the geometry that leaves 32 CUs
    to the communicator (dist.COMM_CUS, AggCsr.cu_budget) against the full-chip geometry and against the row-wave kernel."""
    from scdeepsort_amd import synthetic as S, ops
    G, C, D = 20_000, 12_500, 256
    rp, col, val = S.synth_expression(C, G, 0.04, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg = S.synth_features(G, D, device=DEV); hc = S.synth_features(C, D, seed=3, device=DEV)
    kb = ops.tiled_block_rows(D)
    full = g.cg.tile_plan(kb)
    g.cg.cu_budget = 224
    lean = g.cg.tile_plan(kb)
    assert 224 < full.n_tiles <= 256 and lean.n_tiles <= 224 and lean is not full
    a = ops.agg_fwd_tiled(g.cg, full, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
    b = ops.agg_fwd_tiled(g.cg, lean, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
    saved, ops.TILED_MIN_WORK = ops.TILED_MIN_WORK, None
    try:
        ref = ops.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
    finally:
        ops.TILED_MIN_WORK = saved
    assert float((a - b).abs().max()) < 2e-6 and float((b - ref).abs().max()) < 2e-5


def test_cell_features_through_k1():
    """cell_feat = rownorm(X) . gene_feat (preprocess_internal.py:197-199) as a NO_ALPHA aggregation."""
    c = small_case(cells=150, genes=90, dim=8, seed=4, density=0.3)
    expr = c["expr"]
    gf = np.random.default_rng(2).standard_normal((90, 50)).astype(np.float32)        # width 50: not a multiple of 4
    dense = expr.toarray().astype(np.float64)
    want = (dense / (dense.sum(1, keepdims=True) + 1e-6)) @ gf.astype(np.float64)
    got = sda.CellGeneGraph.cell_features(dev(expr.indptr, torch.int64), dev(expr.indices, torch.int32), dev(expr.data), dev(gf))
    assert got.shape == (150, 50)
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=1e-5)
    assert np.all(got.cpu().numpy()[3] == 0)                                           # the empty cell


def test_sharded_train_step_world1_matches_plain_autograd():
    """ShardedWgnn.train_step (cfg4 path: differentiable partial sums, CE-sum, grad all-reduce) at world size 1,
    forced through the sharded code path, gives the same loss and gradients as GNN.forward + autograd."""
    from scdeepsort_amd import synthetic as S, dist as D
    from scdeepsort_amd.sharded import ShardedWgnn
    G, C, Din, H = 200, 600, 24, 16
    rp, col, val = S.synth_expression(C, G, 0.1, device=DEV)
    torch.manual_seed(1)
    m = sda.GNN(Din, H, 4, 2, G, activation=F.relu).to(DEV)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, Din, device=DEV)
    labels = torch.arange(C, device=DEV) % 4
    full = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    loss_ref = F.cross_entropy(m(full, feats), labels, reduction="sum")
    loss_ref.backward()
    ref = {k: p.grad.clone() for k, p in m.named_parameters()}
    eng = ShardedWgnn.build(m, rp, col, val, G, global_stats=ShardedWgnn.gene_stats(col, val, G))   # 1 shard, sharded code path
    assert eng.world == 2
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    total = eng.train_step(feats[:G], feats[G:], labels, opt)
    assert total == pytest.approx(float(loss_ref.detach()), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref[k].cpu().numpy(), atol=2e-4, rtol=1e-3, err_msg=k)


def test_tiled_backward_kernels_match_rowwave():
    """K2t / K3t (LDS-streamed) == K2 / K3 (row-wave) on the same inputs, both alpha modes, incl. dalpha.
    The row-wave kernels themselves are pinned to fp64 in tests/test_gpu_backward_ops.py."""
    from scdeepsort_amd import ops, synthetic as S
    G, C, D = 500, 3000, 256
    rp, col, val = S.synth_expression(C, G, 0.1, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg = S.synth_features(G, D, device=DEV); hc = S.synth_features(C, D, seed=9, device=DEV)
    gc_ = S.synth_features(C, D, seed=11, device=DEV); gg_ = S.synth_features(G, D, seed=12, device=DEV)
    old = ops.TILED_MIN_WORK
    res = {}
    try:
        for name, thr in (("row", None), ("tiled", 1)):
            ops.TILED_MIN_WORK = thr
            da = torch.zeros(G + 2, device=DEV)
            dh1 = sda.agg_bwd_src(g.cg, alpha, sda.SRC_IS_GENE, gc_, hg, da)          # cells<-genes: dH_g, dalpha[genes]
            dh2 = sda.agg_bwd_src(g.gc, alpha, sda.DST_IS_GENE, gg_, None)            # genes<-cells: dH_c
            dr, ds = sda.agg_bwd_alpha(g.gc, gg_, hc, hg)                             # dalpha (cell->gene) + gene self-loop
            res[name] = (dh1, da.clone(), dh2, dr, ds)
    finally:
        ops.TILED_MIN_WORK = old
    for a, b, tol in zip(res["row"], res["tiled"], (2e-5, 2e-3, 2e-5, 2e-4, 2e-4)):
        assert (a - b).abs().max().item() <= tol * max(1.0, a.abs().max().item())


# ------------------------------------------------------------------------------------------------
# neighbour-subsampled NodeFlows (train.py:37-40, num_neighbors > 0)
def _picker_from(nf, G):
    """{(block, parent id): drawn source parent ids} from a product NodeFlow, for the oracle to replay."""
    table = {}
    for b, (cb, gb) in enumerate(nf.blocks):
        for blk, is_cell in ((cb, True), (gb, False)):
            if blk is None:
                continue
            rows = blk.rows.cpu().numpy()
            rp = blk.csr.rowptr.cpu().numpy()
            col = blk.csr.col.cpu().numpy().astype(np.int64)
            sd = blk.self_drawn.cpu().numpy()
            for j, r in enumerate(rows):
                me = int(r) + (G if is_cell else 0)
                src = col[rp[j]:rp[j + 1]] + (0 if is_cell else G)
                table[(b, me)] = np.concatenate([src, [me]]) if sd[j] > 0 else src
    return lambda block, v: table[(block, v)]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_sampled_nodeflow_matches_oracle_on_same_sample(k):
    from scdeepsort_amd.sampler import sample_nodeflow
    c = small_case(cells=90, genes=40, dim=16, hidden=12, n_classes=4, seed=31, test_cells=0)
    G = c["G"]
    sd = O.init_params(16, 12, 4, 2, G, seed=8)
    sd["alpha"] = sd["alpha"] + 0.1 * torch.randn_like(sd["alpha"])
    rg = O.build_reference_graph(c["expr"])
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    m = make_model(sd, 16, 12, 4, 2, G).train()
    seeds = np.array([G + i for i in (4, 0, 17, 63, 88, 3, 41)])
    labels = torch.tensor([0, 1, 2, 3, 1, 0, 2])
    gen = torch.Generator(device=DEV); gen.manual_seed(100 + k)
    nf = sample_nodeflow(g, torch.from_numpy(seeds - G), 2, k, gen)
    # drawn edge count per node = min(k, in-degree incl. self-loop)
    for cb, gb in nf.blocks:
        for blk, parent in ((cb, g.cg), (gb, g.gc)):
            if blk is None:
                continue
            full = (parent.rowptr[1:] - parent.rowptr[:-1]).long()[blk.rows] + 1
            drawn = (blk.csr.rowptr[1:] - blk.csr.rowptr[:-1]).long() + blk.self_drawn.long()
            assert torch.equal(drawn, torch.clamp(full, max=k))
    logits = m(g, dev(c["feats"]), nodeflow=nf)
    loss = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
    loss.backward()
    osd = {n: t.clone().requires_grad_(True) for n, t in sd.items()}
    want = O.nodeflow_forward(osd, rg, torch.from_numpy(c["feats"]), seeds, 2, picker=_picker_from(nf, G))
    oloss = F.cross_entropy(want, labels, reduction="sum")
    oloss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.detach().numpy(), atol=TOL)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), osd[n].grad.numpy(), atol=TOL * max(1.0, float(osd[n].grad.abs().max())),
                                   err_msg=n)


def test_sampled_nodeflow_properties():
    c = small_case(seed=32)
    G = c["G"]
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, G, seed=9)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, c["dim"], c["hidden"], c["n_classes"], 2, G)
    x = dev(c["feats"])
    seeds = torch.arange(G, G + c["C"], device=DEV)[::3]
    with torch.no_grad():
        full = m(g, x, seeds=seeds)
        # expand_factor >= every in-degree: the NodeFlow is the full neighbourhood (train.py:37-38)
        big = m(g, x, seeds=seeds, num_neighbors=10 ** 6, generator=torch.Generator(device=DEV).manual_seed(1))
        a = m(g, x, seeds=seeds, num_neighbors=4, generator=torch.Generator(device=DEV).manual_seed(7))
        b = m(g, x, seeds=seeds, num_neighbors=4, generator=torch.Generator(device=DEV).manual_seed(7))
        d = m(g, x, seeds=seeds, num_neighbors=4, generator=torch.Generator(device=DEV).manual_seed(8))
    np.testing.assert_allclose(big.cpu().numpy(), full.cpu().numpy(), atol=TOL)
    assert torch.equal(a, b)                      # same seed, same draw
    assert not torch.equal(a, d)


def test_fp16_stored_features_match_oracle_on_rounded_inputs():
    """BASELINE cfg5: node features stored in fp16; the restatement gets the same fp16-rounded values and accumulates
    in fp32 (SURVEY 8d tolerance row)."""
    c = small_case(seed=41)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=11)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    f16 = dev(c["feats"]).half()
    want = O.csr_forward(sd, cg, f16.float().cpu().numpy(), 2)
    for order in ("project_first", "aggregate_first"):
        m = make_model(sd, c["dim"], c["hidden"], c["n_classes"], 2, c["G"], order)
        with torch.no_grad():
            got = m(g, f16).cpu().numpy()
        np.testing.assert_allclose(got, want, atol=TOL, err_msg=order)


@pytest.mark.parametrize("hidden,legacy_pad", [(200, False), (64, False), (50, False), (200, True)])
def test_narrow_hidden_on_the_tiled_path(hidden, legacy_pad):
    """Reference default hidden_dim = 200 (train.py:137) on graphs big enough for the LDS-streamed kernel: the tile
    kernel moves the 200-float rows natively (round 1 carried them as 256 zero-padded columns; `legacy_pad` keeps that
    route covered).  Logits and gradients match the oracle either way; hidden 50 is carried as 52 columns."""
    from scdeepsort_amd import ops
    c = small_case(cells=300, genes=180, dim=260, hidden=hidden, n_classes=6, seed=51, test_cells=0)
    G = c["G"]
    sd = O.init_params(260, hidden, 6, 2, G, seed=12)
    rg = O.build_reference_graph(c["expr"])
    seeds = np.arange(G, G + c["C"])
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 6, c["C"]))
    loss_ref, grads_ref, logits_ref = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, 2)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    m = make_model(sd, 260, hidden, 6, 2, G)
    saved = ops.TILED_MIN_WORK
    ops.TILED_MIN_WORK = 1
    ops.PAD_NARROW_TO_256 = legacy_pad
    try:
        assert m._pad_width(g, hidden) == (256 if legacy_pad else -(-hidden // 4) * 4)
        ops.PROFILE = []
        logits = m(g, dev(c["feats"]))
        kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
        ops.PROFILE = None
        assert kernels == {"agg_tiled_flat4"}
        loss = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
        loss.backward()
    finally:
        ops.TILED_MIN_WORK = saved
        ops.PROFILE = None
        ops.PAD_NARROW_TO_256 = False
    assert logits.shape == (c["C"], 6)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), logits_ref.detach().numpy(), atol=TOL)
    for n, p in m.named_parameters():
        ref = grads_ref[n].numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=TOL * max(1.0, float(np.abs(ref).max())), err_msg=n)
    assert m.embed(g, dev(c["feats"])).shape[1] == hidden
    ops.TILED_MIN_WORK = 1
    try:                                                  # seed subset on the padded path (last layer: row-wave kernel, compact rows)
        ids = torch.tensor([G + 5, G + 0, G + 77, G + 299], device=DEV)
        with torch.no_grad():
            sub = m(g, dev(c["feats"]), seeds=ids)
    finally:
        ops.TILED_MIN_WORK = saved
    np.testing.assert_allclose(sub.cpu().numpy(), logits_ref.detach().numpy()[[5, 0, 77, 299]], atol=TOL)


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer"])
@pytest.mark.parametrize("order", ["project_first", "aggregate_first"])
def test_hip_path_matches_executed_reference_code(name, order):
    """The fixtures hold logits computed by the reference's OWN gnn.py + normalize_weight, executed over a stand-in for
    DGL's NodeFlow / fn.mean (tests/golden/make_refcode_golden.py): the HIP path must reproduce them."""
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G, order)
    with torch.no_grad():
        got = m(g, dev(z["feats"]), seeds=torch.from_numpy(z["seeds"]).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(got, z["logits"], atol=TOL)
    # the device normalisation (K4) against the executed normalize_weight
    want = {(int(s), int(d)): float(w) for s, d, w in zip(z["edge_src"], z["edge_dst"], z["edge_w_norm"])}
    rp, col, val = g.cg.rowptr.cpu().numpy(), g.cg.col.cpu().numpy(), g.cg.val.cpu().numpy()
    for c in range(expr.shape[0]):
        for j in range(rp[c], rp[c + 1]):
            assert abs(val[j] - want[(int(col[j]), G + c)]) < 2e-6            # gene -> cell
    rp, col, val = g.gc.rowptr.cpu().numpy(), g.gc.col.cpu().numpy(), g.gc.val.cpu().numpy()
    for gi in range(G):
        for j in range(rp[gi], rp[gi + 1]):
            assert abs(val[j] - want[(G + int(col[j]), gi)]) < 2e-6            # cell -> gene


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer"])
def test_hip_gradients_match_executed_reference_code(name):
    """K1 forward + K2/K3 backward against the loss and gradients autograd produced through the reference's own code."""
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G).train()
    logits = m(g, dev(z["feats"]), seeds=torch.from_numpy(z["batch"]).to(DEV))
    loss = F.cross_entropy(logits, torch.from_numpy(z["labels"]).to(DEV), reduction="sum")
    loss.backward()
    assert abs(float(loss) - float(z["loss"])) < 1e-4 * max(1.0, abs(float(z["loss"])))
    for k, p in m.named_parameters():
        ref = z["grad." + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=TOL * max(1.0, float(np.abs(ref).max())), err_msg=k)


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer"])
def test_fused_loss_kernel_matches_executed_reference_code(name):
    """Round 4: the same fixtures (loss and gradients autograd produced through the reference's own `GNN.forward` +
    `CrossEntropyLoss(reduction='sum')`, train.py:36,80-84) with the loss computed by `wgnn_ce_sum_fwd_bwd`
    (`sda.cross_entropy_sum`) instead of the framework's log_softmax / nll_loss pair."""
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G).train()
    logits = m(g, dev(z["feats"]), seeds=torch.from_numpy(z["batch"]).to(DEV))
    loss = sda.cross_entropy_sum(logits, torch.from_numpy(z["labels"]).to(DEV))
    loss.backward()
    assert abs(float(loss) - float(z["loss"])) < 1e-4 * max(1.0, abs(float(z["loss"])))
    for k, p in m.named_parameters():
        ref = z["grad." + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=TOL * max(1.0, float(np.abs(ref).max())), err_msg=k)


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer"])
@pytest.mark.parametrize("order", ["auto", "project_first"])
def test_fused_full_batch_step_matches_executed_reference_code(name, order, monkeypatch):
    """Round 4: the full-batch training step on the LDS-streamed route - K1t forward, `wgnn_ce_sum_fwd_bwd`, one
    `wgnn_agg_bwd_prepare` launch per pass, K2t on pre-scaled rows - against the loss and gradients autograd produced through
    the reference's own `GNN.forward` for every cell as a seed (tests/golden/make_refcode_golden.py, `fullgrad.*`)."""
    from scdeepsort_amd import ops
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    calls = []
    real = ops.agg_bwd_prepare
    monkeypatch.setattr(ops, "agg_bwd_prepare", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G, order).train()
    logits = m(g, dev(z["feats"]))                                    # seeds=None: all cells in node order
    loss = sda.cross_entropy_sum(logits, torch.from_numpy(z["full_labels"]).to(DEV))
    loss.backward()
    assert len(calls) == (3 if int(z["n_layers"]) == 2 else 1), calls          # every pass went through the fused glue
    assert abs(float(loss) - float(z["full_loss"])) < 1e-4 * max(1.0, abs(float(z["full_loss"])))
    for k, p in m.named_parameters():
        ref = z["fullgrad." + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=TOL * max(1.0, float(np.abs(ref).max())), err_msg=k)


def test_hipgraph_replay_matches_eager():
    """GraphedForward: the forward captured into a HIP graph replays to the same logits, also on new features."""
    from scdeepsort_amd.graphed import GraphedForward
    c = small_case(seed=61)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=13)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, c["dim"], c["hidden"], c["n_classes"], 2, c["G"])
    x1 = dev(c["feats"]); x2 = dev(np.random.default_rng(9).standard_normal(c["feats"].shape).astype(np.float32))
    with torch.no_grad():
        e1, e2 = m(g, x1), m(g, x2)
    gf = GraphedForward(m, g, x1)
    assert torch.equal(gf().clone(), e1)
    assert torch.equal(gf(x2).clone(), e2)
    assert torch.equal(gf(x1).clone(), e1)


def test_integration_md_ctypes_stub_works_as_documented():
    """The reference-side binding shown in INTEGRATION.md section 2b is executed verbatim (the python block is read
    from the document) on a small block and compared with the oracle."""
    import re
    from pathlib import Path
    from scdeepsort_amd.graph import build_plan
    text = (Path(sda.__file__).resolve().parent.parent / "INTEGRATION.md").read_text()
    block = re.search(r"### 2b\..*?```python\n(.*?)```", text, re.S).group(1)
    block = block.replace('C.CDLL("scdeepsort_amd/libwgnn_hip.so")', f'C.CDLL("{Path(sda.__file__).resolve().parent / "libwgnn_hip.so"}")')
    ns = {}
    exec(block, ns)
    c = small_case(cells=60, genes=37, dim=32, seed=71, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    cg = O.build_csr_graph(c["expr"])
    G = c["G"]
    alpha = np.random.default_rng(1).uniform(0.5, 1.5, G + 2).astype(np.float32)
    bias = np.random.default_rng(2).standard_normal(32).astype(np.float32)
    zc, _ = O.csr_aggregate(cg, alpha, c["feats"][:G].astype(np.float64), c["feats"][G:].astype(np.float64))
    items = build_plan(g.cg.rowptr_host, 2048, device=DEV).items
    out = ns["block_compute_mean"](g.cg.rowptr, g.cg.col, g.cg.val, dev(alpha), dev(c["feats"][:G]), dev(c["feats"][G:]), items,
                                   src_is_gene=True, gene_num=G, bias=dev(bias), relu=True)
    np.testing.assert_allclose(out.cpu().numpy(), np.maximum(zc + bias, 0), atol=TOL)


def test_graph_without_any_edge():
    """Degenerate operand: no expressed gene at all - every node only has its self-loop (deg+1 = 1)."""
    expr = sp.csr_matrix((5, 7), dtype=np.float32)
    c = dict(dim=8, hidden=8, n_classes=3)
    sd = O.init_params(8, 8, 3, 2, 7, seed=21)
    feats = (0.5 * np.random.default_rng(4).standard_normal((12, 8))).astype(np.float32)
    g = sda.CellGeneGraph.from_expression(expr, device=DEV)
    assert g.cg.nnz == 0 and g.gc.nnz == 0
    m = make_model(sd, 8, 8, 3, 2, 7)
    with torch.no_grad():
        got = m(g, dev(feats)).cpu().numpy()
    want = O.csr_forward(sd, O.build_csr_graph(expr), feats, 2)
    np.testing.assert_allclose(got, want, atol=TOL)
    rg = O.build_reference_graph(expr)
    want2 = O.nodeflow_forward(sd, rg, torch.from_numpy(feats), np.arange(7, 12), 2).numpy()
    np.testing.assert_allclose(got, want2, atol=TOL)


@pytest.mark.parametrize("order", ["auto", "project_first", "aggregate_first"])
@pytest.mark.parametrize("dims", [(50, 30), (30, 50), (7, 5)])
def test_widths_that_are_not_multiples_of_four(order, dims):
    """The reference accepts any dense_dim / hidden_dim; the kernels move float4s, so the model carries such widths
    zero-padded (features, weights) - logits and embedding width are unchanged."""
    dim, hidden = dims
    c = small_case(cells=70, genes=45, dim=dim, hidden=hidden, n_classes=4, seed=81)
    sd = O.init_params(dim, hidden, 4, 2, c["G"], seed=14)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, dim, hidden, 4, 2, c["G"], order)
    want = O.csr_forward(sd, O.build_csr_graph(c["expr"], c["support_mask"]), c["feats"], 2)
    with torch.no_grad():
        got = m(g, dev(c["feats"]))
        emb = m.embed(g, dev(c["feats"]))
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL)
    assert emb.shape[1] == hidden
    if order == "auto":                                   # the sampled-NodeFlow path with an all-neighbours draw
        with torch.no_grad():
            big = m(g, dev(c["feats"]), num_neighbors=10 ** 6, generator=torch.Generator(device=DEV).manual_seed(3))
        np.testing.assert_allclose(big.cpu().numpy(), want, atol=TOL)


def test_predict_graph_with_only_test_cells_and_tiny_graphs():
    """(a) no support cell at all: genes have no in-edge besides their self-loop, cells still gather from genes
    (preprocess.py:184-187); (b) a 1 x 1 graph."""
    c = small_case(cells=30, genes=20, dim=16, hidden=12, n_classes=3, seed=91)
    mask = np.zeros(30, bool)
    sd = O.init_params(16, 12, 3, 2, 20, seed=15)
    g = sda.CellGeneGraph.from_expression(c["expr"], mask, device=DEV)
    assert g.gc.nnz == 0 and g.cg.nnz == c["expr"].nnz
    m = make_model(sd, 16, 12, 3, 2, 20)
    with torch.no_grad():
        got = m(g, dev(c["feats"])).cpu().numpy()
    np.testing.assert_allclose(got, O.csr_forward(sd, O.build_csr_graph(c["expr"], mask), c["feats"], 2), atol=TOL)
    rg = O.build_reference_graph(c["expr"], mask)
    np.testing.assert_allclose(got, O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), np.arange(20, 50), 2).numpy(), atol=TOL)
    one = sp.csr_matrix(np.array([[2.5]], dtype=np.float32))
    sd1 = O.init_params(4, 4, 2, 2, 1, seed=16)
    f1 = np.array([[0.3, -1.0, 0.5, 2.0], [1.5, 0.25, -0.75, 0.1]], dtype=np.float32)
    g1 = sda.CellGeneGraph.from_expression(one, device=DEV)
    with torch.no_grad():
        got1 = make_model(sd1, 4, 4, 2, 2, 1)(g1, dev(f1)).cpu().numpy()
    np.testing.assert_allclose(got1, O.csr_forward(sd1, O.build_csr_graph(one), f1, 2), atol=TOL)


@pytest.mark.parametrize("legacy_pad", [False, True])
def test_sharded_engine_narrow_hidden_on_the_tiled_path(legacy_pad):
    """ShardedWgnn on the LDS-streamed path with hidden 30: carried as 32 columns natively (or as 256 zero-padded ones
    on the round-1 route) through both layers and the head; two simulated shards (partial gene sums added by hand)
    reproduce the unsharded logits."""
    from scdeepsort_amd import ops, synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    from scdeepsort_amd.dist import shard_range
    G, C, Din, H = 300, 1000, 40, 30
    Hp = 256 if legacy_pad else 32
    rp, col, val = S.synth_expression(C, G, 0.08, device=DEV)
    torch.manual_seed(1)
    m = sda.GNN(Din, H, 5, 2, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, Din, device=DEV)
    with torch.no_grad():
        want = m(sda.CellGeneGraph.from_device_csr(rp, col, val, G), feats)
    saved = ops.TILED_MIN_WORK
    ops.TILED_MIN_WORK = 1
    ops.PAD_NARROW_TO_256 = legacy_pad
    try:
        with torch.no_grad():
            shards = []
            for r in range(2):
                lo, hi = shard_range(C, r, 2)
                b, e = int(rp[lo]), int(rp[hi])
                shards.append((lo, hi, (rp[lo:hi + 1] - rp[lo]).clone(), col[b:e].clone(), val[b:e].clone()))
            stats = [ShardedWgnn.gene_stats(c_, v_, G) for _, _, _, c_, v_ in shards]
            gstats = (stats[0][0] + stats[1][0], stats[0][1] + stats[1][1])
            eng = [ShardedWgnn.build(m, r_, c_, v_, G, global_stats=gstats) for _, _, r_, c_, v_ in shards]
            (W1, b1), (W2, b2), (Wo, bo) = eng[0]._weights()
            assert W1.shape == (Hp, Din) and W2.shape == (Hp, Hp) and Wo.shape == (5, Hp)
            p_g = F.linear(feats[:G], W1)
            p_c = [F.linear(feats[G + lo:G + hi], W1) for lo, hi, *_ in shards]
            new_c = [e._ops().cells_layer(p_g, pc, b1, True) for e, pc in zip(eng, p_c)]
            total = sum(e._ops().genes_partial(pc) for e, pc in zip(eng, p_c))
            h_g1 = eng[0]._ops().genes_finish(total, p_g, b1, True)
            p_g2 = F.linear(h_g1, W2)
            out = [e._ops().cells_layer(p_g2, F.linear(nc, W2), b2, True) for e, nc in zip(eng, new_c)]
            got = torch.cat([F.linear(o, Wo, bo) for o in out])
    finally:
        ops.TILED_MIN_WORK = saved
        ops.PAD_NARROW_TO_256 = False
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=2e-5)


def test_kat_two_layers_predict_graph_exact_rational_on_gpu():
    """The exact-rational known answer (tests/golden/make_kat_rational.py: D = 4, two layers, hub gene, a test cell and a
    gene fed by nobody) through the HIP path, both multiply orders, plus the layer-1 activations of every node."""
    from test_oracle import _kat_rational
    kat, sd, expr, support, feats = _kat_rational()
    G = kat["genes"]
    g = sda.CellGeneGraph.from_expression(expr, support, device=DEV)
    np.testing.assert_allclose(g.cg.val.cpu().numpy()[-3:], [2 / 3, 2 / 3, 5 / 3], rtol=1e-6)       # into the test cell
    assert g.gc.nnz == 5 and int(g.gc.rowptr[3] - g.gc.rowptr[2]) == 0                               # g2: no in-edge
    for order in ("project_first", "aggregate_first"):
        m = make_model({k: v.float() for k, v in sd.items()}, 4, 4, 2, 2, G, order)
        with torch.no_grad():
            x = dev(feats)
            h_g, h_c = m._layer(g, m.layers[0], x[:G], x[G:], want_genes=True, cell_rows=None)
            logits = m(g, x)
        np.testing.assert_allclose(torch.cat([h_g, h_c]).cpu().numpy(), kat["h1"], atol=2e-6)
        np.testing.assert_allclose(logits.cpu().numpy(), kat["logits"], atol=5e-6)


@pytest.mark.parametrize("unsure_rate", [0.0, 2.0, 3.0])
def test_api_classify_on_gpu_matches_oracle_postprocess(unsure_rate):
    """a10 (predict.py:78-88) on device logits produced by the HIP forward."""
    from scdeepsort_amd.api import _classify
    c = small_case(seed=9)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=4)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, c["dim"], c["hidden"], c["n_classes"], 2, c["G"])
    with torch.no_grad():
        logits = m(g, dev(c["feats"])) * 3.0
    pred, prob = _classify(logits, unsure_rate)
    want, wprob = O.postprocess(logits.cpu().numpy(), unsure_rate)
    np.testing.assert_allclose(prob, wprob, atol=1e-6)
    clear = np.abs(wprob.max(1) - unsure_rate / c["n_classes"]) > 1e-6
    np.testing.assert_array_equal(pred[clear], want[clear])
    if unsure_rate == 3.0:
        assert (pred == -1).any() and (pred >= 0).any()


def test_large_seed_batch_falls_back_to_the_full_transposed_graph():
    """A "batch" whose block capacity (B x longest row) exceeds ops.SEED_BLOCK_MAX_CAP walks the full transposed graph
    with a zero-padded gradient instead of building a seed block: same gradients (incl. alpha of the genes)."""
    from scdeepsort_amd import ops
    c = small_case(cells=80, genes=48, dim=16, hidden=12, n_classes=4, seed=15, test_cells=0)
    sd = O.init_params(16, 12, 4, 1, 48, seed=6)
    rg = O.build_reference_graph(c["expr"])
    seeds = np.array([48 + i for i in (0, 5, 9, 33, 70, 3, 5)])
    labels = torch.tensor([0, 1, 2, 3, 1, 0, 2])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, 1)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    saved, ops.SEED_BLOCK_MAX_CAP = ops.SEED_BLOCK_MAX_CAP, 0
    try:
        m = make_model(sd, 16, 12, 4, 1, 48)
        l = F.cross_entropy(m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds).to(DEV)), labels.to(DEV), reduction="sum")
        l.backward()
    finally:
        ops.SEED_BLOCK_MAX_CAP = saved
    assert l.item() == pytest.approx(float(loss), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=k)


def test_repeated_seeds_accumulate_gradients():
    """A seed listed twice is two NodeFlow rows (train.py:71-81 would never draw that, but the operator must not lose
    a gradient - ADVICE r1): logits repeat, gradients add, both orders, vs the oracle's autograd on the same seed list."""
    c = small_case(cells=60, genes=40, dim=16, hidden=12, n_classes=4, seed=33, test_cells=0)
    sd = O.init_params(16, 12, 4, 2, 40, seed=8)
    rg = O.build_reference_graph(c["expr"])
    seeds = np.array([40 + i for i in (7, 2, 7, 30, 2, 7)])
    labels = torch.tensor([0, 1, 2, 3, 1, 0])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, 2)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    for order in ("project_first", "aggregate_first"):
        m = make_model(sd, 16, 12, 4, 2, 40, order)
        logits = m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds).to(DEV))
        assert torch.equal(logits[0], logits[2]) and torch.equal(logits[1], logits[4])
        l = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
        l.backward()
        assert l.item() == pytest.approx(float(loss), rel=1e-5)
        for k, p in m.named_parameters():
            np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=k)


@pytest.mark.parametrize("B", [1, 5, 64, 300])
def test_device_built_seed_plan_and_block(B):
    """AggCsr.subplan / seed_block_transposed are built on the device with static shapes (no host round trip): the plan
    covers every seed row exactly once in S equal chunks, the source-major block lists every in-edge of the batch once,
    sorted by source then by slot."""
    c = small_case(cells=400, genes=120, dim=8, seed=B, density=0.3, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    rng = np.random.default_rng(B)
    ids = rng.integers(0, 400, B).astype(np.int32)                   # with repeats
    ids[0] = 3                                                       # the empty cell
    ids32, plan = g.cg.subplan(torch.from_numpy(ids).to(DEV))
    rp = c["expr"].indptr
    items = plan.items.cpu().numpy()
    S = len(items) // B
    assert len(items) == B * S and plan.n_partials == (B * S if S > 1 else 0) and plan.n_long == (B if S > 1 else 0)
    for i in range(B):
        segs = items[i * S:(i + 1) * S]
        assert (segs[:, 0] == i).all() and segs[0, 1] == rp[ids[i]] and segs[-1, 2] == rp[ids[i] + 1]
        assert (segs[1:, 1] == segs[:-1, 2]).all() and (segs[:, 2] >= segs[:, 1]).all()
        assert (segs[:, 3] == (np.arange(i * S, (i + 1) * S) if S > 1 else -1)).all()
    t_rowptr, t_slot, t_val, t_items = g.cg.seed_block_transposed(ids32)
    t_rowptr, t_slot, t_val = t_rowptr.cpu().numpy(), t_slot.cpu().numpy(), t_val.cpu().numpy()
    want = []                                                        # (source, slot, weight) of every in-edge of the batch
    val = g.cg.val.cpu().numpy()
    for i, r in enumerate(ids):
        for j in range(rp[r], rp[r + 1]):
            want.append((int(c["expr"].indices[j]), i, float(val[j])))
    want.sort(key=lambda t: (t[0], t[1]))
    assert t_rowptr[-1] == len(want) and t_rowptr[0] == 0
    got = [(int(np.searchsorted(t_rowptr, j, side="right") - 1), int(t_slot[j]), float(t_val[j])) for j in range(len(want))]
    assert got == want
    assert (t_val[len(want):] == 0).all()
    ti = t_items.cpu().numpy()
    assert (ti[:, 1] == t_rowptr[:-1]).all() and (ti[:, 2] == t_rowptr[1:]).all() and (ti[:, 3] == -1).all()


def test_hipgraph_replay_with_seeds_and_graphed_train_step():
    """(a) GraphedForward with a seed list (the seed sub-plan used to be built on the host, illegal during
    capture); (b) GraphedTrainStep: captured mini-batch steps (forward, CE-sum, backward, Adam) reproduce the eager
    run on the same batches."""
    import copy
    from scdeepsort_amd.graphed import GraphedForward, GraphedTrainStep
    c = small_case(cells=300, genes=80, dim=16, hidden=12, n_classes=4, seed=71, test_cells=0)
    sd = O.init_params(16, 12, 4, 1, 80, seed=2)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    x = dev(c["feats"])
    m = make_model(sd, 16, 12, 4, 1, 80)
    seeds = torch.tensor([80 + i for i in (5, 1, 250, 3, 77)], device=DEV)
    with torch.no_grad():
        want = m(g, x, seeds=seeds)
    gf = GraphedForward(m, g, x, seeds=seeds)
    assert torch.equal(gf().clone(), want)
    gf.seeds.copy_(seeds.flip(0))                                    # the plan is rebuilt inside the graph from the id buffer
    assert torch.equal(gf().clone(), want.flip(0))

    y = (torch.arange(300, device=DEV) * 7 % 4).long()
    rng = np.random.default_rng(0)
    batches = [torch.from_numpy(rng.choice(300, 32, replace=False) + 80).to(DEV) for _ in range(9)] + \
              [torch.from_numpy(rng.choice(300, 7, replace=False) + 80).to(DEV)]             # a tail batch

    def run(graphed):
        model = make_model(sd, 16, 12, 4, 1, 80).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4, capturable=True)

        def step(batch):
            loss = F.cross_entropy(model(g, x, seeds=batch), y[batch - 80], reduction="sum")
            opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
            return loss.detach()
        fn = GraphedTrainStep(step, 32, torch.device(DEV)) if graphed else step
        losses = [float(fn(b)) for b in batches]
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, fn

    l_e, sd_e, _ = run(False)
    l_g, sd_g, fn = run(True)
    assert fn.replays == 6                                           # 3 eager warm-up steps, 6 replays, 1 eager tail
    np.testing.assert_allclose(l_g, l_e, rtol=1e-5)
    for k in sd_e:
        np.testing.assert_allclose(sd_g[k].cpu().numpy(), sd_e[k].cpu().numpy(), atol=1e-6, err_msg=k)
    assert l_e[-2] < l_e[0]                                          # and it trains


def test_full_size_cfg3_training_step_matches_cpu_autograd():
    """BASELINE cfg3/cfg4 at FULL size: one training step (2-layer forward through the tiled kernels, CE-sum loss,
    backward through K2t/K3t) against an independent CPU evaluation - torch.sparse CSR matmuls + torch autograd in FP64
    over the same normalised operand (round 6: an fp32 reference carries its own summation error of the size being tested).
    Loss to 1e-6 relative; every parameter gradient in two tiers set from the errors observed on the MI355X (below;
    fp32 sums over up to 1e5 terms); alpha on all 20,002 entries."""
    # Two tiers.  Of the 2.6e7 + 5e6 ReLU units a handful have a pre-activation within fp32 rounding of 0; fp32 and fp64 put
    # them on different sides, and the gradient of such a unit is a discrete jump confined to a few elements (one flipped unit of
    # layer 2 moves ONE row of layers.1's weight gradient and one bias element by ~2e-4 of the tensor's max - observed with one
    # feature draw, not with another; a layer-1 flip reaches the ~800 alpha entries of that cell's genes).  So: the BULK of every
    # gradient tensor (its 99 % error quantile) is held to 4 x the error observed where no unit flipped (alpha 1.3e-4 - row dots
    # of mixed sign -, layers.0 weight 1.8e-5, the others <= 2.4e-6 of their max), the MAXIMUM to what a few flips can do.
    # (second feature draw, with flips: bulk alpha 2.6e-5, layers.0 weight / bias 2.0e-5 / 5.1e-5, layers.1 weight / bias 2.4e-6 /
    #  7.8e-5 - a bias has 256 elements, three flipped units ARE its 99 % quantile -, head 6e-7; maxima alpha 6.3e-4, layers.1 1.9e-4)
    GRAD_TOL = {"alpha": 6e-4}
    GRAD_TOL_DEFAULT = 2e-4
    BULK_Q, FLIP_TOL = 0.99, 5e-3
    from scdeepsort_amd import synthetic as S
    cfg = S.CONFIGS["cfg3"]
    G, C = cfg.genes, cfg.cells
    rp, col, val = S.synth_expression(C, G, cfg.density, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    torch.manual_seed(3)
    m = sda.GNN(cfg.dense_dim, cfg.hidden, cfg.n_classes, 2, G, activation=F.relu).to(DEV)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, cfg.dense_dim, device=DEV)
    labels = (torch.arange(C, device=DEV) * 2654435761 % cfg.n_classes).long()
    loss = F.cross_entropy(m(g, feats), labels, reduction="sum")
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
    # ---- CPU oracle: same math with torch sparse CSR + autograd, in fp64
    def tcsr(d, shape):
        return torch.sparse_csr_tensor(d.rowptr.long().cpu(), d.col.long().cpu(), d.val.cpu().double(), size=shape)
    A_cg, A_gc = tcsr(g.cg, (C, G)), tcsr(g.gc, (G, C))
    inv_c, inv_g = g.cg.inv_deg.cpu().double().unsqueeze(1), g.gc.inv_deg.cpu().double().unsqueeze(1)
    p = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in m.named_parameters()}
    a = p["alpha"].reshape(-1)
    h_g, h_c = feats[:G].cpu().double(), feats[G:].cpu().double()
    for i in range(2):
        W, b = p[f"layers.{i}.fc_neigh.weight"], p[f"layers.{i}.fc_neigh.bias"]
        p_g, p_c = F.linear(h_g, W), F.linear(h_c, W)
        n_c = torch.relu((torch.sparse.mm(A_cg, p_g * a[:G, None]) + a[G + 1] * p_c) * inv_c + b)
        if i == 0:
            h_g = torch.relu((a[:G, None] * torch.sparse.mm(A_gc, p_c) + a[G] * p_g) * inv_g + b)
        h_c = n_c
    ref = F.cross_entropy(F.linear(h_c, p["linear.weight"], p["linear.bias"]), labels.cpu(), reduction="sum")
    ref.backward()
    print(f"full-size cfg3 step: loss {float(loss):.4f} vs fp64 {float(ref):.4f} (rel {abs(float(loss) - float(ref)) / abs(float(ref)):.2e})")
    assert abs(float(loss) - float(ref)) < 1e-6 * abs(float(ref)), (float(loss), float(ref))
    bad = {}
    for k, q in m.named_parameters():
        want, got = p[k].grad.numpy(), q.grad.cpu().double().numpy()
        scale = np.abs(want).max()
        err = np.abs(got - want).reshape(-1) / scale
        bulk, worst = float(np.quantile(err, BULK_Q)), float(err.max())
        print(f"   grad {k}: |err| / max |grad|: {BULK_Q:.0%} quantile {bulk:.2e}, max {worst:.2e}")
        if bulk >= GRAD_TOL.get(k, GRAD_TOL_DEFAULT) or worst >= FLIP_TOL:
            bad[k] = (bulk, worst)
    assert not bad, bad


def test_full_size_cfg4_eight_virtual_ranks_training_gradients_match_unsharded():
    """BASELINE cfg4 at FULL size ("Same 100k x 20k graph, training loop, cells sharded 8-way"): eight `ShardedWgnn` engines of
    12 500 cells each run the production `dist.sharded_forward` training branch in eight threads of ONE process on one GPU;
    the differentiable [G, H] all-reduce is replaced by an in-process rendezvous that sums the eight partial tensors (forward:
    the sum; backward: autograd adds the eight consumers' gradients - what the all-reduce of dH1_g does), the parameter-gradient
    all-reduce by autograd accumulating into the one shared parameter set.  Loss and every gradient (alpha on all 20 002
    entries) against the unsharded full-batch step of the same model on the whole graph."""
    import threading
    from scdeepsort_amd import dist as D, ops, synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    cfg = S.CONFIGS["cfg3"]
    G, C, N = cfg.genes, cfg.cells, 8
    rp, col, val = S.synth_expression(C, G, cfg.density, device=DEV)
    torch.manual_seed(3)
    m = sda.GNN(cfg.dense_dim, cfg.hidden, cfg.n_classes, 2, G, activation=F.relu).to(DEV)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, cfg.dense_dim, device=DEV)
    labels = (torch.arange(C, device=DEV) * 2654435761 % cfg.n_classes).long()
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    ref_loss = sda.cross_entropy_sum(m(g, feats), labels)
    ref_loss.backward()
    want = {k: q.grad.detach().clone() for k, q in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    del g
    stats = ShardedWgnn.gene_stats(col, val, G)
    engines = []
    for r in range(N):
        lo, hi = D.shard_range(C, r, N)
        b, e = int(rp[lo]), int(rp[hi])
        engines.append((lo, hi, ShardedWgnn.build(m, (rp[lo:hi + 1] - rp[lo]).clone(), col[b:e].clone(), val[b:e].clone(), G,
                                                  global_stats=stats)))
    bar, parts, box, tl = threading.Barrier(N), [None] * N, {}, threading.local()

    def rendezvous_sum(x):                                  # stands in for the differentiable SUM all-reduce of dist.sharded_forward
        parts[tl.rank] = x
        if bar.wait() == 0:
            tot = parts[0]
            for q in parts[1:]:
                tot = tot + q
            box["total"] = tot
        bar.wait()
        return box["total"]

    losses, errors = [None] * N, []

    def rank_main(r):
        try:
            tl.rank = r
            lo, hi, eng = engines[r]
            with torch.cuda.device(DEV), torch.enable_grad():
                logits = D.sharded_forward(eng._weights(), None, feats[:G], feats[G + lo:G + hi], eng._ops(), 2, gather_logits=False,
                                           linear=ops.linear)
                losses[r] = sda.cross_entropy_sum(logits, labels[lo:hi])
        except BaseException as ex:                          # a failing rank must not leave the others at the barrier
            errors.append(ex)
            bar.abort()

    met = []
    # (round 6: the training branch issues the all-reduce in two halves around the cells<-genes pass: all_reduce_sum_begin)
    saved, D.all_reduce_sum_begin = D.all_reduce_sum_begin, lambda x: (met.append(1), (rendezvous_sum(x), lambda y: y))[1]
    try:
        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(N)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        D.all_reduce_sum_begin = saved
    assert not errors, errors
    assert len(met) == N, met                               # every virtual rank went through the (stand-in) collective
    loss = losses[0]
    for q in losses[1:]:
        loss = loss + q
    loss.backward()
    lv, rv = float(loss.detach()), float(ref_loss.detach())
    assert abs(lv - rv) < 1e-5 * abs(rv), (lv, rv)
    for k, q in m.named_parameters():
        scale = float(want[k].abs().max())
        err = float((q.grad - want[k]).abs().max())
        assert err < 1e-3 * scale + 1e-6, (k, err, scale)


@pytest.mark.parametrize("M,N,K", [(1, 16, 4), (127, 200, 200), (128, 256, 400), (1000, 16, 256), (777, 132, 52), (4096, 256, 256)])
@pytest.mark.parametrize("relu,with_bias", [(True, True), (False, False)])
def test_linear_fwd_on_the_fp32_matrix_cores(M, N, K, relu, with_bias):
    """wgnn_linear_fwd = NodeUpdate's relu(fc_neigh(.)) / the head (gnn.py:18-25,66-67) on v_mfma_f32_32x32x2_f32:
    against an fp64 evaluation, edge tiles in every dimension, strided inputs."""
    from scdeepsort_amd import ops
    rng = np.random.default_rng(M + N + K)
    xw = rng.standard_normal((M, K + 4)).astype(np.float32); w = rng.standard_normal((N, K)).astype(np.float32) / np.sqrt(K)
    b = rng.standard_normal(N).astype(np.float32) if with_bias else None
    x = dev(xw)[:, :K]                                            # leading dimension K + 4
    out = ops.linear_fwd(x, dev(w), dev(b) if with_bias else None, relu=relu)
    want = xw[:, :K].astype(np.float64) @ w.astype(np.float64).T + (b if with_bias else 0)
    want = np.maximum(want, 0) if relu else want
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=2e-5)


def test_agg_linear_relu_fused_entry_matches_reference_order():
    """wgnn_agg_linear_relu_fwd (SURVEY 8b's optional fused entry): one reference layer on a block in the reference's
    literal order - aggregate (gnn.py:47-56,65) then relu(fc_neigh(neigh)) (gnn.py:18-25) - through the C ABI only."""
    from scdeepsort_amd import _lib
    from scdeepsort_amd.graph import _ptr, _stream
    c = small_case(cells=300, genes=120, dim=24, hidden=20, seed=17, density=0.2, test_cells=0)
    G = c["G"]
    sd = O.init_params(24, 20, 4, 1, G, seed=9)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV, chunk=16)           # long-row splitting too
    cg = O.build_csr_graph(c["expr"])
    alpha = sd["alpha"].numpy().ravel()
    zc, _ = O.csr_aggregate(cg, alpha, c["feats"][:G].astype(np.float64), c["feats"][G:].astype(np.float64), want_genes=False)
    W, b = sd["layers.0.fc_neigh.weight"].numpy(), sd["layers.0.fc_neigh.bias"].numpy()
    want = np.maximum(zc @ W.T.astype(np.float64) + b, 0)
    x = dev(c["feats"]); d = torch.device(DEV)
    csr, plan = g.cg, g.cg.plan
    neigh = torch.empty(csr.n_rows, 24, device=DEV); out = torch.empty(csr.n_rows, 20, device=DEV)
    part = torch.empty(max(1, plan.n_partials) * 24, device=DEV)
    a_d, W_d, b_d = dev(alpha), dev(W), dev(b)
    hs, hc = x[:G].contiguous(), x[G:].contiguous()
    rc = _lib.call(d, "wgnn_agg_linear_relu_fwd", _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(a_d), sda.SRC_IS_GENE,
                   G + 1, _ptr(hs), 24, _ptr(hc), 24, None, _ptr(csr.inv_deg), csr.n_rows, 24, 0,
                   _ptr(plan.items), plan.n_items, _ptr(plan.long_rows) if plan.n_long else None, plan.n_long,
                   _ptr(part), plan.n_partials, _ptr(neigh), _ptr(W_d), 24, _ptr(b_d), 20, 1, _ptr(out), 20, _stream(d))
    assert rc == 0
    np.testing.assert_allclose(neigh.cpu().numpy(), zc, atol=TOL)
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)
    assert _lib.call(d, "wgnn_agg_linear_relu_fwd", _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(a_d), sda.SRC_IS_GENE,
                     G + 1, _ptr(hs), 24, _ptr(hc), 24, None, _ptr(csr.inv_deg), csr.n_rows, 24, 0,
                     _ptr(plan.items), plan.n_items, None, 0, None, 0, None, _ptr(W_d), 24, _ptr(b_d), 20, 1, _ptr(out), 20,
                     _stream(d)) == -4                                             # missing scratch -> WGNN_ERR_WORKSPACE


# ------------------------------------------------------------------------------------------------
# K5: device sampler with static shapes (wgnn_sample_rows)
def _picker_from_static(nf, G):
    table = {}
    for b, (cb, gb) in enumerate(nf.blocks):
        for blk, is_cell in ((cb, True), (gb, False)):
            if blk is None:
                continue
            rows = blk.rows.cpu().numpy(); kk = blk.csr.ell_k
            cnt = blk.csr.ell_cnt.cpu().numpy(); col = blk.csr.col.cpu().numpy().astype(np.int64)
            sd = blk.self_drawn.cpu().numpy()
            for j, r in enumerate(rows):
                me = int(r) + (G if is_cell else 0)
                src = col[j * kk: j * kk + cnt[j]] + (0 if is_cell else G)
                table[(b, me)] = np.concatenate([src, [me]]) if sd[j] > 0 else src
    return lambda block, v: table[(block, v)]


@pytest.mark.parametrize("k,n_layers", [(1, 1), (3, 1), (8, 1), (3, 2), (8, 2), (70, 2)])
def test_device_sampled_nodeflow_matches_oracle_on_same_sample(k, n_layers):
    """num_neighbors > 0 (train.py:37-40,71-78) through K5 + K1/K2/K3: logits and all gradients against the oracle
    replaying exactly the drawn sample; draw counts = min(k, in-degree incl. the self-loop); no edge drawn twice."""
    from scdeepsort_amd.sampler import DeviceSampler, sample_nodeflow_static
    c = small_case(cells=90, genes=40, dim=16, hidden=12, n_classes=4, seed=31, test_cells=0)
    G = c["G"]
    sd = O.init_params(16, 12, 4, n_layers, G, seed=8)
    rg = O.build_reference_graph(c["expr"])
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    m = make_model(sd, 16, 12, 4, n_layers, G).train()
    seeds = np.array([G + i for i in (4, 0, 17, 63, 88, 3, 41)])
    labels = torch.tensor([0, 1, 2, 3, 1, 0, 2])
    smp = DeviceSampler(100 + k, torch.device(DEV))
    nf = sample_nodeflow_static(g, torch.from_numpy(seeds - G).to(DEV), n_layers, k, smp)
    assert int(smp.step) == 1
    for cb, gb in nf.blocks:
        for blk, parent in ((cb, g.cg), (gb, g.gc)):
            if blk is None:
                continue
            full = (parent.rowptr[1:] - parent.rowptr[:-1]).long()[blk.rows] + 1
            drawn = blk.csr.ell_cnt.long() + blk.self_drawn.long()
            assert torch.equal(drawn, torch.clamp(full, max=k))
            np.testing.assert_allclose(blk.csr.inv_deg.cpu().numpy(), 1.0 / drawn.cpu().numpy(), rtol=1e-6)
            kk, cnt, col = blk.csr.ell_k, blk.csr.ell_cnt.cpu().numpy(), blk.csr.col.cpu().numpy()
            prp = parent.rowptr.cpu().numpy(); pcol = parent.col.cpu().numpy()
            for j, r in enumerate(blk.rows.cpu().numpy()):
                mine = col[j * kk: j * kk + cnt[j]]
                assert len(set(mine.tolist())) == len(mine) and set(mine.tolist()) <= set(pcol[prp[r]:prp[r + 1]].tolist())
    logits = m(g, dev(c["feats"]), nodeflow=nf)
    loss = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
    loss.backward()
    osd = {n: t.clone().requires_grad_(True) for n, t in sd.items()}
    want = O.nodeflow_forward(osd, rg, torch.from_numpy(c["feats"]), seeds, n_layers, picker=_picker_from_static(nf, G))
    oloss = F.cross_entropy(want, labels, reduction="sum")
    oloss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.detach().numpy(), atol=TOL)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), osd[n].grad.numpy(), atol=TOL * max(1.0, float(osd[n].grad.abs().max())),
                                   err_msg=n)


def test_device_sampler_is_uniform_seeded_and_advances():
    """Floyd's draw on the device: every candidate of a row (its in-edges and the self-loop) is drawn with probability
    k/m; the same (seed, step) reproduces the sample, the next step differs; k >= every degree = full neighbourhood."""
    from scdeepsort_amd.sampler import DeviceSampler, sample_block_static
    c = small_case(cells=60, genes=50, dim=8, seed=44, density=0.5, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    csr = g.cg
    rp = csr.rowptr.cpu().numpy(); pcol = csr.col.cpu().numpy()
    row = int(np.argmax(np.diff(rp)))                               # the longest row
    deg = int(rp[row + 1] - rp[row]); m = deg + 1; k = 5
    rows = torch.full((512,), row, device=DEV)                      # 512 independent draws of the same row per call
    smp = DeviceSampler(7, torch.device(DEV))
    hits = np.zeros(pcol.max() + 2); selfs = 0; n_draws = 0
    first = None
    for it in range(8):
        blk = sample_block_static(csr, rows, k, smp, stream_id=0)
        col = blk.csr.col.cpu().numpy().reshape(512, -1); cnt = blk.csr.ell_cnt.cpu().numpy()
        if first is None:
            first = col.copy()
            assert (col == col[0]).all()                            # same (seed, step, stream, row) -> same draw
        else:
            assert it == 0 or not (col == first).all()
        hits[col[0, :cnt[0]]] += 1; selfs += float(blk.self_drawn[0]); n_draws += 1
        smp.advance()
    # many steps on one row: empirical inclusion probability ~ k/m for every candidate
    smp2 = DeviceSampler(11, torch.device(DEV))
    freq = np.zeros(m)
    one = torch.tensor([row], device=DEV)
    pos = {int(cv): i for i, cv in enumerate(pcol[rp[row]:rp[row + 1]])}
    N = 3000
    for it in range(N):
        blk = sample_block_static(csr, one, k, smp2, stream_id=3)
        n = int(blk.csr.ell_cnt[0])
        for cv in blk.csr.col[:n].cpu().numpy():
            freq[pos[int(cv)]] += 1
        freq[deg] += float(blk.self_drawn[0])
        smp2.advance()
    p = k / m
    assert abs(freq.sum() / N - k) < 1e-9
    assert np.abs(freq / N - p).max() < 5 * np.sqrt(p * (1 - p) / N) + 0.01
    full = sample_block_static(csr, None, 10 ** 6, DeviceSampler(1, torch.device(DEV)), 0)
    assert torch.equal(full.csr.ell_cnt.long(), (csr.rowptr[1:] - csr.rowptr[:-1]).long()) and bool((full.self_drawn == 1).all())


def test_graphed_training_step_with_device_sampled_neighbours():
    """A captured mini-batch step with num_neighbors > 0 draws a NEW sample at every replay (the sampler's step counter
    lives on the device and is advanced inside the graph) and trains."""
    from scdeepsort_amd.graphed import GraphedTrainStep
    from scdeepsort_amd.sampler import DeviceSampler
    c = small_case(cells=300, genes=80, dim=16, hidden=12, n_classes=4, seed=71, test_cells=0)
    sd = O.init_params(16, 12, 4, 2, 80, seed=2)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    x = dev(c["feats"])
    y = (torch.arange(300, device=DEV) * 7 % 4).long()
    model = make_model(sd, 16, 12, 4, 2, 80).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    smp = DeviceSampler(3, torch.device(DEV))

    def step(batch):
        loss = F.cross_entropy(model(g, x, seeds=batch, num_neighbors=4, generator=smp), y[batch - 80], reduction="sum")
        opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
        return loss.detach()
    fn = GraphedTrainStep(step, 32, torch.device(DEV))
    batch = torch.arange(80, 112, device=DEV)
    losses = [float(fn(batch)) for _ in range(12)]
    assert fn.replays == 9 and int(smp.step) == 12                 # the counter advanced inside every replay
    assert len({round(l, 4) for l in losses}) > 6                  # different samples -> different losses
    assert np.mean(losses[-3:]) < np.mean(losses[:3])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tile_kernel_fuzz_against_rowwave(seed):
    """Randomised shapes / densities / widths / tile geometries / LDS block heights (hub genes, empty cells): the tile
    kernel against the row-wave kernel (both already pinned to the oracle) - a guard for the hand-counted waitcnt /
    computed-branch code paths that fixed-size tests may not reach."""
    from scdeepsort_amd import ops
    from scdeepsort_amd.graph import build_tile_plan
    rng = np.random.default_rng(1000 + seed)
    saved = ops.TILED_MIN_WORK
    ops.TILED_MIN_WORK = None
    try:
        for it in range(12):
            C = int(rng.integers(20, 2500)); G = int(rng.integers(10, 1200)); dens = float(rng.uniform(0.005, 0.4))
            D = int(rng.choice([256, 256, 128, 64, 200, 4 * int(rng.integers(1, 65))]))
            m = rng.random((C, G)) < dens
            if rng.random() < 0.5:
                m[:, rng.integers(0, G)] = True                              # a hub gene
            if rng.random() < 0.5:
                m[rng.integers(0, C), :] = False                             # an empty cell
            x = sp.csr_matrix(np.where(m, rng.uniform(0.5, 7, (C, G)), 0).astype(np.float32))
            if x.nnz == 0:
                continue
            g = sda.CellGeneGraph.from_expression(x, device=DEV)
            alpha = torch.rand(G + 2, device=DEV) + 0.5
            hg = torch.randn(G, D, device=DEV); hc = torch.randn(C, D, device=DEV)
            kb = int(rng.integers(16, 79))
            for csr, mode, si, hs, hself in ((g.cg, sda.SRC_IS_GENE, G + 1, hg, hc), (g.gc, sda.DST_IS_GENE, G, hc, hg)):
                rt = int(rng.integers(1, 8)); cs = int(rng.integers(1, 6))
                tp = build_tile_plan(csr, None if rng.random() < 0.3 else max(rt, -(-csr.n_rows // 256)), cs, block_rows=kb)
                ref = ops.agg_fwd(csr, alpha, mode, si, hs, hself)
                out = ops.agg_fwd_tiled(csr, tp, alpha, mode, si, hs, hself)
                err = float((ref - out).abs().max())
                assert err < TOL, (it, C, G, dens, D, kb, rt, cs, err)
    finally:
        ops.TILED_MIN_WORK = saved


@pytest.mark.parametrize("M,N,K", [(20000, 256, 400), (16400, 200, 52), (70001, 16, 256), (513, 4, 4)])
def test_linear_weight_gradient_on_the_matrix_cores(M, N, K):
    """wgnn_linear_wgrad: dW = g^T x reduced over the node axis in slabs (fixed-order fold), against fp64; and
    ops.linear's autograd (dx, dW, db) against torch's own Linear."""
    from scdeepsort_amd import ops
    rng = np.random.default_rng(M)
    g = rng.standard_normal((M, N)).astype(np.float32); x = rng.standard_normal((M, K)).astype(np.float32)
    dW = ops.linear_wgrad(dev(g), dev(x))
    want = g.astype(np.float64).T @ x.astype(np.float64)
    np.testing.assert_allclose(dW.cpu().numpy(), want, atol=2e-3 * np.sqrt(M / 20000), rtol=1e-4)
    assert torch.equal(dW, ops.linear_wgrad(dev(g), dev(x)))                       # deterministic
    if M >= ops.WGRAD_MIN_ROWS:
        xs = [dev(x).requires_grad_(True) for _ in range(2)]
        Ws = [dev(rng.standard_normal((N, K)).astype(np.float32) * 0.05).requires_grad_(True)]; Ws.append(Ws[0].detach().clone().requires_grad_(True))
        bs = [dev(rng.standard_normal(N).astype(np.float32)).requires_grad_(True)]; bs.append(bs[0].detach().clone().requires_grad_(True))
        up = dev(g)
        (ops.linear(xs[0], Ws[0], bs[0]) * up).sum().backward()
        (F.linear(xs[1], Ws[1], bs[1]) * up).sum().backward()
        np.testing.assert_allclose(Ws[0].grad.cpu().numpy(), Ws[1].grad.cpu().numpy(), atol=2e-3 * np.sqrt(M / 20000), rtol=1e-4)
        np.testing.assert_allclose(xs[0].grad.cpu().numpy(), xs[1].grad.cpu().numpy(), atol=1e-5)
        np.testing.assert_allclose(bs[0].grad.cpu().numpy(), bs[1].grad.cpu().numpy(), atol=1e-3, rtol=1e-5)


# ---- large seed sets: predict.py:61-88 makes EVERY test cell a seed -----------------------------
@pytest.mark.parametrize("n_layers,order", [(1, "auto"), (2, "project_first"), (2, "aggregate_first")])
def test_large_seed_set_runs_the_lds_streamed_kernel_and_matches_oracle(n_layers, order, monkeypatch):
    """A seed set covering >= ops.SEED_FULL_PASS_MIN_FRAC of the rows of a tile-kernel operand must NOT fall to the row-wave
    kernel: the full LDS-streamed pass runs and the seeds' rows are gathered (shuffled order, a repeated seed, test cells
    of a predict graph).  Logits and every gradient against the oracle's NodeFlow emulation on the same seeds."""
    from scdeepsort_amd import ops
    c = small_case(cells=120, genes=64, dim=24, hidden=16, n_classes=5, seed=31, test_cells=10)
    sd = O.init_params(24, 16, 5, n_layers, 64, seed=8)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    rng = np.random.default_rng(3)
    seeds = rng.permutation(np.arange(64, 64 + 120))[:90]
    seeds[7] = seeds[3]                                                    # a repeated seed
    labels = torch.from_numpy(rng.integers(0, 5, len(seeds)))
    loss, grads, want = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, n_layers)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    m = make_model(sd, 24, 16, 5, n_layers, 64, order)
    ops.PROFILE = []
    try:
        logits = m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds).to(DEV))
        kernels = [dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert kernels and set(kernels) == {"agg_tiled_flat4"}, kernels          # no row-wave launch anywhere in the forward
    np.testing.assert_allclose(logits.detach().cpu().numpy(), want.detach().numpy(), atol=TOL)
    l = F.cross_entropy(logits, labels.to(DEV), reduction="sum")
    l.backward()
    assert l.item() == pytest.approx(float(loss), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=k)
    # a SMALL batch on the same operand keeps the row-wave kernel and its bit-identical batching property
    few = torch.from_numpy(seeds[:5]).to(DEV)
    with torch.no_grad():
        a = m(g, dev(c["feats"]), seeds=few)
        b = m(g, dev(c["feats"]), seeds=torch.from_numpy(seeds[:9]).to(DEV))[:5]
    assert torch.equal(a, b)
    np.testing.assert_allclose(a.cpu().numpy(), want.detach().numpy()[:5], atol=TOL)


def test_all_cells_as_shuffled_seeds_at_cfg3_size():
    """GNN.forward(seeds = all 100k cfg3 cells, shuffled) - the shape of DeepSortPredictor.predict at atlas scale - against
    the seeds=None pass: same logits (<= 1e-4) in seed order, only LDS-streamed launches, within 1.2x of its time."""
    from scdeepsort_amd import ops, synthetic as S
    cfg = S.CONFIGS["cfg3"]
    G, C = cfg.genes, cfg.cells
    rp, col, val = S.synth_expression(C, G, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    del rp, col, val
    torch.manual_seed(2)
    m = sda.GNN(cfg.dense_dim, cfg.hidden, cfg.n_classes, 2, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, cfg.dense_dim, device=DEV)
    perm = torch.randperm(C, device=DEV)
    seeds = perm + G

    def timed(fn, reps=5):
        for _ in range(2):
            out = fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record(); torch.cuda.synchronize()
        return out, e0.elapsed_time(e1) / reps

    with torch.no_grad():
        full, t_full = timed(lambda: m(g, feats))
        ops.PROFILE = []
        try:
            m(g, feats, seeds=seeds)
            kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
        finally:
            ops.PROFILE = None
        sub, t_seeds = timed(lambda: m(g, feats, seeds=seeds))
    assert kernels == {"agg_tiled_flat4"}, kernels
    assert (sub - full[perm]).abs().max().item() < TOL
    assert t_seeds < 1.2 * t_full, (t_seeds, t_full)


# ---- ABI 0.2.0: fp16-stored inputs / row-scaled second output of the dense half, int64 row pointers -----------------
@pytest.mark.parametrize("M,N,K", [(5, 16, 8), (300, 200, 52), (2049, 256, 400)])
@pytest.mark.parametrize("half_in", [False, True])
def test_linear_fwd_ex_fp16_input_and_row_scaled_second_output(M, N, K, half_in):
    """wgnn_linear_fwd_ex: x stored in fp16 is widened in the loader (fp16-rounded inputs, fp32 multiply-accumulate; the
    reference against the SAME rounded inputs in fp64), and out_scaled[m] = row_scale[m] * out[m] from the same accumulators."""
    from scdeepsort_amd import ops
    rng = np.random.default_rng(M * 7 + N + K)
    x = rng.standard_normal((M, K)).astype(np.float32); w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32); sc = (rng.random(M) + 0.5).astype(np.float32)
    xd = dev(x).half() if half_in else dev(x)
    out, out2 = ops.linear_fwd(xd, dev(w), dev(b), relu=True, row_scale=dev(sc))
    xin = xd.float().cpu().numpy().astype(np.float64)
    want = np.maximum(xin @ w.astype(np.float64).T + b, 0)
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=2e-5)
    np.testing.assert_allclose(out2.cpu().numpy(), want * sc[:, None], atol=3e-5)
    assert torch.equal(out2, out * dev(sc)[:, None])                       # the same fp32 product, bit for bit
    single = ops.linear_fwd(xd, dev(w), dev(b), relu=True)
    assert torch.equal(single, out)


@pytest.mark.parametrize("n_layers,seeded", [(2, False), (2, True), (1, True)])
def test_nograd_forward_through_wgnn_linear_and_prescaled_source(n_layers, seeded, monkeypatch):
    """The no-grad forward with the projections on wgnn_linear_fwd_ex (P_g and alpha * P_g from one kernel -> the tile kernel's
    WGNN_FLAG_SRC_PRESCALED, fp16-stored features widened in the loader) against the library-GEMM route and the oracle."""
    from scdeepsort_amd import ops
    c = small_case(cells=150, genes=80, dim=24, hidden=20, n_classes=5, seed=41, test_cells=12)
    sd = O.init_params(24, 20, 5, n_layers, 80, seed=2)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, 24, 20, 5, n_layers, 80)
    seeds = torch.arange(80 + 30, 80 + 150, device=DEV) if seeded else None
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    outs = {}
    for mode in ("never", "always"):
        monkeypatch.setattr(ops, "WGNN_LINEAR", mode)
        monkeypatch.setattr(ops, "WGNN_LINEAR_DUAL", mode == "always")
        with torch.no_grad():
            outs[mode] = m(g, dev(c["feats"]), seeds=seeds)
            outs[mode + "16"] = m(g, dev(c["feats"]).half(), seeds=seeds)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    ids = np.arange(80 + 30, 80 + 150) if seeded else np.arange(80, 80 + 150)
    want = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), ids, n_layers).numpy()
    want16 = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]).half().float(), ids, n_layers).numpy()
    for k in ("never", "always"):
        np.testing.assert_allclose(outs[k].cpu().numpy(), want, atol=TOL, err_msg=k)
        np.testing.assert_allclose(outs[k + "16"].cpu().numpy(), want16, atol=TOL, err_msg=k + "16")
    assert (outs["never"] - outs["always"]).abs().max().item() < 2e-5
    # training is untouched by the switch: gradients flow through the library GEMM + scale pass as before
    monkeypatch.setattr(ops, "WGNN_LINEAR", "always")
    m.train()
    out = m(g, dev(c["feats"]), seeds=seeds)
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_int64_row_pointers_at_the_kernel_boundary():
    """"rowptr[R+1] i32 or i64".  wgnn_normalize_rows_i64 and wgnn_agg_fwd / wgnn_agg_fwd_tiled with
    WGNN_FLAG_ROWPTR_I64 (the kernels read rowptr for the inv_deg == NULL fallback) give the int32 results bit for bit."""
    from scdeepsort_amd import _lib, ops
    from scdeepsort_amd.graph import _ptr, _stream
    c = small_case(cells=200, genes=90, dim=32, seed=23, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV, chunk=32)
    d = torch.device(DEV)
    csr = g.cg
    x = sp.csr_matrix(c["expr"]).astype(np.float32); x.sort_indices()
    rp64, raw = dev(x.indptr, torch.int64), dev(x.data)
    v64, inv64 = torch.empty_like(raw), torch.empty(csr.n_rows, device=DEV)
    assert _lib.call(d, "wgnn_normalize_rows_i64", _ptr(rp64), _ptr(raw), _ptr(v64), _ptr(inv64), csr.n_rows, _stream(d)) == 0
    assert torch.equal(v64, csr.val) and torch.equal(inv64, csr.inv_deg)
    alpha = torch.rand(92, device=DEV) + 0.5
    hg, hc = dev(c["feats"][:90]), dev(c["feats"][90:])
    want = sda.agg_fwd(csr, alpha, sda.SRC_IS_GENE, 91, hg, hc)
    plan = csr.plan
    part = torch.empty(max(1, plan.n_partials) * 32, device=DEV)

    def run(rowptr, flags):
        out = torch.empty(csr.n_rows, 32, device=DEV)
        rc = _lib.call(d, "wgnn_agg_fwd", _ptr(rowptr), _ptr(csr.col), _ptr(csr.val), _ptr(alpha), sda.SRC_IS_GENE, 91,
                       _ptr(hg), 32, _ptr(hc), 32, None, None, None, _ptr(out), 32, None, csr.n_rows, 32, 0, 0, flags,
                       _ptr(plan.items), plan.n_items, _ptr(plan.long_rows) if plan.n_long else None, plan.n_long,
                       _ptr(part), plan.n_partials, _stream(d))
        assert rc == 0
        return out
    a32, a64 = run(csr.rowptr, 0), run(rp64, _lib.FLAG_ROWPTR_I64)          # inv_deg = NULL: 1/(deg+1) from rowptr
    assert torch.equal(a32, a64) and torch.equal(a32, want)
    tp = csr.tile_plan(ops.tiled_block_rows(32))
    tpart = torch.empty(max(1, tp.n_partials) * 32, device=DEV)

    def run_tiled(rowptr, flags):
        out = torch.empty(csr.n_rows, 32, device=DEV); scratch = torch.empty_like(hg)
        nl = tp.long_rows.shape[0]
        rc = _lib.call(d, "wgnn_agg_fwd_tiled", _ptr(rowptr), _ptr(alpha), sda.SRC_IS_GENE, 91, _ptr(hg), 90, _ptr(scratch),
                       _ptr(hc), 32, None, None, None, _ptr(out), 32, None, csr.n_rows, 32, flags,
                       _ptr(tp.entries), _ptr(tp.seg_ptr), tp.nblk_max, tp.block_rows, _ptr(tp.items), _ptr(tp.hdr), tp.n_tiles,
                       _ptr(tp.long_rows) if nl else None, nl, _ptr(tpart), tp.n_partials, _stream(d))
        assert rc == 0
        return out
    t32, t64 = run_tiled(csr.rowptr, 0), run_tiled(rp64, _lib.FLAG_ROWPTR_I64)
    assert torch.equal(t32, t64) and (t32 - want).abs().max().item() < 2e-5


@pytest.mark.parametrize("n_layers", [1, 2])
def test_range_seeds_are_the_contiguous_test_cells_of_a_predict_graph(n_layers, monkeypatch):
    """`seeds=range(G + n_support, N)` (what api._predict passes, predict.py:64-76) == the same ids as a tensor == the
    oracle's NodeFlow on those seeds; on a tile-kernel operand the range takes the full pass + slice, below it the
    row-wave seed path."""
    from scdeepsort_amd import ops
    c = small_case(cells=140, genes=60, dim=20, hidden=12, n_classes=4, seed=51, test_cells=100)
    sd = O.init_params(20, 12, 4, n_layers, 60, seed=6)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, 20, 12, 4, n_layers, 60)
    rng_ids = range(60 + 40, 60 + 140)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    want = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), np.arange(100, 200), n_layers).numpy()
    x = dev(c["feats"])
    with torch.no_grad():
        small = m(g, x, seeds=rng_ids)                                   # below TILED_MIN_WORK: row-wave seed path
        monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
        big = m(g, x, seeds=rng_ids)                                     # full LDS-streamed pass, sliced
        as_tensor = m(g, x, seeds=torch.arange(100, 200, device=DEV))
    for got in (small, big, as_tensor):
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL)
    with pytest.raises(ValueError):
        m(g, x, seeds=range(10, 70))                                     # gene ids are not seeds


def test_subplan_with_pathologically_long_rows():
    """a row that needs more than 64 chunks of the plan's chunk length is cut into 64 EQUAL parts by the
    device-built seed plan (graph.AggCsr.subplan) - a different summation order than the full-graph plan, so the seed row
    equals its full-pass row to rounding (not bitwise), deterministically and independently of the batch it arrives in."""
    rng = np.random.default_rng(5)
    C, G, D = 40, 2000, 32
    dense = (rng.random((C, G)) < 0.02) * rng.uniform(0.5, 7.0, (C, G))
    dense[7, :1500] = rng.uniform(0.5, 7.0, 1500)                           # a cell expressing 1500 genes: 94 chunks of 16
    expr = sp.csr_matrix(dense.astype(np.float32))
    g = sda.CellGeneGraph.from_expression(expr, device=DEV, chunk=16)
    assert g.cg.max_row_nnz > 64 * g.cg.plan.chunk
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg, hc = dev(rng.standard_normal((G, D))), dev(rng.standard_normal((C, D)))
    full = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
    ids = torch.tensor([7, 3, 7, 20], device=DEV)
    a = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc, row_ids=ids)
    b = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc, row_ids=torch.tensor([20, 7], device=DEV))
    assert (a - full[ids]).abs().max().item() < 2e-5
    assert torch.equal(a[0], a[2]) and torch.equal(a[0], b[1]) and torch.equal(a[3], b[0])     # batch-independent
    cgo = O.build_csr_graph(expr)
    zc, _ = O.csr_aggregate(cgo, alpha.cpu().numpy(), hg.cpu().numpy().astype(np.float64), hc.cpu().numpy().astype(np.float64), want_genes=False)
    np.testing.assert_allclose(a.cpu().numpy(), zc[[7, 3, 7, 20]], atol=TOL)


# ---- dedicated loader waves of the flat tile kernel (round 3) --------------------------------------------------------
@pytest.mark.parametrize("kb", [16, 23, 78])
@pytest.mark.parametrize("D", [64, 200, 256])
@pytest.mark.parametrize("direction", ["cells", "genes"])
def test_tile_kernel_dedicated_loader_waves(kb, D, direction):
    """Dedicated loader waves: a plan built with n_loaders = L deals waves 0..L-1 of every tile no rows, and the kernel makes
    the leading row-less waves issue the whole global->LDS stream of the steady-state blocks.  Same results as the symmetric
    plan BIT FOR BIT with slot-sorted entries (the per-row summation order does not depend on which wave streams), equal to
    the oracle with and without shared pairs, for L = 1, 2, 3, 5; short LDS blocks (kb = 16 / 23) run the steady-state loop and every tail length, kb = 78 the production block
    height; a plan whose tiles do not fit 16 x (16 - L) rows falls back to L = 0."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops
    c = small_case(cells=1300, genes=620, dim=D, seed=kb + D, density=0.12, test_cells=40)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cgo = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(kb)
    alpha = dev(rng.uniform(0.5, 1.5, G + 2).astype(np.float32)); bias = dev(rng.standard_normal(D).astype(np.float32))
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cgo, alpha.cpu().numpy(), Hg.astype(np.float64), Hc.astype(np.float64))
    if direction == "cells":
        csr, mode, sidx, src, slf, want, geom = g.cg, sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), zc, (8, 1)     # 163 rows per tile
    else:
        csr, mode, sidx, src, slf, want, geom = g.gc, sda.DST_IS_GENE, G, dev(Hc), dev(Hg), zg, (4, 2)         # <= 208 virtual rows per tile
    want = np.maximum(want + bias.cpu().numpy(), 0)
    run = lambda tp: ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf, bias=bias, relu=True)
    from scdeepsort_amd import graph as GR
    was = GR.TILE_SHARED_PAIRS
    try:
        for pairs in (False, True):
            # slot-sorted entries: a row's summation order is its CSR order whatever the wave -> bit-identical across L;
            # shared pairs order a row's entries by what its wave-mates share with it -> equal to rounding
            GR.TILE_SHARED_PAIRS = pairs
            base_plan = build_tile_plan(csr, *geom, block_rows=kb, n_loaders=0)
            assert bool((base_plan.entries[:, 0] < 0).any()) == pairs
            base = run(base_plan)
            np.testing.assert_allclose(base.cpu().numpy(), want, atol=TOL)
            for L in (1, 2, 3, 5):
                tp = build_tile_plan(csr, *geom, block_rows=kb, n_loaders=L)
                assert tp.n_loaders == L
                slots = tp.items[:, :, 0].reshape(tp.n_tiles, 16, 16)                 # [tile, wave, row slot] -> row or -1
                assert (slots[:, :L] < 0).all() and (slots[:, L:] >= 0).any()         # the loader waves own no rows
                out = run(tp)
                if pairs:
                    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)
                else:
                    assert torch.equal(out, base), L
    finally:
        GR.TILE_SHARED_PAIRS = was
    crowded = build_tile_plan(csr, 6 if direction == "cells" else 3, geom[1], block_rows=kb, n_loaders=3)   # > 208 rows per tile
    assert crowded.n_loaders == 0
    np.testing.assert_allclose(run(crowded).cpu().numpy(), want, atol=TOL)


def test_plan_walk_kernel_builds_the_same_plans_as_the_framework_builder():
    """Round 5: `wgnn_tile_plan_count` / `wgnn_tile_plan_fill` (csrc/wgnn_plan.hip: one wavefront per (tile, wave) walks its rows
    in lock step, no sort) against the framework-arithmetic builder of rounds 1-4 on the same operands: identical segment
    boundaries, the same (row, column, weight) multiset per segment, the [unshared][pad][pairs] layout with its invariants,
    and the same forward through either plan - for both tile geometries, column splits, virtual rows of a hub gene, loader
    waves, a support-masked gene side and empty rows."""
    from scdeepsort_amd import ops, graph as GR
    c = small_case(cells=2300, genes=520, dim=64, seed=91, density=0.12, test_cells=60)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    G = c["G"]; rng = np.random.default_rng(4)
    alpha = dev(rng.uniform(0.5, 1.5, G + 2).astype(np.float32))
    Hg, Hc = dev(c["feats"][:G]), dev(c["feats"][G:])
    cases = [(g.cg, sda.SRC_IS_GENE, G + 1, Hg, Hc), (g.gc, sda.DST_IS_GENE, G, Hc, Hg)]
    for csr, mode, sidx, src, slf in cases:
        for geom, rt, cs, kb, L in ((GR.GEOM_FLAT, None, None, 64, 1), (GR.GEOM_FLAT, -(-csr.n_rows // 256), 3, 23, 0),
                                    (GR.GEOM_FLAT, 12, 1, 78, 2), (GR.GEOM_TALL, None, None, 64, 0), (GR.GEOM_TALL, 7, 2, 40, 0)):
            plans = {}
            for kern in (True, False):
                saved, GR.TILE_PLAN_KERNEL = GR.TILE_PLAN_KERNEL, kern
                try:
                    plans[kern] = GR.build_tile_plan(csr, rt, cs, block_rows=kb, n_loaders=L, geom=geom)
                finally:
                    GR.TILE_PLAN_KERNEL = saved
            a, b = plans[True], plans[False]
            assert torch.equal(a.items, b.items) and torch.equal(a.hdr, b.hdr) and a.n_loaders == b.n_loaders
            assert torch.equal(a.seg_ptr, b.seg_ptr), (geom, rt, cs, kb)
            assert a.entries.shape == b.entries.shape
            W, rpw = geom.waves, geom.rpw
            seg = a.seg_ptr.long(); n_seg = seg.shape[0] - 1
            per = seg[1:] - seg[:-1]
            sid = torch.repeat_interleave(torch.arange(n_seg, device=DEV), per)
            off = torch.arange(a.entries.shape[0], device=DEV) - seg[sid]

            def decode(tp):
                meta, wb = tp.entries[:, 0].long(), tp.entries[:, 1]
                slot, srcl = (meta >> 8) & 0x3F, meta & 0xFF
                paired, padded = meta < 0, (meta & GR.TILE_PAD_FLAG) != 0
                wave, blk, tile = sid % W, (sid // W) % tp.nblk_max, sid // (W * tp.nblk_max)
                slots = tp.items[:, :, 0].reshape(tp.n_tiles, W, rpw)
                row = slots[tile, wave, slot].long()
                col = tp.hdr[tile, 0].long() + blk * tp.block_rows + srcl
                key = (sid * (csr.n_rows + 1) + row) * (csr.n_cols + 1) + col          # (segment, row, column)
                keep = ~padded
                order = torch.argsort(key[keep])
                return key[keep][order], wb[keep][order], meta, paired, padded, slot, srcl
            ka, wa, meta, paired, padded, slot, srcl = decode(a)
            kb_, wb_, *_ = decode(b)
            assert torch.equal(ka, kb_) and torch.equal(wa, wb_)                        # same entries in every segment
            # layout invariants of the kernel-built plan
            assert (a.entries[:, 1][padded] == 0).all() and not (paired & padded).any()
            first = torch.nonzero(paired & (off % 2 == 0)).squeeze(1)
            assert first.numel() * 2 == int(paired.sum())
            assert paired[first + 1].all() and (sid[first + 1] == sid[first]).all() and (srcl[first + 1] == srcl[first]).all()
            assert (((meta[first] >> 16) & 0x3F) == slot[first + 1]).all()
            n_pair = torch.bincount(sid[paired], minlength=n_seg)
            assert (paired == (off >= (per - n_pair)[sid])).all() and ((per - n_pair)[n_pair > 0] % 2 == 0).all()
            n_pad = torch.bincount(sid[padded], minlength=n_seg)
            assert (per % 2 == 0).all() and (n_pad == (per - n_pad) % 2).all()          # ABI 0.2.5: odd segments padded to even
            pp = torch.nonzero(padded).squeeze(1)
            assert ((meta[pp] & 0xFFFF) == (meta[pp - 1] & 0xFFFF)).all()               # a zero-weight copy of the entry before it
            out_a = ops.agg_fwd_tiled(csr, a, alpha, mode, sidx, src, slf)
            out_b = ops.agg_fwd_tiled(csr, b, alpha, mode, sidx, src, slf)
            np.testing.assert_allclose(out_a.cpu().numpy(), out_b.cpu().numpy(), atol=2e-5, rtol=1e-5)
    assert GR.TILE_PLAN_KERNEL                                                          # the kernel is the default on the GPU


@pytest.mark.parametrize("D", [64, 200, 256])
def test_tall_tile_kernel_matches_the_oracle_and_the_flat_kernel(D):
    """Round 5: agg_tiled_tall - the entry pipeline on 8 waves x 256 VGPRs, 49 destination rows per wave (`graph.GEOM_TALL`,
    plan bit WGNN_PLAN_TALL; opt-in through `graph.TILE_TALL`, see there for why).  Forward in both directions with explicit and
    heuristic geometries, column splits, several LDS block heights incl. segments of more than four chunks (the on-demand chunk
    path), D = 200 (global rows shorter than their LDS slots: the one-piece DMA form) - against the oracle; and the backward
    entries K2t / K3t with TILE_TALL = "on" against the row-wave kernels.
    The row-wave kernels themselves are pinned to fp64 in tests/test_gpu_backward_ops.py."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops, graph as GR
    c = small_case(cells=1900, genes=420, dim=D, seed=D + 5, density=0.3, test_cells=40)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cgo = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(D)
    alpha = dev(rng.uniform(0.5, 1.5, G + 2).astype(np.float32))
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cgo, alpha.cpu().numpy(), Hg.astype(np.float64), Hc.astype(np.float64))
    for csr, mode, sidx, src, slf, want in ((g.cg, sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), zc),
                                            (g.gc, sda.DST_IS_GENE, G, dev(Hc), dev(Hg), zg)):
        for rt, cs, kb in ((None, None, 78), (-(-csr.n_rows // 392), 1, 78), (7, 2, 23), (5, 3, 64)):
            if kb > ops.tiled_block_rows(D):
                kb = ops.tiled_block_rows(D)
            tp = build_tile_plan(csr, rt, cs, block_rows=kb, geom=GR.GEOM_TALL)
            assert tp.geom.tall and tp.items.shape[1] == 392 and tp.n_loaders == 0
            seg = tp.seg_ptr.long()
            if rt is not None and cs == 1 and kb >= 64:
                assert int((seg[1:] - seg[:-1]).max()) > 256                      # more than four chunks in one (wave, block)
            out = ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf)
            np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL, rtol=1e-5)
            assert torch.equal(ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf), out)      # deterministic
            flat = ops.agg_fwd_tiled(csr, build_tile_plan(csr, None, None, block_rows=kb, n_loaders=1), alpha, mode, sidx, src, slf)
            np.testing.assert_allclose(out.cpu().numpy(), flat.cpu().numpy(), atol=2e-5, rtol=1e-5)
    # backward entries over tall plans (dispatch forced to the tile kernels, TILE_TALL = "on") against the row-wave kernels
    gen = torch.Generator(device=DEV).manual_seed(D)
    gc_ = torch.randn(g.cg.n_rows, D, generator=gen, device=DEV); gg_ = torch.randn(g.gc.n_rows, D, generator=gen, device=DEV)
    hg_, hc_ = dev(Hg), dev(Hc)
    def grads():
        da = torch.zeros(G + 2, device=DEV)
        dh_g = ops.agg_bwd_src(g.cg, alpha, sda.SRC_IS_GENE, gc_, hg_, dalpha=da)
        dh_c = ops.agg_bwd_src(g.gc, alpha, sda.DST_IS_GENE, gg_, hc_)
        k3 = ops.agg_bwd_alpha(g.gc, gg_, hc_, hg_)
        return [dh_g, dh_c, da] + [t for t in k3 if t is not None]
    saved = (ops.TILED_MIN_WORK, GR.TILE_TALL)
    try:
        ops.TILED_MIN_WORK = None
        ref = grads()
        ops.TILED_MIN_WORK, GR.TILE_TALL = 0, "on"
        for csr in (g.cg, g.gc):
            csr._tile_plan = None
            if csr._t is not None:
                csr._t._tile_plan = None
        got = grads()
        assert g.cg.transposed().tile_plan(ops.tiled_block_rows(D)).geom.tall
    finally:
        ops.TILED_MIN_WORK, GR.TILE_TALL = saved
        for csr in (g.cg, g.gc):
            csr._tile_plan = None
            if csr._t is not None:
                csr._t._tile_plan = None
    for a_, b_ in zip(got, ref):
        np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), atol=2e-4 * max(1.0, float(b_.abs().max())), rtol=1e-4)


@pytest.mark.parametrize("density", [0.01, 0.08, 0.5, 0.95])
@pytest.mark.parametrize("D", [64, 256])
def test_tile_kernel_shared_pairs(density, D):
    """Shared pairs of agg_tiled_flat4 (graph._pair_segment_entries): entries of a (wave, block) segment on the same source
    row are consumed two per LDS read by the pipeline's second stream.  Densities from "no pair in most segments" to "every
    entry paired, ~15 chunks of 64 per segment" (the multi-chunk loop, chunks that are all pairs, pads after an odd
    unshared run), both directions, against the oracle; the slot-sorted plan of the same graph must agree to rounding, and
    the generic tile kernel (entry order free) reads the same paired plan."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops, graph as GR
    c = small_case(cells=700, genes=330, dim=D, seed=int(density * 100) + D, density=density, test_cells=30)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cgo = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(D)
    alpha = dev(rng.uniform(0.5, 1.5, G + 2).astype(np.float32))
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cgo, alpha.cpu().numpy(), Hg.astype(np.float64), Hc.astype(np.float64))
    was = GR.TILE_SHARED_PAIRS
    try:
        for csr, mode, sidx, src, slf, want, geom in ((g.cg, sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), zc, (4, 1)),
                                                       (g.gc, sda.DST_IS_GENE, G, dev(Hc), dev(Hg), zg, (2, 3))):
            outs = {}
            for pairs in (False, True):
                GR.TILE_SHARED_PAIRS = pairs
                for kb, L in ((78, 1), (23, 0), (64, 2)):
                    tp = build_tile_plan(csr, *geom, block_rows=kb, n_loaders=L)
                    meta = tp.entries[:, 0]
                    if not pairs:
                        assert not (meta < 0).any()
                    elif density >= 0.5:
                        assert float((meta < 0).float().mean()) > 0.5
                        seg = tp.seg_ptr.long()
                        if kb == 78:
                            assert int((seg[1:] - seg[:-1]).max()) > 64            # more than one chunk of 64 per segment
                    out = ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf)
                    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL, rtol=1e-5)
                    outs[(pairs, kb)] = out
                    if pairs and kb == 78:
                        ops.DEBUG_FLAGS = 1 << 19                                   # the generic tile kernel
                        try:
                            gen = ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf)
                        finally:
                            ops.DEBUG_FLAGS = 0
                        np.testing.assert_allclose(gen.cpu().numpy(), want, atol=TOL, rtol=1e-5)
                        again = ops.agg_fwd_tiled(csr, tp, alpha, mode, sidx, src, slf)
                        assert torch.equal(again, out)                             # deterministic
            for kb in (78, 23, 64):
                np.testing.assert_allclose(outs[(True, kb)].cpu().numpy(), outs[(False, kb)].cpu().numpy(), atol=2e-5, rtol=1e-5)
    finally:
        GR.TILE_SHARED_PAIRS = was


def test_linear_act_fused_epilogue_and_last_layer_order():
    """ops.linear_act: act(x W^T + b) with bias + ReLU in the library GEMM's epilogue when nothing is differentiated - against
    fp64, with and without grad mode.  GNN "auto" order: at equal widths the LAST layer aggregates first (the reference's
    literal order, one projection less); forcing either order gives the same logits to rounding and the oracle's."""
    from scdeepsort_amd import ops
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3000, 256)).astype(np.float32); W = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32)
    want = np.maximum(x.astype(np.float64) @ W.astype(np.float64).T + b, 0)
    with torch.no_grad():
        got = ops.linear_act(dev(x), dev(W), dev(b), True)
        lin = ops.linear_act(dev(x), dev(W), dev(b), False)
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=2e-5)
    np.testing.assert_allclose(lin.cpu().numpy(), x.astype(np.float64) @ W.astype(np.float64).T + b, atol=2e-5)
    xg = dev(x).requires_grad_(True)
    np.testing.assert_allclose(ops.linear_act(xg, dev(W), dev(b), True).detach().cpu().numpy(), want, atol=2e-5)
    c = small_case(cells=500, genes=260, dim=40, hidden=32, n_layers=2, seed=21)
    sd = O.init_params(40, 32, 5, 2, c["G"], seed=3)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    want_logits = O.csr_forward(sd, O.build_csr_graph(c["expr"], c["support_mask"]), c["feats"], 2)
    outs = {}
    with torch.no_grad():
        for order in ("auto", "project_first", "aggregate_first"):
            outs[order] = make_model(sd, 40, 32, 5, 2, c["G"], order)(g, dev(c["feats"])).cpu().numpy()
            np.testing.assert_allclose(outs[order], want_logits, atol=TOL)
    np.testing.assert_allclose(outs["auto"], outs["project_first"], atol=2e-5)
    np.testing.assert_allclose(outs["auto"], outs["aggregate_first"], atol=2e-5)


@pytest.mark.parametrize("route", ["row_wave", "tiled", "tiled_split"])
def test_gene_rows_written_alpha_folded(route, monkeypatch):
    """WGNN_FLAG_OUT_SCALE_ALPHA (round 4): a genes<-cells pass writes alpha[g] * act(mean + bias) - the next layer's
    (h*alpha) source table of gnn.py:54 - from the row-wave epilogue, the tile kernel's two-row epilogue and agg_finalize
    (rows cut into column splits / virtual rows)."""
    from scdeepsort_amd import ops, graph as GR
    c = small_case(cells=400, genes=120, dim=64, seed=77, density=0.3)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(5)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32); bias = rng.standard_normal(64).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    _, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    want = np.maximum(zg + bias, 0) * alpha[:G, None]
    if route == "row_wave":
        monkeypatch.setattr(ops, "TILED_MIN_WORK", None)
        out = sda.agg_fwd(g.gc, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg), bias=dev(bias), relu=True, out_scale_alpha=True)
    else:
        tp = GR.build_tile_plan(g.gc, None if route == "tiled" else 2, 1 if route == "tiled" else 3, block_rows=16)
        assert tp.n_col_splits == (3 if route == "tiled_split" else 1) and (tp.n_partials > 0 or route == "tiled")
        out = ops.agg_fwd_tiled(g.gc, tp, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg), bias=dev(bias), relu=True,
                                out_scale_alpha=True)
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)
    with pytest.raises(sda.WgnnError):                       # defined for gene rows only
        sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), out_scale_alpha=True)


@pytest.mark.parametrize("seeded", [False, True])
def test_nograd_forward_folds_alpha_into_the_gene_rows_below_the_last_layer(seeded, monkeypatch):
    """2-layer no-grad forward on the LDS-streamed route: layer 1's gene pass writes its rows alpha-folded and layer 2's
    cells<-genes pass reads them as WGNN_FLAG_SRC_PRESCALED (no scale launch) - equal to the unfused forward and the
    oracle; with grad enabled, with a small seed batch (row-wave route) or a project-first last layer nothing is folded."""
    from scdeepsort_amd import ops
    c = small_case(cells=220, genes=90, dim=40, hidden=24, n_classes=5, seed=43, test_cells=15)
    sd = O.init_params(40, 24, 5, 2, 90, seed=3)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, 40, 24, 5, 2, 90)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    seeds = torch.arange(90 + 20, 90 + 220, device=DEV) if seeded else None
    calls = []
    real = ops.agg_fwd_tiled
    def spy(csr, tplan, alpha, mode, self_idx, h_src, h_self, **kw):
        calls.append((mode, bool(kw.get("out_scale_alpha")), kw.get("src_scaled") is not None))
        return real(csr, tplan, alpha, mode, self_idx, h_src, h_self, **kw)
    monkeypatch.setattr(ops, "agg_fwd_tiled", spy)
    with torch.no_grad():
        folded = m(g, dev(c["feats"]), seeds=seeds)
    assert (sda.DST_IS_GENE, True, False) in calls and (sda.SRC_IS_GENE, False, True) in calls, calls
    calls.clear()
    m.fold_alpha = False
    with torch.no_grad():
        plain = m(g, dev(c["feats"]), seeds=seeds)
    assert not any(c_[1] or c_[2] for c_ in calls), calls
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    ids = np.arange(90 + 20, 90 + 220) if seeded else np.arange(90, 90 + 220)
    want = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), ids, 2).numpy()
    np.testing.assert_allclose(folded.cpu().numpy(), want, atol=TOL)
    np.testing.assert_allclose(plain.cpu().numpy(), want, atol=TOL)
    assert (folded - plain).abs().max().item() < 2e-6
    # not folded: training (autograd must see alpha), a small seed batch (row-wave kernel folds alpha per edge itself),
    # a project-first last layer (it projects the UNSCALED gene rows)
    m.fold_alpha = True
    for kw, setup in (({"seeds": seeds}, "grad"), ({"seeds": torch.arange(90, 95, device=DEV)}, "small"), ({"seeds": seeds}, "pf")):
        calls.clear()
        m.order = "project_first" if setup == "pf" else "auto"
        if setup == "grad":
            out = m(g, dev(c["feats"]), **kw)
        else:
            with torch.no_grad():
                out = m(g, dev(c["feats"]), **kw)
        assert not any(c_[1] for c_ in calls), (setup, calls)
        assert torch.isfinite(out).all()
    m.order = "auto"


def test_sharded_branch_folds_alpha_in_genes_finish(monkeypatch):
    """The sharded branch (one shard holding every cell, no process group: the collectives are skipped, everything else is
    the N > 1 path) on the LDS-streamed route: `genes_finish` writes the all-reduced gene rows alpha-folded and the last
    layer's cells<-genes pass reads them pre-scaled - equal to the plain forward; off on the row-wave route."""
    from scdeepsort_amd import ops, synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    G, C, Din, H = 200, 700, 40, 32
    rp, col, val = S.synth_expression(C, G, 0.1, device=DEV)
    torch.manual_seed(2)
    m = sda.GNN(Din, H, 5, 2, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, Din, device=DEV)
    with torch.no_grad():
        want = m(sda.CellGeneGraph.from_device_csr(rp, col, val, G), feats)
    eng = ShardedWgnn.build(m, rp, col, val, G, global_stats=ShardedWgnn.gene_stats(col, val, G))
    assert eng.world == 2
    seen = []
    real = ops.agg_fwd
    def spy(csr, alpha, mode, self_idx, h_src, h_self, **kw):
        seen.append((mode, bool(kw.get("out_scale_alpha")), kw.get("src_scaled") is not None))
        return real(csr, alpha, mode, self_idx, h_src, h_self, **kw)
    import scdeepsort_amd.sharded as SH
    monkeypatch.setattr(SH, "agg_fwd", spy); monkeypatch.setattr(ops, "agg_fwd", spy)
    for tiled in (True, False):
        monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if tiled else None)
        seen.clear()
        with torch.no_grad():
            got = eng.forward(feats[:G], feats[G:], gather_logits=False)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=2e-5)
        assert ((sda.DST_IS_GENE, True, False) in seen) == tiled, seen          # genes_finish(scale_out=True)
        assert ((sda.SRC_IS_GENE, False, True) in seen) == tiled, seen          # last layer reads the folded rows


@pytest.mark.parametrize("D", [32, 64, 100, 128, 132, 192, 200, 256])
@pytest.mark.parametrize("direction", ["cells", "genes"])
def test_tile_kernel_packed_lds_rows_at_full_block_height(D, direction):
    """Round 4: the flat tile kernel's LDS rows are 256 / 512 / 1024 bytes by width (512 B at D = 128 instead of a 1 KiB slot),
    and `ops.tiled_block_rows(D)` fills the 160 KiB of a CU with them: 255 / 156 / 78 source rows per block.  Every
    stride at its full block height (several blocks per tile, column splits, loader wave, shared pairs), forward and the
    two backward entries, against the oracle / the row-wave kernels.
    The row-wave kernels themselves are pinned to fp64 in tests/test_gpu_backward_ops.py."""
    from scdeepsort_amd.graph import build_tile_plan
    from scdeepsort_amd import ops
    kb = ops.tiled_block_rows(D)
    assert kb == {256: 255, 512: 156, 1024: 78}[ops.flat_lds_row_bytes(D)]
    assert 2 * kb * ops.flat_lds_row_bytes(D) + 4096 <= 160 * 1024
    c = small_case(cells=900, genes=640, dim=D, seed=D + 3, density=0.2, test_cells=40)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]; rng = np.random.default_rng(9)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32); bias = rng.standard_normal(D).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    ops.PROFILE = []
    for geom in ((None, 1), (3, 2)):
        if direction == "cells":
            tp = build_tile_plan(g.cg, *geom, block_rows=kb, n_loaders=1)
            out = ops.agg_fwd_tiled(g.cg, tp, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(Hg), dev(Hc), bias=dev(bias), relu=True)
            want = np.maximum(zc + bias, 0)
        else:
            tp = build_tile_plan(g.gc, *geom, block_rows=kb, n_loaders=1)
            out = ops.agg_fwd_tiled(g.gc, tp, dev(alpha), sda.DST_IS_GENE, G, dev(Hc), dev(Hg), bias=dev(bias), relu=True)
            want = np.maximum(zg + bias, 0)
        assert tp.block_rows == kb and tp.nblk_max >= (2 if geom[1] == 1 else 1)
        np.testing.assert_allclose(out.cpu().numpy(), want, atol=TOL)
    assert {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE} == {"agg_tiled_flat4"}
    ops.PROFILE = None
    # backward entries K2t / K3t on the same block height against the row-wave K2 / K3
    csr = g.cg if direction == "cells" else g.gc
    mode = sda.SRC_IS_GENE if direction == "cells" else sda.DST_IS_GENE
    gr = dev(rng.standard_normal((csr.n_rows, D)).astype(np.float32))
    h_src = dev(Hg if direction == "cells" else Hc)
    saved = ops.TILED_MIN_WORK
    try:
        res = {}
        for thr in (None, 1):
            ops.TILED_MIN_WORK = thr
            dal = torch.zeros(G + 2, device=DEV)
            dh = ops.agg_bwd_src(csr, dev(alpha), mode, gr, h_src if direction == "cells" else None, dal if direction == "cells" else None)
            res[thr] = (dh.clone(), dal.clone())
            if direction == "genes":
                res[thr] += ops.agg_bwd_alpha(csr, gr, h_src, dev(Hg))
    finally:
        ops.TILED_MIN_WORK = saved
    for a_, b_ in zip(res[None], res[1]):
        np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("n,c", [(1, 2), (7, 5), (1000, 16), (100_003, 16), (513, 33)])
def test_cross_entropy_sum_kernel_matches_torch(n, c):
    """`ops.cross_entropy_sum` = CrossEntropyLoss(reduction='sum') (train.py:36): loss and dloss/dlogits from one read of the
    logits (wgnn_ce_sum_fwd_bwd), against torch in fp64; deterministic run to run."""
    from scdeepsort_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(n + c)
    x = (3.0 * torch.randn(n, c, generator=gen, device=DEV)).requires_grad_(True)
    y = torch.randint(0, c, (n,), generator=gen, device=DEV)
    loss = ops.cross_entropy_sum(x, y)
    (2.0 * loss).backward()
    x64 = x.detach().double().requires_grad_(True)
    ref = F.cross_entropy(x64, y, reduction="sum")
    (2.0 * ref).backward()
    assert abs(loss.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item())) * max(1.0, n ** 0.5 / 30)
    np.testing.assert_allclose(x.grad.cpu().numpy(), x64.grad.cpu().numpy(), atol=2e-6)
    assert ops.cross_entropy_sum(x.detach(), y).item() == ops.cross_entropy_sum(x.detach(), y).item()
    assert ops.cross_entropy_sum(x[:0], y[:0]).item() == 0.0
    # a label outside [0, c) is never used as an index: NaN loss, NaN gradient row, the other rows untouched
    bad = y.clone(); bad[n // 2] = c + 5; bad[0] = -1
    xb = x.detach().clone().requires_grad_(True)
    lb = ops.cross_entropy_sum(xb, bad)
    lb.backward()
    assert torch.isnan(lb).item() and torch.isnan(xb.grad[n // 2]).all() and torch.isnan(xb.grad[0]).all()
    keep = torch.ones(n, dtype=torch.bool, device=DEV); keep[n // 2] = False; keep[0] = False
    if keep.any():
        np.testing.assert_allclose(xb.grad[keep].cpu().numpy(), 0.5 * x.grad[keep].cpu().numpy(), atol=2e-6)
    # a label >= 2^32 must not alias a valid class; -100 is torch's ignore_index (loss 0, zero gradient row)
    big = y.clone(); big[0] = (1 << 32) + 1
    assert torch.isnan(ops.cross_entropy_sum(x.detach(), big)).item()
    ign = y.clone(); ign[0] = -100
    xi = x.detach().clone().requires_grad_(True)
    li = ops.cross_entropy_sum(xi, ign)
    li.backward()
    xi64 = x.detach().double().requires_grad_(True)
    ri = F.cross_entropy(xi64, ign, reduction="sum")
    ri.backward()
    assert abs(li.item() - ri.item()) < 2e-6 * max(1.0, abs(ri.item())) * max(1.0, n ** 0.5 / 30)
    assert (xi.grad[0] == 0).all()
    np.testing.assert_allclose(xi.grad.cpu().numpy(), xi64.grad.cpu().numpy(), atol=2e-6)


@pytest.mark.parametrize("mode", ["cells", "genes", "plain"])
@pytest.mark.parametrize("D", [4, 64, 200, 256, 400])
def test_agg_bwd_prepare_matches_the_framework_glue(mode, D):
    """wgnn_agg_bwd_prepare: ReLU mask, K2t's pre-scaled source rows, the self-row gradient, the alpha row dots and the bias
    gradient from ONE read of the upstream gradient - each output against the torch expression it replaces."""
    from scdeepsort_amd import ops
    R = 777
    gen = torch.Generator(device=DEV).manual_seed(D)
    gout = torch.randn(R, D, generator=gen, device=DEV); out = torch.randn(R, D, generator=gen, device=DEV)
    hs = torch.randn(R, D, generator=gen, device=DEV); ns = torch.randn(R, D, generator=gen, device=DEV)
    invd = torch.rand(R, generator=gen, device=DEV) + 0.1
    alpha = torch.rand(R + 2, generator=gen, device=DEV) + 0.5
    m = {"cells": sda.SRC_IS_GENE, "genes": sda.DST_IS_GENE, "plain": sda.NO_ALPHA}[mode]
    self_idx = R + 1 if mode == "cells" else R
    for relu in (True, False):
        res = ops.agg_bwd_prepare(gout, out if relu else None, invd, None if mode == "plain" else alpha, m, self_idx,
                                  want_scaled=True, h_self=hs, want_dh_self=True, neigh_sum=ns if mode == "genes" else None,
                                  want_dself=mode != "plain", want_dbias=True)
        g = (gout * (out > 0)) if relu else gout
        f = invd * (alpha[:R] if mode == "genes" else 1.0)
        a_self = 1.0 if mode == "plain" else alpha[self_idx]
        np.testing.assert_allclose(res["g_scaled"].cpu().numpy(), (g * f[:, None]).cpu().numpy(), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(res["dh_self"].cpu().numpy(), (g * (a_self * invd)[:, None]).cpu().numpy(), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(res["dbias"].cpu().numpy(), g.double().sum(0).cpu().numpy(), rtol=1e-5, atol=2e-4)
        if mode == "genes":
            np.testing.assert_allclose(res["dalpha_row"].cpu().numpy(), ((g.double() * ns.double()).sum(1) * invd).cpu().numpy(), rtol=1e-5, atol=1e-4)
        else:
            assert res["dalpha_row"] is None
        if mode != "plain":
            np.testing.assert_allclose(res["dself_row"].cpu().numpy(), ((g.double() * hs.double()).sum(1) * invd).cpu().numpy(), rtol=1e-5, atol=1e-4)
    only = ops.agg_bwd_prepare(gout, None, None, None, sda.NO_ALPHA, 0, want_scaled=True)       # nothing optional: a copy
    assert torch.equal(only["g_scaled"], gout) and all(only[k] is None for k in ("dh_self", "dalpha_row", "dself_row", "dbias"))


@pytest.mark.parametrize("order", ["auto", "project_first", "aggregate_first"])
def test_fused_backward_glue_gives_the_same_gradients(order, monkeypatch):
    """Full-batch training step on the LDS-streamed route with the round-4 glue (one wgnn_agg_bwd_prepare launch per pass,
    K2t on pre-scaled rows, fused CE) against the framework glue of before and the autograd oracle."""
    from scdeepsort_amd import ops
    c = small_case(cells=150, genes=70, dim=24, hidden=20, n_classes=4, seed=21, test_cells=0)
    sd = O.init_params(24, 20, 4, 2, 70, seed=8)
    rg = O.build_reference_graph(c["expr"])
    seeds = np.arange(70, 70 + 150)
    labels = torch.arange(150) % 4
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), seeds, labels, 2)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSED_BWD_GLUE", fused)
        calls = []
        real = ops.agg_bwd_prepare
        monkeypatch.setattr(ops, "agg_bwd_prepare", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        m = make_model(sd, 24, 20, 4, 2, 70, order)
        logits = m(g, dev(c["feats"]))
        l = ops.cross_entropy_sum(logits, labels.to(DEV)) if fused else F.cross_entropy(logits, labels.to(DEV), reduction="sum")
        l.backward()
        monkeypatch.setattr(ops, "agg_bwd_prepare", real)
        assert (len(calls) == 3) == fused, calls                     # L2 cells, L1 cells, L1 genes
        assert l.item() == pytest.approx(float(loss), rel=1e-5)
        got[fused] = {k: p.grad.clone() for k, p in m.named_parameters()}
        for k, p in m.named_parameters():
            np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=f"{k} fused={fused}")
    for k in got[True]:
        assert (got[True][k] - got[False][k]).abs().max().item() < 2e-5 * max(1.0, got[False][k].abs().max().item()), k


def test_full_size_properties_cfg5():
    """BASELINE cfg5 at FULL size on one GPU (764,741 cells x 20,000 genes, ~6.1e8 non-zeros per direction - 28 % of the
    2^31 offset range the plans index with -, fp16-STORED features): the 13-round tile geometry of the cells side and the
    one-round column-split geometry of the gene side, driver-verified.  Size-independent properties of both passes
    (linearity, determinism, a row sample against the row-wave kernel, hipSPARSE cross-check, the constant-feature
    checksum), then the whole 2-layer forward on fp16-stored features against the same forward on their fp32 copies."""
    from scdeepsort_amd import ops, synthetic as S
    cfg = S.CONFIGS["cfg5"]
    G, C, H = cfg.genes, cfg.cells, cfg.hidden
    rp, col, val = S.synth_expression(C, G, cfg.density, device=DEV)
    nnz = int(col.shape[0])
    assert 5.5e8 < nnz < 2 ** 31
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    del rp, col, val
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg1, hc1 = S.synth_features(G, H, device=DEV), S.synth_features(C, H, seed=3, device=DEV)
    hg2, hc2 = S.synth_features(G, H, seed=5, device=DEV), S.synth_features(C, H, seed=6, device=DEV)
    ops.PROFILE = []
    f = lambda a, b: sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, a, b)
    fg = lambda a, b: sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, G, b, a)
    z1, z2, z3 = f(hg1, hc1), f(hg2, hc2), f(2 * hg1 - 0.5 * hg2, 2 * hc1 - 0.5 * hc2)
    y1, y2, y3 = fg(hg1, hc1), fg(hg2, hc2), fg(2 * hg1 - 0.5 * hg2, 2 * hc1 - 0.5 * hc2)
    kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
    ops.PROFILE = None
    assert kernels == {"agg_tiled_flat4"}
    tpc, tpg = list(g.cg._tile_plan.values())[0], list(g.gc._tile_plan.values())[0]
    assert tpc.n_col_splits == 1 and tpc.n_row_tiles >= 12 * 256 and tpc.n_loaders == 1        # 13-14 rounds of <= 240-row tiles
    assert tpg.n_row_tiles * tpg.n_col_splits <= 256 and tpg.n_col_splits >= 2 and tpg.n_partials > 0
    assert int(tpc.entries.shape[0]) >= nnz and int(tpc.seg_ptr[-1]) == int(tpc.entries.shape[0])
    assert (2 * z1 - 0.5 * z2 - z3).abs().max().item() < 1e-4
    assert (2 * y1 - 0.5 * y2 - y3).abs().max().item() < 1e-4
    del z2, z3, y2, y3, hg2, hc2
    assert torch.equal(z1, f(hg1, hc1)) and torch.equal(y1, fg(hg1, hc1))          # deterministic (no atomics)
    ids = torch.randperm(C, device=DEV)[:1000]
    sub = sda.agg_fwd(g.cg, alpha, sda.SRC_IS_GENE, G + 1, hg1, hc1, row_ids=ids)    # row-wave kernel (K1)
    assert (sub - z1[ids]).abs().max().item() < 1e-4
    gids = torch.randperm(G, device=DEV)[:200]
    subg = sda.agg_fwd(g.gc, alpha, sda.DST_IS_GENE, G, hc1, hg1, row_ids=gids)
    assert (subg - y1[gids]).abs().max().item() < 1e-4
    # independent formulation: torch's CSR SpMM (hipSPARSE) over the whole operand, compared on a row sample
    A_cg = torch.sparse_csr_tensor(g.cg.rowptr.long(), g.cg.col.long(), g.cg.val, size=(C, G))
    ref_c = (torch.sparse.mm(A_cg, alpha[:G, None] * hg1) + alpha[G + 1] * hc1) * g.cg.inv_deg[:, None]
    samp = torch.randperm(C, device=DEV)[:50_000]
    assert (ref_c[samp] - z1[samp]).abs().max().item() < 1e-4
    del A_cg, ref_c
    # checksum of checksums: constant features
    ones_g, ones_c = torch.ones(G, H, device=DEV), torch.ones(C, H, device=DEV)
    zc, zg = f(ones_g, ones_c), fg(ones_g, ones_c)
    del ones_g, ones_c
    a64 = alpha.double()
    row_c = torch.repeat_interleave(torch.arange(C, device=DEV), (g.cg.rowptr[1:] - g.cg.rowptr[:-1]).long())
    want_c = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, row_c, g.cg.val.double() * a64[g.cg.col.long()])
    want_c = (want_c + a64[G + 1]) * g.cg.inv_deg.double()
    assert (zc.double() - want_c[:, None]).abs().max().item() < 1e-4
    del row_c, want_c, zc
    row_g = torch.repeat_interleave(torch.arange(G, device=DEV), (g.gc.rowptr[1:] - g.gc.rowptr[:-1]).long())
    want_g = torch.zeros(G, dtype=torch.float64, device=DEV).index_add_(0, row_g, g.gc.val.double())
    want_g = (a64[:G] * want_g + a64[G]) * g.gc.inv_deg.double()
    assert (zg.double() - want_g[:, None]).abs().max().item() < 2e-4
    del row_g, want_g, zg, z1, y1, hg1, hc1
    # the bench's cfg5 forward: fp16-STORED [G + C, 400] features widened inside the projection kernel's loader (fp16-rounded
    # inputs, fp32 multiply-accumulate) == the same model on the fp32 copy of those rounded features
    torch.manual_seed(5)
    m = sda.GNN(cfg.dense_dim, H, cfg.n_classes, 2, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
        feats16 = S.synth_features(G + C, cfg.dense_dim, device=DEV, dtype=torch.float16)
        out16 = m(g, feats16)
        out32 = m(g, feats16.float())
    assert out16.shape == (C, cfg.n_classes) and torch.isfinite(out16).all()
    assert (out16 - out32).abs().max().item() < 1e-4


def test_full_size_cfg5_sharded_eight_ways_matches_unsharded():
    """BASELINE cfg5 as the job it names - 764,741 cells sharded 8-way (~95.6k cells, ~7.6e7 non-zeros per rank), fp16-stored
    features - on one GPU: every rank's partial gene sums are computed through its own `ShardedWgnn` engine (gene side normalised
    with the GLOBAL statistics) and added where RCCL would all-reduce them; ranks 0 and 7 then run the production
    `dist.sharded_forward` (overlapped-pass geometry, alpha-folded gene rows, aggregate-first last layer) on that sum, and their
    logits must equal their rows of the UNSHARDED forward of the whole graph."""
    import dataclasses
    from scdeepsort_amd import dist as D, ops, synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    cfg = S.CONFIGS["cfg5"]
    G, C, H, N = cfg.genes, cfg.cells, cfg.hidden, 8
    rp, col, val = S.synth_expression(C, G, cfg.density, device=DEV)
    torch.manual_seed(5)
    m = sda.GNN(cfg.dense_dim, H, cfg.n_classes, 2, G, activation=F.relu).to(DEV).eval()
    feats = S.synth_features(G + C, cfg.dense_dim, device=DEV, dtype=torch.float16)
    feats_g, feats_c = feats[:G], feats[G:]
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
        g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
        want = m(g, feats)
        del g
        stats = ShardedWgnn.gene_stats(col, val, G)
        W1 = m.layers[0].fc_neigh.weight

        def shard(r):
            lo, hi = D.shard_range(C, r, N)
            b, e = int(rp[lo]), int(rp[hi])
            eng = ShardedWgnn.build(m, (rp[lo:hi + 1] - rp[lo]).clone(), col[b:e].clone(), val[b:e].clone(), G, global_stats=stats)
            assert eng.world > 1 and eng.overlap_cu_budget == 224
            return lo, hi, eng

        total = torch.zeros(G, H, device=DEV)
        for r in range(N):                                   # <- what the [G, H] all-reduce adds up
            lo, hi, eng = shard(r)
            total += eng._ops().genes_partial(ops.linear(feats_c[lo:hi], W1))
            del eng
        worst = 0.0
        for r in (0, N - 1):
            lo, hi, eng = shard(r)
            lops = dataclasses.replace(eng._ops(), genes_partial=lambda p_c: total.clone())
            assert lops.overlapped is not None and lops.fold_alpha_ok(H, None)
            got = D.sharded_forward(eng._weights(), None, feats_g, feats_c[lo:hi], lops, 2, gather_logits=False, linear=ops.linear)
            assert got.shape == (hi - lo, cfg.n_classes)
            worst = max(worst, (got - want[lo:hi]).abs().max().item())
            tp = [k for k in eng.graph.cg._tile_plan]        # both geometries of the cells side were used: overlapped pass, last layer
            assert {k[3] for k in tp} == {224, 256}             # key = (block rows, loaders, pairs, CU budget, geometry)
            del eng
    assert worst < 1e-4, worst


def test_fallen_back_dense_paths_give_the_same_results(monkeypatch):
    """the stack-coupled fast paths of the dense half - `torch._addmm_activation` (a private entry point: bias
    + ReLU in the GEMM epilogue, no-grad and training), the tracked TunableOp picks (not loaded in this process), hipBLASLt as
    preferred BLAS - each fall back to a plain composition.  Here the fallen-back state is EXERCISED where it would be used: the
    forward and a training step with `_addmm_activation` absent and with it raising, against the same model with it present
    and against the oracle."""
    from scdeepsort_amd import ops, tuning
    assert not tuning.active()                                  # this process never loaded the picks: library heuristics
    c = small_case(cells=900, genes=300, dim=48, hidden=32, seed=77, density=0.12, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    sd = O.init_params(48, 32, 5, 2, c["G"], seed=3)
    want = O.csr_forward(sd, O.build_csr_graph(c["expr"]), c["feats"], 2)
    feats = dev(c["feats"])
    labels = (torch.arange(900, device=DEV) * 7 % 5).long()

    def run():
        m = sda.GNN(48, 32, 5, 2, c["G"], activation=F.relu).to(DEV)
        m.load_state_dict(sd)
        m.order = "aggregate_first"                             # the order whose Linear + bias + ReLU uses the fused epilogue
        m.eval()
        with torch.no_grad():
            logits = m(g, feats)
        m.train()
        loss = ops.cross_entropy_sum(m(g, feats), labels)
        loss.backward()
        return logits, loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}

    base = run()
    assert hasattr(torch, "_addmm_activation")
    real = torch._addmm_activation
    calls = {"n": 0}

    def raising(*a, **k):
        calls["n"] += 1
        raise RuntimeError("contract changed")
    monkeypatch.setattr(torch, "_addmm_activation", raising)
    raised = run()
    assert calls["n"] > 0                                        # the fast path WAS attempted and fell back
    monkeypatch.delattr(torch, "_addmm_activation")
    absent = run()
    monkeypatch.setattr(torch, "_addmm_activation", real, raising=False)
    for other in (raised, absent):
        np.testing.assert_allclose(other[0].cpu().numpy(), base[0].cpu().numpy(), atol=2e-6, rtol=1e-6)
        assert abs(float(other[1]) - float(base[1])) < 1e-5 * max(1.0, abs(float(base[1])))
        for k in base[2]:
            np.testing.assert_allclose(other[2][k].cpu().numpy(), base[2][k].cpu().numpy(), atol=2e-5, rtol=1e-4, err_msg=k)
    np.testing.assert_allclose(base[0].cpu().numpy(), want, atol=TOL)
    np.testing.assert_allclose(absent[0].cpu().numpy(), want, atol=TOL)
    # the preferred-BLAS switch of bench.py is a hint with a fallback of its own: either answer leaves the results alone
    try:
        torch.backends.cuda.preferred_blas_library("hipblaslt")
        with_lt = run()[0]
        torch.backends.cuda.preferred_blas_library("default")
        np.testing.assert_allclose(with_lt.cpu().numpy(), base[0].cpu().numpy(), atol=2e-6, rtol=1e-6)
    except Exception:
        pass


def test_tuned_gemm_picks_change_speed_not_results():
    """`tuning.use_tuned_gemms()` (PyTorch TunableOp, selection only) routes the dense projections to the library kernels
    recorded per shape in the tracked file: same logits to rounding, and the fp32 projections leave wgnn_linear_fwd for
    the library (which wins once tuned); fp16-stored features keep the widening loader."""
    import subprocess, sys as _sys, json as _json
    from pathlib import Path
    code = r'''
import sys, json, torch, torch.nn.functional as F
sys.path.insert(0, %r)
import scdeepsort_amd as sda
from scdeepsort_amd import synthetic as S, tuning, ops
dev = "cuda:0"
rp, col, val = S.synth_expression(60000, 3000, 0.03, device=dev)
g = sda.CellGeneGraph.from_device_csr(rp, col, val, 3000)
torch.manual_seed(0)
m = sda.GNN(400, 256, 16, 2, 3000, activation=F.relu).to(dev).eval()
f = S.synth_features(63000, 400, device=dev)
x = f[3000:]
with torch.no_grad():
    before = m(g, f)
    routed_before = ops.use_wgnn_linear(x, m.layers[0].fc_neigh.weight)
    ok = tuning.use_tuned_gemms()
    after = m(g, f)
    routed_after = ops.use_wgnn_linear(x, m.layers[0].fc_neigh.weight)
    routed_half = ops.use_wgnn_linear(x.half(), m.layers[0].fc_neigh.weight)
print(json.dumps({"loaded": ok, "active": tuning.active(), "diff": float((before - after).abs().max()),
                  "routed": [routed_before, routed_after, routed_half]}))
''' % str(Path(sda.__file__).resolve().parent.parent)
    r = subprocess.run([_sys.executable, "-c", code], capture_output=True, text=True, timeout=600)     # own process: TunableOp is global state
    assert r.returncode == 0, r.stderr[-2000:]
    rec = _json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["diff"] < 1e-4
    assert rec["routed"][0] is True and rec["routed"][2] is True
    if rec["loaded"]:                                            # (a different library stack ignores the file: nothing changes)
        assert rec["active"] and rec["routed"][1] is False


@pytest.mark.parametrize("M,N,K", [(20000, 256, 256), (16500, 200, 52), (40000, 16, 256)])
def test_linear_act_training_path_fused_relu_and_bias_gradient(M, N, K):
    """ops.linear_act in TRAINING on many rows (the aggregate-first last layer, gnn.py:65-66 under train.py:84): bias + ReLU in the
    GEMM epilogue, backward = one wgnn_agg_bwd_prepare launch (ReLU mask + bias gradient) + matrix-core weight gradient -
    output and all three gradients against torch autograd in fp64."""
    from scdeepsort_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, generator=gen, device=DEV).requires_grad_(True)
    W = (torch.randn(N, K, generator=gen, device=DEV) / K ** 0.5).requires_grad_(True)
    b = torch.randn(N, generator=gen, device=DEV).requires_grad_(True)
    up = torch.randn(M, N, generator=gen, device=DEV)
    out = ops.linear_act(x, W, b, True)
    assert out.grad_fn is not None and "LinearReluBigM" in type(out.grad_fn).__name__
    (out * up).sum().backward()
    x64, W64, b64 = (t.detach().double() for t in (x, W, b))
    pre = F.linear(x64, W64, b64)
    np.testing.assert_allclose(out.detach().cpu().numpy(), torch.relu(pre).cpu().numpy(), atol=2e-5)
    # pre-activations within rounding of 0 may fall on either side of the ReLU in fp32: the gradients are checked for the mask
    # the forward actually produced (it differs from the fp64 mask on a handful of entries at most)
    mask = (out.detach() > 0)
    assert (mask != (pre > 0)).float().mean().item() < 1e-4
    gm = up.double() * mask
    for got, want in ((x.grad, gm @ W64), (W.grad, gm.t() @ x64), (b.grad, gm.sum(0))):
        assert (got.double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_joint_projection_of_one_feature_table_matches_separate_projections():
    """Small graphs: when `features` is ONE [G + C, D] tensor the layer-1 projections of gene and cell rows run as one GEMM over
    the whole table (no copy: the two slices are adjacent rows of one storage); same logits as with (gene, cell) tensors
    passed separately, and as the oracle.  Only without grad, only below GNN.JOINT_PROJECTION_MAX_ROWS."""
    from scdeepsort_amd import ops
    c = small_case(cells=300, genes=120, dim=40, hidden=24, n_classes=5, seed=9, test_cells=20)
    sd = O.init_params(40, 24, 5, 2, 120, seed=4)
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    m = make_model(sd, 40, 24, 5, 2, 120)
    f = dev(c["feats"])
    calls = []
    real = ops.linear
    import scdeepsort_amd.gnn as GN
    spy = lambda x, W, b=None: (calls.append(tuple(x.shape)), real(x, W, b))[1]
    old = GN._linear
    GN._linear = spy
    try:
        with torch.no_grad():
            one = m(g, f)
            n_one = list(calls); calls.clear()
            two = m(g, (f[:120].clone(), f[120:].clone()))
            n_two = list(calls); calls.clear()
        out_grad = m(g, f)                                           # grad mode: separate projections (autograd through slices costs more)
        n_grad = list(calls)
    finally:
        GN._linear = old
    assert (420, 40) in n_one and (120, 40) not in n_one
    assert (120, 40) in n_two and (300, 40) in n_two and (420, 40) not in n_two
    assert (420, 40) not in n_grad
    want = O.csr_forward(sd, O.build_csr_graph(c["expr"], c["support_mask"]), c["feats"], 2)
    np.testing.assert_allclose(one.cpu().numpy(), want, atol=TOL)
    assert (one - two).abs().max().item() < 2e-6 and (one - out_grad.detach()).abs().max().item() < 2e-6
    m.JOINT_PROJECTION_MAX_ROWS = 100
    assert m._adjacent_rows(f[:120], f[120:]) is None


def test_device_built_transpose_cuts_only_the_hub_source():
    """the source-major (transposed) copy of a device-built block - the backward structure of sampled training - cuts only
    sources longer than the chunk (here ONE hub gene drawn by all 3000 seed cells) into parts on static hub slots; every other source
    keeps one item and no partial rows.  K2 over it against a dense evaluation of the same block.
    The row-wave backward kernels are pinned to fp64 at every width, mode and option in tests/test_gpu_backward_ops.py."""
    from scdeepsort_amd import ops
    from scdeepsort_amd.sampler import sample_block
    rng = np.random.default_rng(3)
    C, G, D = 3000, 50, 32
    m = np.zeros((C, G), bool); m[:, 0] = True
    for r in range(C):
        m[r, rng.choice(np.arange(1, G), 3, replace=False)] = True
    expr = sp.csr_matrix(np.where(m, rng.uniform(0.5, 7, (C, G)), 0).astype(np.float32))
    g = sda.CellGeneGraph.from_expression(expr, device=DEV)
    blk = sample_block(g.cg, torch.arange(C, device=DEV), 8, torch.Generator(device=DEV).manual_seed(1))   # k >= deg + 1: every edge drawn
    csr = blk.csr
    t = csr.transposed()
    lens = (t.rowptr[1:] - t.rowptr[:-1]).cpu().numpy()
    assert lens[0] == C and lens[1:].max() < t.plan.chunk
    items = t.plan.items.cpu().numpy()
    live = items[items[:, 0] >= 0]
    assert (live[:, 0] == 0).sum() >= 2 and all((live[:, 0] == s).sum() == 1 for s in range(1, G))   # only the hub is cut
    assert t.plan.n_partials <= 8 * max(1, csr.nnz // t.plan.chunk)                                   # not G x 8 partial rows
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    gr = torch.randn(C, D, device=DEV); h_src = torch.randn(G, D, device=DEV)
    dal = torch.zeros(G + 2, device=DEV)
    dh = ops.agg_bwd_src(csr, alpha, sda.SRC_IS_GENE, gr, h_src, dal)
    A = torch.zeros(C, G, dtype=torch.float64, device=DEV)
    rows = torch.repeat_interleave(torch.arange(C, device=DEV), (csr.rowptr[1:] - csr.rowptr[:-1]).long())
    A[rows, csr.col.long()] = csr.val.double()
    T = A.t() @ (gr.double() * csr.inv_deg.double()[:, None])
    np.testing.assert_allclose(dh.cpu().numpy(), (alpha[:G, None].double() * T).cpu().numpy(), atol=2e-4, rtol=1e-5)
    np.testing.assert_allclose(dal[:G].cpu().numpy(), (h_src.double() * T).sum(1).cpu().numpy(), atol=5e-4, rtol=1e-5)


@pytest.mark.parametrize("route", ["row_wave", "tiled"])
@pytest.mark.parametrize("seeded", [False, True])
def test_three_layer_model_matches_oracle(route, seeded, monkeypatch):
    """`--n_layers 3` (train.py:139 takes any depth): logits of a 3-layer forward - full graph and a seed batch (only the last
    two layers are restricted to the seeds' closure), row-wave and LDS-streamed route (alpha-folded hand-over below the last
    layer) - and the gradients of a seed-batch / full-batch step against the oracle's NodeFlow emulation."""
    from scdeepsort_amd import ops
    c = small_case(cells=160, genes=70, dim=20, hidden=12, n_classes=4, n_layers=3, seed=31, test_cells=10)
    sd = O.init_params(20, 12, 4, 3, 70, seed=9)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    g = sda.CellGeneGraph.from_expression(c["expr"], c["support_mask"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if route == "tiled" else None)
    ids = np.array([70 + i for i in (0, 7, 33, 3, 150, 159, 42)]) if seeded else np.arange(70, 70 + 160)
    seeds = torch.from_numpy(ids).to(DEV) if seeded else None
    m = make_model(sd, 20, 12, 4, 3, 70)
    with torch.no_grad():
        got = m(g, dev(c["feats"]), seeds=seeds)
    want = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), ids, 3).numpy()
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL)
    labels = torch.from_numpy(np.arange(len(ids)) % 4)
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(c["feats"]), ids, labels, 3)
    m.train()
    l = sda.cross_entropy_sum(m(g, dev(c["feats"]), seeds=seeds), labels.to(DEV))
    l.backward()
    assert l.item() == pytest.approx(float(loss), rel=1e-5)
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), atol=2e-4, rtol=1e-3, err_msg=k)


@pytest.mark.parametrize("tiled", [False, True])
def test_sharded_branch_with_three_layers(tiled, monkeypatch):
    """The sharded branch (one shard holding every cell, no process group: the N > 1 code path with the collectives skipped) at
    `n_layers = 3`: two gene<-cell exchanges, the alpha-folded hand-over only below the LAST layer; forward and full-batch
    training gradients equal to the plain model's."""
    from scdeepsort_amd import ops, synthetic as S
    from scdeepsort_amd.sharded import ShardedWgnn
    G, C, Din, H = 150, 500, 24, 16
    rp, col, val = S.synth_expression(C, G, 0.1, device=DEV)
    torch.manual_seed(4)
    m = sda.GNN(Din, H, 4, 3, G, activation=F.relu).to(DEV)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, Din, device=DEV)
    labels = (torch.arange(C, device=DEV) % 4).long()
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if tiled else None)
    g1 = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    m.eval()
    with torch.no_grad():
        want = m(g1, feats)
    m.train()
    sda.cross_entropy_sum(m(g1, feats), labels).backward()
    want_g = {k: p.grad.clone() for k, p in m.named_parameters()}
    eng = ShardedWgnn.build(m, rp, col, val, G, global_stats=ShardedWgnn.gene_stats(col, val, G))
    m.eval()
    with torch.no_grad():
        got = eng.forward(feats[:G], feats[G:], gather_logits=False)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=2e-5)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    eng.train_step(feats[:G], feats[G:], labels, opt)
    for k, p in m.named_parameters():
        scale = max(1.0, want_g[k].abs().max().item())
        assert (p.grad - want_g[k]).abs().max().item() < 3e-4 * scale, k


# ---- round 6 ------------------------------------------------------------------------------------------------------------------
def _oracle_graph_from_raw(rp, col, val, G):
    """The oracle's operand built on the HOST from the raw expression CSR: both directions normalised by the C oracle
    (preprocess_internal.py:17-23), independent of the device's K4 / transpose."""
    from oracle import c_oracle as CO
    C = rp.shape[0] - 1
    X = sp.csr_matrix((val.cpu().numpy(), col.cpu().numpy(), rp.cpu().numpy()), shape=(C, G))
    A_cg = X.copy(); A_cg.data = CO.normalize_rows(X.indptr, X.data)
    XT = sp.csr_matrix(X.T); XT.sort_indices()
    A_gc = XT.copy(); A_gc.data = CO.normalize_rows(XT.indptr, XT.data)
    return O.CsrGraph(G, C, A_cg, A_gc, np.diff(A_cg.indptr) + 1, np.diff(A_gc.indptr) + 1)


def _forward_vs_oracle(name, oracle_forward):
    from scdeepsort_amd import ops, synthetic as S
    cfg = S.CONFIGS[name]
    G, C = cfg.genes, cfg.cells
    rp, col, val = S.synth_expression(C, G, cfg.density, device=DEV)
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    torch.manual_seed(1234)
    m = sda.GNN(cfg.dense_dim, cfg.hidden, cfg.n_classes, cfg.n_layers, G, activation=F.relu).to(DEV).eval()
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    feats = S.synth_features(G + C, cfg.dense_dim, device=DEV)
    ops.PROFILE = []
    with torch.no_grad():
        got = m(g, feats)
    torch.cuda.synchronize()
    kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
    ops.PROFILE = None
    assert "agg_tiled_flat4" in kernels, kernels                      # the dominant kernel is what is being compared
    ocg = _oracle_graph_from_raw(rp, col, val, G)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    want = oracle_forward(sd, ocg, feats.cpu().numpy(), cfg.n_layers)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"{name}: full-size forward, max |logits - oracle| over {C} x {cfg.n_classes} = {err:.3e}")
    assert got.shape == (C, cfg.n_classes) and err < TOL, err


def test_full_size_cfg3_forward_matches_the_oracle_on_every_logit():
    """BASELINE cfg3 at FULL size (100 000 x 20 000, hidden 256, 2 layers, SURVEY 8d's generator) - the bench
    workload through the bench's kernels - compared with the C oracle (reference multiply order, aggregate-first, its own
    normalisation of the raw values) on ALL 100 000 x 16 logits at the north_star tolerance."""
    from oracle import c_oracle as CO
    _forward_vs_oracle("cfg3", CO.forward)


def test_full_size_cfg2_forward_matches_the_python_oracle_on_every_logit():
    """BASELINE cfg2 (10 000 x 5 000, hidden 128) at full size against oracle.wgnn_oracle.csr_forward (the restatement pinned to
    the executed reference code, tests/test_oracle.py)."""
    _forward_vs_oracle("cfg2", lambda sd, ocg, feats, L: O.csr_forward(sd, ocg, feats, L))


@pytest.mark.parametrize("order", ["project_first", "auto"])
def test_tile_kernels_at_headline_width_match_executed_reference_code(order, monkeypatch):
    """`refcode_wide` (300 cells x 200 genes, 60 test cells, dense_dim 64, hidden 256; logits computed by the
    reference's OWN gnn.py + normalize_weight, tests/golden/make_refcode_golden.py) drives the LDS-streamed kernel at the width
    of the bench - agg_tiled_flat4's D = 256 instantiation is compared with executed reference code, not only with the oracle.
    The operand is far below the size at which a pass is routed to the tile kernels by default, so the routing threshold (the
    public knob WGNN_TILED_MIN_WORK / ops.TILED_MIN_WORK) is lowered; the profile proves which kernel produced the logits."""
    from scdeepsort_amd import ops
    z = np.load(GOLDEN / "refcode_wide.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G, order)
    ops.PROFILE = []
    try:
        with torch.no_grad():
            got = m(g, dev(z["feats"]), seeds=torch.from_numpy(z["seeds"]).to(DEV)).cpu().numpy()
        torch.cuda.synchronize()
        launches = [dict(zip(t[::2], t[1::2])) for t, _, _ in ops.PROFILE]
    finally:
        ops.PROFILE = None
    wide = [l for l in launches if l["kernel"] == "agg_tiled_flat4" and int(l["D"]) == 256]
    assert len(wide) >= (3 if order == "project_first" else 1), launches
    assert not [l for l in launches if l["kernel"] == "agg_main"], launches           # no pass fell back to the row-wave kernel
    np.testing.assert_allclose(got, z["logits"], atol=TOL)
    print("refcode_wide", order, "max |logits - reference code| =", float(np.abs(got - z["logits"]).max()))


@pytest.mark.parametrize("order", ["auto", "project_first"])
def test_tile_backward_at_headline_width_matches_executed_reference_code(order, monkeypatch):
    """The full-batch training step of `refcode_wide` on the LDS-streamed route (K1t forward at D = 256, `wgnn_ce_sum_fwd_bwd`,
    K2t backward) against the loss and gradients autograd produced through the reference's own `GNN.forward` (`fullgrad.*`)."""
    from scdeepsort_amd import ops
    z = np.load(GOLDEN / "refcode_wide.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z["n_layers"]), G, order).train()
    ops.PROFILE = []
    try:
        loss = sda.cross_entropy_sum(m(g, dev(z["feats"])), torch.from_numpy(z["full_labels"]).to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        kernels = {dict(zip(t[::2], t[1::2]))["kernel"] for t, _, _ in ops.PROFILE}
    finally:
        ops.PROFILE = None
    assert "agg_tiled_flat4" in kernels, kernels
    assert abs(float(loss) - float(z["full_loss"])) < 1e-4 * max(1.0, abs(float(z["full_loss"])))
    for k, p in m.named_parameters():
        ref = z["fullgrad." + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=TOL * max(1.0, float(np.abs(ref).max())), err_msg=k)


def test_unsorted_device_csr_gives_the_sorted_result():
    """the device plan walk needs ascending columns; `from_device_csr` sorts an unsorted caller CSR within its
    rows, so the tile kernels give the same logits as for the sorted operand (and a repeated (cell, gene) pair is an error)."""
    from scdeepsort_amd import ops, synthetic as S
    C, G, H = 3000, 700, 64
    rp, col, val = S.synth_expression(C, G, 0.1, seed=3, device=DEV)
    perm = torch.argsort(torch.rand(col.shape[0], device=DEV))                     # shuffle inside rows: sort by (row, random)
    rows = torch.repeat_interleave(torch.arange(C, device=DEV), (rp[1:] - rp[:-1]))
    perm = perm[torch.sort(rows[perm], stable=True).indices]
    ucol, uval = col[perm].contiguous(), val[perm].contiguous()
    assert not torch.equal(ucol, col)
    g_sorted = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    g_unsorted = sda.CellGeneGraph.from_device_csr(rp, ucol, uval, G)
    assert torch.equal(g_unsorted.cg.col, g_sorted.cg.col) and torch.equal(g_unsorted.cg.val, g_sorted.cg.val)
    alpha = torch.rand(G + 2, device=DEV) + 0.5
    hg, hc = S.synth_features(G, H, device=DEV), S.synth_features(C, H, seed=3, device=DEV)
    saved, ops.TILED_MIN_WORK = ops.TILED_MIN_WORK, 1
    try:
        a = sda.agg_fwd(g_sorted.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
        b = sda.agg_fwd(g_unsorted.cg, alpha, sda.SRC_IS_GENE, G + 1, hg, hc)
        a2 = sda.agg_fwd(g_sorted.gc, alpha, sda.DST_IS_GENE, G, hc, hg)
        b2 = sda.agg_fwd(g_unsorted.gc, alpha, sda.DST_IS_GENE, G, hc, hg)
    finally:
        ops.TILED_MIN_WORK = saved
    assert torch.equal(a, b) and torch.equal(a2, b2)
    dup_col = col.clone(); dup_col[1] = dup_col[0]
    with pytest.raises(ValueError, match="more than once"):
        sda.CellGeneGraph.from_device_csr(rp, dup_col, val, G)


@pytest.mark.parametrize("cells,genes,density", [(5000, 1200, 0.05), (300, 90, 0.4), (70, 2500, 0.6), (20000, 400, 0.02)])
def test_csr_transpose_kernel_matches_the_sort_path(cells, genes, density):
    """Round 6: `wgnn_csr_transpose_count` / `_fill` (csrc/wgnn_transpose.hip: per-chunk LDS histograms + an in-order walk, no sort)
    against the framework path (bincount, stable radix sort, two gathers): bit-identical gene-major copies - with and without a
    support mask (predict graphs: preprocess.py:184-187), empty cells and genes, a cell with more than 1024 genes, few and many
    chunks - and therefore identical graphs."""
    from scdeepsort_amd import graph as GR, synthetic as S
    rp, col, val = S.synth_expression(cells, genes, density, seed=cells + genes, device=DEV)
    rp32 = rp.to(torch.int32)
    mask = torch.rand(cells, device=DEV) < 0.6
    mask[: min(5, cells)] = False
    for m in (None, mask, torch.zeros(cells, dtype=torch.bool, device=DEV)):
        a = GR._transpose_on_device(rp32, col, val, cells, genes, m)
        b = GR._transpose_by_sort(rp32, col, val, cells, genes, m)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
    saved = GR.CSR_TRANSPOSE_KERNEL
    graphs = {}
    try:
        for kern in (True, False):
            GR.CSR_TRANSPOSE_KERNEL = kern
            graphs[kern] = sda.CellGeneGraph.from_device_csr(rp, col, val, genes, support_mask=mask)
            graphs[kern].cg.transposed()
    finally:
        GR.CSR_TRANSPOSE_KERNEL = saved
    for name in ("rowptr", "col", "val", "inv_deg"):
        assert torch.equal(getattr(graphs[True].gc, name), getattr(graphs[False].gc, name)), name
        assert torch.equal(getattr(graphs[True].cg._t, name), getattr(graphs[False].cg._t, name)), name
    assert GR.CSR_TRANSPOSE_KERNEL                                   # the kernel is the default on the GPU


def test_more_genes_than_the_transpose_kernel_counts_take_the_sort_path():
    """`wgnn_csr_transpose_*` keeps one LDS counter per gene (<= 32768); a wider operand is transposed by the framework path - same
    graph as the oracle's, forward through the row-wave kernel."""
    from scdeepsort_amd import graph as GR, synthetic as S
    C, G, D = 400, 40000, 32
    rp, col, val = S.synth_expression(C, G, 0.002, seed=9, device=DEV)
    with pytest.raises(Exception):
        GR._transpose_on_device(rp.to(torch.int32), col, val, C, G, None)            # WGNN_ERR_UNSUPPORTED, loudly
    g = sda.CellGeneGraph.from_device_csr(rp, col, val, G)
    expr = S.to_scipy(rp, col, val, G)
    cg = O.build_csr_graph(expr)
    alpha = np.random.default_rng(1).uniform(0.5, 1.5, G + 2).astype(np.float32)
    feats = np.random.default_rng(2).standard_normal((G + C, D)).astype(np.float32)
    zc, zg = O.csr_aggregate(cg, alpha, feats[:G].astype(np.float64), feats[G:].astype(np.float64))
    out_g = sda.agg_fwd(g.gc, dev(alpha), sda.DST_IS_GENE, G, dev(feats[G:]), dev(feats[:G]))
    out_c = sda.agg_fwd(g.cg, dev(alpha), sda.SRC_IS_GENE, G + 1, dev(feats[:G]), dev(feats[G:]))
    np.testing.assert_allclose(out_g.cpu().numpy(), zg, atol=TOL)
    np.testing.assert_allclose(out_c.cpu().numpy(), zc, atol=TOL)
