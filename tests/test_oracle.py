"""CPU tests of the oracle itself: known answers, dual-formulation agreement, algebraic
properties, and fixtures made by EXECUTING the reference's own gnn.py / normalize_weight over a
stand-in for DGL (tests/golden/make_refcode_golden.py).  The reference holds no test vectors of its own for this path."""
import json

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import GOLDEN, load_golden, small_case
from oracle import wgnn_oracle as O


def test_kat_2x2_hand_derived():
    kat = json.loads((GOLDEN / "kat_2x2.json").read_text())
    expr = sp.csr_matrix(np.array(kat["expr_rows"], dtype=np.float32))
    g = O.build_reference_graph(expr)
    G = kat["genes"]
    # normalised weights (preprocess_internal.py:17-23), keyed by (src, dst)
    w = {(int(s), int(d)): float(x) for s, d, x in zip(g.src, g.dst, g.weight)}
    assert w[(2, 0)] == pytest.approx(kat["norm_w_into_g0"]["c0"], rel=1e-6)
    assert w[(3, 0)] == pytest.approx(kat["norm_w_into_g0"]["c1"], rel=1e-6)
    assert w[(2, 1)] == pytest.approx(kat["norm_w_into_g1"]["c0"], rel=1e-6)
    assert w[(0, 2)] == pytest.approx(kat["norm_w_into_c0"]["g0"], rel=1e-6)
    assert w[(1, 2)] == pytest.approx(kat["norm_w_into_c0"]["g1"], rel=1e-6)
    assert w[(0, 3)] == pytest.approx(kat["norm_w_into_c1"]["g0"], rel=1e-6)
    for n in range(4):
        assert w[(n, n)] == 1.0                                   # self-loops added after normalisation
    alpha = torch.tensor(kat["alpha"]).unsqueeze(-1)
    x = torch.tensor(kat["features"]).unsqueeze(-1)
    neigh = O.block_compute(x, g.src, g.dst, torch.from_numpy(g.weight), g.node_id, g.node_id, 4, alpha, G).ravel()
    want = [kat["neigh"][k] for k in ("g0", "g1", "c0", "c1")]
    np.testing.assert_allclose(neigh.numpy(), want, rtol=1e-6)
    cg = O.build_csr_graph(expr)
    zc, zg = O.csr_aggregate(cg, alpha.numpy(), x.numpy()[:G], x.numpy()[G:])
    np.testing.assert_allclose(np.concatenate([zg.ravel(), zc.ravel()]), want, rtol=1e-6)


def test_alpha_index_rules():
    # gnn.py:49-53 on the four edge kinds (src_id, dst_id): gene->cell, cell->gene, gene loop, cell loop
    src = np.array([3, -1, 2, -1]); dst = np.array([-1, 4, 2, -1])
    np.testing.assert_array_equal(O.alpha_index(src, dst, 10), [3, 4, 10, 11])


@pytest.mark.parametrize("name", ["testis199", "pancreas11"])
def test_golden_fixture_reproduces(name):
    c = load_golden(name)
    g = O.build_reference_graph(c["expr"], c["support_mask"])
    logits = O.edgelist_full_forward(c["sd"], g, torch.from_numpy(c["feats"]), c["n_layers"]).numpy()[c["G"]:]
    np.testing.assert_allclose(logits, c["z"]["logits_f32"], atol=2e-6)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    csr = O.csr_forward(c["sd"], cg, c["feats"], c["n_layers"])
    np.testing.assert_allclose(csr, c["z"]["logits_f64"], atol=5e-6)


def test_edgelist_vs_csr_random_ragged():
    c = small_case(seed=1)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], c["n_layers"], c["G"], seed=2)
    g = O.build_reference_graph(c["expr"], c["support_mask"])
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    a = O.edgelist_full_forward(sd, g, torch.from_numpy(c["feats"]), c["n_layers"]).numpy()[c["G"]:]
    b = O.csr_forward(sd, cg, c["feats"], c["n_layers"])
    np.testing.assert_allclose(a, b, atol=2e-6)
    assert np.isfinite(a).all()            # empty cell row: only the self-loop, degree 1


def test_seed_batching_invariance_eval_mode():
    """Per-batch NodeFlow (train.py:71-81) == full-graph layer-wise evaluation, any batch split / order."""
    c = small_case(seed=3)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=4)
    g = O.build_reference_graph(c["expr"], c["support_mask"])
    feats = torch.from_numpy(c["feats"])
    full = O.edgelist_full_forward(sd, g, feats, 2)[c["G"]:]
    rng = np.random.default_rng(0)
    seeds = rng.permutation(np.arange(c["G"], c["G"] + c["C"]))
    for batch in np.array_split(seeds, 5):
        out = O.nodeflow_forward(sd, g, feats, batch, 2)
        np.testing.assert_allclose(out.numpy(), full[batch - c["G"]].numpy(), atol=2e-6)


def test_unit_alpha_unit_weight_is_plain_mean():
    c = small_case(seed=5, empty_rows=False, test_cells=0)
    expr = c["expr"].copy(); expr.data[:] = 1.0        # equal weights -> normalised weight = deg*1/deg = 1
    cg = O.build_csr_graph(expr)
    G = c["G"]
    alpha = np.ones(G + 2, np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, _ = O.csr_aggregate(cg, alpha, Hg, Hc)
    dense = (expr.toarray() > 0)
    want = (dense @ Hg + Hc) / (dense.sum(1, keepdims=True) + 1)
    np.testing.assert_allclose(zc, want, atol=1e-5)


def test_linearity_in_features():
    c = small_case(seed=6)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    G = c["G"]
    rng = np.random.default_rng(1)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32)
    f1, f2 = c["feats"], rng.standard_normal(c["feats"].shape).astype(np.float32)
    z1 = O.csr_aggregate(cg, alpha, f1[:G].astype(np.float64), f1[G:].astype(np.float64))
    z2 = O.csr_aggregate(cg, alpha, f2[:G].astype(np.float64), f2[G:].astype(np.float64))
    f3 = 2.0 * f1.astype(np.float64) - 0.5 * f2
    z3 = O.csr_aggregate(cg, alpha, f3[:G], f3[G:])
    for a, b, cc in zip(z1, z2, z3):
        np.testing.assert_allclose(2.0 * a - 0.5 * b, cc, atol=1e-10)


def test_predict_graph_test_cells_feed_nothing_back():
    """preprocess.py:184-187: test cells have gene->cell edges only, so gene rows ignore them."""
    c = small_case(seed=7, test_cells=16)
    cg = O.build_csr_graph(c["expr"], c["support_mask"])
    assert cg.A_gc[:, -16:].nnz == 0
    assert cg.A_cg[-16:, :].nnz > 0


def test_gradient_oracle_matches_finite_difference():
    c = small_case(cells=24, genes=16, dim=8, hidden=6, seed=8, test_cells=0)
    sd = O.init_params(8, 6, 3, 2, 16, seed=9, dtype=torch.float64)
    g = O.build_reference_graph(c["expr"])
    feats = torch.from_numpy(c["feats"]).double()
    seeds = np.arange(16, 16 + 10)
    labels = torch.from_numpy(np.random.default_rng(0).integers(0, 3, 10))
    loss, grads, _ = O.loss_and_grads(sd, g, feats, seeds, labels, 2)
    eps = 1e-6
    for key, idx in (("alpha", (3, 0)), ("alpha", (16, 0)), ("alpha", (17, 0)), ("layers.0.fc_neigh.weight", (2, 5))):
        sp_, sm = {k: v.clone() for k, v in sd.items()}, {k: v.clone() for k, v in sd.items()}
        sp_[key][idx] += eps; sm[key][idx] -= eps
        lp = torch.nn.functional.cross_entropy(O.nodeflow_forward(sp_, g, feats, seeds, 2), labels, reduction="sum")
        lm = torch.nn.functional.cross_entropy(O.nodeflow_forward(sm, g, feats, seeds, 2), labels, reduction="sum")
        fd = float(lp - lm) / (2 * eps)
        assert grads[key][idx].item() == pytest.approx(fd, rel=1e-4, abs=1e-7)


def test_postprocess_unsure_rule():
    logits = np.array([[2.0, 0.0, 0.0, 0.0], [0.1, 0.0, 0.05, 0.0]], dtype=np.float32)
    pred, prob = O.postprocess(logits, unsure_rate=2.0)      # threshold 2/4 = 0.5  (predict.py:82-86)
    assert pred[0] == 0 and prob[0, 0] > 0.5
    assert pred[1] == -1
    pred0, _ = O.postprocess(logits, unsure_rate=0.0)
    assert (pred0 >= 0).all()


def test_sampled_nodeflow_replay_matches_rng_draw():
    """num_neighbors > 0 (train.py:37-40): replaying a recorded draw through ``picker`` reproduces the rng result,
    and a draw no smaller than every in-degree is the full neighbourhood."""
    c = small_case(seed=21)
    sd = O.init_params(c["dim"], c["hidden"], c["n_classes"], 2, c["G"], seed=2)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    x = torch.from_numpy(c["feats"])
    seeds = np.arange(c["G"], c["G"] + 20)
    full = O.nodeflow_forward(sd, rg, x, seeds, 2)
    big = O.nodeflow_forward(sd, rg, x, seeds, 2, num_neighbors=10 ** 6, rng=np.random.default_rng(0))
    assert torch.equal(full, big)
    ine = O._InEdges(rg)
    rec = {}
    rng = np.random.default_rng(4)

    def recording(block, v):
        lo, hi = ine.ptr[v], ine.ptr[v + 1]
        sel = np.arange(lo, hi)
        if hi - lo > 3:
            sel = rng.choice(sel, size=3, replace=False)
        rec[(block, v)] = ine.src[sel]
        return rec[(block, v)]
    a = O.nodeflow_forward(sd, rg, x, seeds, 2, picker=recording)
    b = O.nodeflow_forward(sd, rg, x, seeds, 2, picker=lambda blk, v: rec[(blk, v)])
    assert torch.equal(a, b)
    assert not torch.allclose(a, full)


# ---- fixtures produced by executing the reference's own gnn.py / normalize_weight (tests/golden/make_refcode_golden.py)
def _load_refcode(name):
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    return z, sd


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer", "refcode_wide"])
def test_restatement_matches_executed_reference_code(name):
    """GNN.forward / message_func / NodeUpdate (gnn.py:10-68) and normalize_weight (preprocess_internal.py:15-23) were
    EXECUTED from the reference tree over a stand-in for DGL's NodeFlow / fn.mean; both formulations of the oracle must
    reproduce those logits and those normalised edge weights."""
    z, sd = _load_refcode(name)
    expr = sp.csr_matrix(z["expr"]); mask = z["support_mask"]; L = int(z["n_layers"])
    G = expr.shape[1]
    rg = O.build_reference_graph(expr, mask)
    # normalised weights, edge by edge (the oracle's edge order: cell->gene edges of support cells, then gene->cell)
    got_w = {(int(s), int(d)): float(w) for s, d, w in zip(rg.src, rg.dst, rg.weight) if s != d}
    want_w = {(int(s), int(d)): float(w) for s, d, w in zip(z["edge_src"], z["edge_dst"], z["edge_w_norm"])}
    assert got_w.keys() == want_w.keys()
    assert max(abs(got_w[k] - want_w[k]) for k in want_w) < 2e-6
    feats = torch.from_numpy(z["feats"])
    logits_edge = O.nodeflow_forward(sd, rg, feats, z["seeds"], L).numpy()
    np.testing.assert_allclose(logits_edge, z["logits"], atol=2e-6)
    cg = O.build_csr_graph(expr, mask)
    logits_csr = O.csr_forward(sd, cg, z["feats"], L)
    np.testing.assert_allclose(logits_csr, z["logits"], atol=2e-6)


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer"])
def test_gradient_oracle_matches_executed_reference_code(name):
    """Loss (CrossEntropyLoss sum, train.py:36) and parameter gradients of one seed batch, computed by autograd through
    the reference's own GNN code, against the oracle's edge-list formulation."""
    z, sd = _load_refcode(name)
    rg = O.build_reference_graph(sp.csr_matrix(z["expr"]), z["support_mask"])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(z["feats"]), z["batch"], torch.from_numpy(z["labels"]),
                                      int(z["n_layers"]))
    assert abs(float(loss) - float(z["loss"])) < 1e-5 * max(1.0, abs(float(z["loss"])))
    for k, gval in grads.items():
        np.testing.assert_allclose(gval.numpy(), z["grad." + k], atol=3e-6, rtol=1e-5, err_msg=k)


@pytest.mark.parametrize("name", ["refcode_train", "refcode_predict", "refcode_1layer", "refcode_wide"])
def test_full_batch_gradient_oracle_matches_executed_reference_code(name):
    """Round 4: the FULL-batch step (every cell a seed: BASELINE cfg4's shape) through the reference's own GNN code + autograd,
    against the oracle - the fixture the GPU test of the fused backward glue / loss kernel is pinned to."""
    z, sd = _load_refcode(name)
    rg = O.build_reference_graph(sp.csr_matrix(z["expr"]), z["support_mask"])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(z["feats"]), z["seeds"], torch.from_numpy(z["full_labels"]),
                                      int(z["n_layers"]))
    assert abs(float(loss) - float(z["full_loss"])) < 1e-5 * max(1.0, abs(float(z["full_loss"])))
    for k, gval in grads.items():
        np.testing.assert_allclose(gval.numpy(), z["fullgrad." + k], atol=3e-6, rtol=1e-5, err_msg=k)


# ---- neighbour-sampled NodeFlows (num_neighbors > 0, train.py:37-40): refcode_sampled.npz holds recorded draws and what the
# reference's own GNN.forward computed over them
SAMPLED_CASES = ["L1k3", "L2k1", "L2k3", "L2k7"]


def _sampled_case(prefix):
    z = np.load(GOLDEN / "refcode_sampled.npz")
    sd = {k[len(prefix) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix + ".param.")}
    draw = {}
    for b, d, s in zip(z[prefix + ".draw_block"], z[prefix + ".draw_dst"], z[prefix + ".draw_src"]):
        draw.setdefault((int(b), int(d)), []).append(int(s))
    return z, sd, draw


def test_sampled_fixture_holds_every_case():
    z = np.load(GOLDEN / "refcode_sampled.npz")
    assert list(z["cases"]) == SAMPLED_CASES
    assert int(z["dim"]) % 4 and int(z["hidden"]) % 4              # both widths are padded by the HIP path


@pytest.mark.parametrize("prefix", SAMPLED_CASES)
def test_oracle_replays_the_executed_reference_draw(prefix, monkeypatch):
    """The oracle's NodeFlow, replaying the recorded draw through ``picker``, uses exactly the recorded edges per block and
    reproduces the logits the reference's own GNN.forward computed over that draw."""
    z, sd, draw = _sampled_case(prefix)
    L = int(z[prefix + ".n_layers"])
    rg = O.build_reference_graph(sp.csr_matrix(z["expr"]), z["support_mask"])
    used = []
    real_of = O._InEdges.of

    def recording(self, nodes, rng, num_neighbors, picker=None, block=0):
        s, d, w = real_of(self, nodes, rng, num_neighbors, picker, block)
        used.extend((block, int(nodes[j]), int(v)) for j, v in zip(d, s))
        return s, d, w
    monkeypatch.setattr(O._InEdges, "of", recording)
    logits = O.nodeflow_forward(sd, rg, torch.from_numpy(z["feats"]), z[prefix + ".seeds"], L,
                                picker=lambda block, v: np.array(draw[(block, v)])).numpy()
    want = sorted(zip(z[prefix + ".draw_block"].tolist(), z[prefix + ".draw_dst"].tolist(), z[prefix + ".draw_src"].tolist()))
    assert sorted(used) == want
    np.testing.assert_allclose(logits, z[prefix + ".logits"], atol=2e-6)


@pytest.mark.parametrize("prefix", SAMPLED_CASES)
def test_gradient_oracle_matches_executed_reference_code_on_a_drawn_nodeflow(prefix):
    z, sd, draw = _sampled_case(prefix)
    rg = O.build_reference_graph(sp.csr_matrix(z["expr"]), z["support_mask"])
    loss, grads, _ = O.loss_and_grads(sd, rg, torch.from_numpy(z["feats"]), z[prefix + ".seeds"],
                                      torch.from_numpy(z[prefix + ".labels"]), int(z[prefix + ".n_layers"]),
                                      picker=lambda block, v: np.array(draw[(block, v)]))
    ref = float(z[prefix + ".loss"])
    assert abs(float(loss) - ref) < 1e-5 * max(1.0, abs(ref))
    assert grads.keys() == sd.keys()
    for k, gval in grads.items():
        np.testing.assert_allclose(gval.numpy(), z[f"{prefix}.grad.{k}"], atol=3e-6, rtol=1e-5, err_msg=k)


def _kat_rational():
    import json
    kat = json.loads((GOLDEN / "kat_2layer_predict.json").read_text())
    t = lambda x: torch.tensor(x, dtype=torch.float64)
    sd = {"layers.0.fc_neigh.weight": t(kat["W1"]), "layers.0.fc_neigh.bias": t(kat["b1"]),
          "layers.1.fc_neigh.weight": t(kat["W2"]), "layers.1.fc_neigh.bias": t(kat["b2"]),
          "alpha": t(kat["alpha"]).reshape(-1, 1), "linear.weight": t(kat["W_out"]), "linear.bias": t(kat["b_out"])}
    expr = sp.csr_matrix(np.array(kat["expr_rows"], dtype=np.float32))
    return kat, sd, expr, np.array(kat["support_mask"], bool), np.array(kat["features"], np.float32)


def test_kat_two_layers_predict_graph_exact_rational():
    """D = 4, two layers, a hub gene, a test cell (gene->cell edges only) and a gene whose only expressing cell is that
    test cell: answers derived in exact rational arithmetic from the cited reference lines
    (tests/golden/make_kat_rational.py) - independent of numpy/torch and of the DGL stand-in."""
    kat, sd, expr, support, feats = _kat_rational()
    G, C = kat["genes"], kat["cells"]
    for dt, tol in ((np.float64, 5e-7), (np.float32, 2e-6)):      # graph weights are normalised in fp32 like the reference
        sdd = {k: v if dt == np.float64 else v.float() for k, v in sd.items()}
        logits, hidden = O.csr_forward(sdd, O.build_csr_graph(expr, support, dtype=dt), feats.astype(dt), 2, dtype=dt,
                                       return_hidden=True)
        np.testing.assert_allclose(logits, kat["logits"], atol=tol * 10, rtol=tol)
        np.testing.assert_allclose(np.concatenate([hidden[0][0], hidden[0][1]]), kat["h1"], atol=tol * 10, rtol=tol)
    rg = O.build_reference_graph(expr, support)
    got = O.nodeflow_forward({k: v.double() for k, v in sd.items()}, rg, torch.from_numpy(feats).double(),
                             np.arange(G, G + C), 2)
    np.testing.assert_allclose(got.numpy(), kat["logits"], atol=2e-6)      # fp32-normalised weights in the edge list
    # the gene expressed only by the test cell has no in-edge: its layer-1 row is its self-loop alone
    a, x = kat["alpha"], np.array(kat["features"][2])
    want = np.maximum(np.array(kat["W1"]) @ (a[G] * x) + np.array(kat["b1"]), 0)
    np.testing.assert_allclose(kat["h1"][2], want, atol=1e-12)
    # normalised weights as on paper: into c3 (3 in-edges 2,2,5 -> 3*x/9), into g0 (support cells 1,2,4 -> 3*x/7)
    nw = kat["normalised_weights_exact"]
    assert (nw["g0->c3"], nw["g2->c3"], nw["c0->g0"], nw["c2->g0"]) == ("2/3", "5/3", "3/7", "12/7")
    assert "c3->g0" not in nw and "c3->g2" not in nw


@pytest.mark.parametrize("unsure_rate", [0.0, 2.0, 3.0])
def test_api_classify_matches_oracle_postprocess(unsure_rate):
    """a10 (predict.py:78-88): softmax, 'unsure' iff max_prob < unsure_rate/num_classes (STRICT), else argmax -
    product ``api._classify`` against the restatement, including rows that sit exactly on the boundary."""
    from scdeepsort_amd.api import _classify
    rng = np.random.default_rng(3)
    logits = rng.normal(0, 1.5, (500, 4)).astype(np.float32)
    logits[0] = 0.0                                        # uniform: max_prob = 1/4 exactly
    logits[1] = [np.log(3.0), 0.0, 0.0, 0.0]               # max_prob = 3/6 = 0.5 = 2/4 (up to fp32 rounding)
    logits[2] = [5.0, 5.0, -5.0, -5.0]                     # tie: argmax takes the first
    pred, prob = _classify(torch.from_numpy(logits), unsure_rate)
    want, wprob = O.postprocess(logits, unsure_rate)
    np.testing.assert_allclose(prob, wprob, atol=1e-6)
    # rows whose max prob is within rounding of the threshold may legitimately fall either way; everything else is exact
    clear = np.abs(wprob.max(1) - unsure_rate / 4) > 1e-6
    assert clear.sum() >= 497
    np.testing.assert_array_equal(pred[clear], want[clear])
    if unsure_rate == 0.0:
        assert (pred >= 0).all()
    if unsure_rate == 3.0:
        assert (pred == -1).sum() > 100 and pred[0] == -1
    assert pred[2] in (0, -1) and (pred[2] == want[2])


@pytest.mark.parametrize("blocked", [False, True])
def test_c_port_matches_numpy_restatement(blocked):
    """oracle/wgnn_oracle.c (the timed `cpu_baseline` of bench.py) - the row-wise port and its cache-blocked form (tile of
    destination rows x block of source rows, ragged last tile / block, empty rows) - against the numpy CSR restatement, both
    directions, and the whole forward in the project-first order."""
    from oracle import c_oracle as CO
    c = small_case(cells=130, genes=70, dim=24, hidden=16, n_classes=4, seed=9, test_cells=0)
    G, C = c["G"], c["C"]
    cg = O.build_csr_graph(c["expr"])
    rng = np.random.default_rng(2)
    alpha = (rng.random(G + 2) + 0.5).astype(np.float32)
    Hg, Hc = c["feats"][:G], c["feats"][G:]
    zc, zg = O.csr_aggregate(cg, alpha, Hg.astype(np.float64), Hc.astype(np.float64))
    agg = (lambda *a: CO.aggregate_blocked(*a, tile_rows=32, block_rows=24)) if blocked else CO.aggregate
    got_c = agg(cg.A_cg.indptr, cg.A_cg.indices, cg.A_cg.data, alpha, 0, G + 1, Hg, Hc)
    got_g = agg(cg.A_gc.indptr, cg.A_gc.indices, cg.A_gc.data, alpha, 1, G, Hc, Hg)
    np.testing.assert_allclose(got_c, zc, atol=2e-6)
    np.testing.assert_allclose(got_g, zg, atol=2e-6)
    sd = O.init_params(24, 16, 4, 2, G, seed=4)
    want = O.csr_forward(sd, cg, c["feats"], 2)
    got = CO.forward(sd, cg, c["feats"], 2, order="project_first_blocked" if blocked else "project_first")
    np.testing.assert_allclose(got, want, atol=2e-5)
    np.testing.assert_allclose(CO.forward(sd, cg, c["feats"], 2), want, atol=2e-5)       # the reference's aggregate-first order


def test_two_formulations_agree_at_three_layers():
    """`--n_layers 3`: the edge-list NodeFlow emulation (gnn.py:47-68 literally) and the CSR full-graph formulation agree, on
    a predict graph with test cells (the GPU test of the 3-layer model is checked against the former)."""
    from conftest import small_case
    c = small_case(cells=160, genes=70, dim=20, hidden=12, n_classes=4, n_layers=3, seed=31, test_cells=10)
    sd = O.init_params(20, 12, 4, 3, 70, seed=9)
    rg = O.build_reference_graph(c["expr"], c["support_mask"])
    a = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), np.arange(70, 230), 3).numpy()
    b = O.csr_forward(sd, O.build_csr_graph(c["expr"], c["support_mask"]), c["feats"], 3)
    np.testing.assert_allclose(a, b, atol=2e-6)
    sub = O.nodeflow_forward(sd, rg, torch.from_numpy(c["feats"]), np.array([75, 229, 100]), 3).numpy()
    np.testing.assert_allclose(sub, b[[5, 159, 30]], atol=2e-6)           # a seed batch sees the same 3-hop closure
