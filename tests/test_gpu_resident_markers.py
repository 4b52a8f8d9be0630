"""``ResidentPredictor.markers`` and its kernel ``wgnn_group_gene_reduce`` on the GPU: bit-exact against the fp64
restatement of tests/markers_reference.py on lattice scores, under its derived bound on float scores, the completeness
identity per group end to end, streaming, ranking, and pinned to logits the reference's own code produced.

Figures measured on an MI355X (profiles/resident_markers.md): worst |got - want| / bound over the float cases 0 - every
case, the ~175-term bins of the dense one included: such sums of f32 terms need fewer than 53 bits and fp64 adds them exactly
in any order; end to end the score sums likewise, and the worst identity gap / bound was 0.005 (1 layer, hidden 18).  Every
test prints its own worst ratio before it asserts."""
import ctypes as C
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import attrib_reference as R
import markers_reference as M
from test_gpu_resident_predict import _device_csr, _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(c):
    return t(c.rowptr.astype(np.int64 if c.i64 else np.int32)), t(c.col), t(c.group)


def _check_case(c):
    """Lattice scores bit for bit, float scores under the bound; returns the worst float error / bound ratio."""
    rp, col, group = _operands(c)
    want_s, want_c, mag = M.reduce(c.rowptr, c.col, c.lat, c.group, c.K, c.G)
    assert M.exact_premise(mag)
    total, count = ops.group_gene_reduce(rp, col, t(c.lat), group, c.K, c.G)
    assert total.dtype == torch.float64 and count.dtype == torch.int32 and total.shape == (c.K, c.G) == count.shape
    assert np.array_equal(total.cpu().numpy(), want_s), (c.K, c.G, c.i64)
    assert np.array_equal(count.cpu().numpy(), want_c), (c.K, c.G, c.i64)
    again = ops.group_gene_reduce(rp, col, t(c.lat), group, c.K, c.G)
    assert torch.equal(again[0], total) and torch.equal(again[1], count)
    want_s, want_c, mag = M.reduce(c.rowptr, c.col, c.flt, c.group, c.K, c.G)
    total, count = ops.group_gene_reduce(rp, col, t(c.flt), group, c.K, c.G)
    assert np.array_equal(count.cpu().numpy(), want_c)
    err, bound = np.abs(total.cpu().numpy() - want_s), M.bound(want_c, mag)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert (err <= bound).all(), (c.K, c.G, c.i64, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------
# 5. / 6. the kernel against the fp64 reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", M.GENES)
@pytest.mark.parametrize("K", M.GROUPS)
def test_reduce_is_bit_exact_on_lattice_scores_and_bounded_on_floats(K, G):
    worst = max(_check_case(M.case(K, G, i64)) for i64 in (False, True))
    print(f"K={K} G={G}: worst float |got - want| / bound = {worst:.2e}")


@pytest.mark.parametrize("name", M.SPECIAL)
def test_reduce_special_batches(name):
    c = M.special(name)
    worst = _check_case(c)
    print(f"{name}: worst float |got - want| / bound = {worst:.2e}")


def test_reduce_of_a_dense_group_needs_the_fold():
    """Bins with hundreds of terms (every lane of the wave holds partial sums): 700 cells x 64 genes, all expressed."""
    rng = np.random.default_rng(3)
    B, G, K = 700, 64, 3
    c = M.case(K, G, False, seed=3)
    c.B, c.rowptr, c.col = B, (np.arange(B + 1) * G).astype(np.int64), np.tile(np.arange(G, dtype=np.int32), B)
    c.group = rng.integers(-1, K, B).astype(np.int32)
    c.lat, c.flt = M.lattice(rng, B * G), rng.standard_normal(B * G).astype(np.float32)
    worst = _check_case(c)
    print(f"dense: worst float |got - want| / bound = {worst:.2e}")


# ------------------------------------------------------------------------------------------------
# 7. accumulate / overwrite
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,G", [(16, 6000), (300, 40000)])
def test_accumulate_equals_the_concatenated_batch(K, G):
    a, b = M.case(K, G, False, seed=21), M.case(K, G, True, seed=22)
    rowptr = np.concatenate([a.rowptr, a.rowptr[-1] + b.rowptr[1:]])
    col, group = np.concatenate([a.col, b.col]), np.concatenate([a.group, b.group])
    for name in ("lat", "flt"):
        sa, sb = getattr(a, name), getattr(b, name)
        # without the flag the outputs are fully overwritten, whatever they held
        out = (torch.full((K, G), float("nan"), dtype=torch.float64, device=DEV),
               torch.full((K, G), -77, dtype=torch.int32, device=DEV))
        got = ops.group_gene_reduce(*_operands(a)[:2], t(sa), t(a.group), K, G, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        first_s, first_c, _ = M.reduce(a.rowptr, a.col, sa, a.group, K, G)
        assert np.array_equal(out[1].cpu().numpy(), first_c) and not bool(torch.isnan(out[0]).any())
        ops.group_gene_reduce(*_operands(b)[:2], t(sb), t(b.group), K, G, out=out, accumulate=True)
        want_s, want_c, mag = M.reduce(rowptr, col, np.concatenate([sa, sb]), group, K, G)
        assert np.array_equal(out[1].cpu().numpy(), want_c)
        if name == "lat":
            assert np.array_equal(out[0].cpu().numpy(), want_s)
        else:
            err, bound = np.abs(out[0].cpu().numpy() - want_s), M.bound(want_c, mag)
            print(f"K={K} G={G} accumulate: worst ratio {float((err[bound > 0] / bound[bound > 0]).max()):.2e}")
            assert (err <= bound).all()
    with pytest.raises(sda.WgnnError, match="accumulate needs"):
        ops.group_gene_reduce(*_operands(a)[:2], t(a.lat), t(a.group), K, G, accumulate=True)


# ------------------------------------------------------------------------------------------------
# 8. guard words
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 300])
def test_guard_words_around_every_output(K):
    from scdeepsort_amd.graph import _transpose_on_device
    c = M.case(K, 6000, False, seed=31)
    rp, col, group = _operands(c)
    t_rowptr, t_cell, t_score = _transpose_on_device(rp, col, t(c.lat), c.B, c.G, group >= 0)
    nb = C.c_int64()
    assert _lib.lib().wgnn_group_gene_reduce_workspace(c.B, len(c.col), K, c.G, C.addressof(nb)) == 0
    PAD = 64

    def guarded(n, dtype, sent):
        buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device=DEV)
        return buf, buf[PAD:PAD + n], sent

    bufs = {"sum": guarded(K * c.G, torch.float64, -12345.0), "count": guarded(K * c.G, torch.int32, -12345),
            "ws": guarded(nb.value, torch.uint8, 0xA5)}
    run = lambda: _lib.call(torch.device(DEV), "wgnn_group_gene_reduce", t_rowptr.data_ptr(), t_cell.data_ptr(),
                            t_score.data_ptr(), group.data_ptr(), c.B, K, c.G, bufs["sum"][1].data_ptr(),
                            bufs["count"][1].data_ptr(), bufs["ws"][1].data_ptr() if nb.value else None, nb.value, 0, None)
    assert run() == 0
    torch.cuda.synchronize()
    for name, (buf, view, sent) in bufs.items():
        n = view.numel()
        assert bool((buf[:PAD] == sent).all()) and bool((buf[PAD + n:] == sent).all()), name
    want_s, want_c, _ = M.reduce(c.rowptr, c.col, c.lat, c.group, K, c.G)
    got_s, got_c = bufs["sum"][1].clone(), bufs["count"][1].clone()
    assert np.array_equal(got_s.cpu().numpy().reshape(K, c.G), want_s) and np.array_equal(got_c.cpu().numpy().reshape(K, c.G), want_c)
    assert run() == 0                                          # a second launch is bit-identical
    assert torch.equal(bufs["sum"][1], got_s) and torch.equal(bufs["count"][1], got_c)


# ------------------------------------------------------------------------------------------------
# 9. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_the_check_and_the_process_goes_on():
    c = M.case(16, 6000, False, seed=41)
    rp, col, group = _operands(c)
    s = t(c.lat)
    with pytest.raises(sda.WgnnError, match="one id per cell"):
        ops.group_gene_reduce(rp, col, s, group[:-1], 16, c.G)
    bad = group.clone(); bad[5] = 16
    with pytest.raises(sda.WgnnError, match="group id out of range"):
        ops.group_gene_reduce(rp, col, s, bad, 16, c.G)
    bad = group.clone(); bad[5] = -2
    with pytest.raises(sda.WgnnError, match="group id out of range"):
        ops.group_gene_reduce(rp, col, s, bad, 16, c.G)
    badc = col.clone(); badc[1] = c.G
    with pytest.raises(sda.WgnnError, match="gene id out of range"):
        ops.group_gene_reduce(rp, badc, s, group, 16, c.G)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        ops.group_gene_reduce(rp, col, s, group.cpu(), 16, c.G)
    with pytest.raises(sda.WgnnError, match="must be positive"):
        ops.group_gene_reduce(rp, col, s, group, 0, c.G)
    with pytest.raises(sda.WgnnError, match="out must be"):
        ops.group_gene_reduce(rp, col, s, group, 16, c.G, out=(torch.zeros(16, c.G, device=DEV), torch.zeros(16, c.G, dtype=torch.int32, device=DEV)))
    total, count = ops.group_gene_reduce(rp, col, s, group, 16, c.G)       # and the next call runs
    assert np.array_equal(count.cpu().numpy(), M.reduce(c.rowptr, c.col, c.lat, c.group, 16, c.G)[1])


# ------------------------------------------------------------------------------------------------
# 10. / 11. the predictor end to end
# ------------------------------------------------------------------------------------------------
def _batch(G, n=300, seed=7):
    batch = sp.random(n, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    batch.data = (1.0 + np.round(16.0 * batch.data) / 4.0).astype(np.float32)       # quarters: exact through a CSV file
    batch.sort_indices()
    return batch


def _check_table(table, batch, att, group, names, n_layers, hidden):
    """``table`` against the reference fed with explain's own device scores, labels, base and logit."""
    K, G = len(names), batch.shape[1]
    scores = att.scores.cpu().numpy()
    want_s, want_c, mag = M.reduce(batch.indptr, batch.indices, scores, group, K, G)
    n_cells, n_skipped, base_sum, logit_sum = M.group_stats(group, att.base, att.logit, K)
    assert list(table.group_names) == list(names) and len(table.id2gene) == G
    np.testing.assert_array_equal(table.n_cells, n_cells)
    assert table.n_cells.dtype == np.int64 and table.n_skipped == n_skipped
    assert np.array_equal(table.expr_count.cpu().numpy(), want_c)
    got = table.score_sum.cpu().numpy()
    err, bound = np.abs(got - want_s), M.bound(want_c, mag)
    assert (err <= bound).all()
    np.testing.assert_array_equal(table.base_sum, base_sum)
    np.testing.assert_array_equal(table.logit_sum, logit_sum)
    # the identity: per cell explain's own completeness bound (one per layer, as its test takes it), summed over the group,
    # plus the fp64 roundings: the bins' additions, then G + n terms summed in fp64 (score_sum[k].sum(), base, logit)
    rows = np.repeat(np.arange(batch.shape[0]), np.diff(batch.indptr))
    deg = np.diff(batch.indptr).astype(np.float64)
    per_cell = n_layers * R.completeness_bound(scores.astype(np.float64), att.base.astype(np.float64), rows, deg, hidden)
    on = group >= 0
    cells_bound = np.bincount(group[on], weights=per_cell[on], minlength=K)
    fp64 = bound.sum(1) + (G + n_cells + 2) * M.U64 * (mag.sum(1) + np.bincount(group[on], weights=np.abs(att.base)[on], minlength=K)
                                                       + np.bincount(group[on], weights=np.abs(att.logit)[on], minlength=K))
    gap = np.abs(got.sum(1) + table.base_sum - table.logit_sum)
    limit = cells_bound + fp64
    ratio_s = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    ratio_i = float((gap[limit > 0] / limit[limit > 0]).max())
    print(f"L={n_layers} H={hidden} K={K}: score_sum worst ratio {ratio_s:.2e}, identity worst |gap| / bound {ratio_i:.3f}")
    assert (gap <= limit).all()
    return ratio_s, ratio_i


@pytest.mark.parametrize("n_layers,hidden", [(1, 200), (2, 200), (1, 18), (2, 18)])
def test_markers_end_to_end(tmp_path, n_layers, hidden):
    root, G = _random_bundle(tmp_path, n_layers, hidden=hidden, seed=n_layers + hidden)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    batch = _batch(G)
    att = rp.explain(batch, top_k=0)
    table = rp.markers(batch)
    assert isinstance(table, sda.MarkerTable) and table.score_sum.is_cuda
    _check_table(table, batch, att, att.label, rp.id2label, n_layers, hidden)
    assert table.n_cells.sum() + table.n_skipped == batch.shape[0]
    # explain is untouched: the same bits before and after
    assert torch.equal(rp.explain(batch, top_k=0).scores, att.scores)
    # user-supplied groups (clusters with -1s), by count and by name; a fixed class as target
    rng = np.random.default_rng(n_layers)
    ids = rng.integers(-1, 7, batch.shape[0])
    _check_table(rp.markers(batch, groups=ids, n_groups=7), batch, att, ids, [str(i) for i in range(7)], n_layers, hidden)
    names = [f"cluster{i}" for i in range(7)]
    att3 = rp.explain(batch, top_k=0, target=3)
    tab3 = rp.markers(batch, groups=torch.from_numpy(ids), group_names=names, target=3)
    _check_table(tab3, batch, att3, ids, names, n_layers, hidden)
    _check_table(rp.markers(batch, target="type3"), batch, att3, att3.label, rp.id2label, n_layers, hidden)
    # a device triple gives the same bits
    dev_csr = (t(batch.indptr.astype(np.int64)), t(batch.indices), t(batch.data))
    same = rp.markers(dev_csr)
    assert torch.equal(same.score_sum, table.score_sum) and torch.equal(same.expr_count, table.expr_count)
    with pytest.raises(ValueError, match="group_names or n_groups"):
        rp.markers(batch, groups=ids)
    with pytest.raises(ValueError, match="groups lists"):
        rp.markers(batch, groups=ids[:-1], n_groups=7)
    with pytest.raises(ValueError, match="out of range"):
        rp.markers(batch, groups=ids, n_groups=6)
    with pytest.raises(ValueError, match="into"):
        rp.markers(batch, groups=ids, n_groups=7, into=table)


def test_markers_stream_into_one_table(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=20, seed=9)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    batch = _batch(G, 301, 11)
    whole = rp.markers(batch)
    att = rp.explain(batch, top_k=0)
    table = None
    for lo, hi in ((0, 100), (100, 101), (101, 301)):
        got = rp.markers(batch[lo:hi], into=table)
        assert table is None or got is table
        table = got
    np.testing.assert_array_equal(table.n_cells, whole.n_cells)
    assert table.n_skipped == whole.n_skipped and torch.equal(table.expr_count, whole.expr_count)
    _, want_c, mag = M.reduce(batch.indptr, batch.indices, att.scores.cpu().numpy(), att.label, rp.n_classes, G)
    err = (table.score_sum - whole.score_sum).abs().cpu().numpy()
    assert (err <= 2 * M.bound(want_c, mag)).all()              # each of the two is within the bound of the exact sum
    np.testing.assert_allclose(table.logit_sum, whole.logit_sum, rtol=1e-14)


def test_markers_files(tmp_path):
    root, G = _random_bundle(tmp_path, 1, seed=4)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    parts = [_batch(G, 60, 31), _batch(G, 45, 32)]
    files = []
    for i, part in enumerate(parts):
        f = tmp_path / f"part{i}_data.csv"
        pd.DataFrame(part.toarray().T, index=rp.id2gene, columns=[f"P{i}_C{j}" for j in range(part.shape[0])]).to_csv(f)
        files.append(f)
    out = rp.markers_files(files, top_k=5, save_path=tmp_path / "out")
    assert list(out.columns) == ["cell_type", "n_cells", "rank", "gene", "mean_score", "fraction"]
    saved = tmp_path / "out" / "mouse_Rand_markers.csv"
    assert saved.exists() and len(pd.read_csv(saved)) == len(out)
    stacked = sp.vstack(parts).tocsr()
    want = rp.markers(stacked)
    table = None
    for part in parts:
        table = rp.markers(part, into=table)
    f = table.frame(5)
    assert out["cell_type"].tolist() == f["group"].tolist() and out["gene"].tolist() == f["gene"].tolist()
    np.testing.assert_array_equal(out["mean_score"].to_numpy(), f["mean_score"].to_numpy())
    np.testing.assert_array_equal(table.n_cells, want.n_cells)
    assert torch.equal(table.expr_count, want.expr_count)
    att = rp.explain(stacked, top_k=0)
    _, want_c, mag = M.reduce(stacked.indptr, stacked.indices, att.scores.cpu().numpy(), att.label, rp.n_classes, G)
    err = (table.score_sum - want.score_sum).abs().cpu().numpy()
    assert (err <= 2 * M.bound(want_c, mag)).all()              # each of the two is within the bound of the exact sum


# ------------------------------------------------------------------------------------------------
# 12. ranking
# ------------------------------------------------------------------------------------------------
def _table_of(c, scores):
    total, count = ops.group_gene_reduce(*_operands(c)[:2], t(scores), t(c.group), c.K, c.G)
    n_cells = np.bincount(c.group[c.group >= 0], minlength=c.K).astype(np.int64)
    return sda.MarkerTable(group_names=[f"g{i}" for i in range(c.K)], id2gene=[f"Gene{i}" for i in range(c.G)], n_cells=n_cells,
                           n_skipped=int((c.group < 0).sum()), score_sum=total, expr_count=count, base_sum=np.zeros(c.K),
                           logit_sum=np.zeros(c.K)), n_cells


@pytest.mark.parametrize("min_fraction", [0.0, 0.1])
def test_top_and_frame_against_the_reference_ranking(min_fraction):
    c = M.ranking_case()
    k = 20
    want_s, want_c, _ = M.reduce(c.rowptr, c.col, c.flt, c.group, c.K, c.G)
    n_cells = np.bincount(c.group[c.group >= 0], minlength=c.K)
    ranked = M.ranking(want_s, want_c, n_cells, min_fraction)
    clear, exists = M.clear_pairs(ranked, k)
    left_out = int((exists & ~clear).sum())
    print(f"min_fraction={min_fraction}: {left_out} of {int(exists.sum())} (group, rank) pairs left out")
    assert left_out <= 0.02 * exists.sum() and exists.sum() >= 0.5 * c.K * k      # on the reference alone, first
    table, _ = _table_of(c, c.flt)
    genes, scores = table.top(k, min_fraction)
    assert genes.shape == (c.K, k) == scores.shape
    for g, (order, key) in enumerate(ranked):
        n = min(k, len(order))
        assert (genes[g, n:] == -1).all() and (scores[g, n:] == 0).all()
        ok = clear[g, :n]
        np.testing.assert_array_equal(genes[g, :n][ok], order[:n][ok])
        np.testing.assert_allclose(scores[g, :n][ok], key[:n][ok], rtol=2.0 ** -22)
    f = table.frame(k, min_fraction)
    assert list(f.columns) == ["group", "n_cells", "rank", "gene", "mean_score", "fraction"]
    assert len(f) == int((genes >= 0).sum())
    assert f["gene"].tolist() == [f"Gene{j}" for j in genes[genes >= 0]]
    assert (f["fraction"] >= min_fraction).all() and (f["fraction"] > 0).all()
    with pytest.raises(ValueError, match="64"):
        table.top(65)


def test_top_breaks_exact_ties_by_the_lower_gene_id():
    """Constructed: lattice scores from a handful of values, so that many genes of a group share one mean exactly."""
    rng = np.random.default_rng(77)
    c = M.ranking_case()
    scores = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), len(c.col))
    c.group = (np.arange(c.B) % 4).astype(np.int32)               # 100 cells per group: a power-of-two-free divisor is fine,
    c.K = 4                                                      # equal sums still give equal means
    want_s, want_c, _ = M.reduce(c.rowptr, c.col, scores, c.group, c.K, c.G)
    ranked = M.ranking(want_s, want_c, np.bincount(c.group, minlength=4))
    table, _ = _table_of(c, scores)
    genes, top = table.top(64)
    ties = 0
    for g, (order, key) in enumerate(ranked):
        np.testing.assert_array_equal(genes[g], order[:64])       # no pair left out
        np.testing.assert_array_equal(top[g], key[:64])
        ties += int((key[:63] == key[1:64]).sum())
    assert ties >= 20                                             # the case does hold exact ties


# ------------------------------------------------------------------------------------------------
# 13. pinned to logits of the reference's own code
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refcode_1layer", "refcode_predict"])
def test_group_sums_add_up_to_executed_reference_logits(name):
    """Set up as test_attribution_sums_to_executed_reference_logits (layer 1 in explicit-self mode, the self rows' share next
    to ``base``); cells grouped by the fixture's own arg max."""
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    mask = z["support_mask"].astype(bool)
    L = int(z["n_layers"])
    feats = torch.from_numpy(z["feats"]).to(DEV)
    test = sp.csr_matrix(expr[~mask])
    test.sort_indices()
    rp, col, raw = _device_csr(test, False)
    B = test.shape[0]
    alpha = sd["alpha"].reshape(-1)
    W1, b1 = sd["layers.0.fc_neigh.weight"], sd["layers.0.fc_neigh.bias"]
    test_ids = torch.from_numpy(np.nonzero(~mask)[0]).to(DEV)
    table1 = ops.linear_fwd(feats[:G].contiguous(), W1)
    self1 = ops.linear_fwd(feats[G + test_ids].contiguous(), W1)
    head = (sd["linear.weight"], sd["linear.bias"])
    n_cls = head[0].shape[0]
    back = (alpha[G + 1] / ((rp[1:] - rp[:-1]).float() + 1.0))[:, None]
    want = z["logits"][~mask].astype(np.float64)
    group = want.argmax(1).astype(np.int32)
    n_cells = np.bincount(group, minlength=n_cls)
    dev_group = t(group)
    with torch.no_grad():
        if L == 2:
            h1 = ops.predict_rows(rp, col, raw, table1, alpha, b1, self_rows=self1)
            m = sda.GNN(int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), L, G, activation=F.relu).to(DEV)
            m.load_state_dict({k: v for k, v in sd.items()})
            m.eval()
            g = sda.CellGeneGraph.from_expression(expr, mask, device=DEV)
            h_g, _ = m._layer(g, m.layers[0], feats[:G], feats[G:], want_genes=True, cell_rows=None)
            W2, b2 = sd["layers.1.fc_neigh.weight"], sd["layers.1.fc_neigh.bias"]
            table2 = ops.linear_fwd(h_g[:, :W2.shape[1]].contiguous(), W2)
        worst = 0.0
        for cls in range(n_cls):
            target = torch.full((B,), cls, dtype=torch.int32, device=DEV)
            if L == 1:
                score, _, logit, base, _, v = ops.attrib_rows(rp, col, raw, table1, alpha, b1, self_rows=self1, head=head,
                                                              target=target, want_direction=True)
            else:
                score, _, logit, base, _, v2 = ops.attrib_rows(rp, col, raw, table2, alpha, b2, head=head, target=target,
                                                               self_rows=ops.linear_fwd(h1, W2), want_direction=True)
                v = (h1 > 0) * ops.linear_fwd(v2.contiguous(), W2.t().contiguous()) * back
                base = base + (v * b1).sum(1)
                ops.attrib_rows(rp, col, raw, table1, alpha, b1, direction=v, scores=score, accumulate=True, explicit_self=True)
            share = back[:, 0] * (self1 * v).sum(1)
            total, count = ops.group_gene_reduce(rp, col, score, dev_group, n_cls, G)
            rest = (base.double() + share.double()).cpu().numpy()
            got = total.sum(1).cpu().numpy() + np.bincount(group, weights=rest, minlength=n_cls)
            ref = np.bincount(group, weights=want[:, cls], minlength=n_cls)
            gap = np.abs(got - ref)
            worst = max(worst, float((gap / np.maximum(1e-5 * n_cells, 1e-300)).max()))
            assert (gap <= 1e-5 * n_cells).all(), (cls, gap, n_cells)
            assert int(count.sum()) == int(np.diff(test.indptr).sum())
    print(f"{name}: worst |group sum - reference| / (1e-5 n_cells) = {worst:.3f}")
