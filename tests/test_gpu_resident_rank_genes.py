"""``ResidentPredictor.rank_genes`` end to end on a random bundle: the integer tables exactly the ``rankdata`` reference's
(tests/rank_genes_reference.py) on the aligned batch, ``z`` / ``p`` / ``auc`` bit for bit its host step, ``label`` bit for bit
``classify``'s - over the bundle's own gene ids with the predicted types as groups, and over the caller's shuffled columns with
``normalize="lognorm"`` and groups given per cell; the pairwise recipe against ``scipy.stats.mannwhitneyu``; the refusals;
``compare`` against ``markers`` of the same batch; ``rank_genes_file``.

``mean`` / ``logfc`` carry fp64 sums of f32 values, which ``wgnn_group_gene_reduce`` adds in its own order: they are held to the
bound test_gpu_resident_markers.py applies to ``score_sum`` (markers_reference.bound: n - 1 additions, each rounding a partial
sum of magnitude <= mag by 2^-53), carried through the division by the group's cells (one more rounding on either side) and,
for ``logfc = f(mean) - f(mean_rest)`` with ``f(m) = log2(expm1(m) + 1e-9)``, through ``|f'(m)| = e^m / ((expm1(m) + 1e-9) ln 2)``
plus the roundings of ``expm1``, the quotient and ``log2`` themselves (a relative 2^-53 each inside the logarithm is an absolute
2^-53 / ln 2 outside, so 8 x 2^-53 absolute and 4 x 2^-53 relative cover both sides)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
from scipy.stats import mannwhitneyu

import scdeepsort_amd as sda

import markers_reference as M
import rank_genes_reference as R
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B = 300
U64 = 2.0 ** -53
COLUMNS = ["group", "rank", "gene", "z", "auc", "logfc", "p", "p_adj", "fraction", "fraction_rest", "mean"]


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    return _random_bundle(tmp_path_factory.mktemp("rank_genes"), 2, hidden=12, seed=41)


def _host(csr):
    rowptr, col, val = (x.cpu().numpy() for x in csr)
    return rowptr.astype(np.int64), col, val


def _check(out, csr, group, names):
    """``out`` against the reference on the host CSR ``csr`` with one group id per cell."""
    rowptr, col, val = csr
    K, G = len(names), len(out.id2gene)
    group = np.asarray(group, np.int64)
    r2, count, tie, size = R.tables(rowptr, col, val, group, K, G)
    assert list(out.group_names) == list(names) and out.n_skipped == int((group < 0).sum())
    for got, want, dt in ((out.rank2_sum, r2, np.int64), (out.expr_count, count, np.int32), (out.tie_sum, tie, np.int64),
                          (out.n_cells, size, np.int64)):
        assert got.dtype == dt
        np.testing.assert_array_equal(got, want)
    U, auc, z, p = R.host_stats(r2, tie, size)
    for got, want in ((out.u(), U), (out.auc(), auc), (out.z(), z), (out.pvals(), p)):
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)      # the reference's host step, bit for bit
    adj = out.pvals_adj()
    for k in range(K):
        if size[k] and size[k] < size.sum():
            assert np.array_equal(adj[k], R.benjamini_hochberg(p[k]))
        else:
            assert np.isnan(adj[k]).all() and np.isnan(z[k]).all()
    # means and logfc: markers' bound on the sums (module docstring)
    want_s, want_c, mag = M.reduce(rowptr, col, val, group, K, G)
    np.testing.assert_array_equal(want_c, count)
    n1 = size.astype(np.float64)[:, None]
    n2 = n1.sum() - n1
    on = (size > 0) & (size < size.sum())
    assert on.sum() >= 2
    b = M.bound(want_c, mag)
    rest_b = 2.0 * (b.sum(axis=0) + K * U64 * mag.sum(axis=0))[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean, rest = want_s / n1, (want_s.sum(axis=0)[None, :] - want_s) / n2
        err_mean, err_rest = b / n1 + 2 * U64 * np.abs(mean), rest_b / n2 + 2 * U64 * np.abs(rest)
        slope = lambda m: np.exp(m) / ((np.expm1(m) + 1e-9) * np.log(2.0))
        lf = np.log2((np.expm1(mean) + 1e-9) / (np.expm1(rest) + 1e-9))
        err_lf = slope(mean) * err_mean + slope(rest) * err_rest + 8 * U64 + 4 * U64 * np.abs(lf)
    worst = 0.0
    for got, want, err in ((out.mean, mean, err_mean), (out.mean_rest, rest, err_rest), (out.logfc(), lf, err_lf)):
        gap = np.abs(got[on] - want[on])
        worst = max(worst, float((gap[err[on] > 0] / err[on][err[on] > 0]).max(initial=0.0)))
        assert (gap <= err[on]).all()
    print(f"K={K}: mean / mean_rest / logfc worst |gap| / bound {worst:.3f}")
    np.testing.assert_array_equal(out.fraction()[on], (count[on] / n1[on]))
    return r2, count, tie, size


def test_predicted_types_over_the_bundles_gene_ids(bundle):
    root, G = bundle
    batch = sp.random(B, G, density=0.2, random_state=5, format="csr", dtype=np.float32)
    batch.data = np.log1p(np.ceil(batch.data * 6)).astype(np.float32)                  # six distinct values: ties everywhere
    batch.sort_indices()
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    # an unsure threshold between the batch's lowest top probability and the best one of a cell outside the commonest type:
    # some cells are skipped and two types stay
    label, prob, _ = rp.classify(batch)
    rare = label != np.bincount(label[label >= 0]).argmax()
    assert rare.any() and prob.min() < prob[rare].max()
    rate = 0.5 * (float(prob.min()) + float(prob[rare].max())) * len(rp.id2label)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=rate)
    label, prob, _ = rp.classify(batch)
    assert (label < 0).any() and len(np.unique(label[label >= 0])) >= 2
    out = rp.rank_genes(batch)
    assert isinstance(out, sda.GeneRanks)
    np.testing.assert_array_equal(out.label, label)
    np.testing.assert_array_equal(out.max_prob, prob)                                  # classify's own, bit for bit
    csr = (batch.indptr.astype(np.int64), batch.indices, batch.data)
    _check(out, csr, label, rp.id2label)
    assert list(out.index) == list(range(B)) and list(out.id2gene) == list(rp.id2gene)
    # a device CSR with int32 row pointers gives the same table
    dev_csr = tuple(torch.from_numpy(a).to(rp.device) for a in (batch.indptr.astype(np.int32), batch.indices, batch.data))
    again = rp.rank_genes(dev_csr, index=[f"c{i}" for i in range(B)])
    np.testing.assert_array_equal(again.rank2_sum, out.rank2_sum)
    np.testing.assert_array_equal(again.tie_sum, out.tie_sum)
    assert np.array_equal(again.mean, out.mean, equal_nan=True) and again.index[3] == "c3"
    f = out.frame(5)
    assert list(f.columns) == COLUMNS and set(f["group"]) <= set(rp.id2label) and f["rank"].max() <= 5
    assert "groups" in str(out.summary())
    # compare against markers() of the same batch: the same groups and genes, consistent counts
    c = out.compare(rp.markers(batch), k=10)
    assert c["group"].tolist() == list(rp.id2label)
    for row in c.itertuples():
        assert row.n_shared <= min(row.n_model, row.n_data) <= 10
        assert len(row.model_only) == row.n_model - row.n_shared and len(row.data_only) == row.n_data - row.n_shared
        union = row.n_model + row.n_data - row.n_shared
        assert (np.isnan(row.jaccard) and union == 0) or row.jaccard == row.n_shared / union
        assert not set(row.model_only) & set(row.data_only)
    data, _ = out.top(10)
    model, _ = rp.markers(batch).top(10)
    assert c["n_shared"].tolist() == [len(set(d[d >= 0]) & set(m[m >= 0])) for d, m in zip(data, model)]


def test_groups_per_cell_over_the_callers_columns_and_the_pairwise_recipe(bundle):
    root, G = bundle
    rng = np.random.default_rng(3)
    ids = rng.permutation(G)[:300]
    columns = [f"Gene{i}" for i in ids] + [f"NotAGene{i}" for i in range(20)]
    columns = [columns[i] for i in rng.permutation(len(columns))]
    counts = (rng.geometric(0.5, (B, len(columns))) * (rng.random((B, len(columns))) < 0.3)).astype(np.float32)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    aligned = _host(rp.align(counts, columns, normalize="lognorm"))
    clusters = R.groups_of(B, 7, seed=9)
    names = [f"cl{i}" for i in range(7)]
    out = rp.rank_genes(counts, groups=clusters, genes=columns, normalize="lognorm", group_names=names)
    assert out.label is None and out.max_prob is None
    _check(out, aligned, clusters, names)
    same = rp.rank_genes(counts, groups=torch.from_numpy(clusters), genes=columns, normalize="lognorm", n_groups=7)
    np.testing.assert_array_equal(same.rank2_sum, out.rank2_sum)
    assert list(same.group_names) == [str(i) for i in range(7)]
    # pairwise: cluster 3 against cluster 5, every other cell at -1 - scipy's own test on the two groups' columns
    pair = np.where(clusters == 3, 0, np.where(clusters == 5, 1, -1))
    two = rp.rank_genes(counts, groups=pair, genes=columns, normalize="lognorm", group_names=["cl3", "cl5"])
    _check(two, aligned, pair, ["cl3", "cl5"])
    rowptr, col, val = aligned
    x = np.zeros((B, G), np.float32)
    x[np.repeat(np.arange(B), np.diff(rowptr)), col] = val
    tol = max(16 * R.P_REL_MEASURED, 4 * np.finfo(np.float64).eps)
    seen = 0
    for g in np.unique(col)[:60]:
        want = mannwhitneyu(x[pair == 0, g], x[pair == 1, g], use_continuity=False, method="asymptotic")
        assert two.u()[0, g] == want.statistic
        if len(np.unique(x[pair >= 0, g])) > 1:
            assert abs(two.pvals()[0, g] - want.pvalue) <= tol * want.pvalue
            assert two.pvals()[1, g] == two.pvals()[0, g] and two.z()[1, g] == -two.z()[0, g]
            seen += 1
    assert seen >= 30


def test_refusals(bundle):
    root, G = bundle
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    batch = sp.random(20, G, density=0.2, random_state=1, format="csr", dtype=np.float32)
    ids = np.arange(20) % 3
    with pytest.raises(ValueError, match="predicted"):
        rp.rank_genes(batch, groups="clusters")
    with pytest.raises(ValueError, match="group_names or n_groups"):
        rp.rank_genes(batch, groups=ids)
    with pytest.raises(ValueError, match="group names"):
        rp.rank_genes(batch, groups=ids, group_names=["a", "b", "c"], n_groups=4)
    with pytest.raises(ValueError, match="no groups"):
        rp.rank_genes(batch, groups=ids, group_names=[])
    with pytest.raises(ValueError, match="the batch holds 20 cells"):
        rp.rank_genes(batch, groups=ids[:19], n_groups=3)
    with pytest.raises(ValueError, match="integer ids"):
        rp.rank_genes(batch, groups=ids.astype(np.float32), n_groups=3)
    with pytest.raises(ValueError, match="out of range"):
        rp.rank_genes(batch, groups=ids, n_groups=2)
    with pytest.raises(ValueError, match="out of range"):
        rp.rank_genes(batch, groups=ids - 2, n_groups=3)
    with pytest.raises(ValueError, match="normalize needs genes"):
        rp.rank_genes(batch, normalize="lognorm")
    with pytest.raises(ValueError, match="index names 3 cells"):
        rp.rank_genes(batch, index=["a", "b", "c"])
    with pytest.raises(ValueError, match="n_groups"):
        rp.rank_genes(batch, groups=ids, n_groups=4097)
    assert not hasattr(sda.GeneRanks, "_require_same")                                  # no into=: ranks do not add over batches
    out = rp.rank_genes(batch, groups=ids, n_groups=3)                                  # and the next call runs
    assert out.n_cells.tolist() == [7, 7, 6]


def test_rank_genes_file_writes_the_table(bundle, tmp_path):
    root, G = bundle
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    rng = np.random.default_rng(1)
    genes = [rp.id2gene[i] for i in rng.permutation(G)[:200]] + ["NotAGene0", "NotAGene1"]
    counts = (rng.geometric(0.5, (60, len(genes))) * (rng.random((60, len(genes))) < 0.3)).astype(np.float32)
    cells = [f"C{j}" for j in range(60)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    want = rp.rank_genes(counts, genes=genes, normalize="lognorm", index=cells).frame(8)
    out = rp.rank_genes_file(data, normalize="lognorm", top_k=8, save_path=tmp_path / "res")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_rank_genes.csv")
    assert list(out.columns) == ["cell_type"] + COLUMNS[1:] == list(written.columns) and len(written) == len(out) == len(want) > 0
    assert out["cell_type"].tolist() == want["group"].tolist() and out["gene"].tolist() == want["gene"].tolist()
    for c in ("z", "auc", "logfc", "p", "p_adj", "fraction", "fraction_rest", "mean"):
        np.testing.assert_array_equal(out[c], want[c])
        np.testing.assert_allclose(written[c], want[c], rtol=1e-12)
