"""``ResidentPredictor.signatures`` end to end on a random bundle, B = 64 cells: ``label`` / ``max_prob`` bit for bit
``classify``'s, ``score`` exactly the fp64 score of the ``rankdata`` reference (tests/signatures_reference.py) on the aligned
batch - over the bundle's own gene ids, and over the caller's shuffled columns with names outside the bundle, an alias and
``normalize="lognorm"``; merged columns (``duplicates="sum"``); 70 sets in two launches against two calls of 35; ``missing``;
``signatures_file``; and ``concordant`` / ``by_type`` on a batch whose answer is constructed."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda

import signatures_reference as S
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, N_SETS, MAX_RANK = 64, 70, 60


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    return _random_bundle(tmp_path_factory.mktemp("signatures"), 2, hidden=12, seed=31)


def _sets(names, n=N_SETS, seed=9):
    """``n`` sets of 0 to 50 of the gene names ``names``; two of them also list names that exist nowhere."""
    rng = np.random.default_rng(seed)
    sets = {f"set{i}": [names[j] for j in rng.choice(len(names), size=(5, 20, 50, 0, 33)[i % 5], replace=False)] for i in range(n)}
    sets["set1"] = sets["set1"] + ["Nowhere1", "Nowhere2"]
    sets["set3"] = ["Nowhere3"]
    return sets


def _host(csr):
    rowptr, col, val = (x.cpu().numpy() for x in csr)
    return rowptr.astype(np.int64), col, val


def _member(sets, lookup, G, columns=None):
    """bool [P, G] and the missing names, resolved independently of the predictor: ``lookup`` maps a name to its bundle gene or
    -1; with ``columns`` a name counts only through a caller's column (of that name, or of the bundle gene it resolves to)."""
    measured = None if columns is None else {lookup(c) for c in columns} - {-1}
    member, missing = np.zeros((len(sets), G), bool), {}
    for p, (name, genes) in enumerate(sets.items()):
        missing[name] = []
        for g in genes:
            gid = lookup(g)
            if columns is None:
                hit = gid >= 0
            else:
                hit = g in columns or gid in measured
                gid = gid if gid in measured else -1
            if not hit:
                missing[name].append(g)
            elif gid >= 0:
                member[p, gid] = True
    return member, missing


def _check(out, rp, csr, member, missing, classify, max_rank=MAX_RANK):
    label, prob, _ = classify
    np.testing.assert_array_equal(out.label, label)
    np.testing.assert_array_equal(out.max_prob, prob)                                  # classify's own, bit for bit
    rowptr, col, val = _host(csr)
    r2, present, score = S.rank_sets(rowptr, col, val, rp.n_genes, member, max_rank)
    assert out.score.dtype == np.float64 and out.score.shape == (B, member.shape[0])
    assert np.array_equal(out.score, score, equal_nan=True)                            # exactly the reference's fp64 score
    np.testing.assert_array_equal(out.n_present, present)
    np.testing.assert_array_equal(out.n_genes, np.diff(rowptr))
    np.testing.assert_array_equal(out.set_size, member.sum(axis=1))
    assert out.missing == missing and out.names == list(missing) and out.max_rank == max_rank
    assert np.isnan(out.score[:, member.sum(axis=1) == 0]).all() and np.nanmin(out.score) >= 0 and np.nanmax(out.score) <= 1


def test_over_the_bundles_gene_ids(bundle):
    root, G = bundle
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    batch = sp.random(B, G, density=0.25, random_state=5, format="csr", dtype=np.float32)
    batch.data = np.log1p(np.ceil(batch.data * 6)).astype(np.float32)                  # six distinct values: ties everywhere
    batch.sort_indices()
    sets = _sets(list(rp.id2gene))
    member, missing = _member(sets, lambda g: rp._gene2id.get(g, -1), G)
    assert missing["set1"] == ["Nowhere1", "Nowhere2"] and missing["set3"] == ["Nowhere3"] and not missing["set0"]
    csr = (torch.from_numpy(batch.indptr), torch.from_numpy(batch.indices), torch.from_numpy(batch.data))
    out = rp.signatures(batch, sets, max_rank=MAX_RANK)
    assert int(np.diff(batch.indptr).max()) > MAX_RANK                                 # the cap bites
    _check(out, rp, csr, member, missing, rp.classify(batch))
    # 70 sets are two launches: the same table as two calls of 35
    names = list(sets)
    halves = [rp.signatures(batch, {k: sets[k] for k in names[i:i + 35]}, max_rank=MAX_RANK) for i in (0, 35)]
    assert np.array_equal(np.concatenate([h.score for h in halves], axis=1), out.score, equal_nan=True)
    np.testing.assert_array_equal(np.concatenate([h.n_present for h in halves], axis=1), out.n_present)
    # a device CSR with int32 row pointers and the default max_rank, which no row reaches
    dev_csr = tuple(x.to(rp.device) for x in (csr[0].int(), csr[1], csr[2]))
    _check(rp.signatures(dev_csr, sets), rp, csr, member, missing, rp.classify(batch), max_rank=1500)
    assert len(out.frame()) == B and "max_rank 60" in str(out.summary())


def test_over_the_callers_columns_with_lognorm_an_alias_and_merged_columns(bundle):
    root, G = bundle
    rng = np.random.default_rng(3)
    ids = rng.permutation(G)[:300]
    columns = [f"Gene{i}" for i in ids[:280]] + [f"ENS{i}" for i in ids[280:]] + [f"NotAGene{i}" for i in range(20)]
    aliases = {f"ENS{i}": f"Gene{i}" for i in ids[280:]}
    columns = [columns[i] for i in rng.permutation(len(columns))]
    counts = (rng.geometric(0.5, (B, len(columns))) * (rng.random((B, len(columns))) < 0.3)).astype(np.float32)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2, aliases=aliases)
    lookup = lambda g: rp._gene2id.get(g, rp._gene2id.get(aliases.get(g), -1))
    # names of columns (aliases and strangers included), bundle names behind an alias, and bundle genes that are not measured
    pool = columns + [f"Gene{i}" for i in ids[280:290]] + [f"Gene{i}" for i in sorted(set(range(G)) - set(ids.tolist()))[:15]]
    sets = _sets(pool)
    member, missing = _member(sets, lookup, G, columns)
    assert any(g.startswith("Gene") for lost in missing.values() for g in lost)        # a bundle gene the caller did not measure
    aligned = rp.align(counts, columns, normalize="lognorm")
    out = rp.signatures(counts, sets, genes=columns, normalize="lognorm", max_rank=MAX_RANK)
    _check(out, rp, aligned, member, missing, rp.classify(counts, genes=columns, normalize="lognorm"))
    # what gene_map made of the names gives the same table (the sets then resolve through the bundle genes of the columns)
    by_map = rp.signatures(counts, sets, genes=rp.gene_map(columns, aliases), normalize="lognorm", max_rank=MAX_RANK)
    assert np.array_equal(by_map.score, out.score, equal_nan=True)

    # duplicates="sum": a gene measured under its name and under its alias; the two columns are added before the logarithm
    twice = columns + [f"Gene{i}" for i in ids[280:285]]
    more = np.concatenate([counts, rng.geometric(0.5, (B, 5)).astype(np.float32)], axis=1)
    rs = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2, aliases=aliases, duplicates="sum")
    merged = rs.align(more, twice, normalize="lognorm")
    out = rs.signatures(more, sets, genes=twice, normalize="lognorm", max_rank=MAX_RANK)
    _check(out, rs, merged, *_member(sets, lookup, G, twice), rs.classify(more, genes=twice, normalize="lognorm"))
    with pytest.raises(ValueError, match="normalize"):
        rs.signatures(more, sets, genes=twice)


def test_signatures_file_writes_the_table(bundle, tmp_path):
    root, G = bundle
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    rng = np.random.default_rng(1)
    genes = [rp.id2gene[i] for i in rng.permutation(G)[:200]] + ["NotAGene0", "NotAGene1"]
    counts = (rng.geometric(0.5, (30, len(genes))) * (rng.random((30, len(genes))) < 0.3)).astype(np.float32)
    cells = [f"C{j}" for j in range(30)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    sets = {"first": genes[:30], "second": genes[100:140] + ["Nowhere"], "third": genes[150:155]}
    gmt = tmp_path / "sets.gmt"
    gmt.write_text("".join(f"{k}\tno description\t" + "\t".join(v) + "\n" for k, v in sets.items()))
    expected = {rp.id2label[0]: "first", rp.id2label[1]: "third"}
    want = rp.signatures(counts, sets, genes=genes, normalize="lognorm", expected=expected, index=cells).frame()
    for given in (sets, gmt):
        out = rp.signatures_file(data, given, normalize="lognorm", expected=expected, save_path=tmp_path / "res")
        written = pd.read_csv(tmp_path / "res" / "mouse_Rand_signatures.csv")
        assert list(out.columns) == list(want.columns) == list(written.columns) and len(written) == len(out) == 30
        assert out["index"].tolist() == cells and out["best"].tolist() == want["best"].tolist()
        for c in ("score_first", "score_second", "score_third", "margin"):
            np.testing.assert_array_equal(out[c], want[c])
            np.testing.assert_allclose(written[c], want[c], rtol=1e-12)


def test_concordant_and_by_type_on_a_constructed_batch(bundle):
    root, G = bundle
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    rng = np.random.default_rng(8)
    # three disjoint modules of 20 genes; cell i expresses module i % 3 above everything else and the other modules below it
    modules = rng.permutation(G)[:60].reshape(3, 20)
    rest = np.setdiff1d(np.arange(G), modules.ravel())
    x = np.zeros((B, G), np.float32)
    for i in range(B):
        x[i, rng.choice(rest, 100, replace=False)] = rng.uniform(1.0, 2.0, 100)
        for m in range(3):
            x[i, modules[m]] = rng.uniform(5.0, 6.0, 20) if m == i % 3 else rng.uniform(0.1, 0.5, 20) * (rng.random(20) < 0.5)
    sets = {f"module{m}": [rp.id2gene[g] for g in modules[m]] for m in range(3)}
    label = rp.classify(sp.csr_matrix(x))[0]
    called = np.unique(label[label >= 0])
    assert len(called) >= 2                                                            # the random model makes several calls
    C = len(rp.id2label)
    of_type = {t: t % 3 for t in range(C - 1)}                                         # the last type has no expected set
    expected = {rp.id2label[t]: f"module{m}" for t, m in of_type.items()}
    # max_rank = 100: the own module holds the ranks 1 .. 20 (score 1), every other module's genes lie past the cap (score < 0.1)
    out = rp.signatures(sp.csr_matrix(x), sets, expected=expected, max_rank=100)
    np.testing.assert_array_equal(out.label, label)
    ids, margin = out.best()
    np.testing.assert_array_equal(ids, np.arange(B) % 3)                               # the cell's own module wins, clearly
    assert margin.min() > 0.8
    want = np.array([l in of_type and of_type[l] == i % 3 for i, l in enumerate(label.tolist())])
    assert want.any() and (~want & (label >= 0)).any()
    np.testing.assert_array_equal(out.concordant(), want)
    np.testing.assert_array_equal(out.concordant(0.8), want)
    assert not out.concordant(1.5).any()
    own = out.own()
    assert np.array_equal(np.isnan(own), np.array([l not in of_type for l in label.tolist()]))
    assert (own[want] == 1.0).all() and (own[~want & ~np.isnan(own)] < 0.2).all()
    t = out.by_type()
    assert t["cell_type"].tolist() == out._name(called) and t["n_cells"].tolist() == [int((label == c).sum()) for c in called]
    assert t["expected"].tolist() == [f"module{of_type[c]}" if c in of_type else None for c in called.tolist()]
    for row, c in zip(t.itertuples(), called.tolist()):
        if c in of_type:
            assert row.concordant == want[label == c].mean()
        else:
            assert np.isnan(row.concordant) and np.isnan(row.median_own)
    assert len(out.discordant()) == int((~want & np.isin(label, list(of_type))).sum())
    assert out.discordant()["index"].tolist() == np.flatnonzero(~want & np.isin(label, list(of_type))).tolist()
