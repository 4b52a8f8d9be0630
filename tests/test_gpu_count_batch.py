"""``ResidentPredictor._count_batch`` and the layer driver on the GPU: one preamble for every count-taking call - the batch is
resolved and uploaded once whatever form it comes in, the operand checks speak in the calling op's name, and chunking the cells of
``stability`` / ``panels`` changes no bit."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api

from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
B, N_IN, N_OUT = 7, 9, 3


@pytest.fixture(scope="module")
def predictors(tmp_path_factory):
    made = {}
    for n_layers in (1, 2):
        root, _ = _random_bundle(tmp_path_factory.mktemp(f"bundle{n_layers}"), n_layers, hidden=12, seed=31)
        made[n_layers] = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    return made


def _batch(rp):
    """7 cells over 12 caller columns in shuffled order, 9 of them bundle genes and 3 outside; small integer counts, cell 2
    empty, cell 4 with reads outside the bundle only."""
    rng = np.random.default_rng(5)
    genes = [rp.id2gene[i] for i in rng.permutation(rp.n_genes)[:N_IN]] + [f"Outside{i}" for i in range(N_OUT)]
    counts = (rng.integers(1, 9, (B, N_IN + N_OUT)) * (rng.random((B, N_IN + N_OUT)) < 0.7)).astype(np.float32)
    counts[2] = 0
    counts[4, :N_IN] = 0
    counts[4, N_IN:] = [3, 0, 5]
    perm = rng.permutation(N_IN + N_OUT)
    return counts[:, perm], [genes[j] for j in perm]


def _forms(counts):
    host = sp.csr_matrix(counts)
    triple = tuple(torch.from_numpy(a).cuda() for a in (host.indptr.astype(np.int64), host.indices, host.data))
    return {"dense": torch.from_numpy(counts), "scipy": host, "device": triple}


def test_count_batch_is_the_same_from_every_form(predictors):
    rp = predictors[1]
    counts, genes = _batch(rp)
    inside = np.array([g in rp._gene2id for g in genes])
    want_label, want_prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    first = None
    for name, form in _forms(counts).items():
        cb = rp._count_batch(form, genes, api.LogNormalize(), "doublets")
        np.testing.assert_array_equal(cb.lib.cpu().numpy(), counts.sum(axis=1).astype(np.int64), err_msg=name)
        np.testing.assert_array_equal(cb.rest.cpu().numpy(), counts[:, ~inside].sum(axis=1).astype(np.int64), err_msg=name)
        assert cb.lib.dtype == cb.rest.dtype == torch.int64
        np.testing.assert_array_equal(cb.pred, want_label, err_msg=name)
        np.testing.assert_array_equal(cb.label.cpu().numpy(), want_label, err_msg=name)
        assert cb.max_prob.dtype == np.float32
        np.testing.assert_array_equal(cb.max_prob, want_prob, err_msg=name)
        first = first or cb
        for got, want in zip(cb.csr, first.csr):
            assert torch.equal(got, want), name
    rowptr, col, cnt = (a.cpu().numpy() for a in first.csr)
    np.testing.assert_array_equal(np.diff(rowptr), (counts[:, inside] > 0).sum(axis=1))
    assert rowptr[3] == rowptr[2] and rowptr[5] == rowptr[4]                  # the empty cell; the cell with outside reads only
    ids = np.array([rp._gene2id.get(g, -1) for g in genes])
    r, c = np.nonzero(counts * inside)                                        # row-major: the caller's order within a cell
    np.testing.assert_array_equal(col, ids[c])
    np.testing.assert_array_equal(cnt, counts[r, c])
    bare = rp._count_batch(counts, genes, api.LogNormalize(), "pseudobulk", full_call=False)
    assert bare.pred is None and bare.max_prob is None and bare.label is None and torch.equal(bare.csr[2], first.csr[2])


def test_every_count_taking_call_resolves_the_batch_once(predictors, monkeypatch):
    rp = predictors[2]
    counts, genes = _batch(rp)
    calls, resolve = [], rp._caller_batch
    monkeypatch.setattr(rp, "_caller_batch", lambda *a: (calls.append(1), resolve(*a))[1])
    ring = np.stack([(np.arange(B) + 1) % B, (np.arange(B) + 2) % B], axis=1)
    ops = {"stability": lambda: rp.stability(counts, genes=genes, normalize="lognorm", thin="reads", n_draws=2),
           "panels": lambda: rp.panels(counts, panels={"half": genes[:6]}, genes=genes, normalize="lognorm", renormalize=True),
           "doublets": lambda: rp.doublets(counts, genes, normalize="lognorm", n_partners=2, across="any"),
           "ambient": lambda: rp.ambient(counts, genes, normalize="lognorm", n_draws=2),
           "smooth": lambda: rp.smooth(counts, genes, ring, normalize="lognorm"),
           "pseudobulk": lambda: rp.pseudobulk(counts, genes, ["a", "b", "a", "b", "a", "b", "a"], normalize="lognorm")}
    for name, op in ops.items():
        del calls[:]
        op()
        assert len(calls) == 1, name


def test_operand_errors_name_the_calling_op(predictors):
    rp = predictors[1]
    counts, genes = _batch(rp)
    ring = np.stack([(np.arange(B) + 1) % B], axis=1)
    bad = counts.copy(); bad[1, 0] = -1
    with pytest.raises(sda.WgnnError, match="^doublets: a count is negative, NaN or infinite"):
        rp.doublets(bad, genes, normalize="lognorm", across="any")
    with pytest.raises(sda.WgnnError, match="^smooth: a count is negative, NaN or infinite"):
        rp.smooth(bad, genes, ring, normalize="lognorm")
    deep = counts.copy()
    deep[3, int(np.flatnonzero([g in rp._gene2id for g in genes])[0])] = 2.0 ** 23 + 1
    with pytest.raises(sda.WgnnError, match="cell 3 holds a count above 2\\^23"):
        rp.doublets(deep, genes, normalize="lognorm", across="any")
    st = rp.stability(deep, genes=genes, normalize="lognorm", thin="reads", n_draws=2)        # its bound is 2^24
    assert st.n_reads[3] == deep[3].astype(np.int64).sum()


def _same_tables(x, y, names):
    for name in names:
        a, b = getattr(x, name), getattr(y, name)
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), name
        else:
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_three_launches_equal_one(predictors, monkeypatch):
    rp = predictors[2]
    counts, genes = _batch(rp)
    launches, layers, budget = [], rp._layers, api.STABILITY_CHUNK_BYTES
    monkeypatch.setattr(rp, "_layers", lambda *a, **kw: (launches.append(1), layers(*a, **kw))[1])
    per_unit = rp.hidden_padded * 4 * 3                                       # h, its self rows and the next h of one unit
    runs = {"stability": (4, ("label", "max_prob", "votes", "unsure", "empty", "conf_sum", "n_entries", "n_reads"),
                          lambda **kw: rp.stability(counts, keep=(0.5,), n_draws=4, seed=3, genes=genes, normalize="lognorm", **kw),
                          (dict(thin="genes"), dict(thin="reads"))),
            "panels": (2, ("label", "max_prob", "panel_label", "panel_prob", "n_entries", "n_reads"),
                       lambda **kw: rp.panels(counts, panels={"half": genes[:6]}, without={"rest": genes[:6]}, genes=genes,
                                              normalize="lognorm", **kw),
                       (dict(renormalize=False), dict(renormalize=True)))}
    for name, (n_units, fields, run, modes) in runs.items():
        for mode in modes:
            del launches[:]
            whole = run(**mode)
            assert len(launches) == 2, (name, mode)                           # the call as given, and one launch of all 7 cells
            monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", 3 * n_units * per_unit)             # 3 cells per launch: 3 + 3 + 1
            del launches[:]
            chunked = run(**mode)
            monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", budget)
            assert len(launches) == 4, (name, mode)
            _same_tables(chunked, whole, fields)
