"""CPU checks of per-cell gene attribution: the fp64 restatement (tests/attrib_reference.py) against fp64 autograd and its
completeness identity, the undecided-unit budget of the GPU test's batches, argument validation of ``wgnn_attrib_rows`` /
``wgnn_rows_topk`` (no launch), and the host logic of ``ResidentPredictor.explain`` / ``explain_file`` with the kernel
calls faked."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

import attrib_reference as R


# ------------------------------------------------------------------------------------------------
# 1. the restatement against autograd (gradient x input on the message weights) and completeness
# ------------------------------------------------------------------------------------------------
def _small_model(L, seed, G=60, H=8, n_cls=4, B=7):
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 20, B)
    lens[2] = 0                                               # an empty cell
    lens[4] = 1                                               # a one-gene cell
    rows = np.repeat(np.arange(B), lens)
    cols = np.concatenate([np.sort(rng.choice(G, int(n), replace=False)) for n in lens]).astype(np.int64)
    vals = np.clip(rng.normal(3.0, 1.0, cols.shape[0]), 0.2, 7.0)
    m = sp.csr_matrix((vals, (rows, cols)), shape=(B, G))
    tables = [rng.standard_normal((G, H)) for _ in range(L)]
    biases = [0.3 * rng.standard_normal(H) for _ in range(L)]
    Ws = [None] + [rng.standard_normal((H, H)) / np.sqrt(H) for _ in range(L - 1)]
    alpha = rng.uniform(0.5, 1.5, G + 2)
    return m, tables, alpha, biases, Ws, rng.standard_normal((n_cls, H)), 0.2 * rng.standard_normal(n_cls)


def _autograd_attribution(m, tables, alpha, biases, Ws, Wh, bh, target):
    """logit_t as a torch fp64 function of the per-layer message weights u_l; returns (sum_l u_l * dlogit/du_l, logits)."""
    G = m.shape[1]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    rows = torch.from_numpy(np.repeat(np.arange(m.shape[0]), np.diff(m.indptr)))
    cols = torch.from_numpy(m.indices.astype(np.int64))
    deg = t64(np.diff(m.indptr))
    us = [t64(R.message_weights(m, alpha, l > 0)[0]).requires_grad_() for l in range(len(tables))]
    h = None
    for l, u in enumerate(us):
        z = torch.zeros(m.shape[0], tables[l].shape[1], dtype=torch.float64).index_add(0, rows, u[:, None] * t64(tables[l])[cols])
        if l > 0:
            z = z + float(alpha[G + 1]) * (h @ t64(Ws[l]).T) / (deg + 1)[:, None]
        h = torch.relu(z + t64(biases[l]))
    logits = h @ t64(Wh).T + t64(bh)
    t = logits.argmax(1) if target is None else torch.from_numpy(np.asarray(target, np.int64))
    picked = logits[torch.arange(m.shape[0]), t]
    grads = torch.autograd.grad(picked.sum(), us)
    return sum((u * g).detach().numpy() for u, g in zip(us, grads)), logits.detach().numpy()


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("chosen", [False, True])
def test_reference_equals_autograd_and_is_complete(L, chosen):
    m, tables, alpha, biases, Ws, Wh, bh = _small_model(L, seed=10 * L + chosen)
    target = np.random.default_rng(L).integers(0, Wh.shape[0], m.shape[0]) if chosen else None
    ref = R.attribution(m, tables, alpha, biases, Ws, Wh, bh, target=target)
    want, logits = _autograd_attribution(m, tables, alpha, biases, Ws, Wh, bh, target)
    scale = np.abs(want).max()
    assert np.abs(ref.scores - want).max() <= 1e-12 * scale
    np.testing.assert_allclose(ref.logits, logits, rtol=1e-12, atol=1e-12)
    if chosen:
        np.testing.assert_array_equal(ref.target, target)
    total = np.bincount(ref.rows, weights=ref.scores, minlength=m.shape[0]) + ref.base
    assert np.abs(total - ref.logit).max() <= 1e-12 * max(1.0, np.abs(ref.logit).max())
    assert abs(ref.base[2] - ref.logit[2]) <= 1e-14 and not (ref.rows == 2).any()    # the empty cell: no phi, base is the logit
    assert np.diff(m.indptr)[4] == 1 and (ref.rows == 4).sum() == 1
    assert (ref.tol >= 0).all() and not any(u.any() for u in ref.undecided)     # nothing near a ReLU edge in fp64 terms


def test_reference_with_explicit_self_rows_on_the_first_layer():
    m, tables, alpha, biases, Ws, Wh, bh = _small_model(1, seed=5)
    sr = np.random.default_rng(6).standard_normal((m.shape[0], tables[0].shape[1]))
    ref = R.attribution(m, tables, alpha, biases, Ws, Wh, bh, self_rows0=sr)
    total = np.bincount(ref.rows, weights=ref.scores, minlength=m.shape[0]) + ref.base + ref.self_share
    assert np.abs(total - ref.logit).max() <= 1e-12 * max(1.0, np.abs(ref.logit).max())
    np.testing.assert_allclose(ref.scores, R.direction_scores(m, tables[0], alpha, ref.v[0], True), rtol=1e-13)


def test_stable_topk_reference():
    rowptr = np.array([0, 4, 4, 6])
    col = np.array([7, 3, 9, 1, 5, 2])
    s = np.array([1.0, 2.0, 2.0, -1.0, 0.5, 0.5], np.float32)
    g, t = R.stable_topk(rowptr, col, s, 3)
    np.testing.assert_array_equal(g, [[3, 9, 7], [-1, -1, -1], [5, 2, -1]])
    np.testing.assert_array_equal(t, np.array([[2, 2, 1], [0, 0, 0], [0.5, 0.5, 0]], np.float32))


# ------------------------------------------------------------------------------------------------
# 2. the undecided-unit budget of every batch the GPU kernel test uses
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,i64", R.KERNEL_CASES)
def test_undecided_unit_budget_of_the_gpu_cases(H, i64):
    c = R.kernel_case(H, i64)
    for explicit in (False, True):
        w, b = c.heads[(2, explicit)]
        ref = R.attribution(c.m, [c.table], c.alpha, [c.bias], [None], w, b, self_rows0=c.self_rows if explicit else None)
        und = ref.undecided[0]
        print(f"H={H} i64={i64} explicit={explicit}: undecided {int(und.sum())} of {und.size}, worst row {int(und.sum(1).max())}")
        assert und.sum() <= 1e-3 * c.B * H                   # at most 0.1 % of the batch's B * H units


# ------------------------------------------------------------------------------------------------
# 3. argument validation of the two entry points (no launch)
# ------------------------------------------------------------------------------------------------
def test_attrib_rows_validation_returns_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)      # fake, aligned, never dereferenced: validation happens first

    def call(rowptr=one, col=one, raw=one, B=4, table=one, ld=8, G=10, H=8, alpha=one, bias=one, self_rows=None, ld_self=0,
             w_head=one, b_head=one, C_=3, target=None, label=None, direction=None, ld_dir=0, score=one, target_out=one,
             logit_out=one, base_out=one, dir_out=None, ld_dir_out=0, flags=0):
        return lib.wgnn_attrib_rows(rowptr, col, raw, B, table, ld, G, H, alpha, bias, self_rows, ld_self, w_head, b_head, C_,
                                    target, 0.5, label, direction, ld_dir, score, target_out, logit_out, base_out, dir_out,
                                    ld_dir_out, flags, None)

    assert call(B=0) == 0                                   # empty batch: a no-op
    for k in ("rowptr", "col", "raw", "table", "alpha", "score", "bias", "b_head", "target_out", "logit_out", "base_out"):
        assert call(**{k: None}) == -1, k
    assert call(B=-1) == -1 and call(B=2 ** 31) == -1 and call(G=0) == -1 and call(H=0) == -1 and call(C_=0) == -1
    assert call(flags=_lib.FLAG_RELU) == -1 and call(flags=_lib.FLAG_ROWPTR_I64, B=0) == 0
    assert call(flags=_lib.ATTRIB_ACCUMULATE) == -1          # head mode overwrites
    assert call(H=6, ld=8) == -2
    assert b"multiple of 4" in lib.wgnn_last_error_string(-2)
    assert call(H=260, ld=260) == -3
    first = lib.wgnn_last_error_string(-3)
    assert b"wgnn_attrib_rows" in first and b"H > 256" in first
    assert lib.wgnn_last_error_string(-3) == b"unsupported dtype, feature width (D <= 1024 required) or nnz >= 2^31 (shard the cell axis)"
    assert call(ld=4) == -2 and call(table=C.c_void_p(20)) == -2 and call(self_rows=one, ld_self=4) == -2
    assert call(dir_out=one, ld_dir_out=4) == -2 and call(dir_out=one, ld_dir_out=8, B=0) == 0
    assert call(H=256, ld=256, C_=64, B=0) == 0 and call(H=256, ld=256, C_=65) == -3
    assert b"64 KiB" in lib.wgnn_last_error_string(-3)
    # direction mode: exactly one of head / direction
    assert call(direction=one, ld_dir=8) == -1 and call(w_head=None) == -1
    d = dict(w_head=None, direction=one, ld_dir=8, bias=None, b_head=None, target_out=None, logit_out=None, base_out=None)
    assert call(B=0, **d) == 0
    assert call(B=0, flags=_lib.ATTRIB_ACCUMULATE | _lib.ATTRIB_EXPLICIT_SELF | _lib.FLAG_ROWPTR_I64, **d) == 0
    assert call(**{**d, "ld_dir": 4}) == -2 and call(**{**d, "direction": C.c_void_p(24)}) == -2


def test_rows_topk_validation_returns_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)
    call = lambda rowptr=one, col=one, score=one, B=0, k=10, gene=one, top=one, flags=0: \
        lib.wgnn_rows_topk(rowptr, col, score, B, k, gene, top, flags, None)
    assert call() == 0 and call(flags=_lib.FLAG_ROWPTR_I64) == 0 and call(k=1) == 0 and call(k=64) == 0
    for k in ("rowptr", "col", "score", "gene", "top"):
        assert call(**{k: None}) == -1, k
    assert call(k=0) == -3 and call(k=65) == -3
    assert b"wgnn_rows_topk" in lib.wgnn_last_error_string(-3)
    assert call(B=-1) == -1 and call(flags=_lib.FLAG_RELU) == -1


def test_ops_attrib_wrappers_refuse_cpu_tensors_and_bad_modes():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    args = (rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, 8), torch.ones(5), torch.zeros(8))
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.attrib_rows(*args, head=(torch.zeros(2, 8), torch.zeros(2)))
    with pytest.raises(sda.WgnnError, match="either head"):
        sda.attrib_rows(*args)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.rows_topk(rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), 3)


# ------------------------------------------------------------------------------------------------
# 4. host logic of explain / explain_file with the kernel calls faked
# ------------------------------------------------------------------------------------------------
def _fake_predictor(monkeypatch, n_genes=6, n_classes=3, hidden=8):
    """A ResidentPredictor without a GPU: the fields explain reads, the batch kept on the host."""
    rp = api.ResidentPredictor.__new__(api.ResidentPredictor)
    rp.species, rp.tissue, rp.file_type, rp.threshold = "mouse", "Fake", "csv", 0
    rp.device = torch.device("cpu")
    rp.n_layers, rp.n_genes, rp.n_classes, rp.hidden, rp.hidden_padded = 1, n_genes, n_classes, hidden, hidden
    rp.id2gene = [f"G{i}" for i in range(n_genes)]
    rp.id2label = [f"type{i}" for i in range(n_classes)]
    rp._gene2id = {g: i for i, g in enumerate(rp.id2gene)}
    rp.unsure_threshold = 0.5
    rp.alpha = torch.ones(n_genes + 2)
    rp.tables, rp.biases, rp.self_weights = [torch.zeros(n_genes, hidden)], [torch.zeros(hidden)], [None]
    rp.w_head, rp.b_head = torch.zeros(n_classes, hidden), torch.zeros(n_classes)
    rp.bundle = SimpleNamespace(label_map=lambda: None)
    seen = {}

    def fake_attrib(rowptr, col, raw, table, alpha, bias, *, head, target, **kw):
        B = rowptr.shape[0] - 1
        seen["target"] = None if target is None else target.clone()
        t = torch.arange(B, dtype=torch.int32) % n_classes if target is None else target
        label = t.clone(); label[0] = -1                      # the first cell comes out unsure
        return raw.clone(), t, torch.ones(B), torch.full((B,), 0.25), label, None

    def fake_topk(rowptr, col, scores, k):
        gene, top = R.stable_topk(rowptr.numpy(), col.numpy(), scores.numpy(), k)
        return torch.from_numpy(gene.astype(np.int32)), torch.from_numpy(top)

    monkeypatch.setattr(ops, "attrib_rows", fake_attrib)
    monkeypatch.setattr(ops, "rows_topk", fake_topk)
    monkeypatch.setattr(api.ResidentPredictor, "explain", lambda self, expr, top_k=10, target="predicted":
                        self._explain(expr, top_k, target))      # without the device context of the real entry
    return rp, seen


def test_explain_host_logic_with_faked_kernels(monkeypatch, tmp_path):
    rp, seen = _fake_predictor(monkeypatch)
    X = sp.csr_matrix(np.array([[0, 2, 0, 5, 1, 0], [0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 4.5]], np.float32))
    att = rp.explain(X, top_k=4)
    assert isinstance(att, sda.Attribution) and seen["target"] is None
    assert att.label.tolist() == [-1, 1, 2] and att.target.tolist() == [0, 1, 2]
    assert att.top_genes.shape == (3, 4) and att.top_scores.shape == (3, 4) and att.scores.shape == (X.nnz,)
    np.testing.assert_array_equal(att.top_genes, [[3, 1, 4, -1], [-1, -1, -1, -1], [5, 0, -1, -1]])     # -1 padding
    np.testing.assert_array_equal(att.top_scores, np.array([[5, 2, 1, 0], [0, 0, 0, 0], [4.5, 3, 0, 0]], np.float32))
    assert att.gene_names(0) == ["G3", "G1", "G4"] and att.gene_names(1) == [] and att.gene_names(2) == ["G5", "G0"]
    assert att.base.tolist() == [0.25] * 3 and att.logit.tolist() == [1.0] * 3
    # target parsing: a class id, a label string, one id per cell
    rp.explain(X, target=2); assert seen["target"].tolist() == [2, 2, 2] and seen["target"].dtype == torch.int32
    rp.explain(X, target="type1"); assert seen["target"].tolist() == [1, 1, 1]
    rp.explain(X, target=np.array([2, 0, 1])); assert seen["target"].tolist() == [2, 0, 1]
    assert rp.explain(X, top_k=0).top_genes.shape == (3, 0)
    for bad in (3, -1, "type9", [0, 1], np.array([0, 1, 5])):
        with pytest.raises(ValueError):
            rp.explain(X, target=bad)
    with pytest.raises(ValueError):
        rp.explain(X, top_k=65)
    with pytest.raises(ValueError, match="gene columns"):
        rp.explain(sp.csr_matrix((2, 5), dtype=np.float32))
    # widths the kernel does not build
    rp.hidden, rp.hidden_padded = 300, 300
    with pytest.raises(sda.WgnnError, match="UNSUPPORTED"):
        rp.explain(X)
    rp.hidden, rp.hidden_padded, rp.n_classes = 256, 256, 65
    with pytest.raises(sda.WgnnError, match="UNSUPPORTED"):
        rp.explain(X)


def test_explain_file_frame_with_faked_kernels(monkeypatch, tmp_path):
    rp, _ = _fake_predictor(monkeypatch)
    X = np.array([[0, 2, 0, 5, 1, 0], [0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 4.5]], np.float32)
    data = tmp_path / "mouse_Fake7_data.csv"
    pd.DataFrame(X.T, index=rp.id2gene + [], columns=["c0", "c1", "c2"]).to_csv(data)
    out = rp.explain_file(data, top_k=2, save_path=tmp_path / "res")
    assert list(out.columns) == ["index", "cell_type", "rank", "gene", "score"]
    assert out["index"].tolist() == ["c0", "c0", "c2", "c2"]                  # the cell without genes has no rows
    assert out["cell_type"].tolist() == ["unsure", "unsure", "type2", "type2"]
    assert out["rank"].tolist() == [1, 2, 1, 2] and out["gene"].tolist() == ["G3", "G1", "G5", "G0"]
    assert out["score"].tolist() == [5.0, 2.0, 4.5, 3.0]
    saved = pd.read_csv(tmp_path / "res" / "mouse_Fake_mouse_Fake7_data_genes.csv")
    assert list(saved.columns) == list(out.columns) and len(saved) == 4
