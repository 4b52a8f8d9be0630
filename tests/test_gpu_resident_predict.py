"""ResidentPredictor and its kernel ``wgnn_predict_rows`` on the GPU: the kernel against an fp64 restatement of its formulas,
pinned to logits the reference's own code produced, and equivalent to the existing predictor on fitted and demo bundles."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"


# ------------------------------------------------------------------------------------------------
# 1. the kernel against an fp64 restatement
# ------------------------------------------------------------------------------------------------
def _ragged_batch(rng, B, G, long_row=5000):
    """Ragged raw-value CSR: two empty rows, one row longer than 4096 entries, the rest 1 .. 300 genes."""
    lens = rng.integers(1, 300, B)
    lens[1] = 0
    lens[B - 2] = 0
    lens[3] = long_row
    rows, cols = [], []
    for r, n in enumerate(lens):
        cols.append(np.sort(rng.choice(G, size=int(n), replace=False)))
        rows.append(np.full(int(n), r))
    cols = np.concatenate(cols); rows = np.concatenate(rows)
    vals = np.clip(rng.normal(3.0, 1.0, cols.shape[0]), 0.2, 7.0).astype(np.float32)
    return sp.csr_matrix((vals, (rows, cols)), shape=(B, G))


def _ref_layer(m, table, alpha, bias, self_rows=None):
    """z = sum_g coef_g table[g] / (deg + 1) + b in fp64 (include/wgnn.h, wgnn_predict_rows), then ReLU."""
    G = table.shape[0]
    m = m.tocsr()
    deg = np.diff(m.indptr).astype(np.float64)
    s = np.asarray(m.sum(axis=1)).ravel().astype(np.float64)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    x = m.data.astype(np.float64)
    a = alpha.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = a[m.indices] * deg[rows] * x / s[rows]
        if self_rows is None:
            coef = coef + x * a[G + 1] / (s[rows] + 1e-6)
    M = sp.csr_matrix((coef, m.indices, m.indptr), shape=m.shape)
    acc = M @ table.astype(np.float64)
    if self_rows is not None:
        acc = acc + a[G + 1] * self_rows.astype(np.float64)
    return np.maximum(acc / (deg + 1)[:, None] + bias.astype(np.float64), 0.0)


def _ref_head(h, w, b):
    logits = h @ w.astype(np.float64).T + b.astype(np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return logits, 1.0 / e.sum(axis=1)


def _device_csr(m, i64):
    rp = torch.from_numpy(m.indptr.astype(np.int64 if i64 else np.int32)).to(DEV)
    return rp, torch.from_numpy(m.indices.astype(np.int32)).to(DEV), torch.from_numpy(m.data.astype(np.float32)).to(DEV)


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("H", [12, 16, 64, 200, 256])
def test_kernel_matches_fp64_restatement(H, i64):
    rng = np.random.default_rng(H * 2 + i64)
    G, B = 6000, 40
    m = _ragged_batch(rng, B, G)
    table = (0.5 * rng.standard_normal((G, H))).astype(np.float32)
    alpha = rng.uniform(0.5, 1.5, G + 2).astype(np.float32)
    bias = (0.1 * rng.standard_normal(H)).astype(np.float32)
    self_rows = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    rp, col, raw = _device_csr(m, i64)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for C_ in (2, 5, 16, 40):
        for explicit in (False, True):
            sr = self_rows if explicit else None
            want_h = _ref_layer(m, table, alpha, bias, sr)
            scale = max(1.0, float(np.abs(want_h).max()))
            # without a head: ReLU(z)
            got_h = ops.predict_rows(rp, col, raw, t(table), t(alpha), t(bias), self_rows=None if sr is None else t(sr))
            assert got_h.shape == (B, H)
            assert float(np.abs(got_h.cpu().numpy() - want_h).max()) <= 1e-5 * scale, (C_, explicit)
            if sr is None:                                   # an empty row is ReLU(b), exactly
                np.testing.assert_array_equal(got_h.cpu().numpy()[1], np.maximum(bias, 0))
            # with the fused head
            w = (rng.standard_normal((C_, H)) / np.sqrt(H)).astype(np.float32)
            b = (0.1 * rng.standard_normal(C_)).astype(np.float32)
            want_l, want_p = _ref_head(want_h, w, b)
            thr = float(np.float32(np.median(want_p)))
            run = lambda: ops.predict_rows(rp, col, raw, t(table), t(alpha), t(bias), self_rows=None if sr is None else t(sr),
                                           head=(t(w), t(b)), unsure_threshold=thr)
            logits, label, max_prob = run()
            lscale = max(1.0, float(np.abs(want_l).max()))
            assert float(np.abs(logits.cpu().numpy() - want_l).max()) <= 1e-5 * lscale, (C_, explicit)
            assert float(np.abs(max_prob.cpu().numpy() - want_p).max()) <= 1e-5
            srt = np.sort(want_l, axis=1)
            gap = srt[:, -1] - srt[:, -2] if C_ > 1 else np.full(B, np.inf)
            clear = (gap > 1e-5) & (np.abs(want_p - thr) > 1e-5)
            want_label = np.where(want_p < thr, -1, want_l.argmax(axis=1))
            assert clear.sum() >= B // 2
            np.testing.assert_array_equal(label.cpu().numpy()[clear], want_label[clear])
            assert (label.cpu().numpy() == -1).any() and (label.cpu().numpy() >= 0).any()
            # deterministic: a second launch is bit-identical
            l2, lab2, p2 = run()
            assert torch.equal(l2, logits) and torch.equal(lab2, label) and torch.equal(p2, max_prob)


def test_kernel_labels_ties_by_lowest_index_and_checks_gene_ids():
    G, H = 50, 8
    m = sp.csr_matrix((np.ones(3, np.float32), ([0, 0, 1], [1, 2, 3])), shape=(2, G))
    rp, col, raw = _device_csr(m, False)
    table = torch.randn(G, H, device=DEV)
    alpha = torch.ones(G + 2, device=DEV)
    bias = torch.zeros(H, device=DEV)
    w = torch.zeros(4, H, device=DEV)                         # every logit equal: argmax = 0, max_prob = 1/4
    logits, label, p = ops.predict_rows(rp, col, raw, table, alpha, bias, head=(w, torch.zeros(4, device=DEV)),
                                        unsure_threshold=0.2)
    assert label.tolist() == [0, 0] and torch.allclose(p, torch.full_like(p, 0.25))
    bad = col.clone(); bad[1] = G
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.predict_rows(rp, bad, raw, table, alpha, bias)


# ------------------------------------------------------------------------------------------------
# 2. pinned to logits of the reference's own code (tests/golden/make_refcode_golden.py)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refcode_1layer", "refcode_predict"])
def test_kernel_matches_executed_reference_code(name):
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    mask = z["support_mask"].astype(bool)
    L = int(z["n_layers"])
    feats = torch.from_numpy(z["feats"]).to(DEV)
    test = sp.csr_matrix(expr[~mask])
    rp, col, raw = _device_csr(test, False)
    alpha = sd["alpha"].reshape(-1)
    W1, b1 = sd["layers.0.fc_neigh.weight"], sd["layers.0.fc_neigh.bias"]
    test_ids = torch.from_numpy(np.nonzero(~mask)[0]).to(DEV)
    # layer 1 in explicit-self mode: the features are random (not PCA), so the self rows are h0 . W1^T
    table1 = ops.linear_fwd(feats[:G].contiguous(), W1)
    self1 = ops.linear_fwd(feats[G + test_ids].contiguous(), W1)
    head = (sd["linear.weight"], sd["linear.bias"])
    with torch.no_grad():
        if L == 1:
            logits, _, _ = ops.predict_rows(rp, col, raw, table1, alpha, b1, self_rows=self1, head=head)
        else:
            h1 = ops.predict_rows(rp, col, raw, table1, alpha, b1, self_rows=self1)
            # the layer-2 gene table from the gene pass of the existing GNN over the fixture's graph
            m = sda.GNN(int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), L, G, activation=F.relu).to(DEV)
            m.load_state_dict({k: v for k, v in sd.items()})
            m.eval()
            g = sda.CellGeneGraph.from_expression(expr, mask, device=DEV)
            h_g, _ = m._layer(g, m.layers[0], feats[:G], feats[G:], want_genes=True, cell_rows=None)
            W2, b2 = sd["layers.1.fc_neigh.weight"], sd["layers.1.fc_neigh.bias"]
            table2 = ops.linear_fwd(h_g[:, :W2.shape[1]].contiguous(), W2)
            logits, _, _ = ops.predict_rows(rp, col, raw, table2, alpha, b2, self_rows=ops.linear_fwd(h1, W2), head=head)
    np.testing.assert_allclose(logits.cpu().numpy(), z["logits"][~mask], atol=1e-5)


# ------------------------------------------------------------------------------------------------
# 3. - 6. the predictor against the existing one
# ------------------------------------------------------------------------------------------------
def _write_dataset(tmp, name, n_cells, rng, genes, programs, extra_genes=(), empty_cell=False, with_types=True):
    types = rng.integers(0, len(programs), n_cells)
    X = np.zeros((len(genes), n_cells), np.float32)
    for j, t in enumerate(types):
        on = rng.random(len(genes)) < (0.05 + 0.6 * programs[t])
        X[on, j] = np.clip(rng.normal(3.0, 0.9, on.sum()), 0.5, 7.0)
    all_genes = list(genes)
    if extra_genes:                                           # genes the bundle does not know: dropped (preprocess.py:160-161)
        Xe = np.clip(rng.normal(3.0, 0.9, (len(extra_genes), n_cells)), 0.5, 7.0).astype(np.float32)
        X = np.vstack([X, Xe]); all_genes += list(extra_genes)
    if empty_cell:
        X[: len(genes), 0] = 0.0                              # expresses only genes outside the bundle (or none at all)
    cells = [f"{name}_C{j}" for j in range(n_cells)]
    data = tmp / f"{name}_data.csv"
    pd.DataFrame(X, index=all_genes, columns=cells).to_csv(data)
    if not with_types:
        return data, types
    ct = tmp / f"{name}_celltype.csv"
    pd.DataFrame({"Cell": cells, "Cell_type": [f"type{t} " for t in types]}).to_csv(ct)
    return data, ct, types


def _off_boundary(logits: np.ndarray, unsure_rate: float, tol: float) -> np.ndarray:
    p = torch.softmax(torch.from_numpy(logits).double(), 1).numpy()
    srt = np.sort(logits, axis=1)
    thr = unsure_rate / logits.shape[1]
    return (srt[:, -1] - srt[:, -2] > tol) & (np.abs(p.max(1) - thr) > tol)


@pytest.fixture(scope="module")
def demo_genes():
    genes = [f"G{i}" for i in range(120)]
    programs = [np.zeros(120) for _ in range(3)]
    for t in range(3):
        programs[t][t * 40:(t + 1) * 40] = 1.0
    return genes, programs


@pytest.mark.parametrize("n_layers,hidden", [(1, 12), (2, 12), (1, 20), (2, 20)])
def test_resident_predictor_equals_existing_predictor(tmp_path, monkeypatch, demo_genes, n_layers, hidden):
    genes, programs = demo_genes
    rng = np.random.default_rng(10 * n_layers + hidden)
    d1, c1, _ = _write_dataset(tmp_path, "mouse_Demo1", 240, rng, genes, programs)
    clf = sda.DeepSortClassifier("mouse", "Demo", dense_dim=16, hidden_dim=hidden, batch_size=64, n_epochs=15,
                                 n_layers=n_layers, learning_rate=0.005, random_seed=1, gpu_id=0)
    clf.fit([(d1, c1)], save_path=tmp_path / "bundle")
    files = [_write_dataset(tmp_path, "mouse_Demo11", 90, rng, genes, programs, with_types=False)[0],
             _write_dataset(tmp_path, "mouse_Demo12", 37, rng, genes, programs, extra_genes=["X1", "X2", "X3"],
                            empty_cell=True, with_types=False)[0],
             _write_dataset(tmp_path, "mouse_Demo13", 5, rng, genes, programs, with_types=False)[0]]
    calls = []
    real = api._gene_features
    monkeypatch.setattr(api, "_gene_features", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rp = sda.ResidentPredictor("mouse", "Demo", model_path=tmp_path / "bundle")
    assert len(calls) == 1
    got = rp.predict_many(files, save_path=tmp_path / "res_resident")
    assert len(calls) == 1 and rp.last_route == "fused"       # PCA ran once, at construction
    for f, out in zip(files, got):
        want = sda.DeepSortPredictor("mouse", "Demo").predict(f, save_path=tmp_path / "res_existing", model_path=tmp_path / "bundle")
        ref_logits, index, _, _ = api._predict_logits("mouse", "Demo", f, tmp_path / "bundle", "csv", 0, 0, 10086)
        test, _ = api._read_test_csr(f, "csv", rp._gene2id, 0)
        _, _, logits = rp.classify(test)
        np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.cpu().numpy(), atol=1e-4)
        assert list(out.columns) == list(want.columns) and list(out["index"]) == list(want["index"])
        ok = _off_boundary(ref_logits.cpu().numpy(), 2.0, 1e-4)
        assert ok.mean() > 0.9
        assert out["cell_type"][ok].tolist() == want["cell_type"][ok].tolist()
        name = f"mouse_Demo_{Path(f).stem}.csv"
        assert (tmp_path / "res_resident" / name).exists() and (tmp_path / "res_existing" / name).exists()


def _testis_bundle(tmp_path):
    """A bundle built from tests/golden/testis199.npz: its support rows, synthetic gene names, the fixture's parameters."""
    from scdeepsort_amd.api import BundlePaths
    z = np.load(GOLDEN / "testis199.npz")
    expr = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"]))
    mask = z["support_mask"].astype(bool)
    genes = [f"Gene{i}" for i in range(expr.shape[1])]
    labels = [f"type{i}" for i in range(int(z["n_classes"]))]
    b = BundlePaths(tmp_path / "testis", "mouse", "Testis", layout="flat", for_write=True)
    b.mkdirs()
    b.genes.write_bytes("".join(g + "\r\n" for g in genes).encode())
    b.cell_types.write_bytes("".join(l + "\r\n" for l in labels).encode())
    sp.save_npz(b.support, sp.csr_matrix(expr[mask]))
    state = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    torch.save({"model": state, "optimizer": {}}, b.model)
    test = expr[~mask].toarray()
    cells = [f"T{j}" for j in range(test.shape[0])]
    data = tmp_path / "mouse_Testis199_data.csv"
    pd.DataFrame(test.T, index=genes, columns=cells).to_csv(data)
    return tmp_path / "testis", data


def test_demo_data_bundle(tmp_path):
    root, data = _testis_bundle(tmp_path)
    rp = sda.ResidentPredictor("mouse", "Testis", model_path=root)
    test, _ = api._read_test_csr(data, "csv", rp._gene2id, 0)
    label, _, logits = rp.classify(test)
    assert rp.last_route == "fused"
    ref_logits, _, _, _ = api._predict_logits("mouse", "Testis", data, root, "csv", 0, 0, 10086)
    ref = ref_logits.cpu().numpy()
    np.testing.assert_allclose(logits.cpu().numpy(), ref, atol=1e-4)
    want, _ = api._classify(ref_logits, 2.0)
    ok = _off_boundary(ref, 2.0, 1e-4)
    assert ok.mean() > 0.8
    np.testing.assert_array_equal(label[ok], want[ok])


def _random_bundle(tmp_path, n_layers, G=500, n_sup=200, dense=16, hidden=12, n_cls=5, seed=0):
    """A bundle written by hand from a randomly initialised GNN (no fit)."""
    from scdeepsort_amd.api import BundlePaths
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    genes = [f"Gene{i}" for i in range(G)]
    b = BundlePaths(tmp_path / f"rand{n_layers}", "mouse", "Rand", layout="flat", for_write=True)
    b.mkdirs()
    b.genes.write_bytes("".join(g + "\r\n" for g in genes).encode())
    b.cell_types.write_bytes("".join(f"type{i}\r\n" for i in range(n_cls)).encode())
    sup = sp.random(n_sup, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    sup.data = 1.0 + 4.0 * sup.data
    sp.save_npz(b.support, sup)
    m = sda.GNN(dense, hidden, n_cls, n_layers, G, activation=F.relu)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    torch.save({"model": m.state_dict(), "optimizer": {}}, b.model)
    return tmp_path / f"rand{n_layers}", G


def test_routing_by_work(tmp_path, monkeypatch):
    root, G = _random_bundle(tmp_path, 2)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    batch = sp.random(300, G, density=0.1, random_state=7, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    lab_f, p_f, log_f = rp.classify(batch)
    assert rp.last_route == "fused"
    monkeypatch.setattr(api, "RESIDENT_FUSED_MAX_WORK", batch.nnz * rp.hidden_padded * 2 - 1)
    lab_g, p_g, log_g = rp.classify(batch)
    assert rp.last_route == "graph"
    np.testing.assert_allclose(log_f.cpu().numpy(), log_g.cpu().numpy(), atol=1e-4)
    ok = _off_boundary(log_g.cpu().numpy(), 2.0, 1e-4)
    np.testing.assert_array_equal(lab_f[ok], lab_g[ok])
    np.testing.assert_allclose(p_f, p_g, atol=1e-4)
    # a caller-supplied device CSR takes the same path, gene ids checked once
    dev_csr = (torch.from_numpy(batch.indptr.astype(np.int64)).to(DEV), torch.from_numpy(batch.indices).to(DEV),
               torch.from_numpy(batch.data).to(DEV))
    monkeypatch.setattr(api, "RESIDENT_FUSED_MAX_WORK", 4_000_000_000)
    lab_d, _, log_d = rp.classify(dev_csr)
    assert rp.last_route == "fused" and torch.equal(log_d, log_f)
    bad = (dev_csr[0], dev_csr[1].clone().index_fill_(0, torch.tensor([0], device=DEV), G), dev_csr[2])
    with pytest.raises(sda.WgnnError, match="out of range"):
        rp.classify(bad)


def test_one_layer_classify_is_one_launch(tmp_path):
    from torch.profiler import ProfilerActivity, profile
    root, G = _random_bundle(tmp_path, 1, seed=3)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    batch = sp.random(1000, G, density=0.1, random_state=9, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    rp.classify(batch)                                        # warm-up
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        label, _, _ = rp.classify(batch)
        torch.cuda.synchronize()
    assert rp.last_route == "fused" and label.shape == (1000,)
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    assert len(kernels) == 1 and "predict_rows" in kernels[0], kernels


def test_evaluate_on_demo_bundle(tmp_path):
    root, data = _testis_bundle(tmp_path)
    rp = sda.ResidentPredictor("mouse", "Testis", model_path=root)
    test, index = api._read_test_csr(data, "csv", rp._gene2id, 0)
    label, _, _ = rp.classify(test)
    truth = [f"type{(i * 3) % 8}" for i in range(len(index))]
    ct = tmp_path / "mouse_Testis199_celltype.csv"
    pd.DataFrame({"Cell": list(index), "Cell_type": truth}).to_csv(ct)
    from test_resident_predict_host import _write_xlsx
    rows = [["Tissue", "num", "Test Datasets", "Celltype", "Training dataset cell type"]]
    rows += [["Testis", 199, "mouse_Testis199_data.csv", f"type{i}", f"type{i}"] for i in range(8)]
    rows += [["Testis", 199, "mouse_Testis199_data.csv", "type0", "type1"]]
    _write_xlsx(root / "map.xlsx", rows)
    correct, total, unsure, acc, out = rp.evaluate(data, ct)
    mapping = api.load_map_dict(root / "map.xlsx", "Testis")[199]
    want = api.evaluate_predictions(label, truth, rp.id2label, mapping)
    assert (correct, total, unsure, acc) == want[:4] and total == len(index)
    assert list(out.columns) == ["index", "original label", "cell_type"] and out["original label"].tolist() == truth
