"""``wgnn_predict_rows_thin`` and ``ResidentPredictor.stability(thin="reads")`` on the GPU: the thinning (``draw_reads`` /
``draw_entries``) exactly and the draws within ``TOL`` of the fp64 restatement of tests/thin_reference.py; a materialised draw
through ``align_rows(normalize="lognorm")`` and ``predict_rows``; ``keep = 1`` carrying the bits of ``predict_rows`` on the
lognorm-aligned batch; ``keep = 0``; the tallies against the kernel's own per-draw outputs; determinism, splitting by cells and
by draws, guard rows, and the predictor end to end."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import stability_reference as R
import thin_reference as T
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5                                                        # test_gpu_resident_predict.py's, for this same gather


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_csr(m, i64):
    return t(m.indptr.astype(np.int64 if i64 else np.int32)), t(m.indices.astype(np.int32)), t(m.data.astype(np.float32))


def _run_case(c, i64, keep, D, seed=T.CASE_SEED, **kw):
    rp, col, raw = _device_csr(c["m"], i64)
    args = (rp, col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    common = dict(rest=t(c["rest"]), scale=c["scale"], threshold=c["vthr"], self_rows=t(c["self_rows"]), n_draws=D, keep=keep,
                  seed=seed, **kw)
    out = ops.predict_rows_thin(*args, want_reads=True, **common)
    tabs = ops.predict_rows_thin(*args, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], want_draws=True, want_reads=True,
                                 **common)
    return out, tabs


# ------------------------------------------------------------------------------------------------
# 1. thinned draws against the fp64 reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.THIN_CASES, ids=str)
def test_thinned_draws_match_the_fp64_reference(case):
    H, Cn, explicit, i64, keep, D = case
    c = T.thin_case(H, Cn, explicit, keep, D)
    B = c["m"].shape[0]
    (out, reads0, entries0), (votes, unsure, empty, conf, dl, dp, reads, entries) = _run_case(c, i64, keep, D)
    np.testing.assert_array_equal(reads.cpu().numpy(), c["reads"])                 # the thinning, exactly
    np.testing.assert_array_equal(entries.cpu().numpy(), c["entries"])
    assert torch.equal(reads0, reads) and torch.equal(entries0, entries)
    err_h = float(np.abs(out.cpu().numpy() - c["out"]).max())
    err_p = float(np.abs(dp.cpu().numpy() - c["prob"]).max())
    share = float(c["unclear"].mean())
    print(f"case {case}: max |out - want| = {err_h:.3e} (scale {max(1.0, np.abs(c['out']).max()):.3f}), max |max_prob - want| = "
          f"{err_p:.3e}, unclear pairs {share:.4f}")
    assert err_h <= TOL * max(1.0, float(np.abs(c["out"]).max()))
    assert err_p <= TOL * max(1.0, float(np.abs(c["prob"]).max()))
    assert share <= 0.05
    clear = ~c["unclear"]
    np.testing.assert_array_equal(dl.cpu().numpy()[clear], c["label"][clear])
    np.testing.assert_array_equal(empty.cpu().numpy(), c["empty"].sum(axis=1))
    # the tallies against the kernel's own per-draw outputs, exactly
    g_votes, g_unsure, _, _ = R.tallies(dl.cpu().numpy(), dp.cpu().numpy(), c["empty"], Cn)
    np.testing.assert_array_equal(votes.cpu().numpy(), g_votes)
    np.testing.assert_array_equal(unsure.cpu().numpy(), g_unsure)
    assert ((votes.sum(dim=1) + unsure) == D).all()
    want_conf = torch.zeros(B, dtype=torch.float64, device=DEV)
    for d in range(D):
        want_conf = want_conf + dp[:, d].double()
    assert torch.equal(conf, want_conf)


# ------------------------------------------------------------------------------------------------
# 2. a materialised draw through the existing kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.MATERIALISED_CASES, ids=str)
def test_draw_matches_align_rows_and_predict_rows_on_the_thinned_counts(case):
    H, Cn, explicit, keep, d = case
    D = d + 1
    c = T.thin_case(H, Cn, explicit, keep, D)
    (out, _, _), (_, _, _, _, dl, dp, _, _) = _run_case(c, False, keep, D)
    G = c["m"].shape[1]
    cp, rp_ = T.thin_draw(c["m"], c["rest"], T.CASE_SEED, d, keep)
    gene_map = t(np.concatenate([np.arange(G), [-1]]).astype(np.int32))           # one more column, outside the bundle: rest'
    rp, col, raw = ops.align_rows(t(T.materialised(c["m"], cp, rp_)), gene_map, G, 0.0, normalize="lognorm", scale=c["scale"])
    sr = None if c["self_rows"] is None else t(c["self_rows"][d::D])
    args = (rp, col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    want_h = ops.predict_rows(*args, self_rows=sr)
    _, want_label, want_p = ops.predict_rows(*args, self_rows=sr, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"])
    scale = max(1.0, float(want_h.abs().max()))
    assert float((out[d::D] - want_h).abs().max()) <= TOL * scale
    assert float((dp[:, d] - want_p).abs().max()) <= TOL
    clear = t(~c["unclear"][:, d])
    assert torch.equal(dl[:, d][clear], want_label[clear])


# ------------------------------------------------------------------------------------------------
# 3. keep = 1 carries predict_rows' bits on the lognorm-aligned batch; keep = 0 is the empty row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vthr", [0.0, 1.5])
@pytest.mark.parametrize("H,i64", [(12, False), (64, True), (200, False), (256, True)])
def test_keep_one_carries_the_bits_of_predict_rows_on_the_lognorm_batch(H, i64, vthr):
    m, rest = T.count_batch()
    _, table, alpha, bias = (t(a) if not sp.issparse(a) else a for a in R.operands(H))
    B, G = m.shape
    counts = _device_csr(m, i64)
    x = T.materialised(m, m.data.astype(np.int64), rest)
    gene_map = t(np.concatenate([np.arange(G), [-1]]).astype(np.int32))
    rp, col, raw = ops.align_rows(t(x), gene_map, G, vthr, normalize="lognorm", scale=T.SCALE)
    assert (int(col.shape[0]) < m.nnz) == (vthr > 0)              # a positive threshold drops entries
    for explicit in (False, True):
        sr = t(R.self_operand(H, B)) if explicit else None
        want_h = ops.predict_rows(rp, col, raw, table, alpha, bias, self_rows=sr)
        for D in (1, 9):
            srd = None if sr is None else sr.repeat_interleave(D, dim=0)
            kw = dict(rest=t(rest), scale=T.SCALE, threshold=vthr, self_rows=srd, n_draws=D, keep=1.0, seed=H + D)
            got_h, reads, entries = ops.predict_rows_thin(*counts, table, alpha, bias, want_reads=True, **kw)
            assert torch.equal(got_h.view(B, D, H), want_h[:, None, :].expand(B, D, H)), (explicit, D)
            assert torch.equal(entries, (rp[1:] - rp[:-1]).int()[:, None].expand(B, D))
            assert torch.equal(reads, t(x.sum(axis=1).astype(np.int32))[:, None].expand(B, D))
            for Cn in (2, 16, 40):
                w, b = (t(a) for a in R.head_operands(H, Cn))
                thr = T.full_threshold(H, Cn, explicit, vthr)
                _, label, prob = ops.predict_rows(rp, col, raw, table, alpha, bias, self_rows=sr, head=(w, b), unsure_threshold=thr)
                votes, unsure, empty, conf, dl, dp = ops.predict_rows_thin(*counts, table, alpha, bias, head=(w, b),
                                                                         unsure_threshold=thr, want_draws=True, **kw)
                assert torch.equal(dl, label[:, None].expand(B, D)) and torch.equal(dp, prob[:, None].expand(B, D)), (explicit, D, Cn)
                assert torch.equal(conf, D * prob.double()) and torch.equal(empty, ((rp[1:] - rp[:-1]) == 0).int() * D)
                assert ((votes.sum(dim=1) + unsure) == D).all()


@pytest.mark.parametrize("H", [12, 200])
def test_keep_zero_is_the_empty_row(H):
    m, rest = T.count_batch()
    _, table, alpha, bias = (t(a) if not sp.issparse(a) else a for a in R.operands(H))
    B, D, Cn = m.shape[0], 5, 16
    kw = dict(rest=t(rest), n_draws=D, keep=0.0, seed=1)
    out, reads, entries = ops.predict_rows_thin(*_device_csr(m, False), table, alpha, bias, want_reads=True, **kw)
    assert torch.equal(out, torch.relu(bias)[None, :].expand(B * D, H)) and not reads.any() and not entries.any()
    w, b = (t(a) for a in R.head_operands(H, Cn))
    votes, unsure, empty, conf, dl, dp = ops.predict_rows_thin(*_device_csr(m, False), table, alpha, bias, head=(w, b),
                                                             want_draws=True, **kw)
    assert (empty == D).all() and (dl == dl[0, 0]).all() and (dp == dp[0, 0]).all() and (unsure == 0).all()
    assert int(votes[:, int(dl[0, 0])].min()) == D and torch.equal(conf, D * dp[:, 0].double())


# ------------------------------------------------------------------------------------------------
# 4. determinism, splitting, guard rows
# ------------------------------------------------------------------------------------------------
def test_determinism_and_splitting_by_cells_and_draws():
    H, Cn, explicit, keep, D = 64, 16, True, 0.5, 12
    c = T.thin_case(H, Cn, explicit, keep, D)
    m = c["m"]
    B = m.shape[0]
    (out, _, _), tabs = _run_case(c, False, keep, D)
    (out2, _, _), tabs2 = _run_case(c, False, keep, D)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    rp, col, raw = _device_csr(m, False)
    args = (col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    rest = t(c["rest"])
    kw = dict(head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], keep=keep, seed=T.CASE_SEED, want_draws=True, want_reads=True)
    sr = t(c["self_rows"])
    cut = 17                                                       # cells split in two with row0
    parts = [ops.predict_rows_thin(rp[:cut + 1], *args, rest=rest[:cut], self_rows=sr[:cut * D], n_draws=D, **kw),
             ops.predict_rows_thin(rp[cut:], *args, rest=rest[cut:], self_rows=sr[cut * D:], n_draws=D, row0=cut, **kw)]
    for whole, a, b in zip(tabs, *parts):
        assert torch.equal(whole, torch.cat([a, b]))
    lo = ops.predict_rows_thin(rp[cut:], *args, rest=rest[cut:], self_rows=sr[cut * D:], n_draws=D, keep=keep, seed=T.CASE_SEED, row0=cut)
    assert torch.equal(lo, out[cut * D:])
    D1 = 5                                                         # draws split with draw0 + accumulate
    srv = sr.view(B, D, H)
    first = ops.predict_rows_thin(rp, *args, rest=rest, self_rows=srv[:, :D1].reshape(-1, H), n_draws=D1, **kw)
    second = ops.predict_rows_thin(rp, *args, rest=rest, self_rows=srv[:, D1:].reshape(-1, H), n_draws=D - D1, draw0=D1,
                                   out=first[:4], accumulate=True, **kw)
    for whole, acc in zip(tabs[:4], second[:4]):
        assert torch.equal(whole, acc)                             # conf_sum bit for bit: the running sum continues
    for i in (4, 5, 6, 7):
        assert torch.equal(torch.cat([first[i], second[i]], dim=1), tabs[i])
    # permuting each row's entries: the thinning follows the gene
    rng = np.random.default_rng(5)
    perm = np.concatenate([m.indptr[r] + rng.permutation(m.indptr[r + 1] - m.indptr[r]) for r in range(B)])
    shuffled = sp.csr_matrix((m.data[perm], m.indices[perm], m.indptr), shape=m.shape)
    _, tabs3 = _run_case(dict(c, m=shuffled), False, keep, D)
    assert torch.equal(tabs3[2], tabs[2]) and torch.equal(tabs3[6], tabs[6]) and torch.equal(tabs3[7], tabs[7])
    clear = t(~c["unclear"])
    assert torch.equal(tabs3[4][clear], tabs[4][clear])
    assert float((tabs3[5] - tabs[5]).abs().max()) <= 2 * TOL


def test_outputs_stay_inside_their_views():
    H, Cn, keep, D = 12, 16, 0.5, 7
    c = T.thin_case(H, Cn, False, keep, D)
    B = c["m"].shape[0]
    args = (*_device_csr(c["m"], True), t(c["table"]), t(c["alpha"]), t(c["bias"]))
    kw = dict(rest=t(c["rest"]), n_draws=D, keep=keep, seed=T.CASE_SEED)
    G0, G1 = 3, 2                                                  # guard rows before / after
    ints = lambda *shape: torch.full(shape, -12345, dtype=torch.int32, device=DEV)
    votes_buf, unsure_buf, empty_buf = ints(G0 + B + G1, Cn + 3), ints(G0 + B + G1), ints(G0 + B + G1)
    conf_buf = torch.full((G0 + B + G1,), float("nan"), dtype=torch.float64, device=DEV)
    dl_buf = ints(G0 + B + G1, D)
    dp_buf = torch.full((G0 + B + G1, D), float("nan"), dtype=torch.float32, device=DEV)
    out_buf = torch.full((G0 * D + B * D + G1 * D, H), float("nan"), dtype=torch.float32, device=DEV)
    rows = slice(G0, G0 + B)
    views = (votes_buf[rows, :Cn], unsure_buf[rows], empty_buf[rows], conf_buf[rows], dl_buf[rows], dp_buf[rows])
    head = dict(head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"])
    got = ops.predict_rows_thin(*args, out=views, **head, **kw)
    free = ops.predict_rows_thin(*args, want_draws=True, **head, **kw)
    for g, f in zip(got, free):                                   # every element written, the same values as into fresh tensors
        assert torch.equal(g, f)
    for buf in (votes_buf, unsure_buf, empty_buf, dl_buf):
        assert (buf[:G0] == -12345).all() and (buf[G0 + B:] == -12345).all()
    assert (votes_buf[:, Cn:] == -12345).all()
    for buf in (conf_buf, dp_buf):
        assert torch.isnan(buf[:G0]).all() and torch.isnan(buf[G0 + B:]).all() and not torch.isnan(buf[rows]).any()
    o = ops.predict_rows_thin(*args, out=out_buf[G0 * D:(G0 + B) * D], **kw)
    assert not torch.isnan(o).any() and torch.isnan(out_buf[:G0 * D]).all() and torch.isnan(out_buf[(G0 + B) * D:]).all()
    assert torch.equal(o, ops.predict_rows_thin(*args, **kw))


def test_ops_argument_errors():
    rp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    col, raw = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    table, alpha, bias = torch.zeros(3, 8, device=DEV), torch.ones(5, device=DEV), torch.zeros(8, device=DEV)
    rest = torch.zeros(1, dtype=torch.int64, device=DEV)
    for kw in (dict(n_draws=0, keep=0.5), dict(n_draws=2, keep=1.5), dict(n_draws=2, keep=float("nan")), dict(n_draws=2, keep=0.5, row0=-1),
               dict(n_draws=2, keep=0.5, accumulate=True), dict(n_draws=2, keep=0.5, scale=0.0), dict(n_draws=2, keep=0.5, threshold=-1.0),
               dict(n_draws=2, keep=0.5, rest=rest.int()), dict(n_draws=2, keep=0.5, rest=torch.zeros(2, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            ops.predict_rows_thin(rp, col, raw, table, alpha, bias, seed=0, **{"rest": rest, **kw})
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.predict_rows_thin(rp, torch.full_like(col, 3), raw, table, alpha, bias, rest=rest, n_draws=2, keep=0.5, seed=0)


# ------------------------------------------------------------------------------------------------
# 5. end to end
# ------------------------------------------------------------------------------------------------
def _same(a: api.Stability, b: api.Stability):
    assert a.n_draws == b.n_draws and a.keep == b.keep and a.thin == b.thin
    np.testing.assert_array_equal(a.label, b.label); np.testing.assert_array_equal(a.max_prob, b.max_prob)
    for x, y in ((a.votes, b.votes), (a.unsure, b.unsure), (a.empty, b.empty), (a.conf_sum, b.conf_sum)):
        assert torch.equal(x, y)


def _counts(rp, G, n=60, seed=3):
    rng = np.random.default_rng(seed)
    genes = [rp.id2gene[i] for i in rng.permutation(G)[:300]] + ["NotAGene1", "NotAGene2"]
    counts = rng.geometric(0.5, (n, len(genes))) * (rng.random((n, len(genes))) < 0.2)
    return counts.astype(np.float32), genes


@pytest.mark.parametrize("n_layers", [1, 2])
def test_stability_by_reads_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=n_layers + 12)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _counts(rp, G)
    B = counts.shape[0]
    label, prob, _ = rp.classify(counts, genes=genes, normalize="lognorm")
    st = rp.stability(counts, genes=genes, normalize="lognorm", n_draws=16, seed=11, thin="reads")
    np.testing.assert_array_equal(st.label, label); np.testing.assert_array_equal(st.max_prob, prob)      # the call as given
    assert st.thin == "reads" and st.n_draws == 16 and st.votes.shape == (3, B, rp.n_classes)
    assert ((st.votes.sum(dim=2) + st.unsure) == 16).all()
    np.testing.assert_array_equal(st.n_reads, counts.sum(axis=1).astype(np.int64))
    np.testing.assert_array_equal(st.n_entries, (counts[:, :300] > 0).sum(axis=1))
    assert "n_reads" in st.frame().columns and "thinned by reads" in str(st.summary())
    one = rp.stability(counts, genes=genes, normalize="lognorm", keep=(1.0,), n_draws=5, thin="reads")
    assert (one.agreement() == 1).all() and (one.flips_to()[0] == -1).all()
    np.testing.assert_array_equal(one.mean_prob()[0], prob.astype(np.float64))
    # from a CSR over the caller's columns, and chunked by a tiny byte budget: the same bits
    _same(rp.stability(sp.csr_matrix(counts), genes=genes, normalize="lognorm", n_draws=16, seed=11, thin="reads"), st)
    monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", 16 * rp.hidden_padded * 4 * 3 * 7)
    _same(rp.stability(counts, genes=genes, normalize="lognorm", n_draws=16, seed=11, thin="reads"), st)
    monkeypatch.undo()
    # into: 8 draws and 8 more are 16 at once
    half = rp.stability(counts, genes=genes, normalize="lognorm", n_draws=8, seed=11, thin="reads")
    assert rp.stability(counts, genes=genes, normalize="lognorm", n_draws=8, seed=11, thin="reads", into=half) is half
    _same(half, st)
    with pytest.raises(ValueError, match="thin"):
        rp.stability(counts, genes=genes, normalize="lognorm", n_draws=8, seed=11, into=half)
    # a library size of the caller's: the reads outside the batch's columns
    lib = counts.sum(axis=1) + 500
    deep = rp.stability(counts, genes=genes, normalize=sda.LogNormalize(library_size=lib), n_draws=4, thin="reads")
    np.testing.assert_array_equal(deep.n_reads, np.where(counts.sum(axis=1) > 0, lib, 0).astype(np.int64))
    # operands the thinning cannot take
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, 0] = 2.5
        rp.stability(bad, genes=genes, normalize="lognorm", thin="reads")
    with pytest.raises(sda.WgnnError, match="cell 0"):
        rp.stability(counts, genes=genes, normalize=sda.LogNormalize(library_size=counts.sum(axis=1) - 1), thin="reads")
    # thin="genes" is the call without the argument, bit for bit
    _same(rp.stability(counts, genes=genes, normalize="lognorm", n_draws=8, seed=2, thin="genes"),
          rp.stability(counts, genes=genes, normalize="lognorm", n_draws=8, seed=2))


def test_stability_file_by_reads_writes_the_table(tmp_path):
    import pandas as pd
    root, G = _random_bundle(tmp_path, 2, seed=4)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    counts, genes = _counts(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(counts.shape[0])]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    out = rp.stability_file(data, keep=(0.5, 0.25), n_draws=8, seed=3, save_path=tmp_path / "res", normalize="lognorm", thin="reads")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_stability.csv")
    cols = ["index", "cell_type", "prob", "n_genes", "n_reads", "agree_0.5", "flip_0.5", "flip_share_0.5", "agree_0.25", "flip_0.25",
            "flip_share_0.25"]
    assert list(out.columns) == cols and list(written.columns) == cols and written["index"].tolist() == cells
    st = rp.stability(counts, genes=genes, normalize="lognorm", keep=(0.5, 0.25), n_draws=8, seed=3, thin="reads")
    np.testing.assert_array_equal(out["agree_0.25"], st.agreement()[1])
    np.testing.assert_array_equal(out["n_reads"], counts.sum(axis=1).astype(np.int64))
