"""``wgnn_predict_rows_dropout`` and ``ResidentPredictor.stability`` on the GPU: with ``keep = 1`` the bits of
``wgnn_predict_rows``; masked draws against the fp64 restatement of tests/stability_reference.py and against the existing
kernel on a materialised draw; the tallies against the kernel's own per-draw outputs; determinism, splitting by cells and by
draws, guard rows, the C ABI's errors and the predictor end to end."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import stability_reference as R
from test_gpu_resident_predict import _random_bundle
from test_stability_reference import test_c_abi_errors_return_before_any_launch as _abi_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5                                                        # test_gpu_resident_predict.py's, for this same gather


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_csr(m, i64):
    return t(m.indptr.astype(np.int64 if i64 else np.int32)), t(m.indices.astype(np.int32)), t(m.data.astype(np.float32))


def _operands(H, i64):
    m, table, alpha, bias = R.operands(H)
    return m, _device_csr(m, i64), t(table), t(alpha), t(bias)


# ------------------------------------------------------------------------------------------------
# 1. keep = 1 carries predict_rows' bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("H", [12, 32, 64, 128, 200, 256])
def test_keep_one_carries_the_bits_of_predict_rows(H, i64):
    m, (rp, col, raw), table, alpha, bias = _operands(H, i64)
    B = m.shape[0]
    for explicit in (False, True):
        sr = t(R.self_operand(H, B)) if explicit else None
        want_h = ops.predict_rows(rp, col, raw, table, alpha, bias, self_rows=sr)
        for D in (1, 8, 9):
            srd = None if sr is None else sr.repeat_interleave(D, dim=0)
            got_h = ops.predict_rows_dropout(rp, col, raw, table, alpha, bias, self_rows=srd, n_draws=D, keep=1.0, seed=H + D)
            assert got_h.shape == (B * D, H)
            assert torch.equal(got_h.view(B, D, H), want_h[:, None, :].expand(B, D, H)), (explicit, D)
            for Cn in (2, 16, 40) + ((64,) if H == 256 and D == 9 else ()):       # [64, 256]: a head of exactly 64 KiB
                w, b = (t(a) for a in R.head_operands(H, Cn))
                thr = R.full_threshold(H, Cn, explicit)
                _, label, prob = ops.predict_rows(rp, col, raw, table, alpha, bias, self_rows=sr, head=(w, b),
                                                  unsure_threshold=thr)
                votes, unsure, empty, conf, dl, dp = ops.predict_rows_dropout(
                    rp, col, raw, table, alpha, bias, self_rows=srd, head=(w, b), unsure_threshold=thr, n_draws=D, keep=1.0,
                    seed=3 * H + Cn, want_draws=True)
                assert torch.equal(dl, label[:, None].expand(B, D)) and torch.equal(dp, prob[:, None].expand(B, D)), (explicit, D, Cn)
                lab = label.long()
                want_votes = torch.zeros((B, Cn), dtype=torch.int32, device=DEV)
                want_votes[lab >= 0, lab[lab >= 0]] = D
                assert torch.equal(votes, want_votes) and torch.equal(unsure, ((lab < 0) * D).int())
                assert torch.equal(conf, D * prob.double())
                assert torch.equal(empty, t((np.diff(m.indptr) == 0).astype(np.int32) * D))
                assert (lab < 0).any() and (lab >= 0).any()


# ------------------------------------------------------------------------------------------------
# 2. masked draws against the fp64 reference
# ------------------------------------------------------------------------------------------------
def _run_case(c, i64, keep, D, seed=R.CASE_SEED, **kw):
    rp, col, raw = _device_csr(c["m"], i64)
    args = (rp, col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    common = dict(self_rows=t(c["self_rows"]), n_draws=D, keep=keep, seed=seed, **kw)
    out = ops.predict_rows_dropout(*args, **common)
    tabs = ops.predict_rows_dropout(*args, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], want_draws=True, **common)
    return out, tabs


@pytest.mark.parametrize("case", R.MASKED_CASES, ids=str)
def test_masked_draws_match_the_fp64_reference(case):
    H, Cn, explicit, i64, keep, D = case
    c = R.masked_case(H, Cn, explicit, keep, D)
    B = c["m"].shape[0]
    out, (votes, unsure, empty, conf, dl, dp) = _run_case(c, i64, keep, D)
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
    np.testing.assert_array_equal(empty.cpu().numpy(), c["empty"].sum(axis=1))                 # the mask alone
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
# 3. against the existing kernel on a materialised draw
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.MATERIALISED_CASES, ids=str)
def test_draw_matches_predict_rows_on_the_thinned_batch(case):
    H, Cn, explicit, keep, d = case
    D = d + 1
    c = R.masked_case(H, Cn, explicit, keep, D)
    out, (_, _, _, _, dl, dp) = _run_case(c, False, keep, D)
    thin = R.thinned(c["m"], R.entry_mask(c["m"], R.CASE_SEED, d, keep))
    rp, col, raw = _device_csr(thin, False)
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
# 4. keep = 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [12, 200])
def test_keep_zero_is_the_empty_row(H):
    m, (rp, col, raw), table, alpha, bias = _operands(H, False)
    B, D, Cn = m.shape[0], 5, 16
    out = ops.predict_rows_dropout(rp, col, raw, table, alpha, bias, n_draws=D, keep=0.0, seed=1)
    assert torch.equal(out, torch.relu(bias)[None, :].expand(B * D, H))
    assert not torch.isnan(out).any()
    w, b = (t(a) for a in R.head_operands(H, Cn))
    votes, unsure, empty, conf, dl, dp = ops.predict_rows_dropout(rp, col, raw, table, alpha, bias, head=(w, b), n_draws=D, keep=0.0,
                                                                 seed=1, want_draws=True)
    assert (empty == D).all() and (dl == dl[0, 0]).all() and (dp == dp[0, 0]).all() and (unsure == 0).all()
    assert int(votes[:, int(dl[0, 0])].min()) == D and torch.equal(conf, D * dp[:, 0].double())


# ------------------------------------------------------------------------------------------------
# 5. determinism and splitting
# ------------------------------------------------------------------------------------------------
def test_determinism_and_splitting_by_cells_and_draws():
    H, Cn, explicit, keep, D = 64, 16, True, 0.5, 12
    c = R.masked_case(H, Cn, explicit, keep, D)
    m = c["m"]
    B = m.shape[0]
    out, tabs = _run_case(c, False, keep, D)
    out2, tabs2 = _run_case(c, False, keep, D)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    rp, col, raw = _device_csr(m, False)
    args = (col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    head = dict(head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"])
    sr = t(c["self_rows"])
    # cells split in two with row0
    cut = 17
    parts = [ops.predict_rows_dropout(rp[:cut + 1], *args, self_rows=sr[:cut * D], n_draws=D, keep=keep, seed=R.CASE_SEED,
                                      want_draws=True, **head),
             ops.predict_rows_dropout(rp[cut:], *args, self_rows=sr[cut * D:], n_draws=D, keep=keep, seed=R.CASE_SEED, row0=cut,
                                      want_draws=True, **head)]
    for whole, a, b in zip(tabs, *parts):
        assert torch.equal(whole, torch.cat([a, b]))
    lo = ops.predict_rows_dropout(rp[cut:], *args, self_rows=sr[cut * D:], n_draws=D, keep=keep, seed=R.CASE_SEED, row0=cut)
    assert torch.equal(lo, out[cut * D:])
    # draws split with draw0 + accumulate
    D1 = 5
    srv = sr.view(B, D, H)
    first = ops.predict_rows_dropout(rp, *args, self_rows=srv[:, :D1].reshape(-1, H), n_draws=D1, keep=keep, seed=R.CASE_SEED,
                                     want_draws=True, **head)
    second = ops.predict_rows_dropout(rp, *args, self_rows=srv[:, D1:].reshape(-1, H), n_draws=D - D1, keep=keep, seed=R.CASE_SEED,
                                      draw0=D1, out=first[:4], accumulate=True, want_draws=True, **head)
    for whole, acc in zip(tabs[:4], second[:4]):
        assert torch.equal(whole, acc)                             # conf_sum bit for bit: the running sum continues
    assert torch.equal(torch.cat([first[4], second[4]], dim=1), tabs[4]) and torch.equal(torch.cat([first[5], second[5]], dim=1), tabs[5])
    # permuting each row's entries: the mask follows the gene
    rng = np.random.default_rng(5)
    perm = np.concatenate([m.indptr[r] + rng.permutation(m.indptr[r + 1] - m.indptr[r]) for r in range(B)])
    shuffled = sp.csr_matrix((m.data[perm], m.indices[perm], m.indptr), shape=m.shape)
    c2 = dict(c, m=shuffled)
    _, tabs3 = _run_case(c2, False, keep, D)
    assert torch.equal(tabs3[2], tabs[2])
    clear = t(~c["unclear"])
    assert torch.equal(tabs3[4][clear], tabs[4][clear])
    assert float((tabs3[5] - tabs[5]).abs().max()) <= 2 * TOL


# ------------------------------------------------------------------------------------------------
# 6. guard rows and columns
# ------------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_views():
    H, Cn, keep, D = 32, 16, 0.5, 7
    c = R.masked_case(H, Cn, False, keep, D)
    B = c["m"].shape[0]
    rp, col, raw = _device_csr(c["m"], True)
    args = (rp, col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    G0, G1 = 3, 2                                                  # guard rows before / after
    ints = lambda *shape: torch.full(shape, -12345, dtype=torch.int32, device=DEV)
    votes_buf, unsure_buf, empty_buf = ints(G0 + B + G1, Cn + 3), ints(G0 + B + G1), ints(G0 + B + G1)
    conf_buf = torch.full((G0 + B + G1,), float("nan"), dtype=torch.float64, device=DEV)
    dl_buf = ints(G0 + B + G1, D)
    dp_buf = torch.full((G0 + B + G1, D), float("nan"), dtype=torch.float32, device=DEV)
    out_buf = torch.full((G0 * D + B * D + G1 * D, H), float("nan"), dtype=torch.float32, device=DEV)
    rows = slice(G0, G0 + B)
    views = (votes_buf[rows, :Cn], unsure_buf[rows], empty_buf[rows], conf_buf[rows], dl_buf[rows], dp_buf[rows])
    assert views[0].stride(0) == Cn + 3
    got = ops.predict_rows_dropout(*args, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], n_draws=D, keep=keep,
                                   seed=R.CASE_SEED, out=views)
    free = ops.predict_rows_dropout(*args, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], n_draws=D, keep=keep,
                                    seed=R.CASE_SEED, want_draws=True)
    for g, f in zip(got, free):                                   # every element written, the same values as into fresh tensors
        assert torch.equal(g, f)
    assert not torch.isnan(conf_buf[rows]).any() and not torch.isnan(dp_buf[rows]).any()
    assert (votes_buf[rows, :Cn] >= 0).all() and (unsure_buf[rows] >= 0).all() and (empty_buf[rows] >= 0).all() and (dl_buf[rows] >= -1).all()
    for buf in (votes_buf, unsure_buf, empty_buf, dl_buf):
        assert (buf[:G0] == -12345).all() and (buf[G0 + B:] == -12345).all()
    assert (votes_buf[:, Cn:] == -12345).all()
    for buf in (conf_buf, dp_buf):
        assert torch.isnan(buf[:G0]).all() and torch.isnan(buf[G0 + B:]).all()
    o = ops.predict_rows_dropout(*args, n_draws=D, keep=keep, seed=R.CASE_SEED, out=out_buf[G0 * D:(G0 + B) * D])
    assert not torch.isnan(o).any() and torch.isnan(out_buf[:G0 * D]).all() and torch.isnan(out_buf[(G0 + B) * D:]).all()
    assert torch.equal(o, ops.predict_rows_dropout(*args, n_draws=D, keep=keep, seed=R.CASE_SEED))


# ------------------------------------------------------------------------------------------------
# 7. the C ABI's errors
# ------------------------------------------------------------------------------------------------
def test_c_abi_errors():
    _abi_errors()                                                  # host pointers: every case returns before a launch
    rp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    col, raw = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    table, alpha, bias = torch.zeros(3, 8, device=DEV), torch.ones(5, device=DEV), torch.zeros(8, device=DEV)
    for kw in (dict(n_draws=0, keep=0.5), dict(n_draws=2, keep=1.5), dict(n_draws=2, keep=float("nan")), dict(n_draws=2, keep=0.5, row0=-1),
               dict(n_draws=2, keep=0.5, accumulate=True)):
        with pytest.raises(sda.WgnnError):
            ops.predict_rows_dropout(rp, col, raw, table, alpha, bias, seed=0, **kw)
    bad = torch.full_like(col, 3)
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.predict_rows_dropout(rp, bad, raw, table, alpha, bias, n_draws=2, keep=0.5, seed=0)


# ------------------------------------------------------------------------------------------------
# 8. end to end
# ------------------------------------------------------------------------------------------------
def _batch(G, n=150, seed=7):
    batch = sp.random(n, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    return batch


def _same(a: api.Stability, b: api.Stability):
    assert a.n_draws == b.n_draws and a.keep == b.keep
    np.testing.assert_array_equal(a.label, b.label); np.testing.assert_array_equal(a.max_prob, b.max_prob)
    for x, y in ((a.votes, b.votes), (a.unsure, b.unsure), (a.empty, b.empty), (a.conf_sum, b.conf_sum)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n_layers,hidden", [(1, 12), (2, 12), (1, 20), (2, 20)])
def test_stability_end_to_end(tmp_path, monkeypatch, n_layers, hidden):
    root, G = _random_bundle(tmp_path, n_layers, hidden=hidden, seed=n_layers + hidden)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    batch = _batch(G)
    B = batch.shape[0]
    label, prob, _ = rp.classify(batch)
    st = rp.stability(batch, n_draws=32, seed=11)
    np.testing.assert_array_equal(st.label, label); np.testing.assert_array_equal(st.max_prob, prob)
    assert st.keep == (0.75, 0.5, 0.25) and st.n_draws == 32 and st.votes.shape == (3, B, rp.n_classes)
    assert ((st.votes.sum(dim=2) + st.unsure) == 32).all()
    np.testing.assert_array_equal(st.n_entries, np.diff(batch.indptr))
    agree = st.agreement()
    assert agree.shape == (3, B) and (agree >= 0).all() and (agree <= 1).all()
    one = rp.stability(batch, keep=(1.0,), n_draws=5)
    assert (one.agreement() == 1).all() and (one.flips_to()[0] == -1).all()
    np.testing.assert_array_equal(one.mean_prob()[0], prob.astype(np.float64))
    # chunked by a tiny byte budget: the same bits
    monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", 32 * rp.hidden_padded * 4 * 3 * 7)
    _same(rp.stability(batch, n_draws=32, seed=11), st)
    monkeypatch.undo()
    # into: twice 16 draws are 32 draws
    half = rp.stability(batch, n_draws=16, seed=11)
    assert rp.stability(batch, n_draws=16, seed=11, into=half) is half
    _same(half, st)
    with pytest.raises(ValueError, match="seed"):
        rp.stability(batch, n_draws=16, seed=12, into=half)
    # over the caller's own gene list, raw counts in
    rng = np.random.default_rng(3)
    genes = [rp.id2gene[i] for i in rng.permutation(G)[:300]] + ["NotAGene1", "NotAGene2"]
    counts = rng.poisson(0.3, (40, len(genes))).astype(np.float32)
    got = rp.stability(torch.from_numpy(counts).to(DEV), genes=genes, normalize="lognorm", n_draws=8, seed=2)
    want = rp.stability(rp.align(torch.from_numpy(counts).to(DEV), genes, normalize="lognorm"), n_draws=8, seed=2)
    _same(got, want)
    # the frame and the summary
    f = st.frame()
    assert list(f.columns)[:4] == ["index", "cell_type", "prob", "n_genes"] and len(f) == B
    assert {"agree_0.75", "flip_0.5", "flip_share_0.25"} <= set(f.columns)
    assert "keep 0.25" in str(st.summary())
    monkeypatch.setattr(rp, "hidden_padded", 260)
    with pytest.raises(ValueError, match="fused"):
        rp.stability(batch)


def test_stability_file_writes_the_table(tmp_path):
    import pandas as pd
    root, G = _random_bundle(tmp_path, 2, seed=4)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    batch = _batch(G, n=30, seed=1)
    cells = [f"C{j}" for j in range(batch.shape[0])]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(batch.toarray().T, index=rp.id2gene, columns=cells).to_csv(data)
    out = rp.stability_file(data, keep=(0.5, 0.25), n_draws=8, seed=3, save_path=tmp_path / "res")
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_stability.csv")
    cols = ["index", "cell_type", "prob", "n_genes", "agree_0.5", "flip_0.5", "flip_share_0.5", "agree_0.25", "flip_0.25",
            "flip_share_0.25"]
    assert list(out.columns) == cols and list(written.columns) == cols and written["index"].tolist() == cells
    test, _ = api._read_test_csr(data, "csv", rp._gene2id, 0)
    st = rp.stability(test, keep=(0.5, 0.25), n_draws=8, seed=3)
    np.testing.assert_array_equal(out["agree_0.25"], st.agreement()[1])
