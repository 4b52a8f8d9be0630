"""``ResidentPredictor.explain`` and its kernels ``wgnn_attrib_rows`` / ``wgnn_rows_topk`` on the GPU: against the fp64
restatement of tests/attrib_reference.py under its derived per-entry bound, bit-identical to ``wgnn_predict_rows`` where the
two overlap, pinned to logits the reference's own code produced, and end to end on hand-written bundles.

Worst observed error / bound ratios are printed by the kernel test (profiles/resident_explain.md records them)."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, ops

import attrib_reference as R
from test_gpu_resident_predict import _device_csr, _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _row_sums(rows, w, B):
    return np.bincount(rows, weights=w, minlength=B)


# ------------------------------------------------------------------------------------------------
# 1. the kernels against the fp64 reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,i64", R.KERNEL_CASES)
def test_kernel_matches_fp64_reference(H, i64):
    c = R.kernel_case(H, i64)
    B, m = c.B, c.m
    rp, col, raw = _device_csr(m, i64)
    table, alpha, bias = t(c.table), t(c.alpha), t(c.bias)
    worst = 0.0
    for C_ in R.KERNEL_CLASSES:
        for explicit in (False, True):
            w, b = c.heads[(C_, explicit)]
            sr = c.self_rows if explicit else None
            kw = dict(self_rows=None if sr is None else t(sr))
            thr = 1.5 / C_
            logits, label, _ = ops.predict_rows(rp, col, raw, table, alpha, bias, head=(t(w), t(b)), unsure_threshold=thr, **kw)
            _, argmax, _ = ops.predict_rows(rp, col, raw, table, alpha, bias, head=(t(w), t(b)), unsure_threshold=0.0, **kw)
            for target in (None, c.targets[C_]):
                run = lambda: ops.attrib_rows(rp, col, raw, table, alpha, bias, head=(t(w), t(b)), unsure_threshold=thr,
                                              target=None if target is None else t(target), want_direction=True, **kw)
                score, t_out, logit, base, lab, v = run()
                # the same bits as a classify call
                want_t = argmax if target is None else t(target)
                assert torch.equal(t_out, want_t) and torch.equal(lab, label)
                assert torch.equal(logit, logits.gather(1, t_out.long()[:, None])[:, 0])
                ref = R.attribution(m, [c.table], c.alpha, [c.bias], [None], w, b, target=t_out.cpu().numpy(), self_rows0=sr)
                und = ref.undecided[0]
                assert und.sum() <= 1e-3 * B * H
                if target is None:                             # where fp64 sees a clear maximum it is the kernel's
                    srt = np.sort(ref.logits, axis=1)
                    clear = srt[:, -1] - srt[:, -2] > 1e-5
                    np.testing.assert_array_equal(t_out.cpu().numpy()[clear], ref.logits.argmax(1)[clear])
                got = score.cpu().numpy().astype(np.float64)
                err = np.abs(got - ref.scores)
                ratio = float((err / np.maximum(ref.tol, 1e-300)).max())
                worst = max(worst, ratio)
                assert (err <= ref.tol).all(), (C_, explicit, target is not None, ratio)       # no entry left out
                # v = (z > 0) * Wh[t], away from the undecided units
                np.testing.assert_array_equal(v.cpu().numpy()[~und], ref.v[0].astype(np.float32)[~und])
                # base and completeness: sum_row(score) + base (+ the explicit self share) == logit
                base64, logit64 = base.cpu().numpy().astype(np.float64), logit.cpu().numpy().astype(np.float64)
                wt = np.abs(w.astype(np.float64)[ref.target])
                vb_mag = (np.abs(ref.v[0]) * np.abs(c.bias.astype(np.float64))).sum(1)
                flip = (und * wt * np.abs(c.bias.astype(np.float64))).sum(1)
                # base_out is b_head[t] plus an fp32 dot of H products: its error scales with sum |v_i b_i|, not with |base|
                assert (np.abs(base64 - ref.base) <= (H + 16) * R.EPS * (np.abs(b.astype(np.float64)[ref.target]) + vb_mag) + flip).all()
                bound = R.completeness_bound(got, base64, ref.rows, ref.deg, H)
                share = np.zeros(B)
                if explicit:                                   # the self rows' share is one more fp32 dot next to base
                    dev_v = v.cpu().numpy().astype(np.float64)
                    coef = float(c.alpha[c.G + 1]) / (ref.deg + 1)
                    share = coef * (sr.astype(np.float64) * dev_v).sum(1)
                    bound = bound + (ref.deg + H + 16) * R.EPS * (vb_mag + abs(coef) * (np.abs(sr.astype(np.float64)) * np.abs(dev_v)).sum(1))
                total = _row_sums(ref.rows, got, B) + base64 + share
                assert (np.abs(total - logit64) <= bound).all()
                # an empty cell: no score, base == logit (no self share without self rows)
                if not explicit:
                    assert base64[1] == logit64[1]
                # deterministic: a second launch is bit-identical
                again = run()
                assert all(torch.equal(x, y) for x, y in zip(again, (score, t_out, logit, base, lab, v)))
        # direction mode: overwrite, then accumulate, both coefficient rules
        rng = np.random.default_rng(7 * H + i64)
        d = rng.standard_normal((B, H)).astype(np.float32)
        for explicit in (False, True):
            over = ops.attrib_rows(rp, col, raw, table, alpha, bias, direction=t(d), explicit_self=explicit)
            want = R.direction_scores(m, c.table, c.alpha, d, explicit)
            u, rows, deg = R.message_weights(m, c.alpha, explicit)
            mag = np.einsum("ij,ij->i", np.abs(c.table.astype(np.float64)[m.indices]), np.abs(d.astype(np.float64))[rows])
            tol = (H + 2 * deg[rows] + 16) * R.EPS * np.abs(u) * mag
            err = np.abs(over.cpu().numpy() - want)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all()
            s0 = t(rng.standard_normal(m.nnz).astype(np.float32))
            acc = ops.attrib_rows(rp, col, raw, table, alpha, bias, direction=t(d), explicit_self=explicit, scores=s0.clone(),
                                  accumulate=True)
            assert torch.equal(acc, s0 + over)
            assert torch.equal(ops.attrib_rows(rp, col, raw, table, alpha, bias, direction=t(d), explicit_self=explicit), over)
    print(f"H={H} i64={i64}: worst |got - want| / bound = {worst:.3f}")


def test_target_out_of_range_and_gene_ids_are_refused():
    c = R.kernel_case(12, False)
    rp, col, raw = _device_csr(c.m, False)
    w, b = c.heads[(5, False)]
    args = (rp, col, raw, t(c.table), t(c.alpha), t(c.bias))
    bad_t = torch.full((c.B,), 5, dtype=torch.int32, device=DEV)
    with pytest.raises(sda.WgnnError, match="target class out of range"):
        ops.attrib_rows(*args, head=(t(w), t(b)), target=bad_t)
    bad = col.clone(); bad[1] = c.G
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.attrib_rows(rp, bad, raw, *args[3:], head=(t(w), t(b)))
    with pytest.raises(sda.WgnnError, match="LDS"):
        ops.attrib_rows(*args, head=(torch.zeros(2000, 12, device=DEV), torch.zeros(2000, device=DEV)))


def test_guard_words_around_every_output():
    """Direct C calls on buffers with sentinel words in front of and behind each output."""
    c = R.kernel_case(200, False)
    B, H, C_, nnz, k = c.B, 200, 16, c.m.nnz, 7
    rp, col, raw = _device_csr(c.m, False)
    table, alpha, bias = t(c.table), t(c.alpha), t(c.bias)
    w, b = (t(x) for x in c.heads[(C_, False)])
    PAD, SENT = 64, -12345.0

    def guarded(n, dtype=torch.float32):
        buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=DEV)
        return buf, buf[PAD:PAD + n]

    def intact(buf, n):
        return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all())

    bufs = {name: guarded(n, dt) for name, n, dt in (("score", nnz, torch.float32), ("dir", B * H, torch.float32),
                                                     ("target", B, torch.int32), ("logit", B, torch.float32),
                                                     ("base", B, torch.float32), ("label", B, torch.int32),
                                                     ("gene", B * k, torch.int32), ("top", B * k, torch.float32))}
    p = lambda name: bufs[name][1].data_ptr()
    rc = _lib.call(torch.device(DEV), "wgnn_attrib_rows", rp.data_ptr(), col.data_ptr(), raw.data_ptr(), B, table.data_ptr(), H,
                   c.G, H, alpha.data_ptr(), bias.data_ptr(), None, 0, w.data_ptr(), b.data_ptr(), C_, None, 0.1, p("label"),
                   None, 0, p("score"), p("target"), p("logit"), p("base"), p("dir"), H, 0, None)
    assert rc == 0
    rc = _lib.call(torch.device(DEV), "wgnn_rows_topk", rp.data_ptr(), col.data_ptr(), p("score"), B, k, p("gene"), p("top"), 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        assert intact(buf, view.numel()), name
    assert not bool((bufs["score"][1] == SENT).any()) and not bool((bufs["dir"][1] == SENT).any())
    want = ops.attrib_rows(rp, col, raw, table, alpha, bias, head=(w, b), unsure_threshold=0.1, want_direction=True)
    assert torch.equal(bufs["score"][1], want[0]) and torch.equal(bufs["dir"][1].view(B, H), want[5])


# ------------------------------------------------------------------------------------------------
# 2. top-k
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i64", [False, True])
def test_topk_equals_stable_argsort_of_the_device_scores(i64):
    rng = np.random.default_rng(11 + i64)
    lens = np.array([0, 1, 5, 64, 65, 200, 5000, 0, 63, 130, 3])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(rowptr[-1])
    col = rng.integers(0, 20000, nnz).astype(np.int32)
    s = rng.standard_normal(nnz).astype(np.float32)
    s[rng.random(nnz) < 0.5] = np.float32(0.25)               # repeated scores: ties go to the lower position
    s[rowptr[5]:rowptr[5] + 100] = np.float32(-1.0)
    s[rowptr[8]:rowptr[9]] = 0.0                              # a row of equal scores, with signed zeros
    s[rowptr[8] + 3] = -0.0
    rp = t(rowptr.astype(np.int64 if i64 else np.int32))
    dcol, ds = t(col), t(s)
    before = ds.clone()
    for k in (1, 3, 10, 64):
        gene, top = ops.rows_topk(rp, dcol, ds, k)
        want_g, want_s = R.stable_topk(rowptr, col, s, k)
        np.testing.assert_array_equal(gene.cpu().numpy(), want_g)
        np.testing.assert_array_equal(top.cpu().numpy(), want_s)
        g2, s2 = ops.rows_topk(rp, dcol, ds, k)
        assert torch.equal(g2, gene) and torch.equal(s2, top)
    assert torch.equal(ds, before)                            # the scores are only read
    with pytest.raises(sda.WgnnError):
        ops.rows_topk(rp, dcol, ds, 65)


# ------------------------------------------------------------------------------------------------
# 3. pinned to logits of the reference's own code
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refcode_1layer", "refcode_predict"])
def test_attribution_sums_to_executed_reference_logits(name):
    """Set up as test_kernel_matches_executed_reference_code: layer 1 runs in explicit-self mode (the fixture's features are
    random, not PCA), so the constant self rows' share alpha[G+1] <self1, v_1> / (deg + 1) stands next to ``base``."""
    z = np.load(GOLDEN / f"{name}.npz")
    sd = {k[len("param."):]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("param.")}
    expr = sp.csr_matrix(z["expr"]); G = expr.shape[1]
    mask = z["support_mask"].astype(bool)
    L = int(z["n_layers"])
    feats = torch.from_numpy(z["feats"]).to(DEV)
    test = sp.csr_matrix(expr[~mask])
    rp, col, raw = _device_csr(test, False)
    B = test.shape[0]
    rows = torch.from_numpy(np.repeat(np.arange(B), np.diff(test.indptr))).to(DEV)
    alpha = sd["alpha"].reshape(-1)
    W1, b1 = sd["layers.0.fc_neigh.weight"], sd["layers.0.fc_neigh.bias"]
    test_ids = torch.from_numpy(np.nonzero(~mask)[0]).to(DEV)
    table1 = ops.linear_fwd(feats[:G].contiguous(), W1)
    self1 = ops.linear_fwd(feats[G + test_ids].contiguous(), W1)
    head = (sd["linear.weight"], sd["linear.bias"])
    n_cls = head[0].shape[0]
    back = (alpha[G + 1] / ((rp[1:] - rp[:-1]).float() + 1.0))[:, None]
    want = z["logits"][~mask]
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
            total = torch.zeros(B, device=DEV, dtype=torch.float64).index_add_(0, rows, score.double()) + base.double() + share.double()
            np.testing.assert_allclose(total.cpu().numpy(), want[:, cls], atol=1e-5)
            np.testing.assert_allclose(logit.cpu().numpy(), want[:, cls], atol=1e-5)


# ------------------------------------------------------------------------------------------------
# 4. the predictor end to end
# ------------------------------------------------------------------------------------------------
def _batch(G, n=300, seed=7):
    batch = sp.random(n, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    batch.sort_indices()
    return batch


@pytest.mark.parametrize("n_layers,hidden", [(1, 12), (2, 12), (3, 12), (1, 20), (2, 20), (3, 20)])
def test_explain_end_to_end(tmp_path, n_layers, hidden):
    root, G = _random_bundle(tmp_path, n_layers, hidden=hidden, seed=n_layers + hidden)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    batch = _batch(G)
    label, _, logits = rp.classify(batch)
    att = rp.explain(batch, top_k=5)
    np.testing.assert_array_equal(att.label, label)
    np.testing.assert_array_equal(att.target, logits.argmax(1).cpu().numpy())
    assert torch.equal(torch.from_numpy(att.logit).to(DEV), logits.max(1).values)
    cpu = lambda x: None if x is None else x.cpu().numpy()
    ref = R.attribution(batch, [cpu(x) for x in rp.tables], cpu(rp.alpha), [cpu(x) for x in rp.biases],
                        [cpu(x) for x in rp.self_weights], cpu(rp.w_head), cpu(rp.b_head), target=att.target)
    got = att.scores.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref.scores)
    print(f"L={n_layers} H={hidden}: worst |got - want| / bound = {float((err / np.maximum(ref.tol, 1e-300)).max()):.3f}, "
          f"undecided units {sum(int(u.sum()) for u in ref.undecided)}")
    assert (err <= ref.tol).all()
    # base gathers one <v_l, b_l> per layer and the scores one pass per layer: the one-layer bound once per layer
    bound = n_layers * R.completeness_bound(got, att.base.astype(np.float64), ref.rows, ref.deg, hidden)
    total = _row_sums(ref.rows, got, batch.shape[0]) + att.base
    assert (np.abs(total - att.logit) <= bound).all()
    want_g, want_s = R.stable_topk(batch.indptr, batch.indices, att.scores.cpu().numpy(), 5)
    np.testing.assert_array_equal(att.top_genes, want_g)
    np.testing.assert_array_equal(att.top_scores, want_s)
    assert att.gene_names(0) == [f"Gene{g}" for g in want_g[0] if g >= 0]
    # another class, by name; a device triple gives the same bits; an out-of-range gene id raises
    other = rp.explain(batch, top_k=0, target="type3")
    assert (other.target == 3).all() and torch.equal(torch.from_numpy(other.logit).to(DEV), logits[:, 3])
    np.testing.assert_array_equal(other.label, label)
    dev_csr = (torch.from_numpy(batch.indptr.astype(np.int64)).to(DEV), torch.from_numpy(batch.indices).to(DEV),
               torch.from_numpy(batch.data).to(DEV))
    same = rp.explain(dev_csr, top_k=5)
    assert torch.equal(same.scores, att.scores) and np.array_equal(same.base, att.base) and np.array_equal(same.top_genes, att.top_genes)
    bad = (dev_csr[0], dev_csr[1].clone().index_fill_(0, torch.tensor([0], device=DEV), G), dev_csr[2])
    with pytest.raises(sda.WgnnError, match="out of range"):
        rp.explain(bad)


def test_one_layer_explain_is_two_launches(tmp_path):
    from torch.profiler import ProfilerActivity, profile
    root, G = _random_bundle(tmp_path, 1, seed=3)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    batch = _batch(G, 1000, 9)
    rp.explain(batch)                                         # warm-up
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        att = rp.explain(batch, top_k=10)
        torch.cuda.synchronize()
    assert att.top_genes.shape == (1000, 10)
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    assert len(kernels) == 2 and "attrib_rows" in kernels[0] and "rows_topk" in kernels[1], kernels


def test_planted_marker_gene_is_rank_one(tmp_path):
    """Class 2's head weight reads hidden unit 5 alone, and unit 5 is fed by gene 17 alone: every cell predicted class 2
    that expresses gene 17 must name it first."""
    root, G = _random_bundle(tmp_path, 1, seed=5)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root)
    g_star, unit, cls = 17, 5, 2
    gen = torch.Generator(device="cpu").manual_seed(1)
    table = 0.05 * torch.randn(G, rp.hidden_padded, generator=gen)
    table[:, unit] = 0.0
    table[g_star, unit] = 2000.0
    w = 0.5 * torch.randn(rp.n_classes, rp.hidden_padded, generator=gen)
    w[:, unit] = 0.0
    w[cls] = 0.0
    w[cls, unit] = 1.0
    rp.tables[0], rp.w_head = table.to(DEV), w.to(DEV)
    rp.biases[0].zero_(); rp.b_head.zero_()
    rp.b_head[cls] = -0.2                                     # without the gene the class loses to the others
    batch = _batch(G, 400, 21)
    att = rp.explain(batch, top_k=3)
    expresses = np.asarray((batch[:, g_star] != 0).todense()).ravel()
    hit = (att.label == cls) & expresses
    assert hit.sum() >= 10 and not ((att.label == cls) & ~expresses).any()
    assert (att.top_genes[hit, 0] == g_star).all() and (att.top_scores[hit, 0] > 0).all()
    assert (att.top_scores[hit, 1] == 0).all()               # nothing else feeds that logit
