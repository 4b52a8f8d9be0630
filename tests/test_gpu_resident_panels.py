"""``wgnn_predict_rows_panels`` and ``ResidentPredictor.panels`` on the GPU: every (cell, panel) pair within ``TOL`` of the fp64
restatement of tests/panels_reference.py; THE BITS of ``predict_rows`` on the materialised sub-row (values mode) and on the
lognorm-aligned count matrix with the other columns zeroed (counts mode); determinism, splitting by cells and by panels, the
bits above ``n_panels``, guard rows and columns; and the predictor end to end against ``classify`` of the masked batch."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

import panels_reference as N
import stability_reference as R
import thin_reference as T
from test_gpu_resident_predict import _random_bundle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5                                                        # test_gpu_resident_predict.py's, for this same gather


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words(member):
    return t(N.pack(member).view(np.int64))


def _device_csr(m, i64):
    return t(m.indptr.astype(np.int64 if i64 else np.int32)), t(m.indices.astype(np.int32)), t(m.data.astype(np.float32))


def _run_case(c, i64, P=None, **kw):
    """(out, entries) without a head and (logits, label, max_prob, entries) with it, of one reference case."""
    P = c["member"].shape[0] if P is None else P
    args = (*_device_csr(c["m"], i64), t(c["table"]), t(c["alpha"]), t(c["bias"]), words(c["member"]), P)
    common = dict(self_rows=t(c["self_rows"]), want_entries=True, **kw)
    if "lib" in c:
        common.update(lib=t(c["lib"]), scale=c["scale"], threshold=c["vthr"])
    return (ops.predict_rows_panels(*args, **common),
            ops.predict_rows_panels(*args, head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], want_logits=True, **common))


def _against_reference(case, c, got):
    (out, entries0), (logits, label, prob, entries) = got
    B, P = c["entries"].shape
    np.testing.assert_array_equal(entries.cpu().numpy(), c["entries"])             # which entries take part, exactly
    assert torch.equal(entries0, entries)
    err_h = float(np.abs(out.cpu().numpy() - c["out"]).max())
    err_p = float(np.abs(prob.cpu().numpy() - c["prob"]).max())
    err_l = float(np.abs(logits.cpu().numpy().reshape(B, P, -1) - c["logits"]).max())
    share = float(c["unclear"].mean())
    print(f"case {case}: max |out - want| = {err_h:.3e} (scale {max(1.0, np.abs(c['out']).max()):.3f}), max |max_prob - want| = "
          f"{err_p:.3e}, max |logits - want| = {err_l:.3e}, unclear pairs {share:.4f}")
    assert err_h <= TOL * max(1.0, float(np.abs(c["out"]).max()))
    assert err_p <= TOL * max(1.0, float(np.abs(c["prob"]).max()))
    assert share <= 0.05
    clear = ~c["unclear"]
    np.testing.assert_array_equal(label.cpu().numpy()[clear], c["label"][clear])
    # the empty pairs, exactly: ReLU(bias (+ alpha[G + 1] self_rows)) in the kernel's own operations
    empty = t(c["empty"].reshape(-1))
    z = t(c["bias"])[None, :].expand(B * P, -1)
    if c["self_rows"] is not None:
        z = t(c["self_rows"]) * t(c["alpha"])[-1] + z              # two roundings, as the kernel's fma onto 0 and its epilogue
    assert int(empty.sum()) >= P and torch.equal(out[empty], torch.relu(z)[empty])


# ------------------------------------------------------------------------------------------------
# 1. against the fp64 reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.PANEL_CASES, ids=str)
def test_panels_match_the_fp64_reference(case):
    H, Cn, explicit, i64, P = case
    c = N.panel_case(H, Cn, explicit, P)
    _against_reference(case, c, _run_case(c, i64))


@pytest.mark.parametrize("case", N.COUNT_CASES, ids=str)
def test_count_panels_match_the_fp64_reference(case):
    H, Cn, explicit, i64, P, vthr = case
    c = N.count_case(H, Cn, explicit, P, vthr)
    _against_reference(case, c, _run_case(c, i64))


# ------------------------------------------------------------------------------------------------
# 2. the bits of predict_rows
# ------------------------------------------------------------------------------------------------
BITS_P = 12                                                        # no multiple of the 8 waves; every kind of panel twice


@pytest.mark.parametrize("H", [12, 64, 200, 256])
def test_values_mode_carries_the_bits_of_predict_rows_on_the_sub_row(H):
    m, table, alpha, bias = R.operands(H)
    B, G = m.shape
    P = BITS_P
    member = N.membership(G, P)
    table, alpha, bias, mw = t(table), t(alpha), t(bias), words(member)
    for i64 in (False, True):
        whole = _device_csr(m, i64)
        subs = [_device_csr(R.thinned(m, N.kept_entries(m, member[p])), i64) for p in range(P)]
        assert all(torch.equal(a, b) for a, b in zip(subs[0], whole))              # the all-genes panel is the batch itself
        assert int(subs[7][0][4] - subs[7][0][3]) > 1024                           # the long row outgrows the stash at density 0.9
        for explicit in (False, True):
            sr = t(R.self_operand(H, B * P)) if explicit else None
            pair_rows = lambda p: None if sr is None else sr[p::P].contiguous()
            got, entries = ops.predict_rows_panels(*whole, table, alpha, bias, mw, P, self_rows=sr, want_entries=True)
            for p in range(P):
                assert torch.equal(got[p::P], ops.predict_rows(*subs[p], table, alpha, bias, self_rows=pair_rows(p))), (i64, explicit, p)
                assert torch.equal(entries[:, p], (subs[p][0][1:] - subs[p][0][:-1]).int())
            for Cn in (2, 16, 40):
                head = dict(head=tuple(t(a) for a in R.head_operands(H, Cn)), unsure_threshold=R.full_threshold(H, Cn, explicit))
                logits, label, prob = ops.predict_rows_panels(*whole, table, alpha, bias, mw, P, self_rows=sr, want_logits=True, **head)
                for p in range(P):
                    want = ops.predict_rows(*subs[p], table, alpha, bias, self_rows=pair_rows(p), **head)
                    assert torch.equal(logits[p::P], want[0]) and torch.equal(label[:, p], want[1]) \
                        and torch.equal(prob[:, p], want[2]), (i64, explicit, Cn, p)


@pytest.mark.parametrize("vthr", [0.0, 1.5])
@pytest.mark.parametrize("H,i64", [(12, False), (200, True)])
def test_counts_mode_carries_the_bits_of_predict_rows_on_the_aligned_zeroed_counts(H, i64, vthr):
    m, rest = T.count_batch()
    _, table, alpha, bias = (t(a) if not sp.issparse(a) else a for a in R.operands(H))
    B, G = m.shape
    P, Cn = 9, 16
    member = N.membership(G, P)
    lib = N.panel_reads(m, rest, member)
    assert (lib[:, 1] == 0).any() and (lib[:, 1] > 0).any()        # the empty panel: `rest` alone, 0 on some cells
    gene_map = t(np.concatenate([np.arange(G), [-1]]).astype(np.int32))            # one more column, outside the bundle
    subs, dropped = [], False
    for p in range(P):
        x = N.zeroed_dense(m, rest, member[p], p % 2 == 1)
        subs.append(ops.align_rows(t(x), gene_map, G, vthr, normalize="lognorm", scale=T.SCALE))
        dropped |= int(subs[p][1].shape[0]) < int((x[:, :G] > 0).sum())
    assert dropped == (vthr > 0)                                   # the positive threshold drops entries
    counts = _device_csr(m, i64)
    kw = dict(lib=t(lib), scale=T.SCALE, threshold=vthr)
    for explicit in (False, True):
        sr = t(R.self_operand(H, B * P)) if explicit else None
        pair_rows = lambda p: None if sr is None else sr[p::P].contiguous()
        got, entries = ops.predict_rows_panels(*counts, table, alpha, bias, words(member), P, self_rows=sr, want_entries=True, **kw)
        head = dict(head=tuple(t(a) for a in R.head_operands(H, Cn)), unsure_threshold=T.full_threshold(H, Cn, explicit, vthr))
        logits, label, prob = ops.predict_rows_panels(*counts, table, alpha, bias, words(member), P, self_rows=sr, want_logits=True,
                                                      **head, **kw)
        for p in range(P):
            assert torch.equal(got[p::P], ops.predict_rows(*subs[p], table, alpha, bias, self_rows=pair_rows(p))), (explicit, p)
            assert torch.equal(entries[:, p], (subs[p][0][1:] - subs[p][0][:-1]).int())
            want = ops.predict_rows(*subs[p], table, alpha, bias, self_rows=pair_rows(p), **head)
            assert torch.equal(logits[p::P], want[0]) and torch.equal(label[:, p], want[1]) and torch.equal(prob[:, p], want[2])
    # lib <= 0 is the empty row, whatever the counts
    none = torch.zeros((B, P), dtype=torch.int64, device=DEV)
    none[:, ::2] = -7
    out, entries = ops.predict_rows_panels(*counts, table, alpha, bias, words(member), P, want_entries=True, **{**kw, "lib": none})
    assert torch.equal(out, torch.relu(bias)[None, :].expand(B * P, H)) and not entries.any()


# ------------------------------------------------------------------------------------------------
# 3. structure
# ------------------------------------------------------------------------------------------------
def test_determinism_and_splitting_by_cells_and_panels():
    H, Cn, P = 64, 40, 64
    c = N.panel_case(H, Cn, True, P)
    m, B = c["m"], c["m"].shape[0]
    (out, ent0), tabs = _run_case(c, False)
    (out2, _), tabs2 = _run_case(c, False)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    rp, col, raw = _device_csr(m, False)
    args = (col, raw, t(c["table"]), t(c["alpha"]), t(c["bias"]))
    head = dict(head=(t(c["w"]), t(c["b"])), unsure_threshold=c["thr"], want_logits=True, want_entries=True)
    sr, mw = t(c["self_rows"]), words(c["member"])
    cut = 17                                                       # the cells in two launches
    parts = [ops.predict_rows_panels(rp[:cut + 1], *args, mw, P, self_rows=sr[:cut * P], **head),
             ops.predict_rows_panels(rp[cut:], *args, mw, P, self_rows=sr[cut * P:], **head)]
    for whole, a, b in zip(tabs, *parts):
        assert torch.equal(whole, torch.cat([a, b]))
    assert torch.equal(out[cut * P:], ops.predict_rows_panels(rp[cut:], *args, mw, P, self_rows=sr[cut * P:]))
    P1 = 40                                                        # the panels in two launches, `member` shifted accordingly
    srv = sr.view(B, P, H)
    lo = ops.predict_rows_panels(rp, *args, words(c["member"][:P1]), P1, self_rows=srv[:, :P1].reshape(-1, H), **head)
    hi = ops.predict_rows_panels(rp, *args, words(c["member"][P1:]), P - P1, self_rows=srv[:, P1:].reshape(-1, H), **head)
    Cl = tabs[0].shape[1]
    assert torch.equal(torch.cat([lo[0].view(B, P1, Cl), hi[0].view(B, P - P1, Cl)], dim=1).reshape(B * P, Cl), tabs[0])
    for i in (1, 2, 3):
        assert torch.equal(torch.cat([lo[i], hi[i]], dim=1), tabs[i])
    # bits of `member` at or above n_panels are ignored
    few = ops.predict_rows_panels(rp, *args, mw, 9, self_rows=srv[:, :9].reshape(-1, H), **head)
    own = ops.predict_rows_panels(rp, *args, words(c["member"][:9]), 9, self_rows=srv[:, :9].reshape(-1, H), **head)
    assert all(torch.equal(a, b) for a, b in zip(few, own)) and torch.equal(few[1], tabs[1][:, :9])


def test_outputs_stay_inside_their_views():
    H, Cn, P, vthr = 12, 16, 9, 0.0
    c = N.count_case(64, Cn, False, P, vthr)                       # the counts, the membership and lib; H = 12 operands below
    _, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, Cn)
    m, B = c["m"], c["m"].shape[0]
    rp, col, raw = _device_csr(m, True)
    table, alpha, bias, w, b, mw = t(table), t(alpha), t(bias), t(w), t(b), words(c["member"])
    G0, G1, PAD = 3, 2, 5                                          # guard rows before / after, guard columns
    n = B * P
    lib_buf = torch.full((G0 + B + G1, P + PAD), 2 ** 40, dtype=torch.int64, device=DEV)      # a sentinel no cell's reads reach
    lib_buf[G0:G0 + B, :P] = t(c["lib"])
    lib = lib_buf[G0:G0 + B, :P]
    kw = dict(lib=lib, scale=c["scale"], threshold=vthr)
    free = ops.predict_rows_panels(rp, col, raw, table, alpha, bias, mw, P, want_entries=True, **kw)
    free_head = ops.predict_rows_panels(rp, col, raw, table, alpha, bias, mw, P, head=(w, b), unsure_threshold=0.3,
                                        want_logits=True, want_entries=True, **kw)
    assert torch.equal(free[0], ops.predict_rows_panels(rp, col, raw, table, alpha, bias, mw, P, **{**kw, "lib": t(c["lib"])}))
    # out through ops: a view with a wider row stride and guard rows
    out_buf = torch.full((G0 + n + G1, H + 8), float("nan"), dtype=torch.float32, device=DEV)
    o = ops.predict_rows_panels(rp, col, raw, table, alpha, bias, mw, P, out=out_buf[G0:G0 + n, :H], **kw)
    assert torch.equal(o, free[0]) and torch.isnan(out_buf[:G0]).all() and torch.isnan(out_buf[G0 + n:]).all()
    assert torch.isnan(out_buf[:, H:]).all()
    # the head's outputs through the C entry: ld_logits wider than C, guard rows around every table
    ints = lambda *shape: torch.full(shape, -12345, dtype=torch.int32, device=DEV)
    logits_buf = torch.full((G0 + n + G1, Cn + PAD), float("nan"), dtype=torch.float32, device=DEV)
    label_buf, entries_buf = ints((G0 + B + G1) * P), ints((G0 + B + G1) * P)
    prob_buf = torch.full(((G0 + B + G1) * P,), float("nan"), dtype=torch.float32, device=DEV)
    p_ = ops._ptr
    rc = _lib.call(torch.device(DEV), "wgnn_predict_rows_panels", p_(rp), p_(col), p_(raw), B, p_(table), table.stride(0), m.shape[1], H,
                   p_(alpha), p_(bias), None, 0, p_(mw), P, p_(lib), lib.stride(0), float(c["scale"]), vthr, None, 0,
                   p_(w), p_(b), Cn, 0.3, p_(logits_buf[G0:]), logits_buf.stride(0), p_(label_buf[G0 * P:]), p_(prob_buf[G0 * P:]),
                   p_(entries_buf[G0 * P:]), _lib.FLAG_ROWPTR_I64, ops._stream(torch.device(DEV)))
    _lib.check(rc, "wgnn_predict_rows_panels")
    torch.cuda.synchronize()
    rows = slice(G0 * P, (G0 + B) * P)
    assert torch.equal(logits_buf[G0:G0 + n, :Cn], free_head[0]) and torch.isnan(logits_buf[:, Cn:]).all()
    assert torch.isnan(logits_buf[:G0]).all() and torch.isnan(logits_buf[G0 + n:]).all()
    assert torch.equal(label_buf[rows].view(B, P), free_head[1]) and torch.equal(prob_buf[rows].view(B, P), free_head[2])
    assert torch.equal(entries_buf[rows].view(B, P), free_head[3]) and torch.equal(free_head[3], free[1])
    for buf in (label_buf, entries_buf):
        assert (buf[:G0 * P] == -12345).all() and (buf[(G0 + B) * P:] == -12345).all()
    assert torch.isnan(prob_buf[:G0 * P]).all() and torch.isnan(prob_buf[(G0 + B) * P:]).all()


def test_ops_argument_errors():
    rp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    col, raw = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV)
    table, alpha, bias = torch.zeros(3, 8, device=DEV), torch.ones(5, device=DEV), torch.zeros(8, device=DEV)
    member = torch.ones(3, dtype=torch.int64, device=DEV)
    lib = torch.ones((1, 2), dtype=torch.int64, device=DEV)
    ok = ops.predict_rows_panels(rp, col, raw, table, alpha, bias, member, 2, lib=lib)
    assert ok.shape == (2, 8)
    for kw in (dict(n_panels=0), dict(n_panels=65), dict(member=member.int()), dict(member=member[:2]), dict(lib=lib.int()),
               dict(lib=lib[:, :1]), dict(lib=lib, scale=0.0), dict(lib=lib, threshold=-1.0), dict(lib=lib, threshold=float("nan")),
               dict(self_rows=torch.zeros(3, 8, device=DEV)), dict(out=torch.zeros(3, 8, device=DEV))):
        a = {"member": member, "n_panels": 2, **kw}
        with pytest.raises(ValueError):
            ops.predict_rows_panels(rp, col, raw, table, alpha, bias, a.pop("member"), a.pop("n_panels"), **a)
    with pytest.raises(sda.WgnnError, match="out of range"):
        ops.predict_rows_panels(rp, torch.full_like(col, 3), raw, table, alpha, bias, member, 2)


# ------------------------------------------------------------------------------------------------
# 4. end to end
# ------------------------------------------------------------------------------------------------
N_PANELS = 70                                                      # two launches per layer


def _batch(rp, G, n=40, seed=3):
    """Counts over the caller's own columns: 300 bundle genes shuffled, 20 names outside the bundle mixed in."""
    rng = np.random.default_rng(seed)
    genes = [rp.id2gene[i] for i in rng.permutation(G)[:300]] + [f"NotAGene{i}" for i in range(20)]
    genes = [genes[i] for i in rng.permutation(len(genes))]
    counts = rng.geometric(0.5, (n, len(genes))) * (rng.random((n, len(genes))) < 0.25)
    return counts.astype(np.float32), genes


def _specs(names, seed=9):
    """70 panels over the gene names ``names``: keep lists of several sizes, complements, one with names that do not exist."""
    rng = np.random.default_rng(seed)
    pick = lambda k: [names[i] for i in rng.choice(len(names), size=k, replace=False)]
    keep = {f"keep{i}": pick((5, 40, 150, len(names))[i % 4]) for i in range(N_PANELS - 30)}
    keep["keep1"] = keep["keep1"] + ["Nowhere1", "Nowhere2"]
    without = {f"without{i}": pick((0, 10, 100)[i % 3]) for i in range(30)}
    without["without2"] = without["without2"] + ["Nowhere3"]
    return keep, without


def _column_masks(keep, without, columns):
    cols = np.array(columns)
    return [np.isin(cols, v) for v in keep.values()] + [~np.isin(cols, v) for v in without.values()]


@pytest.mark.parametrize("n_layers", [1, 2])
def test_panels_end_to_end(tmp_path, monkeypatch, n_layers):
    root, G = _random_bundle(tmp_path, n_layers, hidden=12, seed=n_layers + 20)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)
    counts, genes = _batch(rp, G)
    B = counts.shape[0]
    matched = np.array([g in rp._gene2id for g in genes])
    keep, without = _specs(genes)
    masks = _column_masks(keep, without, genes)
    names = list(keep) + list(without)
    missing = {n: [] for n in names}
    missing["keep1"], missing["without2"] = ["Nowhere1", "Nowhere2"], ["Nowhere3"]

    def check(pc, classify_masked, values, mask_list, n_cols):
        label, prob, _ = classify_masked(None)
        np.testing.assert_array_equal(pc.label, label); np.testing.assert_array_equal(pc.max_prob, prob)       # classify's own
        assert pc.names == names and pc.missing == missing and pc.panel_label.shape == (B, N_PANELS)
        for p, mask in enumerate(mask_list):
            lab, pr, _ = classify_masked(mask)
            np.testing.assert_array_equal(pc.panel_label[:, p], lab, err_msg=names[p])
            np.testing.assert_array_equal(pc.panel_prob[:, p], pr, err_msg=names[p])                           # bit for bit
        if n_cols:
            np.testing.assert_array_equal(pc.n_columns, [int(k.sum()) for k in mask_list])
            np.testing.assert_array_equal(pc.n_genes, [int((k & matched).sum()) for k in mask_list])
            np.testing.assert_array_equal(pc.n_entries, np.stack([((values > 0) & (k & matched)).sum(axis=1) for k in mask_list], 1))
        assert len(pc.frame()) == B and len(pc.by_type()) and "agreement" in str(pc.summary())

    # the values as given, over the caller's columns
    values = np.log1p(counts)
    pc = rp.panels(values, panels=keep, without=without, genes=genes)
    check(pc, lambda k: rp.classify(values if k is None else values * k, genes=genes), values, masks, True)
    assert pc.n_reads is None and not pc.renormalize
    # chunked by a tiny byte budget: the same tables
    monkeypatch.setattr(api, "STABILITY_CHUNK_BYTES", 64 * rp.hidden_padded * 4 * 3 * 7)
    again = rp.panels(values, panels=keep, without=without, genes=genes)
    monkeypatch.undo()
    np.testing.assert_array_equal(again.panel_label, pc.panel_label); np.testing.assert_array_equal(again.panel_prob, pc.panel_prob)
    np.testing.assert_array_equal(again.n_entries, pc.n_entries)
    # raw counts, re-normalised per panel against the panel's own reads (columns outside the bundle included)
    rn = rp.panels(counts, panels=keep, without=without, genes=genes, normalize="lognorm", renormalize=True)
    check(rn, lambda k: rp.classify(counts if k is None else counts * k, genes=genes, normalize="lognorm"), counts, masks, True)
    np.testing.assert_array_equal(rn.n_reads, np.stack([(counts * k).sum(axis=1) for k in masks], 1).astype(np.int64))
    assert rn.renormalize and "reads_keep0" in rn.frame().columns
    # the same counts as a CSR over the caller's columns: the library sizes come from index_add_, the same tables
    rc = rp.panels(sp.csr_matrix(counts), panels=keep, without=without, genes=genes, normalize="lognorm", renormalize=True)
    for a, b in ((rc.panel_label, rn.panel_label), (rc.panel_prob, rn.panel_prob), (rc.n_reads, rn.n_reads), (rc.n_entries, rn.n_entries)):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(sda.WgnnError, match="cell 3"):
        bad = counts.copy(); bad[3, int(np.flatnonzero(matched)[0])] = 2.5
        rp.panels(bad, panels=keep, genes=genes, normalize="lognorm", renormalize=True)
    # over the bundle's own gene ids
    batch = sp.random(B, G, density=0.1, random_state=5, format="csr", dtype=np.float32)
    batch.data = 1.0 + 4.0 * batch.data
    batch.sort_indices()
    keep_b, without_b = _specs(list(rp.id2gene), seed=4)
    masks_b = _column_masks(keep_b, without_b, list(rp.id2gene))

    def sub_batch(k):
        sub = batch if k is None else batch.multiply(k[None, :]).tocsr()
        sub.eliminate_zeros()
        sub.sort_indices()
        return sub

    masked = lambda k: rp.classify(sub_batch(k))

    pb = rp.panels(batch, panels=keep_b, without=without_b)
    check(pb, masked, None, masks_b, False)
    assert pb.n_columns is None
    np.testing.assert_array_equal(pb.n_genes, [int(k.sum()) for k in masks_b])
    np.testing.assert_array_equal(pb.n_entries, np.stack([np.diff(sub_batch(k).indptr) for k in masks_b], 1))
    monkeypatch.setattr(rp, "hidden_padded", 260)
    with pytest.raises(ValueError, match="fused"):
        rp.panels(batch, panels=keep_b)


def test_panels_file_writes_the_table(tmp_path):
    import pandas as pd
    root, G = _random_bundle(tmp_path, 2, seed=4)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.2)      # a rate at which the random model makes calls
    counts, genes = _batch(rp, G, n=30, seed=1)
    cells = [f"C{j}" for j in range(counts.shape[0])]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(counts.T, index=genes, columns=cells).to_csv(data)
    spec = dict(panels={"probe": genes[:120]}, without={"spikes": genes[200:230]})
    out = rp.panels_file(data, normalize="lognorm", renormalize=True, save_path=tmp_path / "res", **spec)
    written = pd.read_csv(tmp_path / "res" / "mouse_Rand_panels.csv")
    cols = ["panel", "cell_type", "n_cells", "retained", "unsure", "other", "other_share"]
    assert list(out.columns) == cols and list(written.columns) == cols and len(written) == len(out) > 0
    want = rp.panels(counts, genes=genes, normalize="lognorm", renormalize=True, index=cells, **spec).by_type()
    assert out["panel"].tolist() == want["panel"].tolist() and out["cell_type"].tolist() == want["cell_type"].tolist()
    np.testing.assert_array_equal(out["retained"], want["retained"]); np.testing.assert_array_equal(written["n_cells"], want["n_cells"])
