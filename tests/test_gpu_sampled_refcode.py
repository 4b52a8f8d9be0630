"""Neighbour-sampled training (num_neighbors > 0, train.py:37-40,71-78) on the HIP path against the logits, loss and
gradients that the reference's own GNN.forward computed over recorded draws (tests/golden/refcode_sampled.npz, written by
tests/golden/make_refcode_golden.py).

Each recorded draw is turned into the product's own blocks: the CSR block of ``sampler.block_from_draw`` and K5's ELL
layout through ``sampler.ell_block_from_draw``.  The edge values come from the device-normalised parent graph, not from
the fixture.  So the normalisation, the block assembly, ``GNN.embed_sampled`` and the aggregation kernels, forward and
backward, are all inside what is compared.  The backward transposes a CSR block with the device transpose kernel and an
ELL block with the sentinel sort.  A CSR block is also served by the LDS-streamed tile kernels once ``ops.TILED_MIN_WORK``
is lowered (``csr_tiled``); an ELL block never is (``ops.tiled_kernel_serves``)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from conftest import GOLDEN
from scdeepsort_amd import ops
from scdeepsort_amd.sampler import NodeFlow, block_from_draw, ell_block_from_draw
from test_gpu_parity import DEV, TOL, dev, make_model

pytestmark = pytest.mark.gpu
CASES = ["L1k3", "L2k1", "L2k3", "L2k7"]
FORMS = ["csr", "csr_tiled", "ell"]


def load_case(prefix):
    z = np.load(GOLDEN / "refcode_sampled.npz")
    assert list(z["cases"]) == CASES
    sd = {k[len(prefix) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix + ".param.")}
    draw = {}
    for b, d, s in zip(z[prefix + ".draw_block"].tolist(), z[prefix + ".draw_dst"].tolist(), z[prefix + ".draw_src"].tolist()):
        draw.setdefault((b, d), []).append(s)
    return z, sd, draw


def layer_above(z, prefix, b):
    """Node ids of the layer block ``b`` feeds, in the order the draw lists them (the seed order for the last block)."""
    d = z[prefix + ".draw_dst"][z[prefix + ".draw_block"] == b]
    _, first = np.unique(d, return_index=True)
    return d[np.sort(first)]


def drawn_block(parent, draw, b, rows, shift, G, k, form):
    """The block of one node type: ``rows`` are rows of ``parent`` (cells: node id = row + G, ``shift`` = G; genes:
    node id = row, ``shift`` = 0).  Rows the draw does not list (ELL blocks cover every node) keep their self-loop only."""
    rows = np.asarray(rows, dtype=np.int64)
    rp = parent.rowptr.cpu().numpy().astype(np.int64)
    col, val = parent.col.cpu().numpy(), parent.val.cpu().numpy()
    owner, pos, selfd, per_row = [], [], [], []
    for j, r in enumerate(rows.tolist()):
        v = r + shift
        srcs = draw.get((b, v), [v])
        at = {int(c): i for i, c in enumerate(col[rp[r]:rp[r + 1]])}
        p = sorted(at[s - (G - shift)] for s in srcs if s != v)            # KeyError: a drawn edge the parent does not hold
        owner += [j] * len(p)
        pos += p
        selfd.append(float(v in srcs))
        per_row.append(np.asarray(p, dtype=np.int64))
    d = parent.device
    rows_t = torch.from_numpy(rows).to(d)
    if form != "ell":
        return block_from_draw(parent, rows_t, torch.tensor(owner, dtype=torch.int64, device=d),
                               torch.tensor(pos, dtype=torch.int64, device=d), torch.tensor(selfd, device=d), k)
    n, kk = len(rows), max(1, min(k, parent.max_row_nnz + 1))
    out_col = np.zeros(max(1, n * kk), np.int32)
    out_val = np.zeros(max(1, n * kk), np.float32)
    cnt = np.zeros(n, np.int32)
    rng = np.random.default_rng(n)
    for j, p in enumerate(per_row):
        e = rp[rows[j]] + rng.permutation(p)                # K5 writes a row's edges in draw order, not ascending
        out_col[j * kk: j * kk + len(e)], out_val[j * kk: j * kk + len(e)], cnt[j] = col[e], val[e], len(e)
    inv = (1.0 / np.maximum(1, cnt + np.asarray(selfd))).astype(np.float32)
    return ell_block_from_draw(parent, rows_t, kk, torch.from_numpy(out_col).to(d), torch.from_numpy(out_val).to(d),
                               torch.from_numpy(cnt).to(d), torch.tensor(selfd, device=d), torch.from_numpy(inv).to(d))


def recorded_nodeflow(g, z, prefix, draw, form):
    G, L, k = g.num_genes, int(z[prefix + ".n_layers"]), int(z[prefix + ".k"])
    blocks = []
    for b in range(L):
        nodes = layer_above(z, prefix, b)
        cells, genes = nodes[nodes >= G] - G, nodes[nodes < G]
        if b == L - 1:
            assert np.array_equal(cells + G, z[prefix + ".seeds"]) and len(genes) == 0
        elif form == "ell":                                 # lower K5 blocks cover every node (sample_nodeflow_static)
            cells, genes = np.arange(g.num_cells), np.arange(G)
        cb = drawn_block(g.cg, draw, b, cells, G, G, k, form)
        gb = drawn_block(g.gc, draw, b, genes, 0, G, k, form) if len(genes) else None
        blocks.append((cb, gb))
    return NodeFlow(blocks)


def setup(prefix, form, monkeypatch):
    z, sd, draw = load_case(prefix)
    expr = sp.csr_matrix(z["expr"])
    g = sda.CellGeneGraph.from_expression(expr, z["support_mask"], device=DEV)
    m = make_model(sd, int(z["dim"]), int(z["hidden"]), int(z["n_classes"]), int(z[prefix + ".n_layers"]), expr.shape[1])
    if form == "csr_tiled":
        monkeypatch.setattr(ops, "TILED_MIN_WORK", 1)
    nf = recorded_nodeflow(g, z, prefix, draw, form)
    if form == "csr_tiled":                                 # every non-empty block, at both padded widths (10 -> 12, 6 -> 8)
        served = [ops.tiled_kernel_serves(blk.csr, D) for pair in nf.blocks for blk in pair
                  if blk is not None and blk.csr.nnz for D in (8, 12)]
        assert served and all(served)
    return z, g, m, nf


@pytest.mark.parametrize("prefix", CASES)
@pytest.mark.parametrize("form", ["csr", "ell"])
def test_blocks_hold_the_recorded_draw(prefix, form, monkeypatch):
    """Per node: the recorded number of real edges, the recorded self-loop flag, 1 / (number of drawn edges), and the
    recorded sources."""
    z, g, m, nf = setup(prefix, form, monkeypatch)
    _, _, draw = load_case(prefix)
    G = g.num_genes
    for b, pair in enumerate(nf.blocks):
        for blk, shift in zip(pair, (G, 0)):
            if blk is None:
                continue
            rows = blk.rows.cpu().numpy()
            col = blk.csr.col.cpu().numpy().astype(np.int64)
            if form == "ell":
                cnt, kk = blk.csr.ell_cnt.cpu().numpy(), blk.csr.ell_k
                start = np.arange(len(rows)) * kk
            else:
                rp = blk.csr.rowptr.cpu().numpy()
                start, cnt = rp[:-1], np.diff(rp)
            self_drawn, inv = blk.self_drawn.cpu().numpy(), blk.csr.inv_deg.cpu().numpy()
            listed = 0
            for j, r in enumerate(rows.tolist()):
                v = r + shift
                if (b, v) not in draw:
                    assert form == "ell" and b < len(nf.blocks) - 1
                    continue
                listed += 1
                srcs = draw[(b, v)]
                real = sorted(s - (G - shift) for s in srcs if s != v)
                assert cnt[j] == len(real) and self_drawn[j] == float(v in srcs), (b, v)
                assert sorted(col[start[j]: start[j] + cnt[j]].tolist()) == real, (b, v)
                assert abs(inv[j] - 1.0 / len(srcs)) < 1e-7, (b, v)
            assert listed == sum(1 for (bb, v) in draw if bb == b and (v >= G) == (shift == G))


@pytest.mark.parametrize("prefix", CASES)
@pytest.mark.parametrize("form", FORMS)
def test_sampled_logits_match_executed_reference_code(prefix, form, monkeypatch):
    z, g, m, nf = setup(prefix, form, monkeypatch)
    with torch.no_grad():
        got = m(g, dev(z["feats"]), nodeflow=nf).cpu().numpy()
    np.testing.assert_allclose(got, z[prefix + ".logits"], atol=TOL)


@pytest.mark.parametrize("prefix", CASES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("loss_kind", ["torch", "fused"])
def test_sampled_gradients_match_executed_reference_code(prefix, form, loss_kind, monkeypatch):
    """Loss and every parameter gradient (alpha included) against autograd through the reference's own code."""
    z, g, m, nf = setup(prefix, form, monkeypatch)
    m.train()
    logits = m(g, dev(z["feats"]), nodeflow=nf)
    labels = torch.from_numpy(z[prefix + ".labels"]).to(DEV)
    loss = F.cross_entropy(logits, labels, reduction="sum") if loss_kind == "torch" else sda.cross_entropy_sum(logits, labels)
    loss.backward()
    ref = float(z[prefix + ".loss"])
    assert abs(float(loss.detach()) - ref) < 1e-4 * max(1.0, abs(ref))
    names = [k for k, _ in m.named_parameters()]
    assert sorted(names) == sorted(k[len(prefix) + 6:] for k in z.files if k.startswith(prefix + ".grad."))
    for k, p in m.named_parameters():
        want = z[f"{prefix}.grad.{k}"]
        np.testing.assert_allclose(p.grad.cpu().numpy(), want, atol=TOL * max(1.0, float(np.abs(want).max())), err_msg=k)
