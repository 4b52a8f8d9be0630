"""Golden vectors produced by EXECUTING THE REFERENCE'S OWN CODE for the hot path - run in the BUILD container only:

    python tests/golden/make_refcode_golden.py        ->  tests/golden/refcode_{train,predict,1layer,wide,sampled}.npz

What runs verbatim from /root/reference (imported at generation time, never copied, never shipped):
  * models/gnn.py        : GNN.__init__, GNN.message_func (alpha-index cascade, multiply order), GNN.forward,
                           NodeUpdate.forward                                   (gnn.py:10-68)
  * utils/preprocess_internal.py : normalize_weight                             (preprocess_internal.py:15-23)

What does NOT run: DGL 0.4.3.post2 itself (absent from the image, not installable).  The reference code above only
touches DGL through `graph.in_degrees / in_edges / edata / number_of_nodes`, `nf.layers[i].data`, `nf.block_compute`
and `fn.mean`; those are provided here by a ~70-line STAND-IN that implements their documented semantics:
  - fn.mean('m','neigh'): neigh[v] = sum of the messages on v's in-edges / number of those edges;
  - NodeFlow with expand_factor >= every in-degree: block i holds ALL parent in-edges of layer i+1's nodes,
    layer i = the sources of those edges (train.py:37-38,71-78);
  - `graph.edata['weight'][ids] = x` writes through (the reference relies on it);
  - refcode_sampled only: NodeFlows with expand_factor k below the in-degrees (train.py:37-40), drawn by `in_edge_draw`
    (min(k, in-degree) in-edges per node, the self-loop one of them, uniformly without replacement).  DGL's own random
    stream cannot be reproduced; the fixture records the draw, and pins what the model computes GIVEN that draw.
So these fixtures pin the repo's restatement of the REFERENCE'S OWN arithmetic (alpha indexing, (h*alpha)*w order,
normalise-then-self-loop, Linear+ReLU, head) against that code as executed; the DGL-internal part of the path stays
restated-from-documentation, which is why the oracle header says "pinned against the reference's own Python code,
UNPINNED against DGL".  Also stored: the loss and autograd gradients of one seed batch through the same code
(CrossEntropyLoss(reduction='sum'), train.py:34-36,80-84).
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent


# ------------------------------------------------------------------------------------------------ DGL stand-in
def install_dgl_standin():
    dgl = types.ModuleType("dgl")
    fn = types.ModuleType("dgl.function")
    fn.mean = lambda msg, out: ("mean", msg, out)
    dgl.function = fn
    for name in ("DGLGraph", "NodeFlow", "EdgeBatch"):
        setattr(dgl, name, type(name, (), {}))
    sys.modules["dgl"], sys.modules["dgl.function"] = dgl, fn


class GraphStandIn:
    """The slice of DGLGraph that normalize_weight touches; edges in insertion order."""

    def __init__(self, n_nodes, src, dst, weight):
        self.n, self.src, self.dst = n_nodes, torch.as_tensor(src), torch.as_tensor(dst)
        self.edata = {"weight": torch.as_tensor(weight, dtype=torch.float32).clone().unsqueeze(-1)}

    def number_of_nodes(self):
        return self.n

    def in_degrees(self):
        return torch.bincount(self.dst, minlength=self.n)

    def in_edges(self, v, form="all"):
        eid = torch.nonzero(self.dst == v).squeeze(-1)
        return self.src[eid], self.dst[eid], eid


class _Frame:
    def __init__(self, data):
        self.data = data


class _Batch:
    def __init__(self, src, dst, data):
        self.src, self.dst, self.data = src, dst, data


class NodeFlowStandIn:
    """NodeFlow of `seeds` over a parent graph given as (src, dst, weight, node_id, features).

    Without `draw`: the full neighbourhood (expand_factor >= every in-degree).  With `draw(block, v, edge_ids) -> kept
    edge ids`: block `block` (block 0 feeds layer 1) holds, for every node v of the layer above in layer order, the
    in-edges that `draw` keeps out of ALL of v's parent in-edges `edge_ids` (its self-loop included); every kept edge is
    recorded in `self.drawn` as (block, dst, src) in parent ids."""

    def __init__(self, src, dst, weight, node_id, features, seeds, n_layers, draw=None):
        layers, blocks = [np.asarray(seeds, dtype=np.int64)], []
        self.drawn = []
        for t in range(n_layers):
            cur = layers[0]
            pos = {int(v): j for j, v in enumerate(cur)}
            if draw is None:
                sel = np.nonzero(np.isin(dst, cur))[0]
            else:
                b = n_layers - 1 - t
                sel = np.concatenate([np.asarray(draw(b, int(v), np.nonzero(dst == v)[0]), dtype=np.int64) for v in cur])
                self.drawn += [(b, int(dst[e]), int(src[e])) for e in sel]
            prev, src_local = np.unique(src[sel], return_inverse=True)
            blocks.insert(0, (src_local, np.array([pos[int(d)] for d in dst[sel]], dtype=np.int64), weight[sel]))
            layers.insert(0, prev)
        self.layer_nids = layers
        self.layers = [_Frame({"id": torch.from_numpy(node_id[l]).unsqueeze(-1)}) for l in layers]
        self.layers[0].data["features"] = torch.from_numpy(features[layers[0]])
        self._blocks = blocks

    def block_compute(self, i, message_func, reduce_func, apply_func):
        kind, msg, out = reduce_func
        assert kind == "mean"
        e_src, e_dst, w = self._blocks[i]
        s, d = torch.from_numpy(e_src), torch.from_numpy(e_dst)
        batch = _Batch({k: v[s] for k, v in self.layers[i].data.items()}, {k: v[d] for k, v in self.layers[i + 1].data.items()},
                       {"weight": torch.from_numpy(w)})
        m = message_func(batch)[msg]
        n_dst = len(self.layer_nids[i + 1])
        # fn.mean, written as its definition: one destination at a time, its mailbox = the messages on its in-edges,
        # summed in float64 in edge order and divided by their number.  Deliberately shares no code shape with
        # oracle/wgnn_oracle.py::block_compute (index_add_ + degree vector) so that the two are independent.
        mailbox = [[] for _ in range(n_dst)]
        for e, v in enumerate(e_dst.tolist()):
            mailbox[v].append(e)
        rows = []
        for v in range(n_dst):
            acc = torch.zeros(m.shape[1], dtype=torch.float64)
            for e in mailbox[v]:
                acc = acc + m[e].double()
            rows.append((acc / float(len(mailbox[v]))).to(m.dtype))
        self.layers[i + 1].data[out] = torch.stack(rows)
        self.layers[i + 1].data.update(apply_func(self.layers[i + 1]))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ cases
def build_edges(expr, support_mask):
    """Node order and edge set of the reference graph (preprocess_internal.py:107-110,160-173; predict graphs:
    preprocess.py:126-134,184-187): genes 0..G-1 (id = index), cells after them (id = -1); every stored entry gives a
    gene->cell edge, support cells also the cell->gene edge; raw weight = expression value on both."""
    C, G = expr.shape
    r, c = np.nonzero(expr)
    w = expr[r, c].astype(np.float32)
    sup = support_mask[r]
    src = np.concatenate([r[sup] + G, c]); dst = np.concatenate([c[sup], r + G]); wt = np.concatenate([w[sup], w])
    node_id = np.concatenate([np.arange(G), -np.ones(C)]).astype(np.int32)
    return src.astype(np.int64), dst.astype(np.int64), wt, node_id


def parent_graph(pre_mod, expr, support_mask):
    """Raw edges, their weights after the reference's normalize_weight, and the graph with its unit self-loops."""
    N = sum(expr.shape)
    src, dst, raw, node_id = build_edges(expr, support_mask)
    graph = GraphStandIn(N, src, dst, raw)
    pre_mod.normalize_weight(graph)                                           # REFERENCE CODE
    w_norm = graph.edata["weight"].squeeze(-1).numpy().copy()
    # self-loops AFTER normalisation, weight 1 (preprocess_internal.py:211-214)
    loops = np.arange(N)
    src2, dst2 = np.concatenate([src, loops]), np.concatenate([dst, loops])
    w2 = np.concatenate([w_norm, np.ones(N, np.float32)]).astype(np.float32)[:, None]
    return src, dst, raw, node_id, w_norm, src2, dst2, w2


def make_model(gnn_mod, dim, hidden, n_classes, n_layers, G, seed):
    torch.manual_seed(seed)
    model = gnn_mod.GNN(dim, hidden, n_classes, n_layers, G, activation=torch.nn.functional.relu)   # REFERENCE CODE
    with torch.no_grad():
        model.alpha.uniform_(0.5, 1.5)
        for p in model.parameters():
            if p.dim() == 1:
                p.uniform_(-0.3, 0.3)
    return model.eval()


def make_case(name, gnn_mod, pre_mod, expr, support_mask, dim, hidden, n_classes, n_layers, seed, batch_grads=True):
    C, G = expr.shape
    N = G + C
    src, dst, raw, node_id, w_norm, src2, dst2, w2 = parent_graph(pre_mod, expr, support_mask)
    model = make_model(gnn_mod, dim, hidden, n_classes, n_layers, G, seed)
    rng = np.random.default_rng(seed)
    feats = (0.5 * rng.standard_normal((N, dim))).astype(np.float32)
    seeds = np.arange(G, N)
    nf = NodeFlowStandIn(src2, dst2, w2, node_id, feats, seeds, n_layers)
    with torch.no_grad():
        logits = model(nf).numpy()                                            # REFERENCE CODE (GNN.forward)
    # one training step's loss and gradients on a seed batch (train.py:34-36,80-84): CrossEntropyLoss(reduction='sum')
    batch = seeds[rng.permutation(len(seeds))[: max(3, len(seeds) // 2)]]
    labels = rng.integers(0, n_classes, len(batch))
    nfb = NodeFlowStandIn(src2, dst2, w2, node_id, feats, batch, n_layers)
    loss = torch.nn.CrossEntropyLoss(reduction='sum')(model(nfb), torch.from_numpy(labels))      # REFERENCE CODE + autograd
    model.zero_grad()
    loss.backward()
    out = dict(expr=expr.astype(np.float32), support_mask=support_mask, dim=dim, hidden=hidden, n_classes=n_classes,
               n_layers=n_layers, feats=feats, seeds=seeds, logits=logits,
               edge_src=src, edge_dst=dst, edge_w_raw=raw, edge_w_norm=w_norm,
               batch=batch, labels=labels, loss=float(loss))
    if batch_grads:                       # (the wide case keeps the full-batch set only: the .npz stays under 1 MB)
        for k, p in model.named_parameters():
            out["grad." + k] = p.grad.numpy().copy()
    # round 4: the FULL-batch step (every cell a seed, in node order) - the shape of BASELINE cfg4's training step, which the
    # product runs through its fused backward glue (wgnn_agg_bwd_prepare) and loss kernel; own label stream, drawn last so
    # that everything above is unchanged
    full_labels = np.random.default_rng(seed + 1).integers(0, n_classes, len(seeds))
    nff = NodeFlowStandIn(src2, dst2, w2, node_id, feats, seeds, n_layers)
    full_loss = torch.nn.CrossEntropyLoss(reduction='sum')(model(nff), torch.from_numpy(full_labels))   # REFERENCE CODE + autograd
    model.zero_grad()
    full_loss.backward()
    out.update(full_labels=full_labels, full_loss=float(full_loss))
    for k, p in model.named_parameters():
        out["fullgrad." + k] = p.grad.numpy().copy()
    for k, v in model.state_dict().items():
        out["param." + k] = v.numpy()
    np.savez_compressed(HERE / f"{name}.npz", **out)
    print(f"{name}: {C} cells x {G} genes, {len(src)} edges, logits {logits.shape}, |logits|max {np.abs(logits).max():.3f}")


# ------------------------------------------------------------------------------------------------ sampled NodeFlows
def in_edge_draw(k, rng):
    """DGL's NeighborSampler(expand_factor=k, neighbor_type='in') (train.py:37-40,71-78), restated from its documentation:
    every node of layer i+1 keeps min(k, in-degree) of its in-edges, uniformly without replacement.  The in-degree counts
    the unit self-loop (preprocess_internal.py:213-214), which is one of the candidates.  One permutation per node."""
    def draw(block, v, edge_ids):
        return edge_ids[np.sort(rng.permutation(len(edge_ids))[:k])]
    return draw


def check_draw(drawn, n_layers, k, G, indeg):
    """The draw must contain every situation the sampled path computes differently from the full graph: a regeneration
    that loses one fails here instead of quietly weakening the fixture."""
    srcs = {}
    for b, d, s in drawn:
        srcs.setdefault((b, d), []).append(s)
    self_drawn = {bv: bv[1] in ss for bv, ss in srcs.items()}
    for (b, v), ss in srcs.items():
        assert len(ss) == min(k, indeg[v]) and len(set(ss)) == len(ss)
    assert any(indeg[v] > 1 and not sd for (b, v), sd in self_drawn.items()), "no node with neighbours and an undrawn self-loop"
    assert any(self_drawn.values()), "no drawn self-loop"
    assert any(indeg[v] > k for (b, v) in srcs), "no row cut by k"
    if n_layers == 2:
        assert any(v < G and sd for (b, v), sd in self_drawn.items()), "no gene with a drawn self-loop"
        layer0_cells = {s for b, d, s in drawn if b == 0 and s >= G}
        own_only = [c for c in layer0_cells if all(d == c for b, d, s in drawn if b == 0 and s == c)]
        assert own_only, "no cell in layer 0 only through its own self-loop"


def make_sampled_case(name, gnn_mod, pre_mod, expr, support_mask, dim, hidden, n_classes, seed, cases):
    """One graph, several NodeFlows drawn with expand_factor k (train.py:37-40).  Per case (prefix, n_layers, k): the seeds,
    the recorded draw (block 0 feeds layer 1; parent ids, genes 0..G-1 then cells G + c; a self-loop is src == dst), the
    eval-mode logits of GNN.forward, and the loss (CrossEntropyLoss(reduction='sum')) and autograd gradients of that
    same forward."""
    C, G = expr.shape
    N = G + C
    src, dst, raw, node_id, w_norm, src2, dst2, w2 = parent_graph(pre_mod, expr, support_mask)
    indeg = np.bincount(dst2, minlength=N)
    rng = np.random.default_rng(seed)
    feats = (0.5 * rng.standard_normal((N, dim))).astype(np.float32)
    empty = np.nonzero(~expr.any(axis=1))[0]
    assert len(empty) and support_mask[empty].all() and (~expr.any(axis=0)).any() and (~support_mask).any()
    support = np.nonzero(support_mask)[0]
    out = dict(expr=expr.astype(np.float32), support_mask=support_mask, dim=dim, hidden=hidden, n_classes=n_classes, feats=feats,
               edge_src=src, edge_dst=dst, edge_w_norm=w_norm, cases=np.array([c[0] for c in cases]))
    for j, (prefix, n_layers, k, stream) in enumerate(cases):
        others = rng.permutation(np.setdiff1d(support, empty))[:11]
        seeds = G + rng.permutation(np.concatenate([others, empty]))           # shuffled support cells, the empty cell among them
        labels = rng.integers(0, n_classes, len(seeds))
        model = make_model(gnn_mod, dim, hidden, n_classes, n_layers, G, seed + j)
        nf = NodeFlowStandIn(src2, dst2, w2, node_id, feats, seeds, n_layers, draw=in_edge_draw(k, np.random.default_rng([seed, stream])))
        logits = model(nf)                                                    # REFERENCE CODE (GNN.forward, eval mode)
        loss = torch.nn.CrossEntropyLoss(reduction='sum')(logits, torch.from_numpy(labels))         # REFERENCE CODE + autograd
        model.zero_grad()
        loss.backward()
        check_draw(nf.drawn, n_layers, k, G, indeg)
        blk, d, s = np.array(nf.drawn, dtype=np.int64).T
        out.update({f"{prefix}.n_layers": n_layers, f"{prefix}.k": k, f"{prefix}.seeds": seeds, f"{prefix}.labels": labels,
                    f"{prefix}.draw_block": blk, f"{prefix}.draw_dst": d, f"{prefix}.draw_src": s,
                    f"{prefix}.logits": logits.detach().numpy(), f"{prefix}.loss": float(loss)})
        for key, p in model.named_parameters():
            out[f"{prefix}.grad.{key}"] = p.grad.numpy().copy()
        for key, v in model.state_dict().items():
            out[f"{prefix}.param.{key}"] = v.numpy()
        print(f"{name}/{prefix}: {n_layers} layer(s), k = {k}, {len(blk)} drawn edges, |logits|max {float(logits.abs().max()):.3f}")
    np.savez_compressed(HERE / f"{name}.npz", **out)


def main():
    # one thread, deterministic kernels: the wide case's scatter-adds (the stand-in's fn.mean and its backward) are summed in
    # thread-dependent order otherwise, and a re-run would differ from the committed file in the last bits
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    install_dgl_standin()
    gnn_mod = load(REF / "models" / "gnn.py", "ref_gnn")
    pre_mod = load(REF / "utils" / "preprocess_internal.py", "ref_preprocess_internal")
    rng = np.random.default_rng(2024)
    for name, C, G, test_cells, L, dims in (("refcode_train", 14, 9, 0, 2, (12, 8, 4)), ("refcode_predict", 17, 11, 5, 2, (12, 8, 4)),
                                           ("refcode_1layer", 10, 7, 3, 1, (12, 8, 4)),
                                           # round 6: wide enough for the LDS-streamed tile kernels at their headline width
                                           # (aggregated rows of 256 floats = agg_tiled_flat4's D = 256 instantiation; the tiny
                                           # cases above only reach the row-wave kernel or padded tiles).  Drawn last: the three
                                           # fixtures above stay bit-identical.
                                           ("refcode_wide", 300, 200, 60, 2, (64, 256, 8))):
        expr, support = draw_expression(rng, C, G, test_cells)
        make_case(name, gnn_mod, pre_mod, expr, support, dim=dims[0], hidden=dims[1], n_classes=dims[2], n_layers=L, seed=C * 100 + G,
                  batch_grads=name != "refcode_wide")
    # neighbour-sampled NodeFlows (num_neighbors > 0).  Drawn after every case above, which therefore stays bit-identical.
    expr, support = draw_expression(rng, 40, 25, 8)
    make_sampled_case("refcode_sampled", gnn_mod, pre_mod, expr, support, dim=10, hidden=6, n_classes=4, seed=4025,
                      cases=CASES)


# (prefix, n_layers, k, draw stream): each stream was picked as the first whose draw passes check_draw
CASES = (("L1k3", 1, 3, 0), ("L2k1", 2, 1, 4), ("L2k3", 2, 3, 0), ("L2k7", 2, 7, 0))


def draw_expression(rng, C, G, test_cells):
    mask = rng.random((C, G)) < 0.35
    mask[:, 0] = True                 # a hub gene
    mask[2, :] = False                # a cell expressing nothing
    mask[:, G - 1] = False            # a gene no cell expresses
    expr = np.where(mask, np.clip(rng.normal(3.0, 0.9, (C, G)), 0.5, 7.0), 0.0).astype(np.float32)
    support = np.ones(C, bool)
    if test_cells:
        support[-test_cells:] = False
    return expr, support


if __name__ == "__main__":
    main()
