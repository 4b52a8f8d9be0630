"""Layer 1's genes<-cells pass served from the graph's cached feature sum ``S = A_gc X_c`` (``CellGeneGraph.feature_sum``,
``GNN.embed(..., feature_sum_cache=True)``, ``ShardedWgnn.forward`` from its second forward over the same features).

Case: 300 cells x 200 genes (a gene without cells, a cell without genes, 8 test cells outside the support mask), dense_dim 64,
hidden 16 (project-first: the two-operand GEMM) and 256 (H > D_in: aggregate-first, the elementwise mix), alpha in [0.5, 1.5],
with ``ops.TILED_MIN_WORK`` lowered (tile route, which also writes the alpha-folded gene table) and off (row-wave route).

Bounds.  Against ``oracle.wgnn_oracle.csr_forward``: the suite's 1e-4, and the observed error is asserted below 1e-5.  Against
the cache-off path of the same tree: 1e-5 absolute on these O(1) logits (the two paths differ in the order of summation of
layer 1's gene rows only; the elementwise bound (nnz_max_row + D_in + 8) * 2^-24 * sum|terms| of that layer is of the order of
1e-6 here and is not carried through the second layer and the head).  Where the cache must be bypassed the outputs are EQUAL.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from conftest import small_case
from oracle import wgnn_oracle as O
from scdeepsort_amd import ops
from scdeepsort_amd.sharded import ShardedWgnn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, OBSERVED, SAME_TREE = 1e-4, 1e-5, 1e-5
DIM, N_CLS = 64, 5
CASE = small_case(cells=300, genes=200, dim=DIM, seed=11)
G, C = CASE["G"], CASE["C"]
_ORACLE = {}


def oracle_logits(hidden, n_layers):
    """Computed once per (hidden, n_layers) and shared, never modified."""
    key = (hidden, n_layers)
    if key not in _ORACLE:
        sd = O.init_params(DIM, hidden, N_CLS, n_layers, G, seed=3)
        want = O.csr_forward(sd, O.build_csr_graph(CASE["expr"], CASE["support_mask"]), CASE["feats"], n_layers)
        want.setflags(write=False)
        _ORACLE[key] = (sd, want)
    return _ORACLE[key]


def graph():
    return sda.CellGeneGraph.from_expression(CASE["expr"], CASE["support_mask"], device=DEV)


def model(hidden, n_layers, dropout=0.0):
    sd, _ = oracle_logits(hidden, n_layers)
    m = sda.GNN(DIM, hidden, N_CLS, n_layers, G, activation=F.relu, dropout=dropout).to(DEV)
    m.load_state_dict(sd)
    return m.eval()


def features():
    return torch.from_numpy(CASE["feats"]).to(DEV)


def profiled(fn):
    """(result, [tag dict per launch record]) of one call."""
    ops.PROFILE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [dict(zip(tag[::2], tag[1::2])) for tag, _, _ in ops.PROFILE]
    finally:
        ops.PROFILE = None


def count(tags, kernel):
    return sum(t["kernel"] == kernel for t in tags)


def gene_row_passes(tags):
    return [t for t in tags if t["kernel"].startswith("agg") and t["rows"] == G]


def max_err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def test_case_has_the_edge_rows():
    g = graph()
    deg = (g.gc.rowptr[1:] - g.gc.rowptr[:-1]).cpu().numpy()
    assert (deg == 0).any() and (~CASE["support_mask"]).any()
    assert g.gc.nnz < g.cg.nnz                                  # the support mask removed the test cells' edges from the gene side
    assert np.diff(CASE["expr"].indptr).min() == 0              # a cell without genes


@pytest.mark.parametrize("dim", [64, 50, 400, 260])
@pytest.mark.parametrize("route", ["tile", "rowwave"])
def test_the_sum_itself_against_fp64(monkeypatch, route, dim):
    """``S = A_gc X_c`` on both routes - one pass, or column slabs of <= 256 through the tile kernel for wider features (400 =
    256 + 144, 260 = 256 + 4), a width that is no multiple of 4 carried zero-padded - within ``(nnz_row + 8) * 2^-24 * sum|terms|``
    per element (one rounding per accumulated edge) of the fp64 product of the same fp32 operands."""
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if route == "tile" else None)
    g = graph()
    x = torch.from_numpy((0.5 * np.random.default_rng(dim).standard_normal((C, dim))).astype(np.float32)).to(DEV)
    s, tags = profiled(lambda: g.feature_sum(x))
    passes = [t for t in tags if t["kernel"].startswith("agg")]
    assert [t["kernel"] == "agg_main" for t in passes] == [route == "rowwave"] * (-(-dim // 256) if route == "tile" else 1)
    dp = -(-dim // 4) * 4
    assert s.shape == (G, dp) and s.dtype == torch.float32 and not s[:, dim:].any()
    rp, col, val = (t.cpu().numpy() for t in (g.gc.rowptr, g.gc.col, g.gc.val))
    A = np.zeros((G, C))
    for r in range(G):
        A[r, col[rp[r]:rp[r + 1]]] = val[rp[r]:rp[r + 1]].astype(np.float64)
    x64 = x.double().cpu().numpy()
    want, abs_sum = A @ x64, np.abs(A) @ np.abs(x64)
    bound = (np.diff(rp)[:, None] + 8) * 2.0 ** -24 * abs_sum
    err = np.abs(s[:, :dim].double().cpu().numpy() - want)
    assert (err <= bound).all() and err.max() > 0 and not s.cpu().numpy()[np.diff(rp) == 0].any()
    assert g.feature_sum(x) is s and g.feature_sum(x.half()) is None and g.feature_sum(x[:-1]) is None


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tile", "rowwave"])
@pytest.mark.parametrize("hidden", [16, 256])
@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_engaged_path_against_the_oracle_and_the_cache_off_path(monkeypatch, n_layers, hidden, route):
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if route == "tile" else None)
    _, want = oracle_logits(hidden, n_layers)
    g, m, feats = graph(), model(hidden, n_layers), features()
    with torch.no_grad():
        off = m(g, feats)
        assert getattr(g, "_feature_sum", None) is None         # off by default: nothing was built
        on, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
    if n_layers == 1:                                            # no gene rows are computed at all: nothing to serve
        assert count(tags, "feature_sum_build") == 0 and torch.equal(on, off)
    else:
        assert count(tags, "feature_sum_build") == 1
        assert count(tags, "linear_mix_mfma_f32") == (1 if hidden < DIM else 0)
        assert len(gene_row_passes(tags)) == 1 + (n_layers - 2)         # the build itself + the deeper layers' own passes
        assert not torch.equal(on, off) or hidden > DIM          # another order of summation (the elementwise mix may round alike)
    e_oracle, e_off = max_err(on, want), max_err(on, off)
    print(f"L={n_layers} H={hidden} {route}: |on - oracle| = {e_oracle:.3e}, |off - oracle| = {max_err(off, want):.3e}, "
          f"|on - off| = {e_off:.3e}")
    np.testing.assert_allclose(on.cpu().numpy(), want, atol=TOL)
    assert e_oracle < OBSERVED and e_off < SAME_TREE
    with torch.no_grad():                                        # served from the cache now: no build, no gene-row pass in layer 1
        again, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
    assert torch.equal(again, on) and count(tags, "feature_sum_build") == 0
    assert len(gene_row_passes(tags)) == max(0, n_layers - 2)


@pytest.mark.parametrize("route", ["tile", "rowwave"])
@pytest.mark.parametrize("hidden", [16, 256])
def test_seed_tensor_and_seed_range(monkeypatch, hidden, route):
    monkeypatch.setattr(ops, "TILED_MIN_WORK", 1 if route == "tile" else None)
    _, want = oracle_logits(hidden, 2)
    g, m, feats = graph(), model(hidden, 2), features()
    ids = torch.from_numpy(np.random.default_rng(2).permutation(C)[:70] + G).to(DEV)
    for seeds, rows in ((ids, (ids - G).cpu().numpy()), (range(G + C - 40, G + C), np.arange(C - 40, C)),
                        (range(G + 10, G + 290), np.arange(10, 290))):
        with torch.no_grad():
            off = m(g, feats, seeds=seeds)
            on = m(g, feats, seeds=seeds, feature_sum_cache=True)
        assert on.shape == (len(rows), N_CLS)
        assert max_err(on, want[rows]) < OBSERVED and max_err(on, off) < SAME_TREE


# ---- validity ----------------------------------------------------------------------------------------------------------------
def test_in_place_writes_and_new_tensors_are_followed():
    g, m, feats = graph(), model(16, 2), features()
    call = lambda f: profiled(lambda: m(g, f, feature_sum_cache=True))
    with torch.no_grad():
        first, tags = call(feats)
        assert count(tags, "feature_sum_build") == 1
        feats.mul_(0.5)                                          # in place: same memory, new version
        halved, tags = call(feats)
        assert count(tags, "feature_sum_build") == 1
        assert max_err(halved, m(g, feats)) < SAME_TREE and max_err(halved, first) > 1e-3
        same = feats.clone()                                     # a new tensor with the same contents: a rebuild, the same output
        out, tags = call(same)
        assert count(tags, "feature_sum_build") == 1 and torch.equal(out, halved)
        other = same * -1.5 + 0.25                               # a new tensor with other contents, the old one gone
        want = m(g, other)
        del same, out
        got, tags = call(other)
        assert count(tags, "feature_sum_build") == 1 and max_err(got, want) < SAME_TREE and max_err(got, halved) > 1e-3
        split = (other[:G].clone(), other[G:].clone())           # (gene rows, cell rows) as separate tensors
        got2, tags = call(split)
        assert count(tags, "feature_sum_build") == 1 and torch.equal(got2, got)
        got3, tags = call(split)
        assert count(tags, "feature_sum_build") == 0 and torch.equal(got3, got)


def test_changed_weights_are_followed_without_a_rebuild():
    g, m, feats = graph(), model(16, 2), features()
    builds = 0
    with torch.no_grad():
        for step in range(4):
            if step == 1:
                m.layers[0].fc_neigh.weight.mul_(-0.7)
            elif step == 2:
                m.layers[0].fc_neigh.bias.add_(0.3)
            elif step == 3:
                m.alpha.copy_(torch.rand_like(m.alpha) + 0.5)
            on, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
            builds += count(tags, "feature_sum_build")
            assert count(tags, "linear_mix_mfma_f32") == 1
            off = m(g, feats)
            assert max_err(on, off) < SAME_TREE
            if step:
                assert max_err(on, prev) > 1e-3                  # the change reached the output
            prev = on
    assert builds == 1
    g.invalidate_feature_sums()
    with torch.no_grad():
        again, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
    assert count(tags, "feature_sum_build") == 1 and torch.equal(again, prev)


def test_grad_dropout_and_capture_bypass_the_cache():
    g, feats = graph(), features()
    m = model(16, 2, dropout=0.1)
    with torch.no_grad():
        m(g, feats, feature_sum_cache=True)                      # a valid entry exists: the bypasses below are decisions, not misses
    entry = g._feature_sum
    assert entry is not None
    # something is differentiated
    on, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
    assert on.requires_grad and count(tags, "linear_mix_mfma_f32") == 0 and len(gene_row_passes(tags)) == 1
    assert torch.equal(on, m(g, feats))
    # active dropout: the same generator state gives the same masks
    m.train()
    with torch.no_grad():
        torch.manual_seed(5)
        on, tags = profiled(lambda: m(g, feats, feature_sum_cache=True))
        torch.manual_seed(5)
        off = m(g, feats)
    assert count(tags, "linear_mix_mfma_f32") == 0 and torch.equal(on, off)
    m.eval()
    with torch.no_grad():
        eager = m(g, feats)
    assert not torch.equal(off, eager)                           # (the masks did bite)
    # a stream capture: the replay on new feature contents must not meet a sum of the old ones
    from scdeepsort_amd.graphed import GraphedForward
    m.feature_sum_cache = True                                   # the default GraphedForward's plain model(...) calls run under
    static = feats.clone()
    with torch.no_grad():
        m(g, static)
    entry = g._feature_sum
    assert entry is not None and entry[1].data_ptr() == static[G:].data_ptr()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        m(g, static)
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg), torch.no_grad():
        captured = m(g, static)
    assert g._feature_sum is entry                               # neither used nor rebuilt under capture
    new = feats * 0.25 - 0.5
    static.copy_(new)
    cg.replay()
    torch.cuda.synchronize()
    m.feature_sum_cache = False
    with torch.no_grad():
        want = m(g, new)
    assert torch.equal(captured, want)
    gf = GraphedForward(m, g, feats)                             # the package's own capture helper, flag on
    m.feature_sum_cache = True
    gf2 = GraphedForward(m, g, feats)
    assert torch.equal(gf2(new), gf(new))


def test_engine_switches_over_on_its_second_forward():
    g, m, feats = graph(), model(16, 2), features()
    eng = ShardedWgnn(m, g, 1)
    fg, fc = feats[:G], feats[G:]
    with torch.no_grad():
        plain = m(g, feats)
        first, tags1 = profiled(lambda: eng.forward(fg, fc))
        second, tags2 = profiled(lambda: eng.forward(fg, fc))
        third, tags3 = profiled(lambda: eng.forward(fg, fc))
    # the first forward is the plain model (a single forward never pays for the build)
    assert torch.equal(first, plain) and count(tags1, "feature_sum_build") == 0 and len(gene_row_passes(tags1)) == 1
    assert count(tags1, "linear_mix_mfma_f32") == 0
    assert count(tags2, "feature_sum_build") == 1 and count(tags2, "linear_mix_mfma_f32") == 1
    # after the switch-over: no aggregation launch over the gene rows, one two-operand GEMM tagged with its shape
    assert gene_row_passes(tags3) == [] and count(tags3, "feature_sum_build") == 0
    mix = [t for t in tags3 if t["kernel"] == "linear_mix_mfma_f32"]
    assert len(mix) == 1 and (mix[0]["rows"], mix[0]["N"], mix[0]["K"]) == (G, 16, DIM)
    assert sum(t["kernel"].startswith("agg") for t in tags3) == sum(t["kernel"].startswith("agg") for t in tags1) - 1
    assert torch.equal(third, second) and max_err(third, first) < SAME_TREE
    with torch.no_grad():
        # other features: back to the plain path for one forward, then the switch again
        f2 = feats * 2.0
        a, tags_a = profiled(lambda: eng.forward(f2[:G], f2[G:]))
        assert count(tags_a, "linear_mix_mfma_f32") == 0 and torch.equal(a, m(g, f2))
        # the same memory written in place counts as other features too
        f2.add_(1.0)
        b, tags_b = profiled(lambda: eng.forward(f2[:G], f2[G:]))
        assert count(tags_b, "linear_mix_mfma_f32") == 0 and torch.equal(b, m(g, f2))
        c, tags_c = profiled(lambda: eng.forward(f2[:G], f2[G:]))
        assert count(tags_c, "linear_mix_mfma_f32") == 1 and max_err(c, b) < SAME_TREE
    # with grad enabled the engine never switches
    x, tags = profiled(lambda: eng.forward(f2[:G], f2[G:]))
    y, tags_y = profiled(lambda: eng.forward(f2[:G], f2[G:]))
    assert count(tags + tags_y, "linear_mix_mfma_f32") == 0 and torch.equal(x, y)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_feature_sum_cache as T
from scdeepsort_amd import ops
from scdeepsort_amd.sharded import ShardedWgnn
assert ops.FEATURE_SUM_CACHE is False
g, m, feats = T.graph(), T.model(16, 2), T.features()
eng = ShardedWgnn(m, g, 1)
with torch.no_grad():
    plain = m(g, feats)
    outs = [T.profiled(lambda: eng.forward(feats[:T.G], feats[T.G:])) for _ in range(3)]
    outs.append(T.profiled(lambda: m(g, feats, feature_sum_cache=True)))
for out, tags in outs:
    assert torch.equal(out, plain)
    assert T.count(tags, "feature_sum_build") == 0 and T.count(tags, "linear_mix_mfma_f32") == 0 and len(T.gene_row_passes(tags)) == 1
assert getattr(g, "_feature_sum", None) is None
print("parent path taken")
"""


def test_environment_switch_takes_the_parent_path_in_a_fresh_process():
    root = str(Path(__file__).resolve().parent.parent)
    env = dict(os.environ, WGNN_FEATURE_SUM_CACHE="0")
    r = subprocess.run([sys.executable, "-c", CHILD, root], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "parent path taken" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
