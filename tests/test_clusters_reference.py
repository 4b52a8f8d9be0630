"""CPU side of the per-cluster calls: the C ABI of ``wgnn_group_class_reduce`` without a GPU (every check that returns before
a launch), the fp64 reference of tests/clusters_reference.py against vectors computed by hand, and the host logic of
``ClusterCalls`` (consensus rules, frame, cell_labels, ``into`` checks, cluster-name factorisation) on CPU tensors."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api

import clusters_reference as R

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for s in ("wgnn_group_class_reduce", "wgnn_group_class_reduce_workspace"):
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in wgnn.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert int(re.search(r"#define\s+WGNN_CLUSTERS_ACCUMULATE\s+(\d+)", text).group(1)) == _lib.CLUSTERS_ACCUMULATE
    assert lib.wgnn_version() == 206
    assert sda.group_class_reduce is sda.ops.group_class_reduce and sda.ClusterCalls is api.ClusterCalls
    assert "group_class_reduce" in sda.__all__ and "ClusterCalls" in sda.__all__


def test_argument_checks_return_before_any_launch():
    """Host memory stands in for the operands: every call below must return from its argument checks."""
    lib = _lib.lib()
    K, Cn, B = 3, 5, 10
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    nb = C.c_int64()
    assert lib.wgnn_group_class_reduce_workspace(B, K, Cn, C.addressof(nb)) == 0 and nb.value > 0
    assert lib.wgnn_group_class_reduce_workspace(B, K, Cn, None) == -1
    assert lib.wgnn_group_class_reduce_workspace(-1, K, Cn, C.addressof(nb)) == -1
    assert lib.wgnn_group_class_reduce_workspace(2 ** 31, K, Cn, C.addressof(nb)) == -1
    assert lib.wgnn_group_class_reduce_workspace(B, 0, Cn, C.addressof(nb)) == -1
    assert lib.wgnn_group_class_reduce_workspace(B, K, 0, C.addressof(nb)) == -1
    assert b"n_classes" in lib.wgnn_last_error_string(-1)
    big = 2 ** 31 - 1                                            # sizes whose workspace is beyond int64: refused, not wrapped
    assert lib.wgnn_group_class_reduce_workspace(big, big, big, C.addressof(nb)) == -3
    assert b"2^63" in lib.wgnn_last_error_string(-3)
    assert lib.wgnn_group_class_reduce_workspace(big, big, 1000, C.addressof(nb)) == 0 and nb.value > 2 ** 40
    # workspace bytes grow with every size
    sizes = []
    for args in ((B, K, Cn), (B + 4096, K, Cn), (B, K + 1, Cn), (B, K, Cn + 1)):
        assert lib.wgnn_group_class_reduce_workspace(*args, C.addressof(nb)) == 0
        sizes.append(nb.value)
    assert all(s > sizes[0] for s in sizes[1:])

    def run(logits=base, ld=Cn, label=base + 512, order=base + 1024, seg=base + 2048, n_rows=B, k=K, c=Cn, prob=base + 4096,
            conf=base + 8192, votes=base + 12288, tally=base + 16384, ws=base + 20480, ws_bytes=sizes[0], flags=0):
        return lib.wgnn_group_class_reduce(logits, ld, label, order, seg, n_rows, k, c, prob, conf, votes, tally, ws, ws_bytes,
                                           flags, None)

    bad_arg = [dict(prob=None), dict(conf=None), dict(votes=None), dict(tally=None), dict(seg=None), dict(k=0), dict(k=-2),
               dict(c=0), dict(ld=Cn - 1), dict(n_rows=-1), dict(n_rows=2 ** 31), dict(flags=1), dict(flags=256 | 512)]
    for kw in bad_arg:
        assert run(**kw) == -1, kw
        assert b"wgnn_group_class_reduce" in lib.wgnn_last_error_string(-1), kw
    assert run(flags=2) == -1 and b"WGNN_CLUSTERS_ACCUMULATE" in lib.wgnn_last_error_string(-1)
    assert run(ld=Cn - 1) == -1 and b"ld_logits" in lib.wgnn_last_error_string(-1)
    for kw in (dict(prob=base + 4100), dict(conf=base + 8196), dict(seg=base + 2052), dict(logits=base + 2), dict(label=base + 513),
               dict(order=base + 1025), dict(votes=base + 12290), dict(tally=base + 16387), dict(ws=base + 20484)):
        assert run(**kw) == -2, kw                               # WGNN_ERR_ALIGNMENT
        assert b"aligned" in lib.wgnn_last_error_string(-2), kw
    for kw in (dict(ws=None), dict(ws_bytes=sizes[0] - 1), dict(ws_bytes=0), dict(ws_bytes=-8)):
        assert run(**kw) == -4, kw                               # WGNN_ERR_WORKSPACE
        assert b"workspace" in lib.wgnn_last_error_string(-4), kw
    # the detail is handed out once, then the generic text
    assert run(k=0) == -1
    assert b"n_groups" in lib.wgnn_last_error_string(-1) and b"n_groups" not in lib.wgnn_last_error_string(-1)


def test_op_refuses_host_tensors_and_bad_shapes_without_a_gpu():
    z = torch.zeros(4, 3)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        sda.group_class_reduce(z, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 2)


# ------------------------------------------------------------------------------------------------
# the reference against vectors computed by hand
# ------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_vectors():
    ln3 = math.log(3.0)
    # two cells, two classes, logits (0, ln 3): p = (1/4, 3/4); the mirrored cell (ln 3, 0): p = (3/4, 1/4)
    logits = np.array([[0.0, ln3], [ln3, 0.0]], np.float32)
    prob, conf, votes, tally = R.reduce(logits, [1, -1], [0, 0], 2)
    assert prob.dtype == np.float64 and conf.dtype == np.float64 and votes.dtype == np.int32 and tally.dtype == np.int32
    np.testing.assert_allclose(prob, [[1.0, 1.0], [0.0, 0.0]], rtol=0, atol=1e-7)        # float32(ln 3) is ln 3 within 2^-24
    np.testing.assert_allclose(conf, [1.5, 0.0], rtol=0, atol=1e-7)
    assert votes.tolist() == [[0, 1], [0, 0]] and tally.tolist() == [[2, 1, 0], [0, 0, 0]]
    p, c = R.cell(logits[0])
    assert abs(p[0] - 0.25) < 1e-7 and abs(p[1] - 0.75) < 1e-7 and c == p[1] and abs(c - 1.0 / (1.0 + 1.0 / 3.0)) < 1e-7
    # exact ones: equal logits, a shift changes nothing, a -inf beside finite logits is a 0
    assert R.cell([5.0, 5.0, 5.0, 5.0]) == ([0.25] * 4, 0.25)
    assert R.cell([-1000.0, 0.0, 0.0, -np.inf]) == ([0.0, 0.5, 0.5, 0.0], 0.5)
    assert R.cell([7.0]) == ([1.0], 1.0)
    # groups: -1 and out-of-range groups and labels take no part
    logits = np.zeros((6, 2), np.float32)
    prob, conf, votes, tally = R.reduce(logits, label=[1, 1, 1, 0, 0, 2], group=[0, 1, 1, -1, 2, 0], n_groups=2)
    assert prob.tolist() == [[0.5, 0.5], [1.0, 1.0]] and conf.tolist() == [0.5, 1.0]
    assert votes.tolist() == [[0, 1], [0, 2]] and tally.tolist() == [[1, 0, 0], [2, 0, 0]]   # cells 3 (group -1), 4 (group 2), 5 (label 2) are out
    assert (tally[:, 0] == votes.sum(1) + tally[:, 1]).all()


def test_reference_bad_cell_rule():
    inf, nan = np.inf, np.nan
    logits = np.array([[0.0, nan, 0.0], [inf, 0.0, 0.0], [-inf, -inf, -inf], [-inf, 0.0, -inf], [0.0, 0.0, 0.0]], np.float32)
    assert R.cell(logits[0]) is None and R.cell(logits[1]) is None and R.cell(logits[2]) is None
    assert R.cell(logits[3]) == ([0.0, 1.0, 0.0], 1.0)
    prob, conf, votes, tally = R.reduce(logits, [0, 1, 2, 1, -1], [0, 0, 0, 0, 0], 1)
    assert tally.tolist() == [[2, 1, 3]] and votes.tolist() == [[0, 1, 0]]
    third = 1.0 / 3.0
    assert prob.tolist() == [[third, 1.0 + third, third]] and conf.tolist() == [1.0 + third]


def test_case_builders_hold_their_premises():
    for B, Cn, K in R.CASES:
        c = R.lattice_case(B, Cn, K)
        assert c.logits.shape == (B, Cn) and c.logits.dtype == np.float32 and c.group.dtype == np.int32 == c.label.dtype
        zeros = (c.logits == 0.0).sum(1)
        assert ((zeros & (zeros - 1)) == 0).all() and (zeros >= 1).all()                   # a power of two per row
        assert np.isin(c.logits, [0.0, -1000.0, -np.inf]).all()
        if B >= 63 and Cn >= 5:
            assert len(set(zeros.tolist())) > 1                                            # rows differ in m
    assert math.exp(-1000.0) == 0.0
    assert {b for b, _, _ in R.CASES} == {0, 1, 63, 64, 65, 1500}
    assert {c for _, c, _ in R.CASES} == {1, 2, 5, 16, 17, 64, 65, 80} and {k for _, _, k in R.CASES} == {1, 3, 200}
    c = R.special("three_chunks")
    assert (c.group == 1).sum() > 3 * 256
    c = R.random_case(65, 17, 3)
    prob, conf, votes, tally = R.reduce(c.logits, c.label, c.group, 3)
    np.testing.assert_allclose(prob.sum(1), tally[:, 0], rtol=1e-13)                       # a cell's p adds up to 1
    assert (tally[:, 0] == votes.sum(1) + tally[:, 1]).all() and (conf <= tally[:, 0]).all()


# ------------------------------------------------------------------------------------------------
# ClusterCalls on CPU tensors
# ------------------------------------------------------------------------------------------------
def _calls(votes, unsure=None, prob=None, conf=None, bad=None, names=None, unsure_rate=2.0, labels=None):
    votes = np.asarray(votes, np.int32)
    K, Cn = votes.shape
    unsure = np.zeros(K, np.int32) if unsure is None else np.asarray(unsure, np.int32)
    n = votes.sum(1) + unsure
    tally = np.stack([n, unsure, np.zeros(K, np.int32) if bad is None else np.asarray(bad, np.int32)], 1).astype(np.int32)
    prob = votes.astype(np.float64) if prob is None else np.asarray(prob, np.float64)
    conf = n.astype(np.float64) if conf is None else np.asarray(conf, np.float64)
    return sda.ClusterCalls(cluster_names=names or [f"c{i}" for i in range(K)], id2label=labels or [f"type{j}" for j in range(Cn)],
                            prob_sum=torch.from_numpy(prob), conf_sum=torch.from_numpy(conf), votes=torch.from_numpy(votes),
                            tally=torch.from_numpy(tally), unsure_rate=unsure_rate)


def test_consensus_vote_rule():
    #              tie -> lowest id   unsure plurality   unsure == winner: stays   clear   empty
    calls = _calls([[3, 5, 5, 0], [2, 3, 0, 0], [0, 4, 1, 0], [0, 1, 0, 9], [0, 0, 0, 0]], unsure=[0, 4, 4, 0, 0])
    ids, conf = calls.consensus()
    assert ids.dtype == np.int64 and conf.dtype == np.float64
    assert ids.tolist() == [1, -1, 1, 3, -2]
    np.testing.assert_array_equal(conf[:4], [5 / 13, 3 / 9, 4 / 9, 9 / 10])
    assert math.isnan(conf[4])
    assert calls.n_cells.tolist() == [13, 9, 9, 10, 0] and calls.n_unsure.tolist() == [0, 4, 4, 0, 0] and calls.n_bad.tolist() == [0] * 5
    # min_fraction: the winner's share of n_cells must reach it
    assert calls.consensus(min_fraction=0.4)[0].tolist() == [-1, -1, 1, 3, -2]
    assert calls.consensus(min_fraction=5 / 13)[0].tolist() == [1, -1, 1, 3, -2]          # not below: stays
    assert calls.consensus("vote", 0.95)[0].tolist() == [-1, -1, -1, -1, -2]
    want = R.consensus(calls.prob_sum.numpy(), calls.votes.numpy(), calls.tally.numpy(), 2.0, "vote", 0.4)
    np.testing.assert_array_equal(calls.consensus("vote", 0.4)[0], want[0])
    np.testing.assert_array_equal(calls.consensus("vote", 0.4)[1], want[1])
    np.testing.assert_array_equal(calls.fraction().numpy()[0], np.array([3, 5, 5, 0]) / 13)
    with pytest.raises(ValueError, match="rule"):
        calls.consensus("majority")
    with pytest.raises(ValueError, match="rule"):
        calls.frame("majority")


def test_consensus_mean_prob_rule_and_its_threshold():
    Cn, rate = 3, 2.0
    thr = float(np.float32(rate / Cn))                           # 0.6666667: above 2/3 in fp64
    assert thr > rate / Cn
    n = 8
    below = np.nextafter(thr, 0.0)
    # cluster 0: mean exactly at the threshold -> kept; 1: one ulp below -> unsure; 2: 2/3 in fp64 (< float32(2/3)) -> unsure;
    # 3: a tie of the two leading classes -> the lower id, below the threshold anyway; 4: empty
    mean = np.array([[thr, 1 - thr, 0.0], [0.0, below, 1 - below], [rate / Cn, 0.2, 1 - rate / Cn - 0.2], [0.1, 0.45, 0.45],
                     [0.0, 0.0, 0.0]])
    votes = np.array([[n, 0, 0], [0, n, 0], [n, 0, 0], [0, 0, n], [0, 0, 0]])
    calls = _calls(votes, prob=mean * n, unsure_rate=rate)
    ids, conf = calls.consensus("mean_prob")
    assert ids.tolist() == [0, -1, -1, -1, -2]
    np.testing.assert_array_equal(conf[:4], (mean * n)[[0, 1, 2, 3], [0, 1, 0, 1]] / n)
    assert math.isnan(conf[4])
    assert _calls(votes, prob=mean * n, unsure_rate=1.0).consensus("mean_prob")[0].tolist() == [0, 1, 0, 1, -2]
    want = R.consensus(calls.prob_sum.numpy(), calls.votes.numpy(), calls.tally.numpy(), rate, "mean_prob")
    np.testing.assert_array_equal(ids, want[0])
    np.testing.assert_array_equal(conf, want[1])
    np.testing.assert_array_equal(calls.mean_prob().numpy()[:4], mean[:4] * n / n)


def test_frame_and_cell_labels():
    calls = _calls([[3, 5, 5, 0], [2, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 7]], unsure=[0, 4, 0, 0], bad=[1, 0, 2, 0],
                   conf=[6.5, 4.5, 0.0, 7.0], names=["b cells", "mixed", "nobody", "t cells"])
    f = calls.frame()
    assert list(f.columns) == ["cluster", "n_cells", "n_unsure", "n_bad", "cell_type", "cell_subtype", "fraction", "mean_prob",
                               "mean_confidence", "second_type", "second_fraction"]
    assert f["cluster"].tolist() == ["b cells", "mixed", "nobody", "t cells"]
    assert f["n_cells"].tolist() == [13, 9, 0, 7] and f["n_unsure"].tolist() == [0, 4, 0, 0] and f["n_bad"].tolist() == [1, 0, 2, 0]
    assert f["cell_type"].tolist() == ["type1", "unsure", "empty", "type3"] == f["cell_subtype"].tolist()
    np.testing.assert_array_equal(f["fraction"].to_numpy()[[0, 1, 3]], [5 / 13, 3 / 9, 1.0])
    np.testing.assert_array_equal(f["mean_confidence"].to_numpy()[[0, 1, 3]], [0.5, 0.5, 1.0])
    assert math.isnan(f["fraction"][2]) and math.isnan(f["mean_confidence"][2])
    assert f["second_type"].tolist() == ["type2", "type0", None, None]
    np.testing.assert_array_equal(f["second_fraction"].to_numpy()[:2], [5 / 13, 2 / 9])
    assert math.isnan(f["second_fraction"][2]) and math.isnan(f["second_fraction"][3])
    # a label map renames type and subtype, as _prediction_frame does
    calls.label_map = ({"type1": "B cell"}, {"type1": "B cell, naive"})
    f = calls.frame()
    assert f["cell_type"].tolist() == ["B cell", "unsure", "empty", "type3"]
    assert f["cell_subtype"].tolist() == ["B cell, naive", "unsure", "empty", "type3"]
    # the calls broadcast to the cells: by id and by name; -1 stays -1
    assert calls.cell_labels([0, 3, 3, -1, 1, 2]).tolist() == [1, 3, 3, -1, -1, -2]
    assert calls.cell_labels(np.array(["t cells", "b cells"])).tolist() == [3, 1]
    assert calls.cell_labels([0, 1], min_fraction=0.5).tolist() == [-1, -1]
    assert calls.cell_labels(torch.tensor([3, 0]), rule="mean_prob").dtype == np.int64
    with pytest.raises(ValueError, match="out of range"):
        calls.cell_labels([0, 4])
    with pytest.raises(ValueError, match="not one of"):
        calls.cell_labels(["t cells", "nk cells"])


def test_into_requires_the_same_clusters_and_types():
    calls = _calls([[1, 2], [3, 4]], names=["a", "b"])
    calls._require_same(["a", "b"], ["type0", "type1"])
    with pytest.raises(ValueError, match="into: the table holds 2 clusters"):
        calls._require_same(["a", "b", "c"], ["type0", "type1"])
    with pytest.raises(ValueError, match="into: the table's cluster names differ"):
        calls._require_same(["a", "c"], ["type0", "type1"])
    with pytest.raises(ValueError, match="into: the table's cell types differ"):
        calls._require_same(["a", "b"], ["type0", "other"])
    with pytest.raises(ValueError, match="into: the table's cell types differ"):
        calls._require_same(["a", "b"], ["type0", "type1", "type2"])
    with pytest.raises(ValueError, match="into: the table's cluster names differ"):
        api._cluster_ids([0, 1], cluster_names=["a", "c"], into=calls)


def test_cluster_names_are_factorised_in_sorted_order_or_matched_against_into():
    ids, names = api._cluster_ids(["T", "B", "nk", "B", "T"])
    assert names == ["B", "T", "nk"] and ids.tolist() == [1, 0, 2, 0, 1] and ids.dtype == np.int64
    ids, names = api._cluster_ids(np.array(["10", "2", "10"]))                  # names, so their order is a string's
    assert names == ["10", "2"] and ids.tolist() == [0, 1, 0]
    calls = _calls([[1, 2], [3, 4], [0, 0]], names=["nk", "B", "T"])
    ids, names = api._cluster_ids(["T", "B", "B"], into=calls)
    assert names == ["nk", "B", "T"] and ids.tolist() == [2, 1, 1]
    with pytest.raises(ValueError, match="'mono' is not one of"):
        api._cluster_ids(["T", "mono"], into=calls)
    ids, names = api._cluster_ids(["x", "y"], cluster_names=["y", "x", "z"])
    assert names == ["y", "x", "z"] and ids.tolist() == [1, 0]
    # integer ids
    ids, names = api._cluster_ids(np.array([2, -1, 0], np.int32), n_clusters=3)
    assert names == ["0", "1", "2"] and ids.tolist() == [2, -1, 0]
    assert api._cluster_ids(torch.tensor([1, 0]), cluster_names=["a", "b"])[1] == ["a", "b"]
    assert api._cluster_ids([1, 0], into=calls)[1] == ["nk", "B", "T"]
    with pytest.raises(ValueError, match="cluster_names or n_clusters"):
        api._cluster_ids([0, 1])
    with pytest.raises(ValueError, match="out of range"):
        api._cluster_ids([0, 3], n_clusters=3)
    with pytest.raises(ValueError, match="out of range"):
        api._cluster_ids([0, -2], n_clusters=3)
    with pytest.raises(ValueError, match="n_clusters = 2 but 3"):
        api._cluster_ids([0], cluster_names=["a", "b", "c"], n_clusters=2)
    with pytest.raises(ValueError, match="lists 2 cells, the batch holds 3"):
        api._cluster_ids([0, 1], n_clusters=2, n_cells=3)
    with pytest.raises(ValueError, match="integer ids or str names"):
        api._cluster_ids([0.5, 1.0], n_clusters=2)
    with pytest.raises(ValueError, match="one id or name per cell"):
        api._cluster_ids([[0, 1]], n_clusters=2)
