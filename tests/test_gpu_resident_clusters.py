"""``ResidentPredictor.annotate`` and its kernel ``wgnn_group_class_reduce`` on the GPU, against the plain-loop fp64
restatement of tests/clusters_reference.py: bit for bit on lattice cases (every partial sum exact in fp64), under the derived
bound on N(0, 3) logits, the bad-cell rule, accumulation, malformed operands through the C ABI, and the predictor end to end.

The bound, for an element of ``prob_sum`` / ``conf_sum`` of a group of n_k cells and C classes (u = 2^-52):

    |got - want| <= (n_k + C + 8) u |want| + 2^-1074

Derivation (clusters_reference.py has it in full): a term p_ij = exp(l_j - m) / Z carries the rounding of l_j - m (u/2, and
what exp makes of it: below u for f32 logits), exp's own error (1 ulp), Z's C - 1 additions of non-negative terms ((C - 1) u in
any order, plus the terms' 2 u) and the divide (u/2): within (C + 5) u, the reference's own terms within 4 u.  The bin then
adds n_k non-negative terms in some order: (n_k - 1) u/2.  Non-negative terms carry relative errors to the sum unamplified.
It is not a measured number: any fp32 step in the chain (an f32 exp, an f32 softmax, an f32 sum) is an error of ~2^-24
relative and misses the bound by about 2^28.  Every test prints its worst |got - want| / bound before it asserts."""
import ctypes as C
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api, ops

import clusters_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _wide(logits, extra=3):
    """``logits`` as a view of a wider matrix whose guard columns hold NaN: ld_logits = C + extra."""
    B, Cn = logits.shape
    buf = torch.full((B, Cn + extra), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :Cn] = t(logits)
    return buf[:, :Cn]


def _guarded(K, Cn):
    """The four outputs as views into buffers with PAD guard rows of NaN / -12345 before and after."""
    shapes = ((K, Cn), torch.float64), ((K,), torch.float64), ((K, Cn), torch.int32), ((K, 3), torch.int32)
    bufs = [torch.full((K + 2 * PAD,) + s[1:], float("nan") if d == torch.float64 else -12345, dtype=d, device=DEV) for s, d in shapes]
    return bufs, tuple(b[PAD:PAD + K] for b in bufs)


def _guards_untouched(bufs, K):
    for b in bufs:
        edge = torch.cat([b[:PAD].reshape(-1), b[PAD + K:].reshape(-1)])
        assert bool(torch.isnan(edge).all()) if b.dtype == torch.float64 else bool((edge == -12345).all())


def _host(outs):
    return tuple(o.cpu().numpy() for o in outs)


def _assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("prob_sum", "conf_sum", "votes", "tally")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name)


def _assert_bounded(got, want, Cn, what=""):
    """Counts equal, sums under the bound; returns the worst |got - want| / bound."""
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32 and got[0].dtype == np.float64 and got[1].dtype == np.float64
    worst = 0.0
    for g, w in zip(got[:2], want[:2]):
        err, lim = np.abs(g - w), R.bound(w, want[3][:, 0], Cn)
        worst = max(worst, float((err / lim).max()))
        assert (err <= lim).all(), (what, worst)
    return worst


def _reduce_guarded(c, logits=None, **kw):
    bufs, outs = _guarded(c.K, c.C)
    got = ops.group_class_reduce(_wide(c.logits if logits is None else logits), t(c.label), t(c.group), c.K, out=outs, **kw)
    assert all(g is o for g, o in zip(got, outs))
    _guards_untouched(bufs, c.K)
    return _host(got)


# ------------------------------------------------------------------------------------------------
# 1. the definition, bit for bit on lattice cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cn,K", R.CASES)
def test_lattice_cases_match_the_reference_bit_for_bit(B, Cn, K):
    c = R.lattice_case(B, Cn, K)
    want = R.reduce(c.logits, c.label, c.group, K)
    _assert_equal(_reduce_guarded(c), want, (B, Cn, K))
    if B:
        assert (c.label == -1).any() or B < 5
    # int64 ids and labels, own outputs, contiguous logits: the same bits
    got = ops.group_class_reduce(t(c.logits), t(c.label.astype(np.int64)), t(c.group.astype(np.int64)), K)
    _assert_equal(_host(got), want, (B, Cn, K, "int64"))


@pytest.mark.parametrize("name", R.SPECIAL)
def test_lattice_special_batches(name):
    c = R.special(name)
    want = R.reduce(c.logits, c.label, c.group, c.K)
    _assert_equal(_reduce_guarded(c), want, name)
    if name == "empty_group":
        assert want[3][1].tolist() == [0, 0, 0] and want[3][0, 0] > 0
    if name == "all_skipped":
        assert not want[3].any() and not want[0].any()
    if name == "one_cell_group":
        assert int(want[3][1, 0] + want[3][1, 2]) == 1
    if name == "three_chunks":
        assert want[3][1, 0] > 3 * 256


# ------------------------------------------------------------------------------------------------
# 2. random logits under the derived bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cn,K", [c for c in R.CASES if c[0]])
def test_random_cases_are_within_the_derived_bound(B, Cn, K):
    c = R.random_case(B, Cn, K)
    want = R.reduce(c.logits, c.label, c.group, K)
    worst = _assert_bounded(_reduce_guarded(c), want, Cn, (B, Cn, K))
    print(f"B={B} C={Cn} K={K}: worst |got - want| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------
# 3. bad cells
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [5, 16, 80])
def test_bad_cells_are_counted_in_the_tally_only(Cn):
    c = R.random_case(400, Cn, 3, seed=Cn)
    rng = np.random.default_rng(Cn)
    rows = rng.permutation(c.B)
    nan, pinf, ninf, part = rows[:30], rows[30:60], rows[60:90], rows[90:150]
    c.logits[nan, rng.integers(0, Cn, 30)] = np.nan
    c.logits[pinf, rng.integers(0, Cn, 30)] = np.inf
    c.logits[ninf] = -np.inf
    c.logits[part, rng.integers(0, Cn, 60)] = -np.inf           # beside finite logits: takes part, p = 0
    c.logits[part[:5], :Cn - 1] = -np.inf                       # one finite logit left: p = 1 there
    c.logits[part[:5], Cn - 1] = 0.5
    want = R.reduce(c.logits, c.label, c.group, c.K)
    got = _reduce_guarded(c)
    worst = _assert_bounded(got, want, Cn, Cn)
    print(f"C={Cn}: worst |got - want| / bound = {worst:.3f}")
    bad = np.zeros(c.B, bool)
    bad[rows[:90]] = True
    on = (c.group >= 0)
    np.testing.assert_array_equal(got[3][:, 2], np.bincount(c.group[on & bad], minlength=c.K))
    np.testing.assert_array_equal(got[3][:, 0], np.bincount(c.group[on & ~bad], minlength=c.K))
    assert (got[3][:, 0] == got[2].sum(1) + got[3][:, 1]).all()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the lattice form of the same rule is exact
    c = R.lattice_case(300, Cn, 3, seed=Cn + 1)
    c.logits[::7] = -np.inf
    c.logits[3::11, 0] = np.nan
    c.logits[5::13, Cn - 1] = np.inf
    _assert_equal(_reduce_guarded(c), R.reduce(c.logits, c.label, c.group, c.K), Cn)


# ------------------------------------------------------------------------------------------------
# 4. robustness
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cn,K", [(1500, 16, 3), (1500, 65, 200), (700, 5, 1)])
def test_two_calls_give_identical_bits(B, Cn, K):
    c = R.random_case(B, Cn, K, seed=B + Cn)
    args = (t(c.logits), t(c.label), t(c.group), K)
    a, b = ops.group_class_reduce(*args), ops.group_class_reduce(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("B,Cn,K", [(1500, 16, 3), (1001, 80, 200)])
def test_accumulate_over_two_halves_equals_one_call(B, Cn, K):
    for kind in ("lattice", "random"):
        c = (R.lattice_case if kind == "lattice" else R.random_case)(B, Cn, K, seed=B + K)
        want = R.reduce(c.logits, c.label, c.group, K)
        bufs, outs = _guarded(K, Cn)
        h = B // 2 + 1
        ops.group_class_reduce(_wide(c.logits[:h]), t(c.label[:h]), t(c.group[:h]), K, out=outs)        # overwrites the NaNs
        first = R.reduce(c.logits[:h], c.label[:h], c.group[:h], K)
        assert np.array_equal(outs[2].cpu().numpy(), first[2]) and not bool(torch.isnan(outs[0]).any())
        ops.group_class_reduce(_wide(c.logits[h:]), t(c.label[h:]), t(c.group[h:]), K, out=outs, accumulate=True)
        _guards_untouched(bufs, K)
        if kind == "lattice":
            _assert_equal(_host(outs), want, (B, Cn, K))
        else:
            worst = _assert_bounded(_host(outs), want, Cn, (B, Cn, K))
            print(f"B={B} C={Cn} K={K} accumulate: worst |got - want| / bound = {worst:.3f}")
    with pytest.raises(sda.WgnnError, match="accumulate needs"):
        ops.group_class_reduce(t(c.logits), t(c.label), t(c.group), K, accumulate=True)


def test_op_refusals_name_the_check_and_the_process_goes_on():
    c = R.lattice_case(65, 5, 3)
    lg, lb, gr = t(c.logits), t(c.label), t(c.group)
    for bad in (3, -2):
        g = gr.clone(); g[7] = bad
        with pytest.raises(sda.WgnnError, match="group id out of range"):
            ops.group_class_reduce(lg, lb, g, 3)
    with pytest.raises(sda.WgnnError, match="one id per cell"):
        ops.group_class_reduce(lg, lb, gr[:-1], 3)
    with pytest.raises(sda.WgnnError, match="label must hold"):
        ops.group_class_reduce(lg, lb[:-1], gr, 3)
    with pytest.raises(sda.WgnnError, match="float32"):
        ops.group_class_reduce(lg.double(), lb, gr, 3)
    with pytest.raises(sda.WgnnError, match="must be positive"):
        ops.group_class_reduce(lg, lb, gr, 0)
    with pytest.raises(sda.WgnnError, match="GPU only"):
        ops.group_class_reduce(lg, lb, gr.cpu(), 3)
    with pytest.raises(sda.WgnnError, match="out must be"):
        ops.group_class_reduce(lg, lb, gr, 3, out=tuple(torch.zeros(3, 5, device=DEV) for _ in range(4)))
    # check=False: an id outside [0, K) takes no part instead
    g = c.group.copy(); g[7] = 3; g[9] = -7
    want_group = np.where((g < 0) | (g >= 3), -1, g)
    got = ops.group_class_reduce(lg, lb, t(g), 3, check=False)
    _assert_equal(_host(got), R.reduce(c.logits, c.label, want_group, 3), "check=False")


def _abi(logits, ld, label, order, seg, B, K, Cn, outs, flags=0):
    nb = C.c_int64()
    assert _lib.lib().wgnn_group_class_reduce_workspace(B, K, Cn, C.addressof(nb)) == 0
    ws = torch.full((nb.value // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV)
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = _lib.call(torch.device(DEV), "wgnn_group_class_reduce", ptr(logits), ld, ptr(label), ptr(order), ptr(seg), B, K, Cn,
                   *(o.data_ptr() for o in outs), ws.data_ptr(), nb.value, flags, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("Cn", [16, 65])
def test_out_of_range_order_and_label_entries_take_no_part(Cn):
    """Through the C ABI, past every wrapper check: the kernel must neither read outside its operands nor count the entry."""
    K, B = 3, 700
    c = R.lattice_case(B, Cn, K, seed=11)
    label = c.label.copy()
    label[[3, 50, 300]] = [Cn, -2, 2 ** 30]
    group = c.group.copy()
    group[[3, 50, 300]] = [0, 1, 2]                              # the cells with a label outside [-1, C) are in a group
    order, seg = [], [0]
    for k in range(K):
        ids = np.nonzero(group == k)[0].astype(np.int64)
        ids = np.insert(ids, [0, len(ids) // 2, len(ids)], [-5, B, 2 ** 31 - 1])       # three entries outside [0, B) per group
        order.append(ids)
        seg.append(seg[-1] + len(ids))
    order = np.concatenate(order).astype(np.int32)
    want = R.reduce(c.logits, label, group, K)                   # the reference drops labels outside [-1, C) as well
    # those three cells are counted nowhere: neither among the cells that take part (the unsure ones are among them) nor as bad
    assert int(want[3][:, 0].sum() + want[3][:, 2].sum()) == int((group >= 0).sum()) - 3
    bufs, outs = _guarded(K, Cn)
    wide = _wide(c.logits)
    assert _abi(wide, wide.stride(0), t(label), t(order), t(np.asarray(seg, np.int64)), B, K, Cn, outs) == 0
    _guards_untouched(bufs, K)
    _assert_equal(_host(outs), want, Cn)
    # no cells at all: NULL operands are fine, every output is still written
    bufs, outs = _guarded(K, Cn)
    assert _abi(None, Cn, None, None, t(np.zeros(K + 1, np.int64)), 0, K, Cn, outs) == 0
    _guards_untouched(bufs, K)
    assert all(not bool(o.any()) for o in outs)
    # seg_ptr[K] == 0 with rows: NULL operands too
    bufs, outs = _guarded(K, Cn)
    assert _abi(None, Cn, None, None, t(np.zeros(K + 1, np.int64)), B, K, Cn, outs) == 0
    assert all(not bool(o.any()) for o in outs)


def test_each_abi_error_code_comes_with_a_message():
    lib = _lib.lib()
    K, Cn, B = 3, 5, 65
    c = R.lattice_case(B, Cn, K)
    lg, lb, gr = t(c.logits), t(c.label), t(c.group)
    order = torch.arange(B, dtype=torch.int32, device=DEV)
    seg = t(np.array([0, 20, 40, B], np.int64))
    _, outs = _guarded(K, Cn)
    nb = C.c_int64()
    assert lib.wgnn_group_class_reduce_workspace(B, K, Cn, C.addressof(nb)) == 0
    ws = torch.zeros(nb.value // 8 + 2, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)

    def run(logits=lg.data_ptr(), ld=Cn, label=lb.data_ptr(), order=order.data_ptr(), seg=seg.data_ptr(), n_rows=B, k=K, cn=Cn,
            prob=outs[0].data_ptr(), conf=outs[1].data_ptr(), votes=outs[2].data_ptr(), tally=outs[3].data_ptr(),
            w=ws.data_ptr(), w_bytes=nb.value, flags=0):
        return _lib.call(torch.device(DEV), "wgnn_group_class_reduce", logits, ld, label, order, seg, n_rows, k, cn, prob, conf,
                         votes, tally, w, w_bytes, flags, None)

    before = _host(outs)
    cases = [(-1, "required", dict(prob=None)), (-1, "required", dict(conf=None)), (-1, "required", dict(votes=None)),
             (-1, "required", dict(tally=None)), (-1, "seg_ptr", dict(seg=None)), (-1, "n_groups", dict(k=0)),
             (-1, "n_classes", dict(cn=0)), (-1, "ld_logits", dict(ld=Cn - 1)), (-1, "n_rows", dict(n_rows=-1)),
             (-1, "n_rows", dict(n_rows=2 ** 31)), (-1, "WGNN_CLUSTERS_ACCUMULATE", dict(flags=1)),
             (-2, "8-byte", dict(prob=outs[0].data_ptr() + 4)), (-2, "8-byte", dict(conf=outs[1].data_ptr() + 4)),
             (-2, "8-byte", dict(seg=seg.data_ptr() + 4)), (-2, "4-byte", dict(logits=lg.data_ptr() + 2)),
             (-2, "4-byte", dict(label=i32.data_ptr() + 1)), (-2, "4-byte", dict(order=i32.data_ptr() + 3)),
             (-2, "4-byte", dict(votes=outs[2].data_ptr() + 2)), (-2, "4-byte", dict(tally=outs[3].data_ptr() + 1)),
             (-4, "workspace", dict(w=None)), (-4, "workspace", dict(w_bytes=nb.value - 1)), (-4, "workspace", dict(w_bytes=-1))]
    for code, word, kw in cases:
        assert run(**kw) == code, kw
        msg = lib.wgnn_last_error_string(code).decode()
        assert "wgnn_group_class_reduce" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    for a, b in zip(before, _host(outs)):                        # refused before any launch: nothing was written
        assert np.array_equal(a, b, equal_nan=True)
    assert run() == 0                                            # and the next call runs
    torch.cuda.synchronize()
    group = np.repeat([0, 1, 2], [20, 20, B - 40])
    _assert_equal(_host(outs), R.reduce(c.logits, c.label, group, K), "after the refusals")


# ------------------------------------------------------------------------------------------------
# 5. the predictor end to end
# ------------------------------------------------------------------------------------------------
def _random_bundle(tmp_path, n_layers, G=500, n_sup=200, dense=16, hidden=12, n_cls=5, seed=0):
    """A bundle written by hand from a randomly initialised GNN (no fit)."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    genes = [f"Gene{i}" for i in range(G)]
    root = tmp_path / f"rand{n_layers}"
    b = api.BundlePaths(root, "mouse", "Rand", layout="flat", for_write=True)
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
    return root, G


def _batch(G, n=300, seed=7):
    batch = sp.random(n, G, density=0.1, random_state=seed, format="csr", dtype=np.float32)
    batch.data = (1.0 + np.round(16.0 * batch.data) / 4.0).astype(np.float32)       # quarters: exact through a CSV file
    batch.sort_indices()
    return batch


def _check_calls(calls, label, logits, ids, names, rp, what=""):
    """``calls`` against the reference fed with classify's own labels and logits for the same batch."""
    K = len(names)
    want = R.reduce(logits.cpu().numpy(), label, ids, K)
    assert isinstance(calls, sda.ClusterCalls) and calls.prob_sum.is_cuda
    assert list(calls.cluster_names) == list(names) and list(calls.id2label) == list(rp.id2label)
    assert calls.unsure_rate == rp.unsure_rate
    got = _host((calls.prob_sum, calls.conf_sum, calls.votes, calls.tally))
    worst = _assert_bounded(got, want, rp.n_classes, what)
    print(f"{what}: worst |got - want| / bound = {worst:.3f}")
    np.testing.assert_array_equal(calls.n_cells, want[3][:, 0])
    for rule in ("vote", "mean_prob"):
        ref_ids, ref_conf = R.consensus(want[0], want[2], want[3], rp.unsure_rate, rule)
        got_ids, got_conf = calls.consensus(rule)
        np.testing.assert_array_equal(got_ids, R.consensus(got[0], got[2], got[3], rp.unsure_rate, rule)[0])
        if rule == "vote":                                        # counts alone: equal to the reference's whatever the sums' last bits
            np.testing.assert_array_equal(got_ids, ref_ids)
            np.testing.assert_array_equal(got_conf, ref_conf)
    return want


@pytest.mark.parametrize("route", ["fused", "graph"])
@pytest.mark.parametrize("n_layers", [1, 2])
def test_annotate_end_to_end(tmp_path, monkeypatch, n_layers, route):
    root, G = _random_bundle(tmp_path, n_layers, seed=n_layers)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    if route == "graph":
        monkeypatch.setattr(api, "RESIDENT_FUSED_MAX_WORK", 0)
    batch = _batch(G)
    label, _, logits = rp.classify(batch)
    assert rp.last_route == route
    rng = np.random.default_rng(n_layers)
    ids = rng.integers(-1, 7, batch.shape[0])
    calls = rp.annotate(batch, ids, n_clusters=7)
    assert rp.last_route == route
    _check_calls(calls, label, logits, ids, [str(i) for i in range(7)], rp, f"L={n_layers} {route}")
    assert int(calls.n_cells.sum() + calls.n_bad.sum()) == int((ids >= 0).sum())
    # classify is untouched: the same bits before and after
    again = rp.classify(batch)
    assert torch.equal(again[2], logits) and np.array_equal(again[0], label)
    # names: given with the ids, or as the clusters themselves (factorised in sorted order)
    names = [f"cluster{i}" for i in range(7)]
    by_name = rp.annotate(batch, torch.from_numpy(ids), cluster_names=names)
    assert list(by_name.cluster_names) == names and torch.equal(by_name.votes, calls.votes) and torch.equal(by_name.prob_sum, calls.prob_sum)
    words = np.array(["zeta", "alpha", "mid"])[ids % 3]
    by_word = rp.annotate(batch, words)
    _check_calls(by_word, label, logits, np.array([2, 0, 1])[ids % 3], ["alpha", "mid", "zeta"], rp, f"L={n_layers} {route} names")
    # a device triple gives the same bits
    dev_csr = (t(batch.indptr.astype(np.int64)), t(batch.indices), t(batch.data))
    same = rp.annotate(dev_csr, ids, n_clusters=7)
    assert torch.equal(same.prob_sum, calls.prob_sum) and torch.equal(same.tally, calls.tally)
    f = calls.frame()
    assert len(f) == 7 and f["n_cells"].tolist() == calls.n_cells.tolist()
    cells = calls.cell_labels(ids)
    assert cells.shape == ids.shape and (cells[ids < 0] == -1).all()
    np.testing.assert_array_equal(cells[ids >= 0], calls.consensus()[0][ids[ids >= 0]])
    with pytest.raises(ValueError, match="cluster_names or n_clusters"):
        rp.annotate(batch, ids)
    with pytest.raises(ValueError, match="lists 299 cells"):
        rp.annotate(batch, ids[:-1], n_clusters=7)
    with pytest.raises(ValueError, match="out of range"):
        rp.annotate(batch, ids, n_clusters=6)
    with pytest.raises(ValueError, match="into"):
        rp.annotate(batch, ids, n_clusters=8, into=calls)
    with pytest.raises(ValueError, match="not one of"):
        rp.annotate(batch, np.array(["alpha", "omega"])[ids % 2], into=by_word)


def test_annotate_streams_three_batches_into_one_table(tmp_path):
    root, G = _random_bundle(tmp_path, 2, hidden=20, seed=9)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    batch = _batch(G, 301, 11)
    words = np.array(["b", "a", "c", "d"])[np.random.default_rng(3).integers(0, 4, 301)]
    words[:100][words[:100] == "d"] = "a"                         # the first batch does not meet every cluster: names come from `into`
    label, _, logits = rp.classify(batch)
    names = ["a", "b", "c", "d"]
    ids = np.array([names.index(w) for w in words])
    table = rp.annotate(batch[:100], ids[:100], cluster_names=names)
    for lo, hi in ((100, 101), (101, 301)):
        got = rp.annotate(batch[lo:hi], words[lo:hi], into=table)
        assert got is table
    whole = rp.annotate(batch, words)
    assert list(whole.cluster_names) == names
    assert torch.equal(table.votes, whole.votes) and torch.equal(table.tally, whole.tally)
    _check_calls(table, label, logits, ids, names, rp, "three batches")    # a cell's logits do not depend on its batch
    want = _check_calls(whole, label, logits, ids, names, rp, "one batch")
    for a, b, w in ((table.prob_sum, whole.prob_sum, want[0]), (table.conf_sum, whole.conf_sum, want[1])):
        err = (a - b).abs().cpu().numpy()
        assert (err <= 2 * R.bound(w, want[3][:, 0], rp.n_classes)).all()  # each of the two is within the bound of the exact sum


def test_annotate_passes_genes_and_normalize_through(tmp_path):
    root, G = _random_bundle(tmp_path, 1, seed=5)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    rng = np.random.default_rng(5)
    genes = [f"Gene{i}" for i in rng.permutation(G)[:300]] + [f"Other{i}" for i in range(40)]
    counts = rng.poisson(0.3, (120, len(genes))).astype(np.float32)
    ids = rng.integers(-1, 4, 120)
    for normalize in (None, "lognorm"):
        label, _, logits = rp.classify(counts, genes=genes, normalize=normalize)
        calls = rp.annotate(counts, ids, n_clusters=4, genes=genes, normalize=normalize)
        _check_calls(calls, label, logits, ids, ["0", "1", "2", "3"], rp, f"genes=, normalize={normalize}")
    other = rp.classify(counts, genes=genes)[2]
    assert not torch.equal(other, logits)                        # lognorm did change what the model saw
    with pytest.raises(ValueError, match="normalize needs genes"):
        rp.annotate(_batch(G), np.zeros(300, np.int64), n_clusters=1, normalize="lognorm")


def test_annotate_file_round_trip(tmp_path):
    root, G = _random_bundle(tmp_path, 1, seed=4)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    part = _batch(G, 90, 31)
    cells = [f"C{j}" for j in range(90)]
    data = tmp_path / "mouse_Rand7_data.csv"
    pd.DataFrame(part.toarray().T, index=rp.id2gene, columns=cells).to_csv(data)
    words = np.array(["T cell", "B cell", "3"])[np.random.default_rng(1).integers(0, 3, 90)]
    cf = tmp_path / "mouse_Rand7_clusters.csv"
    pd.DataFrame({"Cell": cells, "Cluster": [" " + w for w in words]}).to_csv(cf)           # stripped, like the cell-type files
    out = rp.annotate_file(data, cf, save_path=tmp_path / "out")
    want = rp.annotate(part, words).frame()
    pd.testing.assert_frame_equal(out, want)
    assert out["cluster"].tolist() == ["3", "B cell", "T cell"]
    saved = pd.read_csv(tmp_path / "out" / "mouse_Rand_clusters.csv")
    assert list(saved.columns) == list(out.columns) and len(saved) == 3
    assert saved["cluster"].astype(str).tolist() == out["cluster"].tolist() and saved["cell_type"].tolist() == out["cell_type"].tolist()
    np.testing.assert_allclose(saved["fraction"].to_numpy(), out["fraction"].to_numpy(), rtol=1e-15)
    by_prob = rp.annotate_file(data, cf, rule="mean_prob")
    pd.testing.assert_frame_equal(by_prob, rp.annotate(part, words).frame("mean_prob"))
    pd.DataFrame({"Cell": cells[::-1], "Cluster": words}).to_csv(cf)
    with pytest.raises(ValueError, match="cell order"):
        rp.annotate_file(data, cf)
    with pytest.raises(ValueError, match="rule"):
        rp.annotate_file(data, cf, rule="majority")


def test_predict_matrix_gains_the_cluster_columns(tmp_path):
    root, G = _random_bundle(tmp_path, 1, seed=6)
    rp = sda.ResidentPredictor("mouse", "Rand", model_path=root, unsure_rate=1.02)
    x = _batch(G, 80, 41).toarray()
    ids = np.random.default_rng(2).integers(-1, 3, 80)
    index = [f"cell{i}" for i in range(80)]
    plain = rp.predict_matrix(x, rp.id2gene, index=index)
    assert list(plain.columns) == ["index", "cell_type"]
    pred = rp.classify(x, genes=rp.id2gene)[0]
    assert plain["cell_type"].tolist() == [rp.id2label[p] if p >= 0 else "unsure" for p in pred]
    for rule in ("vote", "mean_prob"):
        out = rp.predict_matrix(x, rp.id2gene, index=index, clusters=ids, rule=rule)
        assert list(out.columns) == ["index", "cell_type", "cluster_type", "cluster_subtype"]
        pd.testing.assert_frame_equal(out[["index", "cell_type"]], plain)
        calls = rp.annotate(x, ids, n_clusters=3, genes=rp.id2gene)
        per_cell = calls.cell_labels(ids, rule=rule)
        name = lambda p: rp.id2label[p] if p >= 0 else {-1: "unsure", -2: "empty"}[int(p)]
        want = [name(p) if g >= 0 else None for p, g in zip(per_cell, ids)]
        assert out["cluster_type"].tolist() == want == out["cluster_subtype"].tolist()
    words = np.array(["x", "y"])[ids % 2]
    out = rp.predict_matrix(x, rp.id2gene, clusters=words, min_fraction=1.0)
    strict = rp.annotate(x, words, genes=rp.id2gene).cell_labels(words, min_fraction=1.0)
    assert out["cluster_type"].tolist() == [rp.id2label[p] if p >= 0 else "unsure" for p in strict]
    with pytest.raises(ValueError, match="lists 79 cells"):
        rp.predict_matrix(x, rp.id2gene, clusters=ids[:-1])
