"""K5, ``wgnn_sample_rows``, on the GPU against the bit-exact restatement of its draw law (tests/sample_reference.py, from
include/wgnn.h): all five outputs EQUAL, ``out_val`` and ``out_inv`` as uint32 bits, at every k on and around the boundaries of
the lane's four registers, over rows with fewer than, exactly, one more than and far more than k candidates; the padding and
the guards around every output keep their sentinel; every word of the key; and through ``sampler.sample_block_static`` /
``sample_nodeflow_static``.  ``out_inv`` is held to ``np.float32(1) / np.float32(n)`` exactly: the build sets no fast-math flag
(tests/test_sample_abi.py) and the compiler rounds an fp32 division correctly by default.  Every launch runs twice and must
give the same bits."""
import functools

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from conftest import small_case
from scdeepsort_amd import _lib
from scdeepsort_amd.graph import _stream
from scdeepsort_amd.sampler import DeviceSampler, sample_block_static, sample_nodeflow_static

import sample_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "wgnn_sample_rows"
LEAD, TRAIL = 3, 5                                                     # guard elements before and after every output
NAMES = ("out_col", "out_val", "out_cnt", "out_self", "out_inv")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)


def _assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        if g.dtype == np.float32:
            g, w = _bits(g), _bits(w)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, what))


@functools.lru_cache(maxsize=1)
def _operand():
    host = R.fixture()
    return host, tuple(torch.from_numpy(a.copy()).to(DEV) for a in host)


def _launch_once(dev_op, n, k, ids, seed, step, stream_id):
    """one launch into inner views of sentinel-filled tensors; returns the five outputs as numpy, [n, k] and [n], after checking
    that the guards before and after every view kept the sentinel"""
    rowptr, col, val = dev_op
    step_t = torch.tensor([step], dtype=torch.int64, device=DEV)
    sizes = (n * k, n * k, n, n, n)
    dtypes = (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)
    pads = (R.PAD_COL, R.PAD_VAL, R.PAD_COL, R.PAD_VAL, R.PAD_VAL)
    whole = [torch.full((LEAD + s + TRAIL,), p, dtype=t, device=DEV) for s, t, p in zip(sizes, dtypes, pads)]
    views = [w[LEAD: LEAD + s] for w, s in zip(whole, sizes)]
    _lib.run(torch.device(DEV), NAME, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), None if ids is None else ids.data_ptr(),
             n, k, seed, step_t.data_ptr(), stream_id, *(w.data_ptr() + 4 * LEAD for w in whole), _stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert int(step_t[0]) == step                                      # the entry reads the counter, it does not advance it
    for w, s, p, name in zip(whole, sizes, pads, NAMES):
        assert bool((w[:LEAD] == p).all()) and bool((w[LEAD + s:] == p).all()), name
    out = [v.cpu().numpy() for v in views]
    return [out[0].reshape(n, k), out[1].reshape(n, k), *out[2:]]


def _check(k, row_ids=None, seed=7, step=0, stream_id=0):
    """the kernel against the restatement at one (k, row_ids, key): exact, twice the same bits, padding and guards untouched,
    operands unchanged"""
    host, dev_op = _operand()
    ids = None if row_ids is None else torch.from_numpy(np.asarray(row_ids, np.int32)).to(DEV)
    n = len(R.DEGREES) if row_ids is None else len(row_ids)
    got = _launch_once(dev_op, n, k, ids, seed, step, stream_id)
    again = _launch_once(dev_op, n, k, ids, seed, step, stream_id)
    want = R.sample(*host, row_ids, k, seed, step, stream_id)          # its padding holds the same sentinels
    what = "k=%d seed=%d step=%d stream=%d" % (k, seed, step, stream_id)
    _assert_equal(got, want, what)
    _assert_equal(again, got, what + " (second launch)")
    for h, d, name in zip(host, dev_op, ("rowptr", "col", "val")):
        assert _same(d.cpu().numpy(), h), name
    if ids is not None:
        np.testing.assert_array_equal(ids.cpu().numpy(), np.asarray(row_ids, np.int32))
    return got, want


@pytest.mark.parametrize("k", R.KS)
def test_every_k_is_exact(k):
    got, want = _check(k)
    ms = np.array(R.DEGREES) + 1
    np.testing.assert_array_equal(got[2] + got[3].astype(np.int64), np.minimum(k, ms))
    drew = ms > k                                                      # no vacuity: rows that drew, and rows that took everything
    assert drew.any() and (~drew).any()
    # the specials reach the output with their bits: from k = 65 on the row of degree 65 keeps at least three of its four
    if k >= 65:
        assert np.isin(_bits(got[1][8]), np.array(R.SPECIAL_BITS[8], np.uint32)).sum() >= 3
    # draw order is no sorted order: the longest row lists its positions out of ascending order
    if k >= 63:
        rowptr, col, _ = R.fixture()
        r = len(R.DEGREES) - 1
        pos = {int(c): i for i, c in enumerate(col[rowptr[r]: rowptr[r + 1]])}
        p = [pos[int(c)] for c in got[0][r, : got[2][r]]]
        assert p != sorted(p)


@pytest.mark.parametrize("k", [5, 129])
def test_row_ids(k):
    n_rows = len(R.DEGREES)
    rev = np.concatenate([np.arange(n_rows)[::-1], [22, 22, 21, 0, 21, 20, 9, 9]]).astype(np.int32)       # reversed, with repeats
    got, _ = _check(k, rev, stream_id=2)
    for a, b in ((0, 23), (0, 24), (1, 25), (22, 26), (1, 27), (2, 28), (13, 29), (29, 30)):
        assert rev[a] == rev[b]
        for g in got:                                                  # a repeated row gives the same list in every slot
            assert _same(g[a], g[b])
    plain, _ = _check(k, None, stream_id=2)
    for g, p in zip(got, plain):                                       # the key holds the row, not the slot
        assert _same(g[:n_rows], p[::-1])
    for r in (0, 8, 22):
        _check(k, np.array([r], np.int32), step=4)
    many = (np.arange(4097, dtype=np.int64) * 7 % 23).astype(np.int32)                 # 4097 slots: 1025 workgroups, the last one wave
    _check(k, many, seed=2 ** 63 - 1, step=9, stream_id=1)


def test_no_rows_is_ok_and_writes_nothing():
    _, dev_op = _operand()
    for ids in (None, torch.zeros(4, dtype=torch.int32, device=DEV)):
        out = _launch_once(dev_op, 0, 7, ids, 7, 0, 0)                 # the guards (all there is) are checked inside
        assert out[0].size == 0 and out[2].size == 0


@pytest.mark.parametrize("k", [70, 200])
def test_every_key_word(k):
    steps, streams, seeds = (0, 1, 2 ** 40 + 3), (0, 1, 7, -1), (0, 7, 2 ** 63 - 1, 2 ** 64 - 1)
    seen = {}
    for step in steps:
        for stream_id in streams:
            for seed in seeds:
                got, _ = _check(k, None, seed, step, stream_id)
                seen[(seed, step, stream_id)] = got[0][-1].tobytes()   # the row of degree 5000
    assert len(set(seen.values())) == len(seen) == 48                  # no two keys share that row's draw


@functools.lru_cache(maxsize=1)
def _graph():
    c = small_case(cells=60, genes=50, dim=8, seed=44, density=0.5, test_cells=0)
    g = sda.CellGeneGraph.from_expression(c["expr"], device=DEV)
    host = lambda csr: (csr.rowptr.cpu().numpy(), csr.col.cpu().numpy(), csr.val.cpu().numpy())
    return g, host(g.cg), host(g.gc)


def _block_outputs(blk):
    kk, n = blk.csr.ell_k, blk.rows.shape[0]
    return kk, [blk.csr.col.cpu().numpy().reshape(n, kk), blk.csr.val.cpu().numpy().reshape(n, kk), blk.csr.ell_cnt.cpu().numpy(),
                blk.self_drawn.cpu().numpy(), blk.csr.inv_deg.cpu().numpy()]


@pytest.mark.parametrize("k", [5, 12])
def test_sample_block_static_is_the_restatement_and_advances(k):
    g, cg, gc = _graph()
    seed = 2 ** 63 + 12345                                             # DeviceSampler keeps the low 63 bits
    smp = DeviceSampler(seed, torch.device(DEV))
    assert smp.seed == 12345
    rows = np.array([4, 0, 17, 59, 4, 3, 41], np.int64)
    for csr, host, ids in ((g.cg, cg, rows), (g.cg, cg, None), (g.gc, gc, None)):
        m = np.diff(host[0]) + 1
        assert (m > k).sum() * 2 >= len(m)                             # most rows draw
        for step in (0, 1):
            blk = sample_block_static(csr, None if ids is None else torch.from_numpy(ids).to(DEV), k, smp, stream_id=3)
            kk, got = _block_outputs(blk)
            assert kk == R.block_k(host[0], k) == k
            _assert_equal(got, R.sample(*host, ids, kk, smp.seed, step, 3, 0, 0.0), "step %d" % step)     # the wrapper's padding is zero
            np.testing.assert_array_equal(blk.rows.cpu().numpy(), np.arange(len(m)) if ids is None else ids)
            smp.advance()
        smp.step -= 2
    # k beyond the longest row: the clamp, and every edge of every row
    blk = sample_block_static(g.gc, None, 200, smp, stream_id=0)
    kk, got = _block_outputs(blk)
    assert kk == R.block_k(gc[0], 200) == int(np.diff(gc[0]).max()) + 1 < 200
    _assert_equal(got, R.sample(*gc, None, kk, smp.seed, 0, 0, 0, 0.0))
    np.testing.assert_array_equal(got[2], np.diff(gc[0]))


def test_sample_nodeflow_static_is_the_restatement_block_by_block():
    g, cg, gc = _graph()
    seeds = np.array([4, 0, 17, 59, 3, 41], np.int64)
    smp = DeviceSampler(31, torch.device(DEV))
    for step in (0, 1):
        nf = sample_nodeflow_static(g, torch.from_numpy(seeds).to(DEV), 2, 6, smp)
        assert int(smp.step) == step + 1                               # one advance per NodeFlow
        want = R.nodeflow(cg, gc, seeds, 2, 6, 31, step)
        assert len(nf.blocks) == len(want) == 2 and nf.blocks[1][1] is None and want[1][1] is None
        for i, ((cb, gb), (wc, wg)) in enumerate(zip(nf.blocks, want)):
            for blk, w in ((cb, wc), (gb, wg)):
                if blk is None:
                    continue
                kk, got = _block_outputs(blk)
                assert kk == w[0]
                _assert_equal(got, w[1], "layer %d step %d" % (i, step))
    # the cell block and the gene block of a layer, and the two layers' cell blocks, are keyed apart
    (c0, g0), (c1, _) = want
    assert not np.array_equal(c0[1][0][seeds], c1[1][0])
