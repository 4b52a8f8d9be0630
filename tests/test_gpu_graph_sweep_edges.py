"""The edges of ``wgnn_louvain_sweep`` and ``wgnn_leiden_refine_sweep`` that no whole run reaches: single launches from a singleton
state on a 12-vertex graph whose hub goes down each of the three routes by row length, with labels that are no ids, a long row
that meets no scratch and a vertex without an edge.  What is expected is include/wgnn.h's contract: a vertex whose own label is no
id stays with gain 0 and a status bit, a neighbour whose label is no id adds nothing, and the route changes no bit."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from scdeepsort_amd import _lib
from scdeepsort_amd.graph import _ptr, _stream

import leiden_reference as L
import louvain_reference as R
from test_louvain_reference import csr_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N, HUB, ALONE = 12, 11, 10
LEAVES = list(range(8))
EDGES = [(leaf, HUB) for leaf in LEAVES] + [(0, 1), (8, 9)]
P_OF = np.array([0] * 8 + [8, 8, ALONE, 0], np.int32)         # the moving phase's partition: the star, the pair, the lone vertex
FRAC = Fraction(1)

# (wave_rows, block_rows, scratch_blocks): the hub's row of 8 by a wavefront, by a workgroup's LDS table, by the dense scratch
GEOMETRIES = {"wave": (128, 2048, 0), "workgroup": (1, 2048, 0), "scratch": (1, 2, 1)}


def _dev(x, dtype):
    return torch.tensor(np.asarray(x), device=DEV, dtype=dtype)


class Star:
    """The graph (or the graph without the edges in ``without``) and the singleton state on the WHOLE graph: deg, tot and M do not
    follow ``without``, so that a row that loses an entry is scored like the row that skips it."""

    def __init__(self, without=()):
        whole = csr_of(N, EDGES)
        self.rowptr, self.col, self.w = csr_of(N, [e for e in EDGES if e not in without])
        self.row = R._rows(self.rowptr)
        self.deg = np.diff(whole[0]).astype(np.int64)          # unit weights
        self.M = int(whole[2].sum())
        self.ident = np.arange(N, dtype=np.int32)
        self.size = np.ones(N, np.int32)
        self.totP = np.zeros(N, np.int64)
        np.add.at(self.totP, P_OF, self.deg)
        self.ext, self.kinP = L.boundary(R._rows(whole[0]), whole[1], whole[2], P_OF, self.ident)


def _heavy(star, wave_rows):
    return _dev(np.flatnonzero(np.diff(star.rowptr) > wave_rows), torch.int32)


def louvain(star, comm, geometry, sweep=0):
    """One launch: ``(next, gain, status word)``; the scratch is checked to be zero again."""
    wave_rows, block_rows, blocks = geometry
    dev, stream = torch.device(DEV), _stream(torch.device(DEV))
    rowptr, col, w = _dev(star.rowptr, torch.int64), _dev(star.col, torch.int32), _dev(star.w, torch.int32)
    comm_d, deg, size = _dev(comm, torch.int32), _dev(star.deg, torch.int64), _dev(star.size, torch.int32)
    heavy = _heavy(star, wave_rows)
    ws = torch.zeros(max(N * blocks, 1), dtype=torch.int32, device=dev)
    nxt, gain = torch.full((N,), -7, dtype=torch.int32, device=dev), torch.full((N,), -7, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.run(dev, "wgnn_louvain_sweep", _ptr(rowptr), _ptr(col), _ptr(w), N, len(star.col), _ptr(comm_d), _ptr(deg), _ptr(deg),
             _ptr(size), star.M * FRAC.denominator, FRAC.numerator, sweep, _ptr(heavy) if len(heavy) else None, len(heavy),
             wave_rows, block_rows, _ptr(nxt), _ptr(gain), _ptr(stats), _ptr(ws) if blocks else None, N * blocks * 4, blocks, 0,
             stream)
    assert not ws.any()                                        # (f) zero after every row
    stats = stats.tolist()
    assert stats[:3] == [0, 0, 0]
    return nxt.cpu().numpy(), gain.cpu().numpy(), stats[3]


def leiden(star, ref, geometry, sweep=0):
    """One launch: ``(prop, gain, status word)``; the scratch is checked to be zero again."""
    wave_rows, block_rows, blocks = geometry
    dev, stream = torch.device(DEV), _stream(torch.device(DEV))
    rowptr, col, w = _dev(star.rowptr, torch.int64), _dev(star.col, torch.int32), _dev(star.w, torch.int32)
    P, ref_d, size = _dev(P_OF, torch.int32), _dev(ref, torch.int32), _dev(star.size, torch.int32)
    deg, totP = _dev(star.deg, torch.int64), _dev(star.totP, torch.int64)
    ext, kinP = _dev(star.ext, torch.int64), _dev(star.kinP, torch.int64)
    heavy = _heavy(star, wave_rows)
    ws = torch.zeros(max(N * blocks, 1), dtype=torch.int32, device=dev)
    prop, gain = torch.full((N,), -7, dtype=torch.int32, device=dev), torch.full((N,), -7, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.run(dev, "wgnn_leiden_refine_sweep", _ptr(rowptr), _ptr(col), _ptr(w), N, len(star.col), _ptr(P), _ptr(ref_d), _ptr(deg),
             _ptr(totP), _ptr(deg), _ptr(size), _ptr(ext), _ptr(kinP), star.M * FRAC.denominator, FRAC.numerator, sweep,
             _ptr(heavy) if len(heavy) else None, len(heavy), wave_rows, block_rows, _ptr(prop), _ptr(gain), _ptr(stats),
             _ptr(ws) if blocks else None, N * blocks * 4, blocks, 0, stream)
    assert not ws.any()                                        # (f) zero after every row
    stats = stats.tolist()
    assert stats[:3] == [0, 0, 0]
    return prop.cpu().numpy(), gain.cpu().numpy(), stats[3]


KERNELS = {"louvain": (louvain, _lib.LOUVAIN_BAD_LABEL), "leiden": (leiden, _lib.LEIDEN_BAD_PARTITION)}


def _on_every_route(launch, star, label, sweep=0):
    """``{route: (label out, gain)}`` and the one status word, after checking that the routes agree on every vertex."""
    out = {name: launch(star, label, geometry, sweep) for name, geometry in GEOMETRIES.items()}
    first = out["wave"]
    for name, (lab, gain, status) in out.items():
        np.testing.assert_array_equal(lab, first[0], err_msg=name)
        np.testing.assert_array_equal(gain, first[1], err_msg=name)
        assert status == first[2], name
    return first


def test_the_graph_sends_the_hub_down_each_route():
    lens = np.diff(Star().rowptr)
    assert lens[HUB] == 8 and lens[ALONE] == 0 and sorted(lens[LEAVES]) == [1] * 6 + [2] * 2
    for name, (wave_rows, block_rows, blocks) in GEOMETRIES.items():
        route = "wave" if lens[HUB] <= wave_rows else "workgroup" if lens[HUB] <= block_rows else "scratch"
        assert route == name and (blocks > 0) == (route == "scratch")


@pytest.mark.parametrize("sweep", [0, 1])
def test_a_well_formed_state_on_every_route(sweep):
    """(a): the three routes agree, no status bit, and the values are the restatements'.  On sweep 0 the hub joins leaf 2, the
    lowest id among the six leaves of degree 1: score 1 * 20 - 8 * 1 = 12 against 4 for the leaves of degree 2."""
    star = Star()
    nxt, gain, status = _on_every_route(louvain, star, star.ident, sweep)
    want = R.sweep(star.row, star.col, star.w, star.ident, star.deg, star.deg, star.size.astype(np.int64), star.M, FRAC, sweep)
    assert status == 0
    np.testing.assert_array_equal(nxt, want[0])
    np.testing.assert_array_equal(gain, want[1])
    prop, pgain, status = _on_every_route(leiden, star, star.ident, sweep)
    want = L.refine_sweep(star.row, star.col, star.w, P_OF, star.ident, star.deg, star.totP, star.deg, star.size, star.ext, star.kinP,
                          star.M, FRAC, sweep)
    assert status == 0
    np.testing.assert_array_equal(prop, want[0])
    np.testing.assert_array_equal(pgain, want[1])
    if sweep == 0:
        assert (nxt[HUB], gain[HUB], prop[HUB], pgain[HUB]) == (2, 12, 2, 12) and nxt[1] == 0 and nxt[9] == 8
    assert (nxt[ALONE], gain[ALONE], prop[ALONE], pgain[ALONE]) == (ALONE, 0, ALONE, 0)


@pytest.mark.parametrize("kernel", ["louvain", "leiden"])
def test_a_hub_whose_label_is_no_id_stays(kernel):
    """(b): the hub keeps the label with gain 0 and exactly one status bit; its neighbours see a label that is no id, which adds
    nothing and is not theirs to report - every other vertex is the same on the three routes."""
    launch, bit = KERNELS[kernel]
    star = Star()
    for sweep in (0, 1):
        label = star.ident.copy()
        label[HUB] = N
        out, gain, status = _on_every_route(launch, star, label, sweep)
        assert status == bit and (out[HUB], gain[HUB]) == (N, 0)
        assert all(out[leaf] in (leaf, 0, 1) for leaf in LEAVES)          # no leaf joined the hub's label


@pytest.mark.parametrize("kernel", ["louvain", "leiden"])
def test_a_leaf_whose_label_is_no_id_adds_nothing_to_the_hub(kernel):
    """(c): leaf 2, the hub's choice in (a), labelled -1: the leaf stays and is reported, and the hub sees what it sees on the
    graph without that edge (same deg, tot and M) - it joins leaf 3."""
    launch, bit = KERNELS[kernel]
    star, without = Star(), Star(without=[(2, HUB)])
    label = star.ident.copy()
    label[2] = -1
    out, gain, status = _on_every_route(launch, star, label)
    assert status == bit and (out[2], gain[2]) == (-1, 0)
    for name, geometry in GEOMETRIES.items():
        want, want_gain, clean = launch(without, star.ident, geometry)
        assert clean == 0 and (out[HUB], gain[HUB]) == (want[HUB], want_gain[HUB]) == (3, 12), name


@pytest.mark.parametrize("kernel", ["louvain", "leiden"])
def test_a_long_row_without_scratch_is_a_status_bit(kernel):
    """(d): the hub's row is above block_rows and there is no scratch: WGNN_LOUVAIN_NO_SCRATCH, and the hub stays."""
    launch, _ = KERNELS[kernel]
    star = Star()
    out, gain, status = launch(star, star.ident, (1, 2, 0))
    assert status == _lib.LOUVAIN_NO_SCRATCH and (out[HUB], gain[HUB]) == (HUB, 0)
    served = launch(star, star.ident, GEOMETRIES["scratch"])
    others = np.arange(N) != HUB
    np.testing.assert_array_equal(out[others], served[0][others])
    np.testing.assert_array_equal(gain[others], served[1][others])


@pytest.mark.parametrize("kernel", ["louvain", "leiden"])
@pytest.mark.parametrize("value", [N, -1, 2 ** 31 - 1])
def test_a_vertex_without_an_edge_keeps_any_label(kernel, value):
    """(e): nothing is read for an empty row, so a label that is no id is kept with gain 0 and sets no bit."""
    launch, _ = KERNELS[kernel]
    star = Star()
    label = star.ident.copy()
    label[ALONE] = value
    out, gain, status = _on_every_route(launch, star, label)
    assert status == 0 and (out[ALONE], gain[ALONE]) == (value, 0)
    clean = launch(star, star.ident, GEOMETRIES["wave"])
    others = np.arange(N) != ALONE
    np.testing.assert_array_equal(out[others], clean[0][others])
    np.testing.assert_array_equal(gain[others], clean[1][others])
