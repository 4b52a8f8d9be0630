"""The numpy restatement of Harmony (tests/harmony_reference.py) against independent float64 algebra, without a GPU: the closed
form of the ridge system against ``numpy.linalg.solve`` of harmonypy's full system, the assignment with ``theta = 0`` against a
plain softmax, the block tables against one matrix product, and what the whole call does to a cohort whose samples were moved
apart - read with ``NeighborGraph.lisi``.  And the argument refusals of ``ops.harmony_rows`` that need no device."""
import numpy as np
import pytest
import torch

import harmony_reference as hr
from scdeepsort_amd import ops

COHORT_SEED = 1


def _state(B, K, S, D, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, D)) + 1.0
    batch = rng.integers(0, S, B)
    R = rng.random((B, K))
    R /= R.sum(axis=1, keepdims=True)
    return x, batch, R


@pytest.mark.parametrize("S", [1, 2, 5, 64])
def test_the_closed_form_ridge_solves_the_full_system(S):
    K, D = 4, 6
    x, batch, R = _state(300, K, S, D, seed=S)
    if S > 1:
        batch[batch == S - 1] = 0                                      # a batch without a cell: n_ks = 0
    M, n = hr.weighted_group_reduce(x, R, batch, S)
    assert S == 1 or (n[:, S - 1] == 0).all()
    for lamb in (1.0, 0.3):
        W, full = hr.ridge(M, n, lamb), hr.ridge_full(M, n, lamb)
        scale = np.abs(M / (n[:, :, None] + lamb)).max()               # the terms W is a difference of (W itself is 0 at S = 1)
        assert np.abs(W - full).max() <= 1e-12 * scale
    assert S > 1 or np.abs(hr.ridge(M, n, 1.0)).max() <= 1e-12 * np.abs(M).max()      # one batch: no offset at all


def test_theta_zero_is_the_plain_softmax():
    B, K, S, D = 130, 7, 3, 8
    x, batch, _ = _state(B, K, S, D)
    U, Y = hr.unit(x), hr.unit(x[:K])
    _, dist, e = hr.scores(U, Y, 0.1)
    Pr = np.bincount(batch, minlength=S) / B
    R, T = np.zeros((B, K)), np.zeros((20, K, S))
    hr.sweep(R, T, e, batch, Pr, np.zeros(S), 20, first=True)
    first = R.copy()
    hr.sweep(R, T, e, batch, Pr, np.zeros(S), 20)                      # pen = pow(., 0) = 1
    assert np.array_equal(R, first)
    a = -dist / 0.1
    soft = np.exp(a - a.max(axis=1, keepdims=True))
    soft /= soft.sum(axis=1, keepdims=True)
    assert np.abs(R - soft).max() <= 8 * K * 2.0 ** -52
    assert np.abs(R.sum(axis=1) - 1).max() <= K * 2.0 ** -52


def test_one_batch_returns_the_input():
    x, _, _ = _state(40, 3, 1, 8)
    x = x.astype(np.float32)
    r = hr.harmony(x, np.zeros(40, np.int64), 1, None)
    assert np.array_equal(r["coords"], x.astype(np.float64)) and r["n_iter"] == 0


@pytest.mark.parametrize("B, n_blocks", [(19, 20), (1000, 20), (257, 1), (300, 64)])
def test_the_block_tables_add_up(B, n_blocks):
    K, S = 5, 3
    _, batch, R = _state(B, K, S, 4, seed=B)
    T = np.stack([hr.block_table(R, batch, hr.members_of(q, B, n_blocks), S) for q in range(n_blocks)])
    whole = R.T @ np.eye(S)[batch]
    assert np.abs(hr.tables_sum(T) - whole).max() <= B * 2.0 ** -52 * whole.max()
    covered = np.concatenate([hr.members_of(q, B, n_blocks) for q in range(n_blocks)])
    assert np.array_equal(np.sort(covered), np.arange(B))
    for q in range(n_blocks):                                          # the sum without a block, against taking it out again
        assert np.abs(hr.tables_sum(T, skip=q) - (whole - T[q])).max() <= 2 * B * 2.0 ** -52 * whole.max()


@pytest.fixture(scope="module")
def cohort():
    x, batch, cell_type = hr.cohort(COHORT_SEED)
    K = ops.harmony_default_clusters(x.shape[0])
    run = hr.harmony(x, batch, 3, hr.seed_centers(hr.unit(x.astype(np.float64)), K, 0))
    return x, batch, cell_type, run


def test_the_cohort_is_what_the_issue_describes(cohort):
    x, batch, cell_type, _ = cohort
    assert x.shape == (260, 8) and x.dtype == np.float32
    sizes = np.bincount(batch)
    assert len(sizes) == 3 and sizes[2] * 2 == sizes[0] == sizes[1]    # one sample of half size
    assert (np.diff(batch) >= 0).all()                                 # stored sample after sample
    assert not ((batch == 1) & (cell_type == 2)).any() and ((batch == 0) & (cell_type == 2)).any()


def test_the_restatement_mixes_samples_and_keeps_types(cohort):
    x, batch, cell_type, run = cohort
    before = hr.mixing(x.astype(np.float64), batch, cell_type)
    after = hr.mixing(run["coords"], batch, cell_type)
    print("batch LISI %.3f -> %.3f, type LISI %.3f -> %.3f, %d rounds" % (before[0], after[0], before[1], after[1], run["n_iter"]))
    assert before[0] <= 1.05 and after[0] >= 1.5
    assert after[1] - before[1] <= 0.05
    assert run["converged"] and np.all(np.isfinite(run["objective_cluster"]))
    assert np.abs(run["R"].sum(axis=1) - 1).max() <= run["R"].shape[1] * 2.0 ** -52


def test_harmony_rows_refuses_bad_arguments_before_the_device():
    x, b = torch.ones(40, 8), torch.zeros(40, dtype=torch.int64)
    for kw, word in ((dict(n_clusters=257), "n_clusters"), (dict(n_clusters=0), "n_clusters"), (dict(n_clusters=41), "only 40 rows"),
                     (dict(n_batches=0), "n_batches"), (dict(n_batches=65), "n_batches"), (dict(n_blocks=0), "n_blocks"),
                     (dict(n_blocks=65), "n_blocks"), (dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(lamb=-1.0), "lamb"), (dict(theta=-0.5), "theta"), (dict(theta=[1.0, 2.0, 3.0]), "theta"),
                     (dict(epsilon=-1.0), "epsilon"), (dict(max_iter=0), "max_iter")):
        args = dict(n_batches=2, n_clusters=2)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.harmony_rows(x, b, **args)
    with pytest.raises(ValueError, match="float32"):
        ops.harmony_rows(x.double(), b, 2)
    with pytest.raises(ValueError, match="one int32 / int64 id per row"):
        ops.harmony_rows(x, b[:-1], 2)
    with pytest.raises(ValueError, match="D = 1028"):
        ops.harmony_rows(torch.ones(4, 1028), b[:4], 2, n_clusters=1)
    assert [ops.harmony_default_clusters(n) for n in (1, 14, 15, 260, 1000, 100_000)] == [1, 1, 1, 9, 33, 100]
