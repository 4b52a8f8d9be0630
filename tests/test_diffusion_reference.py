"""The numpy restatement of the diffusion map (tests/diffusion_reference.py) against independent float64 linear algebra, without
a GPU: the Ritz values of a path against the dense ``eigh``, the breakdown on a complete graph, and on two kNN fixtures every
component's TRUE residual (a scipy product), its distance to ``eigsh``'s eigenvalues by the residual bound of a symmetric matrix,
and the order diffusion pseudotime gives a noisy arc.  tests/test_gpu_diffusion_rows.py holds the device to the restatement with
no tolerance, so these bounds carry over to it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import eigsh

import diffusion_reference as R

EPS = np.finfo(np.float64).eps
TOL = 1e-8


def _dense(rowptr, col, t):
    n = len(rowptr) - 1
    return sp.csr_matrix((t, np.asarray(col, np.int64), np.asarray(rowptr, np.int64)), shape=(n, n))


def test_the_ritz_values_of_a_path_equal_the_dense_eigenvalues():
    rowptr, col, w = R.path_graph(5)
    op = R.diffusion_operator(rowptr, col, w)
    run = R.lanczos_graph(rowptr, col, op.t, op.z, np.ones(5, bool), n_steps=4)
    # four steps span the whole complement of v_0: the last norm is rounding error, which the rule reports as a breakdown
    assert (run.n_run, run.breakdown, run.n_cells) == (4, True, 5) and run.V.shape == (5, 5) and run.beta[3] <= R.BREAKDOWN
    assert (run.beta[:3] > 0.1).all()
    theta, _, _ = R.lanczos_ritz(run.alpha, run.beta, 4)
    want = np.linalg.eigh(_dense(rowptr, col, op.t).toarray())[0][::-1]
    print("path Ritz values", theta, "dense", want)
    assert abs(want[0] - 1.0) <= 64 * EPS
    assert np.abs(theta - want[1:]).max() <= 64 * EPS
    np.testing.assert_allclose(theta, [np.sqrt(2.0 / 3.0), 0.0, -np.sqrt(2.0 / 3.0), -1.0], atol=64 * EPS)
    # the clip: more steps than the component has directions run n_c - 1 of them
    assert R.lanczos_graph(rowptr, col, op.t, op.z, np.ones(5, bool), n_steps=32).n_run == 4


def test_a_complete_graph_breaks_down_after_one_step():
    rowptr, col, w = R.complete_graph(8)
    op = R.diffusion_operator(rowptr, col, w)
    run = R.lanczos_graph(rowptr, col, op.t, op.z, np.ones(8, bool), n_steps=7)
    print("complete graph beta_1", run.beta[0])
    assert (run.n_run, run.breakdown) == (1, True) and run.beta[0] <= R.BREAKDOWN and (run.V[2:] == 0).all()
    theta, _, _ = R.lanczos_ritz(run.alpha, run.beta, run.n_run)
    assert theta.shape == (1,) and abs(theta[0] + 1.0 / 7.0) <= 64 * EPS
    dm = R.diffmap(rowptr, col, w, n_comps=15, n_steps=7)
    assert dm.Y.shape == (8, 2) and len(dm.eigenvalues) == len(dm.residual) == 2 and dm.eigenvalues[0] == 1.0


def test_the_operator_is_symmetric_in_bits_and_keeps_zero_weights():
    rowptr, col, w = R.hand_graph()
    op = R.diffusion_operator(rowptr, col, w)
    T = _dense(rowptr, col, op.t)
    assert (T != T.T).nnz == 0
    assert op.q[7] == 0 and op.z[7] == 0                               # the isolated vertex
    assert (op.t[np.asarray(w) == 0] == 0).all() and (op.t[np.asarray(w) > 0] > 0).all() and np.isfinite(op.t).all()
    assert np.abs(T @ op.z - op.z).max() <= 8 * EPS                     # z is the eigenvector of eigenvalue 1


@functools.lru_cache(maxsize=None)
def _fixture(name):
    if name == "arc":
        s, g = R.arc()
    else:
        s, g = None, R.blob_cells()
    return s, g, R.diffmap(g.rowptr, g.col, g.w, n_comps=16, n_steps=128)


@pytest.mark.parametrize("name", ["arc", "blobs"])
def test_every_component_meets_the_residual_bound(name):
    _, g, dm = _fixture(name)
    on = dm.mask
    assert on.sum() >= 400 and dm.Y.shape[1] == 16 and not dm.run.breakdown and dm.run.n_run == 128
    T = _dense(g.rowptr, g.col, dm.op.t)[on][:, on]
    Y = dm.Y[on]
    assert (dm.Y[~on] == 0).all()
    rounding = (int(np.diff(g.rowptr).max()) + 2) * EPS
    assert np.abs(T @ Y[:, 0] - Y[:, 0]).max() <= rounding              # T v_0 = v_0
    lam = eigsh(T, k=16, which="LA", tol=0)[0]
    rho = np.array([np.linalg.norm(T @ Y[:, c] - dm.eigenvalues[c] * Y[:, c]) for c in range(16)])
    gap = np.array([np.abs(lam - dm.eigenvalues[c]).min() for c in range(16)])
    print(name, "cells", int(on.sum()), "largest true residual", rho.max(), "largest estimate", dm.residual.max(),
          "largest gap to eigsh", gap.max())
    assert rho.max() <= TOL and dm.residual.max() <= TOL
    assert (gap <= rho + rounding).all()
    assert (np.diff(dm.eigenvalues) <= 0).all() and dm.eigenvalues[0] == 1.0 and dm.residual[0] == 0.0
    first = np.abs(dm.Y[:, 1:]).argmax(axis=0)
    assert (dm.Y[first, np.arange(1, 16)] > 0).all()                    # the sign convention


@pytest.mark.parametrize("n_dcs", [10, 15])
def test_dpt_orders_the_arc(n_dcs):
    s, _, dm = _fixture("arc")
    assert dm.mask.all()
    d = R.diffusion_distance(dm.Y[:, :n_dcs], R.diffusion_weights(dm.eigenvalues[:n_dcs]), 0)
    rho = R.spearman(d, s)
    print("arc: Spearman of DPT from cell 0 with the arc parameter, n_dcs =", n_dcs, ":", rho)
    assert d[0] == 0 and np.isfinite(d).all() and rho >= 0.99
    two = R.diffusion_distance(dm.Y[:, :n_dcs], R.diffusion_weights(dm.eigenvalues[:n_dcs]), [0, 799])
    assert (two <= d).all() and two[799] == 0
