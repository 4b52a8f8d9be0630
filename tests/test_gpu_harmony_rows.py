"""The Harmony kernels (``wgnn_harmony.hip``) and ``ops.harmony_rows`` on the GPU against the numpy restatement
(tests/harmony_reference.py).  Bit for bit wherever no ``exp`` / ``pow`` / ``log`` takes part: the dot products and distances, the
weighted grouped sums, the correction and the unit rows, the block tables given ``R``, and ``R`` itself given the device's
penalty table.  Where one of the three functions takes part the bound is derived in DESIGN.md (section 3, "Harmony") from their
documented errors - at most 1 ulp on either side - and the measured figure is printed before it is gated:

    e      2 ulp                 (one ``exp`` of identical arguments on either side)
    pen    2 ulp                 (one ``pow`` of identical arguments)
    R      (K + 6) * 2^-52       relative, given the same ``e``: a ``pow``, a product, a K-term sum and a quotient
    objective  (K + 256 + n_chunks + 8) * 2^-52 of the sum of the terms' magnitudes

Every output is dense (its row stride is its width), so a guard COLUMN cannot exist: the outputs are views into larger buffers
with guard elements in front and behind, and a write past a row's end lands in the next row, which is compared."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import WgnnError, ops

import harmony_reference as hr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -52
GUARD = 64


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def _same(got, want):
    np.testing.assert_array_equal(_bits(got.cpu().numpy() if isinstance(got, torch.Tensor) else got), _bits(want))


def _guarded(*shape):
    """A float64 output inside a larger buffer, and the check that nothing around it was written."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)

    def untouched():
        host = buf.cpu().numpy()
        return (host[:GUARD] == -7).all() and (host[-GUARD:] == -7).all()
    return buf[GUARD:GUARD + n].view(*shape), untouched


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want))) if want.size else 0.0


def _batches(B, S, rng):
    """One id per row; from three batches on (and enough rows) batch 1 holds ONE cell and the last batch none."""
    b = rng.integers(0, S, B)
    if S >= 3 and B >= 19:
        b[b == S - 1] = 0
        b[b == 1] = 2 % (S - 1)
        b[B // 2] = 1
    return b.astype(np.int32)


def _soft(B, K, rng):
    R = rng.random((B, K)) ** 4
    return R / R.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------ weighted_group_reduce and harmony_apply
SHAPES = [(1, 1, 1, 4), (19, 2, 2, 8), (255, 7, 3, 197), (256, 100, 1, 8), (257, 7, 64, 4), (1000, 256, 3, 256), (1000, 7, 64, 8)]


@pytest.mark.parametrize("B, K, S, D", SHAPES)
def test_reduce_and_apply_restate_numpy_bit_for_bit(B, K, S, D):
    rng = np.random.default_rng(B + K + S + D)
    X, R, b = rng.normal(size=(B, D)) + 0.5, _soft(B, K, rng), _batches(B, S, rng)
    if S >= 3 and B >= 19:
        assert (b == 1).sum() == 1 and (b == S - 1).sum() == 0
    want_M, want_n = hr.weighted_group_reduce(X, R, b, S)
    W = hr.ridge(want_M, want_n, 1.0)
    want_Zc, want_U = hr.apply(X, R, W, b)
    Xd, Rd, bd, Wd = _dev(X), _dev(R), _dev(b), _dev(W)
    for grid in (0, 1, 7):
        (M, M_ok), (n, n_ok) = _guarded(K, S, D), _guarded(K, S)
        ops.weighted_group_reduce(Xd, Rd, bd, S, out=(M, n), grid_blocks=grid)
        _same(M, want_M), _same(n, want_n)
        assert M_ok() and n_ok()
        (Zc, Zc_ok), (U, U_ok) = _guarded(B, D), _guarded(B, D)
        ops.harmony_apply(Xd, Rd, Wd, bd, out=(Zc, U), grid_blocks=grid)
        _same(Zc, want_Zc), _same(U, want_U)
        assert Zc_ok() and U_ok()
    _same(ops.harmony_ridge(_dev(want_M), _dev(want_n), 1.0), W)       # the framework operations of the ridge step
    if S == 1:                                                         # the centres: no group vector, and int64 ids do the same
        _same(ops.weighted_group_reduce(Xd, Rd, None, 1)[0], want_M)
    _same(ops.weighted_group_reduce(Xd, Rd, bd.long(), S)[0], want_M)
    (U, U_ok) = _guarded(B, D)
    same_rows, U = ops.harmony_apply(Xd, out=(Xd, U))                  # without R: the unit rows alone
    _same(U, hr.unit(X))
    assert same_rows is Xd and U_ok()


def test_reduce_leaves_out_ids_outside_the_groups():
    rng = np.random.default_rng(3)
    X, R = rng.normal(size=(300, 8)), _soft(300, 5, rng)
    g = rng.integers(-1, 4, 300)
    g[7] = 9
    want_M, want_n = hr.weighted_group_reduce(X, R, g, 3)              # 3 (= S), -1 and 9 take no part
    M, n = ops.weighted_group_reduce(_dev(X), _dev(R), _dev(g), 3)
    _same(M, want_M), _same(n, want_n)


# ------------------------------------------------------------------------------------------------------ harmony_scores
@pytest.mark.parametrize("B, K, D", [(1, 1, 4), (257, 7, 197), (1000, 100, 8), (300, 256, 256), (65, 65, 33)])
def test_scores(B, K, D):
    rng = np.random.default_rng(B + K + D)
    U, Y = hr.unit(rng.normal(size=(B, D)) + 0.3), hr.unit(rng.normal(size=(K, D)) + 0.3)
    want_dot, want_dist, want_e = hr.scores(U, Y, 0.1)
    dot, dist, e = ops.harmony_scores(_dev(U), _dev(Y), 0.1, want_dot=True)
    _same(dot, want_dot), _same(dist, want_dist)
    e = e.cpu().numpy()
    err = _rel(e, want_e) / ULP
    print(f"HARMONY-FIGURE scores B={B} K={K} D={D}: e differs by at most {err:.3f} * 2^-52 relative (bound 2)")
    assert err <= 2.0 and (e.max(axis=1) == 1.0).all() and (e > 0).all()
    again = ops.harmony_scores(_dev(U), _dev(Y), 0.1)
    assert again[0] is None and torch.equal(again[1], dist) and np.array_equal(_bits(again[2].cpu().numpy()), _bits(e))


# ---------------------------------------------------------------------------------- harmony_assign_block and the fold
class _State:
    """A clustering state in numpy: ``e``, ``R`` and ``T`` as a restatement run holds them after its first sweep."""

    def __init__(self, U, Y, batch, S, theta, n_blocks, e=None):
        self.batch, self.S, self.n_blocks = batch.astype(np.int64), S, n_blocks
        self.theta = np.full(S, float(theta))
        (self.B, _), self.K = U.shape, Y.shape[0]
        self.Pr = np.bincount(self.batch, minlength=S) / float(self.B)
        _, self.dist, self.e = hr.scores(U, Y, 0.1)
        if e is not None:
            self.e = e
        self.R, self.T = np.zeros((self.B, self.K)), np.zeros((n_blocks, self.K, S))
        hr.sweep(self.R, self.T, self.e, self.batch, self.Pr, self.theta, n_blocks, first=True)


def _step(st, q, grid=0):
    """Block ``q`` on the device from the state ``st``, every piece against the restatement; ``st`` then takes the DEVICE's
    rows and table, so that the next step starts from identical bits.  Returns the measured (pen, R) errors in 2^-52."""
    B, K, S = st.B, st.K, st.S
    mem = hr.members_of(q, B, st.n_blocks)
    T_d, R_d, Pr_d, th_d = _dev(st.T), _dev(st.R), _dev(st.Pr), _dev(st.theta)
    e_d, b_d = _dev(st.e), _dev(st.batch.astype(np.int32))
    O_, E_, pen = ops.harmony_fold(T_d, Pr_d, th_d, B, q_skip=q)
    want_O = hr.tables_sum(st.T, skip=q)
    want_E = hr.expected(want_O, st.Pr)
    _same(O_, want_O), _same(E_, want_E)
    want_pen, pen_h = hr.penalty(want_O, want_E, st.theta), pen.cpu().numpy()
    pen_err = _rel(pen_h, want_pen) / ULP
    ws = ops.harmony_assign_block(e_d, b_d, S, st.n_blocks, q, R_d, pen=pen, grid_blocks=grid)
    got = R_d.cpu().numpy()
    rest = np.setdiff1d(np.arange(B), mem)
    np.testing.assert_array_equal(_bits(got[rest]), _bits(st.R[rest]))             # no other row is written
    r_err = 0.0
    if len(mem):
        _same(got[mem], hr.assign_rows(st.e[mem], pen_h[:, st.batch[mem]].T))       # given the device's pen: no pow, bit for bit
        r_err = _rel(got[mem], hr.assign_rows(st.e[mem], want_pen[:, st.batch[mem]].T)) / ULP
        assert np.abs(hr.seq_sum(got[mem], 1) - 1).max() <= K * ULP
    O_all, E_all, none = ops.harmony_fold(T_d, Pr_d, None, B, q_store=q, workspace=ws, want_pen=False)
    T_new = st.T.copy()
    T_new[q] = hr.block_table(got, st.batch, mem, S)
    _same(T_d, T_new)                                                               # T[q] retaken, the other tables untouched
    _same(O_all, hr.tables_sum(T_new)), _same(E_all, hr.expected(hr.tables_sum(T_new), st.Pr))
    assert none is None and pen_err <= 2.0 and r_err <= K + 6, (q, pen_err, r_err)
    st.R, st.T = got, T_new
    return pen_err, r_err


@pytest.fixture(scope="module")
def cohorts():
    """The 260-cell and the 1 000-cell cohort, with the device's own seeding: ``(x, batch, cell_type, centers)``."""
    out = {}
    for n in (260, 1000):
        x, batch, cell_type = hr.cohort(1, n)
        U = ops.harmony_apply(_dev(x).double())[1]
        centers = ops.kmeans_rows(U.float(), ops.harmony_default_clusters(n), seed=0, max_iter=25).centers
        out[n] = (x, batch, cell_type, centers.cpu().numpy())
    return out


def test_a_whole_sweep_step_by_step(cohorts):
    x, batch, _, centers = cohorts[260]
    st = _State(hr.unit(x.astype(np.float64)), hr.unit(centers.astype(np.float64)), batch, 3, 2.0, 20)
    errs = np.asarray([_step(st, q) for q in range(20)])
    print(f"HARMONY-FIGURE sweep B=260 K={st.K}: pen differs by at most {errs[:, 0].max():.3f}, R by at most "
          f"{errs[:, 1].max():.3f} * 2^-52 relative (bounds 2 and {st.K + 6})")
    R_dev, T_dev = st.R.copy(), st.T.copy()
    ref = _State(hr.unit(x.astype(np.float64)), hr.unit(centers.astype(np.float64)), batch, 3, 2.0, 20)
    hr.sweep(ref.R, ref.T, ref.e, ref.batch, ref.Pr, ref.theta, 20)    # the restatement on its own: errors may add up here
    print(f"HARMONY-FIGURE sweep B=260: after the sweep R differs from the free-running restatement by at most "
          f"{np.abs(R_dev - ref.R).max():.3e} absolute, T by {np.abs(T_dev - ref.T).max():.3e}")


@pytest.mark.parametrize("B, K, S, n_blocks", [(1000, 33, 3, 20), (19, 2, 2, 20), (300, 256, 64, 3), (257, 7, 3, 1), (700, 100, 5, 64)])
def test_blocks_from_the_middle_of_a_run(B, K, S, n_blocks):
    rng = np.random.default_rng(B + K)
    x = rng.normal(size=(B, 8)) + 1.0
    U = hr.unit(x)
    st = _State(U, hr.unit(U[rng.choice(B, K, replace=B < K)] + 0.01 * rng.normal(size=(K, 8))), _batches(B, S, rng), S, 2.0, n_blocks)
    for q in range(min(3, n_blocks)):                                  # the middle of a run: a few blocks already re-assigned
        _step(st, q)
    worst = np.zeros(2)
    for q, grid in zip(sorted({0, min(7, n_blocks - 1), n_blocks - 1}), (1, 7, 0)):
        worst = np.maximum(worst, _step(st, q, grid))
    print(f"HARMONY-FIGURE blocks B={B} K={K} S={S} n_blocks={n_blocks}: pen {worst[0]:.3f}, R {worst[1]:.3f} * 2^-52 "
          f"(bounds 2 and {K + 6})")


def test_the_first_assignment_is_the_plain_softmax():
    rng = np.random.default_rng(0)
    B, K, S = 130, 7, 3
    e, b = rng.random((B, K)) + 1e-3, _batches(B, S, rng)
    R = torch.full((B, K), -7.0, dtype=torch.float64, device=DEV)
    for q in range(20):
        ops.harmony_assign_block(_dev(e), _dev(b), S, 20, q, R)
    _same(R, hr.assign_rows(e, np.ones((B, K))))


# --------------------------------------------------------------------------------------------------- harmony_objective
@pytest.mark.parametrize("B, K, S", [(1, 1, 1), (257, 7, 3), (1000, 33, 64), (700, 256, 2)])
def test_objective(B, K, S):
    rng = np.random.default_rng(B + K + S)
    R, dist, b = _soft(B, K, rng), 4.0 * rng.random((B, K)), _batches(B, S, rng)
    R[rng.random((B, K)) < 0.05] = 0.0                                 # 0 log 0 = 0
    theta = np.linspace(0.0, 2.0, S)
    O = R.T @ np.eye(S)[b]
    E = hr.expected(O, np.bincount(b, minlength=S) / float(B))
    want, terms = hr.objective(R, dist, b, O, E, theta, 0.1)
    got = ops.harmony_objective(_dev(R), _dev(dist), _dev(b), _dev(O), _dev(E), _dev(theta), 0.1).cpu().numpy()
    _same(got[1], terms[0])                                            # sum R dist: no log in it
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.asarray([np.abs(R * dist).sum(), np.abs(np.where(R > 0, R * np.log(R), 0.0)).sum(),
                          np.abs(R * (theta[b][:, None] * np.log((O + 1) / (E + 1))[:, b].T)).sum()])
    c = K + 256 + -(-B // 256) + 8
    errs = np.abs(got[1:] - terms) / np.maximum(mag, np.finfo(float).tiny) / ULP
    total = abs(got[0] - want) / (mag[0] + 0.1 * mag[1] + 0.1 * mag[2]) / ULP
    print(f"HARMONY-FIGURE objective B={B} K={K} S={S}: the sums differ by {errs[1]:.3f} and {errs[2]:.3f}, the value by "
          f"{total:.3f} * 2^-52 of the terms' magnitudes (bound {c})")
    assert (errs <= c).all() and total <= c + 2
    assert got[0] == (got[1] + 0.1 * got[2]) + 0.1 * got[3]


# ----------------------------------------------------------------------------------------------------------- whole runs
FIXED = dict(max_iter=2, max_iter_cluster=3, epsilon=0.0, epsilon_cluster=0.0)


@pytest.mark.parametrize("n", [260, 1000])
def test_whole_runs_are_deterministic_and_mix_the_samples(cohorts, n):
    x, batch, cell_type, centers = cohorts[n]
    runs = [ops.harmony_rows(_dev(x), _dev(batch), 3, **FIXED) for _ in range(2)]
    for name in ("coords", "R", "centers", "O", "E"):
        assert torch.equal(getattr(runs[0], name), getattr(runs[1], name)), name
    assert runs[0][5:] == runs[1][5:] and runs[0].inner_iters == [3] * runs[0].n_iter and 1 <= runs[0].n_iter <= 2
    ref = hr.harmony(x, batch, 3, centers, **FIXED)
    coords = runs[0].coords.cpu().numpy()
    assert runs[0].n_iter == ref["n_iter"]
    print(f"HARMONY-FIGURE run B={n}: coords differ from the restatement by at most {np.abs(coords - ref['coords']).max():.3e} "
          f"absolute (largest coordinate {np.abs(coords).max():.3f}), R by {np.abs(runs[0].R.cpu().numpy() - ref['R']).max():.3e}, "
          f"the last objective by {abs(runs[0].objective[-1] - ref['objective'][-1]):.3e} of {ref['objective'][-1]:.6f}")
    before = hr.mixing(x.astype(np.float64), batch, cell_type)
    after = hr.mixing(coords, batch, cell_type)
    wanted = hr.mixing(ref["coords"], batch, cell_type)
    print(f"HARMONY-FIGURE run B={n}: batch LISI {before[0]:.3f} -> {after[0]:.3f} (restatement {wanted[0]:.3f}), type LISI "
          f"{before[1]:.3f} -> {after[1]:.3f} (restatement {wanted[1]:.3f})")
    assert before[0] <= 1.05 and after[0] >= 1.5 and after[1] - before[1] <= 0.05
    assert wanted[0] >= 1.5 and wanted[1] - before[1] <= 0.05
    assert np.abs(runs[0].R.sum(dim=1).cpu().numpy() - 1).max() <= runs[0].R.shape[1] * ULP


def test_one_batch_returns_the_input_bits(cohorts):
    x = cohorts[260][0]
    run = ops.harmony_rows(_dev(x), torch.zeros(260, dtype=torch.int64, device=DEV), 1)
    _same(run.coords, x.astype(np.float64))
    assert run.n_iter == 0 and run.converged and run.R is None


def test_theta_zero_keeps_the_restatements_clusters(cohorts):
    x, _, cell_type, centers = cohorts[260]                            # one batch per type: the batch is the biology
    run = ops.harmony_rows(_dev(x), _dev(cell_type), 3, theta=0.0, **FIXED)
    ref = hr.harmony(x, cell_type, 3, centers, theta=0.0, **FIXED)
    assert np.array_equal(run.R.argmax(dim=1).cpu().numpy(), ref["R"].argmax(axis=1))
    assert run.n_iter == ref["n_iter"]


def test_refusals(cohorts):
    x, batch = _dev(cohorts[260][0]), _dev(cohorts[260][1])
    bad = x.clone()
    bad[3, 2], bad[9, 0] = float("nan"), float("inf")
    with pytest.raises(ValueError, match="2 of the 260 rows hold a non-finite value"):
        ops.harmony_rows(bad, batch, 3)
    bad = x.clone()
    bad[5] = 0
    with pytest.raises(ValueError, match="1 of the 260 rows have a zero norm"):
        ops.harmony_rows(bad, batch, 3)
    for ids in (batch.clone().index_fill_(0, torch.tensor([4], device=DEV), 3), batch - 1):
        with pytest.raises(ValueError, match="batch id out of range"):
            ops.harmony_rows(x, ids, 3)
    with pytest.raises(ValueError, match="n_clusters = 257"):
        ops.harmony_rows(x, batch, 3, n_clusters=257)
    with pytest.raises(WgnnError, match="GPU only"):
        ops.harmony_rows(x.cpu(), batch.cpu(), 3)
    run = ops.harmony_rows(x, batch, 4, **FIXED)                       # an empty batch is allowed
    assert bool(torch.isfinite(run.coords).all()) and float(run.O[:, 3].abs().max()) == 0.0
