"""Plain numpy / Python restatement of ``wgnn_predict_rows_thin`` (include/wgnn.h): the read hash in uint64 with wrap-around,
binomial thinning of integer counts, the draw's library size and log-normalised values in fp64, then the layer, head, label
rule and tallies of tests/stability_reference.py - and the cases the CPU and GPU tests share.  Nothing here imports torch or
the package."""
import functools

import numpy as np
import scipy.sparse as sp

import stability_reference as R

M64 = R.M64
K_READ = 0xA0761D6478BD642F
STASH, COOP = 1024, 16                                           # csrc/wgnn_thin.hip: kTStash, kTCoop


# ------------------------------------------------------------------------------------------------
# the hash
# ------------------------------------------------------------------------------------------------
def mix64(x: int) -> int:
    """The splitmix64 finaliser on Python ints reduced mod 2^64, all 64 bits."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def entry_key(seed: int, cell: int, draw: int, gene: int) -> int:
    key = (seed & M64) ^ ((cell * R.K_CELL) & M64) ^ ((draw * R.K_DRAW) & M64)
    return mix64((key + gene * R.K_GENE) & M64)


def read_u(seed: int, cell: int, draw: int, gene: int, i: int) -> int:
    """The 32-bit hash of read ``i`` of the entry (cell, gene) in this draw."""
    return R.mix32((entry_key(seed, cell, draw, gene) + i * K_READ) & M64)


def _u(v):
    return np.asarray(v).astype(np.uint64)


def mix64_np(x) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = _u(x) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def entry_key_np(seed: int, cell, draw, gene) -> np.ndarray:
    with np.errstate(over="ignore"):
        key = np.uint64(seed & M64) ^ (_u(cell) * np.uint64(R.K_CELL)) ^ (_u(draw) * np.uint64(R.K_DRAW))
        return mix64_np(key + _u(gene) * np.uint64(R.K_GENE))


def kept_reads(seed: int, cell, draw, gene, count, keep: float) -> np.ndarray:
    """c' int64 per entry: the reads ``i`` in [0, count) with ``mix32(ek + i * K_READ) < T``.  Arrays broadcast to the entries."""
    cell, gene, count = (np.atleast_1d(np.asarray(a, np.int64)) for a in (cell, gene, count))
    n = max(cell.shape[0], gene.shape[0], count.shape[0])
    cell, gene, count = (np.broadcast_to(a, (n,)) for a in (cell, gene, count))
    ek = entry_key_np(seed, cell, draw, gene)
    owner = np.repeat(np.arange(n), count)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    i = np.arange(owner.shape[0], dtype=np.int64) - start[owner]
    with np.errstate(over="ignore"):
        u = mix64_np(ek[owner] + _u(i) * np.uint64(K_READ)) >> np.uint64(32)
    return np.bincount(owner, weights=(u < np.uint64(R.threshold(keep))), minlength=n).astype(np.int64)


def thin_draw(m: sp.csr_matrix, rest: np.ndarray, seed: int, draw: int, keep: float, row0: int = 0):
    """``(c' int64 per stored entry in CSR order, rest' int64 [B])`` of one draw of a batch of counts."""
    B, G = m.shape
    rows = np.repeat(np.arange(B, dtype=np.int64), np.diff(m.indptr))
    cp = kept_reads(seed, rows + row0, draw, m.indices.astype(np.int64), m.data.astype(np.int64), keep)
    rp = kept_reads(seed, np.arange(B, dtype=np.int64) + row0, draw, G, np.asarray(rest, np.int64), keep)
    return cp, rp


# ------------------------------------------------------------------------------------------------
# the draw's values and layer
# ------------------------------------------------------------------------------------------------
def lognorm(c, total, scale: float) -> np.ndarray:
    """float32(log1p(c / total * scale)) in fp64, Seurat's operation order; 0 where total is 0."""
    c, total = np.asarray(c, np.float64), np.asarray(total, np.float64)
    safe = np.where(total > 0, total, 1.0)
    return np.where(total > 0, np.log1p(c / safe * scale), 0.0).astype(np.float32)


def draw_values(m: sp.csr_matrix, cp: np.ndarray, rp: np.ndarray, scale: float, vthr: float):
    """``(values csr with v' as data, part bool per entry, total' int64 [B], deg' int64 [B])`` of one draw."""
    B = m.shape[0]
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    total = np.bincount(rows, weights=cp, minlength=B).astype(np.int64) + rp
    v = lognorm(cp, total[rows], scale)
    part = (cp > 0) & (v > np.float32(vthr))
    vals = sp.csr_matrix((v, m.indices, m.indptr), shape=m.shape)
    return vals, part, total, np.bincount(rows, weights=part, minlength=B).astype(np.int64)


def lognorm_batch(m: sp.csr_matrix, rest: np.ndarray, scale: float, vthr: float) -> sp.csr_matrix:
    """The batch as ``align_rows(..., normalize="lognorm")`` leaves it: every read kept."""
    vals, part, _, _ = draw_values(m, m.data.astype(np.int64), np.asarray(rest, np.int64), scale, vthr)
    return R.thinned(vals, part)


def materialised(m: sp.csr_matrix, cp: np.ndarray, rp: np.ndarray) -> np.ndarray:
    """One draw as a dense count matrix [B, G + 1]: the thinned counts, and one more column holding rest'."""
    x = np.zeros((m.shape[0], m.shape[1] + 1), np.float32)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    x[rows, m.indices] = cp
    x[:, -1] = rp
    return x


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
G_CASE, B_CASE = R.G_CASE, R.B_CASE
LONG_ROW = 5500                                                  # outgrows the 1024-entry stash at every level below
ROW_EMPTY, ROW_ONE, ROW_LONG, ROW_ONES, ROW_SPECIAL = 1, 2, 3, 4, 8
SPECIAL_COUNTS = (COOP - 1, COOP, COOP + 1, 1000, 70000)
REST_SPECIAL = {ROW_ONE: 0, 9: 0, 10: 1, 11: 5000, 12: 200000, ROW_EMPTY: 7}


@functools.lru_cache(maxsize=None)
def count_batch(seed: int = 0):
    """``(counts csr [40, 6000] with integer f32 data, rest int64 [40])``: the ragged shape of stability_reference's batch
    (an empty row, a one-entry row of count 1, rows of 63 / 64 / 65 entries, one row longer than the stash), a row of all
    ones, a row that starts with the counts 15, 16, 17, 1000 and 70000, geometric counts elsewhere; rest 0, 1, 5000, 200000
    on four rows, 7 on the empty row, 0 on the one-read row."""
    rng = np.random.default_rng(77_000 + seed)
    lens = rng.integers(6, 300, B_CASE)
    lens[ROW_EMPTY], lens[ROW_ONE], lens[ROW_LONG], lens[ROW_ONES] = 0, 1, LONG_ROW, 100
    lens[5], lens[6], lens[7] = 63, 64, 65
    rows, cols = [], []
    for r, n in enumerate(lens):
        cols.append(np.sort(rng.choice(G_CASE, size=int(n), replace=False)))
        rows.append(np.full(int(n), r))
    cols = np.concatenate(cols); rows = np.concatenate(rows)
    vals = rng.geometric(0.4, cols.shape[0]).astype(np.float32)
    vals[rows == ROW_ONE] = 1
    vals[rows == ROW_ONES] = 1
    first = int(np.flatnonzero(rows == ROW_SPECIAL)[0])
    vals[first:first + len(SPECIAL_COUNTS)] = SPECIAL_COUNTS
    m = sp.csr_matrix((vals, (rows, cols)), shape=(B_CASE, G_CASE))
    m.sort_indices()
    rest = rng.integers(0, 3000, B_CASE).astype(np.int64)
    for r, v in REST_SPECIAL.items():
        rest[r] = v
    return m, rest


SCALE = 1e4


def full_threshold(H: int, C: int, explicit: bool, vthr: float = 0.0) -> float:
    """An unsure threshold in the middle of the batch's own max_prob values (fp64 full call on the lognorm batch)."""
    m, rest = count_batch()
    _, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, C)
    full = lognorm_batch(m, rest, SCALE, vthr)
    sr = R.self_operand(H, m.shape[0]) if explicit else None
    _, p = R.head(R.layer_draw(full, np.ones(full.nnz, bool), table, alpha, bias, sr), w, b)
    return float(np.float32(np.median(p)))


# (H, C, explicit self rows, int64 rowptr, keep, n_draws): the thinned cases of tests/test_gpu_resident_thin.py
THIN_CASES = [(12, 2, False, False, 0.25, 3), (64, 16, True, True, 0.5, 33), (200, 40, False, True, 0.9, 3),
              (256, 16, True, False, 0.25, 33), (200, 16, False, False, 0.5, 3), (256, 40, False, True, 0.9, 3),
              (64, 2, True, False, 0.9, 33), (12, 40, True, True, 0.5, 3)]
# (H, C, explicit self rows, keep, draw): the materialised draws
MATERIALISED_CASES = [(64, 16, False, 0.5, 0), (200, 16, True, 0.25, 2)]
CASE_SEED = 0xBEEF


@functools.lru_cache(maxsize=None)
def thin_case(H, C, explicit, keep, n_draws, seed=CASE_SEED, draw0=0, vthr=0.0):
    """The fp64 reference of one case: ``stability_reference.masked_case``'s dict, and ``reads`` / ``entries`` int64 [B, D]
    (total' and deg'), ``rest``, ``scale``, ``vthr``.  ``empty`` = the draws in which no entry takes part."""
    m, rest = count_batch()
    _, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, C)
    B = m.shape[0]
    sr = R.self_operand(H, B * n_draws) if explicit else None
    thr = full_threshold(H, C, explicit, vthr)
    out = np.zeros((B * n_draws, H))
    logits = np.zeros((B, n_draws, C)); prob = np.zeros((B, n_draws))
    label = np.zeros((B, n_draws), np.int64); unc = np.zeros((B, n_draws), bool)
    reads = np.zeros((B, n_draws), np.int64); entries = np.zeros((B, n_draws), np.int64)
    for d in range(n_draws):
        cp, rp = thin_draw(m, rest, seed, draw0 + d, keep)
        vals, part, total, deg = draw_values(m, cp, rp, SCALE, vthr)
        h = R.layer_draw(vals, part, table, alpha, bias, None if sr is None else sr[d::n_draws])
        out[d::n_draws] = h
        lg, p = R.head(h, w, b)
        logits[:, d], prob[:, d] = lg, p
        label[:, d] = R.labels(lg, p, thr)
        unc[:, d] = R.unclear(lg, p, thr)
        reads[:, d], entries[:, d] = total, deg
    return dict(m=m, rest=rest, scale=SCALE, vthr=vthr, table=table, alpha=alpha, bias=bias, w=w, b=b, self_rows=sr, thr=thr, out=out,
                logits=logits, prob=prob, label=label, empty=entries == 0, unclear=unc, reads=reads, entries=entries)
