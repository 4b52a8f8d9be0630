"""Plain numpy / Python restatement of ``wgnn_predict_rows_dropout`` (include/wgnn.h): the hash and the mask in uint64 with
wrap-around, one draw's layer in fp64 over the kept entries, the head, the label rule and the tallies - and the cases the CPU
and GPU tests share.  Nothing here imports torch or the package."""
import functools
import math

import numpy as np
import scipy.sparse as sp

M64 = (1 << 64) - 1
K_CELL, K_DRAW, K_GENE = 0x9FB21C651E98DF25, 0xD6E8FEB86659FD93, 0xC2B2AE3D27D4EB4F


# ------------------------------------------------------------------------------------------------
# the hash and the mask
# ------------------------------------------------------------------------------------------------
def mix32(x: int) -> int:
    """Upper half of the splitmix64 finaliser, on Python ints reduced mod 2^64."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def hash_u(seed: int, cell: int, draw: int, gene: int) -> int:
    key = (seed & M64) ^ ((cell * K_CELL) & M64) ^ ((draw * K_DRAW) & M64)
    return mix32((key + gene * K_GENE) & M64)


def threshold(keep: float) -> int:
    return int(math.floor(keep * 4294967296.0))


def hash_u_np(seed: int, cell, draw, gene) -> np.ndarray:
    """``hash_u`` over arrays (broadcast), in numpy uint64 arithmetic, which wraps around."""
    u = lambda v: np.asarray(v).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = np.uint64(seed & M64) ^ (u(cell) * np.uint64(K_CELL)) ^ (u(draw) * np.uint64(K_DRAW))
        x = key + u(gene) * np.uint64(K_GENE)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x >> np.uint64(32)


def mask(seed: int, cell, draw, gene, keep: float) -> np.ndarray:
    """Boolean: is the entry (cell, gene) kept in this draw."""
    return hash_u_np(seed, cell, draw, gene) < np.uint64(threshold(keep))


def entry_mask(m: sp.csr_matrix, seed: int, draw: int, keep: float, row0: int = 0) -> np.ndarray:
    """The mask of one draw over the stored entries of a CSR batch, in CSR order."""
    rows = np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr))
    return mask(seed, rows + row0, draw, m.indices.astype(np.int64), keep)


# ------------------------------------------------------------------------------------------------
# one draw's layer, the head, the labels, the tallies
# ------------------------------------------------------------------------------------------------
def layer_draw(m: sp.csr_matrix, kept: np.ndarray, table, alpha, bias, self_rows=None) -> np.ndarray:
    """ReLU(z) [B, H] in fp64 of one draw: wgnn_predict_rows' formula over the kept entries (deg' = their number, S' = their
    sum); a draw that keeps nothing (or whose kept values sum to 0) is the empty row."""
    B, G = m.shape
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    x = m.data.astype(np.float64)
    k = kept.astype(np.float64)
    a = alpha.astype(np.float64)
    deg = np.bincount(rows, weights=k, minlength=B)
    s = np.bincount(rows, weights=k * x, minlength=B)
    ok = s[rows] != 0
    ss = np.where(ok, s[rows], 1.0)
    coef = a[m.indices] * deg[rows] * x / ss
    if self_rows is None:
        coef = coef + x * a[G + 1] / (ss + 1e-6)
    coef = np.where(ok, coef * k, 0.0)
    acc = sp.csr_matrix((coef, m.indices, m.indptr), shape=m.shape) @ table.astype(np.float64)
    if self_rows is not None:
        acc = acc + a[G + 1] * self_rows.astype(np.float64)
    return np.maximum(acc / (deg + 1)[:, None] + bias.astype(np.float64), 0.0)


def head(h, w, b):
    """(logits [B, C], max_prob [B]) in fp64."""
    logits = h @ w.astype(np.float64).T + b.astype(np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return logits, 1.0 / e.sum(axis=1)


def labels(logits, p, thr: float) -> np.ndarray:
    """The arg max (numpy's: the lowest index among equal maxima), or -1 where max_prob is below the f32 threshold."""
    return np.where(p < float(np.float32(thr)), -1, logits.argmax(axis=1)).astype(np.int64)


def unclear(logits, p, thr: float, tol: float = 1e-5) -> np.ndarray:
    """Pairs whose label the f32 kernel may legitimately decide the other way: top-two gap or distance to the threshold <= tol."""
    srt = np.sort(logits, axis=1)
    gap = srt[:, -1] - srt[:, -2] if logits.shape[1] > 1 else np.full(logits.shape[0], np.inf)
    return ~((gap > tol) & (np.abs(p - float(np.float32(thr))) > tol))


def tallies(draw_label: np.ndarray, draw_prob: np.ndarray, draw_empty: np.ndarray, n_classes: int):
    """(votes [B, C], unsure [B], empty [B], conf_sum [B]) of per-draw tables [B, D]; conf_sum adds the f32 values in fp64 in
    ascending draw order."""
    B, D = draw_label.shape
    votes = np.zeros((B, n_classes), np.int64)
    for j in range(n_classes):
        votes[:, j] = (draw_label == j).sum(axis=1)
    conf = np.zeros(B, np.float64)
    for d in range(D):
        conf = conf + draw_prob[:, d].astype(np.float32).astype(np.float64)
    return votes, (draw_label == -1).sum(axis=1), draw_empty.astype(bool).sum(axis=1), conf


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
G_CASE, B_CASE = 6000, 40


def ragged_batch(rng, B=B_CASE, G=G_CASE, long_row=5000) -> sp.csr_matrix:
    """Ragged raw-value CSR: an empty row, a 1-entry row, rows of 63 / 64 / 65 entries, one row longer than 4096 entries, the
    rest 1 .. 300 genes (a cell's genes ascending)."""
    lens = rng.integers(1, 300, B)
    lens[1] = 0
    lens[2] = 1
    lens[3] = long_row
    lens[5], lens[6], lens[7] = 63, 64, 65
    rows, cols = [], []
    for r, n in enumerate(lens):
        cols.append(np.sort(rng.choice(G, size=int(n), replace=False)))
        rows.append(np.full(int(n), r))
    cols = np.concatenate(cols); rows = np.concatenate(rows)
    vals = np.clip(rng.normal(3.0, 1.0, cols.shape[0]), 0.2, 7.0).astype(np.float32)
    m = sp.csr_matrix((vals, (rows, cols)), shape=(B, G))
    m.sort_indices()
    return m


@functools.lru_cache(maxsize=None)
def operands(H: int, seed: int = 0):
    """(batch, table [G, H], alpha [G + 2], bias [H]) of a case; the same for every C / draw count of that H."""
    rng = np.random.default_rng(1000 + 7 * H + seed)
    m = ragged_batch(rng)
    table = (0.5 * rng.standard_normal((G_CASE, H))).astype(np.float32)
    alpha = rng.uniform(0.5, 1.5, G_CASE + 2).astype(np.float32)
    bias = (0.1 * rng.standard_normal(H)).astype(np.float32)
    return m, table, alpha, bias


def head_operands(H: int, C: int):
    rng = np.random.default_rng(50_000 + 41 * H + C)
    return (rng.standard_normal((C, H)) / np.sqrt(H)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)


def self_operand(H: int, n_pairs: int) -> np.ndarray:
    return (0.5 * np.random.default_rng(90_000 + H).standard_normal((n_pairs, H))).astype(np.float32)


def full_threshold(H: int, C: int, explicit: bool) -> float:
    """An unsure threshold in the middle of the batch's own max_prob values (fp64 full call), as a float32 value."""
    m, table, alpha, bias = operands(H)
    w, b = head_operands(H, C)
    sr = self_operand(H, m.shape[0]) if explicit else None
    _, p = head(layer_draw(m, np.ones(m.nnz, bool), table, alpha, bias, sr), w, b)
    return float(np.float32(np.median(p)))


# (H, C, explicit self rows, int64 rowptr, keep, n_draws): the masked cases of tests/test_gpu_resident_stability.py
MASKED_CASES = [(12, 2, False, False, 0.25, 3), (32, 16, True, True, 0.5, 33), (64, 40, False, True, 0.9, 3),
                (128, 16, True, False, 0.25, 33), (200, 16, False, False, 0.5, 33), (256, 40, True, True, 0.9, 3),
                (200, 2, True, False, 0.5, 3), (256, 16, False, False, 0.9, 33)]
# (H, C, explicit self rows, keep, draw): the materialised draws
MATERIALISED_CASES = [(64, 16, False, 0.5, 0), (200, 16, True, 0.25, 7), (12, 40, False, 0.9, 2)]
CASE_SEED = 0xC0FFEE


@functools.lru_cache(maxsize=None)
def masked_case(H, C, explicit, keep, n_draws, seed=CASE_SEED, row0=0, draw0=0):
    """The fp64 reference of one masked case: a dict with ``out`` [B * D, H] (row r * D + d), ``logits`` [B, D, C], ``prob`` /
    ``label`` / ``empty`` / ``unclear`` [B, D], the operands, and ``thr``."""
    m, table, alpha, bias = operands(H)
    w, b = head_operands(H, C)
    B = m.shape[0]
    sr = self_operand(H, B * n_draws) if explicit else None
    thr = full_threshold(H, C, explicit)
    out = np.zeros((B * n_draws, H))
    logits = np.zeros((B, n_draws, C)); prob = np.zeros((B, n_draws))
    label = np.zeros((B, n_draws), np.int64); empty = np.zeros((B, n_draws), bool); unc = np.zeros((B, n_draws), bool)
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    for d in range(n_draws):
        kept = entry_mask(m, seed, draw0 + d, keep, row0)
        h = layer_draw(m, kept, table, alpha, bias, None if sr is None else sr[d::n_draws])
        out[d::n_draws] = h
        lg, p = head(h, w, b)
        logits[:, d], prob[:, d] = lg, p
        label[:, d] = labels(lg, p, thr)
        unc[:, d] = unclear(lg, p, thr)
        empty[:, d] = np.bincount(rows, weights=kept, minlength=B) == 0
    return dict(m=m, table=table, alpha=alpha, bias=bias, w=w, b=b, self_rows=sr, thr=thr, out=out, logits=logits, prob=prob,
                label=label, empty=empty, unclear=unc)


def thinned(m: sp.csr_matrix, kept: np.ndarray) -> sp.csr_matrix:
    """The CSR of one draw materialised: the kept entries only, the order of a row's genes unchanged."""
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))[kept]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m.shape[0]))])
    return sp.csr_matrix((m.data[kept], m.indices[kept], indptr), shape=m.shape)
