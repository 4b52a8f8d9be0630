"""Reference of ``wgnn_rank_sets_rows`` / ``ResidentPredictor.signatures`` (``include/wgnn.h``): UCell's rank-based signature
score, derived WITHOUT the kernel's counting form.  A cell's row is made dense, ``scipy.stats.rankdata(-row, "average")`` gives
the tie-averaged ranks (rank 1 = the highest value; the genes the cell does not store are zeros and tie at the bottom), the ranks
are capped at ``max_rank + 1``, and ``score = 1 - U / (n * max_rank)`` with ``U = sum of the set's ranks - n (n + 1) / 2``.  The
kernel's integer outputs are read off the same ranks: twice a mid-rank is an integer.

``by_key=True`` ranks the stored entries on the order-preserving integer key of their float32 bits instead of their value (the
definition's order, which also places negative values, signed zeros and NaNs); on the positive finite values ``align`` emits
the two orders are the same.  Rows that list a gene twice are outside this reference."""
import numpy as np
from scipy.stats import rankdata


def key32(values) -> np.ndarray:
    """The order-preserving uint32 key of float32 bits: all bits flipped for a set sign bit, else the sign bit set."""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dense_ranks(cols, vals, G: int, by_key: bool = False) -> np.ndarray:
    """f64 [G]: the tie-averaged descending rank of every gene of one cell (stored entries ``cols`` / ``vals``)."""
    cols = np.asarray(cols, np.int64)
    assert len(set(cols.tolist())) == len(cols), "a gene listed twice"
    row = np.zeros(G, np.float64)
    if by_key:
        row[cols] = key32(vals).astype(np.float64) + 1.0          # every stored entry above the zeros of the others
    else:
        vals = np.asarray(vals, np.float64)
        assert np.all(np.isfinite(vals) & (vals > 0)), "the value order needs positive finite values (use by_key)"
        row[cols] = vals
    return rankdata(-row, "average")


def rank_sets(indptr, indices, data, G: int, member: np.ndarray, max_rank: int, by_key: bool = False):
    """``(rank2_sum int64 [B, P], present int64 [B, P], score f64 [B, P])`` of a CSR batch and ``member`` bool [P, G]."""
    B, P = len(indptr) - 1, member.shape[0]
    rank2_sum, present = np.zeros((B, P), np.int64), np.zeros((B, P), np.int64)
    score = np.full((B, P), np.nan)
    for r in range(B):
        cols, vals = indices[indptr[r]:indptr[r + 1]], data[indptr[r]:indptr[r + 1]]
        ranks = np.minimum(dense_ranks(cols, vals, G, by_key), max_rank + 1.0)
        twice = np.rint(2.0 * ranks).astype(np.int64)
        assert np.array_equal(twice, 2.0 * ranks)
        stored = np.zeros(G, bool)
        stored[np.asarray(cols, np.int64)] = True
        for p in range(P):
            n = int(member[p].sum())
            rank2_sum[r, p] = twice[member[p] & stored].sum()
            present[r, p] = int((member[p] & stored).sum())
            if n:
                u = ranks[member[p]].sum() - n * (n + 1) / 2
                score[r, p] = 1.0 - u / (n * max_rank)
    return rank2_sum, present, score


def count_form(indptr, indices, data, member: np.ndarray, max_rank: int):
    """The kernel's definition restated in numpy - ``R2_j = 2 * #{key_i > key_j} + #{key_i == key_j} + 1``, capped - as
    ``(rank2_sum, present)`` int64 [B, P]: what the tests hold against ``rank_sets``, the derivation by ``rankdata``."""
    B, P = len(indptr) - 1, member.shape[0]
    rank2_sum, present = np.zeros((B, P), np.int64), np.zeros((B, P), np.int64)
    for r in range(B):
        cols = np.asarray(indices[indptr[r]:indptr[r + 1]], np.int64)
        k = key32(data[indptr[r]:indptr[r + 1]]).astype(np.int64)
        r2 = 2 * (k[None, :] > k[:, None]).sum(axis=1) + (k[None, :] == k[:, None]).sum(axis=1) + 1
        r2c = np.minimum(r2, 2 * (max_rank + 1))
        for p in range(P):
            on = member[p][cols]
            rank2_sum[r, p], present[r, p] = r2c[on].sum(), on.sum()
    return rank2_sum, present


def pack(member: np.ndarray) -> np.ndarray:
    """bool [P <= 64, G] -> uint64 [G] membership words, bit p of word g = gene g belongs to set p."""
    words = np.zeros(member.shape[1], np.uint64)
    for p in range(member.shape[0]):
        words |= member[p].astype(np.uint64) << np.uint64(p)
    return words


# ------------------------------------------------------------------------------------------------
# the batch of the GPU op test
# ------------------------------------------------------------------------------------------------
VALUES = np.log1p(np.arange(1, 6) / 50 * 1e4).astype(np.float32)        # five distinct values: tie-heavy rows
N_CORE = 20                                                             # genes 0 .. 19 belong to every set that holds a gene
EMPTY_SET, WHOLE_SET = 5, 7
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 129, 9, 10, 11, 101, 102, 103, 50, N_CORE, 299, 300)
EQUAL_PAIR, ONE_VALUE, ALL_MEMBERS = 2, 14, 15                          # rows of ROW_LENGTHS with a special content


def membership(G: int, P: int = 64, seed: int = 0) -> np.ndarray:
    """bool [P, G]: random sets of about G / 8 genes that all hold the core genes; set EMPTY_SET holds no gene, set WHOLE_SET
    every gene."""
    rng = np.random.default_rng(seed)
    member = rng.random((P, G)) < 0.125
    member[:, :N_CORE] = True
    if P > EMPTY_SET:
        member[EMPTY_SET] = False
    if P > WHOLE_SET:
        member[WHOLE_SET] = True
    return member


def case_rows(G: int = 300, lengths=ROW_LENGTHS, seed: int = 1):
    """``(indptr int64, indices int32, data f32)``: one row per entry of ``lengths``, its genes a random subset in random order,
    its values drawn from VALUES.  Row EQUAL_PAIR holds two equal values, row ONE_VALUE one value throughout, row ALL_MEMBERS
    the core genes only - every entry a member of every set but the empty one."""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for i, n in enumerate(lengths):
        cols = rng.permutation(N_CORE)[:n] if (i == ALL_MEMBERS and lengths is ROW_LENGTHS) else rng.permutation(G)[:n]
        vals = VALUES[rng.integers(0, len(VALUES), n)]
        if lengths is ROW_LENGTHS and i in (EQUAL_PAIR, ONE_VALUE):
            vals = np.full(n, VALUES[3], np.float32)
        indices.append(cols.astype(np.int32)); data.append(vals.astype(np.float32))
        indptr.append(indptr[-1] + n)
    return np.asarray(indptr, np.int64), np.concatenate(indices), np.concatenate(data)
