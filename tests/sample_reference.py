"""Restatement of K5, ``wgnn_sample_rows``, from the draw law of ``include/wgnn.h`` - twice: ``sample`` in vectorised numpy
uint64 arithmetic (which wraps around), ``sample_scalar`` row by row on Python ints reduced mod 2^64.  The two share no code,
so a slip in one shows as a difference (tests/test_sample_reference.py).  ``nodeflow`` restates how
``sampler.sample_nodeflow_static`` keys its blocks; ``fixture`` is the operand the CPU and GPU tests share.  Nothing here
imports torch or the package."""
import numpy as np

M64 = (1 << 64) - 1
K_STEP, K_STREAM, K_ROW, K_DRAW = 0xD6E8FEB86659FD93, 0xA24BAED4963EE407, 0x9FB21C651E98DF25, 0xC2B2AE3D27D4EB4F
U = np.uint64

PAD_COL, PAD_VAL = -7, -7.0                                            # what the ELL padding holds unless the caller says otherwise


# ------------------------------------------------------------------------------------------------
# vectorised: numpy uint64
# ------------------------------------------------------------------------------------------------
def mix32_np(x: np.ndarray) -> np.ndarray:
    """Upper half of the splitmix64 finaliser over a uint64 array."""
    with np.errstate(over="ignore"):
        x = x + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return (x ^ (x >> U(31))) >> U(32)


def draw(seed: int, step: int, stream_id: int, rows, m, k: int) -> np.ndarray:
    """Floyd's draw of k of the m candidates for every row id in ``rows`` (m > k: one number, or one per row): int64 [n, k], the
    chosen candidates in draw order."""
    rows = np.asarray(rows, np.int64)
    m = np.broadcast_to(np.asarray(m, np.int64), rows.shape)
    assert k > 0 and (m > k).all()
    with np.errstate(over="ignore"):
        base = (U(seed & M64) ^ (U(step & M64) * U(K_STEP)) ^ (U(stream_id & 0xFFFFFFFF) * U(K_STREAM))
                ^ (rows.astype(U) * U(K_ROW)))
        sel = np.full((len(rows), k), -1, np.int64)
        for i in range(k):
            j = m - k + i
            h = mix32_np(base + U(i) * U(K_DRAW))
            t = ((h * (j + 1).astype(U)) >> U(32)).astype(np.int64)
            taken = (sel[:, :i] == t[:, None]).any(1)
            sel[:, i] = np.where(taken, j, t)
    return sel


def sample(rowptr, col, val, row_ids, k, seed, step, stream_id, pad_col=PAD_COL, pad_val=PAD_VAL):
    """The five outputs of the entry: out_col int32 [n, k], out_val float32 [n, k] (padding = the sentinels), out_cnt int32 [n],
    out_self float32 [n], out_inv float32 [n].  ``row_ids`` None = every row in order."""
    rowptr = np.asarray(rowptr, np.int64)
    col, val = np.asarray(col, np.int32), np.asarray(val, np.float32)
    ids = np.arange(len(rowptr) - 1, dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)
    n = len(ids)
    out_col = np.full((n, k), pad_col, np.int32)
    out_val = np.full((n, k), pad_val, np.float32)
    if n == 0:
        return out_col, out_val, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    b = rowptr[ids]
    deg = rowptr[ids + 1] - b
    m = deg + 1
    x = np.where(np.arange(k)[None, :] < m[:, None], np.arange(k)[None, :], -1)        # m <= k: 0 .. deg, then nothing
    big = m > k
    if big.any():
        x[big] = draw(seed, step, stream_id, ids[big], m[big], k)
    is_self = x == deg[:, None]
    real = (x >= 0) & ~is_self
    order = np.argsort(~real, axis=1, kind="stable")                   # the real edges to the front, draw order kept
    xs, rs = np.take_along_axis(x, order, 1), np.take_along_axis(real, order, 1)
    src = np.where(rs, b[:, None] + xs, 0)
    if len(col):
        out_col = np.where(rs, col[src], np.int32(pad_col))
        out_val = np.where(rs, val[src], np.float32(pad_val))
    cnt, self_ = real.sum(1).astype(np.int32), is_self.any(1).astype(np.float32)
    inv = np.float32(1) / np.maximum(np.float32(1), cnt.astype(np.float32) + self_)
    return out_col, out_val, cnt, self_, inv.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# scalar: Python ints, row by row
# ------------------------------------------------------------------------------------------------
def mix32(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) % (1 << 64)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    x ^= x >> 31
    return x >> 32


def chosen(seed: int, step: int, stream_id: int, r: int, m: int, k: int) -> list:
    """The chosen list x_0, x_1, .. of one row with m candidates."""
    if m <= k:
        return list(range(m))
    wrap = 1 << 64
    base = (seed % wrap) ^ ((step % wrap) * K_STEP % wrap) ^ ((stream_id % (1 << 32)) * K_STREAM % wrap) ^ ((r % wrap) * K_ROW % wrap)
    xs = []
    for i in range(k):
        j = m - k + i
        t = (mix32((base + i * K_DRAW) % wrap) * (j + 1)) >> 32
        xs.append(j if t in xs else t)
    return xs


def sample_scalar(rowptr, col, val, row_ids, k, seed, step, stream_id, pad_col=PAD_COL, pad_val=PAD_VAL):
    """``sample`` again, one slot at a time; the values travel as their uint32 bits."""
    rowptr = [int(v) for v in rowptr]
    bits = np.asarray(val, np.float32).view(np.uint32)
    ids = list(range(len(rowptr) - 1)) if row_ids is None else [int(v) for v in row_ids]
    n = len(ids)
    out_col = np.full((n, k), pad_col, np.int32)
    out_bits = np.full((n, k), np.float32(pad_val).view(np.uint32), np.uint32)
    cnt, self_, inv = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for s, r in enumerate(ids):
        b = rowptr[r]
        deg = rowptr[r + 1] - b
        xs = chosen(seed, step, stream_id, r, deg + 1, k)
        o = 0
        for x in xs:
            if x == deg:
                self_[s] = 1.0
            else:
                out_col[s, o], out_bits[s, o] = col[b + x], bits[b + x]
                o += 1
        cnt[s] = o
        inv[s] = np.float32(1) / np.float32(max(1, o + int(self_[s])))
    return out_col, out_bits.view(np.float32), cnt, self_, inv


# ------------------------------------------------------------------------------------------------
# sampler.sample_nodeflow_static
# ------------------------------------------------------------------------------------------------
def block_k(rowptr, k: int) -> int:
    """``sample_block_static``'s draws per row: k clamped to the longest row and its self-loop (the same lists, by the clamp lemma)."""
    longest = int(np.diff(np.asarray(rowptr, np.int64)).max()) if len(rowptr) > 1 else 0
    return max(1, min(int(k), longest + 1))


def nodeflow(g_cg, g_gc, seed_cells, n_layers: int, k: int, seed: int, step: int, pad_col=0, pad_val=0.0):
    """blocks[i] = (cell block, gene block or None), a block = (kk, the five outputs of ``sample``).  ``g_cg`` / ``g_gc`` are the
    (rowptr, col, val) of cells<-genes and genes<-cells; layer i draws with stream ids 2i (cells) and 2i + 1 (genes), the last
    layer over the seed cells only, every lower one over all rows; the whole NodeFlow at one ``step``."""
    blocks = []
    for i in range(n_layers):
        last = i == n_layers - 1
        kc = block_k(g_cg[0], k)
        cb = (kc, sample(*g_cg, seed_cells if last else None, kc, seed, step, 2 * i, pad_col, pad_val))
        gb = None
        if not last:
            kg = block_k(g_gc[0], k)
            gb = (kg, sample(*g_gc, None, kg, seed, step, 2 * i + 1, pad_col, pad_val))
        blocks.append((cb, gb))
    return blocks


# ------------------------------------------------------------------------------------------------
# the fixture the CPU and GPU tests share
# ------------------------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 4, 5, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 193, 254, 255, 256, 257, 300, 1000, 5000)
KS = (1, 2, 5, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
# float32 bit patterns a copy must carry unchanged, four per row, at the head of the rows of degree 5000, 300 and 65:
# -0.0, the smallest denormal, inf, a quiet NaN with a payload | +0.0, a negative denormal, -inf, a negative NaN with a payload |
# the largest finite value, the largest denormal, a signalling NaN, another denormal
SPECIAL_BITS = {22: (0x80000000, 0x00000001, 0x7F800000, 0x7FC12345),
                20: (0x00000000, 0x80000002, 0xFF800000, 0xFFC54321),
                8: (0x7F7FFFFF, 0x007FFFFF, 0x7F800001, 0x00000003)}


def fixture():
    """23 rows of DEGREES: (rowptr int32, col int32, val float32).  ``col`` is injective within a row (a multiplicative
    permutation of the positions, so nothing is in order); ``val`` is all distinct as BITS: SPECIAL_BITS, elsewhere an exact
    dyadic ramp that never meets zero."""
    rowptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = np.concatenate([(np.arange(d, dtype=np.int64) * 7919 + 13 * r) % 8191 for r, d in enumerate(DEGREES)]).astype(np.int32)
    val = (np.arange(nnz, dtype=np.float32) - 3000.0) / 64.0 + np.float32(1.0 / 128.0)
    bits = val.view(np.uint32).copy()
    for r, four in SPECIAL_BITS.items():
        bits[rowptr[r]: rowptr[r] + 4] = four
    for r, d in enumerate(DEGREES):
        assert len(set(col[rowptr[r]: rowptr[r + 1]].tolist())) == d
    assert len(set(bits.tolist())) == nnz
    return rowptr, col, bits.view(np.float32)
