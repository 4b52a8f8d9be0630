"""Plain numpy restatement of ``wgnn_predict_rows_panels`` (include/wgnn.h): the GIVEN membership of every panel, its packed
words, one pair's layer in fp64 over the kept entries (tests/stability_reference.py's ``layer_draw``, head and label rule),
the counts mode through tests/thin_reference.py's ``lognorm`` - and the cases the CPU and GPU tests share.  Nothing here
imports torch or the package."""
import functools

import numpy as np
import scipy.sparse as sp

import stability_reference as R
import thin_reference as T

DENSITY = (0.02, 0.1, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def membership(G: int, P: int) -> np.ndarray:
    """bool [P, G]: panel 0 all genes, 1 none, 2 the even ids, 3 the ids below G // 2, panel p >= 4 random at a density of
    0.02 / 0.1 / 0.5 / 0.9 by ``p % 4``."""
    m = np.zeros((P, G), bool)
    ids = np.arange(G)
    for p in range(P):
        if p == 0:
            m[p] = True
        elif p == 1:
            pass
        elif p == 2:
            m[p] = ids % 2 == 0
        elif p == 3:
            m[p] = ids < G // 2
        else:
            m[p] = np.random.default_rng(4242 + p).random(G) < DENSITY[p % 4]
    m.setflags(write=False)
    return m


def pack(member: np.ndarray) -> np.ndarray:
    """bool [P <= 64, G] -> uint64 [G]: bit p of word g = gene g belongs to panel p."""
    P = member.shape[0]
    assert 1 <= P <= 64
    words = np.zeros(member.shape[1], np.uint64)
    for p in range(P):
        words |= member[p].astype(np.uint64) << np.uint64(p)
    return words


def unpack(words: np.ndarray, P: int) -> np.ndarray:
    return np.stack([(words >> np.uint64(p)) & np.uint64(1) for p in range(P)]).astype(bool)


def kept_entries(m: sp.csr_matrix, member_p: np.ndarray) -> np.ndarray:
    """The stored entries of a CSR batch whose gene is in the panel, in CSR order."""
    return member_p[m.indices]


# (H, C, explicit self rows, int64 rowptr, P): the cases of tests/test_gpu_resident_panels.py - P = 64 (bit 63), 33 (bit 32),
# 9 and 17 (no multiples of the 8 waves), 3 (fewer panels than waves), every lane ladder H from 12 to 256
PANEL_CASES = [(12, 2, False, False, 3), (32, 16, True, True, 9), (64, 40, False, True, 64), (128, 16, True, False, 8),
               (200, 16, False, False, 64), (256, 40, True, True, 33), (200, 2, True, False, 4), (256, 16, False, False, 17)]


@functools.lru_cache(maxsize=None)
def panel_case(H, C, explicit, P):
    """The fp64 reference of one values-mode case over ``stability_reference.operands(H)`` (B = 40, G = 6000: an empty row, a
    1-entry row, rows of 63 / 64 / 65 entries, a 5000-entry row that outgrows a 1024-entry stash): a dict with ``out``
    [B * P, H] (row r * P + p), ``logits`` [B, P, C], ``prob`` / ``label`` / ``entries`` / ``empty`` / ``unclear`` [B, P], the
    operands, ``member`` bool [P, G] and ``thr``."""
    m, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, C)
    B, G = m.shape
    member = membership(G, P)
    sr = R.self_operand(H, B * P) if explicit else None
    thr = R.full_threshold(H, C, explicit)
    return dict(m=m, table=table, alpha=alpha, bias=bias, w=w, b=b, self_rows=sr, thr=thr, member=member,
                **_pairs(m, [kept_entries(m, member[p]) for p in range(P)], table, alpha, bias, sr, w, b, thr))


def _pairs(vals: sp.csr_matrix, kept_per_panel, table, alpha, bias, sr, w, b, thr):
    B, P, C, H = vals.shape[0], len(kept_per_panel), w.shape[0], table.shape[1]
    rows = np.repeat(np.arange(B), np.diff(vals.indptr))
    out = np.zeros((B * P, H))
    logits = np.zeros((B, P, C)); prob = np.zeros((B, P))
    label = np.zeros((B, P), np.int64); unc = np.zeros((B, P), bool); entries = np.zeros((B, P), np.int64)
    for p, kept in enumerate(kept_per_panel):
        h = R.layer_draw(vals, kept, table, alpha, bias, None if sr is None else sr[p::P])
        out[p::P] = h
        lg, pr = R.head(h, w, b)
        logits[:, p], prob[:, p] = lg, pr
        label[:, p] = R.labels(lg, pr, thr)
        unc[:, p] = R.unclear(lg, pr, thr)
        entries[:, p] = np.bincount(rows, weights=kept, minlength=B)
    return dict(out=out, logits=logits, prob=prob, label=label, unclear=unc, entries=entries, empty=entries == 0)


# ------------------------------------------------------------------------------------------------
# counts mode
# ------------------------------------------------------------------------------------------------
def panel_reads(m: sp.csr_matrix, rest: np.ndarray, member: np.ndarray) -> np.ndarray:
    """int64 [B, P]: the cell's reads inside each panel - its bundle counts there, and ``rest`` (one more caller column,
    outside the bundle) for the ODD-numbered panels."""
    P = member.shape[0]
    counts = sp.csr_matrix((m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape)
    lib = np.asarray(counts @ member.T.astype(np.float64)).astype(np.int64)
    lib[:, 1::2] += np.asarray(rest, np.int64)[:, None]
    return lib


def count_values(m: sp.csr_matrix, member_p: np.ndarray, lib_p: np.ndarray, scale: float, vthr: float):
    """``(values csr with v' as data, part bool per entry)`` of one panel of a batch of counts: v' = lognorm(count, lib[r]),
    an entry takes part iff its gene is in the panel, count > 0 and v' > vthr (never where lib[r] <= 0)."""
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    v = T.lognorm(m.data, lib_p[rows], scale)
    part = member_p[m.indices] & (m.data > 0) & (v > np.float32(vthr)) & (lib_p[rows] > 0)
    return sp.csr_matrix((v, m.indices, m.indptr), shape=m.shape), part


def zeroed_dense(m: sp.csr_matrix, rest: np.ndarray, member_p: np.ndarray, odd: bool) -> np.ndarray:
    """The count matrix [B, G + 1] with the non-panel columns zeroed; the last column is the caller's extra one."""
    x = np.zeros((m.shape[0], m.shape[1] + 1), np.float32)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    keep = member_p[m.indices]
    x[rows[keep], m.indices[keep]] = m.data[keep]
    if odd:
        x[:, -1] = rest
    return x


# (H, C, explicit self rows, int64 rowptr, P, value threshold)
COUNT_CASES = [(64, 16, False, False, 9, 0.0), (200, 40, True, True, 17, 1.5)]


@functools.lru_cache(maxsize=None)
def count_case(H, C, explicit, P, vthr=0.0):
    """``panel_case``'s dict for a counts-mode case over ``thin_reference.count_batch()``, and ``lib`` int64 [B, P], ``rest``,
    ``scale``, ``vthr``."""
    m, rest = T.count_batch()
    _, table, alpha, bias = R.operands(H)
    w, b = R.head_operands(H, C)
    B, G = m.shape
    member = membership(G, P)
    lib = panel_reads(m, rest, member)
    sr = R.self_operand(H, B * P) if explicit else None
    thr = T.full_threshold(H, C, explicit, vthr)
    rows = np.repeat(np.arange(B), np.diff(m.indptr))
    out = np.zeros((B * P, H)); logits = np.zeros((B, P, C)); prob = np.zeros((B, P))
    label = np.zeros((B, P), np.int64); unc = np.zeros((B, P), bool); entries = np.zeros((B, P), np.int64)
    for p in range(P):
        vals, part = count_values(m, member[p], lib[:, p], T.SCALE, vthr)
        h = R.layer_draw(vals, part, table, alpha, bias, None if sr is None else sr[p::P])
        out[p::P] = h
        lg, pr = R.head(h, w, b)
        logits[:, p], prob[:, p] = lg, pr
        label[:, p] = R.labels(lg, pr, thr)
        unc[:, p] = R.unclear(lg, pr, thr)
        entries[:, p] = np.bincount(rows, weights=part, minlength=B)
    return dict(m=m, rest=rest, scale=T.SCALE, vthr=vthr, table=table, alpha=alpha, bias=bias, w=w, b=b, self_rows=sr, thr=thr,
                member=member, lib=lib, out=out, logits=logits, prob=prob, label=label, unclear=unc, entries=entries,
                empty=entries == 0)
