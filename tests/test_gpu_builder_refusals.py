"""What ``ops.pair_rows``, ``pool_rows``, ``pool_rows_grouped`` and ``soup_rows`` refuse before any launch - the exception class
exactly (``ValueError``) and a fragment of the message that tells the check - and what they raise after the launches from the
status word: ``WgnnError`` with the text of the one bit set, a case per bit of ``_PAIR_STATUS``, ``_POOL_STATUS`` and
``_SOUP_STATUS`` (operands the kernels are built to skip and report: nothing here faults).  One table; the operands are the
smallest that reach every branch: 2 cells with 1 and 2 entries, 5 genes, 2 pairs, 2 groups, 2 draws, a ``cdf`` of 7 entries.  The
tensors live on the GPU because the wrappers refuse CPU tensors first."""
import functools
from types import SimpleNamespace

import pytest
import torch

from scdeepsort_amd import WgnnError, _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, G, K, D, NNZ = 2, 5, 2, 2, 3

PAIR, POOL, GROUPED, SOUP = "pair_rows", "pool_rows", "pool_rows_grouped", "soup_rows"
CSR_OPS = (PAIR, POOL, GROUPED, SOUP)                  # all four take the count CSR and the log-normalisation's scale / threshold
SAYS = {PAIR: "pair_rows", POOL: "pool_rows", GROUPED: "pool_rows", SOUP: "soup_rows"}      # the name in an op's messages


@functools.lru_cache(maxsize=1)
def _operands():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=DEV)
    return SimpleNamespace(
        rowptr=i32(0, 1, 3), col=i32(4, 0, 2), cnt=torch.tensor([1.0, 2.0, 3.0], device=DEV), lib=i64(1, 5),
        a=i32(0, 1), b=i32(1, 0), group=i32(0, 1), group_ptr=i64(0, 1, 2), members=i32(0, 1), total=i64(1, 5),
        n_add=i64(1, 2), cdf=i64(0, 1, 2, 3, 4, 5, 6), i32=i32, i64=i64)


def _base(fn, o):
    kw = dict(rowptr=o.rowptr, col=o.col, cnt=o.cnt)
    if fn == PAIR:
        kw.update(lib=o.lib, a=o.a, b=o.b)
    elif fn == POOL:
        kw.update(lib=o.lib, group=o.group, n_groups=K, n_genes=G)
    elif fn == GROUPED:
        kw.update(group_ptr=o.group_ptr, members=o.members, total=o.total, n_genes=G)
    else:
        kw.update(lib=o.lib, n_add=o.n_add, cdf=o.cdf, n_draws=D, scale=1e4, threshold=0.0)
    return kw


def _seed(o, **swap):
    """an earlier ``pool_rows`` result over the two groups - (rowptr, col, cnt, total, n_cells) - with some of it swapped"""
    s = dict(rowptr=o.i64(0, 1, 2), col=o.i32(0, 1), cnt=o.i64(2, 3), total=o.i64(2, 3), n_cells=o.i64(1, 1))
    s.update(swap)
    return tuple(s.values())


def _cases():
    rows = []

    def add(fns, error, fragment, change):
        rows.extend((fn, error, fragment.replace("{name}", SAYS[fn]) if fragment else None, change) for fn in fns)

    add(CSR_OPS, None, None, lambda o: {})                                    # the operands as they are: no refusal
    # the count CSR
    takes = "{name} takes rowptr int32 / int64, col int32, cnt float32"
    add(CSR_OPS, ValueError, takes, lambda o: dict(rowptr=o.rowptr.to(torch.int16)))
    add(CSR_OPS, ValueError, takes, lambda o: dict(col=o.col.long()))
    add(CSR_OPS, ValueError, takes, lambda o: dict(cnt=o.cnt.double()))
    three = (PAIR, GROUPED, SOUP)                                             # pool_rows looks at rowptr's shape before anything else
    add(three, ValueError, "malformed CSR: rowptr (1, 3), col (3,), cnt (3,)", lambda o: dict(rowptr=o.rowptr.reshape(1, 3)))
    add(three, ValueError, "malformed CSR: rowptr (0,), col (3,), cnt (3,)", lambda o: dict(rowptr=o.rowptr[:0]))
    add((POOL,), ValueError, "malformed CSR: rowptr (1, 3)", lambda o: dict(rowptr=o.rowptr.reshape(1, 3)))
    add((POOL,), ValueError, "malformed CSR: rowptr (0,)", lambda o: dict(rowptr=o.rowptr[:0]))
    add(CSR_OPS, ValueError, "malformed CSR: rowptr (3,), col (3, 1), cnt (3, 1)",
        lambda o: dict(col=o.col.reshape(3, 1), cnt=o.cnt.reshape(3, 1)))
    add(CSR_OPS, ValueError, "malformed CSR: rowptr (3,), col (3,), cnt (2,)", lambda o: dict(cnt=o.cnt[:2]))
    # the log-normalisation
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        add(CSR_OPS, ValueError, f"{{name}}: scale = {scale} must be positive and finite", lambda o, scale=scale: dict(scale=scale))
    for thr in (-0.5, float("nan")):
        add(CSR_OPS, ValueError, f"{{name}}: threshold = {thr} must be >= 0", lambda o, thr=thr: dict(threshold=thr))
    # the library sizes
    for fn in (PAIR, POOL, SOUP):
        add((fn,), ValueError, "{name}: lib must be int64 [2]", lambda o: dict(lib=o.lib.to(torch.int32)))
        add((fn,), ValueError, "{name}: lib must be int64 [2]", lambda o: dict(lib=o.i64(1, 5, 7)))
    # pair_rows
    one_length = "pair_rows: a and b must be int32 vectors of one length"
    add((PAIR,), ValueError, one_length, lambda o: dict(a=o.a.long()))
    add((PAIR,), ValueError, one_length, lambda o: dict(b=o.b.long()))
    add((PAIR,), ValueError, one_length, lambda o: dict(a=o.a[:1]))
    add((PAIR,), ValueError, one_length, lambda o: dict(a=o.a.reshape(2, 1), b=o.b.reshape(2, 1)))
    # pool_rows
    add((POOL,), ValueError, "pool_rows: n_groups = -1 must not be negative", lambda o: dict(n_groups=-1))
    add((POOL,), ValueError, "pool_rows: group must be int32 [2]", lambda o: dict(group=o.group.long()))
    add((POOL,), ValueError, "pool_rows: group must be int32 [2]", lambda o: dict(group=o.i32(0, 1, 1)))
    add((POOL,), ValueError, "pool_rows: group id out of range [-1, 2)", lambda o: dict(group=o.i32(0, 2)))
    add((POOL,), ValueError, "pool_rows: group id out of range [-1, 2)", lambda o: dict(group=o.i32(-2, 1)))
    add((POOL,), ValueError, "pool_rows: seed is an earlier result's (rowptr, col, cnt, total, n_cells)", lambda o: dict(seed=_seed(o)[:3]))
    same_groups = "pool_rows: seed must be an earlier result over the same 2 groups"
    add((POOL,), ValueError, same_groups, lambda o: dict(seed=_seed(o, total=o.i64(2, 3, 4))))
    add((POOL,), ValueError, same_groups, lambda o: dict(seed=_seed(o, n_cells=o.i64(1))))
    add((POOL,), ValueError, same_groups, lambda o: dict(seed=_seed(o, rowptr=o.i64(0, 2))))
    add((POOL,), ValueError, same_groups, lambda o: dict(seed=_seed(o, cnt=o.i64(2, 3, 4))))
    add((POOL,), ValueError, same_groups, lambda o: dict(seed=_seed(o, cnt=o.i32(2, 3))))
    add((POOL,), ValueError, "pool_rows: seed holds a gene id outside [0, 5)", lambda o: dict(seed=_seed(o, col=o.i32(0, 5))))
    add((POOL,), ValueError, "pool_rows: seed holds a gene id outside [0, 5)", lambda o: dict(seed=_seed(o, col=o.i32(-1, 1))))
    add((POOL,), ValueError, "pool_rows: group 1 pools a library size of 2^53 or more", lambda o: dict(lib=o.i64(1, 2 ** 53)))
    # pool_rows_grouped
    add((GROUPED,), ValueError, "pool_rows: group_ptr must be an int64 vector [n_groups + 1]", lambda o: dict(group_ptr=o.group_ptr.to(torch.int32)))
    add((GROUPED,), ValueError, "pool_rows: group_ptr must be an int64 vector [n_groups + 1]", lambda o: dict(group_ptr=o.group_ptr[:0]))
    add((GROUPED,), ValueError, "pool_rows: members must be int32 [2], one entry per row", lambda o: dict(members=o.members.long()))
    add((GROUPED,), ValueError, "pool_rows: members must be int32 [2], one entry per row", lambda o: dict(members=o.i32(0, 1, 1)))
    add((GROUPED,), ValueError, "pool_rows: total must be int64 [2]", lambda o: dict(total=o.total.double()))
    add((GROUPED,), ValueError, "pool_rows: total must be int64 [2]", lambda o: dict(total=o.i64(1, 5, 7)))
    add((GROUPED,), ValueError, "pool_rows: seed must be an earlier result over the same 2 groups", lambda o: dict(seed=_seed(o, rowptr=o.i64(0, 2))[:3]))
    for n_genes in (-1, 2 ** 31):
        add((POOL, GROUPED), ValueError, "pool_rows: n_genes, the rows and the groups must each be below 2^31",
            lambda o, n_genes=n_genes: dict(n_genes=n_genes))
    for cells in (-1, 257):
        add((POOL, GROUPED), ValueError, f"pool_rows: cells_per_unit = {cells} must be in [0, 256]", lambda o, cells=cells: dict(cells_per_unit=cells))
    for slab in (-1, 16385):
        add((POOL, GROUPED, SOUP), ValueError, f"{{name}}: slab_genes = {slab} must be in [0, 16384]", lambda o, slab=slab: dict(slab_genes=slab))
    add((POOL, GROUPED), ValueError, "pool_rows: max_bytes = 0 must be positive", lambda o: dict(max_bytes=0))
    # soup_rows
    add((SOUP,), ValueError, "soup_rows: n_add must be int64 [2]", lambda o: dict(n_add=o.n_add.to(torch.int32)))
    add((SOUP,), ValueError, "soup_rows: n_add must be int64 [2]", lambda o: dict(n_add=o.i64(1)))
    vector = "soup_rows: cdf must be an int64 vector [n_genes + 2]"
    add((SOUP,), ValueError, vector, lambda o: dict(cdf=o.cdf.double()))
    add((SOUP,), ValueError, vector, lambda o: dict(cdf=o.cdf[:1]))
    add((SOUP,), ValueError, vector, lambda o: dict(cdf=o.cdf.reshape(1, 7)))
    add((SOUP,), ValueError, "soup_rows: the profile's total weight cdf[-1] must be in (0, 2^63)", lambda o: dict(cdf=torch.zeros_like(o.cdf)))
    add((SOUP,), ValueError, "soup_rows: n_draws = 0 must be >= 1", lambda o: dict(n_draws=0))
    add((SOUP,), ValueError, "soup_rows: row0 and draw0 must not be negative", lambda o: dict(row0=-1))
    add((SOUP,), ValueError, "soup_rows: row0 and draw0 must not be negative", lambda o: dict(draw0=-1))
    # the status word: one malformed operand per bit, skipped by the kernels and reported after the fill pass
    beyond = lambda o: dict(rowptr=o.i32(0, 1, 8))                            # the second cell's row runs past col / cnt
    status = {
        (PAIR, _lib.PAIR_BAD_INDEX): lambda o: dict(b=o.i32(1, B)),
        (PAIR, _lib.PAIR_UNSORTED): lambda o: dict(col=o.i32(4, 2, 0)),
        (PAIR, _lib.PAIR_BAD_ROWPTR): beyond,
        (GROUPED, _lib.POOL_BAD_INDEX): lambda o: dict(members=o.i32(0, B)),
        (GROUPED, _lib.POOL_BAD_ROWPTR): beyond,
        (GROUPED, _lib.POOL_BAD_COL): lambda o: dict(n_genes=G - 1),
        (POOL, _lib.POOL_BAD_ROWPTR): beyond,
        (POOL, _lib.POOL_BAD_COL): lambda o: dict(col=o.i32(4, -3, 2)),
        (SOUP, _lib.SOUP_BAD_ROWPTR): beyond,
        (SOUP, _lib.SOUP_BAD_COL): lambda o: dict(col=o.i32(G, 0, 2)),
        (SOUP, _lib.SOUP_BAD_ADD): lambda o: dict(n_add=o.i64(-1, 2)),
    }
    tables = {PAIR: ops._PAIR_STATUS, GROUPED: ops._POOL_STATUS, POOL: ops._POOL_STATUS, SOUP: ops._SOUP_STATUS}
    for fn in (PAIR, GROUPED, SOUP):
        assert {bit for f, bit in status if f == fn} == {bit for bit, _ in tables[fn]}      # every bit of the table has its case
    for (fn, bit), change in status.items():
        add((fn,), WgnnError, "{name}: " + dict(tables[fn])[bit], change)
    return rows


CASES = _cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i}-{c[0]}-{(c[2] or 'passes')[:40]}" for i, c in enumerate(CASES)])
def test_refusal_class_and_message(i):
    fn, error, fragment, change = CASES[i]
    o = _operands()
    kw = {**_base(fn, o), **change(o)}
    if error is None:
        out = getattr(ops, fn)(**kw)
        assert out[0].dtype == torch.int64 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
        return
    with pytest.raises((ValueError, WgnnError)) as e:
        getattr(ops, fn)(**kw)
    assert type(e.value) is error, (type(e.value), str(e.value))
    if error is WgnnError:
        assert str(e.value) == fragment                                       # the one bit's text, nothing else
    else:
        assert fragment in str(e.value)
