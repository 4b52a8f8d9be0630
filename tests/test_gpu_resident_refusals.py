"""What ``ops.predict_rows``, ``predict_rows_dropout``, ``predict_rows_thin`` and ``attrib_rows`` refuse before any launch: the
exception class exactly (``predict_rows_thin``'s own argument checks are ``ValueError``; the table, alpha and CSR checks it
shares with the others, and everything in the other three, ``WgnnError``) and a fragment of the message that tells the check.
One table; the operands are the smallest that reach every branch: 2 cells with 1 and 2 entries, 5 genes, H = 8, 3 classes,
2 draws.  The tensors live on the GPU because the wrappers refuse CPU tensors first."""
import functools
from types import SimpleNamespace

import pytest
import torch

from scdeepsort_amd import WgnnError, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, G, H, C, D, NNZ = 2, 5, 8, 3, 2, 3
BIG_C = ops.HEAD_LDS_BYTES // (4 * H) + 1              # the first head [C, H] beyond what the kernels stage in LDS

PREDICT, DROPOUT, THIN, ATTRIB = "predict_rows", "predict_rows_dropout", "predict_rows_thin", "attrib_rows"
ALL = (PREDICT, DROPOUT, THIN, ATTRIB)
DRAWS = (DROPOUT, THIN)


@functools.lru_cache(maxsize=1)
def _operands():
    g = torch.Generator().manual_seed(11)
    r = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    o = SimpleNamespace(
        rowptr=torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV), col=torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV),
        raw=torch.tensor([1.0, 2.0, 3.0], device=DEV), table=r(G, H), alpha=r(G + 2), bias=r(H), head=(r(C, H), r(C)),
        big_head=(r(BIG_C, H), r(BIG_C)), rest=torch.zeros(B, dtype=torch.int64, device=DEV), direction=r(B, H),
        votes=i32(B, C), unsure=i32(B), empty=i32(B), conf=torch.zeros(B, dtype=torch.float64, device=DEV),
        draw_label=i32(B, D), draw_prob=torch.zeros(B, D, device=DEV), f32=lambda *shape: torch.zeros(*shape, device=DEV), i32=i32)
    o.tabs = (o.votes, o.unsure, o.empty, o.conf)
    return o


def _base(fn, o):
    kw = dict(rowptr=o.rowptr, col=o.col, raw=o.raw, table=o.table, alpha=o.alpha, bias=o.bias)
    if fn in DRAWS:
        kw.update(n_draws=D, keep=0.5, seed=3)
    if fn == THIN:
        kw.update(rest=o.rest)
    if fn == ATTRIB:
        kw.update(head=o.head)
    return kw


def _tabs(o, **swap):
    """the six draw outputs with some of them swapped"""
    names = ("votes", "unsure", "empty", "conf", "draw_label", "draw_prob")
    return tuple(swap.get(n, getattr(o, n)) for n in names)


OWN, SHARED, PASSES = "own", "shared", "passes"        # a wrapper's own check | one all four share | no refusal


def _cases():
    rows = []

    def add(fns, kind, fragment, change):
        rows.extend((fn, kind, fragment, change) for fn in fns)

    # the table, alpha and CSR checks all four share
    add(ALL, SHARED, "table must be [G, >= 8]", lambda o: dict(table=o.table[:, :4]))
    add(ALL, SHARED, "table must be [G, >= 8]", lambda o: dict(table=o.table[0]))
    add(ALL, SHARED, "alpha has 6 entries, the table 5 rows (want G + 2)", lambda o: dict(alpha=o.alpha[:-1]))
    add(ALL, SHARED, "col has 3 entries, raw 2", lambda o: dict(raw=o.raw[:2]))
    add(ALL, SHARED, "takes rowptr int32 / int64, col int32, raw float32", lambda o: dict(rowptr=o.rowptr.to(torch.int16)))
    add(ALL, SHARED, "takes rowptr int32 / int64, col int32, raw float32", lambda o: dict(col=o.col.long()))
    add(ALL, SHARED, "takes rowptr int32 / int64, col int32, raw float32", lambda o: dict(raw=o.raw.double()))
    add(ALL, SHARED, "gene id out of range [0, 5) in the batch's CSR (min -1, max 2)",
        lambda o: dict(col=torch.tensor([-1, 0, 2], dtype=torch.int32, device=DEV)))
    add(ALL, SHARED, "gene id out of range [0, 5) in the batch's CSR (min 0, max 5)",
        lambda o: dict(col=torch.tensor([5, 0, 2], dtype=torch.int32, device=DEV)))
    # ... an empty batch whose CSR arrays still hold an id: refused with check_cols, never read by a launch without
    empty = lambda o, **kw: dict(rowptr=o.rowptr[:1], col=o.col[:1] + G, raw=o.raw[:1], rest=o.rest[:0], **kw)
    add((PREDICT, DROPOUT, ATTRIB), SHARED, "gene id out of range [0, 5)", lambda o: {k: v for k, v in empty(o).items() if k != "rest"})
    add((THIN,), SHARED, "gene id out of range [0, 5)", lambda o: empty(o))
    add((PREDICT, DROPOUT, ATTRIB), PASSES, None, lambda o: {k: v for k, v in empty(o, check_cols=False).items() if k != "rest"})
    add((THIN,), PASSES, None, lambda o: empty(o, check_cols=False))
    # the self rows
    add((PREDICT, ATTRIB), OWN, "self_rows has 3 rows, the batch 2", lambda o: dict(self_rows=o.f32(3, H)))
    add(DRAWS, OWN, "self_rows has 3 rows, the batch 2 cells x 2 draws", lambda o: dict(self_rows=o.f32(3, H)))
    add(DRAWS, OWN, "self_rows has 2 rows, the batch 2 cells x 2 draws", lambda o: dict(self_rows=o.f32(B, H)))
    # the draws
    add(DRAWS, OWN, "n_draws = 0 must be >= 1", lambda o: dict(n_draws=0))
    for keep in (-0.1, 1.5, float("nan")):
        add(DRAWS, OWN, f"keep = {keep} must be in [0, 1]", lambda o, keep=keep: dict(keep=keep))
    add(DRAWS, OWN, "row0 and draw0 must not be negative", lambda o: dict(row0=-1))
    add(DRAWS, OWN, "row0 and draw0 must not be negative", lambda o: dict(draw0=-1))
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        add((THIN,), OWN, f"scale = {scale} must be positive and finite", lambda o, scale=scale: dict(scale=scale))
    for thr in (-0.5, float("nan")):
        add((THIN,), OWN, f"threshold = {thr} must be >= 0", lambda o, thr=thr: dict(threshold=thr))
    add((THIN,), OWN, "rest must be int64 [2]", lambda o: dict(rest=torch.zeros(3, dtype=torch.int64, device=DEV)))
    add((THIN,), OWN, "rest must be int64 [2]", lambda o: dict(rest=o.rest.to(torch.int32)))
    add((THIN,), OWN, "rest must be int64 [2]", lambda o: dict(rest=o.rest.double()))
    # without a head
    add(DRAWS, OWN, "accumulate and want_draws need a head", lambda o: dict(accumulate=True))
    add(DRAWS, OWN, "accumulate and want_draws need a head", lambda o: dict(want_draws=True))
    headless = "out must be float32 [4, 8], unit column stride, 16-byte aligned rows"
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D, H).double()))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D + 1, H)))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D, H + 4)))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D, 2 * H)[:, ::2]))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D, H + 1)[:, :H]))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.f32(B * D * H + 1)[1:].view(B * D, H)))
    add(DRAWS, OWN, headless, lambda o: dict(out=o.tabs))
    # with a head
    add(DRAWS, OWN, "accumulate needs the tables to add to (out=)", lambda o: dict(head=o.head, accumulate=True))
    wrong_len = "out must be (votes, unsure, empty, conf_sum[, draw_label, draw_prob])"
    add(DRAWS, OWN, wrong_len, lambda o: dict(head=o.head, out=o.tabs[:3]))
    add(DRAWS, OWN, wrong_len, lambda o: dict(head=o.head, out=_tabs(o)[:5]))
    votes = "votes must be int32 [2, 3] with unit column stride and a row stride >= 3"
    add(DRAWS, OWN, votes, lambda o: dict(head=o.head, out=_tabs(o, votes=o.votes.long())[:4]))
    add(DRAWS, OWN, votes, lambda o: dict(head=o.head, out=_tabs(o, votes=o.i32(B, C + 1))[:4]))
    add(DRAWS, OWN, votes, lambda o: dict(head=o.head, out=_tabs(o, votes=o.i32(B, 2 * C)[:, ::2])[:4]))
    add(DRAWS, OWN, votes, lambda o: dict(head=o.head, out=_tabs(o, votes=o.i32(1, C).expand(B, C))[:4]))
    per_cell = "unsure and empty must be contiguous int32 [2], conf_sum float64 [2]"
    for name in ("unsure", "empty"):
        add(DRAWS, OWN, per_cell, lambda o, name=name: dict(head=o.head, out=_tabs(o, **{name: o.i32(B).long()})[:4]))
        add(DRAWS, OWN, per_cell, lambda o, name=name: dict(head=o.head, out=_tabs(o, **{name: o.i32(B + 1)})[:4]))
        add(DRAWS, OWN, per_cell, lambda o, name=name: dict(head=o.head, out=_tabs(o, **{name: o.i32(2 * B)[::2]})[:4]))
    add(DRAWS, OWN, per_cell, lambda o: dict(head=o.head, out=_tabs(o, conf=o.f32(B))[:4]))
    add(DRAWS, OWN, per_cell, lambda o: dict(head=o.head, out=_tabs(o, conf=o.conf.new_zeros(B + 1))[:4]))
    add(DRAWS, OWN, per_cell, lambda o: dict(head=o.head, out=_tabs(o, conf=o.conf.new_zeros(2 * B)[::2])[:4]))
    per_draw = "draw_label / draw_prob must be contiguous int32 / float32 [2, 2]"
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_label=o.draw_label.long())))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_label=o.i32(B, D + 1))))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_label=o.i32(B, 2 * D)[:, ::2])))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_prob=o.draw_prob.double())))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_prob=o.f32(B + 1, D))))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_prob=o.f32(B, 2 * D)[:, ::2])))
    add(DRAWS, OWN, per_draw, lambda o: dict(head=o.head, out=_tabs(o, draw_prob=None)))
    # a head beyond what the kernels stage in LDS (predict_rows takes the GEMM route instead: its own test below)
    add(DRAWS, OWN, f"a [{BIG_C}, 8] head is beyond the 65536 bytes the kernel stages", lambda o: dict(head=o.big_head))
    add((ATTRIB,), OWN, f"a [{BIG_C}, 8] head does not fit the 64 KiB the kernel stages in LDS", lambda o: dict(head=o.big_head))
    # attrib_rows
    either = "attrib_rows takes either head= (last layer) or direction= (layers below it)"
    add((ATTRIB,), OWN, either, lambda o: dict(head=None))
    add((ATTRIB,), OWN, either, lambda o: dict(direction=o.direction))
    scores = "scores must be a contiguous float32 [3]"
    add((ATTRIB,), OWN, scores, lambda o: dict(scores=o.f32(NNZ + 1)))
    add((ATTRIB,), OWN, scores, lambda o: dict(scores=o.f32(NNZ).double()))
    add((ATTRIB,), OWN, scores, lambda o: dict(scores=o.f32(2 * NNZ)[::2]))
    add((ATTRIB,), OWN, scores, lambda o: dict(head=None, direction=o.direction, scores=o.f32(NNZ + 1)))
    add((ATTRIB,), OWN, "accumulate needs the scores to add to", lambda o: dict(accumulate=True))
    add((ATTRIB,), OWN, "accumulate needs the scores to add to", lambda o: dict(head=None, direction=o.direction, accumulate=True))
    add((ATTRIB,), OWN, "head mode overwrites the scores", lambda o: dict(scores=o.f32(NNZ), accumulate=True))
    add((ATTRIB,), OWN, "target must hold one class per cell ([2])", lambda o: dict(target=o.i32(B + 1)))
    add((ATTRIB,), OWN, "target must hold one class per cell ([2])", lambda o: dict(target=o.i32(B, 1)))
    add((ATTRIB,), OWN, "target class out of range [0, 3) (min -1, max 0)", lambda o: dict(target=o.i32(B) - torch.tensor([1, 0], device=DEV)))
    add((ATTRIB,), OWN, "target class out of range [0, 3) (min 0, max 3)", lambda o: dict(target=o.i32(B) + torch.tensor([0, 3], device=DEV)))
    add((ATTRIB,), OWN, "direction must be [2, >= 8]", lambda o: dict(head=None, direction=o.f32(B + 1, H)))
    add((ATTRIB,), OWN, "direction must be [2, >= 8]", lambda o: dict(head=None, direction=o.f32(B, H - 4)))
    return rows


CASES = _cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i}-{c[0]}-{(c[2] or 'passes')[:40]}" for i, c in enumerate(CASES)])
def test_refusal_class_and_message(i):
    fn, kind, fragment, change = CASES[i]
    o = _operands()
    kw = {**_base(fn, o), **change(o)}
    if kind == PASSES:
        getattr(ops, fn)(**kw)
        return
    want = ValueError if (fn == THIN and kind == OWN) else WgnnError
    with pytest.raises((ValueError, WgnnError)) as e:
        getattr(ops, fn)(**kw)
    assert type(e.value) is want, (type(e.value), str(e.value))
    assert fragment in str(e.value)


def test_predict_rows_runs_a_head_beyond_lds_as_a_gemm():
    o = _operands()
    logits, label, max_prob = ops.predict_rows(o.rowptr, o.col, o.raw, o.table, o.alpha, o.bias, head=o.big_head)
    h = ops.predict_rows(o.rowptr, o.col, o.raw, o.table, o.alpha, o.bias)
    assert logits.shape == (B, BIG_C) and label.dtype == torch.int32
    want = h.double() @ o.big_head[0].double().T + o.big_head[1].double()
    assert float((logits.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    clear = (want.topk(2, dim=1).values.diff(dim=1).abs().squeeze(1) > 1e-4)     # a margin a float32 GEMM cannot flip
    assert torch.equal(label[clear].long(), want.argmax(dim=1)[clear])
    assert torch.equal(max_prob, torch.softmax(logits, dim=1).max(dim=1).values)
