"""Timing of ResidentPredictor.align against two ways of doing the same without it (profiles/resident_align.md).

Shape and bundle as examples/resident_predict_timing.py: G = 20 000 bundle genes, 800 expressed genes per cell, hidden 200,
16 classes, one layer.  The caller's matrix has the bundle's genes in a random order plus 25 % foreign columns (5 000, each
cell expressing about 200 of them): 25 000 columns, about 800 kept per cell.  Batches of B in {200, 2 000, 20 000}, as a DENSE
float32 device matrix and as a device CSR over the caller's columns.  Per (form, B), in one process, the calls ALTERNATING
inside every repetition:
  align    - ResidentPredictor.align(batch, gene_map): wgnn_align_count, cumsum, read-back, wgnn_align_fill, status read-back
  host     - (a) the tail of api._read_test_csr as it stands, from the same matrix on the host: column select, np.nonzero of
             `> threshold`, sp.csr_matrix, and the upload of the three arrays (for the CSR form: the same selection on a
             scipy COO).  What a user writes today.
  framework- (b) the same triple from framework ops on the device: mask, nonzero, gather, bincount, cumsum
  classify - the call that follows: ResidentPredictor.classify on the aligned triple
  wall_ms: host clock around the call, ending in a device synchronise; median of `reps` after a warm-up.
`kernel`: wgnn_align_count and wgnn_align_fill alone between HIP events, and the bytes they must read (dense: the matrix,
once per pass) over that time.

    python examples/resident_align_timing.py --out profiles/resident_align.json [--batches 200 2000]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, expression, write_bundle      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import _lib                                # noqa: E402
from scdeepsort_amd.graph import _ptr, _stream                 # noqa: E402

N_FOREIGN, FOREIGN_PER_CELL = G // 4, PER_CELL // 4


def callers_matrix(B, seed):
    """(dense [B, G + N_FOREIGN] f32 on the host, gene ids of the columns with -1 = foreign)."""
    rng = np.random.default_rng(seed)
    n_cols = G + N_FOREIGN
    ids = np.full(n_cols, -1, np.int32)
    ids[rng.permutation(n_cols)[:G]] = rng.permutation(G).astype(np.int32)
    where = np.empty(G, np.int64)
    where[ids[ids >= 0]] = np.flatnonzero(ids >= 0)                  # bundle gene -> caller's column
    own = expression(B, seed)
    x = np.zeros((B, n_cols), np.float32)
    rows = np.repeat(np.arange(B), np.diff(own.indptr))
    x[rows, where[own.indices]] = own.data
    foreign = np.flatnonzero(ids < 0)
    fr = np.repeat(np.arange(B), FOREIGN_PER_CELL)
    x[fr, foreign[rng.integers(0, len(foreign), fr.shape[0])]] = rng.uniform(0.5, 5.0, fr.shape[0]).astype(np.float32)
    return x, ids


def timed_alternating(fns, reps):
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: float(np.median(v)) for name, v in ms.items()}


def kernel_ms(batch, gmap, out, thr, reps=10):
    """Device ms of one wgnn_align_count and one wgnn_align_fill launch (HIP events around `reps` launches each)."""
    dev = gmap.device
    dense = isinstance(batch, torch.Tensor)
    B = batch.shape[0] if dense else batch[0].shape[0] - 1
    x, ld, (rowptr, col, val) = (batch, batch.stride(0), (None, None, None)) if dense else (None, 0, batch)
    flags = 0 if dense or rowptr.dtype == torch.int32 else _lib.FLAG_ROWPTR_I64
    head = (_ptr(x), ld, _ptr(rowptr), _ptr(col), _ptr(val), B, gmap.shape[0], _ptr(gmap), G, float(thr))
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    o_rowptr, o_col, o_raw = out[0], torch.empty_like(out[1]), torch.empty_like(out[2])
    calls = {"count": lambda: _lib.call(dev, "wgnn_align_count", *head, _ptr(counts), _ptr(status), flags, _stream(dev)),
             "fill": lambda: _lib.call(dev, "wgnn_align_fill", *head, _ptr(o_rowptr), _ptr(o_col), _ptr(o_raw), _ptr(status),
                                       flags, _stream(dev))}
    ms = {}
    for name, fn in calls.items():
        fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            assert fn() == 0
        e.record()
        torch.cuda.synchronize()
        ms[name] = s.elapsed_time(e) / reps
    assert int(status) == 0 and torch.equal(o_col, out[1]) and torch.equal(o_raw, out[2])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, foreign_columns=N_FOREIGN, kept_per_cell=PER_CELL, foreign_per_cell=FOREIGN_PER_CELL,
                          hidden=HIDDEN, classes=N_CLS, layers=1), device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td)
        thr = float(rp.threshold)
        for B in args.batches:
            x_host, ids = callers_matrix(B, 100 + B)
            names = [rp.id2gene[g] if g >= 0 else f"Foreign{j}" for j, g in enumerate(ids)]
            gmap = rp.gene_map(names)
            assert gmap.cpu().numpy().tolist() == ids.tolist()
            sel = np.flatnonzero(ids >= 0)
            x_dev = torch.from_numpy(x_host).cuda()
            csr_host = sp.csr_matrix(x_host)
            csr_dev = (torch.from_numpy(csr_host.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr_host.indices).cuda(),
                       torch.from_numpy(csr_host.data).cuda())
            up = lambda m: (torch.from_numpy(m.indptr).cuda(), torch.from_numpy(m.indices).cuda(), torch.from_numpy(m.data).cuda())

            def host_dense():                                    # the tail of api._read_test_csr, then the upload
                arr = x_host[:, sel]
                cid = ids[sel]
                r, c = np.nonzero(arr > thr)
                return up(sp.csr_matrix((arr[r, c], (r, cid[c])), shape=(B, G)))

            def host_csr():
                coo = csr_host.tocoo()
                g = ids[coo.col]
                on = (g >= 0) & (coo.data > thr)
                return up(sp.csr_matrix((coo.data[on], (coo.row[on], g[on])), shape=(B, G)))

            def framework_dense():
                keep = (x_dev > thr) & (gmap >= 0)
                rc = keep.nonzero()                              # row-major: a row's entries in column order
                counts = torch.bincount(rc[:, 0], minlength=B)
                rowptr = torch.zeros(B + 1, dtype=torch.int64, device=x_dev.device)
                torch.cumsum(counts, 0, out=rowptr[1:])
                return rowptr, gmap[rc[:, 1]], x_dev[keep]

            def framework_csr():
                rowptr, col, val = csr_dev
                g = gmap[col.long()]
                keep = (g >= 0) & (val > thr)
                row = torch.repeat_interleave(torch.arange(B, device=col.device), rowptr[1:] - rowptr[:-1])
                counts = torch.bincount(row[keep], minlength=B)
                out = torch.zeros(B + 1, dtype=torch.int64, device=col.device)
                torch.cumsum(counts, 0, out=out[1:])
                return out, g[keep], val[keep]

            for form, batch, host, framework in (("dense", x_dev, host_dense, framework_dense),
                                                 ("csr", csr_dev, host_csr, framework_csr)):
                out = rp.align(batch, gmap)
                for a, b in zip(out, framework()):               # the three routes agree (the host one up to its row order)
                    assert torch.equal(a, b)
                h = host()
                assert torch.equal(h[0].long(), out[0]) and h[1].shape == out[1].shape
                fns = {"align": lambda: rp.align(batch, gmap), "host": host, "framework": framework,
                       "classify": lambda: rp.classify(out)}
                timed_alternating(fns, 1)                        # warm-up
                ms = timed_alternating(fns, args.reps)
                k = kernel_ms(batch, gmap, out, thr)
                read = x_dev.numel() * 4 if form == "dense" else csr_host.nnz * 8 + (B + 1) * 8
                row = dict(form=form, batch=B, columns=int(x_host.shape[1]), stored=int(csr_host.nnz), kept=int(out[1].shape[0]),
                           **{f"{n}_wall_ms": v for n, v in ms.items()}, count_kernel_ms=k["count"], fill_kernel_ms=k["fill"],
                           bytes_read_per_pass=int(read),
                           count_TBps=read / k["count"] / 1e9, fill_TBps=read / k["fill"] / 1e9,
                           align_over_host=ms["align"] / ms["host"], align_over_framework=ms["align"] / ms["framework"])
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
            del x_dev, csr_dev, out
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
