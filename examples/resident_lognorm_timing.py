"""Timing of ResidentPredictor.align(..., normalize="lognorm") against two ways of doing the same without it
(profiles/resident_lognorm.md).

Shape and bundle as examples/resident_align_timing.py, with a wider caller: G = 20 000 bundle genes in a random order plus
10 000 foreign columns - 30 000 columns of which 20 000 map; a cell holds raw counts on 800 bundle genes and about 400 foreign
ones.  Batches of B in {200, 2 000, 20 000}, as a DENSE float32 device matrix and as a device CSR over the caller's columns.
Per (form, B), in one process, the calls ALTERNATING inside every repetition:
  host      - (a) numpy / scipy on the host: fp64 row totals, log1p(x / total * 1e4), float32; the upload; align
  framework - (b) framework ops on the device: fp64 row sum, divide, scale, log1p, cast to float32 (a normalised [B, n_cols]
              matrix, or a normalised value array for the CSR form); align
  fused     - (c) align(batch, gene_map, normalize="lognorm"): wgnn_align_count_ln (which sums the rows), cumsum, read-back,
              wgnn_align_fill_ln, status read-back
  wall_ms: host clock around the call, ending in a device synchronise; median, minimum and maximum of `reps` (default 20)
  after a warm-up.
`kernel`: each kernel alone between HIP events, and the bytes it must read over that time.

    python examples/resident_lognorm_timing.py --out profiles/resident_lognorm.json [--batches 200 2000]
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

N_FOREIGN, FOREIGN_PER_CELL, SCALE = G // 2, PER_CELL // 2, 1e4


def callers_counts(B, seed):
    """(dense [B, G + N_FOREIGN] f32 raw counts on the host, gene ids of the columns with -1 = foreign)."""
    rng = np.random.default_rng(seed)
    n_cols = G + N_FOREIGN
    ids = np.full(n_cols, -1, np.int32)
    ids[rng.permutation(n_cols)[:G]] = rng.permutation(G).astype(np.int32)
    where = np.empty(G, np.int64)
    where[ids[ids >= 0]] = np.flatnonzero(ids >= 0)                  # bundle gene -> caller's column
    own = expression(B, seed)
    x = np.zeros((B, n_cols), np.float32)
    rows = np.repeat(np.arange(B), np.diff(own.indptr))
    x[rows, where[own.indices]] = 1 + rng.poisson(1.5, own.nnz)
    foreign = np.flatnonzero(ids < 0)
    fr = np.repeat(np.arange(B), FOREIGN_PER_CELL)
    x[fr, foreign[rng.integers(0, len(foreign), fr.shape[0])]] = 1 + rng.poisson(1.5, fr.shape[0])
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
    return {name: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for name, v in ms.items()}


def kernel_ms(batch, gmap, out, thr, reps=10):
    """Device ms of one launch of each kernel (HIP events around `reps` launches)."""
    dev = gmap.device
    dense = isinstance(batch, torch.Tensor)
    B = batch.shape[0] if dense else batch[0].shape[0] - 1
    x, ld, (rowptr, col, val) = (batch, batch.stride(0), (None, None, None)) if dense else (None, 0, batch)
    flags = 0 if dense or rowptr.dtype == torch.int32 else _lib.FLAG_ROWPTR_I64
    head = (_ptr(x), ld, _ptr(rowptr), _ptr(col), _ptr(val), B, gmap.shape[0], _ptr(gmap), G, float(thr))
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    total = torch.empty(B, dtype=torch.float64, device=dev)
    o_rowptr, o_col, o_raw = out[0], torch.empty_like(out[1]), torch.empty_like(out[2])
    s = _stream(dev)
    calls = {"count_ln": lambda: _lib.call(dev, "wgnn_align_count_ln", *head, None, _ptr(total), SCALE, _ptr(counts), _ptr(status),
                                           flags, s),
             "fill_ln": lambda: _lib.call(dev, "wgnn_align_fill_ln", *head, _ptr(total), SCALE, _ptr(o_rowptr), _ptr(o_col),
                                          _ptr(o_raw), _ptr(status), flags, s),
             "count": lambda: _lib.call(dev, "wgnn_align_count", *head, _ptr(counts), _ptr(status), flags, s)}
    ms = {}
    for name, fn in calls.items():
        fn()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            assert fn() == 0
        e.record()
        torch.cuda.synchronize()
        ms[name] = a.elapsed_time(e) / reps
    assert int(status) == 0 and torch.equal(o_col, out[1]) and torch.equal(o_raw, out[2])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, foreign_columns=N_FOREIGN, kept_per_cell=PER_CELL, foreign_per_cell=FOREIGN_PER_CELL,
                          hidden=HIDDEN, classes=N_CLS, layers=1), device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td)
        thr = float(rp.threshold)
        for B in args.batches:
            x_host, ids = callers_counts(B, 100 + B)
            gmap = torch.from_numpy(ids).cuda()
            x_dev = torch.from_numpy(x_host).cuda()
            csr_host = sp.csr_matrix(x_host)
            csr_dev = (torch.from_numpy(csr_host.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr_host.indices).cuda(),
                       torch.from_numpy(csr_host.data).cuda())
            row_of = torch.repeat_interleave(torch.arange(B, device="cuda"), csr_dev[0][1:] - csr_dev[0][:-1])

            def host_dense():
                total = x_host.sum(axis=1, dtype=np.float64)
                v = np.log1p(x_host / total[:, None] * SCALE).astype(np.float32)
                return rp.align(torch.from_numpy(v).cuda(), gmap)

            def host_csr():
                total = np.asarray(csr_host.sum(axis=1, dtype=np.float64)).ravel()
                v = np.log1p(csr_host.data / np.repeat(total, np.diff(csr_host.indptr)) * SCALE).astype(np.float32)
                return rp.align((torch.from_numpy(csr_host.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr_host.indices).cuda(),
                                 torch.from_numpy(v).cuda()), gmap)

            def framework_dense():
                total = x_dev.sum(dim=1, dtype=torch.float64)
                return rp.align(torch.log1p(x_dev.double() / total[:, None] * SCALE).float(), gmap)

            def framework_csr():
                rowptr, col, val = csr_dev
                total = torch.zeros(B, dtype=torch.float64, device=val.device).index_add_(0, row_of, val.double())
                return rp.align((rowptr, col, torch.log1p(val.double() / total[row_of] * SCALE).float()), gmap)

            for form, batch, host, framework in (("dense", x_dev, host_dense, framework_dense),
                                                 ("csr", csr_dev, host_csr, framework_csr)):
                out = rp.align(batch, gmap, normalize="lognorm")
                differ = {}
                for name, other in (("host", host()), ("framework", framework())):
                    assert torch.equal(other[0], out[0]) and torch.equal(other[1], out[1])
                    off = (other[2].view(torch.int32) - out[2].view(torch.int32)).abs()
                    assert int(off.max()) <= 1                   # another log1p: the last float32 bit of a few values
                    differ[name] = int((off != 0).sum())
                del other, off
                fns = {"host": host, "framework": framework, "fused": lambda: rp.align(batch, gmap, normalize="lognorm")}
                timed_alternating(fns, 1)                        # warm-up
                ms = timed_alternating(fns, args.reps)
                k = kernel_ms(batch, gmap, out, thr)
                read = x_dev.numel() * 4 if form == "dense" else csr_host.nnz * 8 + (B + 1) * 8
                row = dict(form=form, batch=B, columns=int(x_host.shape[1]), stored=int(csr_host.nnz), kept=int(out[1].shape[0]),
                           **{f"{n}_wall_ms": v["median"] for n, v in ms.items()},
                           **{f"{n}_wall_ms_min_max": [v["min"], v["max"]] for n, v in ms.items()},
                           **{f"{n}_kernel_ms": v for n, v in k.items()},
                           bytes_read_per_pass=int(read), values_differing_from_fused=differ,
                           fused_over_host=ms["fused"]["median"] / ms["host"]["median"],
                           fused_over_framework=ms["fused"]["median"] / ms["framework"]["median"])
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
            del x_dev, csr_dev, out, row_of
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
