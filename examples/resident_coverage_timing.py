"""Timing of ResidentPredictor.coverage against align(..., normalize="lognorm") of the same batch and against the same six
outputs composed of framework ops (profiles/resident_coverage.md).

Shape, bundle and batches as examples/resident_lognorm_timing.py: 30 000 caller columns of which 20 000 map, a cell holds raw
counts on 800 bundle genes and about 400 foreign ones; B in {200, 2 000, 20 000}, as a DENSE float32 device matrix and as a
device CSR over the caller's columns.  Per (form, B), in one process, the calls ALTERNATING inside every repetition:
  coverage  - rp.coverage(batch, gene_map): wgnn_coverage_rows (the row walk; for the dense form the column walk too), the status
              read-back and the five per-cell vectors and the gene map copied to the host
  lognorm   - rp.align(batch, gene_map, normalize="lognorm"): what a caller runs next on the same batch
  framework - the six outputs from framework ops on the device: (x > 0) & isfinite, masked sums in fp64, sum(0); the five
              per-cell vectors copied to the host as coverage does
  wall_ms: host clock around the call, ending in a device synchronise; median, minimum and maximum of `reps` (default 20)
  after a warm-up.
`coverage_kernel_ms`: ops.coverage_rows alone between HIP events (the entry point's launches and the status read-back), and
the bytes it must read over that time (dense: the matrix twice).

    python examples/resident_coverage_timing.py --out profiles/resident_coverage.json [--batches 200 2000]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle                    # noqa: E402
from resident_lognorm_timing import FOREIGN_PER_CELL, N_FOREIGN, callers_counts, timed_alternating      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import ops                                 # noqa: E402


def framework_dense(x, gmap):
    on = (x > 0) & torch.isfinite(x)
    m = (gmap >= 0)[None, :]
    xo = torch.where(on, x, 0.0)
    return (on.sum(1, dtype=torch.int32), (on & m).sum(1, dtype=torch.int32), ((x < 0) | ~torch.isfinite(x)).sum(1, dtype=torch.int32),
            xo.sum(1, dtype=torch.float64), torch.where(m, xo, 0.0).sum(1, dtype=torch.float64), on.sum(0, dtype=torch.int32))


def framework_csr(csr, row_of, gmap):
    rowptr, col, val = csr
    B = rowptr.shape[0] - 1
    on = (val > 0) & torch.isfinite(val)
    m = on & (gmap[col.long()] >= 0)
    bad = (val < 0) | ~torch.isfinite(val)
    v = torch.where(on, val, 0.0).double()

    def per_row(w, dtype):
        return torch.zeros(B, dtype=dtype, device=val.device).index_add_(0, row_of, w)

    return (per_row(on.int(), torch.int32), per_row(m.int(), torch.int32), per_row(bad.int(), torch.int32),
            per_row(v, torch.float64), per_row(torch.where(m, v, 0.0), torch.float64),
            torch.bincount(col[on].long(), minlength=gmap.shape[0]).int())


def to_host(outs):
    return [o.cpu() for o in outs[:5]]


def coverage_kernel_ms(batch, gmap, reps=10):
    fn = lambda: ops.coverage_rows(batch, gmap, G)
    fn()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()                                                     # ends in the status read-back: launches do not pile up
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / reps


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
        for B in args.batches:
            x_host, ids = callers_counts(B, 100 + B)
            gmap = torch.from_numpy(ids).cuda()
            x_dev = torch.from_numpy(x_host).cuda()
            csr_host = sp.csr_matrix(x_host)
            csr_dev = (torch.from_numpy(csr_host.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr_host.indices).cuda(),
                       torch.from_numpy(csr_host.data).cuda())
            row_of = torch.repeat_interleave(torch.arange(B, device="cuda"), csr_dev[0][1:] - csr_dev[0][:-1])
            for form, batch, framework in (("dense", x_dev, lambda: framework_dense(x_dev, gmap)),
                                           ("csr", csr_dev, lambda: framework_csr(csr_dev, row_of, gmap))):
                got = ops.coverage_rows(batch, gmap, G)
                other = framework()
                for k in (0, 1, 2, 5):
                    assert torch.equal(got[k], other[k]), k
                for k in (3, 4):                                 # another order of addition: the last bits
                    assert torch.allclose(got[k], other[k], rtol=1e-12, atol=0), k
                again = ops.coverage_rows(batch, gmap, G)
                assert all(torch.equal(a, b) for a, b in zip(got, again))
                cov = rp.coverage(batch, gmap)
                del other, again
                fns = {"coverage": lambda: rp.coverage(batch, gmap), "lognorm": lambda: rp.align(batch, gmap, normalize="lognorm"),
                       "framework": lambda: to_host(framework())}
                timed_alternating(fns, 1)                        # warm-up
                ms = timed_alternating(fns, args.reps)
                k_ms = coverage_kernel_ms(batch, gmap)
                read = 2 * x_dev.numel() * 4 if form == "dense" else csr_host.nnz * 8 + (B + 1) * 8
                row = dict(form=form, batch=B, columns=int(x_host.shape[1]), stored=int(csr_host.nnz),
                           median_fraction_counts=float(np.median(cov.fraction_counts())),
                           **{f"{n}_wall_ms": v["median"] for n, v in ms.items()},
                           **{f"{n}_wall_ms_min_max": [v["min"], v["max"]] for n, v in ms.items()},
                           coverage_kernel_ms=k_ms, bytes_read=int(read), read_GB_per_s=read / k_ms / 1e6,
                           coverage_over_lognorm=ms["coverage"]["median"] / ms["lognorm"]["median"],
                           coverage_over_framework=ms["coverage"]["median"] / ms["framework"]["median"])
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
            del x_dev, csr_dev, row_of, got
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
