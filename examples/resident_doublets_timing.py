"""Timing of ResidentPredictor.doublets, of the pair merge inside it, of the classify launches it feeds and of the host route
it replaces (profiles/resident_doublets.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model).  Batches of B in {2 000, 20 000} cells of raw counts over the caller's own 30 000 columns - the bundle's 20 000 genes
and 10 000 columns outside it, 800 expressed bundle genes and 80 outside columns per cell, counts geometric with mean 2.5 and
one gene in 200 a hundred times deeper - and 16 partners per cell.  Per B, in one process, the calls ALTERNATING inside every
repetition:
  doublets  - ResidentPredictor.doublets(counts, genes, normalize="lognorm", n_partners=16): the whole call
  pair_rows - its merge alone: ops.pair_rows on the same operands and pairs, chunk by chunk as doublets cuts them
  classify  - the floor the merge adds to: classify of the B x 16 merged rows, already on the device, chunk by chunk
  host      - the route doublets replaces: per draw the two scipy count matrices added on the host, the sum uploaded and
              classify(..., normalize="lognorm")
  wall ms: perf_counter around the call until the device is idle; median and min .. max of `reps` after 1 warm-up round.

    python examples/resident_doublets_timing.py --out profiles/resident_doublets.json [--batches 2000]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle      # noqa: E402
import resident_thin_timing as thin_timing                     # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import api, ops                            # noqa: E402

N_PARTNERS, N_OUTSIDE = 16, 10_000


def timed_alternating(fns, reps):
    """Wall ms per call as (median, min, max), the calls taking turns inside every repetition."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    thin_timing.N_OUTSIDE = N_OUTSIDE                              # count_batch's columns outside the bundle
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, n_partners=N_PARTNERS),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        genes = rp.gene_map(list(rp.id2gene) + [f"Outside{i}" for i in range(N_OUTSIDE)])
        for B in args.batches:
            host = thin_timing.count_batch(B, 100 + B)
            batch = tuple(torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
            db = rp.doublets(batch, genes, normalize="lognorm", n_partners=N_PARTNERS, seed=1)
            # the operands and chunks doublets works on, for the shares timed alone
            with torch.no_grad():
                (rowptr, col, cnt), _, lib, *_ = rp._count_batch(batch, genes, api.LogNormalize(), "doublets", full_call=False)
            a = torch.arange(B, dtype=torch.int32, device="cuda").repeat_interleave(N_PARTNERS)
            b = torch.from_numpy(db.partner.ravel()).cuda()
            lens = (rowptr[1:] - rowptr[:-1])
            bound = torch.cumsum((lens[a.long()] + lens[b.long()]) * 8, 0).cpu().numpy()
            cuts = [0]
            while cuts[-1] < B * N_PARTNERS:
                done = int(bound[cuts[-1] - 1]) if cuts[-1] else 0
                cuts.append(max(cuts[-1] + 1, int(np.searchsorted(bound, done + api.DOUBLETS_CHUNK_BYTES, side="right"))))
            merge = lambda: [ops.pair_rows(rowptr, col, cnt, lib, a[s:e], b[s:e]) for s, e in zip(cuts, cuts[1:])]
            merged = merge()

            def host_route():
                for d in range(N_PARTNERS):
                    rp.classify((host + host[db.partner[:, d]]).tocsr(), genes=genes, normalize="lognorm")

            fns = {"doublets": lambda: rp.doublets(batch, genes, normalize="lognorm", n_partners=N_PARTNERS, seed=1),
                   "pair_rows": merge,
                   "classify": lambda: [rp.classify(m) for m in merged],
                   "host": host_route}
            timed_alternating(fns, 1)                                # warm-up
            ms = timed_alternating(fns, args.reps)
            row = dict(batch=B, pairs=B * N_PARTNERS, chunks=len(cuts) - 1, nnz=int(host.nnz),
                       merged_nnz=int(sum(int(m[1].shape[0]) for m in merged)),
                       **{f"{k}_wall_ms": dict(median=v[0], min=v[1], max=v[2]) for k, v in ms.items()},
                       pair_rows_over_classify=ms["pair_rows"][0] / ms["classify"][0],
                       doublets_over_host=ms["doublets"][0] / ms["host"][0],
                       caught=db.caught(), heterotypic=int(db.summary()["n_heterotypic"]),
                       identical_bits_twice=bool(np.array_equal(db.draw_prob, fns["doublets"]().draw_prob)))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            del batch, merged
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
