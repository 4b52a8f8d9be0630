"""Timing of ResidentPredictor.pseudobulk, of the pooling inside it and of the two routes a user has without it
(profiles/resident_pseudobulk.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model).  Batches of B in {2 000, 20 000, 100 000} cells of raw counts over the caller's own 30 000 columns - the bundle's 20 000
genes and 10 000 columns outside it, 800 expressed bundle genes and 80 outside columns per cell (the 100 000-cell batch is the
20 000-cell one five times over, the copies in shuffled order) - grouped into 20 clusters (cells dealt at random) and into
metacells of 20 cells (B / 20 groups).  Per (B, grouping), in one process, the calls ALTERNATING inside every repetition:
  pseudobulk - ResidentPredictor.pseudobulk(counts, genes, clusters, normalize="lognorm"): the whole call
  pool_rows  - its pooling alone: ops.pool_rows (wgnn_pool_rows_accumulate / _count / _fill) on the aligned counts
  host       - (a) the host route: a scipy indicator product [K, B] x [B, columns] on the host, the sums uploaded and
               classify(..., normalize="lognorm")
  framework  - (b) framework ops on the device: the bundle's columns scatter-added into a dense fp64 [K, G] (index_add_), the
               library sizes with index_add_, then classify of the float32 matrix with LogNormalize(library_size=...)
  wall ms: perf_counter around the call until the device is idle; median and min .. max of `reps` after 1 warm-up round.

    python examples/resident_pseudobulk_timing.py --out profiles/resident_pseudobulk.json [--batches 2000]
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
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle      # noqa: E402
from resident_doublets_timing import timed_alternating         # noqa: E402
import resident_thin_timing as thin_timing                     # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import api, ops                            # noqa: E402

N_OUTSIDE, N_CLUSTERS, METACELL = 10_000, 20, 20
BASE_CELLS = 20_000


def count_batch(B):
    if B <= BASE_CELLS:
        return thin_timing.count_batch(B, 100 + B)
    base = thin_timing.count_batch(BASE_CELLS, 100 + BASE_CELLS)
    rng = np.random.default_rng(B)
    return sp.vstack([base[rng.permutation(BASE_CELLS)] for _ in range(-(-B // BASE_CELLS))]).tocsr()[:B]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    thin_timing.N_OUTSIDE = N_OUTSIDE                              # count_batch's columns outside the bundle
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, clusters=N_CLUSTERS,
                          metacell=METACELL), device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        genes = rp.gene_map(list(rp.id2gene) + [f"Outside{i}" for i in range(N_OUTSIDE)])
        own = torch.arange(G, dtype=torch.int32, device="cuda")   # the dense [K, G] matrix of route (b) is over the bundle's ids
        for B in args.batches:
            host = count_batch(B)
            batch = tuple(torch.from_numpy(a).cuda() for a in (host.indptr.astype(np.int64), host.indices, host.data))
            rows = torch.repeat_interleave(torch.arange(B, device="cuda"), batch[0][1:] - batch[0][:-1])
            cell_total = torch.zeros(B, dtype=torch.float64, device="cuda").index_add_(0, rows, batch[2].double())
            with torch.no_grad():
                (rowptr, col, cnt), _, lib, *_ = rp._count_batch(batch, genes, api.LogNormalize(), "pseudobulk", full_call=False)
            rng = np.random.default_rng(7)
            for grouping, ids in (("clusters", rng.integers(0, N_CLUSTERS, B)), ("metacells", rng.permutation(B) // METACELL)):
                K = int(ids.max()) + 1
                group = torch.from_numpy(ids.astype(np.int32)).cuda()
                indicator = sp.csr_matrix((np.ones(B, np.float32), (ids, np.arange(B))), shape=(K, B))
                pb = rp.pseudobulk(batch, genes, ids, normalize="lognorm", n_clusters=K)

                def host_route():
                    return rp.classify((indicator @ host).tocsr(), genes=genes, normalize="lognorm")

                def framework_route():
                    g = genes[batch[1].long()].long()
                    on = g >= 0
                    flat = group.long()[rows[on]] * G + g[on]
                    dense = torch.zeros(K * G, dtype=torch.float64, device="cuda").index_add_(0, flat, batch[2][on].double())
                    total = torch.zeros(K, dtype=torch.float64, device="cuda").index_add_(0, group.long(), cell_total)
                    return rp.classify(dense.view(K, G).float(), genes=own, normalize=api.LogNormalize(library_size=total))

                fns = {"pseudobulk": lambda: rp.pseudobulk(batch, genes, ids, normalize="lognorm", n_clusters=K),
                       "pool_rows": lambda: ops.pool_rows(rowptr, col, cnt, lib, group, K, n_genes=G),
                       "host": host_route,
                       "framework": framework_route}
                same = {name: bool(np.array_equal(fn()[0], pb.label)) for name, fn in (("host", host_route), ("framework", framework_route))}
                timed_alternating(fns, 1)                            # warm-up
                ms = timed_alternating(fns, args.reps)
                row = dict(batch=B, grouping=grouping, groups=K, nnz=int(host.nnz), pooled_nnz=int(pb.col.shape[0]),
                           **{f"{k}_wall_ms": dict(median=v[0], min=v[1], max=v[2]) for k, v in ms.items()},
                           pseudobulk_over_host=ms["pseudobulk"][0] / ms["host"][0],
                           pseudobulk_over_framework=ms["pseudobulk"][0] / ms["framework"][0],
                           host_labels_equal=same["host"], framework_labels_equal=same["framework"],
                           identical_bits_twice=bool(torch.equal(pb.val, fns["pseudobulk"]().val)))
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                         # after every row: a run cut short keeps what it measured
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                del pb
                torch.cuda.empty_cache()
            del batch, rows
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
