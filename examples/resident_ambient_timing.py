"""Timing of ResidentPredictor.ambient, of the soup merge inside it, of the classify launches it feeds and of two routes that
do without the kernel (profiles/resident_ambient.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model).  Batches of B in {2 000, 20 000} cells of raw counts over the caller's own 30 000 columns - the bundle's 20 000 genes
and 10 000 columns outside it, 800 expressed bundle genes and 80 outside columns per cell, counts geometric with mean 2.5 and
one gene in 200 a hundred times deeper -, 3 levels of rho x 8 draws, the soup profile the batch's own column sums.  Per B, in
one process, the calls ALTERNATING inside every repetition:
  ambient   - ResidentPredictor.ambient(counts, genes, normalize="lognorm", rho=(0.05, 0.1, 0.2), n_draws=8): the whole call
  soup_rows - its merge alone: ops.soup_rows on the same operands, level by level and chunk by chunk as ambient cuts them
  classify  - the floor the merge adds to: classify of the B x 3 x 8 contaminated rows, already on the device
  host      - the host route: per level and draw the soup reads of all cells drawn with numpy (every cell's multinomial by
              inverse-cdf lookup of its reads, all cells of a draw in one call - faster than one numpy multinomial per cell),
              added to the scipy count matrix, the sum uploaded and classify(..., normalize="lognorm")
  torch     - a framework-op route: per level, draw and block of 2 000 cells torch.multinomial draws the block's reads on the
              device, index_add_ puts them on the block's dense count matrix, and classify(..., normalize="lognorm") aligns
              and classifies it
  wall ms: perf_counter around the call until the device is idle; median and min .. max of `reps` after 1 warm-up round.

    python examples/resident_ambient_timing.py --out profiles/resident_ambient.json [--batches 2000]
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

RHO, N_DRAWS, N_OUTSIDE, BLOCK = (0.05, 0.1, 0.2), 8, 10_000, 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    thin_timing.N_OUTSIDE = N_OUTSIDE                              # count_batch's columns outside the bundle
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, rho=RHO, n_draws=N_DRAWS),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        genes = rp.gene_map(list(rp.id2gene) + [f"Outside{i}" for i in range(N_OUTSIDE)])
        n_cols = G + N_OUTSIDE
        for B in args.batches:
            host = thin_timing.count_batch(B, 100 + B)
            batch = tuple(torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
            kw = dict(normalize="lognorm", rho=RHO, n_draws=N_DRAWS, seed=1)
            am = rp.ambient(batch, genes, **kw)
            # the operands and chunks ambient works on, for the shares timed alone
            with torch.no_grad():
                (rowptr, col, cnt), _, lib, *_ = rp._count_batch(batch, genes, api.LogNormalize(), "ambient", full_call=False)
            bundle = torch.from_numpy(am.profile[0]).cuda()
            cdf = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
            torch.cumsum(torch.cat([bundle, torch.tensor([am.profile[1]], device="cuda")]), 0, out=cdf[1:])
            lens = rowptr[1:] - rowptr[:-1]
            work = []                                              # (n_add of the level, the level's cuts)
            for k in RHO:
                n_add = torch.floor(lib.double() * (k / (1.0 - k)) + 0.5).long()
                bound = torch.cumsum((lens + torch.clamp(n_add, max=G)) * (8 * N_DRAWS), 0).cpu().numpy()
                cuts = [0]
                while cuts[-1] < B:
                    done = int(bound[cuts[-1] - 1]) if cuts[-1] else 0
                    cuts.append(max(cuts[-1] + 1, int(np.searchsorted(bound, done + api.AMBIENT_CHUNK_BYTES, side="right"))))
                work.append((n_add, cuts))
            merge = lambda: [ops.soup_rows(rowptr[s:e + 1], col, cnt, lib[s:e], n_add[s:e], cdf, N_DRAWS, row0=s, seed=1, scale=1e4,
                                           threshold=0.0) for n_add, cuts in work for s, e in zip(cuts, cuts[1:])]
            merged = merge()
            # the soup over the caller's columns, for the two routes that draw there
            sums = np.asarray(host.sum(axis=0)).ravel()
            p_host = sums / sums.sum()
            cum = np.cumsum(p_host)
            p_dev = torch.from_numpy(p_host).cuda().float()
            n_adds = [w[0].cpu().numpy() for w in work]
            rng = np.random.default_rng(B)

            def host_route():
                for n_add in n_adds:
                    rows = np.repeat(np.arange(B), n_add)
                    for _ in range(N_DRAWS):
                        bins = np.minimum(np.searchsorted(cum, rng.random(rows.shape[0]), side="right"), n_cols - 1)
                        soup = sp.csr_matrix((np.ones(rows.shape[0], np.float32), (rows, bins)), shape=host.shape)
                        rp.classify((host + soup).tocsr(), genes=genes, normalize="lognorm")

            def torch_route():
                for level_add, _ in work:
                    for _ in range(N_DRAWS):
                        for s in range(0, B, BLOCK):
                            e = min(B, s + BLOCK)
                            lo, hi = int(batch[0][s]), int(batch[0][e])
                            r = torch.repeat_interleave(torch.arange(e - s, device="cuda"), (batch[0][s + 1:e + 1] - batch[0][s:e]))
                            dense = torch.zeros((e - s) * n_cols, dtype=torch.float32, device="cuda")
                            dense.index_add_(0, r * n_cols + batch[1][lo:hi].long(), batch[2][lo:hi])
                            n = level_add[s:e]
                            bins = torch.multinomial(p_dev, int(n.sum()), replacement=True)
                            rows = torch.repeat_interleave(torch.arange(e - s, device="cuda"), n)
                            dense.index_add_(0, rows * n_cols + bins, torch.ones(bins.shape[0], device="cuda"))
                            rp.classify(dense.view(e - s, n_cols), genes=genes, normalize="lognorm")

            fns = {"ambient": lambda: rp.ambient(batch, genes, **kw),
                   "soup_rows": merge,
                   "classify": lambda: [rp.classify(m[:3]) for m in merged],
                   "host": host_route,
                   "torch": torch_route}
            timed_alternating(fns, 1)                                # warm-up
            ms = timed_alternating(fns, args.reps)
            agree = am.agreement()
            row = dict(batch=B, units=B * len(RHO) * N_DRAWS, chunks=sum(len(c) - 1 for _, c in work), nnz=int(host.nnz),
                       soup_reads=int(sum(int(n.sum()) for n in n_adds)) * N_DRAWS,
                       merged_nnz=int(sum(int(m[1].shape[0]) for m in merged)),
                       **{f"{k}_wall_ms": dict(median=v[0], min=v[1], max=v[2]) for k, v in ms.items()},
                       soup_rows_over_classify=ms["soup_rows"][0] / ms["classify"][0],
                       ambient_over_host=ms["ambient"][0] / ms["host"][0], ambient_over_torch=ms["ambient"][0] / ms["torch"][0],
                       median_agreement=[float(np.nanmedian(agree[:, l])) if np.isfinite(agree[:, l]).any() else None
                                         for l in range(len(RHO))],
                       identical_bits_twice=bool(np.array_equal(am.draw_prob, fns["ambient"]().draw_prob)))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            del batch, merged
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
