"""Timing of ResidentPredictor.stability(thin="reads") against the host route it replaces, and against thin="genes"
(profiles/resident_thin.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model).  Batches of B in {200, 2 000, 20 000} cells of raw counts at 10x-like depth over the caller's own gene list: the
bundle's 20 000 genes and 2 000 columns outside it, 800 expressed bundle genes per cell, counts geometric with mean 2.5 and one
gene in 200 a hundred times deeper, so a cell holds about 3 000 reads.  32 draws, three levels (0.75, 0.5, 0.25).  Per B, in one
process, the calls ALTERNATING inside every repetition:
  classify - ResidentPredictor.classify(counts, genes=, normalize="lognorm") once, the yardstick
  reads    - stability(thin="reads"): wgnn_predict_rows_thin draws, re-normalises and classifies every (cell, draw, level)
  genes    - stability(thin="genes") on the same batch (uniform per-gene dropout on the normalised values)
  host     - the route thin="reads" replaces: per level and draw numpy.random.Generator.binomial on the host counts, the
             thinned CSR uploaded, classify(..., normalize="lognorm"), the labels tallied on the host
  wall_ms: perf_counter around the call until the device is idle, median of `reps` after 1 warm-up round.
`reads_over_host` and `reads_over_genes` are ratios of wall_ms; below 1 thin="reads" is faster.

    python examples/resident_thin_timing.py --out profiles/resident_thin.json [--batches 200 2000]
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
from resident_clusters_timing import timed_alternating        # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402

N_DRAWS, LEVELS, N_OUTSIDE = 32, (0.75, 0.5, 0.25), 2000


def count_batch(B, seed):
    """A host CSR [B, G + N_OUTSIDE] of integer counts: PER_CELL bundle genes and PER_CELL // 10 outside columns per cell."""
    rng = np.random.default_rng(seed)
    per = PER_CELL + PER_CELL // 10
    cols = np.empty((B, per), np.int32)
    for r in range(B):
        cols[r, :PER_CELL] = np.sort(rng.choice(G, PER_CELL, replace=False))
        cols[r, PER_CELL:] = G + np.sort(rng.choice(N_OUTSIDE, per - PER_CELL, replace=False))
    vals = rng.geometric(0.4, (B, per))
    vals = np.where(rng.random((B, per)) < 0.005, vals * 100, vals).astype(np.float32)
    return sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(B + 1, dtype=np.int64) * per), shape=(B, G + N_OUTSIDE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, n_draws=N_DRAWS, keep=LEVELS),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        genes = rp.gene_map(list(rp.id2gene) + [f"Outside{i}" for i in range(N_OUTSIDE)])
        for B in args.batches:
            host = count_batch(B, 100 + B)
            batch = tuple(torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
            rng = np.random.default_rng(B)

            def host_route():
                votes = np.zeros((len(LEVELS), B, N_CLS), np.int64)
                for li, k in enumerate(LEVELS):
                    for _ in range(N_DRAWS):
                        thin = sp.csr_matrix((rng.binomial(host.data.astype(np.int64), k).astype(np.float32), host.indices, host.indptr),
                                             shape=host.shape)
                        pred, _, _ = rp.classify(thin, genes=genes, normalize="lognorm")
                        on = pred >= 0
                        np.add.at(votes[li], (np.flatnonzero(on), pred[on]), 1)
                return votes

            kw = dict(genes=genes, normalize="lognorm", keep=LEVELS, n_draws=N_DRAWS, seed=1)
            fns = {"classify": lambda: rp.classify(batch, genes=genes, normalize="lognorm"),
                   "reads": lambda: rp.stability(batch, thin="reads", **kw),
                   "genes": lambda: rp.stability(batch, thin="genes", **kw),
                   "host": host_route}
            timed_alternating(fns, 1)                                # warm-up
            ms = timed_alternating(fns, args.reps)
            st = fns["reads"]()
            row = dict(batch=B, nnz=int(host.nnz), reads_per_cell=float(host.data.sum() / B),
                       **{f"{k}_wall_ms": v for k, v in ms.items()},
                       reads_over_host=ms["reads"] / ms["host"], reads_over_genes=ms["reads"] / ms["genes"],
                       median_agreement=[float(np.median(a)) for a in st.agreement()], empty_draws=int(st.empty.sum()),
                       identical_bits_twice=bool(torch.equal(st.conf_sum, fns["reads"]().conf_sum)))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            del batch
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
