"""Timing of ResidentPredictor.smooth, of the pooling launches inside it, of the classify launches they feed and of two routes
that do without the kernel (profiles/resident_smooth.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model).  Batches of B in {2 000, 20 000, 100 000} cells of raw counts over the caller's own 30 000 columns - the bundle's 20 000
genes and 10 000 columns outside it, 800 expressed bundle genes and 80 outside columns per cell (the 100 000-cell batch is the
20 000-cell one five times over, the copies in shuffled order) -, every cell with k in {15, 30} distinct neighbours drawn at
random (the cells are random, so a random graph pools what a kNN graph would: k + 1 rows of 800 genes).  Per (B, k), in one
process, the calls ALTERNATING inside every repetition:
  smooth    - ResidentPredictor.smooth(counts, genes, neighbors, normalize="lognorm"): the whole call
  hood_rows - its pooling alone: ops.hood_rows (wgnn_hood_rows_count / _fill) on the aligned counts, chunk by chunk as smooth
              cuts them
  classify  - (a) the classify launches the pooling feeds: classify of the pooled rows, already on the device
  host      - (b) the host route: the scipy product (A + I) @ X on the host, the sums uploaded and
              classify(..., normalize="lognorm")
  framework - (c) framework ops on the device: torch.sparse.mm of the indicator A + I with the count matrix, the product as a CSR
              over the caller's columns through classify(..., normalize="lognorm") (align, then the layers)
  Routes (b) and (c) MATERIALISE the pooled matrix over the caller's columns; above --max-entries estimated stored entries they
  are not attempted and the row says so, and a route that fails (out of memory, an operator the framework lacks) is recorded
  with its error, not hidden.
  wall ms: perf_counter around the call until the device is idle; median and min .. max of `reps` after 1 warm-up round.

    python examples/resident_smooth_timing.py --out profiles/resident_smooth.json [--batches 2000] [--k 15]
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
from resident_pseudobulk_timing import count_batch             # noqa: E402
import resident_thin_timing as thin_timing                     # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import api, ops                            # noqa: E402

N_OUTSIDE = 10_000


def random_neighbors(B, k, seed):
    """int64 [B, k]: k distinct neighbours per cell, none the cell itself (ascending random offsets around the ring of cells)."""
    rng = np.random.default_rng(seed)
    off = np.cumsum(rng.integers(1, (B - 1) // k + 1, (B, k)), axis=1)
    return (np.arange(B)[:, None] + off) % B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--k", type=int, nargs="+", default=[15, 30])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-entries", type=float, default=6e8,
                    help="routes (b) and (c) are not attempted above this many estimated stored entries of the pooled matrix")
    args = ap.parse_args()
    thin_timing.N_OUTSIDE = N_OUTSIDE                              # count_batch's columns outside the bundle
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, max_entries=args.max_entries),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        genes = rp.gene_map(list(rp.id2gene) + [f"Outside{i}" for i in range(N_OUTSIDE)])
        n_cols = G + N_OUTSIDE
        for B in args.batches:
            host = count_batch(B)
            batch = tuple(torch.from_numpy(a).cuda() for a in (host.indptr.astype(np.int64), host.indices, host.data))
            with torch.no_grad():
                (rowptr, col, cnt), _, lib, *_ = rp._count_batch(batch, genes, api.LogNormalize(), "smooth", full_call=False)
            lens = (rowptr[1:] - rowptr[:-1]).cpu().numpy()
            x_dev = torch.sparse_csr_tensor(batch[0], batch[1].long(), batch[2], size=(B, n_cols))
            for k in args.k:
                nb = random_neighbors(B, k, 1000 * k + B)
                hood_ptr, members = api._neighbor_lists(nb, B, True)
                d_ptr, d_members = torch.from_numpy(hood_ptr).cuda(), torch.from_numpy(members).cuda()
                pooled_len = np.diff(np.concatenate([[0], np.cumsum(lens[members])])[hood_ptr])
                chunks = list(api._byte_chunks(np.cumsum(np.minimum(pooled_len, G) * 8), api.SMOOTH_CHUNK_BYTES))
                sm = rp.smooth(batch, genes, nb, normalize="lognorm")
                pool = lambda: [ops.hood_rows(rowptr, col, cnt, lib, d_ptr[s:e + 1], d_members, G) for s, e in chunks]
                pooled = pool()
                pooled_nnz = int(sum(int(p[1].shape[0]) for p in pooled))
                # what routes (b) and (c) store: the pooled rows over the caller's columns (a pooled row's outside columns in
                # proportion to its bundle genes)
                estimate = pooled_nnz * (1.0 + N_OUTSIDE / G)
                indicator = sp.csr_matrix((np.ones(members.shape[0], np.float32), members, hood_ptr), shape=(B, B))
                a_dev = torch.sparse_csr_tensor(d_ptr, d_members.long(), torch.ones(members.shape[0], device="cuda"), size=(B, B))

                def host_route():
                    return rp.classify((indicator @ host).tocsr(), genes=genes, normalize="lognorm")

                def framework_route():
                    prod = torch.sparse.mm(a_dev, x_dev)
                    prod = prod if prod.layout == torch.sparse_csr else prod.to_sparse_csr()
                    csr = (prod.crow_indices(), prod.col_indices().to(torch.int32), prod.values())
                    return rp.classify(csr, genes=genes, normalize="lognorm")

                fns = {"smooth": lambda: rp.smooth(batch, genes, nb, normalize="lognorm"),
                       "hood_rows": pool,
                       "classify": lambda: [rp.classify(p[:3]) for p in pooled]}
                notes = {}
                for name, fn in (("host", host_route), ("framework", framework_route)):
                    if estimate > args.max_entries:
                        notes[name] = f"not attempted: about {estimate:.3g} stored entries to materialise (--max-entries {args.max_entries:g})"
                        continue
                    try:                                             # once, outside the timed window: does the route run at all?
                        notes[name] = "labels equal smooth's" if np.array_equal(fn()[0], sm.smooth_label) else "labels DIFFER from smooth's"
                        fns[name] = fn
                    except (RuntimeError, MemoryError, NotImplementedError) as e:
                        notes[name] = f"failed: {type(e).__name__}: {str(e).splitlines()[0][:200]}"
                        torch.cuda.empty_cache()
                timed_alternating(fns, 1)                            # warm-up
                ms = timed_alternating(fns, args.reps)
                row = dict(batch=B, k=k, chunks=len(chunks), nnz=int(host.nnz), members=int(members.shape[0]), pooled_nnz=pooled_nnz,
                           # count and fill each read col + cnt of every member row once per slab of 16384 genes
                           rows_read_bytes=int(lens[members].sum()) * 8 * 2 * -(-G // 16384),
                           **{f"{name}_wall_ms": dict(median=v[0], min=v[1], max=v[2]) for name, v in ms.items()},
                           hood_rows_over_classify=ms["hood_rows"][0] / ms["classify"][0],
                           **{f"smooth_over_{name}": ms["smooth"][0] / ms[name][0] for name in ("host", "framework") if name in ms},
                           notes=notes, rescued=int(sm.rescued().sum()), lost=int(sm.lost().sum()), changed=int(sm.changed().sum()),
                           identical_bits_twice=bool(torch.equal(sm.logits, fns["smooth"]().logits)))
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                         # after every row: a run cut short keeps what it measured
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                del pooled, sm, a_dev
                torch.cuda.empty_cache()
            del batch, x_dev
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
