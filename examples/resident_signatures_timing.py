"""Timing of ResidentPredictor.signatures' scoring launches against three yardsticks (profiles/resident_signatures.md).

Bundle and batches as examples/resident_predict_timing.py: G = 20 000 genes, 800 expressed genes per cell, hidden 200, C = 16
classes, a randomly initialised 1-layer model; batches of B in {2 000, 20 000, 100 000} cells that are already on the device (a
device CSR triple over the bundle's gene ids; above 20 000 cells the 20 000-cell batch is repeated on the device).  P in
{16, 64} sets of 50 random genes, max_rank = 1500.  Per shape, in one process, the calls ALTERNATING inside every repetition:
  scoring   - ops.rank_sets_rows alone: the one wgnn_rank_sets_rows launch signatures() adds per 64 sets
  classify  - ResidentPredictor.classify of the same batch, (a): the launch signatures() runs first, unchanged
  framework - (c): the dense [cells, G] matrix in chunks of --chunk-cells cells, torch.sort along the genes, the doubled mid-ranks
              of every gene by two torch.searchsorted, capped, and the sets' sums by one fp64 matmul with the membership matrix
  host      - (b): per cell scipy.stats.rankdata(-dense row, "average"), capped, then the same formula in numpy; timed on the
              first --host-cells cells of the batch and scaled to B cells (host_cells_timed says how many were timed)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.  scoring and classify run `inner` = --inner calls per window, framework and signatures one; host
  runs once, after the alternating rounds.
`scoring_over_*` are ratios of wall_ms; below 1 the kernel is faster.  `signatures_wall_ms` is the whole call (classify, the
launch, the read-back and the fp64 host step) for orientation.  Every route's scores are compared with the kernel's
(`framework_equal`, `host_equal`: exactly equal fp64 scores on the cells the route ran).

    python examples/resident_signatures_timing.py --out profiles/resident_signatures.json [--batches 2000 20000]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from scipy.stats import rankdata

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle      # noqa: E402
from resident_clusters_timing import device_batch              # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import api, ops                            # noqa: E402

SET_SIZE, MAX_RANK = 50, 1500


def timed_alternating(fns, reps):
    """Median wall ms per call; ``fns[name] = (fn, inner)``: ``inner`` back-to-back calls per timed window, the routes taking
    turns inside every repetition."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, (fn, inner) in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / inner)
    return {name: float(np.median(v)) for name, v in ms.items()}


def finish(rank_sum_all, set_size):
    """fp64 scores [cells, P] from the sets' sums of capped doubled ranks over ALL their genes (stored or not)."""
    n = set_size.astype(np.float64)[None, :]
    two_u = rank_sum_all - n * (n + 1)
    return 1.0 - two_u / (2 * n * MAX_RANK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--sets", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--chunk-cells", type=int, default=2000)
    ap.add_argument("--host-cells", type=int, default=1000)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, set_size=SET_SIZE, max_rank=MAX_RANK,
                          chunk_cells=args.chunk_cells, inner=args.inner, reps=args.reps),
               device=torch.cuda.get_device_name(0), rows=[])
    cap = 2 * (MAX_RANK + 1)
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            rowptr, col, val = device_batch(B)
            rows = torch.repeat_interleave(torch.arange(B, device="cuda"), rowptr[1:] - rowptr[:-1])
            n_host = min(B, args.host_cells)
            h_ptr = rowptr[:n_host + 1].cpu().numpy()
            h_col, h_val = col[:h_ptr[-1]].cpu().numpy(), val[:h_ptr[-1]].cpu().numpy()
            for P in args.sets:
                rng = np.random.default_rng(7 * P + B)
                member = np.zeros((P, G), bool)
                for p in range(P):
                    member[p, rng.choice(G, SET_SIZE, replace=False)] = True
                sets = {f"s{p}": [rp.id2gene[g] for g in np.flatnonzero(member[p])] for p in range(P)}
                set_size = member.sum(axis=1)
                words = torch.from_numpy(api._member_words(member)).cuda()
                member_t = torch.from_numpy(np.ascontiguousarray(member.T)).cuda().to(torch.float64)       # [G, P]

                def scoring():
                    return ops.rank_sets_rows(rowptr, col, val, words, P, MAX_RANK, G, check_cols=False)

                def classify():
                    return rp.classify((rowptr, col, val))

                def framework():
                    out = []
                    for r0 in range(0, B, args.chunk_cells):
                        r1 = min(B, r0 + args.chunk_cells)
                        e0, e1 = int(rowptr[r0]), int(rowptr[r1])
                        dense = torch.zeros((r1 - r0, G), dtype=torch.float32, device="cuda")
                        dense[rows[e0:e1] - r0, col[e0:e1].long()] = val[e0:e1]
                        ordered = torch.sort(dense, dim=1).values
                        ge = G - torch.searchsorted(ordered, dense, right=False)                # entries >= the value
                        gt = G - torch.searchsorted(ordered, dense, right=True)                 # entries > the value
                        r2c = (gt + ge + 1).clamp_(max=cap).to(torch.float64)                   # 2 gt + eq + 1
                        out.append(r2c @ member_t)
                    return torch.cat(out)

                def host():
                    sums = np.empty((n_host, P))
                    m_t = member.T.astype(np.float64)
                    for r in range(n_host):
                        row = np.zeros(G)
                        row[h_col[h_ptr[r]:h_ptr[r + 1]]] = h_val[h_ptr[r]:h_ptr[r + 1]]
                        sums[r] = np.minimum(2.0 * rankdata(-row, "average"), cap) @ m_t
                    return finish(sums, set_size)

                def whole():
                    return rp.signatures((rowptr, col, val), sets, max_rank=MAX_RANK)

                fns = {"scoring": (scoring, args.inner), "classify": (classify, args.inner), "framework": (framework, 1),
                       "signatures": (whole, 1)}
                timed_alternating(fns, 1)                                                        # warm-up
                ms = timed_alternating(fns, args.reps)
                t0 = time.perf_counter()
                host_score = host()
                host_ms = 1e3 * (time.perf_counter() - t0) * (B / n_host)
                r2, present = (x.cpu().numpy() for x in scoring())
                deg = (rowptr[1:] - rowptr[:-1]).cpu().numpy()
                score = api._signature_scores(r2, present, deg, set_size, G, MAX_RANK)
                row = dict(batch=B, sets=P, nnz=int(col.shape[0]), scoring_wall_ms=ms["scoring"], classify_wall_ms=ms["classify"],
                           framework_wall_ms=ms["framework"], host_wall_ms=host_ms, host_cells_timed=n_host,
                           signatures_wall_ms=ms["signatures"], scoring_over_classify=ms["scoring"] / ms["classify"],
                           scoring_over_framework=ms["scoring"] / ms["framework"], scoring_over_host=ms["scoring"] / host_ms,
                           framework_equal=bool(np.array_equal(finish(framework().cpu().numpy(), set_size), score)),
                           host_equal=bool(np.array_equal(host_score, score[:n_host])),
                           signatures_equal=bool(np.array_equal(whole().score, score)))
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                                                     # after every row: a run cut short keeps its rows
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
            del rowptr, col, val, rows
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
