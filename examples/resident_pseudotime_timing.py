"""Timing of ops.geodesic_rows / ResidentPredictor.pseudotime (profiles/resident_pseudotime.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200, k = 15.  Rows: a seeded noisy arc - (20 cos 3s, 20 sin 3s, 0, ...) + 0.15
N(0, 1) in every one of the D columns, s uniform - so that the kNN graph is one long component and the rounds are many; the exact
kNN lists come from ops.knn_rows (not timed), the graph from ops.distance_graph, the root is cell 0.  Per shape, in one process,
the routes ALTERNATING inside every repetition:
  round_kernel    - one wgnn_geodesic_round launch on the state after half of the run's rounds: the kernel alone, no read-back
  round_framework - the same round composed of framework ops on the same state: a gather, an add, scatter_reduce_(amin) over the
                    rows, a second pass (compare, scatter_reduce_(amin) of the ids) for the predecessor, two selects and the count;
                    its result is checked against the kernel's, bit for bit, before anything is timed
  rows_1, rows_8  - ops.geodesic_rows end to end (all rounds, every read-back) with check_every = 1 and 8
  distance_graph  - ops.distance_graph on the lists
  pseudotime, louvain - the whole ResidentPredictor calls on the synthetic batch of examples/resident_rank_genes_timing.py (root 0)
  host            - scipy.sparse.csgraph.dijkstra on the host on the same CSR in float64 (the copy to the host is not in it)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`rounds`: the rounds that changed something; `round_bytes` = 12 nnz + 24 B: per stored entry col, length and the gathered distance,
per vertex two rowptr words' worth, dist and pred in and out; `round_gbs` = round_bytes over round_kernel's wall time.  `max_rel`:
the largest relative distance of the device's float32 result to scipy's float64 one, in units of 2^-24.

One batch size per process, each under its own time limit; rows are merged into --out by batch and the .md is rewritten:

    timeout -k 10 600 python examples/resident_pseudotime_timing.py --out profiles/resident_pseudotime.json --batches 2000
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
from resident_predict_timing import G, HIDDEN, write_bundle   # noqa: E402
from resident_rank_genes_timing import device_batch           # noqa: E402
from resident_signatures_timing import timed_alternating      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import _lib, ops                           # noqa: E402
from scdeepsort_amd.graph import _ptr, _stream                 # noqa: E402

D, K_NN = HIDDEN, 15
INT_MAX = 2 ** 31 - 1


def write_md(rec, path):
    lines = ["# ResidentPredictor.pseudotime: the geodesic rounds against framework ops and a host Dijkstra", "",
             f"Measured by `examples/resident_pseudotime_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k = {K_NN}, a noisy arc, root 0; wall ms per call.", "",
             "| cells | stored edges | rounds | round, kernel | round, framework ops | kernel GB/s | geodesic_rows, check_every 1 | "
             "check_every 8 | distance_graph | scipy dijkstra (host) | max rel. to scipy (x 2^-24) | pseudotime() | louvain() | "
             "pseudotime() rounds |", "|" + "---|" * 14]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['rounds']} | {r['round_kernel_wall_ms']:.4f} | "
                     f"{r['round_framework_wall_ms']:.3f} | {r['round_gbs']:.0f} | {r['rows_1_wall_ms']:.2f} | "
                     f"{r['rows_8_wall_ms']:.2f} | {r['distance_graph_wall_ms']:.2f} | {r['host_wall_ms']:.1f} | {r['max_rel']:.2f} | "
                     f"{r['pseudotime_wall_ms']:.1f} | {r['louvain_wall_ms']:.1f} | {r['pseudotime_rounds']} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, k=K_NN, inner=args.inner, reps=args.reps), device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            gen = torch.Generator("cuda").manual_seed(B)
            s = torch.rand(B, device="cuda", generator=gen)
            rows = 0.15 * torch.randn((B, D), device="cuda", generator=gen)
            rows[:, 0] += 20 * torch.cos(3 * s)
            rows[:, 1] += 20 * torch.sin(3 * s)
            idx, d2 = ops.knn_rows(rows, K_NN)
            dev = rows.device
            rowptr, col, length = ops.distance_graph(idx, d2)
            nnz = int(col.shape[0])
            stream = _stream(dev)
            whole = ops.geodesic_rows(rowptr, col, length, 0)
            assert whole.converged
            half = ops.geodesic_rows(rowptr, col, length, 0, max_rounds=max(1, whole.rounds // 2))
            dist, pred = half.dist, half.pred
            dist2, pred2 = torch.empty_like(dist), torch.empty_like(pred)
            slots = torch.zeros(2, dtype=torch.int64, device=dev)
            row = torch.repeat_interleave(torch.arange(B, device=dev), rowptr[1:] - rowptr[:-1], output_size=nnz)
            col64 = col.long()
            inf = torch.full((), float("inf"), device=dev)

            def round_kernel():
                _lib.run(dev, "wgnn_geodesic_round", _ptr(rowptr), _ptr(col), _ptr(length), B, nnz, _ptr(dist), _ptr(pred),
                         _ptr(dist2), _ptr(pred2), slots.data_ptr(), slots.data_ptr() + 8, 0, 0, stream)

            def round_framework():
                du = dist[col64]
                cand = torch.where(torch.isfinite(du), du + length, inf)
                best = torch.full((B,), float("inf"), device=dev).scatter_reduce_(0, row, cand, "amin")
                ids = torch.where(cand == best[row], col, INT_MAX)
                came = torch.full((B,), INT_MAX, dtype=torch.int32, device=dev).scatter_reduce_(0, row, ids, "amin")
                better = best < dist
                return torch.where(better, best, dist), torch.where(better, came, pred), better.sum()

            round_kernel()
            fd, fp, fc = round_framework()
            assert torch.equal(fd.view(torch.int32), dist2.view(torch.int32)) and torch.equal(fp, pred2) and int(fc) == int(slots[0]) > 0
            assert int(slots[1]) == 0

            inner = args.inner
            fns = {"round_kernel": (round_kernel, inner), "round_framework": (round_framework, inner),
                   "rows_1": (lambda: ops.geodesic_rows(rowptr, col, length, 0, check_every=1), 1),
                   "rows_8": (lambda: ops.geodesic_rows(rowptr, col, length, 0, check_every=8), 1),
                   "distance_graph": (lambda: ops.distance_graph(idx, d2), 1),
                   "pseudotime": (lambda: rp.pseudotime(batch, 0, k=K_NN), 1), "louvain": (lambda: rp.louvain(batch, k=K_NN), 1)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)

            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import dijkstra
            m = csr_matrix((length.cpu().numpy().astype(np.float64), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(B, B))
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = dijkstra(m, directed=True, indices=0)
                host.append(1e3 * (time.perf_counter() - t0))
            got = whole.dist.cpu().numpy().astype(np.float64)
            fin = np.isfinite(want)
            assert (fin == np.isfinite(got)).all()
            rel = np.abs(got[fin] - want[fin]) / np.maximum(want[fin], np.finfo(np.float64).tiny)
            table = rp.pseudotime(batch, 0, k=K_NN)
            round_bytes = 12 * nnz + 24 * B
            rec_row = dict(batch=B, nnz=nnz, rounds=whole.rounds, reached=whole.reached, **{f"{name}_wall_ms": v for name, v in ms.items()},
                           round_bytes=round_bytes, round_gbs=round_bytes / (ms["round_kernel"] * 1e-3) / 1e9,
                           host_wall_ms=float(np.median(host)), max_rel=float(rel.max() / 2.0 ** -24),
                           pseudotime_rounds=table.rounds, pseudotime_reached=table.reached)
            print(json.dumps(rec_row), flush=True)
            rec["rows"].append(rec_row)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                write_md(rec, Path(args.out).with_suffix(".md"))
            del batch, rows
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
