"""Timing of ResidentPredictor.knn's search op against two yardsticks (profiles/resident_knn.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200 (the hidden width of the timing bundle of
examples/resident_predict_timing.py), k in {15, 30}.  Two kinds of rows:
  normal    - seeded standard-normal float32 rows [B, D] made on the device: distances concentrate, the selection sees many
              survivors - the hard case for the staging lists
  embedding - ResidentPredictor.embed of examples/resident_rank_genes_timing.py's synthetic batch (above 20 000 cells the
              20 000-cell batch repeated, so every cell then has exact duplicates)
Per shape and k, in one process, the routes ALTERNATING inside every repetition:
  launch     - ops.knn_rows on the normal rows: wgnn_knn_rows (and its merge kernel when the scan is split), nothing else
  launch_emb - the same on the embedding
  framework  - chunks of queries: torch.cdist against all rows, the diagonal set to +inf, torch.topk(largest=False); the chunk
               keeps the [chunk, B] float32 distance block under --chunk-bytes
  knn        - the whole ResidentPredictor.knn call on the batch: classify, embed, the search, the read-back, the table
  host       - sklearn.neighbors.NearestNeighbors(algorithm="brute") on the normal rows (its BLAS threads), up to
               --host-max-cells cells (without sklearn: numpy at the smallest shape only); run once, after the rounds
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`launch_share_of_peak`: B * B * D * 3 flop (a subtract and a fused multiply-add per pair and column) over launch wall time,
over the float32 vector peak of 157.3 Tflop/s - a whole-call rate over peak, not a kernel-trace figure.  `framework_same_sets`
/ `host_same_sets`: the share of cells whose neighbour SET equals the kernel's (the framework route takes distances in norm
form through a GEMM, so near-ties may order differently); `*_overlap`: the mean share of a cell's neighbours found by both.

One batch size per process, each under its own time limit; rows are merged into --out by (batch, k) and the .md is rewritten:

    timeout -k 10 600 python examples/resident_knn_timing.py --out profiles/resident_knn.json --batches 2000
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
from scdeepsort_amd import ops                                 # noqa: E402

D, KS, PEAK_TFLOPS = HIDDEN, (15, 30), 157.3


def same_sets(a: np.ndarray, b: np.ndarray):
    """(share of rows with equal neighbour sets, mean share of a row's neighbours in both)"""
    a, b = np.sort(a, axis=1), np.sort(b, axis=1)
    both = np.array([np.intersect1d(x, y).size for x, y in zip(a, b)])
    return float((both == a.shape[1]).mean()), float(both.mean() / a.shape[1])


def write_md(rec, path):
    lines = ["# ResidentPredictor.knn: the search op against a framework route and a host route", "",
             f"Measured by `examples/resident_knn_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}; wall ms per call.", "",
             "| cells | k | splits | launch | launch (embedding) | share of f32 vector peak | framework | host | launch / framework | "
             "launch / host | knn() | framework same sets (overlap) | host same sets (overlap) |", "|" + "---|" * 13]
    for r in sorted(rec["rows"], key=lambda r: (r["batch"], r["k"])):
        host = "not run" if r["host_wall_ms"] is None else f"{r['host_wall_ms']:.0f} ({r['host_route']})"
        over_host = "-" if r["host_wall_ms"] is None else f"{r['launch_wall_ms'] / r['host_wall_ms']:.5f}"
        host_sets = "-" if r["host_wall_ms"] is None else f"{r['host_same_sets']:.4f} ({r['host_overlap']:.5f})"
        lines.append(f"| {r['batch']} | {r['k']} | {r['splits']} | {r['launch_wall_ms']:.2f} | {r['launch_emb_wall_ms']:.2f} | "
                     f"{r['launch_share_of_peak']:.3f} | {r['framework_wall_ms']:.2f} | {host} | "
                     f"{r['launch_wall_ms'] / r['framework_wall_ms']:.3f} | {over_host} | {r['knn_wall_ms']:.1f} | "
                     f"{r['framework_same_sets']:.4f} ({r['framework_overlap']:.5f}) | {host_sets} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--host-max-cells", type=int, default=20000)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, inner=args.inner, reps=args.reps, chunk_bytes=args.chunk_bytes),
               device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        NearestNeighbors = None
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            rows = torch.randn((B, D), device="cuda", generator=torch.Generator("cuda").manual_seed(B))
            emb = rp.embed(batch).contiguous()
            step = max(1, min(B, args.chunk_bytes // (4 * B)))
            for k in KS:
                def launch():
                    return ops.knn_rows(rows, k)

                def launch_emb():
                    return ops.knn_rows(emb, k)

                def framework():
                    out = torch.empty((B, k), dtype=torch.int64, device="cuda")
                    for r0 in range(0, B, step):
                        d = torch.cdist(rows[r0:r0 + step], rows)
                        n = d.shape[0]
                        d[torch.arange(n, device="cuda"), torch.arange(r0, r0 + n, device="cuda")] = float("inf")
                        out[r0:r0 + n] = torch.topk(d, k, dim=1, largest=False).indices
                    return out

                def whole():
                    return rp.knn(batch, k=k)

                inner = args.inner if B <= 20000 else 2
                fns = {"launch": (launch, inner), "launch_emb": (launch_emb, inner), "framework": (framework, inner), "knn": (whole, 1)}
                timed_alternating(fns, 1)                                                        # warm-up
                ms = timed_alternating(fns, args.reps if B <= 20000 else 3)
                got = launch()[0].cpu().numpy()
                fw_same, fw_overlap = same_sets(framework().cpu().numpy(), got)
                host_ms = host_route = host_same = host_overlap = None
                host_rows = rows.cpu().numpy()
                if NearestNeighbors is not None and B <= args.host_max_cells:
                    t0 = time.perf_counter()
                    found = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(host_rows).kneighbors(host_rows)[1]
                    host_ms, host_route = 1e3 * (time.perf_counter() - t0), "sklearn brute"
                    found = np.array([r[r != i][:k] for i, r in enumerate(found)])                 # the cell itself left out
                    host_same, host_overlap = same_sets(found, got)
                elif NearestNeighbors is None and B == min(args.batches):
                    t0 = time.perf_counter()
                    sq = (host_rows.astype(np.float64) ** 2).sum(1)
                    dist = sq[:, None] + sq[None, :] - 2.0 * host_rows.astype(np.float64) @ host_rows.astype(np.float64).T
                    np.fill_diagonal(dist, np.inf)
                    found = np.argpartition(dist, k, axis=1)[:, :k]
                    host_ms, host_route = 1e3 * (time.perf_counter() - t0), "numpy"
                    host_same, host_overlap = same_sets(found, got)
                nb = __import__("ctypes").c_int64()
                sda._lib.lib().wgnn_knn_workspace_bytes(B, B, k, 0, __import__("ctypes").addressof(nb))
                row = dict(batch=B, k=k, splits=max(1, nb.value // (8 * B * k)), launch_wall_ms=ms["launch"],
                           launch_emb_wall_ms=ms["launch_emb"], framework_wall_ms=ms["framework"], knn_wall_ms=ms["knn"],
                           launch_share_of_peak=3.0 * B * B * D / (ms["launch"] * 1e-3) / (PEAK_TFLOPS * 1e12),
                           host_wall_ms=host_ms, host_route=host_route, framework_same_sets=fw_same, framework_overlap=fw_overlap,
                           host_same_sets=host_same, host_overlap=host_overlap)
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                                                     # after every (batch, k)
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                    write_md(rec, Path(args.out).with_suffix(".md"))
            del batch, rows, emb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
