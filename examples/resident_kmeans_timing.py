"""Timing of ResidentPredictor.kmeans' three device parts against two yardsticks (profiles/resident_kmeans.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200 (the hidden width of the timing bundle of
examples/resident_predict_timing.py), K in {16, 256, 1 024}.  Rows: 32 seeded unit-variance Gaussians around N(0, 1) centres,
float32 [B, D] made on the device (they overlap, so Lloyd's iterations have work to do).
Per shape and K, in one process, the routes ALTERNATING inside every repetition:
  seed         - ops.kmeans_seed: the validity check (one read-back) and wgnn_kmeans_seed's 2 K + 1 launches
  seed_fw      - the framework route of the same seeding, no read-back either: per round torch.cdist against the newest seed
                 row, squared, torch.minimum, a float64 torch.cumsum and torch.searchsorted of u * total
  assign       - ops.knn_rows(C, 1, queries=rows, exclude_self=False) against the K seed rows: wgnn_knn_rows
  assign_fw    - torch.cdist(rows, C) in query chunks that keep the [chunk, K] block under --chunk-bytes, torch.argmin
  update       - ops.group_rows_reduce(rows, label, K): the sort into group-major order and wgnn_group_rows_reduce
  update_fw    - a float64 [K, D] index_add_ of rows.double(), torch.bincount and the divide
  kmeans       - the whole ResidentPredictor.kmeans call on the synthetic batch of examples/resident_rank_genes_timing.py
                 (classify, embed, seeding, every iteration with its read-backs, the table); `kmeans_n_iter` assignments
  host         - sklearn.cluster.KMeans(init="k-means++", n_init=1, algorithm="lloyd") on the rows (its BLAS / OpenMP
                 threads), up to --host-max-cells cells; run once, after the rounds; `host_n_iter` iterations
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`seed_share_of_bandwidth`: (K + 1) * B * D * 4 bytes (every pass reads X once) over the seed route's wall time, over 8 TB/s - a
whole-call rate, not a kernel-trace figure.  `lloyd_ms` = assign + update, `lloyd_fw_ms` likewise.

One batch size per process, each under its own time limit; rows are merged into --out by (batch, K) and the .md is rewritten:

    timeout -k 10 600 python examples/resident_kmeans_timing.py --out profiles/resident_kmeans.json --batches 2000
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

D, KS, PEAK_TBS = HIDDEN, (16, 256, 1024), 8.0


def write_md(rec, path):
    lines = ["# ResidentPredictor.kmeans: seeding, assignment and update against a framework route and a host route", "",
             f"Measured by `examples/resident_kmeans_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}; wall ms per call.", "",
             "| cells | K | seed | seed (framework) | seed / framework | share of 8 TB/s | assign | assign (framework) | update | "
             "update (framework) | Lloyd step / framework | kmeans() (assignments) | host (iterations) |", "|" + "---|" * 13]
    for r in sorted(rec["rows"], key=lambda r: (r["batch"], r["K"])):
        host = "not run" if r["host_wall_ms"] is None else f"{r['host_wall_ms']:.0f} ({r['host_n_iter']})"
        lines.append(f"| {r['batch']} | {r['K']} | {r['seed_wall_ms']:.2f} | {r['seed_fw_wall_ms']:.2f} | "
                     f"{r['seed_wall_ms'] / r['seed_fw_wall_ms']:.3f} | {r['seed_share_of_bandwidth']:.3f} | "
                     f"{r['assign_wall_ms']:.3f} | {r['assign_fw_wall_ms']:.3f} | {r['update_wall_ms']:.3f} | "
                     f"{r['update_fw_wall_ms']:.3f} | {r['lloyd_ms'] / r['lloyd_fw_ms']:.3f} | "
                     f"{r['kmeans_wall_ms']:.1f} ({r['kmeans_n_iter']}) | {host} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--host-max-cells", type=int, default=20000)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, inner=args.inner, reps=args.reps, chunk_bytes=args.chunk_bytes),
               device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            gen = torch.Generator("cuda").manual_seed(B)
            centres = torch.randn((32, D), device="cuda", generator=gen)
            rows = centres[torch.randint(0, 32, (B,), device="cuda", generator=gen)] + torch.randn((B, D), device="cuda", generator=gen)
            rows64 = rows.double()
            for K in KS:
                seed_row, _ = ops.kmeans_seed(rows, K)
                C = rows[seed_row.long()].contiguous()
                label = ops.knn_rows(C, 1, queries=rows, exclude_self=False)[0][:, 0].contiguous()
                label64 = label.long()
                draws = torch.rand(K, dtype=torch.float64, device="cuda", generator=gen)
                step = max(1, min(B, args.chunk_bytes // (4 * K)))

                def seed():
                    return ops.kmeans_seed(rows, K)

                def seed_fw():
                    picked = torch.empty(K, dtype=torch.int64, device="cuda")
                    w = torch.ones(B, dtype=torch.float32, device="cuda")
                    for r in range(K):
                        prefix = torch.cumsum(w.double(), 0)
                        s = torch.searchsorted(prefix, (draws[r] * prefix[-1]).reshape(1), right=True).clamp_(max=B - 1)
                        picked[r] = s
                        d = torch.cdist(rows, rows[s])[:, 0] ** 2
                        w = d if r == 0 else torch.minimum(w, d)
                    return picked

                def assign():
                    return ops.knn_rows(C, 1, queries=rows, exclude_self=False)

                def assign_fw():
                    out = torch.empty(B, dtype=torch.int64, device="cuda")
                    for r0 in range(0, B, step):
                        out[r0:r0 + step] = torch.argmin(torch.cdist(rows[r0:r0 + step], C), dim=1)
                    return out

                def update():
                    return ops.group_rows_reduce(rows, label, K)

                def update_fw():
                    total = torch.zeros((K, D), dtype=torch.float64, device="cuda").index_add_(0, label64, rows64)
                    count = torch.bincount(label64, minlength=K)
                    return (total / count.clamp(min=1)[:, None]).float()

                n_iter = []

                def whole():
                    n_iter.append(rp.kmeans(batch, K).n_iter)

                inner = args.inner if B <= 20000 else 1
                fns = {"seed": (seed, inner), "seed_fw": (seed_fw, inner), "assign": (assign, inner), "assign_fw": (assign_fw, inner),
                       "update": (update, inner), "update_fw": (update_fw, inner), "kmeans": (whole, 1)}
                timed_alternating(fns, 1)                                                        # warm-up
                ms = timed_alternating(fns, args.reps)
                host_ms = host_iter = None
                if KMeans is not None and B <= args.host_max_cells:
                    host_rows = rows.cpu().numpy()
                    t0 = time.perf_counter()
                    fit = KMeans(n_clusters=K, init="k-means++", n_init=1, algorithm="lloyd", random_state=0).fit(host_rows)
                    host_ms, host_iter = 1e3 * (time.perf_counter() - t0), int(fit.n_iter_)
                row = dict(batch=B, K=K, seed_wall_ms=ms["seed"], seed_fw_wall_ms=ms["seed_fw"], assign_wall_ms=ms["assign"],
                           assign_fw_wall_ms=ms["assign_fw"], update_wall_ms=ms["update"], update_fw_wall_ms=ms["update_fw"],
                           lloyd_ms=ms["assign"] + ms["update"], lloyd_fw_ms=ms["assign_fw"] + ms["update_fw"],
                           kmeans_wall_ms=ms["kmeans"], kmeans_n_iter=int(n_iter[-1]),
                           seed_share_of_bandwidth=(K + 1) * B * D * 4 / (ms["seed"] * 1e-3) / (PEAK_TBS * 1e12),
                           host_wall_ms=host_ms, host_n_iter=host_iter)
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                                                     # after every (batch, K)
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                    write_md(rec, Path(args.out).with_suffix(".md"))
            del batch, rows, rows64
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
