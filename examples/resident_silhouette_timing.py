"""Timing of ops.silhouette_rows / ResidentPredictor.silhouette against three yardsticks (profiles/resident_silhouette.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200 (the hidden width of the timing bundle of
examples/resident_predict_timing.py).  Rows: 32 seeded unit-variance Gaussians around N(0, 1) centres, float32 [B, D] made on
the device.  Groupings: `even` - K in {16, 1 024} groups drawn uniformly; `dominant` - K = 16 with nine cells in ten in group 0
(whole groups are dealt to the splits, so one dominant group bounds the balance: this row shows what that costs).
Per shape and grouping, in one process, the routes ALTERNATING inside every repetition:
  launch     - wgnn_silhouette_rows alone on rows already gathered group-major (the plan, the pair kernel and the merge)
  op         - ops.silhouette_rows: the validity mask, the sort into group-major order, the gather, `launch`, the scatter back
  knn        - ops.knn_rows(rows, 15): a wgnn_knn_rows launch of the same shape - the same pair tiles with a top-k selection in
               place of the group sums; the yardstick for what the tile padding of small groups costs
  framework  - torch.cdist(rows, rows[chunk]) in query chunks that keep the [B, chunk] float32 block under --chunk-bytes, a
               float64 [K, chunk] index_add_ of the block by group, then a, b, nearest and the score with framework ops
  silhouette - the whole ResidentPredictor.silhouette call on the synthetic batch of examples/resident_rank_genes_timing.py with
               the same grouping (classify, embed, the op, the read-back, the table)
  host       - sklearn.metrics.silhouette_samples on the rows (its BLAS / OpenMP threads), up to --host-max-cells cells; run once,
               after the rounds
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`tiles`: the (query tile, candidate tile) pairs the pair kernel walks, ceil(B / 64) * sum_c ceil(n_c / 64), over the
ceil(B / 64)^2 of a dense scan - the padding factor.  `share_of_peak`: B * B * D * 3 flop over the launch's wall time, over 157.3
Tflop/s - a whole-launch rate, not a kernel-trace figure.  `max_abs_diff`: the largest |score - framework score|.

One batch size per process, each under its own time limit; rows are merged into --out by (batch, grouping, K) and the .md is
rewritten:

    timeout -k 10 600 python examples/resident_silhouette_timing.py --out profiles/resident_silhouette.json --batches 2000
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

D, PEAK_TFLOPS = HIDDEN, 157.3
CASES = (("even", 16), ("dominant", 16), ("even", 1024))


def write_md(rec, path):
    lines = ["# ResidentPredictor.silhouette: the pair kernel against a kNN launch, a framework route and a host route", "",
             f"Measured by `examples/resident_silhouette_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}; wall ms per call.", "",
             "| cells | grouping | K | splits | tiles / dense | launch | op | share of f32 vector peak | knn launch | launch / knn | "
             "framework | launch / framework | host | silhouette() | max abs diff |", "|" + "---|" * 15]
    for r in sorted(rec["rows"], key=lambda r: (r["batch"], r["K"], r["grouping"])):
        host = "not run" if r["host_wall_ms"] is None else f"{r['host_wall_ms']:.0f}"
        lines.append(f"| {r['batch']} | {r['grouping']} | {r['K']} | {r['splits']} | {r['tiles_over_dense']:.2f} | "
                     f"{r['launch_wall_ms']:.2f} | {r['op_wall_ms']:.2f} | {r['share_of_peak']:.3f} | {r['knn_wall_ms']:.2f} | "
                     f"{r['launch_wall_ms'] / r['knn_wall_ms']:.2f} | {r['framework_wall_ms']:.2f} | "
                     f"{r['launch_wall_ms'] / r['framework_wall_ms']:.3f} | {host} | {r['silhouette_wall_ms']:.1f} | "
                     f"{r['max_abs_diff']:.2e} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def grouping(kind, B, K, gen):
    g = torch.randint(0, K, (B,), device="cuda", generator=gen)
    if kind == "dominant":
        g = torch.where(torch.rand(B, device="cuda", generator=gen) < 0.9, torch.zeros_like(g), g)
    return g


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
        from sklearn.metrics import silhouette_samples
    except ImportError:
        silhouette_samples = None
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            gen = torch.Generator("cuda").manual_seed(B)
            centres = torch.randn((32, D), device="cuda", generator=gen)
            rows = centres[torch.randint(0, 32, (B,), device="cuda", generator=gen)] + torch.randn((B, D), device="cuda", generator=gen)
            step = max(1, min(B, args.chunk_bytes // (4 * B)))
            for kind, K in CASES:
                group = grouping(kind, B, K, gen)
                host_group = group.cpu().numpy()
                size = torch.bincount(group, minlength=K)
                q_tiles = -(-B // 64)
                tiles = q_tiles * int(((size + 63) // 64).sum())
                order, seg_ptr = ops._group_major(group, K)
                major = rows[order.long()].contiguous()
                outs = [torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(3)] + \
                       [torch.empty(B, dtype=torch.int32, device="cuda")]
                ws, ws_bytes = ops._workspace(rows.device, "wgnn_silhouette_workspace_bytes", B, K, 0)
                splits = 1 if ws_bytes == 0 else (ws_bytes - 8) // (8 + 20 * B)

                def launch():
                    _lib.run(rows.device, "wgnn_silhouette_rows", _ptr(major), D, B, D, _ptr(seg_ptr), K, 0, *map(_ptr, outs),
                             _ptr(ws), ws_bytes, 0, _stream(rows.device))

                def op():
                    return ops.silhouette_rows(rows, group, K)

                def knn():
                    return ops.knn_rows(rows, 15)

                def framework():
                    n_c = size.double()
                    a, b = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
                    nearest = torch.empty(B, dtype=torch.int64, device="cuda")
                    for r0 in range(0, B, step):
                        own = group[r0:r0 + step]
                        block = torch.cdist(rows, rows[r0:r0 + step])                            # [B, chunk]
                        S = torch.zeros((K, block.shape[1]), dtype=torch.float64, device="cuda").index_add_(0, group, block.double())
                        mine = S.gather(0, own[None, :])[0]
                        a[r0:r0 + step] = mine / (n_c[own] - 1).clamp(min=1)
                        mean = S / n_c[:, None]
                        mean[n_c == 0] = float("inf")
                        mean.scatter_(0, own[None, :], float("inf"))
                        b[r0:r0 + step], nearest[r0:r0 + step] = mean.min(dim=0)
                    score = torch.where(n_c[group] > 1, (b - a) / torch.maximum(a, b), torch.zeros_like(a))
                    return score, nearest

                def whole():
                    return rp.silhouette(batch, groups=host_group, n_groups=K)

                inner = args.inner if B <= 20000 else 1
                fns = {"launch": (launch, inner), "op": (op, inner), "knn": (knn, inner), "framework": (framework, inner),
                       "silhouette": (whole, 1)}
                timed_alternating(fns, 1)                                                        # warm-up
                ms = timed_alternating(fns, args.reps)
                diff = float((op().score - framework()[0]).abs().max())
                host_ms = None
                if silhouette_samples is not None and B <= args.host_max_cells:
                    host_rows = rows.cpu().numpy()
                    t0 = time.perf_counter()
                    silhouette_samples(host_rows, host_group)
                    host_ms = 1e3 * (time.perf_counter() - t0)
                row = dict(batch=B, grouping=kind, K=K, splits=int(splits), tiles_over_dense=tiles / (q_tiles * q_tiles),
                           launch_wall_ms=ms["launch"], op_wall_ms=ms["op"], knn_wall_ms=ms["knn"],
                           framework_wall_ms=ms["framework"], silhouette_wall_ms=ms["silhouette"], host_wall_ms=host_ms,
                           share_of_peak=B * B * D * 3 / (ms["launch"] * 1e-3) / (PEAK_TFLOPS * 1e12), max_abs_diff=diff,
                           largest_group=int(size.max()))
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                if args.out:                                                                     # after every case
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                    write_md(rec, Path(args.out).with_suffix(".md"))
            del batch, rows
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
