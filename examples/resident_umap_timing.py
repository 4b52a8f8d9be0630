"""Timing of ops.fuzzy_graph / ops.layout_graph / ResidentPredictor.umap (profiles/resident_umap.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200 (the hidden width of the timing bundle of
examples/resident_predict_timing.py), k = 15.  Rows: 32 seeded unit-variance Gaussians around N(0, 1) centres, float32 [B, D] made
on the device; their exact kNN lists come from ops.knn_rows and are not timed here (profiles/resident_knn.md has that launch).
Per shape, in one process, the routes ALTERNATING inside every repetition:
  fuzzy      - ops.fuzzy_graph on the lists: snn_graph's union structure (framework ops), wgnn_fuzzy_rows, wgnn_fuzzy_union
  rows       - wgnn_fuzzy_rows and wgnn_fuzzy_union alone, on a structure built before
  epoch      - one wgnn_layout_epoch launch (a, b = layout_curve(0.1, 1): the float64 pow runs), in a window of `inner` back-to-back
               launches that ping-pong two position buffers, at the middle epoch of the schedule, from positions spread by 10
               epochs; wall time until the device is idle, per launch
  epoch_b1   - the same with b = 1 (no pow): what the float64 pow costs is epoch - epoch_b1
  enqueue    - the host time to enqueue one such launch through ops' ctypes path (perf_counter around the calls, before any
               synchronise); `launch_share` = enqueue / epoch, capped at 1: at 1 the loop is bound by the host's launches
  framework  - the same epoch's arithmetic with framework ops: the firing mask, a gather of both ends, the coefficient, the clamp
               and index_add_ into the force, then the negatives drawn by torch.randint (one gather + index_add_ per draw) and the
               update; not bit-compatible with the kernel (other draws, atomically ordered sums), the same work
  layout     - the whole ops.layout_graph (500 epochs below 10 000 cells, 200 from there on; one read-back before, one after)
  umap       - the whole ResidentPredictor.umap call with init="hash" on the synthetic batch of
               examples/resident_rank_genes_timing.py (classify, embed, the kNN search, fuzzy_graph, layout_graph, the table)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`bytes`: what one epoch has to move, counted from the graph - per stored edge col and w (8 B), per firing edge the other end's
position and n_neg drawn positions (8 B each), per vertex rowptr, its position in and out and its firing count (32 B); `fire_rate`
is the measured share of stored edges firing per epoch (n_fired / (nnz n_epochs)); `GB/s` = bytes / epoch.  Positions are 8 B per
cell and stay in L2, so this is no HBM figure.

One batch size per process, each under its own time limit; rows are merged into --out by batch and the .md is rewritten:

    timeout -k 10 600 python examples/resident_umap_timing.py --out profiles/resident_umap.json --batches 2000
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

D, K_NN, N_NEG = HIDDEN, 15, 5


def write_md(rec, path):
    lines = ["# ResidentPredictor.umap: the fuzzy graph and the synchronous layout against a framework epoch", "",
             f"Measured by `examples/resident_umap_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k = {K_NN}, {N_NEG} negatives, a, b = layout_curve(0.1, 1); wall ms per call.", "",
             "| cells | stored edges | fuzzy_graph | its two kernels | epoch | epoch, b = 1 | enqueue | launch share | fire rate | "
             "MB / epoch | GB/s | framework epoch | epoch / framework | epochs | layout_graph | per epoch | umap() |",
             "|" + "---|" * 17]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['fuzzy_wall_ms']:.2f} | {r['rows_wall_ms']:.3f} | {r['epoch_wall_ms']:.4f} | "
                     f"{r['epoch_b1_wall_ms']:.4f} | {r['enqueue_ms']:.4f} | {r['launch_share']:.2f} | {r['fire_rate']:.3f} | "
                     f"{r['epoch_bytes'] / 1e6:.2f} | {r['epoch_gbs']:.0f} | {r['framework_wall_ms']:.3f} | "
                     f"{r['epoch_wall_ms'] / r['framework_wall_ms']:.3f} | {r['n_epochs']} | {r['layout_wall_ms']:.1f} | "
                     f"{r['layout_wall_ms'] / r['n_epochs']:.4f} | {r['umap_wall_ms']:.1f} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, k=K_NN, n_neg=N_NEG, inner=args.inner, reps=args.reps), device=torch.cuda.get_device_name(0),
               rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    a, b = ops.layout_curve(0.1, 1.0)
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            gen = torch.Generator("cuda").manual_seed(B)
            centres = torch.randn((32, D), device="cuda", generator=gen)
            rows = centres[torch.randint(0, 32, (B,), device="cuda", generator=gen)] + torch.randn((B, D), device="cuda", generator=gen)
            idx, d2 = ops.knn_rows(rows, K_NN)
            dev = rows.device
            stream = _stream(dev)
            graph = ops.fuzzy_graph(idx, d2)
            rowptr, col, w = graph.rowptr, graph.col, graph.w
            nnz = int(col.shape[0])
            n_epochs = ops.layout_epochs(B)
            mid = n_epochs // 2
            alpha = 1.0 - mid / n_epochs
            wmax = float(w.max())
            y = ops.layout_graph(rowptr, col, w, "hash", n_epochs=10, a=a, b=b).y.clone()
            other = torch.empty_like(y)
            member, rho, sigma, w2 = torch.empty_like(graph.member), torch.empty_like(graph.rho), torch.empty_like(graph.sigma), torch.empty_like(w)
            row = torch.repeat_interleave(torch.arange(B, device=dev), rowptr[1:] - rowptr[:-1], output_size=nnz)
            buffers = [y, other]

            def fuzzy():
                return ops.fuzzy_graph(idx, d2)

            def kernels():
                _lib.run(dev, "wgnn_fuzzy_rows", _ptr(idx), K_NN, _ptr(d2), K_NN, B, K_NN, float(np.log2(K_NN + 1)), _ptr(rho),
                         _ptr(sigma), _ptr(member), 0, stream)
                _lib.run(dev, "wgnn_fuzzy_union", _ptr(idx), K_NN, _ptr(member), B, K_NN, _ptr(rowptr), _ptr(col), nnz, _ptr(w2), 0, stream)

            def epoch(bb=b):
                _lib.run(dev, "wgnn_layout_epoch", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, wmax, _ptr(buffers[0]), _ptr(buffers[1]),
                         mid, n_epochs, a, bb, 1.0, alpha, N_NEG, 0, None, 0, stream)
                buffers.reverse()

            def epoch_b1():
                epoch(1.0)

            def framework():
                yy = buffers[0]
                r = w / wmax
                fire = torch.floor((mid + 1) * r) != torch.floor(mid * r)
                i, j = row[fire], col[fire].long()
                force = torch.zeros_like(yy)
                dx = yy[i] - yy[j]
                q = (dx * dx).sum(1, keepdim=True)
                qb = q.double().pow(b).float()
                c = torch.where(q > 0, (-2.0 * a * b) * qb / q / (1.0 + a * qb), torch.zeros_like(q))
                force.index_add_(0, i, (c * dx).clamp_(-4.0, 4.0))
                for _ in range(N_NEG):
                    t = torch.randint(0, B, i.shape, device=dev)
                    dx = yy[i] - yy[t]
                    q = (dx * dx).sum(1, keepdim=True)
                    qb = q.double().pow(b).float()
                    c = torch.where((q > 0) & (t != i)[:, None], (2.0 * b) / ((0.001 + q) * (1.0 + a * qb)), torch.zeros_like(q))
                    force.index_add_(0, i, (c * dx).clamp_(-4.0, 4.0))
                return yy + alpha * force

            def layout():
                return ops.layout_graph(rowptr, col, w, "hash", a=a, b=b)

            def whole():
                return rp.umap(batch, k=K_NN, init="hash")

            inner = args.inner
            fns = {"fuzzy": (fuzzy, 2), "rows": (kernels, 2), "epoch": (epoch, inner), "epoch_b1": (epoch_b1, inner),
                   "framework": (framework, 4), "layout": (layout, 1), "umap": (whole, 1)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)
            assert torch.equal(w2, w) and torch.equal(member, graph.member), "the kernels alone and fuzzy_graph disagree"
            enqueue = []
            for _ in range(args.reps):                                                           # the host's side of a launch alone
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    epoch()
                enqueue.append(1e3 * (time.perf_counter() - t0) / inner)
                torch.cuda.synchronize()
            out = layout()
            fire_rate = out.n_fired / (nnz * out.n_epochs)
            epoch_bytes = 8 * nnz + fire_rate * nnz * 8 * (1 + N_NEG) + 32 * B
            rec_row = dict(batch=B, nnz=nnz, fuzzy_wall_ms=ms["fuzzy"], rows_wall_ms=ms["rows"], epoch_wall_ms=ms["epoch"],
                           epoch_b1_wall_ms=ms["epoch_b1"], enqueue_ms=float(np.median(enqueue)),
                           launch_share=min(1.0, float(np.median(enqueue)) / ms["epoch"]), framework_wall_ms=ms["framework"],
                           layout_wall_ms=ms["layout"], umap_wall_ms=ms["umap"], n_epochs=out.n_epochs, n_fired=out.n_fired,
                           fire_rate=fire_rate, epoch_bytes=epoch_bytes, epoch_gbs=epoch_bytes / (ms["epoch"] * 1e-3) / 1e9,
                           longest_row=int((rowptr[1:] - rowptr[:-1]).max()), span=float(out.y.abs().max()),
                           finite=bool(torch.isfinite(out.y).all()))
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
