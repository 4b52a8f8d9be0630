"""Timing of ResidentPredictor.markers against explain on the same batches (profiles/resident_markers.json).

Shape, bundles and batches as examples/resident_explain_timing.py: G = 20 000 genes, 800 expressed genes per cell, hidden 200,
16 classes, a randomly initialised model with 1 and 2 layers (unsure_rate 0: every cell keeps its label and takes part),
batches of B in {200, 2 000, 20 000, 100 000} that are already on the device (a device CSR triple).  Per (layers, B), in one process, the calls ALTERNATING inside every repetition:
  explain  - ResidentPredictor.explain(top_k=0), the yardstick: the code markers runs first, unchanged
  markers  - ResidentPredictor.markers (explain, then transpose + wgnn_group_gene_reduce, per-group host sums)
  reduce   - ops.group_gene_reduce alone on explain's scores and labels (transpose + reduce: the kernel route)
  index_add- the same table by the framework: zeros(K * G, f64).index_add_(0, group[row] * G + col, scores.double()) with
             float atomics (not deterministic, no counts), the row ids built by repeat_interleave
  device_ms: HIP events around the call on the current stream, median of `reps` after 2 warm-ups.
`markers_over_explain` and `reduce_over_index_add` are ratios of device_ms.

    python examples/resident_markers_timing.py --out profiles/resident_markers.json [--batches 200 2000] [--layers 1]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, expression, write_bundle      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402


def timed_alternating(fns, reps):
    """Median device ms per call, the calls taking turns inside every repetition."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms[name].append(s.elapsed_time(e))
    return {name: float(np.median(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, density=PER_CELL / G, hidden=HIDDEN, classes=N_CLS), device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        for L in args.layers:
            write_bundle(Path(td), L)
            rp = sda.ResidentPredictor("mouse", f"Timing{L}", model_path=td, unsure_rate=0.0)     # no cell is unsure
            for B in args.batches:
                host = expression(B, 100 + B)
                batch = (torch.from_numpy(host.indptr).cuda(), torch.from_numpy(host.indices).cuda(), torch.from_numpy(host.data).cuda())
                rowptr, col, _ = batch
                att = rp.explain(batch, top_k=0)
                group = torch.from_numpy(att.label.astype(np.int32)).cuda()
                scores = att.scores

                def index_add():
                    row = torch.repeat_interleave(torch.arange(B, device=col.device), rowptr[1:] - rowptr[:-1])
                    g = group.long()[row]
                    on = g >= 0
                    return torch.zeros(N_CLS * G, dtype=torch.float64, device=col.device).index_add_(
                        0, g[on] * G + col.long()[on], scores[on].double())

                fns = {"explain": lambda: rp.explain(batch, top_k=0), "markers": lambda: rp.markers(batch),
                       "reduce": lambda: sda.group_gene_reduce(rowptr, col, scores, group, N_CLS, G, check=False),
                       "index_add": index_add}
                timed_alternating(fns, 2)                                # warm-up
                ms = timed_alternating(fns, args.reps)
                row = dict(layers=L, batch=B, nnz=int(host.nnz), cells_in_groups=int((att.label >= 0).sum()),
                           **{f"{k}_device_ms": v for k, v in ms.items()})
                row["markers_over_explain"] = ms["markers"] / ms["explain"]
                row["reduce_over_index_add"] = ms["reduce"] / ms["index_add"]
                total, _ = fns["reduce"]()
                row["max_abs_diff_vs_index_add"] = float((total.reshape(-1) - index_add()).abs().max())
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                del att, scores, total
            del rp
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
