"""Timing of ResidentPredictor.explain against classify on the same batches (profiles/resident_explain.json).

Shape, bundles and batches as examples/resident_predict_timing.py: G = 20 000 genes, 800 expressed genes per cell, dense 400,
hidden 200, 16 classes, a randomly initialised model with 1 and 2 layers, batches of B in {200, 2 000, 20 000, 100 000}.
Per (layers, B), both calls in one process on a batch that is already on the device (a device CSR triple):
  classify - ResidentPredictor.classify (wgnn_predict_rows, one launch per layer), the yardstick
  explain  - ResidentPredictor.explain(top_k=10) (wgnn_attrib_rows per layer, wgnn_rows_topk)
  device_ms: HIP events around the call on the current stream; wall_ms: the call until its results are on the host.
`ratio` = explain device_ms / classify device_ms.

    python examples/resident_explain_timing.py --out profiles/resident_explain.json [--batches 200 2000] [--layers 1]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, expression, timed, write_bundle      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--top-k", type=int, default=10)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, density=PER_CELL / G, hidden=HIDDEN, classes=N_CLS, top_k=args.top_k),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        for L in args.layers:
            write_bundle(Path(td), L)
            rp = sda.ResidentPredictor("mouse", f"Timing{L}", model_path=td)
            for B in args.batches:
                host = expression(B, 100 + B)
                batch = (torch.from_numpy(host.indptr).cuda(), torch.from_numpy(host.indices).cuda(), torch.from_numpy(host.data).cuda())
                row = dict(layers=L, batch=B, nnz=int(host.nnz))
                for name, fn in (("classify", lambda: rp.classify(batch)), ("explain", lambda: rp.explain(batch, top_k=args.top_k))):
                    fn(); fn()                                           # warm-up
                    row[f"{name}_device_ms"], row[f"{name}_wall_ms"] = timed(fn, args.reps)
                row["ratio"] = row["explain_device_ms"] / row["classify_device_ms"]
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
            del rp
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
