"""Timing of ResidentPredictor.stability against the two ways to ask the same question without its kernel
(profiles/resident_stability.md).

Bundle and batches as examples/resident_predict_timing.py: G = 20 000 genes, 800 expressed genes per cell, hidden 200, C = 16
classes, randomly initialised 1- and 2-layer models; batches of B in {200, 2 000, 20 000} cells that are already on the device
(a device CSR triple); one level, keep = 0.5, n_draws = 32.  Per (layers, B), in one process, the calls ALTERNATING inside
every repetition:
  classify   - ResidentPredictor.classify once, the yardstick
  stability  - ResidentPredictor.stability(keep=(0.5,), n_draws=32): the full call, then wgnn_predict_rows_dropout per layer
  level      - the draws of that level alone (stability minus the full call it starts with; computed, not timed)
  n_classify - (a) n_draws classify calls of the same, unthinned batch, back to back
  framework  - (b) per draw a thinned CSR materialised with framework ops (a boolean mask, cumsum, gather) and classified:
               n_draws matrices, n_draws x n_layers launches, a host round trip per draw for the labels, the tally by bincount
  wall_ms: perf_counter around the call until the device is idle, median of `reps` after 2 warm-up rounds.
`level_over_n_classify` and `level_over_framework` are ratios of wall_ms; below 1 the kernel is faster.

    python examples/resident_stability_timing.py --out profiles/resident_stability.json [--batches 200 2000]
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
from resident_clusters_timing import timed_alternating        # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402

N_DRAWS, KEEP = 32, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, density=PER_CELL / G, hidden=HIDDEN, classes=N_CLS, n_draws=N_DRAWS, keep=KEEP),
               device=torch.cuda.get_device_name(0), rows=[])
    for n_layers in args.layers:
        with tempfile.TemporaryDirectory() as td:
            write_bundle(Path(td), n_layers)
            rp = sda.ResidentPredictor("mouse", f"Timing{n_layers}", model_path=td, unsure_rate=1.5)
            for B in args.batches:
                host = expression(B, 100 + B)
                rowptr, col, raw = (torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
                batch = (rowptr, col, raw)
                rows = torch.repeat_interleave(torch.arange(B, device="cuda"), rowptr[1:] - rowptr[:-1])
                gen = torch.Generator(device="cuda").manual_seed(B)

                def framework():
                    votes = torch.zeros((B, N_CLS), dtype=torch.int64, device="cuda")
                    for _ in range(N_DRAWS):
                        kept = torch.rand(col.shape[0], device="cuda", generator=gen) < KEEP
                        n = torch.zeros(B, dtype=torch.int64, device="cuda").index_add_(0, rows, kept.long())
                        rp_d = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(n, 0)])
                        pred, _, _ = rp.classify((rp_d, col[kept], raw[kept]))
                        lab = torch.from_numpy(pred).cuda()
                        on = lab >= 0
                        votes.view(-1).index_add_(0, (torch.arange(B, device="cuda") * N_CLS + lab)[on], on[on].long())
                    return votes

                def n_classify():
                    for _ in range(N_DRAWS):
                        rp.classify(batch)

                fns = {"classify": lambda: rp.classify(batch),
                       "stability": lambda: rp.stability(batch, keep=(KEEP,), n_draws=N_DRAWS, seed=1),
                       "n_classify": n_classify, "framework": framework}
                timed_alternating(fns, 2)                                # warm-up
                ms = timed_alternating(fns, args.reps)
                level = ms["stability"] - ms["classify"]
                st = fns["stability"]()
                row = dict(layers=n_layers, batch=B, nnz=int(col.shape[0]), **{f"{k}_wall_ms": v for k, v in ms.items()},
                           level_wall_ms=level, level_over_n_classify=level / ms["n_classify"],
                           level_over_framework=level / ms["framework"],
                           median_agreement=float(np.median(st.agreement()[0])), empty_draws=int(st.empty.sum()),
                           identical_bits_twice=bool(torch.equal(st.conf_sum, fns["stability"]().conf_sum)))
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                del batch, rowptr, col, raw, rows
                torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
