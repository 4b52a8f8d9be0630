"""Timing of ResidentPredictor.annotate's reduction against the classify call it follows (profiles/resident_clusters.json).

Bundle and batches as examples/resident_predict_timing.py: G = 20 000 genes, 800 expressed genes per cell, hidden 200, C = 16
classes, a randomly initialised 1-layer model; batches of B in {2 000, 20 000, 200 000} cells that are already on the device (a
device CSR triple; above 20 000 cells the 20 000-cell batch is repeated on the device), K = 30 clusters drawn at random, one
cell in twenty in no cluster.  Per B, in one process, the calls ALTERNATING inside every repetition:
  classify  - ResidentPredictor.classify, the yardstick: the code annotate runs first, unchanged
  annotate  - ResidentPredictor.annotate (classify, then the group-major re-ordering and wgnn_group_class_reduce)
  reduce    - ops.group_class_reduce alone on classify's logits and labels (stable sort + search + the two kernels)
  framework - the same four tables by framework ops: softmax(logits.double()), index_add_ of the probabilities and of their
              row maxima (fp64 atomics: not deterministic), the counts by bincount
  wall_ms: perf_counter around the call until the device is idle, median of `reps` after 2 warm-up rounds.
`annotate_over_classify` and `reduce_over_framework` are ratios of wall_ms.  No speed is promised for this kernel (B x C is a
few MB: every route is launch- and latency-bound); what it adds is fp64, one addition order and streaming.

    python examples/resident_clusters_timing.py --out profiles/resident_clusters.json [--batches 2000 20000]
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
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, expression, write_bundle      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402

K = 30
HOST_CELLS = 20_000


def timed_alternating(fns, reps):
    """Median wall ms per call, the calls taking turns inside every repetition."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: float(np.median(v)) for name, v in ms.items()}


def device_batch(B):
    host = expression(min(B, HOST_CELLS), 100 + B)
    rowptr, col, raw = (torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
    times = -(-B // HOST_CELLS) if B > HOST_CELLS else 1
    if times > 1:
        col, raw = col.repeat(times), raw.repeat(times)
        rowptr = torch.arange(0, times * HOST_CELLS * PER_CELL + 1, PER_CELL, dtype=torch.int64, device="cuda")
    return rowptr, col, raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 200000])
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, density=PER_CELL / G, hidden=HIDDEN, classes=N_CLS, clusters=K, layers=1),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            n = int(batch[0].shape[0]) - 1
            rng = np.random.default_rng(B)
            clusters = rng.integers(0, K, n)
            clusters[rng.random(n) < 0.05] = -1
            pred, _, logits = rp.classify(batch)
            label = torch.from_numpy(pred.astype(np.int32)).cuda()
            group = torch.from_numpy(clusters.astype(np.int32)).cuda()

            def framework():
                on = group >= 0
                g = group[on].long()
                p = torch.softmax(logits[on].double(), dim=1)
                prob = torch.zeros((K, N_CLS), dtype=torch.float64, device="cuda").index_add_(0, g, p)
                conf = torch.zeros(K, dtype=torch.float64, device="cuda").index_add_(0, g, p.max(dim=1).values)
                lab = label[on].long()
                votes = torch.bincount((g * N_CLS + lab)[lab >= 0], minlength=K * N_CLS).reshape(K, N_CLS)
                return prob, conf, votes, torch.bincount(g, minlength=K), torch.bincount(g[lab < 0], minlength=K)

            fns = {"classify": lambda: rp.classify(batch), "annotate": lambda: rp.annotate(batch, clusters, n_clusters=K),
                   "reduce": lambda: sda.group_class_reduce(logits, label, group, K, check=False), "framework": framework}
            timed_alternating(fns, 2)                                # warm-up
            ms = timed_alternating(fns, args.reps)
            row = dict(batch=n, cells_in_clusters=int((clusters >= 0).sum()), unsure=int((pred < 0).sum()),
                       **{f"{k}_wall_ms": v for k, v in ms.items()})
            row["annotate_over_classify"] = ms["annotate"] / ms["classify"]
            row["reduce_over_framework"] = ms["reduce"] / ms["framework"]
            mine, theirs = fns["reduce"](), framework()
            row["max_rel_diff_vs_framework"] = float(((mine[0] - theirs[0]).abs() / theirs[0].clamp(min=1e-300)).max())
            row["counts_equal"] = bool(torch.equal(mine[2].long(), theirs[2]) and torch.equal(mine[3][:, 0].long(), theirs[3]))
            row["identical_bits_twice"] = all(torch.equal(a, b) for a, b in zip(mine, fns["reduce"]()))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            del batch, logits
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
