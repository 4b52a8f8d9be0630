"""Timing of ResidentPredictor's two routes against the existing predict path (profiles/resident_predict.json).

Shape: G = 20 000 genes, density 0.04 (800 expressed genes per cell), dense 400, hidden 200, 16 classes, 10 000 support
cells, a randomly initialised model with 1 and 2 layers, batches of B in {200, 2 000, 20 000, 100 000} test cells.
Per (layers, B):
  fused   - ResidentPredictor.classify on the fused route (wgnn_predict_rows, one launch per layer)
  graph   - the same call on the graph route (predict graph of support + test cells, cached gene features)
  device_ms: HIP events around the call on the current stream; wall_ms: the call until its results are on the host.
The existing path (DeepSortPredictor.predict) is the graph route plus the host PCA it runs on every call; the PCA time is
measured once per bundle (the ResidentPredictor constructor runs the same helper) and reported as `pca_ms`, and
`existing_end_to_end_ms` = graph wall + pca (bundle and file parsing excluded on every route).

    python examples/resident_predict_timing.py --out profiles/resident_predict.json [--batches 200 2000] [--layers 1] [--routes fused]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import api                                 # noqa: E402
from scdeepsort_amd.api import BundlePaths                     # noqa: E402

G, PER_CELL, DENSE, HIDDEN, N_CLS, N_SUP = 20_000, 800, 400, 200, 16, 10_000


def expression(n_cells, seed):
    """n_cells x G raw values, PER_CELL distinct sorted genes per cell (one gene per window of G / PER_CELL, shifted)."""
    rng = np.random.default_rng(seed)
    win = G // PER_CELL
    base = np.arange(PER_CELL) * win + rng.integers(0, win, (n_cells, PER_CELL))
    cols = np.sort((base + rng.integers(0, G, (n_cells, 1))) % G, axis=1).astype(np.int32)
    vals = np.clip(rng.normal(3.0, 1.0, cols.shape), 0.2, 7.0).astype(np.float32)
    indptr = np.arange(0, n_cells * PER_CELL + 1, PER_CELL, dtype=np.int64)
    return sp.csr_matrix((vals.ravel(), cols.ravel(), indptr), shape=(n_cells, G))


def write_bundle(root, n_layers):
    b = BundlePaths(root, "mouse", f"Timing{n_layers}", layout="flat", for_write=True)
    b.mkdirs()
    b.genes.write_bytes("".join(f"Gene{i}\r\n" for i in range(G)).encode())
    b.cell_types.write_bytes("".join(f"type{i}\r\n" for i in range(N_CLS)).encode())
    sp.save_npz(b.support, expression(N_SUP, 1))
    torch.manual_seed(n_layers)
    m = sda.GNN(DENSE, HIDDEN, N_CLS, n_layers, G, activation=F.relu)
    with torch.no_grad():
        m.alpha.uniform_(0.5, 1.5)
    torch.save({"model": m.state_dict(), "optimizer": {}}, b.model)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    dev_ms, wall_ms = [], []
    for s, e in ev:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        wall_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(s.elapsed_time(e))
    return float(np.median(dev_ms)), float(np.median(wall_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", nargs="+", default=["fused", "graph"], choices=["fused", "graph"])
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, density=PER_CELL / G, dense=DENSE, hidden=HIDDEN, classes=N_CLS, support_cells=N_SUP),
               device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        for L in args.layers:
            write_bundle(Path(td), L)
            calls = []
            real = api._gene_features

            def counted(*a, **k):
                t0 = time.perf_counter()
                out = real(*a, **k)
                calls.append(1e3 * (time.perf_counter() - t0))
                return out
            api._gene_features = counted
            t0 = time.perf_counter()
            rp = sda.ResidentPredictor("mouse", f"Timing{L}", model_path=td)
            ctor_ms = 1e3 * (time.perf_counter() - t0)
            api._gene_features = real
            pca_ms = calls[0]
            for B in args.batches:
                batch = expression(B, 100 + B)
                row = dict(layers=L, batch=B, nnz=int(batch.nnz), work=int(batch.nnz) * rp.hidden_padded * L, pca_ms=pca_ms,
                           constructor_ms=ctor_ms)
                for route, limit in (("fused", 1 << 62), ("graph", -1)):
                    if route not in args.routes:
                        continue
                    api.RESIDENT_FUSED_MAX_WORK = limit
                    rp.classify(batch)                                   # warm-up (and plan / kernel caches)
                    assert rp.last_route == route
                    reps = args.reps if (route == "fused" or B <= 20000) else max(2, args.reps // 2)
                    row[f"{route}_device_ms"], row[f"{route}_wall_ms"] = timed(lambda: rp.classify(batch), reps)
                if "graph_wall_ms" in row:
                    row["existing_end_to_end_ms"] = row["graph_wall_ms"] + pca_ms
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
            del rp
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
