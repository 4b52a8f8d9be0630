"""Timing of ResidentPredictor.panels against the two routes it replaces (profiles/resident_panels.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, randomly initialised 1- and
2-layer models).  Batches of B in {200, 2 000, 20 000} cells of raw counts over the caller's own gene list: the bundle's
20 000 genes and 2 000 columns outside it, 800 + 80 expressed per cell, counts geometric with mean 2.5.  P in {8, 64} panels,
alternately 500 random genes of the caller's list to KEEP and the complement of 100 random genes ("mix"); at B = 2 000, P = 64
also P keep-500 panels ("keep500") and P complements ("without100") on their own.  Two modes: the counts taken as values
(renormalize=False) and re-normalised per panel (renormalize=True, normalize="lognorm").  Per shape, in one process, the calls
ALTERNATING inside every repetition:
  panels - ResidentPredictor.panels(...): one wgnn_predict_rows_panels launch per layer and 64 panels
  device - per panel a sub-CSR materialised with framework ops on the device (boolean mask over the entries, cumsum for the
           row pointers, gather), then classify(sub, genes=[, normalize=LogNormalize(library_size=the panel's reads)])
  host   - per panel a scipy column mask of the host CSR, then classify(sub, genes=[, normalize="lognorm"]) (upload included);
           left out (null) where B * P exceeds --host-max-pairs
  wall_ms: perf_counter around the call until the device is idle, median of `reps` after 1 warm-up round.
`panels_over_device` and `panels_over_host` are ratios of wall_ms; below 1 panels() is faster.

    python examples/resident_panels_timing.py --out profiles/resident_panels.json [--batches 200 2000] [--layers 1]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle      # noqa: E402
from resident_clusters_timing import timed_alternating        # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402

N_OUTSIDE, KEEP, REMOVE = 2000, 500, 100


def count_batch(B, seed):
    """A host CSR [B, G + N_OUTSIDE] of integer counts: PER_CELL bundle genes and PER_CELL // 10 outside columns per cell
    (one column per window of the range, so a cell's columns are distinct and ascending)."""
    rng = np.random.default_rng(seed)

    def spread(n_cols, per):
        win = n_cols // per
        return np.arange(per)[None, :] * win + rng.integers(0, win, (B, per))

    per_out = PER_CELL // 10
    cols = np.concatenate([spread(G, PER_CELL), G + spread(N_OUTSIDE, per_out)], axis=1).astype(np.int32)
    vals = rng.geometric(0.4, cols.shape).astype(np.float32)
    per = PER_CELL + per_out
    return sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(B + 1, dtype=np.int64) * per), shape=(B, G + N_OUTSIDE))


def panel_specs(names, P, kind, seed):
    """(panels, without, column masks bool [P, n_cols]) of P panels over the caller's column names."""
    rng = np.random.default_rng(seed)
    keep, without, masks = {}, {}, []
    for p in range(P):
        complement = kind == "without100" or (kind == "mix" and p % 2 == 1)
        ids = rng.choice(len(names), REMOVE if complement else KEEP, replace=False)
        m = np.zeros(len(names), bool)
        m[ids] = True
        (without if complement else keep)[f"p{p}"] = [names[i] for i in ids]
        masks.append(~m if complement else m)
    order = [int(n[1:]) for n in list(keep) + list(without)]        # panels() lists the keep panels first
    return keep, without, np.stack(masks)[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--panels", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max-pairs", type=int, default=200_000)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, outside=N_OUTSIDE, per_cell=PER_CELL, hidden=HIDDEN, classes=N_CLS, keep=KEEP, remove=REMOVE),
               device=torch.cuda.get_device_name(0), rows=[])
    names = [f"Gene{i}" for i in range(G)] + [f"Outside{i}" for i in range(N_OUTSIDE)]
    for n_layers in args.layers:
        with tempfile.TemporaryDirectory() as td:
            write_bundle(Path(td), n_layers)
            rp = sda.ResidentPredictor("mouse", f"Timing{n_layers}", model_path=td, unsure_rate=1.5)
            gmap = rp.gene_map(names)
            for B in args.batches:
                host = count_batch(B, 100 + B)
                rowptr, col, val = (torch.from_numpy(a).cuda() for a in (host.indptr, host.indices, host.data))
                rows = torch.repeat_interleave(torch.arange(B, device="cuda"), rowptr[1:] - rowptr[:-1])
                for P in args.panels:
                    kinds = ["mix"] + (["keep500", "without100"] if (B, P) == (2000, 64) else [])
                    for kind in kinds:
                        keep, without, masks = panel_specs(names, P, kind, 7 * P + B)
                        dev_masks = torch.from_numpy(masks).cuda()
                        for renorm in (False, True):
                            norm = "lognorm" if renorm else None

                            def panels_route():
                                return rp.panels((rowptr, col, val), panels=keep, without=without, genes=names, normalize=norm,
                                                 renormalize=renorm)

                            def device_route():
                                out = []
                                for p in range(P):
                                    on = dev_masks[p][col.long()]
                                    sub_ptr = torch.cat([on.new_zeros(1, dtype=torch.int64), torch.cumsum(on, 0)])[rowptr]
                                    sub = (sub_ptr, col[on], val[on])
                                    spec = None
                                    if renorm:
                                        lib = torch.zeros(B, dtype=torch.float64, device="cuda").index_add_(0, rows[on], val[on].double())
                                        spec = sda.LogNormalize(library_size=lib)
                                    out.append(rp.classify(sub, genes=gmap, normalize=spec)[0])
                                return np.stack(out, 1)

                            def host_route():
                                out = []
                                for p in range(P):
                                    sub = host.multiply(masks[p][None, :]).tocsr()
                                    sub.eliminate_zeros()
                                    out.append(rp.classify(sub, genes=gmap, normalize=norm)[0])
                                return np.stack(out, 1)

                            fns = {"panels": panels_route, "device": device_route}
                            if B * P <= args.host_max_pairs and kind == "mix":
                                fns["host"] = host_route
                            timed_alternating(fns, 1)                                # warm-up
                            ms = timed_alternating(fns, args.reps)
                            pc = panels_route()
                            row = dict(layers=n_layers, batch=B, panels=P, kind=kind, renormalize=renorm, nnz=int(host.nnz),
                                       **{f"{k}_wall_ms": ms.get(k) for k in ("panels", "device", "host")},
                                       panels_over_device=ms["panels"] / ms["device"],
                                       panels_over_host=ms["panels"] / ms["host"] if "host" in ms else None,
                                       mean_agreement=float(np.nanmean(pc.agreement())),
                                       same_labels_as_device_route=bool((pc.panel_label == device_route()).all()))
                            print(json.dumps(row), flush=True)
                            rec["rows"].append(row)
                            if args.out:                                             # after every row: a run cut short keeps its rows
                                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                del rowptr, col, val, rows
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
