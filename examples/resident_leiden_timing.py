"""Timing of ops.leiden_graph / ResidentPredictor.leiden against ops.louvain_graph on the same graph (profiles/resident_leiden.md).

Shapes, rows and lists: those of examples/resident_louvain_timing.py - B in {2 000, 20 000, 100 000} cells x D = 200, k = 15, 32
seeded Gaussian blobs, the exact kNN lists from ops.knn_rows (not timed), shared-neighbour weights, resolution 1.  Per shape, in
one process, the routes ALTERNATING inside every repetition:
  move_sweep   - one wgnn_louvain_sweep launch on the level-0 graph, every cell its own community: the yardstick kernel
  refine_sweep - one wgnn_leiden_refine_sweep launch on the level-0 graph in the refinement's initial state (ref = identity) inside
                 the partition P that louvain_graph's first level left: the kernel alone, no read-back
  refine_late  - the same launch on the state after the refinement's first kept sweep, when most vertices may no longer move
  boundary     - one wgnn_leiden_boundary launch (ext and kinP) on the initial state
  refine_step  - a whole refinement step as leiden_graph runs it: boundary, refine sweep, accept, wgnn_louvain_apply,
                 wgnn_louvain_modularity and the read-back of the four integers
  louvain_graph, leiden_graph - the whole calls on the same graph (all levels, every read-back, the aggregations)
  louvain, leiden - the whole ResidentPredictor calls on the synthetic batch of examples/resident_rank_genes_timing.py
  host         - igraph's / leidenalg's Leiden on the same graph when one of them can be imported (networkx has none); else not run
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`move_sweeps` / `refine_sweeps`: all sweeps of all levels of leiden_graph; `louvain_sweeps`: louvain_graph's.  `q` / `louvain_q`:
the two modularities; `louvain_disconnected`: how many of louvain_graph's communities are disconnected on the graph (scipy, host).

One batch size per process, each under its own time limit; rows are merged into --out by batch and the .md is rewritten:

    timeout -k 10 600 python examples/resident_leiden_timing.py --out profiles/resident_leiden.json --batches 2000
"""
import argparse
import json
import sys
import tempfile
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

D, K_NN = HIDDEN, 15


def disconnected(rowptr, col, label):
    """How many communities of ``label`` have a disconnected induced subgraph (host, scipy)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col, label = rowptr.cpu().numpy(), col.cpu().numpy(), label.cpu().numpy()
    n = len(label)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    keep = label[row] == label[col]
    _, part = connected_components(csr_matrix((np.ones(int(keep.sum())), (row[keep], col[keep])), shape=(n, n)), directed=False)
    pairs = np.unique(np.stack([label, part]), axis=1)
    return int((np.bincount(pairs[0][pairs[0] >= 0]) > 1).sum())


def write_md(rec, path):
    lines = ["# ResidentPredictor.leiden: the integer Leiden against the integer Louvain on the same graph", "",
             f"Measured by `examples/resident_leiden_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k = {K_NN}, shared-neighbour weights, resolution 1; wall ms per call.", "",
             "| cells | stored edges | move sweep | refine sweep | refine sweep, late | boundary | refine step | louvain_graph | "
             "leiden_graph | leiden / louvain | sweeps (move + refine; louvain) | levels (leiden; louvain) | louvain() | leiden() | "
             "Q | louvain Q | louvain disconnected | host Leiden |", "|" + "---|" * 18]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        host = "not run" if r["host_wall_ms"] is None else f"{r['host_wall_ms']:.0f}"
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['move_sweep_wall_ms']:.3f} | {r['refine_sweep_wall_ms']:.3f} | "
                     f"{r['refine_late_wall_ms']:.3f} | {r['boundary_wall_ms']:.3f} | {r['refine_step_wall_ms']:.3f} | "
                     f"{r['louvain_graph_wall_ms']:.1f} | {r['leiden_graph_wall_ms']:.1f} | "
                     f"{r['leiden_graph_wall_ms'] / r['louvain_graph_wall_ms']:.2f} | {r['move_sweeps']} + {r['refine_sweeps']}; "
                     f"{r['louvain_sweeps']} | {r['levels']}; {r['louvain_levels']} | {r['louvain_wall_ms']:.1f} | "
                     f"{r['leiden_wall_ms']:.1f} | {r['q']:.4f} | {r['louvain_q']:.4f} | {r['louvain_disconnected']} | {host} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def host_leiden(row, col, w, B):
    """Wall ms of a host Leiden on the same graph, or None when neither igraph nor leidenalg can be imported."""
    import time
    try:
        import igraph
    except ImportError:
        return None
    up = row < col
    g = igraph.Graph(n=B, edges=list(zip(row[up].tolist(), col[up].tolist())))
    t0 = time.perf_counter()
    g.community_leiden(objective_function="modularity", weights=w[up].tolist())
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, k=K_NN, inner=args.inner, reps=args.reps), device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            batch = device_batch(B)
            gen = torch.Generator("cuda").manual_seed(B)
            centres = torch.randn((32, D), device="cuda", generator=gen)
            rows = centres[torch.randint(0, 32, (B,), device="cuda", generator=gen)] + torch.randn((B, D), device="cuda", generator=gen)
            idx, _ = ops.knn_rows(rows, K_NN)
            dev = rows.device
            rowptr, col, w = ops.snn_graph(idx)
            nnz = int(col.shape[0])
            M = int(w.sum(dtype=torch.int64))
            row = torch.repeat_interleave(torch.arange(B, device=dev), rowptr[1:] - rowptr[:-1], output_size=nnz)
            deg = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, row, w.long())
            ids = torch.arange(B, dtype=torch.int32, device=dev)
            ones = torch.ones(B, dtype=torch.int32, device=dev)
            lens = rowptr[1:] - rowptr[:-1]
            heavy = torch.nonzero(lens > ops.LOUVAIN_WAVE_ROWS).reshape(-1).to(torch.int32)
            assert int(lens.max()) <= ops.LOUVAIN_BLOCK_ROWS, "a hub row: this script sizes no scratch"
            routes = (_ptr(heavy) if len(heavy) else None, len(heavy), ops.LOUVAIN_WAVE_ROWS, ops.LOUVAIN_BLOCK_ROWS)
            stream = _stream(dev)
            stats = torch.zeros(4, dtype=torch.int64, device=dev)
            nxt, gain = torch.empty_like(ids), torch.empty_like(deg)
            # P: what the moving phase of level 0 leaves (ids of its own, as the sweeps leave them, are any ids in [0, B))
            first = ops.louvain_graph(rowptr, col, w)
            P = first.level_labels[0].to(torch.int32)
            P = torch.full((B,), B, dtype=torch.int32, device=dev).scatter_reduce_(0, P.long(), ids, "amin")[P.long()]   # the founder's id
            totP = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, P.long(), deg)
            ext, kinP = torch.empty_like(deg), torch.empty_like(deg)
            prop, late = torch.empty_like(ids), torch.empty_like(ids)
            tot2, size2 = torch.empty_like(deg), torch.empty_like(ones)

            def move_sweep():
                _lib.run(dev, "wgnn_louvain_sweep", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(ids), _ptr(deg), _ptr(deg),
                         _ptr(ones), M, 1, 0, *routes, _ptr(nxt), _ptr(gain), _ptr(stats), None, 0, 0, 0, stream)

            def boundary(ref=ids, out=ext):
                _lib.run(dev, "wgnn_leiden_boundary", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(P), _ptr(ref), _ptr(out),
                         _ptr(kinP), _ptr(stats), 0, stream)

            def refine_sweep(ref=ids, tot=deg, size=ones, ext=ext, r=0, out=prop):
                _lib.run(dev, "wgnn_leiden_refine_sweep", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(P), _ptr(ref), _ptr(deg),
                         _ptr(totP), _ptr(tot), _ptr(size), _ptr(ext), _ptr(kinP), M, 1, r, *routes, _ptr(out), _ptr(gain),
                         _ptr(stats), None, 0, 0, 0, stream)

            def refine_step():
                boundary()
                refine_sweep()
                _lib.run(dev, "wgnn_leiden_accept", _ptr(ids), _ptr(prop), B, _ptr(nxt), _ptr(gain), _ptr(stats), 0, stream)
                _lib.run(dev, "wgnn_louvain_apply", _ptr(ids), _ptr(nxt), _ptr(deg), B, _ptr(tot2), _ptr(size2), _ptr(stats), 0, stream)
                _lib.run(dev, "wgnn_louvain_modularity", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(nxt), _ptr(tot2), _ptr(stats),
                         0, stream)
                return stats.tolist()

            refine_step()                                              # the state after the first sweep, for refine_late
            ref1, tot1, size1, ext1 = nxt.clone(), tot2.clone(), size2.clone(), torch.empty_like(deg)
            boundary(ref1, ext1)

            def refine_late():
                refine_sweep(ref1, tot1, size1, ext1, 1, late)

            def louvain_graph():
                return ops.louvain_graph(rowptr, col, w)

            def leiden_graph():
                return ops.leiden_graph(rowptr, col, w)

            inner = args.inner if B <= 20000 else 1
            fns = {"move_sweep": (move_sweep, inner), "refine_sweep": (refine_sweep, inner), "refine_late": (refine_late, inner),
                   "boundary": (boundary, inner), "refine_step": (refine_step, inner), "louvain_graph": (louvain_graph, 1),
                   "leiden_graph": (leiden_graph, 1), "louvain": (lambda: rp.louvain(batch, k=K_NN), 1),
                   "leiden": (lambda: rp.leiden(batch, k=K_NN), 1)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)
            out, lou = leiden_graph(), louvain_graph()
            assert disconnected(rowptr, col, out.cluster) == 0
            host_ms = host_leiden(row.cpu().numpy(), col.cpu().numpy(), w.cpu().numpy(), B)
            rec_row = dict(batch=B, nnz=nnz, M=M, **{f"{name}_wall_ms": v for name, v in ms.items()},
                           move_sweeps=sum(level["sweeps"] for level in out.levels),
                           refine_sweeps=sum(level["refine_sweeps"] for level in out.levels),
                           refine_fallback_moves=sum(level["refine_fallback_moves"] for level in out.levels),
                           split=out.levels[-1]["split"], louvain_sweeps=sum(level["sweeps"] for level in lou.levels),
                           levels=len(out.levels), louvain_levels=len(lou.levels), n_clusters=int(out.cluster.max()) + 1,
                           louvain_clusters=int(lou.cluster.max()) + 1, q=out.modularity, louvain_q=lou.modularity,
                           louvain_disconnected=disconnected(rowptr, col, lou.cluster), movers_late=int((size1[ref1.long()] == 1).sum()),
                           host_wall_ms=host_ms)
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
