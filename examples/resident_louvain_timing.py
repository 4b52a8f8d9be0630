"""Timing of ops.snn_graph / ops.louvain_graph / ResidentPredictor.louvain against the host (profiles/resident_louvain.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200 (the hidden width of the timing bundle of
examples/resident_predict_timing.py), k = 15.  Rows: 32 seeded unit-variance Gaussians around N(0, 1) centres, float32 [B, D] made
on the device; their exact kNN lists come from ops.knn_rows and are not timed here (profiles/resident_knn.md has that launch).
Per shape, in one process, the routes ALTERNATING inside every repetition:
  snn        - ops.snn_graph on the lists: the 64-bit keys, sort and unique with framework ops, then wgnn_snn_weights
  sweep      - one wgnn_louvain_sweep launch on the level-0 graph in its initial state (every cell its own community): the kernel
               alone, no read-back
  step       - a whole sweep step as louvain_graph runs it: sweep, wgnn_louvain_apply, wgnn_louvain_modularity and the read-back of
               the four integers - what a sweep costs with its host synchronisation
  framework  - one sweep's decisions with framework ops alone: kin per (vertex, community) by a 64-bit key sort + unique + integer
               index_add_, the int64 scores, the gate, and a sort for the best candidate per vertex (no apply, no modularity)
  graph      - the whole ops.louvain_graph (all levels, every sweep's read-back, the aggregations)
  louvain    - the whole ResidentPredictor.louvain call on the synthetic batch of examples/resident_rank_genes_timing.py (classify,
               embed, the kNN search, snn_graph, louvain_graph, the table)
  host       - networkx.community.louvain_communities(seed=0) on the same weighted graph, graph construction not counted, up to
               --host-max-cells cells; run once, after the rounds
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`sweeps`: all sweeps of all levels of `graph`; `step_share`: sweeps * step / graph - how much of the whole is sweep steps, the rest
being the per-level set-up and the aggregation.  `q` / `host_q`: the two modularities.

One batch size per process, each under its own time limit; rows are merged into --out by batch and the .md is rewritten:

    timeout -k 10 600 python examples/resident_louvain_timing.py --out profiles/resident_louvain.json --batches 2000
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

D, K_NN = HIDDEN, 15


def write_md(rec, path):
    lines = ["# ResidentPredictor.louvain: the integer Louvain against a framework sweep and networkx on the host", "",
             f"Measured by `examples/resident_louvain_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k = {K_NN}, shared-neighbour weights, resolution 1; wall ms per call.", "",
             "| cells | stored edges | snn_graph | sweep kernel | sweep step | framework sweep | kernel / framework | sweeps | levels | "
             "louvain_graph | step share | louvain() | networkx | Q | networkx Q |", "|" + "---|" * 15]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        host = "not run" if r["host_wall_ms"] is None else f"{r['host_wall_ms']:.0f}"
        host_q = "-" if r["host_q"] is None else f"{r['host_q']:.4f}"
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['snn_wall_ms']:.2f} | {r['sweep_wall_ms']:.3f} | {r['step_wall_ms']:.3f} | "
                     f"{r['framework_wall_ms']:.2f} | {r['sweep_wall_ms'] / r['framework_wall_ms']:.3f} | {r['sweeps']} | "
                     f"{r['levels']} | {r['graph_wall_ms']:.1f} | {r['step_share']:.2f} | {r['louvain_wall_ms']:.1f} | {host} | "
                     f"{r['q']:.4f} | {host_q} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--host-max-cells", type=int, default=20000)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, D=D, k=K_NN, inner=args.inner, reps=args.reps), device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    try:
        import networkx as nx
    except ImportError:
        nx = None
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
            comm = torch.arange(B, dtype=torch.int32, device=dev)
            tot, size = deg.clone(), torch.ones(B, dtype=torch.int32, device=dev)
            nxt, gain = torch.empty_like(comm), torch.empty_like(deg)
            tot2, size2 = torch.empty_like(tot), torch.empty_like(size)
            stats = torch.zeros(4, dtype=torch.int64, device=dev)
            lens = rowptr[1:] - rowptr[:-1]
            heavy = torch.nonzero(lens > ops.LOUVAIN_WAVE_ROWS).reshape(-1).to(torch.int32)
            assert int(lens.max()) <= ops.LOUVAIN_BLOCK_ROWS, "a hub row: this script sizes no scratch"
            stream = _stream(dev)

            def snn():
                return ops.snn_graph(idx)

            def sweep():
                _lib.run(dev, "wgnn_louvain_sweep", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(comm), _ptr(deg), _ptr(tot),
                         _ptr(size), M, 1, 0, _ptr(heavy) if len(heavy) else None, len(heavy), ops.LOUVAIN_WAVE_ROWS,
                         ops.LOUVAIN_BLOCK_ROWS, _ptr(nxt), _ptr(gain), _ptr(stats), None, 0, 0, 0, stream)

            def step():
                sweep()
                _lib.run(dev, "wgnn_louvain_apply", _ptr(comm), _ptr(nxt), _ptr(deg), B, _ptr(tot2), _ptr(size2), _ptr(stats), 0, stream)
                _lib.run(dev, "wgnn_louvain_modularity", _ptr(rowptr), _ptr(col), _ptr(w), B, nnz, _ptr(nxt), _ptr(tot2), _ptr(stats),
                         0, stream)
                return stats.tolist()

            def framework():
                cu = comm.long()[col.long()]
                key, inv = torch.unique(row * B + cu, return_inverse=True)
                kin = torch.zeros(key.shape[0], dtype=torch.int64, device=dev).index_add_(0, inv, w.long())
                v = torch.div(key, B, rounding_mode="floor")
                C = key - v * B
                own = comm.long()[v]
                score = kin * M - deg[v] * tot[C]
                ok = (C < own) & ~((size[own] == 1) & (size[C] == 1) & (C > own)) & (score > 0)      # singletons: score(own) = 0
                v, C, score = v[ok], C[ok], score[ok]
                order = torch.argsort(C, stable=True)
                order = order[torch.argsort(-score[order], stable=True)]
                order = order[torch.argsort(v[order], stable=True)]
                v, C = v[order], C[order]
                first = torch.ones_like(v, dtype=torch.bool)
                first[1:] = v[1:] != v[:-1]
                out = comm.long().clone()
                out[v[first]] = C[first]
                return out

            def graph():
                return ops.louvain_graph(rowptr, col, w)

            def whole():
                return rp.louvain(batch, k=K_NN)

            sweep()
            assert torch.equal(framework(), nxt.long()), "the framework sweep and the kernel disagree"
            inner = args.inner if B <= 20000 else 1
            fns = {"snn": (snn, inner), "sweep": (sweep, inner), "step": (step, inner), "framework": (framework, inner),
                   "graph": (graph, 1), "louvain": (whole, 1)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)
            out = graph()
            sweeps = sum(level["sweeps"] for level in out.levels)
            host_ms = host_q = None
            if nx is not None and B <= args.host_max_cells:
                g = nx.Graph()
                g.add_nodes_from(range(B))
                hr, hc, hw = row.cpu().numpy(), col.cpu().numpy(), w.cpu().numpy()
                up = hr < hc
                g.add_weighted_edges_from(zip(hr[up].tolist(), hc[up].tolist(), hw[up].tolist()))
                t0 = time.perf_counter()
                parts = nx.community.louvain_communities(g, weight="weight", seed=0)
                host_ms = 1e3 * (time.perf_counter() - t0)
                host_q = float(nx.community.modularity(g, parts, weight="weight"))
            rec_row = dict(batch=B, nnz=nnz, M=M, snn_wall_ms=ms["snn"], sweep_wall_ms=ms["sweep"], step_wall_ms=ms["step"],
                           framework_wall_ms=ms["framework"], graph_wall_ms=ms["graph"], louvain_wall_ms=ms["louvain"],
                           sweeps=sweeps, levels=len(out.levels), step_share=sweeps * ms["step"] / ms["graph"],
                           n_clusters=int(out.cluster.max()) + 1, q=out.modularity, host_wall_ms=host_ms, host_q=host_q,
                           longest_row=int(lens.max()), n_heavy=int(len(heavy)))
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
