"""Timing of ResidentPredictor.rank_genes' ranking op against three yardsticks (profiles/resident_rank_genes.md).

Bundle as examples/resident_predict_timing.py (G = 20 000 genes, hidden 200, C = 16 classes, a randomly initialised 1-layer
model); the batch is synthetic.synth_expression's (the benchmark's gene-popularity curve, density 0.04: a few genes in almost
every cell, most in few), B in {2 000, 20 000, 100 000} cells on the device - above 20 000 cells the 20 000-cell batch is
repeated on the device - in K = 16 groups of equal size, every cell taking part.  Per shape, in one process, the calls
ALTERNATING inside every repetition:
  ranking   - ops.rank_genes_groups: the stable transpose and the wgnn_rank_genes_groups launch (four kernels)
  transpose - the transpose alone (graph._transpose_on_device), which `ranking` contains
  classify  - ResidentPredictor.classify of the same batch: the launch rank_genes(groups="predicted") runs first, unchanged
  framework - dense gene-major columns in chunks of --chunk-genes genes: torch.sort along the cells, the doubled mid-ranks by
              two torch.searchsorted, the groups' sums by index_add_
  host      - per gene scipy.stats.rankdata on the densified column and np.add.at per group; timed on the first --host-genes
              genes (gene ids carry no popularity order) and scaled to G (host_genes_timed says how many were timed)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.  host runs once, after the alternating rounds.
`ranking_over_*` are ratios of wall_ms; below 1 the kernel is faster.  `rank_genes_wall_ms` is the whole call with the same
groups given per cell (both reductions with a transpose each, the read-back and the fp64 host step; no classify) for
orientation.  `compares` is the cost model, the sum over genes of (stored entries)^2.  Every route's integer tables are
compared with the kernel's (`framework_equal`, `host_equal`).

One batch size per process, each under its own time limit; rows are merged into --out by batch size and the .md is rewritten:

    timeout -k 10 900 python examples/resident_rank_genes_timing.py --out profiles/resident_rank_genes.json --batches 2000
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from scipy.stats import rankdata

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_predict_timing import G, HIDDEN, N_CLS, write_bundle      # noqa: E402
from resident_signatures_timing import timed_alternating      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import ops, synthetic                      # noqa: E402
from scdeepsort_amd.graph import _transpose_on_device          # noqa: E402

K, DENSITY, DRAWN_CELLS = 16, 0.04, 20_000


def device_batch(B):
    rowptr, col, val = synthetic.synth_expression(min(B, DRAWN_CELLS), G, DENSITY, device="cuda")
    times = -(-B // DRAWN_CELLS) if B > DRAWN_CELLS else 1
    if times > 1:
        deg = (rowptr[1:] - rowptr[:-1]).repeat(times)
        rowptr = torch.cat([rowptr[:1], torch.cumsum(deg, 0)])
        col, val = col.repeat(times), val.repeat(times)
    return rowptr, col, val


def write_md(rec, path):
    lines = ["# ResidentPredictor.rank_genes: the ranking op against three yardsticks", "",
             f"Measured by `examples/resident_rank_genes_timing.py` on {rec['device']}; its docstring defines every column.",
             f"G = {G} genes, K = {K} groups, the benchmark's gene-popularity curve at density {DENSITY}; wall ms per call.", "",
             "| cells | nnz | compares | ranking | transpose | classify | framework | host (scaled) | ranking / classify | "
             "ranking / framework | ranking / host | rank_genes() | tables equal |", "|" + "---|" * 13]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['compares']:.2e} | {r['ranking_wall_ms']:.2f} | {r['transpose_wall_ms']:.2f} | "
                     f"{r['classify_wall_ms']:.2f} | {r['framework_wall_ms']:.1f} | {r['host_wall_ms']:.0f} | "
                     f"{r['ranking_over_classify']:.2f} | {r['ranking_over_framework']:.3f} | {r['ranking_over_host']:.5f} | "
                     f"{r['rank_genes_wall_ms']:.1f} | {r['framework_equal'] and r['host_equal']} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--chunk-genes", type=int, default=500)
    ap.add_argument("--host-genes", type=int, default=200)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, hidden=HIDDEN, classes=N_CLS, groups=K, density=DENSITY, chunk_genes=args.chunk_genes,
                          inner=args.inner, reps=args.reps), device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td, unsure_rate=1.5)
        for B in args.batches:
            rowptr, col, val = device_batch(B)
            nnz = int(col.shape[0])
            rows = torch.repeat_interleave(torch.arange(B, device="cuda"), rowptr[1:] - rowptr[:-1])
            group = (torch.arange(B, device="cuda") % K)[torch.randperm(B, device="cuda", generator=torch.Generator("cuda").manual_seed(B))]
            group32, rowptr32 = group.to(torch.int32), rowptr.to(torch.int32)
            n_g = torch.bincount(col.long(), minlength=G)
            compares = float((n_g.double() ** 2).sum())

            def ranking():
                return ops.rank_genes_groups(rowptr, col, val, group32, K, G, check=False)

            def transpose():
                return _transpose_on_device(rowptr32, col, val, B, G, group32 >= 0)

            def classify():
                return rp.classify((rowptr, col, val))

            def framework():
                r2 = torch.zeros((K, G), dtype=torch.int64, device="cuda")
                cnt = torch.zeros((K, G), dtype=torch.int64, device="cuda")
                tie = torch.zeros(G, dtype=torch.int64, device="cuda")
                order = torch.sort(col.to(torch.int16) if G < 2 ** 15 else col, stable=True).indices
                s_col, s_row, s_val = col[order].long(), rows[order], val[order]
                ptr = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
                torch.cumsum(n_g, 0, out=ptr[1:])
                for g0 in range(0, G, args.chunk_genes):
                    g1 = min(G, g0 + args.chunk_genes)
                    e0, e1 = int(ptr[g0]), int(ptr[g1])
                    dense = torch.zeros((g1 - g0, B), dtype=torch.float32, device="cuda")
                    dense[s_col[e0:e1] - g0, s_row[e0:e1]] = s_val[e0:e1]
                    ordered = torch.sort(dense, dim=1).values
                    lt = torch.searchsorted(ordered, dense, right=False)
                    le = torch.searchsorted(ordered, dense, right=True)
                    r2[:, g0:g1].index_add_(0, group, (lt + le + 1).t())                  # 2 lt + eq + 1
                    cnt[:, g0:g1].index_add_(0, group, (dense != 0).t().to(torch.int64))
                    eq = le - lt
                    tie[g0:g1] = (eq * eq - 1).sum(dim=1)
                return r2, cnt.to(torch.int32), tie

            n_host = min(G, args.host_genes)

            def host():
                t_rowptr, t_cell, t_val = (x.cpu().numpy() for x in transpose())
                grp = group.cpu().numpy()
                r2, cnt, tie = np.zeros((K, n_host), np.int64), np.zeros((K, n_host), np.int32), np.zeros(n_host, np.int64)
                t0 = time.perf_counter()
                for g in range(n_host):
                    column = np.zeros(B, np.float32)
                    b, e = t_rowptr[g], t_rowptr[g + 1]
                    column[t_cell[b:e]] = t_val[b:e]
                    np.add.at(r2[:, g], grp, np.rint(2.0 * rankdata(column, "average")).astype(np.int64))
                    np.add.at(cnt[:, g], grp, (column != 0).astype(np.int32))
                    t = np.unique(column, return_counts=True)[1].astype(np.int64)
                    tie[g] = (t ** 3 - t).sum()
                return (r2, cnt, tie), 1e3 * (time.perf_counter() - t0) * (G / n_host)

            def whole():
                return rp.rank_genes((rowptr, col, val), groups=group, n_groups=K)

            fns = {"ranking": (ranking, args.inner), "transpose": (transpose, args.inner), "classify": (classify, args.inner),
                   "framework": (framework, 1), "rank_genes": (whole, 1)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)
            host_tables, host_ms = host()
            got = [x.cpu().numpy() for x in ranking()[:3]]
            same = lambda a, b: bool(all(np.array_equal(x, y) for x, y in zip(a, b)))
            row = dict(batch=B, nnz=nnz, compares=compares, longest_gene=int(n_g.max()), ranking_wall_ms=ms["ranking"],
                       transpose_wall_ms=ms["transpose"], classify_wall_ms=ms["classify"], framework_wall_ms=ms["framework"],
                       host_wall_ms=host_ms, host_genes_timed=n_host, rank_genes_wall_ms=ms["rank_genes"],
                       ranking_over_classify=ms["ranking"] / ms["classify"], ranking_over_framework=ms["ranking"] / ms["framework"],
                       ranking_over_host=ms["ranking"] / host_ms,
                       framework_equal=same([x.cpu().numpy() for x in framework()], got),
                       host_equal=same(host_tables, [got[0][:, :n_host], got[1][:, :n_host], got[2][:n_host]]))
            print(json.dumps(row), flush=True)
            assert row["framework_equal"] and row["host_equal"], "the routes' integer tables differ"
            rec["rows"].append(row)
            if args.out:                                                                         # after every batch size
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                write_md(rec, Path(args.out).with_suffix(".md"))
            del rowptr, col, val, rows
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
