"""Timing of ResidentPredictor.bbknn's search op against two yardsticks (profiles/resident_bbknn.md).

Shapes: B in {2 000, 20 000, 100 000} rows x D = 200, seeded standard-normal float32 rows made on the device (distances
concentrate: the hard case for the staging lists), S in {4, 16} equal batches dealt round-robin (row i is of batch i % S, so
the gather by `order` is a real one), k_within = 3.  Per shape, in one process, the routes ALTERNATING inside every repetition:
  launch      - ops.knn_segments: the stable sort of the batch ids, wgnn_knn_segments' two kernels, the status read-back
  composition - what the package offered before: per batch the rows gathered into a copy and two ops.knn_rows calls on it, the
                batch's own rows as queries with exclude_self and all other rows without, the lists translated back to row
                ids on the device; then the merged list by a stable sort on the id and one on the distance.  2 S searches,
                S gathers of the candidates, S gathers of the queries
  framework   - the rows copied batch-major once per call; chunks of queries: torch.cdist against that copy, the query's own
                column set to +inf, per batch torch.topk(largest=False) over the batch's slice of columns; the chunk keeps the
                [chunk, B] float32 distance block under --chunk-bytes
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`launch_share_of_peak`: B * B * D * 3 flop (a subtract and a fused multiply-add per pair and column) over launch wall time,
over the float32 vector peak of 157.3 Tflop/s - a whole-call rate over peak, not a kernel-trace figure.
`composition_same_cells`: the share of cells whose [S, k] lists AND merged list equal the launch's, ids and distance bits (the
composition runs the same distance chain; it leaves the order of equal distances ACROSS batches to its sort, which the two
stable sorts here settle by id as the kernel does).  `framework_same_cells`: the share of cells whose [S, k] id lists equal the
launch's (norm-form distances through a GEMM: near-ties may order differently).

One batch size per process, each under its own time limit; rows are merged into --out by (batch, S) and the .md is rewritten:

    timeout -k 10 600 python examples/resident_bbknn_timing.py --out profiles/resident_bbknn.json --batches 2000
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resident_signatures_timing import timed_alternating      # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import ops                                 # noqa: E402

D, SEGS, K_WITHIN, PEAK_TFLOPS = 200, (4, 16), 3, 157.3


def merged_by_sort(idx, d2):
    """[n, S, k] lists as one list by (d2, id): a stable sort on the id, then one on the distance; -1 / +inf entries last."""
    n = idx.shape[0]
    flat_i, flat_d = idx.reshape(n, -1), d2.reshape(n, -1)
    by_id = torch.sort(torch.where(flat_i < 0, torch.full_like(flat_i, 2 ** 31 - 1), flat_i), dim=1, stable=True).indices
    flat_i, flat_d = torch.gather(flat_i, 1, by_id), torch.gather(flat_d, 1, by_id)
    by_d = torch.sort(flat_d, dim=1, stable=True).indices
    return torch.gather(flat_i, 1, by_d), torch.gather(flat_d, 1, by_d)


def composition(rows, group, S, k):
    n = rows.shape[0]
    idx = torch.full((n, S, k), -1, dtype=torch.int32, device=rows.device)
    d2 = torch.full((n, S, k), float("inf"), device=rows.device)
    for s in range(S):
        members, others = torch.nonzero(group == s).flatten(), torch.nonzero(group != s).flatten()
        gathered = rows[members]
        back = members.to(torch.int32)
        for queries, found in ((members, ops.knn_rows(gathered, k)), (others, ops.knn_rows(gathered, k, queries=rows[others], exclude_self=False))):
            idx[queries, s] = torch.where(found[0] >= 0, back[found[0].clamp(min=0).long()], found[0])
            d2[queries, s] = found[1]
    return (idx, d2) + merged_by_sort(idx, d2)


def framework(rows, group, S, k, chunk_bytes):
    n = rows.shape[0]
    order, seg_ptr = ops._group_major(group, S)
    order = order.long()
    at = torch.empty_like(order)
    at[order] = torch.arange(n, device=rows.device)                               # a row's column in the batch-major copy
    major, bounds = rows[order], seg_ptr.tolist()
    idx = torch.empty((n, S, k), dtype=torch.int64, device=rows.device)
    step = max(1, min(n, chunk_bytes // (4 * n)))
    for r0 in range(0, n, step):
        d = torch.cdist(rows[r0:r0 + step], major)
        m = d.shape[0]
        d[torch.arange(m, device=rows.device), at[r0:r0 + m]] = float("inf")
        for s in range(S):
            idx[r0:r0 + m, s] = order[bounds[s] + torch.topk(d[:, bounds[s]:bounds[s + 1]], k, dim=1, largest=False).indices]
    return idx


def write_md(rec, path):
    lines = ["# ResidentPredictor.bbknn: the segmented search against the composition it replaces and a framework route", "",
             f"Measured by `examples/resident_bbknn_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k_within = {K_WITHIN}; wall ms per call.", "",
             "| rows | batches | splits per batch | launch | share of f32 vector peak | composition | framework | launch / composition | "
             "launch / framework | composition same cells | framework same cells |", "|" + "---|" * 11]
    for r in sorted(rec["rows"], key=lambda r: (r["batch"], r["segs"])):
        lines.append(f"| {r['batch']} | {r['segs']} | {r['splits']} | {r['launch_wall_ms']:.2f} | {r['launch_share_of_peak']:.3f} | "
                     f"{r['composition_wall_ms']:.2f} | {r['framework_wall_ms']:.2f} | "
                     f"{r['launch_wall_ms'] / r['composition_wall_ms']:.3f} | {r['launch_wall_ms'] / r['framework_wall_ms']:.3f} | "
                     f"{r['composition_same_cells']:.4f} | {r['framework_same_cells']:.4f} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    rec = dict(shape=dict(D=D, k_within=K_WITHIN, inner=args.inner, reps=args.reps, chunk_bytes=args.chunk_bytes),
               device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    for B in args.batches:
        rows = torch.randn((B, D), device="cuda", generator=torch.Generator("cuda").manual_seed(B))
        for S in SEGS:
            group = torch.arange(B, device="cuda") % S
            inner = args.inner if B <= 20000 else 2
            fns = {"launch": (lambda: ops.knn_segments(rows, group, S, K_WITHIN), inner),
                   "composition": (lambda: composition(rows, group, S, K_WITHIN), inner),
                   "framework": (lambda: framework(rows, group, S, K_WITHIN, args.chunk_bytes), inner)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps if B <= 20000 else 3)
            got, comp, fw = fns["launch"][0](), fns["composition"][0](), fns["framework"][0]()
            same = torch.ones(B, dtype=torch.bool, device="cuda")
            for mine, theirs in zip(got, comp):
                eq = mine == theirs if mine.dtype == torch.int32 else mine.view(torch.int32) == theirs.view(torch.int32)
                same &= eq.reshape(B, -1).all(dim=1)
            fw_same = (got.idx.long() == fw).reshape(B, -1).all(dim=1)
            nb = ctypes.c_int64()
            sda._lib.lib().wgnn_knn_segments_workspace_bytes(B, B, S, K_WITHIN, 0, ctypes.addressof(nb))
            row = dict(batch=B, segs=S, k_within=K_WITHIN, splits=nb.value // (8 * B * K_WITHIN * S), launch_wall_ms=ms["launch"],
                       composition_wall_ms=ms["composition"], framework_wall_ms=ms["framework"],
                       launch_share_of_peak=3.0 * B * B * D / (ms["launch"] * 1e-3) / (PEAK_TFLOPS * 1e12),
                       composition_same_cells=float(same.float().mean()), framework_same_cells=float(fw_same.float().mean()))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            if args.out:                                                                         # after every (batch, S)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                write_md(rec, Path(args.out).with_suffix(".md"))
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
