"""Timing of ops.harmony_rows and its pieces against two yardsticks (profiles/resident_harmony.md).

Shapes: B in {2 000, 20 000, 100 000} rows x D = 200, S in {4, 16} batches dealt round-robin, K = min(round(B / 30), 100)
clusters, n_blocks = 20, theta = 2, sigma = 0.1.  The rows are seeded on the device: K / 2 standard-normal cluster centres
scaled by 3, a per-batch offset of 1.5 per column, unit noise.  Per shape, in one process:
  scores      - one ops.harmony_scores launch ([B, K] dot products over D, the row maximum, exp)
  block       - one block of the sweep: ops.harmony_assign_block and ops.harmony_fold, B / 20 cells
  iteration   - one clustering iteration as ops.harmony_rows runs it: the centres (ops.weighted_group_reduce with S = 1 and the
                unit rows), the scores, 1 + 2 x 20 launches of the sweep, the objective and its 8-byte read-back
  call        - the whole ops.harmony_rows call with its defaults (k-means++ seeding and the convergence tests included);
                `rounds` / `iterations` say how long it ran
  framework   - the same clustering iteration composed from float64 framework operations: a GEMM for the dot products, a
                softmax, per block an index_select, a one-hot GEMM for the block's table and pow for the penalty, the objective
                by elementwise operations and sums.  It computes the same quantities in the framework's own summation orders
  numpy       - the same iteration by tests/harmony_reference.py, the restatement the tests hold the kernels to (a Python
                loop per cell; timed at 2 000 rows only, once)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round, the routes ALTERNATING inside every repetition.
`iteration_vs_framework_R`: the largest absolute difference of the memberships R after that iteration from the same state.

One batch size per process, each under its own time limit; rows are merged into --out by (batch, S) and the .md is rewritten:

    timeout -k 10 600 python examples/resident_harmony_timing.py --out profiles/resident_harmony.json --batches 2000
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from resident_signatures_timing import timed_alternating      # noqa: E402
from scdeepsort_amd import ops                                 # noqa: E402

D, SEGS, N_BLOCKS, THETA, SIGMA = 200, (4, 16), 20, 2.0, 0.1


def cohort(B, S, K):
    g = torch.Generator("cuda").manual_seed(B + S)
    centres = 3.0 * torch.randn((max(2, K // 2), D), device="cuda", generator=g)
    offsets = 1.5 * torch.randn((S, D), device="cuda", generator=g)
    batch = (torch.arange(B, device="cuda") % S).to(torch.int32)
    kind = torch.randint(0, centres.shape[0], (B,), device="cuda", generator=g)
    return centres[kind] + offsets[batch.long()] + torch.randn((B, D), device="cuda", generator=g), batch


class State:
    """What ops.harmony_rows holds between two clustering iterations, after its first assignment."""

    def __init__(self, x, batch, S, K):
        B = x.shape[0]
        self.B, self.S, self.K, self.batch = B, S, K, batch
        self.U = ops.harmony_apply(x.double().contiguous())[1]
        self.Y = ops.harmony_apply(ops.kmeans_rows(self.U.float(), K, seed=0, max_iter=25).centers.double().contiguous())[1]
        self.theta = torch.full((S,), THETA, dtype=torch.float64, device="cuda")
        self.Pr = (torch.bincount(batch.long(), minlength=S).double() / B).contiguous()
        self.R = torch.empty((B, K), dtype=torch.float64, device="cuda")
        self.T = torch.zeros((N_BLOCKS, K, S), dtype=torch.float64, device="cuda")
        self.tables = tuple(torch.empty((K, S), dtype=torch.float64, device="cuda") for _ in range(3))
        self.rows = (torch.arange(B, dtype=torch.int32, device="cuda"), torch.tensor([0, B], dtype=torch.int64, device="cuda"))
        self.M, self.n = torch.empty((K, 1, D), dtype=torch.float64, device="cuda"), torch.empty((K, 1), dtype=torch.float64, device="cuda")
        self.dist, self.e = ops.harmony_scores(self.U, self.Y, SIGMA)[1:]
        self.ws = None
        for q in range(N_BLOCKS):
            self.block(q, first=True)

    def block(self, q, first=False):
        self.ws = ops.harmony_assign_block(self.e, self.batch, self.S, N_BLOCKS, q, self.R, pen=None if first else self.tables[2],
                                           workspace=self.ws)
        ops.harmony_fold(self.T, self.Pr, self.theta, self.B, q_store=q, q_skip=-1 if first or q + 1 == N_BLOCKS else q + 1,
                         workspace=self.ws, out=self.tables)

    def iteration(self):
        ops.weighted_group_reduce(self.U, self.R, None, 1, out=(self.M, self.n), major=self.rows)
        ops.harmony_apply(self.M.view(self.K, D), out=(self.M.view(self.K, D), self.Y))
        self.dist, self.e = ops.harmony_scores(self.U, self.Y, SIGMA)[1:]
        ops.harmony_fold(self.T, self.Pr, self.theta, self.B, q_skip=0, out=self.tables)
        for q in range(N_BLOCKS):
            self.block(q)
        return float(ops.harmony_objective(self.R, self.dist, self.batch, self.tables[0], self.tables[1], self.theta, SIGMA)[0])


def framework_iteration(U, R, batch, Pr, theta):
    """One clustering iteration from float64 framework operations; returns (R, objective)."""
    B, S = U.shape[0], Pr.shape[0]
    onehot = torch.nn.functional.one_hot(batch.long(), S).double()
    Y = torch.nn.functional.normalize(R.T @ U, dim=1)
    dist = 2.0 * (1.0 - U @ Y.T)
    e = torch.softmax(-dist / SIGMA, dim=1)
    R = R.clone()
    T = torch.stack([R[q::N_BLOCKS].T @ onehot[q::N_BLOCKS] for q in range(N_BLOCKS)])
    for q in range(N_BLOCKS):
        O = T.sum(dim=0) - T[q]
        E = O.sum(dim=1, keepdim=True) * Pr[None, :]
        pen = torch.pow((E + 1.0) / (O + 1.0), theta[None, :])
        t = e[q::N_BLOCKS] * pen.T[batch[q::N_BLOCKS].long()]
        R[q::N_BLOCKS] = t / t.sum(dim=1, keepdim=True)
        T[q] = R[q::N_BLOCKS].T @ onehot[q::N_BLOCKS]
    O = T.sum(dim=0)
    E = O.sum(dim=1, keepdim=True) * Pr[None, :]
    cross = (theta[None, :] * torch.log((O + 1.0) / (E + 1.0))).T[batch.long()]
    obj = (R * dist).sum() + SIGMA * torch.xlogy(R, R).sum() + SIGMA * (R * cross).sum()
    return R, float(obj)


def numpy_iteration(st):
    import harmony_reference as hr
    U, R, T = st.U.cpu().numpy(), st.R.cpu().numpy(), st.T.cpu().numpy()
    batch, Pr, theta = st.batch.cpu().numpy().astype(np.int64), st.Pr.cpu().numpy(), st.theta.cpu().numpy()
    t0 = time.perf_counter()
    Y = hr.unit(hr.weighted_group_reduce(U, R, None, 1)[0][:, 0])
    _, dist, e = hr.scores(U, Y, SIGMA)
    O, E = hr.sweep(R, T, e, batch, Pr, theta, N_BLOCKS)
    hr.objective(R, dist, batch, O, E, theta, SIGMA)
    return 1e3 * (time.perf_counter() - t0)


def write_md(rec, path):
    lines = ["# ops.harmony_rows: the kernels against a framework composition and the numpy restatement", "",
             f"Measured by `examples/resident_harmony_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, n_blocks = {N_BLOCKS}, theta = {THETA}, sigma = {SIGMA}; wall ms.", "",
             "| rows | batches | clusters | scores | block | iteration | framework iteration | iteration / framework | numpy iteration | "
             "whole call | rounds | iterations | max abs R difference to the framework |", "|" + "---|" * 13]
    for r in sorted(rec["rows"], key=lambda r: (r["batch"], r["segs"])):
        numpy_ms = "not run" if r["numpy_wall_ms"] is None else f"{r['numpy_wall_ms']:.0f}"
        lines.append(f"| {r['batch']} | {r['segs']} | {r['clusters']} | {r['scores_wall_ms']:.3f} | {r['block_wall_ms']:.3f} | "
                     f"{r['iteration_wall_ms']:.2f} | {r['framework_wall_ms']:.2f} | "
                     f"{r['iteration_wall_ms'] / r['framework_wall_ms']:.3f} | {numpy_ms} | {r['call_wall_ms']:.1f} | {r['rounds']} | "
                     f"{r['iterations']} | {r['iteration_vs_framework_R']:.2e} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    rec = dict(shape=dict(D=D, n_blocks=N_BLOCKS, theta=THETA, sigma=SIGMA, inner=args.inner, reps=args.reps),
               device=torch.cuda.get_device_name(0), rows=[])
    if args.out and Path(args.out).exists():
        rec["rows"] = [r for r in json.loads(Path(args.out).read_text())["rows"] if r["batch"] not in args.batches]
    for B in args.batches:
        K = ops.harmony_default_clusters(B)
        for S in SEGS:
            x, batch = cohort(B, S, K)
            st = State(x, batch, S, K)
            start = (st.R.clone(), st.T.clone(), st.Y.clone())
            st.iteration()
            mine = st.R.clone()
            theirs, _ = framework_iteration(st.U, start[0], batch, st.Pr, st.theta)
            fns = {"scores": (lambda: ops.harmony_scores(st.U, st.Y, SIGMA), 10), "block": (lambda: st.block(7), 10),
                   "iteration": (st.iteration, args.inner),
                   "framework": (lambda: framework_iteration(st.U, st.R, batch, st.Pr, st.theta), args.inner)}
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps)
            t0 = time.perf_counter()
            run = ops.harmony_rows(x, batch, S, n_clusters=K, theta=THETA, sigma=SIGMA, n_blocks=N_BLOCKS)
            torch.cuda.synchronize()
            call_ms = 1e3 * (time.perf_counter() - t0)
            row = dict(batch=B, segs=S, clusters=K, scores_wall_ms=ms["scores"], block_wall_ms=ms["block"],
                       iteration_wall_ms=ms["iteration"], framework_wall_ms=ms["framework"],
                       numpy_wall_ms=numpy_iteration(st) if B <= 2000 else None, call_wall_ms=call_ms, rounds=run.n_iter,
                       iterations=sum(run.inner_iters), converged=run.converged,
                       iteration_vs_framework_R=float((mine - theirs).abs().max()))
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
            if args.out:                                                                         # after every (batch, S)
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                write_md(rec, Path(args.out).with_suffix(".md"))
            del x, st, run
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
