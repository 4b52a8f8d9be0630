"""Timing of ops.lanczos_graph / ResidentPredictor.diffmap / dpt (profiles/resident_diffmap.md).

Shapes: B in {2 000, 20 000, 100 000} cells x D = 200, k = 15.  Rows: the seeded noisy arc of
examples/resident_pseudotime_timing.py, so that the kNN graph is one long component; the exact kNN lists come from ops.knn_rows
(not timed), the graph from ops.fuzzy_graph, the operator from ops.diffusion_operator, the mask is the largest component.  The
number of steps m is ops.lanczos_steps(B): 128 below 10 000 cells, 256 from there on.  Per shape, in one process, the routes
ALTERNATING inside every repetition:
  apply        - one wgnn_lanczos_apply launch on the last basis vector
  reorth       - one re-orthogonalisation pass against the FULL basis of m + 1 vectors: wgnn_lanczos_dots (two launches) and
                 wgnn_lanczos_update.  reorth_bytes = 2 (m + 1) B 8: the basis is read once by each; reorth_gbs = that over the
                 pass's wall time, reorth_of_peak against 8 TB/s
  step         - one whole step at the full basis: apply, two passes, the norm, the scale: ten launches
  operator     - ops.diffusion_operator
  lanczos      - ops.lanczos_graph end to end (all steps, every read-back)
  framework    - the same iteration composed of framework ops in float64: torch.sparse.mm for the product, torch.mv against the
                 basis for the coefficients and the update (twice), torch.linalg.vector_norm; its Ritz values are compared with
                 the device route's (framework_gap: the largest difference over the 15 leading ones)
  host         - scipy.sparse.linalg.eigsh(T, k = 16, which = "LA") on the host in float64 on the component's block (the copy to
                 the host is not in it); host_gap: the largest distance of a device eigenvalue to one of eigsh's
  diffmap, dpt - the whole ResidentPredictor calls on the synthetic batch of examples/resident_rank_genes_timing.py (root: the
                 first cell of the component)
  wall_ms: perf_counter around `inner` back-to-back calls until the device is idle, divided by `inner`; the median of `reps`
  after one warm-up round.
`max_residual`: the largest residual estimate over the 16 leading components at the default number of steps, on the arc and
(`diffmap_max_residual`) on the synthetic batch.

One batch size per process, each under its own time limit; rows are merged into --out by batch and the .md is rewritten:

    timeout -k 10 600 python examples/resident_diffmap_timing.py --out profiles/resident_diffmap.json --batches 2000
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

D, K_NN, N_COMPS = HIDDEN, 15, 16
PEAK_GBS = 8000.0


def write_md(rec, path):
    lines = ["# ResidentPredictor.diffmap / dpt: the Lanczos steps against framework ops and a host eigsh", "",
             f"Measured by `examples/resident_diffmap_timing.py` on {rec['device']}; its docstring defines every column.",
             f"D = {D}, k = {K_NN}, a noisy arc, {N_COMPS} components; wall ms per call.", "",
             "| cells | stored edges | steps | apply | reorth pass | reorth GB/s | of 8 TB/s | step | operator | lanczos_graph | "
             "framework ops | eigsh (host) | gap to framework | gap to eigsh | max residual | diffmap() | dpt() | "
             "diffmap() max residual |", "|" + "---|" * 18]
    for r in sorted(rec["rows"], key=lambda r: r["batch"]):
        lines.append(f"| {r['batch']} | {r['nnz']} | {r['steps']} | {r['apply_wall_ms']:.4f} | {r['reorth_wall_ms']:.4f} | "
                     f"{r['reorth_gbs']:.0f} | {r['reorth_of_peak']:.3f} | {r['step_wall_ms']:.3f} | {r['operator_wall_ms']:.3f} | "
                     f"{r['lanczos_wall_ms']:.1f} | {r['framework_wall_ms']:.1f} | {r['host_wall_ms']:.0f} | {r['framework_gap']:.1e} | "
                     f"{r['host_gap']:.1e} | {r['max_residual']:.1e} | {r['diffmap_wall_ms']:.1f} | {r['dpt_wall_ms']:.1f} | "
                     f"{r['diffmap_max_residual']:.1e} |")
    notes = Path(path).read_text() if Path(path).exists() else ""                # what was written under "## Notes" by hand stays
    notes = notes[notes.index("\n## Notes"):] if "\n## Notes" in notes else ""
    Path(path).write_text("\n".join(lines) + "\n" + notes)


def framework_lanczos(T, v0, v1, m):
    """The iteration with framework ops: ``(alpha, beta)`` on the host."""
    B = v0.shape[0]
    V = torch.zeros((m + 1, B), dtype=torch.float64, device=v0.device)
    V[0], V[1] = v0, v1
    alpha, beta = torch.zeros(m, dtype=torch.float64, device=v0.device), torch.zeros(m, dtype=torch.float64, device=v0.device)
    for j in range(1, m + 1):
        w = torch.sparse.mm(T, V[j][:, None])[:, 0]
        c = torch.mv(V[:j + 1], w)
        alpha[j - 1] = c[j]
        w = w - torch.mv(V[:j + 1].T, c)
        w = w - torch.mv(V[:j + 1].T, torch.mv(V[:j + 1], w))
        beta[j - 1] = torch.linalg.vector_norm(w)
        if j < m:
            V[j + 1] = w / beta[j - 1]
    return alpha, beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 20000, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
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
            s = torch.rand(B, device="cuda", generator=gen)
            rows = 0.15 * torch.randn((B, D), device="cuda", generator=gen)
            rows[:, 0] += 20 * torch.cos(3 * s)
            rows[:, 1] += 20 * torch.sin(3 * s)
            idx, d2 = ops.knn_rows(rows, K_NN)
            dev = rows.device
            fuzzy = ops.fuzzy_graph(idx, d2)
            rowptr, col, w = fuzzy.rowptr, fuzzy.col, fuzzy.w
            nnz = int(col.shape[0])
            stream = _stream(dev)
            lowest = ops.graph_components(rowptr, col)
            size = torch.bincount(lowest, minlength=B)
            mask = lowest == torch.nonzero(size == size.max())[0, 0]
            op = ops.diffusion_operator(rowptr, col, w)
            run = ops.lanczos_graph(rowptr, col, op.t, op.z, mask)
            m = run.n_run
            assert not run.breakdown
            theta, S, res = ops.lanczos_ritz(run.alpha, run.beta, m)
            V, rows_all = run.V, m + 1
            vec, c = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(rows_all, dtype=torch.float64, device=dev)
            nrm, v_out = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
            ws_bytes = int(_lib.lib().wgnn_lanczos_dots_workspace_bytes(B, rows_all))
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            words = torch.zeros(2, dtype=torch.int64, device=dev)
            halt, status = words.data_ptr(), words.data_ptr() + 8
            last = V.data_ptr() + 8 * B * m

            def apply():
                _lib.run(dev, "wgnn_lanczos_apply", _ptr(rowptr), _ptr(col), _ptr(op.t), B, nnz, last, _ptr(vec), halt, status, 0, 0,
                         stream)

            def reorth():
                _lib.run(dev, "wgnn_lanczos_dots", _ptr(V), B, rows_all, _ptr(vec), B, _ptr(c), None, halt, 1, _ptr(ws), ws_bytes, 0, 0,
                         stream)
                _lib.run(dev, "wgnn_lanczos_update", _ptr(V), B, rows_all, _ptr(c), _ptr(vec), B, halt, 0, 0, stream)

            def step():
                apply()
                reorth()
                reorth()
                _lib.run(dev, "wgnn_lanczos_dots", None, 0, 1, _ptr(vec), B, _ptr(nrm), None, None, 1, _ptr(ws), ws_bytes, 0,
                         _lib.LANCZOS_NORM, stream)
                _lib.run(dev, "wgnn_lanczos_scale", _ptr(vec), _ptr(nrm), _ptr(v_out), B, None, 0, 0, stream)

            row = torch.repeat_interleave(torch.arange(B, device=dev), rowptr[1:] - rowptr[:-1], output_size=nnz)
            T = torch.sparse_coo_tensor(torch.stack([row, col.long()]), op.t, (B, B)).coalesce().to_sparse_csr()
            fa, fb = framework_lanczos(T, V[0], V[1], m)
            ftheta = ops.lanczos_ritz(fa, fb, m)[0]
            framework_gap = float(np.abs(ftheta[:N_COMPS - 1] - theta[:N_COMPS - 1]).max())

            inner = args.inner
            root = int(torch.nonzero(mask)[0, 0])
            fns = {"apply": (apply, inner), "reorth": (reorth, inner), "step": (step, inner),
                   "operator": (lambda: ops.diffusion_operator(rowptr, col, w), 1),
                   "lanczos": (lambda: ops.lanczos_graph(rowptr, col, op.t, op.z, mask), 1),
                   "framework": (lambda: framework_lanczos(T, V[0], V[1], m), 1),
                   "diffmap": (lambda: rp.diffmap(batch, n_comps=N_COMPS, k=K_NN), 1),
                   "dpt": (lambda: rp.dpt(batch, 0, n_dcs=10, n_comps=N_COMPS, k=K_NN), 1)}
            table = rp.diffmap(batch, n_comps=N_COMPS, k=K_NN)
            if not table.in_component[0]:
                del fns["dpt"]
            timed_alternating(fns, 1)                                                            # warm-up
            ms = timed_alternating(fns, args.reps if B < 100000 else 3)
            ms.setdefault("dpt", float("nan"))
            assert words.tolist() == [0, 0]

            from scipy.sparse import csr_matrix
            from scipy.sparse.linalg import eigsh
            on = mask.cpu().numpy()
            Th = csr_matrix((op.t.cpu().numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(B, B))[on][:, on]
            t0 = time.perf_counter()
            lam = eigsh(Th, k=N_COMPS, which="LA")[0]
            host_ms = 1e3 * (time.perf_counter() - t0)
            mine = np.concatenate([[1.0], theta[:N_COMPS - 1]])
            host_gap = float(max(np.abs(lam - v).min() for v in mine))
            reorth_bytes = 2 * rows_all * B * 8
            rec_row = dict(batch=B, nnz=nnz, steps=m, cells_in_component=int(on.sum()), **{f"{name}_wall_ms": v for name, v in ms.items()},
                           reorth_bytes=reorth_bytes, reorth_gbs=reorth_bytes / (ms["reorth"] * 1e-3) / 1e9,
                           reorth_of_peak=reorth_bytes / (ms["reorth"] * 1e-3) / 1e9 / PEAK_GBS, host_wall_ms=host_ms,
                           framework_gap=framework_gap, host_gap=host_gap, max_residual=float(res[:N_COMPS - 1].max()),
                           diffmap_max_residual=float(table.residual.max()), diffmap_steps=int(table.n_steps),
                           diffmap_components=int(table.n_components), diffmap_in_component=int(table.in_component.sum()))
            print(json.dumps(rec_row), flush=True)
            rec["rows"].append(rec_row)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
                write_md(rec, Path(args.out).with_suffix(".md"))
            del batch, rows, V, run, T
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
