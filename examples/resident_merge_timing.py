"""Timing of ResidentPredictor.align over a gene list in which columns collide (a GeneMap, duplicates="sum") against the same
batch under a collision-free map and against merging the columns on the host first (profiles/resident_merge.md).

Shape and bundle as examples/resident_lognorm_timing.py: 30 000 caller columns, 20 000 of which name the bundle's G = 20 000
genes, 10 000 foreign ones; a cell holds raw counts on 800 bundle genes and about 400 foreign columns.  Here about 2 % of the
columns (600) are in groups of 2 - 3: foreign columns renamed, as an alias table would, to a bundle gene that already has a
column - so the batch is the SAME in all three timings, only the map differs.  Batches of B in {200, 2 000, 20 000}, as a
dense float32 device matrix and as a device CSR.  Per (form, B), in one process, the calls ALTERNATING inside every repetition:
  merge - align(batch, GeneMap, normalize="lognorm"): wgnn_align_count_ln_merge, cumsum, read-back, wgnn_align_fill_ln_merge
  plain - align(batch, the collision-free map, normalize="lognorm"): the existing kernels on the same batch - the yardstick
  host  - the member columns summed on the host (numpy for the dense form, a scipy product for the CSR), the upload, and
          align(merged batch, a map with one column per gene, normalize="lognorm", library sizes = the original totals)
  wall_ms: host clock around the call, ending in a device synchronise; median, minimum and maximum of `reps` (default 20)
  after a warm-up.
`kernel`: each of the four kernels alone between HIP events.

    python examples/resident_merge_timing.py --out profiles/resident_merge.json [--batches 200 2000]
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
from resident_predict_timing import G, HIDDEN, N_CLS, PER_CELL, write_bundle                  # noqa: E402
from resident_lognorm_timing import FOREIGN_PER_CELL, N_FOREIGN, SCALE, callers_counts, timed_alternating   # noqa: E402
import scdeepsort_amd as sda                                   # noqa: E402
from scdeepsort_amd import _lib, api                           # noqa: E402
from scdeepsort_amd.graph import _ptr, _stream                 # noqa: E402

N_GROUPS, SHARE_OF_THREE = 250, 0.4            # 250 groups, 100 of them of three: 600 member columns of 30 000


def colliding_ids(ids, seed):
    """``ids`` with foreign columns renamed to genes that already have a column: (ids with collisions, the tables)."""
    rng = np.random.default_rng(seed)
    ids = ids.copy()
    genes = rng.permutation(G)[:N_GROUPS]
    extra = np.where(np.arange(N_GROUPS) < SHARE_OF_THREE * N_GROUPS, 2, 1)
    foreign = rng.permutation(np.flatnonzero(ids < 0))[:extra.sum()]
    ids[foreign] = np.repeat(genes, extra)
    members = {}
    for j in np.flatnonzero(np.isin(ids, genes)):
        members.setdefault(int(ids[j]), []).append(int(j))
    col_group = np.full(len(ids), -1, np.int32)
    ptr, cols = [0], []
    for g in sorted(members):
        col_group[members[g]] = len(ptr) - 1
        cols += members[g]
        ptr.append(len(cols))
    return ids, (col_group, np.asarray(ptr, np.int32), np.asarray(cols, np.int32))


def kernel_ms(batch, gm, plain, thr, reps=10):
    """Device ms of one launch of each kernel (HIP events around `reps` launches)."""
    dev = plain.device
    dense = isinstance(batch, torch.Tensor)
    B = batch.shape[0] if dense else batch[0].shape[0] - 1
    x, ld, (rowptr, col, val) = (batch, batch.stride(0), (None, None, None)) if dense else (None, 0, batch)
    flags = 0 if dense or rowptr.dtype == torch.int32 else _lib.FLAG_ROWPTR_I64
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    total = torch.empty(B, dtype=torch.float64, device=dev)
    s = _stream(dev)
    ms = {}
    for tag, gmap, tables in (("merge", gm.ids, (_ptr(gm.col_group), _ptr(gm.group_ptr), _ptr(gm.group_cols), gm.n_groups,
                                                 gm.n_merged_columns)), ("plain", plain, ())):
        sfx = "_merge" if tables else ""
        head = (_ptr(x), ld, _ptr(rowptr), _ptr(col), _ptr(val), B, gmap.shape[0], _ptr(gmap), G, float(thr), *tables)
        assert _lib.call(dev, "wgnn_align_count_ln" + sfx, *head, None, _ptr(total), SCALE, _ptr(counts), _ptr(status), flags, s) == 0
        o_rowptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, dtype=torch.int64, out=o_rowptr[1:])
        o_col = torch.empty(int(o_rowptr[-1]), dtype=torch.int32, device=dev)
        o_raw = torch.empty(int(o_rowptr[-1]), dtype=torch.float32, device=dev)
        calls = {"count": lambda: _lib.call(dev, "wgnn_align_count_ln" + sfx, *head, None, _ptr(total), SCALE, _ptr(counts),
                                            _ptr(status), flags, s),
                 "fill": lambda: _lib.call(dev, "wgnn_align_fill_ln" + sfx, *head, _ptr(total), SCALE, _ptr(o_rowptr), _ptr(o_col),
                                           _ptr(o_raw), _ptr(status), flags, s)}
        for name, fn in calls.items():
            fn()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                assert fn() == 0
            e.record()
            torch.cuda.synchronize()
            ms[f"{tag}_{name}"] = a.elapsed_time(e) / reps
    assert int(status) == 0
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rec = dict(shape=dict(genes=G, foreign_columns=N_FOREIGN, kept_per_cell=PER_CELL, foreign_per_cell=FOREIGN_PER_CELL,
                          groups=N_GROUPS, hidden=HIDDEN, classes=N_CLS, layers=1), device=torch.cuda.get_device_name(0), rows=[])
    with tempfile.TemporaryDirectory() as td:
        write_bundle(Path(td), 1)
        rp = sda.ResidentPredictor("mouse", "Timing1", model_path=td)
        thr = float(rp.threshold)
        for B in args.batches:
            x_host, ids0 = callers_counts(B, 100 + B)
            ids, (col_group, group_ptr, group_cols) = colliding_ids(ids0, 7)
            n_cols = len(ids)
            plain = torch.from_numpy(ids0).cuda()
            gm = api.GeneMap(ids=torch.from_numpy(ids).cuda(), col_group=torch.from_numpy(col_group).cuda(),
                             group_ptr=torch.from_numpy(group_ptr).cuda(), group_cols=torch.from_numpy(group_cols).cuda(),
                             n_groups=len(group_ptr) - 1, n_merged_columns=len(group_cols))
            # the host route: every member column added into its group's first column
            first = np.arange(n_cols)
            first[group_cols] = np.repeat(group_cols[group_ptr[:-1]], np.diff(group_ptr))
            later = np.flatnonzero(first != np.arange(n_cols))
            ids_first = ids.copy()
            ids_first[later] = -1
            host_map = torch.from_numpy(ids_first).cuda()
            fold = sp.csr_matrix((np.ones(n_cols, np.float32), (np.arange(n_cols), first)), shape=(n_cols, n_cols))
            x_dev = torch.from_numpy(x_host).cuda()
            csr_host = sp.csr_matrix(x_host)
            csr_dev = (torch.from_numpy(csr_host.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr_host.indices).cuda(),
                       torch.from_numpy(csr_host.data).cuda())

            def host_dense():
                total = x_host.sum(axis=1, dtype=np.float64)
                merged = x_host.copy()
                np.add.at(merged, (slice(None), first[later]), x_host[:, later])
                merged[:, later] = 0
                return rp.align(torch.from_numpy(merged).cuda(), host_map, normalize=sda.LogNormalize(library_size=total))

            def host_csr():
                total = np.asarray(csr_host.sum(axis=1, dtype=np.float64)).ravel()
                merged = (csr_host @ fold).tocsr()
                merged.sort_indices()
                return rp.align((torch.from_numpy(merged.indptr.astype(np.int64)).cuda(), torch.from_numpy(merged.indices).cuda(),
                                 torch.from_numpy(merged.data.astype(np.float32)).cuda()), host_map,
                                normalize=sda.LogNormalize(library_size=total))

            for form, batch, host in (("dense", x_dev, host_dense), ("csr", csr_dev, host_csr)):
                out = rp.align(batch, gm, normalize="lognorm")
                base = rp.align(batch, plain, normalize="lognorm")
                other = host()                                   # the sum sits at the group's first column there: same entries
                assert torch.equal(other[0], out[0])             # per cell, possibly in another order
                assert torch.equal(other[2].sort().values, out[2].sort().values)
                fns = {"merge": lambda: rp.align(batch, gm, normalize="lognorm"),
                       "plain": lambda: rp.align(batch, plain, normalize="lognorm"), "host": host}
                timed_alternating(fns, 1)                        # warm-up
                ms = timed_alternating(fns, args.reps)
                k = kernel_ms(batch, gm, plain, thr)
                row = dict(form=form, batch=B, columns=n_cols, member_columns=int(len(group_cols)), stored=int(csr_host.nnz),
                           kept_merge=int(out[1].shape[0]), kept_plain=int(base[1].shape[0]),
                           **{f"{n}_wall_ms": v["median"] for n, v in ms.items()},
                           **{f"{n}_wall_ms_min_max": [v["min"], v["max"]] for n, v in ms.items()},
                           **{f"{n}_kernel_ms": v for n, v in k.items()},
                           merge_over_plain=ms["merge"]["median"] / ms["plain"]["median"],
                           merge_over_host=ms["merge"]["median"] / ms["host"]["median"])
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
                del out, base, other
            del x_dev, csr_dev
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
