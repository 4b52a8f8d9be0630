"""What ``ResidentPredictor``'s calls return: the result tables, their ``*Summary`` dicts and the host helpers they share with the
predictor - pandas / numpy logic over what a call left behind.  Nothing here imports ``api`` or ``ops``; ``api`` imports this
module and re-exports every name of it."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from ._lib import HOOD_MAX_MEMBERS

_rows_topk = None      # ops.rows_topk, the device route of MarkerTable.top: set by api.py, this module imports no ops


@dataclass
class Attribution:
    """What ``ResidentPredictor.explain`` returns for a batch of B cells.  ``label`` as ``classify`` gives it (-1 = unsure),
    ``target`` the class explained, ``logit`` its logit, ``base`` the bias share (numpy, [B]); ``scores`` the per-entry
    shares (device f32 [nnz], in the CSR order of the batch): ``sum(scores of a cell) + base == logit``.  ``top_genes``
    [B, k] gene ids by descending score (-1 where a cell expresses fewer than k genes), ``top_scores`` [B, k] (0 there)."""
    label: np.ndarray
    target: np.ndarray
    logit: np.ndarray
    base: np.ndarray
    scores: torch.Tensor
    top_genes: np.ndarray
    top_scores: np.ndarray
    id2gene: Sequence[str] = field(default=(), repr=False)

    def gene_names(self, i: int) -> List[str]:
        """The names of cell ``i``'s top genes, best first (shorter than k when the cell expresses fewer genes)."""
        return [self.id2gene[g] for g in self.top_genes[i] if g >= 0]


@dataclass
class MarkerTable:
    """What ``ResidentPredictor.markers`` returns: the attribution scores of a cohort summed per (group, gene).  K groups
    (``group_names``), G genes (``id2gene``).  ``n_cells`` int64 [K]: the cells of each group that took part; ``n_skipped``:
    cells with group -1 (unsure, or excluded by the caller); ``score_sum`` f64 [K, G] and ``expr_count`` int32 [K, G] (on the
    device): the summed scores of the group's cells that express the gene, and how many do; ``base_sum`` / ``logit_sum`` f64
    [K]: ``Attribution.base`` / ``.logit`` summed over the group's cells, so that for every group
    ``score_sum[k].sum() + base_sum[k] == logit_sum[k]`` up to rounding."""
    group_names: Sequence[str]
    id2gene: Sequence[str]
    n_cells: np.ndarray
    n_skipped: int
    score_sum: torch.Tensor
    expr_count: torch.Tensor
    base_sum: np.ndarray
    logit_sum: np.ndarray

    def _cells(self) -> torch.Tensor:
        return torch.from_numpy(np.asarray(self.n_cells, np.float64)).to(self.score_sum.device)[:, None]

    def mean_score(self) -> torch.Tensor:
        """f64 [K, G]: ``score_sum / n_cells`` - a cell that does not express the gene counts 0; 0 for an empty group."""
        n = self._cells()
        return torch.where(n > 0, self.score_sum / n.clamp(min=1.0), torch.zeros_like(self.score_sum))

    def fraction(self) -> torch.Tensor:
        """f64 [K, G]: the share of the group's cells that express the gene (0 for an empty group)."""
        n = self._cells()
        return torch.where(n > 0, self.expr_count.to(torch.float64) / n.clamp(min=1.0), torch.zeros_like(self.score_sum))

    def top(self, k: int = 20, min_fraction: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
        """Per group the ``k`` genes with the highest ``float32(mean_score)``, descending, equal scores by the lower gene
        id, among the genes with ``expr_count > 0`` and ``fraction >= min_fraction``: (genes int64 [K, k], -1 where a group
        has fewer; scores f32 [K, k], 0 there).  Device tables go through ``wgnn_rows_topk`` (``k <= 64``)."""
        k = int(k)
        K, G = self.score_sum.shape
        if k < 1:
            raise ValueError(f"top: k = {k} must be positive")
        key = self.mean_score().to(torch.float32)
        ok = (self.expr_count > 0) & (self.fraction() >= float(min_fraction))
        key = torch.where(ok, key, torch.full_like(key, -float("inf")))
        if key.is_cuda:
            if k > 64:
                raise ValueError(f"top: k = {k} > 64 is not built (wgnn_rows_topk)")
            dev = key.device
            rowptr = torch.arange(K + 1, dtype=torch.int64, device=dev) * G
            col = torch.arange(G, dtype=torch.int32, device=dev).repeat(K)
            genes, scores = _rows_topk(rowptr, col, key.reshape(-1).contiguous(), k)
        else:
            order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k]
            genes, scores = order, key.gather(1, order)
            if k > G:
                genes = F.pad(genes, (0, k - G), value=-1)
                scores = F.pad(scores, (0, k - G), value=-float("inf"))
        genes, scores = genes.cpu().numpy().astype(np.int64), scores.cpu().numpy().astype(np.float32)
        out = np.isneginf(scores) | (genes < 0)
        genes[out] = -1
        scores[out] = 0.0
        return genes, scores

    def frame(self, k: int = 20, min_fraction: float = 0.0) -> pd.DataFrame:
        """Long form, one row per (group, rank): ``group``, ``n_cells``, ``rank`` (1 = highest), ``gene``, ``mean_score``
        (f64), ``fraction``."""
        genes, _ = self.top(k, min_fraction)
        r, c = np.nonzero(genes >= 0)
        g = genes[r, c]
        at = (torch.from_numpy(r).to(self.score_sum.device), torch.from_numpy(g).to(self.score_sum.device))
        return pd.DataFrame({"group": [self.group_names[i] for i in r], "n_cells": np.asarray(self.n_cells)[r], "rank": c + 1,
                             "gene": [self.id2gene[j] for j in g], "mean_score": self.mean_score()[at].cpu().numpy(),
                             "fraction": self.fraction()[at].cpu().numpy()})

    def _require_same(self, group_names: Sequence[str], n_genes: int, id2gene: Optional[Sequence[str]] = None) -> None:
        """``into=``: the batch must be grouped and indexed as this table is."""
        K, G = self.score_sum.shape
        if len(group_names) != K:
            raise ValueError(f"into: the table holds {K} groups, the batch is grouped into {len(group_names)}")
        if int(n_genes) != G:
            raise ValueError(f"into: the table holds {G} genes, the bundle {int(n_genes)}")
        if list(group_names) != list(self.group_names):
            raise ValueError("into: the table's group names differ from the batch's")
        if id2gene is not None and list(id2gene) != list(self.id2gene):
            raise ValueError("into: the table's gene names differ from the bundle's")

    def _add_cells(self, group: np.ndarray, base: np.ndarray, logit: np.ndarray) -> None:
        """The [B] vectors of one batch into the per-group host sums (fp64)."""
        K = len(self.group_names)
        group = np.asarray(group, np.int64)
        on = group >= 0
        self.n_cells = np.asarray(self.n_cells, np.int64) + np.bincount(group[on], minlength=K).astype(np.int64)
        self.n_skipped = int(self.n_skipped) + int((~on).sum())
        self.base_sum = self.base_sum + np.bincount(group[on], weights=np.asarray(base, np.float64)[on], minlength=K)
        self.logit_sum = self.logit_sum + np.bincount(group[on], weights=np.asarray(logit, np.float64)[on], minlength=K)


def _cluster_ids(clusters, cluster_names=None, n_clusters=None, into: Optional["ClusterCalls"] = None,
                 n_cells: Optional[int] = None) -> Tuple[np.ndarray, List[str]]:
    """``annotate``'s ``clusters`` as ``(ids int64 [B], names)``.  A sequence of ``str`` is matched against ``into``'s names,
    else against ``cluster_names``, else factorised in sorted order; an unknown name raises ValueError.  Integer ids (-1 =
    the cell takes no part) need ``cluster_names``, ``n_clusters`` or ``into`` and are checked against ``[-1, K)``."""
    if cluster_names is not None:
        names = [str(n) for n in cluster_names]
        if n_clusters is not None and int(n_clusters) != len(names):
            raise ValueError(f"n_clusters = {n_clusters} but {len(names)} cluster names")
    elif n_clusters is not None:
        names = [str(i) for i in range(int(n_clusters))]
    else:
        names = None
    if into is not None:
        if names is not None and names != list(into.cluster_names):
            raise ValueError("into: the table's cluster names differ from the batch's")
        names = list(into.cluster_names)
    arr = clusters.detach().cpu().numpy() if isinstance(clusters, torch.Tensor) else np.asarray(clusters)
    if arr.ndim != 1:
        raise ValueError(f"clusters must hold one id or name per cell, got shape {arr.shape}")
    if n_cells is not None and arr.shape[0] != n_cells:
        raise ValueError(f"clusters lists {arr.shape[0]} cells, the batch holds {n_cells}")
    if arr.dtype.kind in "USO" and all(isinstance(c, str) for c in arr.tolist()):
        if names is None:
            names = sorted(set(arr.tolist()))
        lookup = {n: i for i, n in enumerate(names)}
        unknown = sorted(set(arr.tolist()) - set(lookup))
        if unknown:
            raise ValueError(f"cluster name {unknown[0]!r} is not one of the table's {len(names)} clusters")
        ids = np.fromiter((lookup[c] for c in arr.tolist()), dtype=np.int64, count=arr.shape[0])
    elif np.issubdtype(arr.dtype, np.integer):
        if names is None:
            raise ValueError("clusters given as integer ids need cluster_names or n_clusters")
        ids = arr.astype(np.int64)
        if ids.size and (ids.min() < -1 or ids.max() >= len(names)):
            raise ValueError(f"cluster id out of range [-1, {len(names)})")
    else:
        raise ValueError(f"clusters must be integer ids or str names, got {arr.dtype}")
    if not names:
        raise ValueError("no clusters")
    return ids, names


def _call_names(ids, id2label: Sequence[str], label_map=None) -> Tuple[list, list]:
    """(cell_type, cell_subtype) of cluster calls as ``_prediction_frame`` names per-cell ones: the label map's new type and
    subtype names when there is one, ``unsure`` for -1, ``empty`` for -2, ``None`` for anything below (no call)."""
    old2new, old2sub = label_map if label_map is not None else ({}, {})
    names = [id2label[p] if p >= 0 else {-1: "unsure", -2: "empty"}.get(int(p)) for p in ids]
    return [old2new.get(p, p) for p in names], [old2sub.get(p, p) for p in names]


class _NamesCalls:
    """For a result table with ``id2label`` and ``label_map``: label ids as the type names ``predict`` gives them."""

    def _name(self, ids) -> list:
        return _call_names(np.asarray(ids, np.int64), self.id2label, self.label_map)[0]


def _require_same_draws(table, n_cells: int, id2label: Sequence[str], seed: int) -> None:
    """``into=`` of ``Stability`` / ``Doublets`` / ``Ambient``, after the table's own checks: the same batch shape, cell types, seed."""
    if n_cells != len(table.label):
        raise ValueError(f"into: the table holds {len(table.label)} cells, the batch {n_cells}")
    if list(id2label) != list(table.id2label):
        raise ValueError("into: the table's cell types differ from the bundle's")
    if int(seed) != int(table.seed):
        raise ValueError(f"into: the table was drawn with seed {table.seed}, this call passes {seed}")


def _check_index(index, B: int) -> None:
    """``index=`` of a call on a batch of ``B`` cells: one name per cell, when given."""
    if index is not None and len(index) != B:
        raise ValueError(f"index names {len(index)} cells, the batch holds {B}")


@dataclass
class ClusterCalls:
    """What ``ResidentPredictor.annotate`` returns: one row per cluster of a cohort.  K clusters (``cluster_names``), C cell
    types (``id2label``).  The four tables of ``wgnn_group_class_reduce``, on the device they were made on (tables built
    from CPU tensors serve the host logic just as well): ``prob_sum`` f64 [K, C] the cells' softmax probabilities summed
    (fp64 from the f32 logits), ``conf_sum`` f64 [K] their largest probability summed, ``votes`` int32 [K, C] the cells per
    predicted type, ``tally`` int32 [K, 3] = (cells that took part, of them unsure, bad cells: logits with a NaN or +inf or
    all -inf, counted nowhere else).  ``unsure_rate``: the predictor's, for the ``"mean_prob"`` rule.  ``label_map``:
    ``load_label_map``'s two dicts when the bundle has one."""
    cluster_names: Sequence[str]
    id2label: Sequence[str]
    prob_sum: torch.Tensor
    conf_sum: torch.Tensor
    votes: torch.Tensor
    tally: torch.Tensor
    unsure_rate: float = 2.0
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    RULES = ("vote", "mean_prob")

    @property
    def n_cells(self) -> np.ndarray:
        """int64 [K]: the cells of each cluster that took part (bad cells are not among them)."""
        return self.tally[:, 0].cpu().numpy().astype(np.int64)

    @property
    def n_unsure(self) -> np.ndarray:
        return self.tally[:, 1].cpu().numpy().astype(np.int64)

    @property
    def n_bad(self) -> np.ndarray:
        return self.tally[:, 2].cpu().numpy().astype(np.int64)

    def _cells(self) -> torch.Tensor:
        return self.tally[:, :1].to(torch.float64)

    def fraction(self) -> torch.Tensor:
        """f64 [K, C]: ``votes / n_cells``, the share of a cluster's cells called each type (NaN for an empty cluster)."""
        return self.votes.to(torch.float64) / self._cells()

    def mean_prob(self) -> torch.Tensor:
        """f64 [K, C]: ``prob_sum / n_cells``, the cluster's mean softmax distribution (NaN for an empty cluster)."""
        return self.prob_sum / self._cells()

    def _ranked(self, rule: str) -> Tuple[np.ndarray, np.ndarray]:
        """The rule's score table as f64 [K, C] on the host (vote share | mean probability) and the classes of every cluster by
        descending score, equal scores by the lower id (int64 [K, C])."""
        if rule not in self.RULES:
            raise ValueError(f"rule = {rule!r}: pass one of {', '.join(map(repr, self.RULES))}")
        score = (self.fraction() if rule == "vote" else self.mean_prob()).cpu().numpy()
        key = (self.votes if rule == "vote" else self.prob_sum).cpu().numpy()
        return score, np.argsort(-key.astype(np.float64), axis=1, kind="stable")

    def consensus(self, rule: str = "vote", min_fraction: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
        """One call per cluster: ``(ids int64 [K], confidence f64 [K])``.  ``"vote"``: the type most of the cluster's cells were
        called (equal counts: the lower id), confidence = its share of ``n_cells``; -1 (unsure) when strictly more cells are
        unsure than voted for it, or when the share is ``< min_fraction``.  ``"mean_prob"``: the arg max of the cluster's mean
        distribution, confidence = that mean probability; -1 when it is ``< float32(unsure_rate / C)`` - the per-cell rule
        (reference ``predict.py:83``) applied to the mean.  A cluster without cells: -2 and NaN."""
        score, ranked = self._ranked(rule)
        K, C = score.shape
        n, win = self.n_cells, ranked[:, 0]
        conf = score[np.arange(K), win]
        ids = win.astype(np.int64)
        if rule == "vote":
            top = self.votes.cpu().numpy().astype(np.int64)[np.arange(K), win]
            ids[(self.n_unsure > top) | (conf < float(min_fraction))] = -1
        else:
            ids[conf < float(np.float32(self.unsure_rate / C))] = -1
        ids[n == 0] = -2
        return ids, np.where(n == 0, np.nan, conf)

    def frame(self, rule: str = "vote", min_fraction: float = 0.0) -> pd.DataFrame:
        """One row per cluster: ``cluster``, ``n_cells``, ``n_unsure``, ``n_bad``, the call as ``cell_type`` /
        ``cell_subtype`` (named as ``predict`` names cells; ``unsure`` / ``empty`` spelled out; without a label map both hold
        the bundle's name), then of the LEADING type - the rule's winner, also where the call came out unsure - ``fraction``
        (its vote share), ``mean_prob`` and the cluster's ``mean_confidence`` (``conf_sum / n_cells``), and the runner-up
        under the rule as ``second_type`` with its score (vote share | mean probability) as ``second_fraction`` (``None`` /
        NaN when no other type scored)."""
        ids, _ = self.consensus(rule, min_fraction)
        score, ranked = self._ranked(rule)
        K, C = score.shape
        n, rows, win = self.n_cells, np.arange(K), ranked[:, 0]
        types, subtypes = _call_names(ids, self.id2label, self.label_map)
        second = ranked[:, 1] if C > 1 else np.zeros(K, np.int64)
        second_score = score[rows, second] if C > 1 else np.full(K, np.nan)
        has = (n > 0) & (second_score > 0) if C > 1 else np.zeros(K, bool)
        second_names, _ = _call_names(np.where(has, second, -3), self.id2label, self.label_map)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_conf = self.conf_sum.cpu().numpy() / n
        return pd.DataFrame({"cluster": list(self.cluster_names), "n_cells": n, "n_unsure": self.n_unsure, "n_bad": self.n_bad,
                             "cell_type": types, "cell_subtype": subtypes,
                             "fraction": self.fraction().cpu().numpy()[rows, win], "mean_prob": self.mean_prob().cpu().numpy()[rows, win],
                             "mean_confidence": mean_conf, "second_type": second_names,
                             "second_fraction": np.where(has, second_score, np.nan)})

    def cell_labels(self, clusters, rule: str = "vote", min_fraction: float = 0.0) -> np.ndarray:
        """The clusters' calls broadcast back to the cells: int64 [B] for ``clusters`` as ``annotate`` takes them (ids, or
        names of this table); a cell of cluster -1 gets -1."""
        ids, _ = _cluster_ids(clusters, into=self)
        calls, _ = self.consensus(rule, min_fraction)
        return np.where(ids >= 0, calls[np.maximum(ids, 0)], -1).astype(np.int64)

    def _require_same(self, cluster_names: Sequence[str], id2label: Sequence[str]) -> None:
        """``into=``: the batch must be clustered and classified as this table is."""
        K, C = self.prob_sum.shape
        if len(cluster_names) != K:
            raise ValueError(f"into: the table holds {K} clusters, the batch is clustered into {len(cluster_names)}")
        if list(cluster_names) != list(self.cluster_names):
            raise ValueError("into: the table's cluster names differ from the batch's")
        if len(id2label) != C or list(id2label) != list(self.id2label):
            raise ValueError("into: the table's cell types differ from the bundle's")


class CoverageSummary(dict):
    """``Coverage.summary()``: a dict that prints as two or three lines."""

    def __str__(self) -> str:
        d = self
        lines = [f"{d['n_matched']} of {d['n_columns']} columns are genes of the bundle; {d['n_bundle_absent']} of its "
                 f"{d['n_bundle_genes']} genes are absent from the list",
                 f"{d['n_cells']} cells: fraction of counts seen median {d['median_fraction_counts']:.3f}, min "
                 f"{d['min_fraction_counts']:.3f}; fraction of expressed genes seen median {d['median_fraction_genes']:.3f}, "
                 f"min {d['min_fraction_genes']:.3f}; {d['n_cells_below']} cells below {d['min_counts']:g} of their counts"]
        if d["n_bad"]:
            lines.append(f"{d['n_bad']} values are negative, NaN or infinite (left out of everything above)")
        return "\n".join(lines)


@dataclass
class Coverage:
    """``ResidentPredictor.coverage``'s report.  An entry COUNTS iff its value is finite and ``> 0``; a column is MATCHED iff
    its name is a gene of the bundle.  Per cell (numpy ``[B]``): ``n_expressed`` / ``total`` = the counting entries over ALL
    of the caller's columns and their fp64 sum (the library size ``align(..., normalize="lognorm")`` divides by),
    ``n_mapped`` / ``total_mapped`` = the same over the matched columns - what the model sees - and ``n_bad`` = the values
    that are negative, NaN or infinite (in none of the others).  ``col_cells`` (int32 ``[n_columns]``, on the device): the
    cells in which each column counts.  ``columns``: the caller's names (``None`` when a gene map was passed)."""
    n_columns: int
    n_matched: int
    n_bundle_genes: int
    n_bundle_absent: int
    n_expressed: np.ndarray
    n_mapped: np.ndarray
    n_bad: np.ndarray
    total: np.ndarray
    total_mapped: np.ndarray
    col_cells: torch.Tensor
    index: Sequence
    columns: Optional[List[str]] = None
    matched: Optional[np.ndarray] = None             # bool [n_columns]
    absent_ids: Optional[np.ndarray] = None          # bundle gene ids no column names, ascending
    absent_support_cells: Optional[np.ndarray] = None  # support cells that express each of them
    absent_names: Optional[List[str]] = None
    n_support_cells: int = 0
    n_merged_columns: int = 0                        # matched columns that share their gene with another (a GeneMap's groups)

    def fraction_counts(self) -> np.ndarray:
        """``total_mapped / total`` per cell: the share of the cell's counts on genes the model knows; 0 where ``total == 0``."""
        t = np.asarray(self.total, np.float64)
        return np.divide(np.asarray(self.total_mapped, np.float64), t, out=np.zeros_like(t), where=t > 0)

    def fraction_genes(self) -> np.ndarray:
        """``n_mapped / n_expressed`` per cell; 0 where ``n_expressed == 0``."""
        n = np.asarray(self.n_expressed, np.float64)
        return np.divide(np.asarray(self.n_mapped, np.float64), n, out=np.zeros_like(n), where=n > 0)

    def frame(self) -> pd.DataFrame:
        """One row per cell: the per-cell columns and the two fractions."""
        return pd.DataFrame({"n_expressed": self.n_expressed, "n_mapped": self.n_mapped, "n_bad": self.n_bad,
                             "total": self.total, "total_mapped": self.total_mapped,
                             "fraction_counts": self.fraction_counts(), "fraction_genes": self.fraction_genes()},
                            index=self.index)

    def unmatched(self, k: int = 20) -> pd.DataFrame:
        """The caller's columns outside the bundle, by the cells in which they count (descending, ties by lower position):
        ``position``, ``gene`` (when the names are known), ``cells``, ``fraction_of_cells``."""
        cells = self.col_cells.cpu().numpy().astype(np.int64)
        pos = np.flatnonzero(~np.asarray(self.matched, bool))
        pos = pos[np.argsort(-cells[pos], kind="stable")][:k]
        B = len(self.n_expressed)
        out = {"position": pos}
        if self.columns is not None:
            out["gene"] = [self.columns[i] for i in pos]
        out["cells"] = cells[pos]
        out["fraction_of_cells"] = cells[pos] / B if B else np.zeros(len(pos))
        return pd.DataFrame(out)

    def absent(self, k: int = 20) -> pd.DataFrame:
        """The bundle's genes the caller's list lacks, by the support cells that express them (descending, ties by lower gene
        id) - which missing genes the model leaned on in training: ``gene_id``, ``gene``, ``support_cells``,
        ``fraction_of_support``."""
        ids = np.asarray(self.absent_ids, np.int64)
        n = np.asarray(self.absent_support_cells, np.int64)
        order = np.argsort(-n, kind="stable")[:k]
        out = {"gene_id": ids[order]}
        if self.absent_names is not None:
            out["gene"] = [self.absent_names[i] for i in order]
        out["support_cells"] = n[order]
        out["fraction_of_support"] = n[order] / self.n_support_cells if self.n_support_cells else np.zeros(len(order))
        return pd.DataFrame(out)

    def below(self, min_counts: float = 0.5, min_genes: int = 0) -> np.ndarray:
        """Boolean ``[B]``: cells whose ``fraction_counts`` is below ``min_counts`` or whose ``n_mapped`` is below ``min_genes``."""
        return (self.fraction_counts() < min_counts) | (np.asarray(self.n_mapped) < min_genes)

    def summary(self, min_counts: float = 0.5, min_genes: int = 0) -> CoverageSummary:
        """Matched and absent counts, the median and minimum of both fractions, the cells ``below`` the given bounds and the
        number of bad values; ``print`` it."""
        fc, fg = self.fraction_counts(), self.fraction_genes()
        stat = lambda a, f: float(f(a)) if a.size else 0.0
        return CoverageSummary(
            n_columns=self.n_columns, n_matched=self.n_matched, n_bundle_genes=self.n_bundle_genes,
            n_bundle_absent=self.n_bundle_absent, n_cells=int(fc.size),
            median_fraction_counts=stat(fc, np.median), min_fraction_counts=stat(fc, np.min),
            median_fraction_genes=stat(fg, np.median), min_fraction_genes=stat(fg, np.min),
            min_counts=float(min_counts), min_genes=int(min_genes),
            n_cells_below=int(self.below(min_counts, min_genes).sum()), n_bad=int(np.asarray(self.n_bad, np.int64).sum()))


def _keep_levels(keep) -> Tuple[float, ...]:
    """``stability``'s ``keep`` as a tuple of floats in [0, 1] (a single number is one level); ValueError otherwise."""
    levels = (keep,) if isinstance(keep, (int, float, np.integer, np.floating)) else tuple(keep)
    if not levels:
        raise ValueError("keep: no levels")
    out = []
    for k in levels:
        k = float(k)
        if not 0.0 <= k <= 1.0:                               # NaN fails both comparisons
            raise ValueError(f"keep = {k!r}: every level must be in [0, 1]")
        out.append(k)
    return tuple(out)


class StabilitySummary(dict):
    """``Stability.summary()``: a dict that prints as one line per level and one about the fragile cells."""

    def __str__(self) -> str:
        d = self
        lines = [f"{d['n_cells']} cells, {d['n_draws']} draws per level" + (f", thinned by {d['thin']}" if "thin" in d else "")]
        for k, med, p5 in zip(d["keep"], d["median_agreement"], d["p5_agreement"]):
            lines.append(f"keep {k:g}: agreement median {med:.3f}, 5th percentile {p5:.3f}")
        lines.append(f"{d['n_fragile']} cells below {d['min_agreement']:g} agreement at keep {d['at']:g}: median n_genes "
                     f"{d['median_n_genes_fragile']:g} against {d['median_n_genes_rest']:g} for the rest")
        return "\n".join(lines)


@dataclass
class Stability(_NamesCalls):
    """What ``ResidentPredictor.stability`` returns: per cell, how its call fares when only a share ``keep`` of its detected
    genes is left.  B cells (``index``), C cell types (``id2label``), L levels (``keep``), ``n_draws`` draws per level.
    ``label`` int64 [B] / ``max_prob`` f32 [B]: the call on the cell as given (``classify``'s, -1 = unsure); ``n_entries``
    int64 [B]: its stored genes.  The tallies of ``wgnn_predict_rows_dropout``, on the device they were made on (tables built
    from CPU tensors serve the host logic just as well): ``votes`` int32 [L, B, C] the draws per label, ``unsure`` int32
    [L, B] the draws labelled -1, ``empty`` int32 [L, B] the draws that kept no gene at all (also counted under the label
    they got), ``conf_sum`` f64 [L, B] the draws' largest softmax probability summed.  ``seed``: the masks' seed.
    ``thin``: what a draw drops - ``"genes"`` (whole genes of the values as given, ``wgnn_predict_rows_dropout``) or ``"reads"``
    (single reads of the raw counts, ``wgnn_predict_rows_thin``; ``keep`` is then a share of the DEPTH, ``empty`` counts the
    draws in which no gene took part, and ``n_reads`` int64 [B] holds a cell's library size, else ``None``)."""
    keep: Tuple[float, ...]
    n_draws: int
    label: np.ndarray
    max_prob: np.ndarray
    votes: torch.Tensor
    unsure: torch.Tensor
    empty: torch.Tensor
    conf_sum: torch.Tensor
    n_entries: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    seed: int = 0
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)
    thin: str = "genes"
    n_reads: Optional[np.ndarray] = None

    def _host(self) -> Tuple[np.ndarray, np.ndarray]:
        return self.votes.cpu().numpy().astype(np.int64), self.unsure.cpu().numpy().astype(np.int64)

    def agreement(self) -> np.ndarray:
        """f64 [L, B]: the share of a cell's draws whose label equals the full call - for a cell that is unsure as given, the
        share of draws that are unsure too."""
        votes, unsure = self._host()
        lab = np.asarray(self.label, np.int64)
        L, B, _ = votes.shape
        same = np.where(lab[None, :] >= 0, votes[:, np.arange(B), np.maximum(lab, 0)], unsure) if B else np.zeros((L, 0))
        return same.astype(np.float64) / self.n_draws

    def mean_prob(self) -> np.ndarray:
        """f64 [L, B]: the draws' mean largest softmax probability (whatever label it belongs to)."""
        return self.conf_sum.cpu().numpy().astype(np.float64) / self.n_draws

    def flips_to(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(ids int64 [L, B], share f64 [L, B])``: per level the cell type OTHER than the full call that most draws were
        labelled (equal counts: the lower id) and its share of the draws; -1 and 0 when no draw went to another type (draws
        that came out unsure are in ``unsure``, not here)."""
        votes, _ = self._host()
        L, B, C = votes.shape
        lab = np.asarray(self.label, np.int64)
        other = votes.copy()
        if B:
            other[:, np.arange(B), np.maximum(lab, 0)] = np.where(lab >= 0, -1, other[:, np.arange(B), np.maximum(lab, 0)])
        ids = other.argmax(axis=2) if C else np.zeros((L, B), np.int64)
        top = np.take_along_axis(other, ids[:, :, None], axis=2)[:, :, 0] if C else np.zeros((L, B), np.int64)
        none = top <= 0
        return np.where(none, -1, ids).astype(np.int64), np.where(none, 0.0, top / self.n_draws)

    def _level(self, at: float) -> int:
        return int(np.argmin(np.abs(np.asarray(self.keep, np.float64) - float(at))))

    def fragile(self, at: float = 0.5, min_agreement: float = 0.9) -> np.ndarray:
        """Boolean [B]: cells whose agreement at the level nearest ``at`` (the first of equally near ones) is below
        ``min_agreement``."""
        return self.agreement()[self._level(at)] < float(min_agreement)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` (named as ``predict`` names it), ``prob`` (the full call's), ``n_genes``
        (and ``n_reads`` under ``thin="reads"``), then per level ``agree_{keep}``, ``flip_{keep}`` (``flips_to``'s type by name, ``None`` without one) and
        ``flip_share_{keep}``."""
        out = {"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob), "n_genes": np.asarray(self.n_entries)}
        if self.n_reads is not None:
            out["n_reads"] = np.asarray(self.n_reads)
        agree = self.agreement()
        ids, share = self.flips_to()
        for l, k in enumerate(self.keep):
            out[f"agree_{k:g}"] = agree[l]
            out[f"flip_{k:g}"] = self._name(np.where(ids[l] >= 0, ids[l], -3))
            out[f"flip_share_{k:g}"] = share[l]
        return pd.DataFrame(out)

    def summary(self, at: float = 0.5, min_agreement: float = 0.9) -> StabilitySummary:
        """Per level the median and the 5th percentile of the agreement, the number of ``fragile(at, min_agreement)`` cells
        and the median ``n_genes`` of the fragile cells against the rest (NaN for an empty side); ``print`` it."""
        agree = self.agreement()
        frag = self.fragile(at, min_agreement)
        n = np.asarray(self.n_entries, np.float64)
        med = lambda a: float(np.median(a)) if a.size else float("nan")
        return StabilitySummary(
            n_cells=int(agree.shape[1]), n_draws=int(self.n_draws), keep=tuple(self.keep), thin=self.thin,
            median_agreement=[med(a) for a in agree], p5_agreement=[float(np.percentile(a, 5)) if a.size else float("nan") for a in agree],
            at=float(self.keep[self._level(at)]), min_agreement=float(min_agreement), n_fragile=int(frag.sum()),
            median_n_genes_fragile=med(n[frag]), median_n_genes_rest=med(n[~frag]))

    def by_cluster(self, clusters) -> pd.DataFrame:
        """Mean agreement per cluster and level: ``clusters`` holds one name or id per cell; one row per distinct value (sorted)
        with ``cluster``, ``n_cells`` and ``agree_{keep}`` per level.  Host code over the per-cell table."""
        arr = clusters.detach().cpu().numpy() if isinstance(clusters, torch.Tensor) else np.asarray(clusters)
        agree = self.agreement()
        if arr.ndim != 1 or arr.shape[0] != agree.shape[1]:
            raise ValueError(f"clusters must hold one id or name per cell ({agree.shape[1]}), got shape {arr.shape}")
        names, inv = np.unique(arr, return_inverse=True)
        n = np.bincount(inv, minlength=len(names))
        out = {"cluster": names.tolist(), "n_cells": n}
        for l, k in enumerate(self.keep):
            out[f"agree_{k:g}"] = np.bincount(inv, weights=agree[l], minlength=len(names)) / np.maximum(n, 1)
        return pd.DataFrame(out)

    def _require_same(self, keep: Sequence[float], n_cells: int, id2label: Sequence[str], seed: int, thin: str = "genes") -> None:
        """``into=``: the further draws must be of the same batch shape, levels, cell types, seed and kind of thinning."""
        if thin != self.thin:
            raise ValueError(f"into: the table was drawn with thin={self.thin!r}, this call passes thin={thin!r}")
        if tuple(keep) != tuple(self.keep):
            raise ValueError(f"into: the table holds the levels {tuple(self.keep)}, this call asks for {tuple(keep)}")
        _require_same_draws(self, n_cells, id2label, seed)


class DoubletsSummary(dict):
    """``Doublets.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells x {d['n_partners']} partners drawn across {d['across']}: {d['n_heterotypic']} heterotypic pairs",
            f"called as a parent {d['parent_share']:.3f}, as a third type {d['third_share']:.3f}, unsure (caught) {d['caught']:.3f}",
            f"largest sink: {d['top_sink']} takes {d['top_sink_pairs']} pairs neither of whose parents it is"])


@dataclass
class Doublets(_NamesCalls):
    """What ``ResidentPredictor.doublets`` returns: what the model calls synthetic doublets of a batch.  B cells (``index``), C
    cell types (``id2label``), D = ``n_partners`` draws per cell.  ``label`` int64 [B] / ``max_prob`` f32 [B]: the call on the
    real cell (``classify``'s, -1 = unsure).  Per (cell, draw), numpy arrays [B, D]: ``partner`` int32 = the second cell of the
    pair, ``draw_label`` int32 / ``draw_prob`` f32 = the call on the summed counts of the two.  ``seed`` / ``across``: how the
    partners were drawn.

    In the methods a pair's PARENTS are the real calls of its two cells.  A pair is HETEROTYPIC when both parents are called
    (not unsure) and differ; the other pairs are in ``pair_table`` and in nothing else.  This table characterises the MODEL on
    doublets; it does not say which real cells are doublets."""
    label: np.ndarray
    max_prob: np.ndarray
    partner: np.ndarray
    draw_label: np.ndarray
    draw_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    seed: int = 0
    across: str = "types"
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    @property
    def n_partners(self) -> int:
        return int(self.partner.shape[1])

    def _parents(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(type of the cell, type of the partner, heterotypic) as [B, D] arrays."""
        lab = np.asarray(self.label, np.int64)
        own = np.broadcast_to(lab[:, None], self.partner.shape)
        other = lab[self.partner.astype(np.int64)] if self.partner.size else own
        return own, other, (own >= 0) & (other >= 0) & (own != other)

    def pair_table(self) -> np.ndarray:
        """int64 [C + 1, C + 1, C + 1]: the pairs by (type of the cell, type of the partner, call of the pair), unsure as the
        last slot of every axis."""
        C = len(self.id2label)
        own, other, _ = self._parents()
        slot = lambda x: np.where(x >= 0, x, C).astype(np.int64).ravel()
        flat = (slot(own) * (C + 1) + slot(other)) * (C + 1) + slot(np.asarray(self.draw_label, np.int64))
        return np.bincount(flat, minlength=(C + 1) ** 3).reshape(C + 1, C + 1, C + 1)

    def frame(self) -> pd.DataFrame:
        """One row per unordered heterotypic type pair that was drawn: ``type_a`` / ``type_b`` (the lower id first, named as
        ``predict`` names a call), ``n`` pairs, ``parent_share`` (called as either parent), ``third_share`` (called a third
        type), ``unsure_share``, ``top_third`` (the most frequent third type, the lower id among equals, ``None`` without one)
        and ``mean_prob`` (the pairs' mean largest softmax probability)."""
        C = len(self.id2label)
        t = self.pair_table()[:C, :C]
        t = t + t.transpose(1, 0, 2)                                  # unordered: (S, T) and (T, S) together
        own, other, het = self._parents()
        lo, hi = np.minimum(own, other)[het], np.maximum(own, other)[het]
        prob = np.bincount(lo * C + hi, weights=np.asarray(self.draw_prob, np.float64)[het], minlength=C * C).reshape(C, C)
        rows = []
        for s in range(C):
            for u in range(s + 1, C):
                n = int(t[s, u].sum())
                if n == 0:
                    continue
                third = t[s, u, :C].copy()
                third[[s, u]] = 0
                top = int(third.argmax())
                rows.append((s, u, n, (t[s, u, s] + t[s, u, u]) / n, third.sum() / n, t[s, u, C] / n,
                             top if third[top] > 0 else -3, prob[s, u] / n))
        cols = list(zip(*rows)) if rows else [[] for _ in range(8)]
        return pd.DataFrame({"type_a": self._name(cols[0]), "type_b": self._name(cols[1]), "n": np.asarray(cols[2], np.int64),
                             "parent_share": np.asarray(cols[3], np.float64), "third_share": np.asarray(cols[4], np.float64),
                             "unsure_share": np.asarray(cols[5], np.float64), "top_third": self._name(cols[6]),
                             "mean_prob": np.asarray(cols[7], np.float64)})

    def _het_calls(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The heterotypic pairs' (type of the cell, type of the partner, call) as flat arrays."""
        own, other, het = self._parents()
        return own[het], other[het], np.asarray(self.draw_label, np.int64)[het]

    def caught(self) -> float:
        """The share of the heterotypic pairs that the unsure rule flags (NaN without such a pair)."""
        _, _, call = self._het_calls()
        return float((call < 0).mean()) if call.size else float("nan")

    def sinks(self) -> np.ndarray:
        """f64 [C]: per type T, of the heterotypic pairs CALLED T, the share neither of whose parents is T (NaN for a type no
        such pair was called).  A type with a high share and many pairs takes in doublets of other types."""
        C = len(self.id2label)
        own, other, call = self._het_calls()
        called = np.bincount(call[call >= 0], minlength=C).astype(np.float64)
        foreign = np.bincount(call[(call >= 0) & (call != own) & (call != other)], minlength=C)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(called > 0, foreign / called, np.nan)

    def artifact_risk(self, rate: float = 0.05) -> np.ndarray:
        """f64 [C]: per type T, the share of the cells called T that would be doublets of two OTHER types if a fraction ``rate``
        of the barcodes were heterotypic doublets: ``rate * q / (rate * q + (1 - rate) * r)`` with ``q`` = the share of the
        heterotypic pairs that are called T while T is neither parent and ``r`` = the share of the real cells called T (NaN where
        both are 0).  An approximation: the doublets' composition is the partner rule's (``across``), not the sample's;
        homotypic doublets and doublets called as a parent count as harmless; and ``r`` is taken from this batch, which holds
        its own doublets."""
        rate = float(rate)
        if not 0.0 <= rate <= 1.0:
            raise ValueError(f"rate = {rate!r} must be in [0, 1]")
        C = len(self.id2label)
        own, other, call = self._het_calls()
        q = np.bincount(call[(call >= 0) & (call != own) & (call != other)], minlength=C) / max(call.size, 1)
        lab = np.asarray(self.label, np.int64)
        r = np.bincount(lab[lab >= 0], minlength=C) / max(lab.size, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(rate * q + (1 - rate) * r > 0, rate * q / (rate * q + (1 - rate) * r), np.nan)

    def dominance(self) -> np.ndarray:
        """f64 [B]: per cell, the share of its heterotypic draws that keep the cell's own call (NaN for a cell without one -
        an unsure cell has none)."""
        own, _, het = self._parents()
        same = (het & (np.asarray(self.draw_label, np.int64) == own)).sum(axis=1)
        n = het.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, same / n, np.nan)

    def summary(self) -> DoubletsSummary:
        """The heterotypic pairs at a glance - their number, the shares called as a parent, as a third type and unsure
        (``caught``) - and the type that takes in most pairs it is no parent of; ``print`` it."""
        C = len(self.id2label)
        own, other, call = self._het_calls()
        n = int(call.size)
        parent = (call == own) | (call == other)
        foreign = np.bincount(call[(call >= 0) & ~parent], minlength=C)
        top = int(foreign.argmax()) if C and foreign.max(initial=0) > 0 else -3
        share = lambda m: float(m.mean()) if n else float("nan")
        return DoubletsSummary(n_cells=len(self.label), n_partners=self.n_partners, across=self.across, seed=int(self.seed),
                               n_heterotypic=n, parent_share=share(parent), third_share=share((call >= 0) & ~parent),
                               caught=self.caught(), top_sink=self._name([top])[0],
                               top_sink_pairs=int(foreign[top]) if top >= 0 else 0)

    def _require_same(self, n_cells: int, id2label: Sequence[str], seed: int, across: str) -> None:
        """``into=``: the further partners must be of the same batch shape, cell types, seed and partner rule."""
        if across != self.across:
            raise ValueError(f"into: the table was drawn across={self.across!r}, this call passes across={across!r}")
        _require_same_draws(self, n_cells, id2label, seed)


def _rho_levels(rho) -> Tuple[float, ...]:
    """``ambient``'s ``rho`` as an ascending tuple of distinct floats in [0, 1) (a single number is one level); ValueError
    otherwise."""
    levels = (rho,) if isinstance(rho, (int, float, np.integer, np.floating)) else tuple(rho)
    if not levels:
        raise ValueError("rho: no levels")
    out = []
    for k in levels:
        k = float(k)
        if not 0.0 <= k < 1.0:                                # NaN fails both comparisons
            raise ValueError(f"rho = {k!r}: every level must be in [0, 1)")
        out.append(k)
    return tuple(sorted(set(out)))


class AmbientSummary(dict):
    """``Ambient.summary()``: a dict that prints as one line about the soup and one per level."""

    def __str__(self) -> str:
        d = self
        lines = [f"{d['n_cells']} cells, {d['n_draws']} draws per level; the soup itself is called {d['soup_type']} "
                 f"(probability {d['soup_prob']:.3f})"]
        for k, med, p5 in zip(d["rho"], d["median_agreement"], d["p5_agreement"]):
            lines.append(f"rho {k:g}: agreement median {med:.3f}, 5th percentile {p5:.3f}")
        return "\n".join(lines)


@dataclass
class Ambient(_NamesCalls):
    """What ``ResidentPredictor.ambient`` returns: how a batch's calls fare under ambient-RNA contamination.  B cells (``index``),
    C cell types (``id2label``), L levels (``rho``, ascending: the share of the CONTAMINATED cell's reads that are soup), D draws
    per level.  ``label`` int64 [B] / ``max_prob`` f32 [B]: the call on the cell as given (``classify``'s, -1 = unsure).  Numpy
    arrays per (cell, level, draw) [B, L, D]: ``draw_label`` int32 / ``draw_prob`` f32 = the call on the contaminated counts,
    ``n_mapped`` int32 = the soup reads that fell on bundle genes; ``n_added`` int64 [B, L] = the soup reads a cell takes at a
    level.  ``soup_label`` / ``soup_prob``: what the model calls the soup profile itself - an empty droplet.  ``profile``: the
    soup's weights as ``(int64 [G] over the bundle's genes, the weight outside the bundle)``.  ``seed``: the draws' seed.

    This table characterises the MODEL under contamination; it neither estimates a sample's contamination nor decontaminates
    counts."""
    rho: Tuple[float, ...]
    label: np.ndarray
    max_prob: np.ndarray
    draw_label: np.ndarray
    draw_prob: np.ndarray
    n_added: np.ndarray
    n_mapped: np.ndarray
    soup_label: int
    soup_prob: float
    profile: Tuple[np.ndarray, int]
    index: Sequence
    id2label: Sequence[str]
    seed: int = 0
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    @property
    def n_draws(self) -> int:
        return int(self.draw_label.shape[2])

    def agreement(self) -> np.ndarray:
        """f64 [B, L]: the share of a cell's draws that keep the call as given; NaN for a cell that is unsure as given."""
        lab = np.asarray(self.label, np.int64)
        same = (np.asarray(self.draw_label, np.int64) == lab[:, None, None]).mean(axis=2) if self.n_draws else \
            np.full(self.draw_label.shape[:2], np.nan)
        return np.where(lab[:, None] >= 0, same, np.nan)

    def mean_prob(self) -> np.ndarray:
        """f64 [B, L]: the draws' mean largest softmax probability (whatever label it belongs to)."""
        return np.asarray(self.draw_prob, np.float64).mean(axis=2)

    def _votes(self) -> np.ndarray:
        """int64 [B, L, C]: the draws per label (unsure draws are in none)."""
        B, L, D = self.draw_label.shape
        C = len(self.id2label)
        lab = np.asarray(self.draw_label, np.int64)
        cell_level = np.broadcast_to(np.arange(B * L).reshape(B, L, 1), lab.shape)
        ok = lab >= 0
        return np.bincount(cell_level[ok] * C + lab[ok], minlength=B * L * C).reshape(B, L, C)

    def flips_to(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(ids int64 [B, L], share f64 [B, L])``: per level the cell type OTHER than the call as given that most draws were
        labelled (equal counts: the lower id) and its share of the draws; -1 and 0 when no draw went to another type."""
        other = self._votes()
        B, L, C = other.shape
        lab = np.asarray(self.label, np.int64)
        if B:
            other[np.arange(B), :, np.maximum(lab, 0)] = np.where(lab[:, None] >= 0, -1, other[np.arange(B), :, np.maximum(lab, 0)])
        ids = other.argmax(axis=2) if C else np.zeros((B, L), np.int64)
        top = np.take_along_axis(other, ids[:, :, None], axis=2)[:, :, 0] if C else np.zeros((B, L), np.int64)
        none = top <= 0
        return np.where(none, -1, ids).astype(np.int64), np.where(none, 0.0, top / max(self.n_draws, 1))

    def _level(self, at: float) -> int:
        return int(np.argmin(np.abs(np.asarray(self.rho, np.float64) - float(at))))

    def fragile(self, at: float = 0.1, min_agreement: float = 0.9) -> np.ndarray:
        """Boolean [B]: cells whose agreement at the level nearest ``at`` (the first of equally near ones) is below
        ``min_agreement`` (never a cell that is unsure as given)."""
        with np.errstate(invalid="ignore"):
            return self.agreement()[:, self._level(at)] < float(min_agreement)

    def sinks(self) -> np.ndarray:
        """f64 [L, C]: per level and type T, of the draws CALLED T, the share whose cell is called another type as given (cells
        unsure as given take no part; NaN for a type no draw was called).  A type with a high share takes in contaminated
        cells of other types - for a soup that looks like T, that is the drift this method is about."""
        B, L, D = self.draw_label.shape
        C = len(self.id2label)
        own = np.broadcast_to(np.asarray(self.label, np.int64)[:, None, None], (B, L, D))
        call = np.asarray(self.draw_label, np.int64)
        level = np.broadcast_to(np.arange(L)[None, :, None], (B, L, D))
        ok = (own >= 0) & (call >= 0)
        called = np.bincount(level[ok] * C + call[ok], minlength=L * C).reshape(L, C).astype(np.float64)
        foreign = np.bincount(level[ok & (call != own)] * C + call[ok & (call != own)], minlength=L * C).reshape(L, C)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(called > 0, foreign / called, np.nan)

    def by_type(self) -> pd.DataFrame:
        """One row per level and type that a cell is called as given: ``rho``, ``cell_type``, ``n_cells``, ``retained`` (the share
        of those cells' draws that keep the type), ``unsure`` (the share that come out unsure) and ``becomes`` (the type most of
        the remaining draws are called, the lower id among equals, ``None`` without one)."""
        votes = self._votes()
        lab = np.asarray(self.label, np.int64)
        draws_unsure = (np.asarray(self.draw_label, np.int64) < 0).sum(axis=2)
        rows = []
        for l, k in enumerate(self.rho):
            for t in np.unique(lab[lab >= 0]):
                cells = lab == t
                n = int(cells.sum()) * self.n_draws
                v = votes[cells, l].sum(axis=0)
                rest = v.copy()
                rest[t] = 0
                top = int(rest.argmax())
                rows.append((k, int(t), int(cells.sum()), v[t] / max(n, 1), draws_unsure[cells, l].sum() / max(n, 1),
                             top if rest[top] > 0 else -3))
        cols = list(zip(*rows)) if rows else [[] for _ in range(6)]
        return pd.DataFrame({"rho": np.asarray(cols[0], np.float64), "cell_type": self._name(cols[1]),
                             "n_cells": np.asarray(cols[2], np.int64), "retained": np.asarray(cols[3], np.float64),
                             "unsure": np.asarray(cols[4], np.float64), "becomes": self._name(cols[5])})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` (named as ``predict`` names it), ``prob`` (the call's as given), then per
        level ``added_{rho}`` (the soup reads), ``agree_{rho}``, ``prob_{rho}`` (``mean_prob``), ``flip_{rho}`` (``flips_to``'s
        type by name, ``None`` without one) and ``flip_share_{rho}``."""
        out = {"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob)}
        agree, prob = self.agreement(), self.mean_prob()
        ids, share = self.flips_to()
        for l, k in enumerate(self.rho):
            out[f"added_{k:g}"] = np.asarray(self.n_added)[:, l]
            out[f"agree_{k:g}"] = agree[:, l]
            out[f"prob_{k:g}"] = prob[:, l]
            out[f"flip_{k:g}"] = self._name(np.where(ids[:, l] >= 0, ids[:, l], -3))
            out[f"flip_share_{k:g}"] = share[:, l]
        return pd.DataFrame(out)

    def summary(self) -> AmbientSummary:
        """The soup's own call and, per level, the median and the 5th percentile of the agreement over the cells that are
        called as given (NaN without one); ``print`` it."""
        agree = self.agreement()
        called = np.asarray(self.label, np.int64) >= 0
        stat = lambda f: [float(f(agree[called, l])) if called.any() else float("nan") for l in range(len(self.rho))]
        return AmbientSummary(n_cells=len(self.label), n_draws=self.n_draws, rho=tuple(self.rho), seed=int(self.seed),
                              soup_type=self._name([self.soup_label])[0], soup_label=int(self.soup_label),
                              soup_prob=float(self.soup_prob), median_agreement=stat(np.median),
                              p5_agreement=stat(lambda a: np.percentile(a, 5)))

    def _require_same(self, rho: Sequence[float], n_cells: int, id2label: Sequence[str], seed: int) -> None:
        """``into=``: the further draws must be of the same batch shape, levels, cell types and seed (the profile is compared
        once it is made)."""
        if tuple(rho) != tuple(self.rho):
            raise ValueError(f"into: the table holds the levels {tuple(self.rho)}, this call asks for {tuple(rho)}")
        _require_same_draws(self, n_cells, id2label, seed)


SMOOTH_MAX_NEIGHBORS = HOOD_MAX_MEMBERS - 1         # a cell and its neighbours are one unit of wgnn_hood_rows_*


def _neighbor_lists(neighbors, B: int, include_self: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """``smooth``'s ``neighbors`` as ``(hood_ptr int64 [B + 1], members int32)``: cell ``i`` pools the rows
    ``members[hood_ptr[i]:hood_ptr[i + 1]]`` - with ``include_self`` the cell itself first, then its neighbours in the caller's
    order.  ``neighbors``: an integer ``[B, k]`` array or tensor (-1 = no neighbour) or a scipy sparse ``[B, B]`` matrix whose
    stored non-zero entries of row ``i`` are cell ``i``'s neighbours.  A cell that is its own neighbour (a diagonal entry) is
    dropped; an index outside ``[0, B)``, a neighbour listed twice for one cell and more than 255 neighbours raise
    ``ValueError`` naming the cell.  Host only."""
    B = int(B)
    if sp.issparse(neighbors):
        if tuple(neighbors.shape) != (B, B):
            raise ValueError(f"neighbors: a sparse matrix of shape {tuple(neighbors.shape)}, the batch holds {B} cells ([{B}, {B}])")
        m = sp.csr_matrix(neighbors, copy=True)
        m.sum_duplicates()
        m.eliminate_zeros()
        rows = np.repeat(np.arange(B, dtype=np.int64), np.diff(m.indptr))
        cols = m.indices.astype(np.int64)
    else:
        a = neighbors.detach().cpu().numpy() if isinstance(neighbors, torch.Tensor) else np.asarray(neighbors)
        if a.ndim != 2 or a.shape[0] != B or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise ValueError(f"neighbors: pass an integer [{B}, k] array of cell indices (-1 = no neighbour) or a sparse "
                             f"[{B}, {B}] matrix, got {a.dtype} {tuple(a.shape)}")
        rows = np.repeat(np.arange(B, dtype=np.int64), a.shape[1])
        cols = a.reshape(-1).astype(np.int64)
        listed = cols != -1
        rows, cols = rows[listed], cols[listed]
    outside = np.flatnonzero((cols < 0) | (cols >= B))
    if outside.size:
        raise ValueError(f"neighbors: cell {int(rows[outside[0]])} lists the index {int(cols[outside[0]])}, outside [0, {B})")
    other = cols != rows
    rows, cols = rows[other], cols[other]
    order = np.argsort(rows * max(B, 1) + cols, kind="stable")
    twice = np.flatnonzero((rows[order][1:] == rows[order][:-1]) & (cols[order][1:] == cols[order][:-1]))
    if twice.size:
        at = order[twice[0]]
        raise ValueError(f"neighbors: cell {int(rows[at])} lists the neighbour {int(cols[at])} twice")
    n = np.bincount(rows, minlength=B).astype(np.int64)
    over = np.flatnonzero(n > SMOOTH_MAX_NEIGHBORS)
    if over.size:
        raise ValueError(f"neighbors: cell {int(over[0])} lists {int(n[over[0]])} neighbours, more than {SMOOTH_MAX_NEIGHBORS}")
    own = 1 if include_self else 0
    hood_ptr = np.zeros(B + 1, np.int64)
    np.cumsum(n + own, out=hood_ptr[1:])
    members = np.empty(int(hood_ptr[-1]), np.int32)
    if include_self:
        members[hood_ptr[:-1]] = np.arange(B, dtype=np.int32)
    start = np.concatenate([[0], np.cumsum(n)[:-1]]) if B else np.zeros(0, np.int64)      # rows is ascending: a cell's run
    members[hood_ptr[rows] + own + (np.arange(rows.shape[0]) - start[rows])] = cols
    return hood_ptr, members


class SmoothedSummary(dict):
    """``Smoothed.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells pooled with their neighbours (median {d['median_neighbors']:g}, "
            f"{'with' if d['include_self'] else 'without'} the cell itself)",
            f"unsure as given {d['n_unsure']}, unsure when pooled {d['n_smooth_unsure']}: {d['n_rescued']} rescued, {d['n_lost']} lost, "
            f"{d['n_changed']} called another type",
            f"median neighbour agreement {d['median_agreement']:.3f}"])


@dataclass
class Smoothed(_NamesCalls):
    """What ``ResidentPredictor.smooth`` returns: a batch's calls on kNN-POOLED counts next to the calls as given.  B cells
    (``index``), C cell types (``id2label``).  ``label`` int64 [B] / ``max_prob`` f32 [B]: the call on the cell as given
    (``classify``'s, -1 = unsure).  ``smooth_label`` int64 [B] / ``smooth_prob`` f32 [B] / ``logits`` [B, C] (on the device, as
    ``classify`` returns them): the call on the summed counts of the cell's pool.  ``n_neighbors`` int64 [B]: the neighbours the
    cell was pooled with (itself not counted); ``n_reads`` int64 [B]: the pool's library size, reads outside the bundle
    included; ``n_genes`` / ``smooth_n_genes`` int64 [B]: the bundle genes the cell's own row holds, and the entries its pooled row
    kept.  ``hood_ptr`` / ``members``: the pools as ``_neighbor_lists`` made them; ``include_self``: whether a pool opens with
    the cell itself.

    Pooling across a type boundary blurs a rare cell into its neighbours' type: ``neighbor_agreement`` is the warning."""
    label: np.ndarray
    max_prob: np.ndarray
    smooth_label: np.ndarray
    smooth_prob: np.ndarray
    logits: torch.Tensor
    n_neighbors: np.ndarray
    n_reads: np.ndarray
    n_genes: np.ndarray
    smooth_n_genes: np.ndarray
    hood_ptr: np.ndarray
    members: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    include_self: bool = True
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def _calls(self) -> Tuple[np.ndarray, np.ndarray]:
        return np.asarray(self.label, np.int64), np.asarray(self.smooth_label, np.int64)

    def rescued(self) -> np.ndarray:
        """Boolean [B]: unsure as given, called when pooled."""
        own, pooled = self._calls()
        return (own < 0) & (pooled >= 0)

    def lost(self) -> np.ndarray:
        """Boolean [B]: called as given, unsure when pooled."""
        own, pooled = self._calls()
        return (own >= 0) & (pooled < 0)

    def changed(self) -> np.ndarray:
        """Boolean [B]: called both ways, and another type when pooled."""
        own, pooled = self._calls()
        return (own >= 0) & (pooled >= 0) & (own != pooled)

    def transitions(self) -> np.ndarray:
        """int64 [C + 1, C + 1]: the cells by (call as given, call when pooled), unsure as the last slot of both axes."""
        C = len(self.id2label)
        own, pooled = self._calls()
        slot = lambda x: np.where(x >= 0, x, C)
        return np.bincount(slot(own) * (C + 1) + slot(pooled), minlength=(C + 1) ** 2).reshape(C + 1, C + 1)

    def neighbor_agreement(self) -> np.ndarray:
        """f64 [B]: per cell, the share of its neighbours (itself not counted) whose OWN call is the cell's pooled call; NaN for
        a cell without a neighbour or whose pooled call is unsure.  A low share under a confident pooled call says that the
        neighbourhood straddles two types - or that the pool called what none of its shallow members could."""
        own, pooled = self._calls()
        B = own.shape[0]
        ptr = np.asarray(self.hood_ptr, np.int64)
        cell = np.repeat(np.arange(B), np.diff(ptr))
        member = np.asarray(self.members, np.int64)
        if self.include_self and member.size:                             # a pool opens with the cell itself
            keep = np.ones(member.shape[0], bool)
            keep[ptr[:-1]] = False
            cell, member = cell[keep], member[keep]
        same = np.bincount(cell, weights=(own[member] == pooled[cell]).astype(np.float64), minlength=B)
        n = np.bincount(cell, minlength=B)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((n > 0) & (pooled >= 0), same / n, np.nan)

    def by_type(self) -> pd.DataFrame:
        """One row per call as given (unsure included, last): ``cell_type``, ``n_cells``, ``kept`` (the share whose pooled call
        is the same), ``unsure`` (the share that come out unsure when pooled) and ``becomes`` (the type most of the remaining
        cells are called when pooled, the lower id among equals, ``None`` without one)."""
        C = len(self.id2label)
        t = self.transitions()
        rows = []
        for s in list(range(C)) + [C]:
            n = int(t[s].sum())
            if n == 0:
                continue
            rest = t[s, :C].copy()
            if s < C:
                rest[s] = 0
            top = int(rest.argmax()) if C else 0
            rows.append((s if s < C else -1, n, t[s, s] / n, t[s, C] / n, top if C and rest[top] > 0 else -3))
        cols = list(zip(*rows)) if rows else [[] for _ in range(5)]
        return pd.DataFrame({"cell_type": self._name(cols[0]), "n_cells": np.asarray(cols[1], np.int64),
                             "kept": np.asarray(cols[2], np.float64), "unsure": np.asarray(cols[3], np.float64),
                             "becomes": self._name(cols[4])})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (the call as given, named as ``predict`` names it),
        ``smooth_type`` / ``smooth_prob`` (the call when pooled), ``n_neighbors``, ``n_reads``, ``n_genes``, ``smooth_n_genes`` and
        ``neighbor_agreement``."""
        return pd.DataFrame({"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
                             "smooth_type": self._name(self.smooth_label), "smooth_prob": np.asarray(self.smooth_prob),
                             "n_neighbors": np.asarray(self.n_neighbors), "n_reads": np.asarray(self.n_reads),
                             "n_genes": np.asarray(self.n_genes), "smooth_n_genes": np.asarray(self.smooth_n_genes),
                             "neighbor_agreement": self.neighbor_agreement()})

    def summary(self) -> SmoothedSummary:
        """The cells that pooling rescued, lost and moved to another type, and the median neighbour agreement (NaN without a
        cell that has one); ``print`` it."""
        own, pooled = self._calls()
        agree = self.neighbor_agreement()
        known = ~np.isnan(agree)
        return SmoothedSummary(n_cells=len(own), include_self=bool(self.include_self),
                               median_neighbors=float(np.median(self.n_neighbors)) if len(own) else float("nan"),
                               n_unsure=int((own < 0).sum()), n_smooth_unsure=int((pooled < 0).sum()),
                               n_rescued=int(self.rescued().sum()), n_lost=int(self.lost().sum()), n_changed=int(self.changed().sum()),
                               median_agreement=float(np.median(agree[known])) if known.any() else float("nan"))


class PseudobulkSummary(dict):
    """``Pseudobulk.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_clusters']} clusters pooled from {d['n_cells']} cells: {d['n_called']} called, {d['n_unsure']} unsure, "
            f"{d['n_empty']} empty",
            f"reads per cluster: median {d['median_reads']:.0f}, smallest {d['min_reads']}; genes per cluster: median "
            f"{d['median_genes']:.0f}"])


@dataclass
class Pseudobulk:
    """What ``ResidentPredictor.pseudobulk`` returns: one pooled profile per cluster.  K clusters (``names``), G bundle genes
    (``id2gene``).  Per cluster, numpy arrays [K]: ``n_cells`` int64 the cells pooled, ``n_reads`` int64 their summed library
    sizes (ALL reads, those of genes outside the bundle included), ``n_genes`` int64 the pooled row's entries, ``label`` int64 /
    ``max_prob`` f32 the call on the pooled profile as ``classify`` makes it (-1 = unsure; what an EMPTY cluster's row of zeros
    is called is in here too - ``calls()`` puts -2 there).  On the device: ``logits`` [K, C], the pooled rows as the CSR
    ``(rowptr int64 [K + 1], col int32, val f32)`` the classify path took - ``val`` the log-normalised value of the summed
    count against ``n_reads`` - and ``cnt`` int64, the summed count of every entry."""
    names: Sequence[str]
    n_cells: np.ndarray
    n_reads: np.ndarray
    n_genes: np.ndarray
    label: np.ndarray
    max_prob: np.ndarray
    logits: torch.Tensor
    rowptr: torch.Tensor
    col: torch.Tensor
    val: torch.Tensor
    cnt: torch.Tensor
    id2label: Sequence[str]
    id2gene: Sequence[str] = field(repr=False, default=())
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    @property
    def cluster_names(self) -> Sequence[str]:
        return self.names

    def counts(self) -> sp.csr_matrix:
        """The pooled count matrix, a scipy int64 CSR ``[K, G]`` over the bundle's genes (columns in ``id2gene``'s order) - what
        pseudobulk differential expression starts from.  Reads of genes OUTSIDE the bundle are not in it: they are only in
        ``n_reads``.  With a predictor ``threshold > 0`` the entries whose normalised value is at or below it are absent too."""
        K = len(self.names)
        return sp.csr_matrix((self.cnt.cpu().numpy(), self.col.cpu().numpy(), self.rowptr.cpu().numpy()),
                             shape=(K, len(self.id2gene)), dtype=np.int64)

    def calls(self) -> np.ndarray:
        """int64 [K]: ``label``, with -2 for a cluster without cells (as ``ClusterCalls.consensus`` gives)."""
        return np.where(np.asarray(self.n_cells) == 0, -2, np.asarray(self.label, np.int64)).astype(np.int64)

    def frame(self, calls: Optional["ClusterCalls"] = None, rule: str = "vote", min_fraction: float = 0.0) -> pd.DataFrame:
        """One row per cluster: ``cluster``, ``n_cells``, ``n_reads``, ``n_genes``, the call on the pooled profile as ``cell_type``
        / ``cell_subtype`` (named as ``predict`` names cells; ``unsure`` / ``empty`` spelled out) and its ``probability`` (NaN
        for an empty cluster).  ``calls``: ``annotate``'s table of the same clusters - the frame gains ``vote_type``, the
        per-cell consensus under ``rule`` / ``min_fraction``, and ``agrees``, whether the two calls are the same id."""
        ids = self.calls()
        types, subtypes = _call_names(ids, self.id2label, self.label_map)
        out = pd.DataFrame({"cluster": list(self.names), "n_cells": self.n_cells, "n_reads": self.n_reads, "n_genes": self.n_genes,
                            "cell_type": types, "cell_subtype": subtypes,
                            "probability": np.where(ids == -2, np.nan, np.asarray(self.max_prob, np.float64))})
        if calls is not None:
            if list(calls.cluster_names) != list(self.names):
                raise ValueError("calls: the table's cluster names differ from the pooled profiles'")
            vote, _ = calls.consensus(rule, min_fraction)
            out["vote_type"] = _call_names(vote, self.id2label, self.label_map)[0]
            out["agrees"] = vote == ids
        return out

    def summary(self) -> PseudobulkSummary:
        """The pooled profiles at a glance - clusters called, unsure and empty, reads and genes per cluster; ``print`` it."""
        ids = self.calls()
        on = ids != -2
        med = lambda x: float(np.median(x[on])) if on.any() else float("nan")
        return PseudobulkSummary(n_clusters=len(self.names), n_cells=int(np.sum(self.n_cells)), n_called=int((ids >= 0).sum()),
                                 n_unsure=int((ids == -1).sum()), n_empty=int((~on).sum()), median_reads=med(self.n_reads),
                                 min_reads=int(self.n_reads[on].min()) if on.any() else 0, median_genes=med(self.n_genes))

    def _require_same(self, names: Sequence[str], id2label: Sequence[str], id2gene: Sequence[str]) -> None:
        """``into=``: the batch must be clustered as these profiles are, over the same bundle."""
        if list(names) != list(self.names):
            raise ValueError("into: the profiles' cluster names differ from the batch's")
        if list(id2label) != list(self.id2label) or len(id2gene) != len(self.id2gene):
            raise ValueError("into: the profiles were pooled over another bundle")


class PanelSummary(dict):
    """``PanelCalls.summary()``: a dict that prints as one line per panel."""

    def __str__(self) -> str:
        d = self
        lines = [f"{d['n_cells']} cells ({d['n_called']} with a call), {len(d['names'])} panels"
                 + (", re-normalised per panel" if d["renormalize"] else "")]
        for name, n, a, lost, miss in zip(d["names"], d["n_genes"], d["agreement"], d["n_lost_types"], d["n_missing"]):
            lines.append(f"{name}: {n} bundle genes, agreement {a:.3f}, {lost} types below {d['min_agreement']:g} retained"
                         + (f", {miss} names not found" if miss else ""))
        return "\n".join(lines)


@dataclass
class PanelCalls(_NamesCalls):
    """What ``ResidentPredictor.panels`` returns: per cell, its call when only a NAMED set of genes is measured.  B cells
    (``index``), C cell types (``id2label``), P panels (``names``, ``panels=`` first, then ``without=``), all small host tables.
    ``missing[name]``: the gene names of that panel that resolved nowhere; ``n_genes`` int64 [P]: a panel's bundle genes;
    ``n_columns`` int64 [P]: its caller columns (``None`` without ``genes=``).  ``label`` int64 [B] / ``max_prob`` f32 [B]: the
    call on the cell as given (``classify``'s, -1 = unsure).  ``panel_label`` int64 [B, P] / ``panel_prob`` f32 [B, P]: the call
    on the panel's genes alone; ``n_entries`` int64 [B, P]: the cell's entries that took part; ``n_reads`` int64 [B, P]: the
    cell's reads inside the panel, its library size there (``renormalize=True`` only, else ``None``)."""
    names: List[str]
    missing: dict
    n_genes: np.ndarray
    n_columns: Optional[np.ndarray]
    label: np.ndarray
    max_prob: np.ndarray
    panel_label: np.ndarray
    panel_prob: np.ndarray
    n_entries: np.ndarray
    n_reads: Optional[np.ndarray]
    index: Sequence
    id2label: Sequence[str]
    renormalize: bool = False
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def _panel(self, name) -> int:
        if name not in self.names:
            raise ValueError(f"no panel {name!r}: the panels are {', '.join(map(repr, self.names))}")
        return list(self.names).index(name)

    def agreement(self) -> np.ndarray:
        """f64 [P]: the share of the cells with a full call (``label != -1``) whose panel call equals it (NaN without one)."""
        lab = np.asarray(self.label, np.int64)
        called = lab >= 0
        same = np.asarray(self.panel_label, np.int64)[called] == lab[called, None]
        return same.mean(axis=0) if called.any() else np.full(len(self.names), np.nan)

    def confusion(self, name) -> np.ndarray:
        """int64 [C + 1, C + 1]: cells by full call (rows) and the call on panel ``name`` (columns), the last index = unsure."""
        C = len(self.id2label)
        full = np.asarray(self.label, np.int64)
        sub = np.asarray(self.panel_label, np.int64)[:, self._panel(name)]
        full, sub = np.where(full >= 0, full, C), np.where(sub >= 0, sub, C)
        return np.bincount(full * (C + 1) + sub, minlength=(C + 1) ** 2).reshape(C + 1, C + 1).astype(np.int64)

    def by_type(self) -> pd.DataFrame:
        """One row per (panel, cell type that holds a cell's full call): ``panel``, ``cell_type`` (named as ``predict`` names
        it), ``n_cells``, ``retained`` (the share whose panel call is the same type), ``unsure`` (the share the panel leaves
        unsure), ``other`` (the other type most of them become, the lower id among equals, ``None`` without one) and
        ``other_share``."""
        C = len(self.id2label)
        rows = {k: [] for k in ("panel", "cell_type", "n_cells", "retained", "unsure", "other", "other_share")}
        for name in self.names:
            conf = self.confusion(name)
            for t in np.flatnonzero(conf[:C].sum(axis=1)):
                n = int(conf[t].sum())
                others = conf[t, :C].copy()
                others[t] = 0
                o = int(others.argmax()) if C else 0
                rows["panel"].append(name); rows["cell_type"].append(int(t)); rows["n_cells"].append(n)
                rows["retained"].append(conf[t, t] / n); rows["unsure"].append(conf[t, C] / n)
                rows["other"].append(o if C and others[o] > 0 else -3); rows["other_share"].append(others[o] / n if C else 0.0)
        rows["cell_type"], rows["other"] = self._name(rows["cell_type"]), self._name(rows["other"])
        return pd.DataFrame(rows)

    def lost(self, min_agreement: float = 0.9) -> pd.DataFrame:
        """The rows of ``by_type()`` whose ``retained`` is below ``min_agreement``: the cell types a panel does not carry."""
        t = self.by_type()
        return t[t["retained"] < float(min_agreement)].reset_index(drop=True)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` (named as ``predict`` names it), ``prob`` (the full call's), then per panel
        ``call_{name}``, ``prob_{name}``, ``entries_{name}`` (and ``reads_{name}`` under ``renormalize``)."""
        out = {"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob)}
        for p, name in enumerate(self.names):
            out[f"call_{name}"] = self._name(np.asarray(self.panel_label)[:, p])
            out[f"prob_{name}"] = np.asarray(self.panel_prob)[:, p]
            out[f"entries_{name}"] = np.asarray(self.n_entries)[:, p]
            if self.n_reads is not None:
                out[f"reads_{name}"] = np.asarray(self.n_reads)[:, p]
        return pd.DataFrame(out)

    def summary(self, min_agreement: float = 0.9) -> PanelSummary:
        """Per panel its bundle genes, ``agreement()``, the number of ``lost(min_agreement)`` cell types and of names that were
        not found; ``print`` it."""
        lost = self.lost(min_agreement)
        return PanelSummary(n_cells=int(len(self.label)), n_called=int((np.asarray(self.label) >= 0).sum()), names=list(self.names),
                            renormalize=bool(self.renormalize), n_genes=[int(n) for n in self.n_genes],
                            agreement=[float(a) for a in self.agreement()], min_agreement=float(min_agreement),
                            n_lost_types=[int((lost["panel"] == n).sum()) for n in self.names],
                            n_missing=[len(self.missing.get(n, ())) for n in self.names])


def _signature_scores(rank2_sum, present, deg, set_size, n_genes: int, max_rank: int) -> np.ndarray:
    """The host step of ``wgnn_rank_sets_rows`` (``include/wgnn.h``): f64 [B, P] UCell scores from the kernel's integer sums
    ``rank2_sum`` / ``present`` [B, P], the cells' stored entries ``deg`` [B] and the sets' sizes ``set_size`` [P].  The genes of
    a set that the cell does not store all take the doubled rank ``min(deg + 1 + n_genes, 2 * (max_rank + 1))``; a set of no
    gene scores NaN."""
    n_p = np.asarray(set_size, np.int64)[None, :]
    r2_zero = np.minimum(np.asarray(deg, np.int64) + 1 + int(n_genes), 2 * (int(max_rank) + 1))[:, None]
    # score = 1.0 - float64(two_u) / float64(2 * n_p * max_rank), in place: the tables are [cells, sets], and a fresh temporary
    # per operator is most of this step's time
    two_u = n_p - np.asarray(present, np.int64)
    two_u *= r2_zero
    two_u += np.asarray(rank2_sum, np.int64)
    two_u -= n_p * (n_p + 1)
    score = two_u.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        score /= (2 * n_p * int(max_rank)).astype(np.float64)
    np.subtract(1.0, score, out=score)
    score[:, n_p[0] == 0] = np.nan
    return score


class SignatureSummary(dict):
    """``SignatureScores.summary()``: a dict that prints as one line about the batch and one per set."""

    def __str__(self) -> str:
        d = self
        head = f"{d['n_cells']} cells ({d['n_called']} with a call), {len(d['names'])} sets, max_rank {d['max_rank']}"
        if d["concordant"] is not None:
            head += f"; {d['n_expected']} cells of a type with an expected set, {d['concordant']:.3f} of them concordant"
        lines = [head]
        for name, n, med, top, miss in zip(d["names"], d["set_size"], d["median_score"], d["n_best"], d["n_missing"]):
            lines.append(f"{name}: {n} bundle genes, median score {med:.3f}, the best set of {top} cells"
                         + (f", {miss} names not found" if miss else ""))
        return "\n".join(lines)


@dataclass
class SignatureScores(_NamesCalls):
    """What ``ResidentPredictor.signatures`` returns: per cell, its call next to UCell's rank-based score of every NAMED gene
    set.  B cells (``index``), C cell types (``id2label``), P sets (``names``), all small host tables.  ``missing[name]``: the gene
    names of that set that resolved nowhere; ``set_size`` int64 [P]: a set's genes in the bundle's vocabulary.  ``score`` f64
    [B, P]: ``1 - U / (n * max_rank)`` in [0, 1], NaN for a set of no gene; ``n_present`` int64 [B, P]: the set's genes the cell
    stores; ``n_genes`` int64 [B]: the cell's stored entries, the genes its ranks run over.  ``label`` int64 [B] / ``max_prob``
    f32 [B]: the call on the cell as given (``classify``'s, -1 = unsure).  ``expected``: ``{cell type: set}`` by name, the
    signature the caller expects for a type (or ``None``).

    The scores have no null distribution: 0.3 for one set and 0.3 for another are not the same evidence when their sizes
    differ, and nothing here is a p-value."""
    names: List[str]
    missing: dict
    set_size: np.ndarray
    score: np.ndarray
    n_present: np.ndarray
    n_genes: np.ndarray
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    max_rank: int = 1500
    expected: Optional[dict] = None
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def _set(self, name) -> int:
        if name not in self.names:
            raise ValueError(f"no set {name!r}: the sets are {', '.join(map(repr, self.names))}")
        return list(self.names).index(name)

    def _expected_sets(self) -> np.ndarray:
        """int64 [C]: the index of the set expected for a cell type, -1 without one."""
        of_type = np.full(len(self.id2label), -1, np.int64)
        at = {str(t): i for i, t in enumerate(self.id2label)}
        for cell_type, name in (self.expected or {}).items():
            of_type[at[str(cell_type)]] = self._set(str(name))
        return of_type

    def _own_set(self) -> np.ndarray:
        """int64 [B]: the index of the set expected for the cell's called type, -1 when unsure or without one."""
        lab = np.asarray(self.label, np.int64)
        of_type = self._expected_sets()
        return np.where(lab >= 0, of_type[np.maximum(lab, 0)], -1) if len(of_type) else np.full(lab.shape, -1, np.int64)

    @staticmethod
    def _top(score: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(index, value) of each row's largest entry, NaN skipped, the lower index among equals; (-1, NaN) for a row of NaN."""
        B, P = score.shape
        if P == 0:
            return np.full(B, -1, np.int64), np.full(B, np.nan)
        s = np.where(np.isnan(score), -np.inf, score)
        ids = s.argmax(axis=1)
        val = s[np.arange(B), ids]
        none = np.isneginf(val)
        return np.where(none, -1, ids).astype(np.int64), np.where(none, np.nan, val)

    def best(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(ids int64 [B], margin f64 [B])``: per cell the top-scoring set (equal scores: the lower index; sets that score NaN
        take no part; -1 without one) and its score less the runner-up's (NaN with fewer than two scored sets)."""
        score = np.asarray(self.score, np.float64)
        ids, top = self._top(score)
        rest = score.copy()
        if rest.shape[1]:
            rest[np.arange(rest.shape[0]), np.maximum(ids, 0)] = np.nan
        return ids, top - self._top(rest)[1]

    def own(self) -> np.ndarray:
        """f64 [B]: the score of the set expected for the cell's called type; NaN when the cell is unsure or its type has no
        expected set."""
        own = self._own_set()
        score = np.asarray(self.score, np.float64)
        if not score.shape[1]:
            return np.full(own.shape, np.nan)
        return np.where(own >= 0, score[np.arange(score.shape[0]), np.maximum(own, 0)], np.nan)

    def _rival(self) -> np.ndarray:
        """f64 [B]: the best score among the EXPECTED sets other than the cell's own (NaN without one)."""
        of_type = self._expected_sets()
        sets = np.unique(of_type[of_type >= 0])                        # the expected sets, ascending
        rivals = np.asarray(self.score, np.float64)[:, sets].copy()
        own = self._own_set()
        rows = np.flatnonzero(own >= 0)
        if rows.size:
            rivals[rows, np.searchsorted(sets, own[rows])] = np.nan
        return self._top(rivals)[1]

    def concordant(self, min_margin: float = 0.0) -> np.ndarray:
        """Boolean [B]: among the expected sets, the one of the cell's called type scores highest, by at least ``min_margin``
        (``own() - the best other expected set >= min_margin``; a type whose set is the only expected one is concordant).
        False for a cell that is unsure, whose type has no expected set, or whose own set scores NaN."""
        own, rival = self.own(), self._rival()
        with np.errstate(invalid="ignore"):
            return ~np.isnan(own) & (np.isnan(rival) | (own - rival >= float(min_margin)))

    def by_type(self, min_margin: float = 0.0) -> pd.DataFrame:
        """One row per cell type that holds a cell's call: ``cell_type`` (named as ``predict`` names it), ``n_cells``,
        ``expected`` (its set, ``None`` without one), ``median_own`` (the median of ``own()``), ``concordant`` (the share of
        ``concordant(min_margin)``; NaN without an expected set), ``other`` (among all sets but the expected one, the set that is
        the best of most of the type's cells - the lower index among equals, ``None`` without one) and ``other_share``."""
        lab = np.asarray(self.label, np.int64)
        of_type, own, ok = self._expected_sets(), self.own(), self.concordant(min_margin)
        score = np.asarray(self.score, np.float64)
        P = len(self.names)
        rows = {k: [] for k in ("cell_type", "n_cells", "expected", "median_own", "concordant", "other", "other_share")}
        for t in np.unique(lab[lab >= 0]):
            cells = lab == t
            n = int(cells.sum())
            rest = score[cells].copy()
            if of_type[t] >= 0:
                rest[:, of_type[t]] = np.nan
            wins = self._top(rest)[0]
            votes = np.bincount(wins[wins >= 0], minlength=P)
            o = int(votes.argmax()) if P else 0
            rows["cell_type"].append(int(t)); rows["n_cells"].append(n)
            rows["expected"].append(self.names[of_type[t]] if of_type[t] >= 0 else None)
            rows["median_own"].append(float(np.median(own[cells])) if of_type[t] >= 0 else np.nan)
            rows["concordant"].append(float(ok[cells].mean()) if of_type[t] >= 0 else np.nan)
            rows["other"].append(self.names[o] if P and votes[o] > 0 else None)
            rows["other_share"].append(votes[o] / n if P else 0.0)
        rows["cell_type"] = self._name(rows["cell_type"])
        return pd.DataFrame(rows)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` (named as ``predict`` names it), ``prob``, ``n_genes``, ``best`` (the
        top-scoring set's name, ``None`` without one), ``margin``, with ``expected`` also ``own`` and ``concordant``, then per
        set ``score_{name}``."""
        ids, margin = self.best()
        out = {"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
               "n_genes": np.asarray(self.n_genes), "best": [self.names[i] if i >= 0 else None for i in ids], "margin": margin}
        if self.expected:
            out["own"] = self.own()
            out["concordant"] = self.concordant()
        for p, name in enumerate(self.names):
            out[f"score_{name}"] = np.asarray(self.score)[:, p]
        return pd.DataFrame(out)

    def discordant(self, min_margin: float = 0.0) -> pd.DataFrame:
        """The rows of ``frame()`` to look at: cells whose called type has an expected set and that are not
        ``concordant(min_margin)``."""
        rows = (self._own_set() >= 0) & ~self.concordant(min_margin)
        return self.frame()[rows].reset_index(drop=True)

    def summary(self) -> SignatureSummary:
        """Per set its bundle genes, its median score, the cells it is the best set of and the names that were not found; with
        ``expected`` the share of concordant cells among those whose type has an expected set; ``print`` it."""
        ids = self.best()[0]
        score = np.asarray(self.score, np.float64)
        with_set = self._own_set() >= 0
        scored = [score[:, p][~np.isnan(score[:, p])] for p in range(len(self.names))]
        med = [float(np.median(c)) if c.size else float("nan") for c in scored]
        return SignatureSummary(n_cells=int(len(self.label)), n_called=int((np.asarray(self.label) >= 0).sum()),
                                names=list(self.names), max_rank=int(self.max_rank), set_size=[int(n) for n in self.set_size],
                                median_score=med, n_best=[int((ids == p).sum()) for p in range(len(self.names))],
                                n_missing=[len(self.missing.get(n, ())) for n in self.names],
                                n_expected=int(with_set.sum()),
                                concordant=float(self.concordant()[with_set].mean()) if with_set.any() else None)


def _rank_genes_stats(rank2_sum, tie_sum, n_cells) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The host step of ``wgnn_rank_genes_groups`` (``include/wgnn.h``): ``(U, auc, z, p)`` f64 [K, G] from the kernel's integer
    tables ``rank2_sum`` [K, G] / ``tie_sum`` [G] and the groups' cells ``n_cells`` [K] - a group against the rest of the
    participating cells, the normal approximation with the tie correction and without a continuity correction.  A group that
    is empty or holds every cell has NaN throughout; a gene whose values all tie has ``z = 0, p = 1, auc = 0.5``."""
    from scipy.special import ndtr
    r2 = np.asarray(rank2_sum, np.int64)
    n1 = np.asarray(n_cells, np.int64)[:, None]
    N = int(n1.sum())
    n2 = N - n1
    with np.errstate(invalid="ignore", divide="ignore"):
        U = (r2 - n1 * (n1 + 1)) / 2.0
        mu = (n1 * n2) / 2.0
        var = (n1 * n2) / 12.0 * ((N + 1) - np.asarray(tie_sum, np.int64)[None, :] / (N * (N - 1.0)))
        z = (U - mu) / np.sqrt(var)
        p = 2 * ndtr(-np.abs(z))
        auc = U / (n1 * n2)
    tied = np.broadcast_to(var == 0, U.shape)
    z, p, auc = np.where(tied, 0.0, z), np.where(tied, 1.0, p), np.where(tied, 0.5, auc)
    void = np.broadcast_to((n1 == 0) | (n2 == 0), U.shape)
    return U, np.where(void, np.nan, auc), np.where(void, np.nan, z), np.where(void, np.nan, p)


def _benjamini_hochberg(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg adjusted p-values along the last axis (a row's NaNs stay NaN and take no part)."""
    p = np.asarray(p, np.float64)
    out = np.full(p.shape, np.nan)
    for row, res in zip(p.reshape(-1, p.shape[-1]), out.reshape(-1, p.shape[-1])):
        ok = np.flatnonzero(~np.isnan(row))
        if ok.size:
            order = ok[np.argsort(row[ok], kind="stable")]
            scaled = row[order] * ok.size / np.arange(1, ok.size + 1)
            res[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return out


class GeneRanksSummary(dict):
    """``GeneRanks.summary()``: a dict that prints as one line about the batch and one per group."""

    def __str__(self) -> str:
        d = self
        lines = [f"{d['n_cells']} cells in {len(d['group_names'])} groups ({d['n_skipped']} skipped), {d['n_genes']} genes, "
                 f"p_adj < {d['alpha']}"]
        for name, n, up, down, top in zip(d["group_names"], d["group_cells"], d["n_up"], d["n_down"], d["top_gene"]):
            lines.append(f"{name}: {n} cells, {up} genes up, {down} down" + (f", top {top}" if top is not None else ""))
        return "\n".join(lines)


@dataclass
class GeneRanks:
    """What ``ResidentPredictor.rank_genes`` returns: a Wilcoxon rank-sum test of every gene, each group's cells against the
    rest of the participating cells.  K groups (``group_names``), G genes (``id2gene``), all host tables.  ``n_cells`` int64
    [K]: the cells of each group; ``n_skipped``: the cells with group -1 (unsure, or excluded by the caller), which take no part.
    The kernel's integers: ``rank2_sum`` int64 [K, G] (the doubled tie-averaged ranks of ALL the group's cells, a cell that does
    not store the gene holding 0), ``expr_count`` int32 [K, G] (the group's cells that store the gene), ``tie_sum`` int64 [G]
    (``sum(t^3 - t)`` over the gene's tie groups).  ``mean`` / ``mean_rest`` f64 [K, G]: the mean value in the group and in the
    rest, over all their cells.  ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call when the groups were the
    predicted types, else ``None``; ``index``: the cells' names.

    ``p`` is the normal approximation (ties corrected, no continuity correction).  Cells are not samples: with several donors
    the p-values are far too small (pseudoreplication); ``ResidentPredictor.pseudobulk().counts()`` feeds DESeq2 / edgeR."""
    group_names: Sequence[str]
    id2gene: Sequence[str]
    n_cells: np.ndarray
    n_skipped: int
    rank2_sum: np.ndarray
    expr_count: np.ndarray
    tie_sum: np.ndarray
    mean: np.ndarray
    mean_rest: np.ndarray
    label: Optional[np.ndarray] = None
    max_prob: Optional[np.ndarray] = None
    index: Optional[Sequence] = None

    @functools.cached_property
    def _stats(self):
        return _rank_genes_stats(self.rank2_sum, self.tie_sum, self.n_cells)

    def u(self) -> np.ndarray:
        """f64 [K, G]: Mann-Whitney's U of the group against the rest (``scipy.stats.mannwhitneyu``'s statistic)."""
        return self._stats[0]

    def auc(self) -> np.ndarray:
        """f64 [K, G]: ``U / (n1 * n2)``, the chance that a cell of the group holds more of the gene than one of the rest."""
        return self._stats[1]

    def z(self) -> np.ndarray:
        """f64 [K, G]: the tie-corrected normal score of U (scanpy's ``scores``); positive = higher in the group."""
        return self._stats[2]

    def pvals(self) -> np.ndarray:
        """f64 [K, G]: two-sided, ``2 * ndtr(-|z|)``."""
        return self._stats[3]

    def pvals_adj(self) -> np.ndarray:
        """f64 [K, G]: Benjamini-Hochberg over the genes of one group."""
        return _benjamini_hochberg(self.pvals())

    def logfc(self) -> np.ndarray:
        """f64 [K, G]: scanpy's ``log2((expm1(mean) + 1e-9) / (expm1(mean_rest) + 1e-9))`` (the values taken as log1p's)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.log2((np.expm1(self.mean) + 1e-9) / (np.expm1(self.mean_rest) + 1e-9))

    def _share(self, count: np.ndarray, n: np.ndarray) -> np.ndarray:
        n = np.asarray(n, np.float64)[:, None]
        return np.where(n > 0, count / np.maximum(n, 1.0), 0.0)

    def fraction(self) -> np.ndarray:
        """f64 [K, G]: the share of the group's cells that store the gene (0 for an empty group)."""
        return self._share(np.asarray(self.expr_count, np.float64), self.n_cells)

    def fraction_rest(self) -> np.ndarray:
        """f64 [K, G]: the same among the rest of the participating cells."""
        count = np.asarray(self.expr_count, np.int64)
        n = np.asarray(self.n_cells, np.int64)
        return self._share((count.sum(axis=0)[None, :] - count).astype(np.float64), n.sum() - n)

    def top(self, k: int = 20, min_fraction: float = 0.0, min_logfc: Optional[float] = None,
            max_padj: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Per group the ``k`` genes with the highest ``z``, descending, equal scores by the lower gene id, among the genes with
        ``fraction >= min_fraction``, ``logfc >= min_logfc`` and ``p_adj <= max_padj`` where given: (genes int64 [K, k], -1
        where a group has fewer; z f64 [K, k], 0 there).  An empty group, or one that holds every cell, has none."""
        k = int(k)
        if k < 1:
            raise ValueError(f"top: k = {k} must be positive")
        z = self.z()
        ok = ~np.isnan(z) & (self.fraction() >= float(min_fraction))
        if min_logfc is not None:
            ok &= self.logfc() >= float(min_logfc)
        if max_padj is not None:
            ok &= self.pvals_adj() <= float(max_padj)
        K, G = z.shape
        genes, score = np.full((K, k), -1, np.int64), np.zeros((K, k), np.float64)
        for i in range(K):
            cand = np.flatnonzero(ok[i])
            order = cand[np.argsort(-z[i, cand], kind="stable")][:k]
            genes[i, :order.size], score[i, :order.size] = order, z[i, order]
        return genes, score

    def frame(self, k: int = 20, min_fraction: float = 0.0, min_logfc: Optional[float] = None,
              max_padj: Optional[float] = None) -> pd.DataFrame:
        """Long form, one row per (group, rank): ``group``, ``rank`` (1 = highest z), ``gene``, ``z``, ``auc``, ``logfc``, ``p``,
        ``p_adj``, ``fraction``, ``fraction_rest``, ``mean``."""
        genes, _ = self.top(k, min_fraction, min_logfc, max_padj)
        r, c = np.nonzero(genes >= 0)
        at = (r, genes[r, c])
        return pd.DataFrame({"group": [self.group_names[i] for i in r], "rank": c + 1, "gene": [self.id2gene[j] for j in at[1]],
                             "z": self.z()[at], "auc": self.auc()[at], "logfc": self.logfc()[at], "p": self.pvals()[at],
                             "p_adj": self.pvals_adj()[at], "fraction": self.fraction()[at],
                             "fraction_rest": self.fraction_rest()[at], "mean": np.asarray(self.mean)[at]})

    def compare(self, table: "MarkerTable", k: int = 20) -> pd.DataFrame:
        """Does the model lean on the genes that separate the type?  Per group the model's top-``k`` attribution genes
        (``table.top(k)``, ``ResidentPredictor.markers`` of the same bundle and grouping) against the data's top-``k`` by z:
        ``group``, ``n_model``, ``n_data``, ``n_shared``, ``jaccard`` (NaN when both lists are empty), ``model_only`` and
        ``data_only`` (gene names, in rank order).  ``ValueError`` when the two tables' group or gene names differ."""
        if list(table.group_names) != list(self.group_names):
            raise ValueError("compare: the marker table's group names differ from this table's")
        if list(table.id2gene) != list(self.id2gene):
            raise ValueError("compare: the marker table's gene names differ from this table's")
        model, _ = table.top(k)
        data, _ = self.top(k)
        rows = []
        for i, name in enumerate(self.group_names):
            m, d = [int(g) for g in model[i] if g >= 0], [int(g) for g in data[i] if g >= 0]
            shared = set(m) & set(d)
            union = len(set(m) | set(d))
            rows.append({"group": name, "n_model": len(m), "n_data": len(d), "n_shared": len(shared),
                         "jaccard": len(shared) / union if union else float("nan"),
                         "model_only": [self.id2gene[g] for g in m if g not in shared],
                         "data_only": [self.id2gene[g] for g in d if g not in shared]})
        return pd.DataFrame(rows, columns=["group", "n_model", "n_data", "n_shared", "jaccard", "model_only", "data_only"])

    def summary(self, alpha: float = 0.05) -> GeneRanksSummary:
        """Per group its cells, the genes up and down at ``p_adj < alpha`` and the top gene by z; ``print`` it."""
        z, adj = self.z(), self.pvals_adj()
        with np.errstate(invalid="ignore"):
            sig = adj < float(alpha)
            up, down = (sig & (z > 0)).sum(axis=1), (sig & (z < 0)).sum(axis=1)
        first = self.top(1)[0][:, 0]
        return GeneRanksSummary(n_cells=int(np.asarray(self.n_cells).sum()), n_skipped=int(self.n_skipped),
                                n_genes=len(self.id2gene), alpha=float(alpha), group_names=list(self.group_names),
                                group_cells=[int(n) for n in self.n_cells], n_up=[int(n) for n in up],
                                n_down=[int(n) for n in down],
                                top_gene=[self.id2gene[g] if g >= 0 else None for g in first])


KNN_SPACES = ("hidden", "features")
KNN_METRICS = ("euclidean", "cosine")


class NeighborGraphSummary(dict):
    """``NeighborGraph.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells, k = {d['k']} nearest neighbours in the {d['space']} space ({d['metric']}), "
            f"{d['n_edges']} edges, {d['n_without']} cells without a neighbour",
            f"median distance to the nearest {d['median_nearest']:.4g}, to the last listed {d['median_kth']:.4g}; "
            f"{d['mutual_share']:.3f} of the edges are mutual",
            f"median label agreement {d['median_agreement']:.3f} ({d['n_unsure']} cells unsure)"])


@dataclass
class NeighborGraph(_NamesCalls):
    """What ``ResidentPredictor.knn`` returns: the exact k-nearest-neighbour graph of one batch, among the batch's own cells.
    B cells (``index``), C cell types (``id2label``).  ``indices`` int64 [B, k]: a cell's neighbours by ascending (distance,
    index), the cell itself left out, -1 = none (a batch of fewer than k + 1 cells, NaN rows) - as it stands the ``neighbors``
    argument of ``ResidentPredictor.smooth``.  ``sq_distances`` f32 [B, k]: the kernel's squared Euclidean distances, bit for
    bit (+inf beside a -1); under ``metric="cosine"`` they are those of the L2-normalised rows, ``2 (1 - cos)``.  ``space``
    ("hidden" | "features") and ``metric`` ("euclidean" | "cosine") say what was measured; ``label`` int64 [B] / ``max_prob``
    f32 [B]: ``classify``'s call of the batch (-1 = unsure).

    A graph in the hidden space is the classifier's own view of the batch: ``label_agreement`` is high there by construction."""
    indices: np.ndarray
    sq_distances: np.ndarray
    k: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def _listed(self) -> np.ndarray:
        return np.asarray(self.indices, np.int64) >= 0

    def distances(self) -> np.ndarray:
        """f32 [B, k]: Euclidean distances (the square roots, taken on the host), or for ``metric="cosine"`` the cosine
        distances ``1 - cos = d2 / 2`` of the unit rows; +inf beside a -1."""
        d2 = np.asarray(self.sq_distances, np.float32)
        return d2 / np.float32(2) if self.metric == "cosine" else np.sqrt(d2)

    def to_scipy(self) -> sp.csr_matrix:
        """CSR ``[B, B]`` of ``distances()``, one stored entry per listed neighbour in the order of the lists - the layout of
        ``adata.obsp["distances"]`` (a neighbour at distance 0 is a stored zero)."""
        ok = self._listed()
        B = ok.shape[0]
        indptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int64)
        return sp.csr_matrix((self.distances()[ok], np.asarray(self.indices, np.int64)[ok], indptr), shape=(B, B))

    def mutual(self) -> np.ndarray:
        """Boolean [B, k]: true where the listed neighbour lists the cell back."""
        idx, ok = np.asarray(self.indices, np.int64), self._listed()
        B = idx.shape[0]
        rows = np.repeat(np.arange(B), ok.sum(axis=1))
        edges = sp.csr_matrix((np.ones(rows.shape[0], np.int8), (rows, idx[ok])), shape=(B, B))
        out = np.zeros(idx.shape, bool)
        out[ok] = np.asarray(edges.T.tocsr()[rows, idx[ok]]).ravel() > 0
        return out

    def label_agreement(self) -> np.ndarray:
        """f64 [B]: per cell, the share of its neighbours whose call equals the cell's own; an unsure neighbour, and every
        neighbour of an unsure cell, counts as disagreeing.  NaN for a cell without a neighbour."""
        idx, ok = np.asarray(self.indices, np.int64), self._listed()
        own = np.asarray(self.label, np.int64)
        theirs = own[np.where(ok, idx, 0)]
        same = ok & (theirs == own[:, None]) & (theirs >= 0)
        n = ok.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, same.sum(axis=1) / n, np.nan)

    def by_type(self) -> pd.DataFrame:
        """One row per call (unsure included, last): ``cell_type``, ``n_cells``, ``median_nearest`` / ``median_kth`` (the
        distance to the first and to the last listed neighbour), ``mutual`` (the share of the cells' edges that are mutual) and
        ``agreement`` (the mean ``label_agreement``)."""
        own, ok = np.asarray(self.label, np.int64), self._listed()
        dist, mutual, agree = self.distances(), self.mutual(), self.label_agreement()
        n = ok.sum(axis=1)
        last = dist[np.arange(len(n)), np.maximum(n - 1, 0)] if dist.shape[1] else np.full(len(n), np.nan, np.float32)
        rows = []
        for s in sorted(set(own[own >= 0].tolist())) + ([-1] if (own < 0).any() else []):
            m = (own == s) if s >= 0 else (own < 0)
            has = m & (n > 0)
            med = lambda v: float(np.median(v[has])) if has.any() else float("nan")
            edges = int(ok[m].sum())
            rows.append((s, int(m.sum()), med(dist[:, 0]) if dist.shape[1] else float("nan"), med(last),
                         mutual[m].sum() / edges if edges else float("nan"), float(np.mean(agree[has])) if has.any() else float("nan")))
        cols = list(zip(*rows)) if rows else [[] for _ in range(6)]
        return pd.DataFrame({"cell_type": self._name(cols[0]), "n_cells": np.asarray(cols[1], np.int64),
                             "median_nearest": np.asarray(cols[2], np.float64), "median_kth": np.asarray(cols[3], np.float64),
                             "mutual": np.asarray(cols[4], np.float64), "agreement": np.asarray(cols[5], np.float64)})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (named as ``predict`` names them), ``n_neighbors``,
        ``nearest`` (the first neighbour's name, ``None`` without one), ``nearest_distance``, ``kth_distance`` (to the last
        listed neighbour), ``n_mutual`` and ``label_agreement``."""
        idx, ok = np.asarray(self.indices, np.int64), self._listed()
        dist, n = self.distances(), ok.sum(axis=1)
        names = list(self.index)
        B = len(n)
        has = n > 0
        pick = lambda j: np.where(has, dist[np.arange(B), j], np.nan) if dist.shape[1] else np.full(B, np.nan)
        return pd.DataFrame({"index": names, "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
                             "n_neighbors": n.astype(np.int64),
                             "nearest": [names[idx[i, 0]] if has[i] else None for i in range(B)],
                             "nearest_distance": pick(np.zeros(B, np.int64)), "kth_distance": pick(np.maximum(n - 1, 0)),
                             "n_mutual": self.mutual().sum(axis=1).astype(np.int64), "label_agreement": self.label_agreement()})

    def summary(self) -> NeighborGraphSummary:
        """Cells, edges, the median nearest and last listed distance, the share of mutual edges and the median label
        agreement; ``print`` it."""
        ok, dist, agree = self._listed(), self.distances(), self.label_agreement()
        n = ok.sum(axis=1)
        has = n > 0
        med = lambda v: float(np.median(v)) if len(v) else float("nan")
        last = dist[np.arange(len(n)), np.maximum(n - 1, 0)][has] if dist.shape[1] else np.zeros(0)
        return NeighborGraphSummary(n_cells=len(n), k=int(self.k), space=self.space, metric=self.metric, n_edges=int(ok.sum()),
                                    n_without=int((~has).sum()), median_nearest=med(dist[has, 0]) if dist.shape[1] else float("nan"),
                                    median_kth=med(last), mutual_share=float(self.mutual().sum() / ok.sum()) if ok.any() else float("nan"),
                                    n_unsure=int((np.asarray(self.label) < 0).sum()), median_agreement=med(agree[has]))

    def _named_labels(self, name: str) -> np.ndarray:
        """``lisi``'s ``labels`` given as a word."""
        if name == "predicted":
            return np.asarray(self.label, np.int64)
        raise ValueError(f"labels = {name!r}: pass one id per cell or 'predicted'")

    def lisi(self, labels="predicted", perplexity: Optional[float] = None, n_labels: Optional[int] = None) -> np.ndarray:
        """f64 [B]: the Local Inverse Simpson's Index of ``labels`` on this graph (Korsunsky et al. 2019) - per cell the
        effective number of labels among its neighbours, between 1 (one label) and the number of labels (all equally
        present).  On the host in float64; ``O(B k)``.  ``labels``: one integer id per cell in ``[-1, n_labels)``
        (``n_labels`` = None: the largest id + 1), or ``"predicted"`` for the graph's own ``label``.

        Per cell, over its listed neighbours ``j`` with a finite distance: ``D_j = distances()[j]`` minus the nearest of them,
        ``P_j = exp(-beta D_j)``, with ``beta`` from the t-SNE search of the published ``compute_simpson_index`` - start at 1,
        double or halve until bracketed, then bisect - towards the entropy ``log(perplexity)``, a fixed 64 tries with no
        tolerance exit (so that the result is a function of the lists alone); then ``1 / sum_l (sum_{j in l} P_j / sum_j P_j)^2``.
        ``perplexity`` defaults to ``k / 3``; outside ``[1, k)`` it raises ``ValueError``.  A cell with fewer than two such
        neighbours gives NaN.  A neighbour with label -1 (unsure) counts as a label of its own kind: its ``P_j`` stays in
        ``sum_j P_j`` and is left out of every label's numerator, so it raises the index like a stranger would; a cell whose
        neighbours are all -1 gives NaN.

        LISI over BATCHES measures the mixing of a PLAIN ``knn`` graph - whether ``bbknn`` is needed at all.  A ``BatchGraph``
        is balanced by construction and its batch LISI says nothing."""
        idx = np.asarray(self.indices, np.int64)
        B, k = idx.shape
        lab = self._named_labels(labels) if isinstance(labels, str) else np.asarray(labels)
        if lab.ndim != 1 or lab.shape[0] != B or lab.dtype.kind not in "iu":
            raise ValueError(f"labels must hold one integer id per cell ([{B}]), got {lab.dtype} {lab.shape}")
        lab = lab.astype(np.int64)
        L = int(n_labels) if n_labels is not None else (int(lab.max()) + 1 if B else 0)
        if B and (lab.min() < -1 or lab.max() >= L):
            raise ValueError(f"label id out of range [-1, {L})")
        perplexity = k / 3 if perplexity is None else float(perplexity)
        if not 1 <= perplexity < k:
            raise ValueError(f"perplexity = {perplexity:g} is outside [1, k = {k})")
        dist = self.distances().astype(np.float64)
        ok = (idx >= 0) & np.isfinite(dist)
        with np.errstate(invalid="ignore"):
            D = np.where(ok, dist - np.min(np.where(ok, dist, np.inf), axis=1, keepdims=True), 0.0)
        theirs = np.where(ok, lab[np.where(ok, idx, 0)], -1)
        target = np.log(perplexity)

        def entropy(beta):                                   # column by column: a row's sums run in list order
            P = np.where(ok, np.exp(-D * beta[:, None]), 0.0)
            total, weighted = np.zeros(B), np.zeros(B)
            for j in range(k):
                total, weighted = total + P[:, j], weighted + D[:, j] * P[:, j]
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.log(total) + beta * weighted / total, P, total

        beta, low, high = np.ones(B), np.full(B, -np.inf), np.full(B, np.inf)
        H, P, total = entropy(beta)
        for _ in range(64):
            up = H > target                                  # too flat: sharpen
            with np.errstate(invalid="ignore"):
                low, high = np.where(up, beta, low), np.where(up, high, beta)
                beta = np.where(up, np.where(np.isinf(high), beta * 2.0, (beta + high) / 2.0),
                                np.where(np.isinf(low), beta / 2.0, (beta + low) / 2.0))
            H, P, total = entropy(beta)
        share = np.zeros((B, max(L, 1)))
        for j in range(k):
            rows = np.flatnonzero(theirs[:, j] >= 0)
            share[rows, theirs[rows, j]] += P[rows, j]
        simpson = np.zeros(B)
        with np.errstate(invalid="ignore", divide="ignore"):
            for l in range(L):
                s = share[:, l] / total
                simpson = simpson + s * s
            return np.where((ok.sum(axis=1) >= 2) & (simpson > 0), 1.0 / simpson, np.nan)


class BatchGraphSummary(NeighborGraphSummary):
    """``BatchGraph.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        sizes = ", ".join(f"{name}: {n}" for name, n in d["batch_sizes"].items())
        return "\n".join([NeighborGraphSummary.__str__(self),
                          f"{d['n_batches']} batches, {d['k_within']} neighbours from each ({sizes}); {d['n_short']} cells with a "
                          f"short list, median share of neighbours from another batch {d['median_batch_share']:.3f}"])


@dataclass(kw_only=True)
class BatchGraph(NeighborGraph):
    """What ``ResidentPredictor.bbknn`` returns: a batch-balanced kNN graph (BBKNN, Polanski et al. 2020) - every cell lists its
    ``k_within`` nearest cells in EACH of S batches.  It IS a ``NeighborGraph``: ``indices`` / ``sq_distances`` [B, k] with ``k =
    S * k_within`` are the union of a cell's S lists as one list, ascending by (distance, index), -1 / +inf last - what every
    ``graph=`` argument reads.  ``batch`` int64 [B]: a cell's batch id; ``batch_names``: the S names; ``by_batch_indices`` int64 /
    ``by_batch_sq_distances`` f32 [B, S, k_within]: the lists one batch at a time, each ascending, a cell left out of the list
    into its own batch, -1 / +inf where a batch holds fewer cells."""
    batch: np.ndarray
    batch_names: Sequence[str]
    k_within: int
    by_batch_indices: np.ndarray
    by_batch_sq_distances: np.ndarray

    def _named_labels(self, name: str) -> np.ndarray:
        if name == "batch":
            return np.asarray(self.batch, np.int64)
        return super()._named_labels(name)

    def batch_share(self) -> np.ndarray:
        """f64 [B]: per cell, the share of its listed neighbours that come from another batch - ``(S - 1) / S`` by construction
        wherever all S lists are full.  NaN for a cell without a neighbour."""
        idx, ok = np.asarray(self.indices, np.int64), self._listed()
        own = np.asarray(self.batch, np.int64)
        other = ok & (own[np.where(ok, idx, 0)] != own[:, None])
        n = ok.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, other.sum(axis=1) / n, np.nan)

    def _nearest_by_batch(self) -> np.ndarray:
        """f32 [B, S]: a cell's distance (as ``distances()`` measures) to its nearest cell of every batch, +inf without one."""
        d2 = np.asarray(self.by_batch_sq_distances, np.float32)[:, :, 0]
        return d2 / np.float32(2) if self.metric == "cosine" else np.sqrt(d2)

    def by_batch(self) -> pd.DataFrame:
        """One row per batch, over the cells OF that batch: ``batch``, ``n_cells``, ``n_short`` (its cells with fewer than ``k``
        listed neighbours - some batch holds fewer than ``k_within`` other cells) and one column ``nearest_{name}`` per batch:
        the median distance from the row's cells to their nearest cell of that batch (NaN without one).  The row's own column is
        the scale within the batch that the others are read against."""
        own, n = np.asarray(self.batch, np.int64), self._listed().sum(axis=1)
        near = self._nearest_by_batch().astype(np.float64)
        near[~np.isfinite(near)] = np.nan
        names = list(self.batch_names)
        out = {"batch": names, "n_cells": np.asarray([(own == s).sum() for s in range(len(names))], np.int64),
               "n_short": np.asarray([((own == s) & (n < self.k)).sum() for s in range(len(names))], np.int64)}
        for c, name in enumerate(names):
            col = [near[own == s, c] for s in range(len(names))]
            out[f"nearest_{name}"] = np.asarray([np.nanmedian(v) if np.isfinite(v).any() else np.nan for v in col], np.float64)
        return pd.DataFrame(out)

    def summary(self) -> BatchGraphSummary:
        """``NeighborGraph.summary()`` with the batch sizes, the cells with a short list and the median ``batch_share``."""
        own, share = np.asarray(self.batch, np.int64), self.batch_share()
        share = share[~np.isnan(share)]
        return BatchGraphSummary(**NeighborGraph.summary(self), n_batches=len(self.batch_names), k_within=int(self.k_within),
                                 batch_sizes={str(name): int((own == s).sum()) for s, name in enumerate(self.batch_names)},
                                 n_short=int((self._listed().sum(axis=1) < self.k).sum()),
                                 median_batch_share=float(np.median(share)) if len(share) else float("nan"))


class KMeansSummary(dict):
    """``KMeans.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        how = f"converged after {d['n_iter']} assignments" if d["converged"] else f"NOT converged after {d['n_iter']} assignments"
        return "\n".join([
            f"{d['n_cells']} cells in {d['n_clusters']} clusters of the {d['space']} space ({d['metric']}), {how}; "
            f"{d['n_skipped']} cells without a cluster, {d['n_empty']} empty clusters",
            f"cluster sizes {d['min_size']} .. {d['max_size']} (median {d['median_size']:.4g}), inertia {d['inertia']:.6g}",
            f"median purity {d['median_purity']:.3f}, {d['n_mixed']} clusters below 0.9 ({d['n_unsure']} cells unsure)"])


class _CellClusters(_NamesCalls):
    """What the tables of per-cell clusters (``KMeans``, ``Communities``) share: ``cluster`` int64 [B] with -1 = none, ``size``
    int64 [K], ``label`` / ``index`` / ``id2label``."""

    @property
    def n_clusters(self) -> int:
        return int(np.asarray(self.size).shape[0])

    @property
    def cluster_names(self) -> List[str]:
        width = max(4, len(str(self.n_clusters - 1)))
        return [f"c{k:0{width}d}" for k in range(self.n_clusters)]

    def composition(self) -> pd.DataFrame:
        """Clusters x called types, as counts: one row per cluster (``cluster_names``), one column per cell type in ``id2label``'s
        order (named as ``predict`` names them) and ``unsure`` last.  A cell without a cluster is counted nowhere."""
        K, C = self.n_clusters, len(self.id2label)
        cl, lab = np.asarray(self.cluster, np.int64), np.asarray(self.label, np.int64)
        on = cl >= 0
        table = np.zeros((K, C + 1), np.int64)
        np.add.at(table, (cl[on], np.where(lab[on] >= 0, lab[on], C)), 1)
        return pd.DataFrame(table, index=self.cluster_names, columns=self._name(np.arange(C)) + ["unsure"])

    def purity(self) -> np.ndarray:
        """f64 [K]: per cluster, the share of its CALLED cells (unsure ones left out) that carry the cluster's majority call;
        NaN for a cluster without a called cell."""
        called = self.composition().to_numpy()[:, :-1]
        n = called.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, called.max(axis=1, initial=0) / n, np.nan)

    def clusters_frame(self) -> pd.DataFrame:
        """One row per cell - a running number, the cell's name, its cluster's name (empty for a cell without one): written with
        its header and without pandas' own index this is the clusters file ``annotate_file`` / ``pseudobulk_file`` read."""
        names = self.cluster_names
        return pd.DataFrame({"index": np.arange(len(self.cluster), dtype=np.int64), "cell": [str(c) for c in self.index],
                             "cluster": [names[k] if k >= 0 else "" for k in np.asarray(self.cluster, np.int64)]})


@dataclass
class KMeans(_CellClusters):
    """What ``ResidentPredictor.kmeans`` returns: the k-means clusters of one batch in the model's space.  B cells (``index``),
    K clusters (``cluster_names``: ``"c0000"``, ... - zero-padded, so sorted order is id order), C cell types (``id2label``).
    ``cluster`` int64 [B]: a cell's cluster, -1 for a cell whose embedding holds a non-finite value - as it stands, with
    ``n_clusters=K``, the ``clusters`` argument of ``annotate`` / ``pseudobulk`` and ``rank_genes``' ``groups``.
    ``sq_distance`` f32 [B]: the squared distance to the cell's centre (NaN beside a -1); ``centers`` f32 [K, D];
    ``size`` int64 [K]; ``seed_cells`` int64 [K]: the cells the seeding chose (``None`` with an init array); ``inertia``: the sum
    of ``sq_distance``, ``inertia_trace`` the same after every assignment; ``n_iter`` / ``converged``: ``ops.kmeans_rows``'.
    ``space`` / ``metric`` say what was clustered (under ``"cosine"`` the L2-normalised rows; the centres are their plain means,
    not re-normalised); ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure)."""
    cluster: np.ndarray
    sq_distance: np.ndarray
    centers: np.ndarray
    size: np.ndarray
    seed_cells: Optional[np.ndarray]
    inertia: float
    inertia_trace: Sequence[float]
    n_iter: int
    converged: bool
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (named as ``predict`` names them), ``cluster`` (its name, ``None``
        without one), ``sq_distance``, and the cluster's ``cluster_size`` and ``cluster_purity``."""
        names, cl = self.cluster_names, np.asarray(self.cluster, np.int64)
        on, at = cl >= 0, np.maximum(cl, 0)
        return pd.DataFrame({"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
                             "cluster": [names[k] if k >= 0 else None for k in cl],
                             "sq_distance": np.asarray(self.sq_distance, np.float32),
                             "cluster_size": np.where(on, np.asarray(self.size, np.int64)[at], 0),
                             "cluster_purity": np.where(on, self.purity()[at], np.nan)})

    def summary(self) -> KMeansSummary:
        """Cells, clusters, sizes, the inertia and the clusters' purity against ``classify``'s calls; ``print`` it."""
        size, purity = np.asarray(self.size, np.int64), self.purity()
        filled = size[size > 0]
        known = purity[~np.isnan(purity)]
        return KMeansSummary(n_cells=len(self.cluster), n_clusters=self.n_clusters, space=self.space, metric=self.metric,
                             n_iter=int(self.n_iter), converged=bool(self.converged),
                             n_skipped=int((np.asarray(self.cluster) < 0).sum()), n_empty=int((size == 0).sum()),
                             min_size=int(filled.min()) if filled.size else 0, max_size=int(filled.max()) if filled.size else 0,
                             median_size=float(np.median(filled)) if filled.size else float("nan"), inertia=float(self.inertia),
                             median_purity=float(np.median(known)) if known.size else float("nan"),
                             n_mixed=int((known < 0.9).sum()), n_unsure=int((np.asarray(self.label) < 0).sum()))


class SilhouetteSummary(dict):
    """``Silhouette.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells in {d['n_groups']} non-empty groups of the {d['space']} space ({d['metric']}); "
            f"{d['n_skipped']} cells take no part, {d['n_singletons']} groups are singletons",
            f"mean silhouette {d['mean']:.4f} (median {d['median']:.4f}); {d['n_misplaced']} cells ({d['misplaced_share']:.3f}) "
            f"sit closer to another group than to their own",
            f"worst group {d['worst_group']} (mean {d['worst_mean']:.4f}), best group {d['best_group']} (mean {d['best_mean']:.4f}) "
            f"({d['n_unsure']} cells unsure)"])


@dataclass
class Silhouette(_NamesCalls):
    """What ``ResidentPredictor.silhouette`` returns: the exact silhouette (Rousseeuw 1987) of every cell of one batch against
    given groups, in the model's space.  B cells (``index``), K groups (``group_names``), C cell types (``id2label``).
    ``group`` int64 [B]: the cell's group as the call resolved it (-1 = the cell takes no part: skipped by the caller, unsure
    under ``groups="predicted"``, or an embedding with a non-finite value).  ``a`` f64 [B]: the mean distance to the other cells
    of the cell's own group (0 for a singleton); ``b`` f64 [B]: the lowest mean distance to the cells of another group;
    ``nearest`` int64 [B]: that group; ``score`` f64 [B]: ``(b - a) / max(a, b)`` in [-1, 1] - 0 for a singleton and where
    ``max(a, b) == 0``, below 0 where the cell sits closer to ``nearest`` than to its own group.  NaN / NaN / -1 / NaN for a
    cell that takes no part.  ``size`` int64 [K]: the participating cells per group; ``n_skipped``: the cells that take no part.
    ``space`` / ``metric`` say what was measured (under ``"cosine"`` the Euclidean distances of the L2-normalised rows);
    ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure)."""
    a: np.ndarray
    b: np.ndarray
    score: np.ndarray
    nearest: np.ndarray
    group: np.ndarray
    group_names: Sequence[str]
    size: np.ndarray
    n_skipped: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def _on(self) -> np.ndarray:
        return np.asarray(self.group, np.int64) >= 0

    def mean(self) -> float:
        """The mean ``score`` over the participating cells - the figure to compare across ``n_clusters``; NaN without one."""
        s = np.asarray(self.score, np.float64)[self._on()]
        return float(s.mean()) if s.size else float("nan")

    def by_group(self) -> pd.DataFrame:
        """One row per group (``group_names``' order, empty groups included): ``group``, ``n_cells``, ``mean`` and ``median``
        score, ``negative`` (the share of its cells with ``score < 0``) and ``nearest`` (the group most of THOSE cells are
        nearest to - of equal counts the lower id; ``None`` without such a cell)."""
        K = len(self.group_names)
        g, s, near = np.asarray(self.group, np.int64), np.asarray(self.score, np.float64), np.asarray(self.nearest, np.int64)
        rows = []
        for k in range(K):
            m = g == k
            n = int(m.sum())
            neg = m & (s < 0) & (near >= 0)
            to = np.bincount(near[neg], minlength=K) if neg.any() else None
            rows.append((self.group_names[k], n, float(s[m].mean()) if n else float("nan"),
                         float(np.median(s[m])) if n else float("nan"), float((s[m] < 0).mean()) if n else float("nan"),
                         None if to is None else self.group_names[int(np.argmax(to))]))
        cols = list(zip(*rows)) if rows else [[] for _ in range(6)]
        return pd.DataFrame({"group": list(cols[0]), "n_cells": np.asarray(cols[1], np.int64), "mean": np.asarray(cols[2], np.float64),
                             "median": np.asarray(cols[3], np.float64), "negative": np.asarray(cols[4], np.float64),
                             "nearest": list(cols[5])})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (named as ``predict`` names them), ``group`` and ``nearest``
        (the groups' names, ``None`` without one), ``a``, ``b`` and ``score``."""
        names = list(self.group_names)
        pick = lambda ids: [names[k] if k >= 0 else None for k in np.asarray(ids, np.int64)]
        return pd.DataFrame({"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
                             "group": pick(self.group), "nearest": pick(self.nearest), "a": np.asarray(self.a, np.float64),
                             "b": np.asarray(self.b, np.float64), "score": np.asarray(self.score, np.float64)})

    def misplaced(self, max_score: float = 0.0) -> pd.DataFrame:
        """The rows of ``frame()`` to look at: the participating cells with ``score < max_score``, lowest score first (equal
        scores in batch order)."""
        s = np.asarray(self.score, np.float64)
        rows = np.nonzero(self._on() & (s < float(max_score)))[0]
        rows = rows[np.argsort(s[rows], kind="stable")]
        return self.frame().iloc[rows].reset_index(drop=True)

    def summary(self) -> SilhouetteSummary:
        """Cells, groups, the mean and median score, the cells with a negative score and the worst and best group; ``print`` it."""
        on, s, size = self._on(), np.asarray(self.score, np.float64), np.asarray(self.size, np.int64)
        part = s[on]
        per = self.by_group()
        known = per[~np.isnan(per["mean"].to_numpy())]
        worst = known.iloc[int(np.argmin(known["mean"].to_numpy()))] if len(known) else None
        best = known.iloc[int(np.argmax(known["mean"].to_numpy()))] if len(known) else None
        return SilhouetteSummary(n_cells=int(on.sum()), n_groups=int((size > 0).sum()), space=self.space, metric=self.metric,
                                 n_skipped=int(self.n_skipped), n_singletons=int((size == 1).sum()), mean=self.mean(),
                                 median=float(np.median(part)) if part.size else float("nan"),
                                 n_misplaced=int((part < 0).sum()),
                                 misplaced_share=float((part < 0).mean()) if part.size else float("nan"),
                                 worst_group=None if worst is None else worst["group"],
                                 worst_mean=float("nan") if worst is None else float(worst["mean"]),
                                 best_group=None if best is None else best["group"],
                                 best_mean=float("nan") if best is None else float(best["mean"]),
                                 n_unsure=int((np.asarray(self.label) < 0).sum()))


class CommunitiesSummary(dict):
    """``Communities.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        how = "converged" if d["converged"] else "NOT converged (a level stopped at max_sweeps)"
        return "\n".join([
            f"{d['n_cells']} cells in {d['n_clusters']} {d.get('method', 'louvain').capitalize()} communities of the k = {d['k']} graph in the {d['space']} space "
            f"({d['metric']}, {d['weights']} weights), resolution {d['resolution']}, {how}; {d['n_skipped']} cells without an edge",
            f"{d['n_levels']} levels, {d['n_sweeps']} sweeps, {d['n_fallback']} fallback moves, modularity {d['modularity']:.4f}",
            f"community sizes {d['min_size']} .. {d['max_size']} (median {d['median_size']:.4g})",
            f"median purity {d['median_purity']:.3f}, {d['n_mixed']} communities below 0.9 ({d['n_unsure']} cells unsure)"])


@dataclass
class Communities(_CellClusters):
    """What ``ResidentPredictor.louvain`` returns: the Louvain communities of one batch's kNN graph.  B cells (``index``), K
    communities (``cluster_names``: ``"c0000"``, ... as ``KMeans``), C cell types (``id2label``).  ``cluster`` int64 [B]: a cell's
    community, ids by descending size (ties by the lowest member), -1 for a cell without an edge (a NaN row) - as it stands, with
    ``n_clusters=K``, the ``clusters`` argument of ``annotate`` / ``pseudobulk`` and the ``groups`` of ``rank_genes`` /
    ``silhouette``.  ``size`` int64 [K]; ``modularity``: ``Qnum / (den M^2)`` of the final cut at ``resolution`` (the ``Fraction``
    used); ``weights`` ("snn" | "unit"); ``level_labels``: one int64 [B] per level of the dendrogram (``at_level``), ``levels`` the
    per-level dicts of ``ops.louvain_graph``; ``converged``.  ``space`` / ``metric`` / ``k`` say which graph was cut; ``label``
    int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure).  ``method``: "louvain", or "leiden" for what
    ``ResidentPredictor.leiden`` returns - then every community is connected, ``levels`` are ``ops.leiden_graph``'s dicts,
    ``level_labels`` its moving-phase partitions (and the final cut when it split something) and ``refined_labels`` its refined
    partitions, one int64 [B] per level."""
    cluster: np.ndarray
    size: np.ndarray
    modularity: float
    resolution: object
    weights: str
    levels: Sequence[dict]
    level_labels: Sequence[np.ndarray]
    converged: bool
    k: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)
    method: str = "louvain"
    refined_labels: Optional[Sequence[np.ndarray]] = field(default=None, repr=False)

    def at_level(self, level: int) -> np.ndarray:
        """int64 [B]: the cut after level ``level`` (0 = the finest, -1 = the final one), ids renumbered as ``cluster``'s are - by
        descending size, ties by the lowest member - and -1 where ``cluster`` is."""
        lab = np.asarray(self.level_labels[level], np.int64)
        on = np.asarray(self.cluster, np.int64) >= 0
        out = np.full(lab.shape[0], -1, np.int64)
        if on.any():
            uniq, first, inv, count = np.unique(lab[on], return_index=True, return_inverse=True, return_counts=True)
            rank = np.empty(len(uniq), np.int64)
            rank[np.lexsort((first, -count))] = np.arange(len(uniq))
            out[on] = rank[inv.reshape(-1)]
        return out

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (named as ``predict`` names them), ``cluster`` (its name, ``None``
        without one), and the community's ``cluster_size`` and ``cluster_purity``."""
        names, cl = self.cluster_names, np.asarray(self.cluster, np.int64)
        on, at = cl >= 0, np.maximum(cl, 0)
        size = np.asarray(self.size, np.int64)
        return pd.DataFrame({"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
                             "cluster": [names[k] if k >= 0 else None for k in cl],
                             "cluster_size": np.where(on, size[at], 0) if size.size else np.zeros(len(cl), np.int64),
                             "cluster_purity": np.where(on, self.purity()[at], np.nan) if size.size else np.full(len(cl), np.nan)})

    def summary(self) -> CommunitiesSummary:
        """Cells, communities, levels and sweeps, the modularity, sizes and the purity against ``classify``'s calls; ``print`` it."""
        size, purity = np.asarray(self.size, np.int64), self.purity()
        known = purity[~np.isnan(purity)]
        return CommunitiesSummary(n_cells=len(self.cluster), n_clusters=self.n_clusters, k=int(self.k), space=self.space,
                                  metric=self.metric, weights=self.weights, resolution=str(self.resolution), method=self.method,
                                  converged=bool(self.converged), n_skipped=int((np.asarray(self.cluster) < 0).sum()),
                                  n_levels=len(self.levels), n_sweeps=int(sum(l["sweeps"] for l in self.levels)),
                                  n_fallback=int(sum(l["fallback_moves"] for l in self.levels)), modularity=float(self.modularity),
                                  min_size=int(size.min()) if size.size else 0, max_size=int(size.max()) if size.size else 0,
                                  median_size=float(np.median(size)) if size.size else float("nan"),
                                  median_purity=float(np.median(known)) if known.size else float("nan"),
                                  n_mixed=int((known < 0.9).sum()), n_unsure=int((np.asarray(self.label) < 0).sum()))


class LayoutSummary(dict):
    """``Layout.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells laid out in 2-D from the k = {d['k']} graph in the {d['space']} space ({d['metric']}): "
            f"{d['n_edges']} undirected edges, {d['n_unplaced']} cells without an edge keep their start",
            f"{d['n_epochs']} synchronous epochs from the {d['init']} start, a = {d['a']:.4g}, b = {d['b']:.4g}, seed {d['seed']}; "
            f"{d['n_fired']} edge firings",
            f"x in [{d['x_min']:.4g}, {d['x_max']:.4g}], y in [{d['y_min']:.4g}, {d['y_max']:.4g}]; median sigma {d['median_sigma']:.4g}",
            f"{d['n_types']} called types, median spread around a type's centroid {d['median_spread']:.4g} ({d['n_unsure']} cells unsure)"])


@dataclass
class Layout(_NamesCalls):
    """What ``ResidentPredictor.umap`` returns: a 2-D layout of one batch from the fuzzy graph of its own kNN lists.  B cells
    (``index``), C cell types (``id2label``).  ``coords`` f32 [B, 2]; ``placed`` bool [B]: False for a cell without an edge (a NaN
    row), which keeps its start position; ``rho`` / ``sigma`` f64 [B]: the cell's nearest positive distance and the bandwidth of
    its memberships (``ops.fuzzy_graph``); ``rowptr`` int64 [B + 1] / ``col`` int32 / ``weight`` f32: the symmetric union graph with
    UMAP's connectivities, on the host (``connectivities()``).  ``a`` / ``b``: the curve used; ``n_epochs``, ``n_fired`` (edge
    firings over all epochs), ``seed``, ``init`` ("pca" | "hash" | "array"); ``k`` / ``space`` / ``metric`` say which graph was laid
    out; ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure)."""
    coords: np.ndarray
    placed: np.ndarray
    rho: np.ndarray
    sigma: np.ndarray
    rowptr: np.ndarray
    col: np.ndarray
    weight: np.ndarray
    a: float
    b: float
    n_epochs: int
    n_fired: int
    seed: int
    init: str
    k: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def connectivities(self) -> sp.csr_matrix:
        """CSR ``[B, B]`` float32 of the union graph's weights, symmetric, columns ascending - the layout of
        ``adata.obsp["connectivities"]``."""
        B = len(self.rowptr) - 1
        return sp.csr_matrix((np.asarray(self.weight, np.float32), np.asarray(self.col, np.int32), np.asarray(self.rowptr, np.int64)),
                             shape=(B, B))

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``x``, ``y``, ``label`` (the call's name, as ``predict`` names it) and ``max_prob``."""
        xy = np.asarray(self.coords, np.float32)
        return pd.DataFrame({"index": list(self.index), "x": xy[:, 0], "y": xy[:, 1], "label": self._name(self.label),
                             "max_prob": np.asarray(self.max_prob)})

    def coords_frame(self) -> pd.DataFrame:
        """One row per cell - ``cell`` (its name), ``x`` and ``y``: what ``umap_file`` writes."""
        xy = np.asarray(self.coords, np.float32)
        return pd.DataFrame({"cell": [str(c) for c in self.index], "x": xy[:, 0], "y": xy[:, 1]})

    def by_type(self) -> pd.DataFrame:
        """One row per call (unsure included, last) over the placed cells: ``cell_type``, ``n_cells``, the centroid ``x`` / ``y`` and
        ``spread`` (the root mean squared distance of the type's cells to it)."""
        own, xy = np.asarray(self.label, np.int64), np.asarray(self.coords, np.float64)
        on = np.asarray(self.placed, bool)
        rows = []
        for s in sorted(set(own[on & (own >= 0)].tolist())) + ([-1] if (on & (own < 0)).any() else []):
            m = on & ((own == s) if s >= 0 else (own < 0))
            centre = xy[m].mean(axis=0)
            rows.append((s, int(m.sum()), centre[0], centre[1], float(np.sqrt(((xy[m] - centre) ** 2).sum(axis=1).mean()))))
        cols = list(zip(*rows)) if rows else [[] for _ in range(5)]
        return pd.DataFrame({"cell_type": self._name(cols[0]), "n_cells": np.asarray(cols[1], np.int64),
                             "x": np.asarray(cols[2], np.float64), "y": np.asarray(cols[3], np.float64),
                             "spread": np.asarray(cols[4], np.float64)})

    def summary(self) -> LayoutSummary:
        """Cells, edges, epochs and firings, the extent of the layout and the spread of the called types; ``print`` it."""
        xy, on = np.asarray(self.coords, np.float64), np.asarray(self.placed, bool)
        types = self.by_type()
        if (on & (np.asarray(self.label, np.int64) < 0)).any():                 # the unsure cells' row comes last
            types = types.iloc[:-1]
        ext = lambda v, f: float(f(v)) if len(v) else float("nan")
        sigma = np.asarray(self.sigma, np.float64)[on]
        return LayoutSummary(n_cells=len(xy), k=int(self.k), space=self.space, metric=self.metric, n_edges=int(len(self.col) // 2),
                             n_unplaced=int((~on).sum()), n_epochs=int(self.n_epochs), n_fired=int(self.n_fired), init=self.init,
                             a=float(self.a), b=float(self.b), seed=int(self.seed),
                             x_min=ext(xy[on, 0], np.min), x_max=ext(xy[on, 0], np.max), y_min=ext(xy[on, 1], np.min),
                             y_max=ext(xy[on, 1], np.max), median_sigma=ext(sigma, np.median), n_types=int(len(types)),
                             median_spread=ext(np.asarray(types["spread"]), np.median),
                             n_unsure=int((np.asarray(self.label) < 0).sum()))


class PseudotimeSummary(dict):
    """``Pseudotime.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        how = "converged" if d["converged"] else "NOT converged (stopped at max_rounds)"
        return "\n".join([
            f"{d['n_cells']} cells ordered by geodesic distance on the k = {d['k']} graph in the {d['space']} space ({d['metric']}) "
            f"from {d['n_roots']} root cell(s); {d['n_reached']} reached, {d['n_unreached']} not",
            f"{d['rounds']} rounds, {how}; the farthest cell lies {d['max_distance']:.4g} away over {d['max_hops']} hops "
            f"(median {d['median_distance']:.4g})",
            f"{d['n_types']} called types, earliest {d['first_type']}, latest {d['last_type']} by median pseudotime "
            f"({d['n_unsure']} cells unsure)"])


class _OrderedCells(_NamesCalls):
    """For a result table with ``pseudotime`` f64 [B] (NaN = the cell has none), ``label`` and ``index``: the views by group, by
    called type and per cell that ``Pseudotime`` and ``DiffusionPseudotime`` share."""

    def by_group(self, groups, group_names: Optional[Sequence[str]] = None) -> pd.DataFrame:
        """One row per group of ``groups`` (one integer id per cell, -1 = skip) that has a reached cell, sorted by median
        pseudotime (ties by id): ``group`` (its name from ``group_names``, else the id), ``n_cells`` (reached ones), ``median``,
        ``min`` and ``max`` pseudotime."""
        g, t = np.asarray(groups), np.asarray(self.pseudotime, np.float64)
        if g.shape != t.shape or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"groups must hold one integer id per cell ([{len(t)}]), got {g.dtype} {g.shape}")
        on = (g >= 0) & ~np.isnan(t)
        rows = [(int(s), int((on & (g == s)).sum()), float(np.median(t[on & (g == s)])), float(t[on & (g == s)].min()),
                 float(t[on & (g == s)].max())) for s in sorted(set(g[on].tolist()))]
        rows.sort(key=lambda r: (r[2], r[0]))
        cols = list(zip(*rows)) if rows else [[] for _ in range(5)]
        names = list(cols[0]) if group_names is None else [group_names[s] for s in cols[0]]
        return pd.DataFrame({"group": names, "n_cells": np.asarray(cols[1], np.int64), "median": np.asarray(cols[2], np.float64),
                             "min": np.asarray(cols[3], np.float64), "max": np.asarray(cols[4], np.float64)})

    def by_type(self) -> pd.DataFrame:
        """``by_group`` over the called types (unsure cells skipped): ``cell_type``, ``n_cells``, ``median``, ``min``, ``max``,
        sorted by median pseudotime."""
        label = np.asarray(self.label, np.int64)
        out = self.by_group(np.where(label >= 0, label, -1))
        out["group"] = self._name(out["group"].tolist())
        return out.rename(columns={"group": "cell_type"})

    def pseudotime_frame(self) -> pd.DataFrame:
        """One row per cell - ``cell`` (its name) and ``pseudotime`` (empty where not reached): what ``pseudotime_file`` writes."""
        return pd.DataFrame({"cell": [str(c) for c in self.index], "pseudotime": np.asarray(self.pseudotime, np.float64)})


@dataclass
class Pseudotime(_OrderedCells):
    """What ``ResidentPredictor.pseudotime`` returns: every cell's geodesic distance from the root cells along one batch's own kNN
    graph.  B cells (``index``), C cell types (``id2label``).  ``distance`` f32 [B]: ``ops.geodesic_rows``' bits, the shortest path
    over the union graph's edges in the searched space (+inf = not reached); ``pseudotime`` f64 [B]: ``distance`` over the largest
    finite distance, in [0, 1], NaN where not reached and all 0 when that largest distance is 0; ``pred`` int64 [B]: the
    neighbour the distance came through (-1 = a root or not reached); ``root`` int64: the root cells' positions, ascending;
    ``reached`` (cells with a finite distance), ``rounds`` (Bellman-Ford rounds that changed something) and ``converged`` (False
    when ``max_rounds`` stopped the run early).  ``k`` / ``space`` / ``metric`` say which graph was walked; ``label`` int64 [B] /
    ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure)."""
    distance: np.ndarray
    pseudotime: np.ndarray
    pred: np.ndarray
    root: np.ndarray
    reached: int
    rounds: int
    converged: bool
    k: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def hops(self) -> np.ndarray:
        """int64 [B]: the number of edges on the cell's path from its root (0 at a root, -1 where not reached), by pointer
        jumping on ``pred`` - ``ceil(log2(longest path))`` passes."""
        pred = np.asarray(self.pred, np.int64)
        B = len(pred)
        hops = (pred >= 0).astype(np.int64)
        up = np.where(pred >= 0, pred, np.arange(B))
        for _ in range(max(1, B).bit_length() + 1):
            if not (hops[up] > 0).any():
                break
            hops, up = hops + hops[up], up[up]
        hops[~np.isfinite(np.asarray(self.distance, np.float64))] = -1
        return hops

    def path(self, cell: int) -> np.ndarray:
        """int64: the positions from a root to ``cell`` along ``pred``, both included; empty where the cell was not reached."""
        pred, cell = np.asarray(self.pred, np.int64), int(cell)
        if not 0 <= cell < len(pred):
            raise ValueError(f"cell = {cell} is outside [0, {len(pred)})")
        if not np.isfinite(float(np.asarray(self.distance)[cell])):
            return np.zeros(0, np.int64)
        out = [cell]
        while pred[out[-1]] >= 0 and len(out) <= len(pred):
            out.append(int(pred[out[-1]]))
        return np.asarray(out[::-1], np.int64)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``pseudotime``, ``distance``, ``pred``, ``label`` (the call's name, as ``predict`` names
        it) and ``max_prob``."""
        return pd.DataFrame({"index": list(self.index), "pseudotime": np.asarray(self.pseudotime, np.float64),
                             "distance": np.asarray(self.distance, np.float32), "pred": np.asarray(self.pred, np.int64),
                             "label": self._name(self.label), "max_prob": np.asarray(self.max_prob)})

    def summary(self) -> PseudotimeSummary:
        """Cells, roots, rounds, the farthest cell and the earliest and latest called type; ``print`` it."""
        d = np.asarray(self.distance, np.float64)
        fin = d[np.isfinite(d)]
        types, hops = self.by_type(), self.hops()
        return PseudotimeSummary(n_cells=len(d), k=int(self.k), space=self.space, metric=self.metric, n_roots=len(self.root),
                                 n_reached=int(self.reached), n_unreached=len(d) - int(self.reached), rounds=int(self.rounds),
                                 converged=bool(self.converged), max_distance=float(fin.max()) if fin.size else float("nan"),
                                 median_distance=float(np.median(fin)) if fin.size else float("nan"),
                                 max_hops=int(hops.max()) if hops.size else 0, n_types=len(types),
                                 first_type=types["cell_type"].iloc[0] if len(types) else None,
                                 last_type=types["cell_type"].iloc[-1] if len(types) else None,
                                 n_unsure=int((np.asarray(self.label) < 0).sum()))


def _scaled_pseudotime(distance) -> np.ndarray:
    """``Pseudotime.pseudotime`` of ``distance``: float64, over the largest finite distance; NaN where not reached, all 0 when that
    largest distance is 0."""
    d = np.asarray(distance, np.float32).astype(np.float64)
    fin = np.isfinite(d)
    top = d[fin].max() if fin.any() else 0.0
    out = np.where(fin, d / top if top > 0 else 0.0, np.nan)
    return out


def _paga_connectivities(edges, size) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(out_edges int64 [K], expected f64 [K, K], connectivities f64 [K, K])`` of ``ops.group_edges``' tables, the PAGA
    connectivity (Wolf et al. 2019) on the unit-weight directed kNN graph: with ``es[a] = sum_b edges[a, b]``, ``n = sum size``
    and ``inter[a, b] = edges[a, b] + edges[b, a]`` for ``a != b``, ``den = es[a] size[b] + es[b] size[a]``, ``expected = den /
    (n - 1)`` (one fp64 division of integers) and the connectivity 0 where ``inter == 0``, 1 where ``inter (n - 1) >= den`` (an
    integer comparison), else ``float64(inter (n - 1)) / float64(den)``.  Symmetric, zero diagonal."""
    e, ns = np.asarray(edges, np.int64), np.asarray(size, np.int64)
    K = len(ns)
    if e.shape != (K, K) or (e < 0).any() or (ns < 0).any():
        raise ValueError(f"edges must be a non-negative [{K}, {K}] table beside size [{K}]")
    es, n = e.sum(axis=1), int(ns.sum())
    if int(e.sum()) * max(n, 1) >= 2 ** 62:
        raise ValueError("the PAGA tables would not fit 64-bit integers")
    inter = e + e.T
    np.fill_diagonal(inter, 0)
    den = es[:, None] * ns[None, :] + es[None, :] * ns[:, None]
    np.fill_diagonal(den, 0)
    num = inter * (n - 1)
    expected = np.zeros((K, K), np.float64)
    conn = np.zeros((K, K), np.float64)
    if n > 1:
        expected = den.astype(np.float64) / np.float64(n - 1)
        part = (inter > 0) & (num < den)
        conn[(inter > 0) & (num >= den)] = 1.0
        conn[part] = num[part].astype(np.float64) / den[part].astype(np.float64)
    return es, expected, conn


class AbstractionSummary(dict):
    """``Abstraction.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells in {d['n_groups']} non-empty groups on the k = {d['k']} graph in the {d['space']} space "
            f"({d['metric']}); {d['n_skipped']} cells take no part",
            f"{d['n_edges']} list entries between participating cells, {d['n_within']} inside a group; {d['n_pairs']} pairs of groups "
            f"share an edge, {d['n_tree_edges']} of them on the spanning forest ({d['n_components']} components)",
            f"strongest pair {d['top_pair']} (connectivity {d['top_connectivity']:.4f}); median connectivity of the connected pairs "
            f"{d['median_connectivity']:.4f}"])


@dataclass
class Abstraction:
    """What ``ResidentPredictor.paga`` returns: how the groups of one batch hang together on its own kNN graph - the PAGA
    connectivity (Wolf et al. 2019) on the unit-weight directed graph.  K groups (``group_names``).  ``edges`` int64 [K, K]: the
    list entries from a cell of group a to a cell of group b; ``size`` int64 [K]: the participating cells; ``out_edges`` int64
    [K]: ``edges``' row sums; ``expected`` f64 [K, K]: the entries a random wiring of the same out-degrees would put between the
    pair; ``connectivities`` f64 [K, K]: the observed over the expected, capped at 1 - symmetric, zero diagonal
    (``tables._paga_connectivities`` has the formula).  ``n_skipped``: the cells that take no part; ``group`` int64 [B]: every cell's
    group as the call resolved it (-1 = it takes no part); ``k`` / ``space`` / ``metric`` say which graph was counted."""
    edges: np.ndarray
    size: np.ndarray
    out_edges: np.ndarray
    connectivities: np.ndarray
    expected: np.ndarray
    group_names: Sequence[str]
    n_skipped: int
    group: Optional[np.ndarray] = field(default=None, repr=False)
    k: int = 0
    space: str = ""
    metric: str = ""

    def _inter(self) -> np.ndarray:
        e = np.asarray(self.edges, np.int64)
        inter = e + e.T
        np.fill_diagonal(inter, 0)
        return inter

    def tree(self) -> np.ndarray:
        """int64 [K, K], symmetric 0 / 1: the maximum spanning forest of ``connectivities`` - scipy's
        ``minimum_spanning_tree`` on ``1 / connectivities`` of the non-zero entries - the backbone PAGA draws."""
        from scipy.sparse.csgraph import minimum_spanning_tree
        c = np.asarray(self.connectivities, np.float64)
        a, b = np.nonzero(np.triu(c, 1))
        K = c.shape[0]
        forest = minimum_spanning_tree(sp.csr_matrix((1.0 / c[a, b], (a, b)), shape=(K, K))).tocoo()
        out = np.zeros((K, K), np.int64)
        out[forest.row, forest.col] = 1
        out[forest.col, forest.row] = 1
        return out

    def frame(self, min_connectivity: float = 0.0) -> pd.DataFrame:
        """One row per unordered pair of groups that share a list entry (``a`` before ``b`` in ``group_names``' order) with
        ``connectivity >= min_connectivity``: ``a``, ``b``, ``edges`` (both directions), ``expected``, ``connectivity``,
        ``in_tree``."""
        inter, c = self._inter(), np.asarray(self.connectivities, np.float64)
        a, b = np.nonzero(np.triu(inter, 1))
        keep = c[a, b] >= float(min_connectivity)
        a, b = a[keep], b[keep]
        names = list(self.group_names)
        return pd.DataFrame({"a": [names[i] for i in a], "b": [names[i] for i in b], "edges": inter[a, b],
                             "expected": np.asarray(self.expected, np.float64)[a, b], "connectivity": c[a, b],
                             "in_tree": self.tree()[a, b].astype(bool)})

    def _cells(self, what, shape) -> np.ndarray:
        if self.group is None:
            raise ValueError(f"{what} needs the cells' groups: this table was built without ``group``")
        g = np.asarray(self.group, np.int64)
        if g.shape != tuple(shape):
            raise ValueError(f"{what}: the table holds {len(g)} cells, got {tuple(shape)}")
        return g

    def centroids(self, coords) -> np.ndarray:
        """f64 [K, 2]: the mean of ``coords`` ([B, 2], a ``Layout.coords`` of the same batch) over the cells of every group - where
        to draw the groups on the UMAP; NaN for an empty group."""
        xy = np.asarray(coords, np.float64)
        K = len(self.group_names)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"coords must be [B, 2], got {xy.shape}")
        g = self._cells("centroids", xy.shape[:1])
        on = g >= 0
        count = np.bincount(g[on], minlength=K).astype(np.float64)
        out = np.stack([np.bincount(g[on], weights=xy[on, j], minlength=K) for j in range(2)], axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return out / count[:, None]

    def directed(self, pseudotime) -> pd.DataFrame:
        """``frame()`` with every pair oriented in time: ``a`` is the group of lower median pseudotime (``pseudotime``: a
        ``Pseudotime`` of the same batch, or one value per cell; ties and groups without a reached cell keep ``group_names``'
        order), with ``median_a`` / ``median_b`` added."""
        t = np.asarray(getattr(pseudotime, "pseudotime", pseudotime), np.float64)
        g = self._cells("directed", t.shape)
        names = list(self.group_names)
        med = {names[s]: float(np.median(t[(g == s) & ~np.isnan(t)])) for s in range(len(names)) if ((g == s) & ~np.isnan(t)).any()}
        out = self.frame()
        ma = np.asarray([med.get(x, np.nan) for x in out["a"]], np.float64)
        mb = np.asarray([med.get(x, np.nan) for x in out["b"]], np.float64)
        flip = mb < ma
        a, b = out["a"].to_numpy(object), out["b"].to_numpy(object)
        out["a"], out["b"] = np.where(flip, b, a), np.where(flip, a, b)
        out["median_a"], out["median_b"] = np.where(flip, mb, ma), np.where(flip, ma, mb)
        return out

    def summary(self) -> AbstractionSummary:
        """Cells, groups, edges, the connected pairs, the spanning forest and the strongest pair; ``print`` it."""
        from scipy.sparse.csgraph import connected_components
        e, ns, per = np.asarray(self.edges, np.int64), np.asarray(self.size, np.int64), self.frame()
        live = ns > 0
        n_comp = int(connected_components(sp.csr_matrix(self._inter()[live][:, live] > 0), directed=False)[0]) if live.any() else 0
        top = per.iloc[int(np.argmax(per["connectivity"].to_numpy()))] if len(per) else None
        return AbstractionSummary(n_cells=int(ns.sum()), n_groups=int(live.sum()), k=int(self.k), space=self.space, metric=self.metric,
                                  n_skipped=int(self.n_skipped), n_edges=int(e.sum()), n_within=int(np.trace(e)), n_pairs=len(per),
                                  n_tree_edges=int(per["in_tree"].sum()) if len(per) else 0, n_components=n_comp,
                                  top_pair=None if top is None else (top["a"], top["b"]),
                                  top_connectivity=float("nan") if top is None else float(top["connectivity"]),
                                  median_connectivity=float(np.median(per["connectivity"])) if len(per) else float("nan"))


class DiffusionMapSummary(dict):
    """``DiffusionMap.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        how = "converged" if d["converged"] else f"NOT converged (largest residual {d['max_residual']:.3g} > tol {d['tol']:.3g}: raise n_steps)"
        return "\n".join([
            f"{d['n_cells']} cells, k = {d['k']} graph in the {d['space']} space ({d['metric']}): {d['n_components']} connected "
            f"components, the largest holds {d['n_in_component']} cells ({d['n_outside']} outside have no coordinates)",
            f"{d['n_found']} diffusion components from {d['n_steps']} Lanczos steps (seed {d['seed']}"
            f"{', breakdown: the Krylov space is exhausted' if d['breakdown'] else ''}), {how}",
            f"eigenvalues 1, {d['second']:.6g} ... {d['last']:.6g}; gap after the stationary one {d['gap']:.4g}",
            f"{d['n_types']} called types in the component ({d['n_unsure']} cells unsure)"])


@dataclass
class DiffusionMap(_NamesCalls):
    """What ``ResidentPredictor.diffmap`` returns: the diffusion map of the largest connected component of one batch's own kNN
    graph.  B cells (``index``), C cell types (``id2label``).  ``coords`` f64 [B, n_found]: the leading eigenvectors of the
    density-normalised symmetric transition matrix, unit length, column 0 the stationary one - scanpy's ``X_diffmap`` - NaN in
    the rows of cells outside the component; ``eigenvalues`` f64 [n_found], descending, ``eigenvalues[0] == 1``; ``residual`` f64
    [n_found]: the Lanczos estimate ``|beta_m s_mc|`` of ``||T y - lambda y||`` per component (0 for the stationary one, which is
    known and not searched for); ``converged``: every residual is at most ``tol``; ``n_steps``: the Lanczos steps actually run;
    ``breakdown``: the run ended because a step left no new direction (always on a component of fewer than ``n_steps + 2``
    cells); ``in_component`` bool [B]; ``n_components``: the graph's connected components, single cells included; ``seed``.
    ``n_found`` can be below the ``n_comps`` asked for: a small component, or a breakdown.  ``k`` / ``space`` / ``metric`` say
    which graph it was; ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure)."""
    coords: np.ndarray
    eigenvalues: np.ndarray
    residual: np.ndarray
    converged: bool
    tol: float
    n_steps: int
    breakdown: bool
    in_component: np.ndarray
    n_components: int
    seed: int
    k: int
    space: str
    metric: str
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    @property
    def n_found(self) -> int:
        return int(np.asarray(self.coords).shape[1])

    def spectral_init(self) -> np.ndarray:
        """f32 [B, 2]: components 1 and 2 scaled to max-abs 10, zero rows outside the component (and a zero column where the
        component was not found) - a start for ``umap(init=...)`` as it stands."""
        xy = np.zeros((len(self.in_component), 2), np.float64)
        have = min(2, self.n_found - 1)
        xy[:, :have] = np.nan_to_num(np.asarray(self.coords, np.float64)[:, 1:1 + have], nan=0.0)
        top = np.abs(xy).max() if xy.size else 0.0
        return (xy * (10.0 / top) if top > 0 else xy).astype(np.float32)

    def coords_frame(self) -> pd.DataFrame:
        """One row per cell - ``cell`` (its name), ``dc1``, ``dc2``, ... (column 0, the stationary component, is left out; empty
        outside the component): what ``diffmap_file`` writes."""
        y = np.asarray(self.coords, np.float64)
        return pd.DataFrame({"cell": [str(c) for c in self.index], **{f"dc{c}": y[:, c] for c in range(1, y.shape[1])}})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``in_component``, ``dc1``, ``dc2``, ..., ``label`` (the call's name, as ``predict`` names
        it) and ``max_prob``."""
        y = np.asarray(self.coords, np.float64)
        return pd.DataFrame({"index": list(self.index), "in_component": np.asarray(self.in_component, bool),
                             **{f"dc{c}": y[:, c] for c in range(1, y.shape[1])}, "label": self._name(self.label),
                             "max_prob": np.asarray(self.max_prob)})

    def by_type(self) -> pd.DataFrame:
        """One row per call (unsure included, last) over the cells of the component: ``cell_type``, ``n_cells`` and the type's
        mean ``dc1``, ``dc2``, ..."""
        own, y, on = np.asarray(self.label, np.int64), np.asarray(self.coords, np.float64), np.asarray(self.in_component, bool)
        ids = sorted(set(own[on & (own >= 0)].tolist())) + ([-1] if (on & (own < 0)).any() else [])
        members = [on & ((own == s) if s >= 0 else (own < 0)) for s in ids]
        out = pd.DataFrame({"cell_type": self._name(ids), "n_cells": np.asarray([int(m.sum()) for m in members], np.int64)})
        for c in range(1, y.shape[1]):
            out[f"dc{c}"] = np.asarray([y[m, c].mean() for m in members], np.float64)
        return out

    def summary(self) -> DiffusionMapSummary:
        """Cells, components, steps, convergence and the leading eigenvalues; ``print`` it."""
        lam, res, on = np.asarray(self.eigenvalues, np.float64), np.asarray(self.residual, np.float64), np.asarray(self.in_component, bool)
        own = np.asarray(self.label, np.int64)
        at = lambda i: float(lam[i]) if -len(lam) <= i < len(lam) and len(lam) > 1 else float("nan")
        return DiffusionMapSummary(n_cells=len(on), k=int(self.k), space=self.space, metric=self.metric,
                                   n_components=int(self.n_components), n_in_component=int(on.sum()), n_outside=int((~on).sum()),
                                   n_found=self.n_found, n_steps=int(self.n_steps), seed=int(self.seed), breakdown=bool(self.breakdown),
                                   converged=bool(self.converged), tol=float(self.tol),
                                   max_residual=float(res.max()) if res.size else 0.0, second=at(1), last=at(-1),
                                   gap=1.0 - at(1), n_types=len(set(own[on & (own >= 0)].tolist())),
                                   n_unsure=int((own < 0).sum()))


class DiffusionPseudotimeSummary(dict):
    """``DiffusionPseudotime.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        return "\n".join([
            f"{d['n_cells']} cells ordered by diffusion distance over {d['n_dcs']} diffusion components from {d['n_roots']} root "
            f"cell(s); {d['n_ordered']} in the component, {d['n_outside']} outside it have none",
            f"the farthest cell lies {d['max_distance']:.4g} away (median {d['median_distance']:.4g})",
            f"{d['n_types']} called types, earliest {d['first_type']}, latest {d['last_type']} by median pseudotime "
            f"({d['n_unsure']} cells unsure)"])


@dataclass
class DiffusionPseudotime(_OrderedCells):
    """What ``ResidentPredictor.dpt`` returns: every cell's diffusion distance from the root cells.  B cells (``index``), C cell
    types (``id2label``).  ``distance`` f64 [B]: ``ops.diffusion_distance``' bits - ``sqrt(sum_l (lambda_l / (1 - lambda_l))^2
    (y_l[root] - y_l[cell])^2)`` over the components ``l = 1 .. n_dcs - 1``, to the nearest root - NaN for a cell outside the
    component; ``pseudotime`` f64 [B]: ``distance`` over the largest one, in [0, 1], NaN outside the component (``Pseudotime``'s
    scaling); ``roots`` int64: the root cells' positions, ascending; ``n_dcs``: the diffusion components used, the stationary one
    counted; ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch (-1 = unsure).  ``by_group``,
    ``by_type`` and ``pseudotime_frame`` are ``Pseudotime``'s, and ``Abstraction.directed`` takes the table as it stands."""
    distance: np.ndarray
    pseudotime: np.ndarray
    roots: np.ndarray
    n_dcs: int
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``pseudotime``, ``distance``, ``label`` (the call's name, as ``predict`` names it) and
        ``max_prob``."""
        return pd.DataFrame({"index": list(self.index), "pseudotime": np.asarray(self.pseudotime, np.float64),
                             "distance": np.asarray(self.distance, np.float64), "label": self._name(self.label),
                             "max_prob": np.asarray(self.max_prob)})

    def summary(self) -> DiffusionPseudotimeSummary:
        """Cells, roots, the farthest cell and the earliest and latest called type; ``print`` it."""
        d = np.asarray(self.distance, np.float64)
        fin = d[np.isfinite(d)]
        types = self.by_type()
        return DiffusionPseudotimeSummary(n_cells=len(d), n_dcs=int(self.n_dcs), n_roots=len(self.roots), n_ordered=int(fin.size),
                                          n_outside=len(d) - int(fin.size), max_distance=float(fin.max()) if fin.size else float("nan"),
                                          median_distance=float(np.median(fin)) if fin.size else float("nan"), n_types=len(types),
                                          first_type=types["cell_type"].iloc[0] if len(types) else None,
                                          last_type=types["cell_type"].iloc[-1] if len(types) else None,
                                          n_unsure=int((np.asarray(self.label) < 0).sum()))


@dataclass(kw_only=True)
class HarmonizedGraph(NeighborGraph):
    """The kNN graph of a cohort's unit rows, before or after ``ResidentPredictor.harmony`` corrected them.  It IS a
    ``NeighborGraph`` (``metric="cosine"``) - what every ``graph=`` argument reads - that also knows the cells' batches:
    ``batch`` int64 [B], ``batch_names`` the S names, and ``lisi("batch")`` is the mixing of the samples on it."""
    batch: np.ndarray
    batch_names: Sequence[str]

    def _named_labels(self, name: str) -> np.ndarray:
        if name == "batch":
            return np.asarray(self.batch, np.int64)
        return super()._named_labels(name)


class HarmonizedSummary(dict):
    """``Harmonized.summary()``: a dict that prints as a few lines."""

    def __str__(self) -> str:
        d = self
        how = f"converged after {d['n_iter']} rounds" if d["converged"] else f"NOT converged after {d['n_iter']} rounds"
        sizes = ", ".join(f"{name}: {n}" for name, n in d["batch_sizes"].items())
        lines = [f"{d['n_cells']} cells of {d['n_batches']} batches ({sizes}) in the {d['space']} space, {d['n_clusters']} soft "
                 f"clusters, {how}; objective {d['objective_first']:.6g} -> {d['objective_last']:.6g}",
                 f"median shift {d['median_shift']:.4g} (median row length {d['median_norm']:.4g})"]
        if d["batch_lisi_after"] is not None:
            before = lambda v: "not compared" if v is None else f"{v:.3f}"
            lines.append(f"median batch LISI {before(d['batch_lisi_before'])} -> {d['batch_lisi_after']:.3f}, median type LISI "
                         f"{before(d['type_lisi_before'])} -> {d['type_lisi_after']:.3f} (k = {d['k']})")
            if d["type_lisi_before"] is not None and d["type_lisi_after"] > d["type_lisi_before"]:
                lines.append("WARNING: the predicted-type LISI rose - the correction mixed cell types as well as batches")
        return "\n".join(lines)


@dataclass
class Harmonized(_NamesCalls):
    """What ``ResidentPredictor.harmony`` returns: the batch-corrected embedding of one cohort (Harmony, Korsunsky et al. 2019).
    B cells (``index``), D columns, K soft clusters, S batches (``batch_names``), C cell types (``id2label``).  ``coords`` f32
    [B, D]: the corrected rows - ``ops.kmeans_rows`` / ``ops.knn_rows`` take them as they are; ``embedding`` f32 [B, D]: the rows
    before; ``cluster_prob`` f64 [B, K]: Harmony's soft memberships ``R`` and ``cluster`` int64 [B] their argmax; ``centers`` f64
    [K, D]: the unit centres; ``batch`` int64 [B]; ``objective``: one value per round (the seeding's first); ``n_iter`` /
    ``converged``: ``ops.harmony_rows``'; ``label`` int64 [B] / ``max_prob`` f32 [B]: ``classify``'s call of the batch, made on
    the uncorrected input (-1 = unsure).  ``graph`` / ``graph_before``: the kNN graphs (``HarmonizedGraph``, cosine, ``k``
    neighbours) of the corrected and of the uncorrected unit rows, ``None`` where the call skipped them.  With a single batch
    nothing is corrected: ``coords`` equals ``embedding``, ``cluster_prob`` / ``centers`` are empty and ``cluster`` is 0."""
    coords: np.ndarray
    embedding: np.ndarray
    cluster_prob: np.ndarray
    cluster: np.ndarray
    centers: np.ndarray
    batch: np.ndarray
    batch_names: Sequence[str]
    objective: Sequence[float]
    n_iter: int
    converged: bool
    space: str
    graph: Optional[HarmonizedGraph]
    graph_before: Optional[HarmonizedGraph]
    label: np.ndarray
    max_prob: np.ndarray
    index: Sequence
    id2label: Sequence[str]
    label_map: Optional[Tuple[dict, dict]] = field(default=None, repr=False)

    def shift(self) -> np.ndarray:
        """f64 [B]: the length of each cell's correction, ``|coords - embedding|``."""
        return np.sqrt(((np.asarray(self.coords, np.float64) - np.asarray(self.embedding, np.float64)) ** 2).sum(axis=1))

    def mixing(self) -> pd.DataFrame:
        """One row per cell: ``batch_lisi_before`` / ``batch_lisi_after`` - ``NeighborGraph.lisi`` of the batch ids on
        ``graph_before`` / ``graph`` - and ``type_lisi_before`` / ``type_lisi_after``, the same of ``classify``'s calls.  A
        correction that works raises the first pair and leaves the second where it was.  NaN columns where a graph was skipped;
        without ``graph`` it raises ``ValueError``."""
        if self.graph is None:
            raise ValueError("mixing needs the graph of the corrected rows: call harmony with k, not k=None")
        B = len(self.batch)
        nan = np.full(B, np.nan)
        lisi = lambda g, what: nan if g is None else g.lisi(what, n_labels=len(self.batch_names) if what == "batch" else len(self.id2label))
        return pd.DataFrame({"index": list(self.index),
                             "batch_lisi_before": lisi(self.graph_before, "batch"), "batch_lisi_after": lisi(self.graph, "batch"),
                             "type_lisi_before": lisi(self.graph_before, "predicted"),
                             "type_lisi_after": lisi(self.graph, "predicted")})

    def by_batch(self) -> pd.DataFrame:
        """One row per batch: ``batch``, ``n_cells`` and ``median_shift``, the median length of its cells' corrections (NaN for
        an empty batch)."""
        own, shift = np.asarray(self.batch, np.int64), self.shift()
        names = list(self.batch_names)
        return pd.DataFrame({"batch": names, "n_cells": np.asarray([(own == s).sum() for s in range(len(names))], np.int64),
                             "median_shift": np.asarray([np.median(shift[own == s]) if (own == s).any() else np.nan
                                                         for s in range(len(names))], np.float64)})

    def frame(self) -> pd.DataFrame:
        """One row per cell: ``index``, ``cell_type`` / ``prob`` (named as ``predict`` names them), ``batch`` (its name),
        ``cluster`` and ``cluster_prob`` (the largest membership), ``shift``, then the corrected coordinates ``h1`` .. ``hD``."""
        coords, prob = np.asarray(self.coords, np.float32), np.asarray(self.cluster_prob, np.float64)
        out = {"index": list(self.index), "cell_type": self._name(self.label), "prob": np.asarray(self.max_prob),
               "batch": [self.batch_names[s] for s in np.asarray(self.batch, np.int64)],
               "cluster": np.asarray(self.cluster, np.int64),
               "cluster_prob": prob.max(axis=1) if prob.shape[1] else np.ones(len(self.batch)), "shift": self.shift()}
        out.update({f"h{j + 1}": coords[:, j] for j in range(coords.shape[1])})
        return pd.DataFrame(out)

    def summary(self) -> HarmonizedSummary:
        """Cells, batches, rounds, the objective, the median shift and - where the graphs were built - the median batch and
        predicted-type LISI before -> after, with a warning line when the type LISI rises; ``print`` it."""
        own = np.asarray(self.batch, np.int64)
        med = lambda v: None if np.isnan(v).all() else float(np.nanmedian(v))
        mix = self.mixing() if self.graph is not None else None
        get = lambda col: None if mix is None else med(mix[col].to_numpy())
        objective = list(self.objective) or [float("nan")]
        return HarmonizedSummary(
            n_cells=len(own), n_batches=len(self.batch_names), space=self.space,
            batch_sizes={str(name): int((own == s).sum()) for s, name in enumerate(self.batch_names)},
            n_clusters=int(np.asarray(self.cluster_prob).shape[1]), n_iter=int(self.n_iter), converged=bool(self.converged),
            objective_first=float(objective[0]), objective_last=float(objective[-1]),
            median_shift=float(np.median(self.shift())) if len(own) else float("nan"),
            median_norm=float(np.median(np.sqrt((np.asarray(self.embedding, np.float64) ** 2).sum(axis=1)))) if len(own) else float("nan"),
            k=None if self.graph is None else int(self.graph.k),
            batch_lisi_before=get("batch_lisi_before"), batch_lisi_after=get("batch_lisi_after"),
            type_lisi_before=get("type_lisi_before"), type_lisi_after=get("type_lisi_after"))
