"""Thin counterparts of the documented ``deepsort`` package classes (reference ``docs/api.rst:6-130``), whose
source is not in the reference tree; the tree holds the equivalent CLI classes ``Trainer`` (``train.py:16-123``)
and ``Runner`` (``predict.py:17-152``).  Same constructor keywords, same ``fit`` / ``predict`` signatures, same
bundle on disk (``{species}-{tissue}.pt`` = ``{'model', 'optimizer'}`` (train.py:117-123), ``{tissue}_genes.txt`` /
``{tissue}_cell_type.txt`` written with ``\\r\\n`` (preprocess_internal.py:59-67), ``{species}_{tissue}_data.npz``
support matrix (preprocess_internal.py:180)), read and written either as the reference's
``pretrained/{species}/{models,graphs,statistics}/`` tree or as one flat directory (:class:`BundlePaths`).

Only the per-cell hot path (graph normalisation, aggregation, autograd) runs on the GPU through the HIP
kernels; file ingest, vocabularies and PCA are ordinary host code kept deliberately small.
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from ._lib import WgnnError
from .gnn import GNN
from .graph import CellGeneGraph
from . import ops as _ops
from . import tables as _tables
from .ops import cross_entropy_sum
# the result tables and the host helpers they share with the predictor: every name of tables.py is reachable through this module
from .tables import (Ambient, AmbientSummary, Attribution, BatchGraph, BatchGraphSummary, ClusterCalls, Communities, CommunitiesSummary, Coverage, CoverageSummary, Doublets, DoubletsSummary,
                     GeneRanks, GeneRanksSummary, KMeans, KMeansSummary, Layout, LayoutSummary, MarkerTable, NeighborGraph, NeighborGraphSummary, PanelCalls, PanelSummary,
                     Pseudobulk, PseudobulkSummary, SignatureScores, SignatureSummary, Silhouette, SilhouetteSummary, Smoothed, SmoothedSummary, Stability,
                     StabilitySummary, KNN_METRICS, KNN_SPACES, SMOOTH_MAX_NEIGHBORS, _NamesCalls, _benjamini_hochberg, _call_names, _check_index, _cluster_ids, _keep_levels,
                     _neighbor_lists, _rank_genes_stats, _rho_levels, _signature_scores,
                     Abstraction, AbstractionSummary, Pseudotime, PseudotimeSummary, _paga_connectivities, _scaled_pseudotime,
                     DiffusionMap, DiffusionMapSummary, DiffusionPseudotime, DiffusionPseudotimeSummary,
                     Harmonized, HarmonizedGraph, HarmonizedSummary)

_tables._rows_topk = lambda *a: _ops.rows_topk(*a)      # MarkerTable.top's device route: tables.py itself imports no ops


def _device(gpu_id: int) -> torch.device:
    if not torch.cuda.is_available():
        raise WgnnError("the MI355X path needs a GPU (gpu_id=-1 meant CPU in the reference; there is no CPU fallback here)")
    # ``fit`` / ``_predict`` run under ``torch.cuda.device(dev)`` (restored on exit): C-ABI calls are guarded per call by
    # ``_lib.call``, but hipGraph capture (GraphedTrainStep / GraphedForward) opens its stream on the CURRENT device
    return torch.device("cuda", max(gpu_id, 0))


def _read_expression(path, file_type: str) -> pd.DataFrame:
    """(genes x cells) table as produced by pre-process.R:72-74 -> DataFrame (cells x genes)."""
    if file_type == "csv":
        df = pd.read_csv(path, index_col=0)
    elif file_type == "gz":
        df = pd.read_csv(path, compression="gzip", index_col=0)
    else:
        raise ValueError(f"Not supported type {file_type!r}: csv or gz")
    return df.transpose(copy=True)


def _gene_features(expr: sp.csr_matrix, n_support: int, dense_dim: int, seed, device) -> torch.Tensor:
    """gene_feat = PCA(dense_dim) of the support cells' (genes x cells) matrix (host, sklearn, like the reference,
    preprocess.py:194-196); the support cells are the first ``n_support`` rows of ``expr``."""
    from sklearn.decomposition import PCA
    dense_sup = expr[:n_support].toarray().astype(np.float64)
    k = min(dense_dim, dense_sup.shape[1], n_support)
    gene_feat = PCA(k, random_state=seed).fit_transform(dense_sup.T)
    if k < dense_dim:
        gene_feat = np.pad(gene_feat, ((0, 0), (0, dense_dim - k)))
    return torch.from_numpy(gene_feat.astype(np.float32)).to(device)


def _cell_features(expr: sp.csr_matrix, gf: torch.Tensor, device) -> torch.Tensor:
    """cell_feat = rownorm(X) . gene_feat on the device through K1 (preprocess_internal.py:197-202, preprocess.py:201-210)."""
    return CellGeneGraph.cell_features(torch.from_numpy(expr.indptr.astype(np.int64)).to(device),
                                       torch.from_numpy(expr.indices.astype(np.int32)).to(device),
                                       torch.from_numpy(expr.data.astype(np.float32)).to(device), gf)


def _features(expr: sp.csr_matrix, n_support: int, dense_dim: int, seed, device) -> torch.Tensor:
    """[gene_feat; cell_feat] (preprocess_internal.py:183-202, preprocess.py:194-210)."""
    gf = _gene_features(expr, n_support, dense_dim, seed, device)
    return torch.cat([gf, _cell_features(expr, gf, device)])


def read_xlsx_sheet(path, sheet_name: Optional[str]) -> List[List[Optional[str]]]:
    """Rows of one worksheet of an .xlsx workbook as lists of strings (None = empty cell).  A minimal reader (zip + XML,
    shared and inline strings, plain numbers) for ``map/celltype2subtype.xlsx`` (predict.py:125-128): neither xlrd nor
    openpyxl is a dependency here.  ``sheet_name=None``: the first sheet (pandas.read_excel's default)."""
    import re
    import zipfile
    import xml.etree.ElementTree as ET
    ns = {"m": "http://schemas.openxmlformats.org/spreadsheetml/2006/main",
          "r": "http://schemas.openxmlformats.org/officeDocument/2006/relationships"}
    with zipfile.ZipFile(path) as z:
        wb = ET.fromstring(z.read("xl/workbook.xml"))
        rid = None
        for sh in wb.find("m:sheets", ns):
            if sh.get("name") == sheet_name or (sheet_name is None and rid is None):
                rid = sh.get(f"{{{ns['r']}}}id")
        if rid is None:
            raise KeyError(f"no sheet {sheet_name!r} in {path}")
        rels = ET.fromstring(z.read("xl/_rels/workbook.xml.rels"))
        target = next(r.get("Target") for r in rels if r.get("Id") == rid)
        target = target.lstrip("/")
        target = target if target.startswith("xl/") else "xl/" + target
        shared: List[str] = []
        if "xl/sharedStrings.xml" in z.namelist():
            for si in ET.fromstring(z.read("xl/sharedStrings.xml")).findall("m:si", ns):
                shared.append("".join(t.text or "" for t in si.iter(f"{{{ns['m']}}}t")))
        rows: List[List[Optional[str]]] = []
        for row in ET.fromstring(z.read(target)).find("m:sheetData", ns).findall("m:row", ns):
            cells: List[Optional[str]] = []
            for c in row.findall("m:c", ns):
                letters = re.match(r"[A-Z]+", c.get("r", "A")).group(0)
                col = 0
                for ch in letters:
                    col = col * 26 + ord(ch) - 64
                while len(cells) < col:
                    cells.append(None)
                v, t = c.find("m:v", ns), c.get("t")
                if t == "s" and v is not None:
                    val = shared[int(v.text)]
                elif t == "inlineStr":
                    val = "".join(x.text or "" for x in c.iter(f"{{{ns['m']}}}t"))
                else:
                    val = v.text if v is not None else None
                cells[col - 1] = val
            rows.append(cells)
        return rows


_PANDAS_NA = {"", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
              "NULL", "NaN", "None", "n/a", "nan", "null"}


def load_label_map(path, species: str) -> Tuple[dict, dict]:
    """old cell type -> (new type, new subtype) from the ``species`` sheet of celltype2subtype.xlsx; empty cells become
    'N/A' (predict.py:125-133)."""
    old2new, old2sub = {}, {}
    for row in read_xlsx_sheet(path, species)[1:]:                     # header=0
        row = (row + [None] * 4)[:4]
        # pandas.read_excel parses its default NA strings as NaN, which the reference then fills with 'N/A'
        _, old, new, sub = [("N/A" if x is None or x in _PANDAS_NA else x) for x in row]
        old2new[old], old2sub[old] = new, sub
    return old2new, old2sub


class BundlePaths:
    """Where the four files of a trained bundle live.  Two layouts:

    * ``reference`` - the tree the reference's CLI writes and every released bundle ships as (``root`` = its ``pretrained``
      directory): ``{root}/{species}/models/{species}-{tissue}.pt`` (train.py:20,117-123; predict.py:57),
      ``{root}/{species}/graphs/{species}_{tissue}_data.npz`` (preprocess_internal.py:79,180; preprocess.py:114),
      ``{root}/{species}/statistics/{tissue}_genes.txt`` / ``{tissue}_cell_type.txt`` (preprocess_internal.py:80,59-67;
      preprocess.py:67-78).  ``root`` may also be the species directory itself (``pretrained/mouse``).
    * ``flat`` - all four files in ``root`` (what ``fit(save_path=...)`` of the documented package example produces when it is
      handed a plain directory, docs/api.rst:120-130).

    ``layout="auto"`` is deterministic: a bundle of this (species, tissue) that already exists under ``root``
    decides - its layout is kept, for reading and for re-fitting in place; BOTH layouts present is an error (pass the layout).
    With nothing there yet, writing takes ``reference`` iff ``root`` is named ``pretrained`` (the reference tree's own name),
    else ``flat``; reading falls back to ``flat`` (and the caller reports the missing file)."""

    def __init__(self, root, species: str, tissue: str, layout: str = "auto", for_write: bool = False):
        root = Path(root)
        if layout not in ("auto", "flat", "reference"):
            raise ValueError(f"bundle layout {layout!r}: auto, flat or reference")
        ref_base = root if (root / "models").is_dir() and not (root / species).is_dir() else root / species
        pt_name = f"{species}-{tissue}.pt"
        if layout == "auto":
            has_ref, has_flat = (ref_base / "models" / pt_name).exists(), (root / pt_name).exists()
            if has_ref and has_flat:
                raise ValueError(f"{root} holds {pt_name} in BOTH bundle layouts ({ref_base / 'models' / pt_name} and "
                                 f"{root / pt_name}): pass bundle_layout='reference' or 'flat'")
            if has_ref or has_flat:
                layout = "reference" if has_ref else "flat"
            else:
                layout = "reference" if (for_write and root.name == "pretrained") else "flat"
        self.layout, self.root = layout, root
        if layout == "reference":
            self.model = ref_base / "models" / pt_name
            self.support = ref_base / "graphs" / f"{species}_{tissue}_data.npz"
            self.genes = ref_base / "statistics" / f"{tissue}_genes.txt"
            self.cell_types = ref_base / "statistics" / f"{tissue}_cell_type.txt"
            # the label map sits next to ``pretrained/`` in the reference tree (predict.py:125 reads ./map/ from the cwd)
            self.map_candidates = [root / "celltype2subtype.xlsx", ref_base / "celltype2subtype.xlsx",
                                   root.parent / "map" / "celltype2subtype.xlsx", ref_base.parent.parent / "map" / "celltype2subtype.xlsx",
                                   Path("map") / "celltype2subtype.xlsx"]
        else:
            self.model = root / pt_name
            self.support = root / f"{species}_{tissue}_data.npz"
            self.genes = root / f"{tissue}_genes.txt"
            self.cell_types = root / f"{tissue}_cell_type.txt"
            self.map_candidates = [root / "celltype2subtype.xlsx", Path("map") / "celltype2subtype.xlsx"]

    def mkdirs(self) -> None:
        for f in (self.model, self.support, self.genes, self.cell_types):
            f.parent.mkdir(parents=True, exist_ok=True)

    def label_map(self) -> Optional[Path]:
        return next((f for f in self.map_candidates if f.exists()), None)


def _classify(logits: torch.Tensor, unsure_rate: float) -> Tuple[np.ndarray, np.ndarray]:
    """softmax -> 'unsure' iff max_prob < unsure_rate/num_classes, else argmax (predict.py:78-88)."""
    prob = F.softmax(logits.float(), dim=1)
    mx, arg = prob.max(dim=1)
    unsure = mx < unsure_rate / logits.shape[1]
    return torch.where(unsure, torch.full_like(arg, -1), arg).cpu().numpy(), prob.cpu().numpy()


class DeepSortClassifier:
    def __init__(self, species, tissue, dense_dim=400, hidden_dim=200, batch_size=256, dropout=0.1, gpu_id=-1,
                 file_type='csv', learning_rate=0.001, weight_decay=5e-4, n_epochs=300, n_layers=1, threshold=0,
                 num_neighbors=None, exclude_rate=0.005, random_seed=None, validation_fraction=0.1):
        self.num_neighbors = int(num_neighbors or 0)          # 0 / None = every in-edge (train.py:37-38)
        self.species, self.tissue = species, tissue
        self.dense_dim, self.hidden_dim, self.batch_size, self.dropout = dense_dim, hidden_dim, batch_size, dropout
        self.gpu_id, self.file_type = gpu_id, file_type
        self.learning_rate, self.weight_decay, self.n_epochs, self.n_layers = learning_rate, weight_decay, n_epochs, n_layers
        self.threshold, self.exclude_rate = threshold, exclude_rate
        self.random_seed, self.validation_fraction = random_seed, validation_fraction
        self.graph_steps = True                               # replay full-size mini-batch steps as one hipGraph each
        self.bundle_layout = "auto"                           # "auto" | "flat" | "reference" (see BundlePaths)
        self.model: Optional[GNN] = None
        self.history: List[dict] = []

    # ---------------------------------------------------------------------------------------------
    def fit(self, files: Sequence[Tuple[str, str]], save_path=None):
        """``files`` = list of (data_file, celltype_file) (docs/api.rst:89-95)."""
        # everything below - allocations, Adam state, hipGraph capture streams (``torch.cuda.graph`` opens its capture stream
        # on the CURRENT device) - must see ``gpu_id``'s device as current; the caller's device is restored on exit
        with torch.cuda.device(_device(self.gpu_id)):
            return self._fit(files, save_path)

    def _fit(self, files: Sequence[Tuple[str, str]], save_path=None):
        dev = _device(self.gpu_id)
        if self.random_seed is not None:
            np.random.seed(self.random_seed); torch.manual_seed(self.random_seed)
        tables, types = [], []
        for data_file, type_file in files:
            df = _read_expression(data_file, self.file_type)
            ct = pd.read_csv(type_file, index_col=0)
            ct.columns = ['cell', 'type']                                   # preprocess_internal.py:125-127
            ct['type'] = ct['type'].map(str.strip)
            assert ct['cell'].tolist() == df.index.tolist(), 'cell order of data and celltype files differs'
            tables.append(df); types.append(ct['type'])
        id2gene = sorted(set().union(*[set(map(str, t.columns)) for t in tables]))     # :26-41 union of genes
        all_types = pd.concat(types)
        counts = all_types.value_counts()
        id2label = sorted(t for t, n in counts.items() if n / len(all_types) > self.exclude_rate)   # :91-96
        gene2id = {g: i for i, g in enumerate(id2gene)}
        label2id = {l: i for i, l in enumerate(id2label)}
        mats, labels = [], []
        for df, ty in zip(tables, types):
            keep = ty.isin(label2id).to_numpy()
            arr = df.to_numpy(dtype=np.float32)[keep]
            cols = np.array([gene2id[str(c)] for c in df.columns])
            r, c = np.nonzero(arr > self.threshold)                          # :158
            mats.append(sp.csr_matrix((arr[r, c], (r, cols[c])), shape=(arr.shape[0], len(id2gene))))
            labels += [label2id[t] for t in ty[keep]]
        expr = sp.vstack(mats).tocsr(); expr.sort_indices()
        C, G = expr.shape
        feats = _features(expr, C, self.dense_dim, self.random_seed, dev)
        graph = CellGeneGraph.from_expression(expr, device=dev)
        y = torch.tensor(labels, dtype=torch.long, device=dev)
        perm = np.random.permutation(C)
        n_val = int(C * self.validation_fraction)
        val_ids = torch.from_numpy(perm[:n_val] + G).to(dev); train_ids = torch.from_numpy(perm[n_val:] + G).to(dev)
        model = GNN(self.dense_dim, self.hidden_dim, len(id2label), self.n_layers, G, activation=F.relu,
                    dropout=self.dropout).to(dev)
        best, self.history = -1.0, []
        sample_gen = None
        if self.num_neighbors:                                               # train.py:39-40,71-78
            from .sampler import DeviceSampler
            seed = self.random_seed if self.random_seed is not None else torch.initial_seed() % 2 ** 31
            kk = min(self.num_neighbors, max(graph.cg.max_row_nnz, graph.gc.max_row_nnz) + 1)
            # K5's static NodeFlow draws for ALL cells and genes below the last block (O((C+G) k) per layer, capturable);
            # the closure sampler only touches the nodes a batch reaches (~ B k^(L-1)) but has data-dependent shapes.
            # Static pays off when the closure is a sizeable part of the graph anyway, and always for one layer.
            closure = self.batch_size * kk ** max(0, self.n_layers - 1)
            if kk <= 256 and (self.n_layers == 1 or 4 * closure >= C + G):
                sample_gen = DeviceSampler(seed, dev)                        # K5: static shapes, sync-free, capturable
            else:                                                            # very wide draws / shallow closures: torch-op sampler
                sample_gen = torch.Generator(device=dev)
                sample_gen.manual_seed(seed)
        # static shapes (full neighbourhoods, or NodeFlows drawn by the device sampler): one hipGraph launch per batch
        static_shapes = not self.num_neighbors or not isinstance(sample_gen, torch.Generator)
        will_graph = self.graph_steps and static_shapes and len(train_ids) >= 8 * self.batch_size
        # train.py:34-35.  `capturable` (step counter and bias correction on device tensors) only when a step is actually
        # replayed as a hipGraph; otherwise the reference's plain Adam arithmetic
        # (fused=True: the same Adam arithmetic - L2 weight decay folded into the gradient - in one multi-tensor launch instead
        # of ~10 per step)
        opt = torch.optim.Adam(model.parameters(), lr=self.learning_rate, weight_decay=self.weight_decay, capturable=will_graph,
                               fused=True)
        bundle = BundlePaths(save_path, self.species, self.tissue, self.bundle_layout, for_write=True) if save_path is not None else None
        if bundle is not None:
            bundle.mkdirs()
            bundle.genes.write_bytes("".join(g + "\r\n" for g in id2gene).encode())
            bundle.cell_types.write_bytes("".join(l + "\r\n" for l in id2label).encode())
            sp.save_npz(bundle.support, expr)

        def accuracy(ids):
            if len(ids) == 0:
                return 1.0, 0
            model.eval()
            with torch.no_grad():
                # the same (graph, feats) after every weight update: layer 1's gene rows come from the graph's cached feature sum
                pred, _ = _classify(model(graph, feats, seeds=ids, feature_sum_cache=True), 2.0)
            truth = y[ids - G].cpu().numpy()
            return float((pred == truth).mean()), int((pred < 0).sum())

        def train_step(batch):                                               # train.py:71-87, no host synchronisation
            logits = model(graph, feats, seeds=batch, num_neighbors=self.num_neighbors, generator=sample_gen)
            loss = cross_entropy_sum(logits, y[batch - G])                   # CrossEntropyLoss(reduction='sum'), train.py:36
            opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
            return loss.detach()

        step = train_step
        if will_graph:
            from .graphed import GraphedTrainStep
            step = GraphedTrainStep(train_step, self.batch_size, dev)
        self._step = step
        for epoch in range(self.n_epochs):
            model.train()
            total = torch.zeros((), device=dev)
            order = train_ids[torch.randperm(len(train_ids), device=dev)]
            for batch in torch.split(order, self.batch_size):
                total += step(batch)                                         # accumulated on the device
            total = float(total)                                             # ONE read-back per epoch
            tr_acc, _ = accuracy(train_ids)
            va_acc, va_unsure = accuracy(val_ids)
            self.history.append(dict(epoch=epoch, loss=total / max(1, len(train_ids)), train_acc=tr_acc, val_acc=va_acc))
            if va_acc >= best:                                                # train.py:52-58
                best = va_acc
                if bundle is not None:
                    torch.save({'model': model.state_dict(), 'optimizer': opt.state_dict()}, bundle.model)
            if tr_acc == 1:                                                   # train.py:62-63
                break
        self.model, self._graph, self._feats, self._id2label, self._id2gene = model, graph, feats, id2label, id2gene
        return self

    # ---------------------------------------------------------------------------------------------
    def predict(self, input_file, model_path, save_path=None, unsure_rate=2., file_type='csv') -> pd.DataFrame:
        return _predict(self.species, self.tissue, input_file, Path(model_path), save_path, unsure_rate, file_type,
                        self.dense_dim, self.hidden_dim, self.gpu_id, self.threshold, self.random_seed)


class DeepSortPredictor:
    def __init__(self, species, tissue, file_type='csv', unsure_rate=2.):
        self.species, self.tissue, self.file_type, self.unsure_rate = species, tissue, file_type, unsure_rate

    def predict(self, input_file, save_path=None, model_path='pretrained') -> pd.DataFrame:
        """docs/api.rst:25-26 (the doc example also passes ``model_path=``, :42).  Uses the reference's fixed
        predict-time sizes dense_dim=400, hidden_dim=200 (predict.py:170-172)."""
        return _predict(self.species, self.tissue, input_file, Path(model_path), save_path, self.unsure_rate,
                        self.file_type, 400, 200, -1, 0, 10086)


def _predict(species, tissue, input_file, model_path: Path, save_path, unsure_rate, file_type, dense_dim, hidden_dim,
             gpu_id, threshold, seed) -> pd.DataFrame:
    with torch.cuda.device(_device(gpu_id)):                 # current device = gpu_id's for the call, restored on exit
        return _predict_on(species, tissue, input_file, model_path, save_path, unsure_rate, file_type, dense_dim, hidden_dim,
                           gpu_id, threshold, seed)


def _load_bundle(species, tissue, model_path: Path, dev) -> dict:
    """The four files of a trained bundle (BundlePaths), parsed: vocabularies, support matrix, state dict and its sizes."""
    bundle = BundlePaths(model_path, species, tissue)
    missing = [str(f) for f in (bundle.model, bundle.support, bundle.genes, bundle.cell_types) if not f.exists()]
    if missing:
        raise FileNotFoundError(f"bundle for {species}/{tissue} under {model_path} ({bundle.layout} layout) lacks: " + ", ".join(missing))
    id2gene = [l.strip() for l in bundle.genes.read_text().splitlines() if l.strip()]
    id2label = [l.strip() for l in bundle.cell_types.read_text().splitlines() if l.strip()]
    support = sp.load_npz(bundle.support).tocsr()                                        # preprocess.py:114-117
    state = torch.load(bundle.model, map_location=dev)['model']                          # predict.py:56-59
    n_layers = sum(1 for k in state if k.endswith("fc_neigh.weight"))
    hidden_dim, dense_dim = state["layers.0.fc_neigh.weight"].shape
    return dict(bundle=bundle, id2gene=id2gene, id2label=id2label, support=support, state=state, n_layers=n_layers,
                hidden_dim=hidden_dim, dense_dim=dense_dim, gene2id={g: i for i, g in enumerate(id2gene)})


def _read_test_csr(input_file, file_type, gene2id: dict, threshold) -> Tuple[sp.csr_matrix, pd.Index]:
    """A test file as a (cells x bundle genes) CSR of raw values > threshold; genes outside the bundle are dropped
    (preprocess.py:160-161, 173-178)."""
    df = _read_expression(input_file, file_type)
    cols = [c for c in df.columns if str(c) in gene2id]                                  # preprocess.py:160-161
    arr = df[cols].to_numpy(dtype=np.float32)
    cid = np.array([gene2id[str(c)] for c in cols])
    r, c = np.nonzero(arr > threshold)
    test = sp.csr_matrix((arr[r, c], (r, cid[c])), shape=(arr.shape[0], len(gene2id)))
    return test, df.index


DUPLICATES = ("error", "drop", "first", "sum")


def _resolve_genes(genes, gene2id: dict, aliases=None, duplicates: str = "error"):
    """The caller's gene list as bundle ids, and the columns that share a gene: ``(ids int32 [len(genes)], groups)``.
    Names are compared as ``str`` (as ``_read_test_csr`` compares column names); a name outside the bundle is looked up in
    ``aliases`` (caller name -> bundle gene name) - a name that IS a bundle gene is never aliased (exact symbols first, as
    reference ``pre-process.R:14-16``), an alias whose target is no bundle gene leaves -1.  No name inside the bundle at all
    raises ValueError.  Positions that name the same bundle gene form a group, and ``duplicates`` says what becomes of it:
    ``"error"`` raises ValueError, ``"drop"`` sets every member to -1 (the reference keeps the names that occur once,
    ``pre-process.R``: ``genedata1$Freq == 1``), ``"first"`` keeps the lowest position, ``"sum"`` keeps all of them and returns
    ``groups = (col_group int32 [len(genes)], group_ptr int32 [n_groups + 1], group_cols int32 [n_members])`` - a position's
    group or -1, and each group's positions, ascending (groups by ascending gene id).  ``groups`` is ``None`` otherwise, and
    whenever nothing collides."""
    if duplicates not in DUPLICATES:
        raise ValueError(f"duplicates = {duplicates!r}: pass one of {', '.join(map(repr, DUPLICATES))}")
    alias = {str(k): str(v) for k, v in aliases.items()} if aliases else {}

    def lookup(g):
        name = str(g)
        i = gene2id.get(name, -1)
        return gene2id.get(alias[name], -1) if i < 0 and name in alias else i

    ids = np.fromiter((lookup(g) for g in genes), dtype=np.int64, count=len(genes)).astype(np.int32)
    hit = ids[ids >= 0]
    if hit.size == 0:
        raise ValueError(f"none of the {len(ids)} gene names is a gene of the bundle ({len(gene2id)} genes)")
    uniq, first, n = np.unique(hit, return_index=True, return_counts=True)
    if not (n > 1).any():
        return ids, None
    if duplicates == "error":
        dup = int(uniq[n > 1][0])
        where = np.flatnonzero(ids == dup)[:2].tolist()
        raise ValueError(f"positions {where[0]} and {where[1]} of the gene list both name bundle gene {dup} "
                         f"({str(genes[where[0]])!r}): a cell may list a gene once")
    member = np.isin(ids, uniq[n > 1])
    if duplicates == "drop":
        ids[member] = -1
        return ids, None
    pos = np.flatnonzero(member)
    pos = pos[np.argsort(ids[pos], kind="stable")]                       # by gene, ascending position within a gene
    starts = np.flatnonzero(np.r_[True, np.diff(ids[pos]) != 0])
    if duplicates == "first":
        ids[np.delete(pos, starts)] = -1
        return ids, None
    col_group = np.full(len(ids), -1, np.int32)
    col_group[pos] = np.repeat(np.arange(len(starts), dtype=np.int32), np.diff(np.r_[starts, len(pos)]))
    return ids, (col_group, np.r_[starts, len(pos)].astype(np.int32), pos.astype(np.int32))


def _gene_map_ids(genes, gene2id: dict, aliases=None, duplicates: str = "error") -> np.ndarray:
    """``_resolve_genes``' ids alone (``duplicates="sum"`` needs the groups as well: use ``_resolve_genes``)."""
    return _resolve_genes(genes, gene2id, aliases, duplicates)[0]


def _load_model(b: dict, dev) -> GNN:
    model = GNN(b["dense_dim"], b["hidden_dim"], len(b["id2label"]), b["n_layers"], len(b["id2gene"]), activation=F.relu,
                dropout=0.1).to(dev)
    model.load_state_dict(b["state"])
    model.eval()
    return model


def _graph_logits(model: GNN, support: sp.csr_matrix, test: sp.csr_matrix, gene_feat: torch.Tensor, dev,
                  expr: Optional[sp.csr_matrix] = None) -> torch.Tensor:
    """Logits of the test cells through the predict graph of support + test cells (test cells: gene->cell edges only,
    preprocess.py:184-187) with the given gene features (predict.py:61-88).  ``expr``: the stacked, index-sorted matrix
    when the caller has it already."""
    G = support.shape[1]
    if expr is None:
        expr = sp.vstack([support, test]).tocsr(); expr.sort_indices()
    n_sup = support.shape[0]
    mask = np.zeros(expr.shape[0], bool); mask[:n_sup] = True
    feats = torch.cat([gene_feat, _cell_features(expr, gene_feat, dev)])
    graph = CellGeneGraph.from_expression(expr, support_mask=mask, device=dev)
    seeds = range(G + n_sup, G + expr.shape[0])           # the test cells: one contiguous block of node ids (predict.py:64-76)
    with torch.no_grad():
        return model(graph, feats, seeds=seeds)


def _predict_logits(species, tissue, input_file, model_path: Path, file_type, gpu_id, threshold, seed):
    """The graph-side half of ``predict``: bundle -> predict graph (support cells + test cells) -> logits of the test cells.
    Returns (logits [n_test, n_classes] on the device, test cell names, id2label, BundlePaths)."""
    dev = _device(gpu_id)
    b = _load_bundle(species, tissue, model_path, dev)
    test, index = _read_test_csr(input_file, file_type, b["gene2id"], threshold)
    support = b["support"]
    expr = sp.vstack([support, test]).tocsr(); expr.sort_indices()
    gf = _gene_features(expr, support.shape[0], b["dense_dim"], seed, dev)
    logits = _graph_logits(_load_model(b, dev), support, test, gf, dev, expr)
    return logits, index, b["id2label"], b["bundle"]


def _predict_on(species, tissue, input_file, model_path: Path, save_path, unsure_rate, file_type, dense_dim, hidden_dim,
                gpu_id, threshold, seed) -> pd.DataFrame:
    logits, index, id2label, bundle = _predict_logits(species, tissue, input_file, model_path, file_type, gpu_id, threshold, seed)
    pred, _ = _classify(logits, unsure_rate)
    return _prediction_frame(species, tissue, input_file, index, pred, id2label, bundle, save_path)


def _prediction_frame(species, tissue, input_file, index, pred, id2label, bundle: BundlePaths, save_path,
                      original=None) -> pd.DataFrame:
    """The output table of predict.py:124-146 (new type / subtype names when the bundle has a label map), optionally with
    the evaluate mode's 'original label' column (:138-143); written to ``save_path`` when given."""
    names = [id2label[p] if p >= 0 else "unsure" for p in pred]
    cols = {"index": index}
    if original is not None:
        cols["original label"] = list(original)
    map_file = bundle.label_map()
    if map_file is not None:                                             # predict.py:124-146: new type / subtype names
        old2new, old2sub = load_label_map(map_file, species)
        cols["cell_type"] = [old2new.get(p, p) for p in names]
        cols["cell_subtype"] = [old2sub.get(p, p) for p in names]
    else:
        cols["cell_type"] = names
    return _write_table(pd.DataFrame(cols), save_path, species, tissue, Path(input_file).stem)


def _write_table(out: pd.DataFrame, save_path, species, tissue, suffix: str) -> pd.DataFrame:
    """``out``, written as ``{species}_{tissue}_{suffix}.csv`` under ``save_path`` when one is given."""
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        out.to_csv(Path(save_path) / f"{species}_{tissue}_{suffix}.csv", index=False)
    return out


# ------------------------------------------------------------------------------------------------
# resident prediction
# ------------------------------------------------------------------------------------------------
# nnz x H x n_layers of a batch above which ResidentPredictor takes the graph route.  A per-entry gather re-reads a whole
# H-wide table row for every non-zero, which the LDS-streamed tile kernel of the graph route avoids; but the graph route
# rebuilds the predict graph on every call.  Measured (profiles/resident_predict.json): no crossover up
# to the largest batch timed - 100 000 cells x 800 genes, 2 layers, H 200 = 3.2e10 - where the fused call takes 24.7 ms and
# the graph call 748 ms.  The limit is that largest measured point: beyond it the graph route, whose scaling is known.
RESIDENT_FUSED_MAX_WORK = int(os.environ.get("WGNN_RESIDENT_FUSED_MAX_WORK", 32_000_000_000))
# ResidentPredictor.stability: bytes of [cells x draws, H] f32 intermediates one launch of a deeper model may hold; the cells
# of a batch are chunked under it (the masks follow the cell's number in the batch, so chunking changes no bit)
STABILITY_CHUNK_BYTES = 256 * 1024 * 1024
# ResidentPredictor.doublets: bytes of merged CSR (col + val, 8 per entry) one chunk of pairs may hold; a pair's merged row is
# at most as long as its two rows together, so the chunks are cut before any launch (chunking changes no bit)
DOUBLETS_CHUNK_BYTES = 256 * 1024 * 1024
# ResidentPredictor.ambient: bytes of contaminated CSR (col + val, 8 per entry) one chunk of cells x draws may hold; a unit's row
# keeps at most its own entries plus min(n_add, G) soup genes, so the chunks are cut before any launch (chunking changes no bit)
AMBIENT_CHUNK_BYTES = 256 * 1024 * 1024
# ResidentPredictor.smooth: bytes of pooled CSR (col + val, 8 per entry) one chunk of cells may hold; a pooled row keeps at most
# min(G, its members' row lengths together) entries, so the chunks are cut before any launch (chunking changes no bit)
SMOOTH_CHUNK_BYTES = 256 * 1024 * 1024


def _byte_chunks(bound, budget: int, max_units: Optional[int] = None):
    """``(start, stop)`` of chunks of consecutive units whose output bytes fit ``budget``; ``bound``: the cumulative bytes per
    unit, on the host.  Every chunk takes at least one unit, and at most ``max_units``."""
    start, cap = 0, len(bound) if max_units is None else max_units
    while start < len(bound):
        done = int(bound[start - 1]) if start else 0
        stop = min(start + cap, max(start + 1, int(np.searchsorted(bound, done + budget, side="right"))))
        yield start, stop
        start = stop


def load_map_dict(path, tissue: str) -> dict:
    """``get_map_dict`` (reference preprocess.py:14-29): ``{num: {test cell type: {training cell types}}}`` from the rows of
    ``map/{species}/map.xlsx`` (first sheet; columns Tissue, num, Test Datasets, Celltype, Training dataset cell type)
    whose Tissue is ``tissue``."""
    rows = read_xlsx_sheet(path, None)
    if not rows:
        return {}
    header = [h.strip() if isinstance(h, str) else h for h in rows[0]]
    try:
        i_t, i_n, i_c = header.index("Tissue"), header.index("num"), header.index("Celltype")
    except ValueError as e:
        raise ValueError(f"{path}: map header {header} lacks {e}") from None
    i_train = 4                                          # itertuples' `_5` = the fifth column (:22)
    out: dict = {}
    for row in rows[1:]:
        row = row + [None] * (max(i_t, i_n, i_c, i_train) + 1 - len(row))
        if row[i_t] != tissue:
            continue
        num = int(float(row[i_n]))
        out.setdefault(num, {}).setdefault(row[i_c], set()).add(row[i_train])
    return out


def evaluate_predictions(pred, truth: Sequence[str], id2label: Sequence[str], mapping: dict):
    """``evaluate_test``'s counting (predict.py:104-118): ``pred`` = label ids with -1 for unsure; a prediction is correct
    iff its label is one of ``mapping[true label]``; unsure cells are counted and never correct.
    Returns (correct, total, unsure, acc, predicted names)."""
    correct = unsure = 0
    names = []
    for p, t in zip(pred, truth):
        if p < 0:
            unsure += 1
            names.append("unsure")
            continue
        if t not in mapping:
            raise ValueError(f"true cell type {t!r} is not in the evaluation map (its rows for this dataset: {sorted(mapping)})")
        if id2label[p] in mapping[t]:
            correct += 1
        names.append(id2label[p])
    total = len(names)
    return correct, total, unsure, (correct / total if total else 0.0), names


def dataset_number(data_file, tissue: str) -> int:
    """The dataset number of a test file named as the reference's (``{species}_{tissue}{num}_data.csv``, preprocess.py:141):
    the digits after the tissue name in the file's stem (``mouse_Testis199_data`` -> 199)."""
    stem = Path(data_file).name.split(".")[0]
    m = re.search(re.escape(tissue) + r"(\d+)", stem)
    if m is None:
        raise ValueError(f"no dataset number after {tissue!r} in {Path(data_file).name!r}: pass dataset_num")
    return int(m.group(1))


_PAIR_K_CELL, _PAIR_K_DRAW, _PAIR_GOLDEN = 0x9FB21C651E98DF25, 0xD6E8FEB86659FD93, 0x9E3779B97F4A7C15


def _i64(x: int) -> int:
    """A 64-bit pattern as the int64 that holds it (two's complement)."""
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >= 2 ** 63 else x


def _lsr(x: torch.Tensor, s: int) -> torch.Tensor:
    """Logical right shift of int64 bit patterns."""
    return (x >> s) & ((1 << (64 - s)) - 1)


def _mix64(x: torch.Tensor) -> torch.Tensor:
    """The splitmix64 finaliser of include/wgnn.h (``mix64``) on int64 tensors holding uint64 bit patterns: sums and products
    wrap around, shifts are logical."""
    x = x + _i64(_PAIR_GOLDEN)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def _draw_partners(label: torch.Tensor, n_partners: int, seed: int, across: str, draw0: int = 0) -> torch.Tensor:
    """``doublets``' partner rule (its docstring states it) on the device: ``label`` int [B] = the cells' full calls (-1 =
    unsure), returns int32 [B, n_partners]."""
    B, dev = int(label.shape[0]), label.device
    cell = torch.arange(B, dtype=torch.int64, device=dev)[:, None]
    draw = torch.arange(draw0, draw0 + n_partners, dtype=torch.int64, device=dev)[None, :]
    key = (cell * _i64(_PAIR_K_CELL)) ^ (draw * _i64(_PAIR_K_DRAW)) ^ _i64(int(seed))
    u = _mix64(key + _i64(_PAIR_GOLDEN))
    if across == "any":
        if B < 2:
            raise ValueError("doublets: a batch of one cell has no partner")
        M = torch.full((B, 1), B - 1, dtype=torch.int64, device=dev)
    else:
        sorted_label, order = torch.sort(label.to(torch.int64), stable=True)      # by (full call, index); -1 = its own group
        start = torch.searchsorted(sorted_label, label.to(torch.int64), right=False)[:, None]
        size = torch.searchsorted(sorted_label, label.to(torch.int64), right=True)[:, None] - start
        if int(size.max()) >= B:
            raise ValueError("doublets: every cell of the batch has the same call, so across=\"types\" has no partner to draw - "
                             "pass across=\"any\"")
        M = B - size
    # u mod M for the unsigned u = hi * 2^32 + lo: every intermediate is below 2^63 (M < 2^31)
    hi, lo = _lsr(u, 32), u & 0xFFFFFFFF
    k = ((hi % M) * ((1 << 32) % M) + lo) % M
    if across == "any":
        return (k + (k >= cell).to(torch.int64)).to(torch.int32)
    return order[k + torch.where(k >= start, size, torch.zeros_like(size))].to(torch.int32)


def _resolve_panels(panels, without, gene2id: dict, aliases=None, columns=None, column_ids=None):
    """``ResidentPredictor.panels``' specifications as membership tables: ``(names, complement bool [P], member_genes bool
    [P, G], member_cols bool [P, n_cols] | None, missing)``.  ``panels`` maps a name to the gene names to keep, ``without`` a name
    to those to remove (its panel is the complement); the order is ``panels`` first, then ``without``.  Gene names are compared
    as ``str``; a name that is no bundle gene is looked up in ``aliases`` (caller name -> bundle gene name), as
    ``_resolve_genes`` does.  ``column_ids`` (int [n_cols], a column's bundle gene or -1): the batch is over the caller's own
    columns, ``columns`` their names when the caller gave names - a gene name then hits the columns of that very name and the
    columns of the bundle gene it resolves to; the complement is taken over the caller's columns, and a bundle gene belongs to a
    panel iff one of the panel's columns maps to it.  Without ``column_ids`` names resolve against the bundle vocabulary.  A
    name that resolves nowhere is collected in ``missing[panel]``, in the order given.  ValueError: no panel at all, a panel
    name used twice."""
    specs = [(str(k), v, False) for k, v in (panels or {}).items()] + [(str(k), v, True) for k, v in (without or {}).items()]
    if not specs:
        raise ValueError("panels: pass at least one panel (panels={name: genes to keep}) or one set to remove (without=)")
    names = [s[0] for s in specs]
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise ValueError(f"panels: the name {twice[0]!r} is used twice (names are unique across panels= and without=)")
    alias = {str(k): str(v) for k, v in aliases.items()} if aliases else {}
    G, P = len(gene2id), len(specs)

    def bundle_id(name):
        i = gene2id.get(name, -1)
        return gene2id.get(alias[name], -1) if i < 0 and name in alias else i

    member_cols = cols_of_name = cols_of_gene = None
    if column_ids is not None:
        column_ids = np.asarray(column_ids, np.int64)
        member_cols = np.zeros((P, column_ids.shape[0]), bool)
        cols_of_name, cols_of_gene = {}, {}
        for j, g in enumerate(column_ids.tolist()):
            if g >= 0:
                cols_of_gene.setdefault(g, []).append(j)
        for j, c in enumerate(columns if columns is not None else ()):
            cols_of_name.setdefault(str(c), []).append(j)
    member_genes = np.zeros((P, G), bool)
    missing = {}
    for p, (name, gene_names, complement) in enumerate(specs):
        if isinstance(gene_names, (str, bytes)):
            raise ValueError(f"panels: {name!r} must list gene names, got one string")
        lost = []
        for g in gene_names:
            g = str(g)
            gid = bundle_id(g)
            if column_ids is None:
                if gid >= 0:
                    member_genes[p, gid] = True
                else:
                    lost.append(g)
                continue
            hit = cols_of_name.get(g, []) + (cols_of_gene.get(gid, []) if gid >= 0 else [])
            if hit:
                member_cols[p, hit] = True
            else:
                lost.append(g)
        missing[name] = lost
        if complement:
            if column_ids is None:
                member_genes[p] = ~member_genes[p]
            else:
                member_cols[p] = ~member_cols[p]
        if column_ids is not None:
            on = column_ids[member_cols[p]]
            member_genes[p, on[on >= 0]] = True
    return names, np.array([s[2] for s in specs], bool), member_genes, member_cols, missing


def _member_words(member_genes: np.ndarray) -> np.ndarray:
    """bool [P <= 64, G] -> the membership words of ``wgnn_predict_rows_panels`` as int64 [G]: bit ``p`` of word ``g`` = gene
    ``g`` belongs to panel ``p``."""
    P = member_genes.shape[0]
    shifted = member_genes.astype(np.uint64) << np.arange(P, dtype=np.uint64)[:, None]
    return np.bitwise_or.reduce(shifted, axis=0).view(np.int64)


def read_gmt(path) -> dict:
    """A gene-set file in the standard tab-separated GMT layout - one set per line: its name, a description, then its genes -
    as ``{name: [genes]}`` in file order, which ``ResidentPredictor.signatures`` takes as ``sets``.  Empty lines and empty
    fields are skipped; a line without a name and a name that occurs twice raise ``ValueError``."""
    sets = {}
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            fields = [x.strip() for x in line.rstrip("\r\n").split("\t")]
            if not any(fields):
                continue
            if not fields[0]:
                raise ValueError(f"{path}, line {n}: a gene set without a name")
            if fields[0] in sets:
                raise ValueError(f"{path}, line {n}: the set {fields[0]!r} occurs twice")
            sets[fields[0]] = [g for g in fields[2:] if g]
    return sets


@dataclass(frozen=True)
class LogNormalize:
    """``normalize=`` of ``ResidentPredictor``: the batch holds raw counts, and Seurat's ``NormalizeData`` defaults
    (``LogNormalize``, reference ``pre-process.R:33``) are applied on the device while the batch is aligned -
    ``log1p(count / library size * scale_factor)`` in fp64, the library size taken over ALL of the caller's columns, those
    outside the bundle included.  ``library_size``: one value per cell that replaces that total, for a caller who has
    already subset the genes but kept the true depths.  ``normalize="lognorm"`` is ``LogNormalize()``."""
    scale_factor: float = 1e4
    library_size: Optional[object] = None


def _normalize_spec(normalize) -> Optional[LogNormalize]:
    if normalize is None or isinstance(normalize, LogNormalize):
        return normalize
    if isinstance(normalize, str) and normalize == "lognorm":
        return LogNormalize()
    raise ValueError(f"normalize = {normalize!r}: pass None, \"lognorm\" or a LogNormalize")


@dataclass
class GeneMap:
    """``ResidentPredictor.gene_map(..., duplicates="sum")`` of a gene list in which several columns name one bundle gene:
    ``ids`` (int32 ``[n_cols]``, on the device) as the plain map, and the colliding columns as the tables the merging walk
    takes (``wgnn_align_count_ln_merge``): ``col_group`` int32 ``[n_cols]`` = a column's group or -1 when it is alone in its
    gene, ``group_ptr`` int32 ``[n_groups + 1]`` / ``group_cols`` int32 = each group's columns, ascending.
    ``n_merged_columns`` = the columns that are in a group.  Pass it as ``genes=`` wherever a gene map is taken; the batch
    must then hold raw counts (``normalize=``): the members' counts are added per cell before the logarithm."""
    ids: torch.Tensor
    col_group: torch.Tensor
    group_ptr: torch.Tensor
    group_cols: torch.Tensor
    n_groups: int
    n_merged_columns: int

    @property
    def groups(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.col_group, self.group_ptr, self.group_cols


@dataclass
class _Aligned:
    """``ResidentPredictor.align``'s output on its way into the kernels: gene ids in range by construction."""
    csr: Tuple[torch.Tensor, torch.Tensor, torch.Tensor]


# The calls that take raw counts, in the words of ``_count_spec``'s two refusals: how the caller asked for the call, what it does
# to the counts, what the normalize spec is for, and what merged columns would have to be merged under.  The key opens the
# bad-value error of ``_count_batch``.
_COUNT_OPS = {
    "stability": ("thin=\"reads\"", "thins raw counts",
                  " (the values a draw leaves are log-normalised against the draw's own library size)", "thinning"),
    "panels": ("renormalize=True", "re-normalises raw counts per panel", "", "panels"),
    "doublets": ("doublets", "adds raw counts",
                 " (the summed counts are log-normalised against the sum of the two library sizes)", "pairing"),
    "ambient": ("ambient", "adds soup reads to raw counts",
                " (the contaminated counts are log-normalised against the contaminated library size)", "contamination"),
    "smooth": ("smooth", "adds raw counts", " (the pooled counts are log-normalised against the pooled library size)", "pooling"),
    "pseudobulk": ("pseudobulk", "adds raw counts",
                   " (the summed counts are log-normalised against the summed library sizes)", "pooling"),
}


class _CountBatch(NamedTuple):
    """``ResidentPredictor._count_batch``'s output: a batch of raw counts, resolved and uploaded once, as the count-taking calls
    use it.  ``_values_batch`` fills ``csr`` (the values as given) and the call alone."""
    csr: Tuple[torch.Tensor, torch.Tensor, torch.Tensor]      # (rowptr, col, cnt): the counts over the bundle's genes
    rest: Optional[torch.Tensor] = None              # int64 [B]: a cell's reads outside the bundle
    lib: Optional[torch.Tensor] = None               # int64 [B]: its library size
    batch: object = None                             # the caller's batch on the device (_caller_batch)
    gmap: Optional[torch.Tensor] = None              # int32 [n_cols]: a column's bundle gene or -1
    pred: Optional[np.ndarray] = None                # the call as given (full_call): classify's labels,
    max_prob: Optional[np.ndarray] = None            # its probabilities (f32)
    label: Optional[torch.Tensor] = None             # and the labels on the device (int32 [B], either route)


class ResidentPredictor:
    """A trained bundle loaded ONCE, its gene side resident on the GPU, classifying any batch of test cells.

    For a given bundle everything except the test rows is constant: gene features (PCA of the support cells), and - since
    test cells feed no genes - every gene's embedding at every layer.  So a test cell's logits depend on its own expression
    row alone, and a layer is one weighted gather over one [G, H] table per entry (``wgnn_predict_rows``; the head, softmax
    and the unsure rule fused into the last layer's launch).  No graph build, no plans, no per-call PCA.

    Resident: ``Q = gene_feat . W1^T``, ``T_l = h_{l-1}[genes] . W_l^T`` for l >= 2 (h of the genes from the existing
    ``GNN._layer`` over a support-only graph), alpha, biases and the head.  A batch whose ``nnz * H * n_layers`` exceeds
    ``RESIDENT_FUSED_MAX_WORK`` (or with a hidden width above 256) takes the graph route instead - the predict graph of
    ``DeepSortPredictor`` with the cached gene features; ``last_route`` says which one ran ("fused" | "graph").

    ``normalize`` (``None`` | ``"lognorm"`` | ``LogNormalize``): the default of the ``normalize=`` argument of every method
    that takes ``genes=`` or a file - set it when the batches and files hold raw counts (``LogNormalize``).  A batch given
    over the bundle's own gene ids (no ``genes=``) is never normalised.

    ``aliases`` / ``duplicates``: how a list of NAMES passed as ``genes=``, and a file's column names, are resolved
    (``gene_map``): a mapping from other names (Ensembl ids, synonyms) to bundle gene names, and what becomes of columns
    that then name the same gene - ``"error"`` | ``"drop"`` | ``"first"`` | ``"sum"`` (add their raw counts on the device;
    needs ``normalize``).  With either set, files are read through ``align``; with both at their defaults nothing changes."""

    normalize: Optional[LogNormalize] = None
    aliases: Optional[dict] = None
    duplicates: str = "error"

    def __init__(self, species, tissue, model_path='pretrained', gpu_id=0, unsure_rate=2., file_type='csv', threshold=0,
                 seed=10086, normalize=None, aliases=None, duplicates="error"):
        self.species, self.tissue, self.unsure_rate, self.file_type, self.threshold = species, tissue, unsure_rate, file_type, threshold
        self.normalize = _normalize_spec(normalize)
        if duplicates not in DUPLICATES:
            raise ValueError(f"duplicates = {duplicates!r}: pass one of {', '.join(map(repr, DUPLICATES))}")
        self.aliases, self.duplicates = (dict(aliases) if aliases else None), duplicates
        self.model_path = Path(model_path)
        self.device = _device(gpu_id)
        self.last_route: Optional[str] = None
        with torch.cuda.device(self.device), torch.no_grad():
            self._setup(seed)

    def _setup(self, seed):
        dev = self.device
        b = _load_bundle(self.species, self.tissue, self.model_path, dev)
        self.bundle, self.id2label, self.id2gene, self._gene2id = b["bundle"], b["id2label"], b["id2gene"], b["gene2id"]
        self.support: sp.csr_matrix = b["support"]
        self.support.sort_indices()
        self.model = _load_model(b, dev)
        self.n_layers, self.n_genes, self.n_classes = b["n_layers"], len(self.id2gene), len(self.id2label)
        self.gene_feat = _gene_features(self.support, self.support.shape[0], b["dense_dim"], seed, dev)
        m = self.model
        H = m.layers[0].fc_neigh.weight.shape[0]
        self.hidden, self.hidden_padded = H, -(-H // 4) * 4
        Hp = self.hidden_padded
        self.unsure_threshold = float(np.float32(self.unsure_rate / self.n_classes))    # the comparison _classify makes
        self.alpha = m.alpha.detach().reshape(-1).float().contiguous()

        def rows_padded(w, n_cols):                      # [H, K] -> [Hp, n_cols] with zero rows / columns
            w = w.detach().float()
            return F.pad(w, (0, n_cols - w.shape[1], 0, Hp - w.shape[0])).contiguous()

        gf = self.gene_feat
        if gf.shape[1] % 4:                              # linear_fwd's K must be a multiple of 4
            gf = F.pad(gf, (0, -gf.shape[1] % 4))
        W1 = rows_padded(m.layers[0].fc_neigh.weight, gf.shape[1])
        self.tables = [_ops.linear_fwd(gf.contiguous(), W1)]                 # Q = gene_feat . W1^T  [G, Hp]
        self.biases = [F.pad(m.layers[0].fc_neigh.bias.detach().float(), (0, Hp - H)).contiguous()]
        self.self_weights: List[Optional[torch.Tensor]] = [None]
        if self.n_layers >= 2:
            # h_{l-1}[genes] from the existing layer code over a SUPPORT-ONLY graph: test cells feed no genes, so its gene rows
            # are those of every predict graph of this bundle
            g = CellGeneGraph.from_expression(self.support, device=dev)
            h_g, h_c = self.gene_feat, _cell_features(self.support, self.gene_feat, dev)
            for l in range(1, self.n_layers):
                h_g, h_c = m._layer(g, m.layers[l - 1], h_g, h_c, want_genes=True, cell_rows=None)
                Wl = rows_padded(m.layers[l].fc_neigh.weight, Hp)
                hg = h_g.float()
                hg = F.pad(hg, (0, Hp - hg.shape[1])) if hg.shape[1] < Hp else hg[:, :Hp]
                self.tables.append(_ops.linear_fwd(hg.contiguous(), Wl))     # T_l = h_{l-1}[genes] . W_l^T
                self.biases.append(F.pad(m.layers[l].fc_neigh.bias.detach().float(), (0, Hp - H)).contiguous())
                self.self_weights.append(Wl)
            del g, h_g, h_c
        self.w_head = F.pad(m.linear.weight.detach().float(), (0, Hp - H)).contiguous()
        self.b_head = m.linear.bias.detach().float().contiguous()

    # ---------------------------------------------------------------------------------------------
    def _route(self, nnz: int) -> str:
        if self.hidden_padded > 256 or nnz * self.hidden_padded * self.n_layers > RESIDENT_FUSED_MAX_WORK:
            return "graph"
        return "fused"

    def classify(self, expr, genes=None, normalize=None) -> Tuple[np.ndarray, np.ndarray, torch.Tensor]:
        """Classify a batch: ``expr`` = a scipy CSR (cells x the bundle's genes, raw values) or a device
        ``(rowptr, col, raw)`` triple over the bundle's gene ids.  Returns (label ids with -1 = unsure, max softmax
        probability, logits on the device).  With ``genes`` the batch is over the caller's own gene list, in any of the
        forms ``align`` takes, and goes through ``align`` first - with ``normalize`` as ``align`` takes it (raw counts in)."""
        with torch.cuda.device(self.device), torch.no_grad():
            return self._classify(self._over_genes(expr, genes, normalize))

    def _spec(self, normalize) -> Optional[LogNormalize]:
        """``normalize=`` of a call as a spec: ``None`` stands for the predictor's default."""
        return self.normalize if normalize is None else _normalize_spec(normalize)

    def _over_genes(self, expr, genes, normalize):
        """``expr`` as the kernels' routes take it: untouched without ``genes``, else ``align``'s output."""
        if genes is None:
            if normalize is not None:
                raise ValueError("normalize needs genes=: a batch over the bundle's gene ids has lost the columns the cell's total "
                                 "is taken over (pass genes=predictor.id2gene if the batch really holds all of them)")
            return expr
        return _Aligned(self._align(expr, genes, None, normalize))

    # ---------------------------------------------------------------------------------------------
    def gene_map(self, genes, aliases=None, duplicates="error"):
        """The caller's gene list as ``align`` wants it: int32 ``[len(genes)]`` on the device, a name's bundle gene id or -1
        for a name outside the bundle (names compared as ``str``).  Raises ValueError when two positions name the same
        bundle gene (a cell may list a gene once) or when no name is in the bundle.  Build it once for a stream of batches
        and pass it as ``genes=``.

        ``aliases``: a mapping from a caller's name to a bundle gene name (an Ensembl id or a synonym to its symbol),
        consulted only for names that are no bundle gene themselves; a target outside the bundle leaves the column
        unmatched.  ``duplicates``: what becomes of columns that name the same bundle gene - ``"error"`` (the ValueError
        above), ``"drop"`` (all of them unmatched: the reference's R step keeps the names that occur once), ``"first"`` (the
        lowest position stays) or ``"sum"``: all stay and their raw counts are added per cell inside ``align`` - the return
        value is then a ``GeneMap``, which every ``genes=`` takes, and the batch must be normalised there.  Without a
        collision the result is the plain tensor whatever ``duplicates`` is."""
        ids, groups = _resolve_genes(genes, self._gene2id, aliases, duplicates)
        dev = self.device
        if groups is None:
            return torch.from_numpy(ids).to(dev)
        col_group, group_ptr, group_cols = (torch.from_numpy(a).to(dev) for a in groups)
        return GeneMap(ids=torch.from_numpy(ids).to(dev), col_group=col_group, group_ptr=group_ptr, group_cols=group_cols,
                       n_groups=int(group_ptr.shape[0]) - 1, n_merged_columns=int(group_cols.shape[0]))

    def align(self, expr, genes, threshold=None, normalize=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """An in-memory batch over the caller's own gene list as the device ``(rowptr int64, col int32, raw f32)`` triple
        over the bundle's gene ids that ``classify`` / ``explain`` / ``markers`` take (``wgnn_align_count`` / ``_fill``):
        columns outside the bundle and values ``<= threshold`` (default: the predictor's) are dropped, a cell's kept
        entries keep the caller's order and their bits.  ``expr``: a 2-D ``torch.Tensor`` on any device (other dtypes are
        converted to float32), a 2-D numpy array, a scipy sparse matrix, or a device ``(rowptr, col, val)`` triple whose
        column ids index ``genes``.  ``genes``: the column names (resolved with the predictor's ``aliases`` / ``duplicates``),
        or what ``gene_map`` made of them - a tensor, or a ``GeneMap`` whose colliding columns are added per cell before the
        logarithm (``wgnn_align_count_ln_merge`` / ``_fill_ln_merge``; raw counts and ``normalize`` required, else
        ``ValueError``; the merged entry sits where the cell's first counting member sits).  The file route
        (``predict``) lists a cell's genes by ascending bundle id instead; the two orders coincide, and the results are
        bit-identical, when the caller's bundle genes come in the bundle's order.

        ``normalize`` (``None`` = the predictor's default | ``"lognorm"`` | ``LogNormalize``): ``expr`` holds raw counts
        (they need not be integers) and the values that leave are Seurat's ``LogNormalize`` of them, computed in fp64 inside
        the same walk (``wgnn_align_count_ln`` / ``_fill_ln``) - no normalised matrix is stored.  A cell's
        total is taken over ALL of ``genes``' columns before the ones outside the bundle are dropped, as the reference's R
        step does (``pre-process.R`` normalises at line 33 and filters symbols at line 61); an entry is kept iff its count
        is ``> 0`` and its normalised value ``> threshold``, which must be ``>= 0`` (``ValueError``).  A negative, NaN or
        infinite count anywhere in the batch raises ``WgnnError``."""
        with torch.cuda.device(self.device), torch.no_grad():
            return self._align(expr, genes, threshold, normalize)

    def _caller_batch(self, expr, genes):
        """``expr`` and ``genes`` of ``align`` / ``coverage`` as the ops take them: the batch on the device (a float32 matrix or
        a CSR triple over the caller's columns), the int32 gene map, and the ``GeneMap`` it came from (or ``None``).  A list
        of names is resolved with the predictor's ``aliases`` / ``duplicates``."""
        dev = self.device
        merged = None
        if not isinstance(genes, (torch.Tensor, GeneMap)):
            genes = self.gene_map(genes, self.aliases, self.duplicates)
        if isinstance(genes, GeneMap):
            merged, genes = genes, genes.ids
        gmap = genes.to(device=dev, dtype=torch.int32).contiguous()
        if gmap.dim() != 1:
            raise ValueError("a gene map is a vector (ResidentPredictor.gene_map)")
        n_cols = int(gmap.shape[0])
        if isinstance(expr, (tuple, list)):
            rowptr, col, val = expr
            _ops._require_cuda(rowptr, col, val)
            rowptr = rowptr if rowptr.dtype in (torch.int32, torch.int64) else rowptr.long()
            batch = (rowptr.contiguous(), col.to(torch.int32).contiguous(), val.to(torch.float32).contiguous())
        elif sp.issparse(expr):
            host = expr.tocsr()
            if host.shape[1] != n_cols:
                raise ValueError(f"expression matrix has {host.shape[1]} columns, the gene list {n_cols} names")
            batch = (torch.from_numpy(host.indptr).to(dev), torch.from_numpy(host.indices.astype(np.int32, copy=False)).to(dev),
                     torch.from_numpy(host.data.astype(np.float32, copy=False)).to(dev))
        else:
            x = expr if isinstance(expr, torch.Tensor) else torch.from_numpy(np.asarray(expr))
            if x.dim() != 2:
                raise ValueError(f"expression matrix must be 2-D (cells x genes), got {x.dim()} dimensions")
            if x.shape[1] != n_cols:
                raise ValueError(f"expression matrix has {x.shape[1]} columns, the gene list {n_cols} names")
            x = x.to(device=dev, dtype=torch.float32)
            batch = x if x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= n_cols) else x.contiguous()
        return batch, gmap, merged

    def _align(self, expr, genes, threshold, normalize=None):
        spec = self._spec(normalize)
        by_name = not isinstance(genes, (torch.Tensor, GeneMap))
        if spec is None and (isinstance(genes, GeneMap) or (by_name and self.duplicates == "sum")):
            raise ValueError("duplicates=\"sum\" needs normalize=: the batch then holds log-values, and their sum is not the log "
                             "of the summed counts (pass raw counts and normalize=\"lognorm\", or duplicates=\"drop\" / \"first\")")
        return self._align_batch(*self._caller_batch(expr, genes), threshold, spec)

    def _align_batch(self, batch, gmap, merged, threshold, spec: Optional[LogNormalize]):
        """``_align`` of a batch that ``_caller_batch`` has resolved already."""
        thr = self.threshold if threshold is None else threshold
        if spec is None:
            return _ops.align_rows(batch, gmap, self.n_genes, float(thr))
        return _ops.align_rows(batch, gmap, self.n_genes, float(thr), normalize="lognorm", scale=float(spec.scale_factor),
                               library_size=spec.library_size, groups=None if merged is None else merged.groups)

    def predict_matrix(self, expr, genes, index=None, normalize=None, clusters=None, rule: str = "vote",
                       min_fraction: float = 0.0) -> pd.DataFrame:
        """``predict`` for an in-memory batch over the caller's gene list (``expr``, ``genes``, ``normalize`` as ``align``
        takes them): the same table, ``index`` (default ``range(B)``) in place of the file's cell names.  ``clusters`` (one
        ``str`` name or integer id per cell, -1 = none; ids are taken as ``0 .. max``): the table gains ``cluster_type`` and
        ``cluster_subtype``, the call of the cell's cluster (``annotate``, ``ClusterCalls.consensus(rule, min_fraction)``) named
        as ``cell_type`` is - both hold the bundle's name without a label map, ``None`` for a cell of no cluster."""
        if clusters is None:
            pred, _, _ = self.classify(expr, genes=genes, normalize=normalize)
        else:
            if rule not in ClusterCalls.RULES:
                raise ValueError(f"rule = {rule!r}: pass one of {', '.join(map(repr, ClusterCalls.RULES))}")
            arr = clusters.detach().cpu().numpy() if isinstance(clusters, torch.Tensor) else np.asarray(clusters)
            by_id = np.issubdtype(arr.dtype, np.integer)
            ids, names = _cluster_ids(arr, n_clusters=max(int(arr.max(initial=0)) + 1, 1) if by_id else None,
                                      n_cells=self._n_cells(expr))
            with torch.cuda.device(self.device), torch.no_grad():
                calls, pred = self._annotate(self._over_genes(expr, genes, normalize), ids, names, None)
        _check_index(index, len(pred))
        out = _prediction_frame(self.species, self.tissue, "matrix", pd.RangeIndex(len(pred)) if index is None else index, pred,
                                self.id2label, self.bundle, None)
        if clusters is not None:
            per_cluster, _ = calls.consensus(rule, min_fraction)
            per_cell = np.where(ids >= 0, per_cluster[np.maximum(ids, 0)], -3)
            out["cluster_type"], out["cluster_subtype"] = _call_names(per_cell, self.id2label, calls.label_map)
        return out

    def coverage(self, expr, genes, index=None) -> "Coverage":
        """How much of a batch over the caller's own gene list the bundle's vocabulary sees - what ``align`` drops without a
        word (``wgnn_coverage_rows``, computed on the device where the batch is).  ``expr`` and ``genes`` exactly as ``align``
        takes them; there is no ``normalize`` or ``threshold``: the report describes the operand as given, and an entry
        counts iff its value is finite and ``> 0``.  A ``GeneMap`` (or names that collide under ``duplicates="sum"``) counts
        every member column as matched and reports them in ``n_merged_columns``.  ``index``: the cells' names (default
        ``range(B)``).  A matrix with
        Ensembl ids, another species' casing or old synonyms classifies from a fraction of each cell's reads; read
        ``Coverage.summary()`` before trusting ``classify`` on a new source.  Nothing else of the predictor calls this."""
        with torch.cuda.device(self.device), torch.no_grad():
            batch, gmap, merged = self._caller_batch(expr, genes)
            n_expressed, n_mapped, n_bad, total, total_mapped, col_cells = _ops.coverage_rows(batch, gmap, self.n_genes)
        ids = gmap.cpu().numpy()
        matched = ids >= 0
        present = np.zeros(self.n_genes, bool)
        present[ids[matched]] = True
        absent = np.flatnonzero(~present)
        if getattr(self, "_support_detected", None) is None:                      # support cells that express each gene: once
            self._support_detected = np.bincount(self.support.indices, minlength=self.n_genes)
        detected = self._support_detected
        names = None if isinstance(genes, (torch.Tensor, GeneMap)) else [str(g) for g in genes]
        B = int(n_expressed.shape[0])
        _check_index(index, B)
        index = pd.RangeIndex(B) if index is None else index
        return Coverage(n_columns=int(ids.shape[0]), n_matched=int(matched.sum()), n_bundle_genes=self.n_genes,
                        n_bundle_absent=int(absent.shape[0]), n_expressed=n_expressed.cpu().numpy(),
                        n_mapped=n_mapped.cpu().numpy(), n_bad=n_bad.cpu().numpy(), total=total.cpu().numpy(),
                        total_mapped=total_mapped.cpu().numpy(), col_cells=col_cells, index=index, columns=names,
                        matched=matched, absent_ids=absent, absent_support_cells=detected[absent],
                        absent_names=[self.id2gene[i] for i in absent], n_support_cells=int(self.support.shape[0]),
                        n_merged_columns=0 if merged is None else merged.n_merged_columns)

    def coverage_file(self, input_file) -> "Coverage":
        """``coverage`` of a test file: its full table and gene names, the cells named by the file's index."""
        matrix, names, index = self._read_counts_file(input_file)
        return self.coverage(matrix, names, index=index)

    def _device_csr(self, expr):
        """A batch as the kernels take it: (rowptr, col int32, raw f32) on the device, whether its gene ids are in range by
        construction, and the host CSR when the batch came as one."""
        dev = self.device
        if isinstance(expr, _Aligned):                   # align's output: ids in range by construction
            return (*expr.csr, True, None)
        if isinstance(expr, (tuple, list)):
            rowptr, col, raw = expr
            _ops._require_cuda(rowptr, col, raw)
            rowptr = rowptr if rowptr.dtype in (torch.int32, torch.int64) else rowptr.long()
            col, raw = col.to(torch.int32), raw.to(torch.float32)
            return rowptr, col, raw, False, None
        host = sp.csr_matrix(expr)
        if host.shape[1] != self.n_genes:
            raise ValueError(f"expression matrix has {host.shape[1]} gene columns, the bundle {self.n_genes}")
        rowptr = torch.from_numpy(host.indptr).to(dev)
        col = torch.from_numpy(host.indices.astype(np.int32, copy=False)).to(dev)
        raw = torch.from_numpy(host.data.astype(np.float32, copy=False)).to(dev)
        return rowptr, col, raw, True, host

    def _classify(self, expr):
        return self._classify_on_device(expr)[:3]

    def _device_labels(self, pred: np.ndarray, label: Optional[torch.Tensor]) -> torch.Tensor:
        """``_classify_on_device``'s labels on the device (int32 [B]) on either route: the graph route classifies on the host."""
        return torch.from_numpy(pred.astype(np.int32)).to(self.device) if label is None else label

    def _classify_on_device(self, expr):
        """``_classify``'s three results, and the labels as the fused route leaves them on the device (int32 [B]; ``None`` on
        the graph route, whose labels are made on the host)."""
        dev = self.device
        rowptr, col, raw, checked, host = self._device_csr(expr)
        nnz = int(col.shape[0])
        self.last_route = self._route(nnz)
        if self.last_route == "graph":
            if host is None:
                if nnz and (int(col.min()) < 0 or int(col.max()) >= self.n_genes):
                    raise WgnnError(f"gene id out of range [0, {self.n_genes}) in the batch's CSR")
                n = rowptr.shape[0] - 1
                host = sp.csr_matrix((raw.cpu().numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(n, self.n_genes))
            host = host.astype(np.float32)
            logits = _graph_logits(self.model, self.support, host, self.gene_feat, dev)
            pred, prob = _classify(logits, self.unsure_rate)
            return pred, prob.max(axis=1) if prob.shape[0] else np.zeros(0, np.float32), logits, None
        def rows(table, alpha, bias, **kw):               # gene ids the caller made are checked in the first layer's launch
            return _ops.predict_rows(rowptr, col, raw, table, alpha, bias, check_cols=not checked and table is self.tables[0], **kw)

        logits, label, max_prob = self._layers(rows)
        return label.cpu().numpy().astype(np.int64), max_prob.cpu().numpy(), logits, label

    def _layers(self, rows, **head_kw):
        """The fused route's layers over one batch.  ``rows(table, alpha, bias, self_rows=..., **kw)`` launches one layer: a row op
        of ``ops`` closed over the batch and the operands it takes in every layer.  A hidden layer returns ``h`` [units, Hp], which
        feeds the next layer's self rows; the last one is launched with the head, the unsure threshold and ``head_kw``, and what
        it returns is returned."""
        h = None
        for l in range(self.n_layers):
            kw = dict(self_rows=None if l == 0 else _ops.linear_fwd(h, self.self_weights[l]))
            if l == self.n_layers - 1:
                kw.update(head=(self.w_head, self.b_head), unsure_threshold=self.unsure_threshold, **head_kw)
            h = rows(self.tables[l], self.alpha, self.biases[l], **kw)
        return h

    def _cells_per_launch(self, n_units: int) -> int:
        """Cells per launch of a row op that runs ``n_units`` units (draws, panels) per cell: the [cells x units, Hp] f32
        intermediates of a deeper model (h, its self rows, the next h) under ``STABILITY_CHUNK_BYTES``, and cells x units below the
        kernels' 2^31.  Units follow the cell's number in the batch, so chunking changes no bit."""
        most = (2 ** 31 - 1) // n_units
        per_cell = n_units * self.hidden_padded * 4 * (3 if self.n_layers > 1 else 0)
        return most if per_cell == 0 else max(1, min(STABILITY_CHUNK_BYTES // per_cell, most))

    def _require_fused(self, name: str) -> None:
        """``stability`` and ``panels`` have no graph route: ValueError for a bundle the fused kernels cannot serve."""
        if self.hidden_padded > 256 or self.n_classes * self.hidden_padded * 4 > _ops.HEAD_LDS_BYTES:
            raise ValueError(f"{name} runs on the fused kernels only (hidden width <= 256, head <= {_ops.HEAD_LDS_BYTES} bytes); "
                             f"this bundle has hidden width {self.hidden_padded} and {self.n_classes} cell types")

    # ---------------------------------------------------------------------------------------------
    def annotate(self, expr, clusters, cluster_names: Optional[Sequence[str]] = None, n_clusters: Optional[int] = None,
                 into: Optional[ClusterCalls] = None, genes=None, normalize=None) -> ClusterCalls:
        """One cell type per CLUSTER: the batch is classified as ``classify`` does (either route), and its logits and labels
        are reduced per (cluster, type) where they lie (``wgnn_group_class_reduce``: softmax and sums in fp64, deterministic,
        no atomics) into a ``ClusterCalls`` - votes, summed probabilities, unsure and bad cells per cluster, with
        ``consensus`` / ``frame`` / ``cell_labels`` on top.  ``expr``, ``genes`` and ``normalize`` as for ``classify``.
        ``clusters``: one integer id per cell (-1 = skip) with ``cluster_names`` or ``n_clusters``, or one ``str`` name per
        cell - factorised in sorted order, or matched against ``into``'s names.  ``into``: an earlier table of the same
        bundle and clusters, which this batch is ADDED to (and which is returned): a cohort of any size streams through.
        Shape, range and name errors are ``ValueError`` before anything is launched."""
        ids, names = _cluster_ids(clusters, cluster_names, n_clusters, into, n_cells=self._n_cells(expr))
        if into is not None:
            into._require_same(names, self.id2label)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._annotate(self._over_genes(expr, genes, normalize), ids, names, into)[0]

    @staticmethod
    def _n_cells(expr) -> int:
        if isinstance(expr, _Aligned):
            expr = expr.csr
        return int(expr[0].shape[0]) - 1 if isinstance(expr, (tuple, list)) else int(expr.shape[0])

    def _label_names(self) -> Optional[Tuple[dict, dict]]:
        map_file = self.bundle.label_map()
        return None if map_file is None else load_label_map(map_file, self.species)

    def _table_fields(self, B: int, index) -> dict:
        """The keywords the per-cell result tables share: the cells' names (default ``range(B)``), the cell types, the label map."""
        return dict(index=pd.RangeIndex(B) if index is None else index, id2label=list(self.id2label), label_map=self._label_names())

    def _read_counts_file(self, path) -> Tuple[np.ndarray, List[str], pd.Index]:
        """A test file as ``genes=`` calls take it: its full (cells x genes) float32 table, its gene names, its cell names."""
        df = _read_expression(path, self.file_type)
        return df.to_numpy(dtype=np.float32), [str(c) for c in df.columns], df.index

    @staticmethod
    def _read_clusters_file(path, input_file, index) -> List[str]:
        """A clusters file laid out as the reference's cell-type files (an index column, the cell's name, its cluster's name) as
        one stripped ``str`` cluster name per cell of ``input_file``, whose cell names ``index`` holds."""
        ct = pd.read_csv(path, index_col=0)
        if ct.shape[1] != 2:
            raise ValueError(f"{path}: expected an index column, the cell names and the cluster names")
        ct.columns = ['cell', 'cluster']
        if [str(c) for c in ct['cell']] != [str(c) for c in index]:
            raise ValueError(f"cell order of {input_file} and {path} differs")
        return [str(c).strip() for c in ct['cluster']]

    def _typed_groups(self, out: pd.DataFrame) -> pd.DataFrame:
        """A per-group frame whose groups are the predicted types, with ``cell_type`` (and ``cell_subtype`` with a label map, as
        ``_prediction_frame`` names them) in place of ``group``."""
        names, label_map = out.pop("group").tolist(), self._label_names()
        if label_map is not None:
            out.insert(0, "cell_subtype", [label_map[1].get(p, p) for p in names])
        out.insert(0, "cell_type", names if label_map is None else [label_map[0].get(p, p) for p in names])
        return out

    def _save_frame(self, out: pd.DataFrame, save_path, suffix: str) -> pd.DataFrame:
        return _write_table(out, save_path, self.species, self.tissue, suffix)

    def _annotate(self, expr, ids: np.ndarray, names: Sequence[str], into: Optional[ClusterCalls]):
        """(the table, the per-cell labels) of one classified batch; ``ids`` / ``names`` as ``_cluster_ids`` made them."""
        pred, _, logits, label = self._classify_on_device(expr)
        label = self._device_labels(pred, label)
        group = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        out = None if into is None else (into.prob_sum, into.conf_sum, into.votes, into.tally)
        tables = _ops.group_class_reduce(logits.float(), label, group, len(names), out=out, accumulate=into is not None,
                                         check=False)
        calls = into if into is not None else ClusterCalls(list(names), list(self.id2label), *tables,
                                                           unsure_rate=self.unsure_rate, label_map=self._label_names())
        return calls, pred

    def annotate_file(self, input_file, clusters_file, save_path=None, normalize=None, rule: str = "vote",
                      min_fraction: float = 0.0) -> pd.DataFrame:
        """``annotate`` on a test file and a clusters file laid out as the reference's cell-type files (an index column, the
        cell's name, its cluster's name; the cells in the data file's order, else ``ValueError``): ``ClusterCalls.frame(rule,
        min_fraction)``, written as ``{species}_{tissue}_clusters.csv`` under ``save_path`` when given.  ``normalize``: as for
        ``predict``.  Cluster names are compared as stripped ``str`` and come in sorted order."""
        if rule not in ClusterCalls.RULES:
            raise ValueError(f"rule = {rule!r}: pass one of {', '.join(map(repr, ClusterCalls.RULES))}")
        test, index = self._read_test(input_file, normalize)
        clusters = self._read_clusters_file(clusters_file, input_file, index)
        return self._save_frame(self.annotate(test, clusters).frame(rule, min_fraction), save_path, "clusters")

    # ---------------------------------------------------------------------------------------------
    def stability(self, expr, keep=(0.75, 0.5, 0.25), n_draws: int = 32, seed: int = 0, genes=None, normalize=None,
                  index=None, into: Optional[Stability] = None, thin: str = "genes") -> Stability:
        """Would the call survive a shallower sequencing run?  The batch is classified once as given (``classify``'s call,
        bit for bit), then every cell is re-classified ``n_draws`` times per level of ``keep`` on a thinned copy of itself -
        the kernels draw the copies themselves, run every layer per (cell, draw) and tally a cell's draws on the device - into
        a ``Stability``: ``agreement`` / ``flips_to`` / ``fragile`` / ``frame`` / ``summary`` / ``by_cluster`` on top.  ``expr``,
        ``genes`` and ``normalize`` as for ``classify``; ``index``: the cells' names (default ``range(B)``).

        ``thin="genes"`` (the default) is UNIFORM PER-GENE DROPOUT on the values as given (``wgnn_predict_rows_dropout``): every
        stored gene of a cell is kept with probability ``keep``, whatever its value, and the survivors keep their values.

        ``thin="reads"`` is what a shallower run does (``wgnn_predict_rows_thin``): the batch holds raw integer COUNTS
        (``genes=`` and a ``normalize`` spec are required, else ``ValueError``), every READ is kept with probability ``keep`` -
        binomial thinning of each count, so a one-read gene drops out long before a 400-read gene - the reads in columns
        outside the bundle are thinned with the rest, and the surviving counts are log-normalised against the draw's OWN
        library size before the layers run; no thinned matrix is stored.  With ``LogNormalize(library_size=)`` the reads
        outside the batch's columns are ``library_size`` minus the cell's matched reads.  A count that is no integer in
        [1, 2^24], a library size below the matched reads, or a cell of 2^31 reads or more raises ``WgnnError`` naming the
        cell (one device check); a ``GeneMap`` with merged columns raises ``ValueError``.  A deeper model redoes the thinning
        in every layer's launch.

        Either way a draw is a pure function of ``(seed, cell, draw, gene[, read])``: the same whatever the order of a cell's
        genes, nested across levels (what survives at 0.25 survives at 0.5), the same however the cells are chunked.

        ``into``: an earlier ``Stability`` of the same batch, levels, seed and ``thin``, to which ``n_draws`` FURTHER draws are
        added (and which is returned): 32 draws and 32 more equal 64 at once.  Cells are chunked so that the ``[cells x draws,
        H]`` intermediates of a deeper model stay under ``STABILITY_CHUNK_BYTES``.  The draws run on the fused kernels only: a
        bundle they cannot serve (hidden width above 256) raises ValueError, there is no graph route.  Argument errors are
        ValueError before anything is launched."""
        if thin not in ("genes", "reads"):
            raise ValueError(f"thin = {thin!r}: pass \"genes\" or \"reads\"")
        levels = _keep_levels(keep)
        n_draws = int(n_draws)
        if n_draws < 1:
            raise ValueError(f"n_draws = {n_draws} must be >= 1")
        B = self._n_cells(expr)
        if into is not None:
            into._require_same(levels, B, self.id2label, seed, thin)
        _check_index(index, B)
        self._require_fused("stability")
        counts = (expr, genes, self._count_spec(genes, normalize, "stability")) if thin == "reads" else None
        with torch.cuda.device(self.device), torch.no_grad():
            values = None if counts else self._over_genes(expr, genes, normalize)
            return self._stability(values, levels, n_draws, int(seed), index, into, counts)

    def _count_spec(self, genes, normalize, op: str) -> LogNormalize:
        """The normalize spec of a call that takes raw counts (``op``: its key in ``_COUNT_OPS``), which needs ``genes=`` and a
        spec and takes no merged columns: ValueError otherwise, before anything is launched."""
        name, what, why, under = _COUNT_OPS[op]
        spec = self._spec(normalize)
        if genes is None or spec is None:
            raise ValueError(f"{name} {what}: pass the batch over its own gene list (genes=) and a normalize spec{why}")
        by_name = not isinstance(genes, (torch.Tensor, GeneMap))
        if (isinstance(genes, GeneMap) and genes.n_merged_columns) or (by_name and self.duplicates == "sum"):
            raise ValueError(f"{name} does not take merged columns (duplicates=\"sum\"): merging under {under} is not built")
        return spec

    def _count_batch(self, counts, genes, spec: LogNormalize, op: str, *, pair_check: Optional[str] = None,
                     full_call: bool = True) -> _CountBatch:
        """What every count-taking call opens with, on a batch resolved and uploaded ONCE (``_caller_batch``): the raw counts
        aligned to the bundle (threshold 0, no normalisation), a cell's reads outside the bundle and its library size, from one
        ``coverage_rows`` launch and one fused check (``thin_operand_check``; with ``pair_check``, the sentence
        ``pair_operand_check`` takes, the 2^23 bound as well) - and, with ``full_call``, the call as given: ``classify``'s on the
        lognorm-aligned batch.  A bad count raises ``WgnnError`` that opens with ``op``."""
        batch, gmap, _ = self._caller_batch(counts, genes)
        _, _, n_bad, total, total_mapped, _ = _ops.coverage_rows(batch, gmap, self.n_genes)
        if int(n_bad.sum()):
            raise WgnnError(f"{op}: a count is negative, NaN or infinite")
        if spec.library_size is not None:
            lib = spec.library_size if isinstance(spec.library_size, torch.Tensor) else torch.as_tensor(spec.library_size)
            if lib.dim() != 1 or lib.shape[0] != total.shape[0] or lib.is_complex():
                raise ValueError(f"library_size must be a real vector with one entry per cell ({total.shape[0]}), got {tuple(lib.shape)}")
            total = torch.where(total > 0, lib.to(self.device).to(torch.float64), total)     # as align: only on a cell with a count
        rest = total - total_mapped
        csr = _ops.align_rows(batch, gmap, self.n_genes, 0.0)
        _ops.thin_operand_check(csr[0], csr[2], rest, total)
        if pair_check is not None:
            _ops.pair_operand_check(csr[0], csr[2], pair_check)
        out = _CountBatch(csr, rest.to(torch.int64), total.to(torch.int64), batch, gmap)
        if not full_call:
            return out
        pred, max_prob, _, label = self._classify_on_device(_Aligned(self._align_batch(batch, gmap, None, None, spec)))
        return out._replace(pred=pred, max_prob=np.asarray(max_prob, np.float32), label=self._device_labels(pred, label))

    def _values_batch(self, device_csr, full_call: bool = True) -> _CountBatch:
        """What a call on the VALUES as given opens with, on ``_device_csr``'s output: the gene ids checked once for the whole call
        when they are not in range by construction (every launch after it skips the check), then - with ``full_call`` - the call as
        given, ``classify``'s: ``csr``, ``pred``, ``max_prob`` and ``label`` (as the route leaves it: ``None`` on the graph route)."""
        rowptr, col, raw, checked, _ = device_csr
        if not checked:
            _ops.check_gene_ids(col, self.n_genes)
        out = _CountBatch((rowptr, col, raw))
        if not full_call:
            return out
        pred, max_prob, _, label = self._classify_on_device(_Aligned(out.csr))
        return out._replace(pred=pred, max_prob=np.asarray(max_prob, np.float32), label=label)

    def _stability(self, expr, levels, n_draws, seed, index, into, counts=None):
        dev = self.device
        if counts is not None:                             # thin="reads": the draws run on the counts, the full call on the values
            thin, cb = "reads", self._count_batch(*counts, "stability")
            draw = functools.partial(_ops.predict_rows_thin, scale=float(counts[2].scale_factor), threshold=float(self.threshold))
        else:
            thin, cb = "genes", self._values_batch(self._device_csr(expr))
            draw = _ops.predict_rows_dropout
        rowptr, col, raw = cb.csr
        B, L, C = int(rowptr.shape[0]) - 1, len(levels), self.n_classes
        if into is None:
            st = Stability(keep=levels, n_draws=0, label=cb.pred, max_prob=cb.max_prob,
                           votes=torch.zeros((L, B, C), dtype=torch.int32, device=dev),
                           unsure=torch.zeros((L, B), dtype=torch.int32, device=dev),
                           empty=torch.zeros((L, B), dtype=torch.int32, device=dev),
                           conf_sum=torch.zeros((L, B), dtype=torch.float64, device=dev),
                           n_entries=np.diff(rowptr.cpu().numpy()).astype(np.int64), seed=seed, thin=thin,
                           n_reads=None if cb.lib is None else cb.lib.cpu().numpy(), **self._table_fields(B, index))
        else:
            st = into
        draw0 = st.n_draws
        step = self._cells_per_launch(n_draws)
        for li, k in enumerate(levels):
            for r0 in range(0, B, step):
                r1 = min(B, r0 + step)
                kw = dict(check_cols=False, n_draws=n_draws, keep=k, seed=seed, row0=r0, draw0=draw0)
                if thin == "reads":
                    kw["rest"] = cb.rest[r0:r1]
                self._layers(functools.partial(draw, rowptr[r0:r1 + 1], col, raw, **kw), accumulate=draw0 > 0,
                             out=(st.votes[li, r0:r1], st.unsure[li, r0:r1], st.empty[li, r0:r1], st.conf_sum[li, r0:r1]))
        st.n_draws = draw0 + n_draws
        return st

    def stability_file(self, input_file, keep=(0.75, 0.5, 0.25), n_draws: int = 32, seed: int = 0, save_path=None,
                       normalize=None, thin: str = "genes") -> pd.DataFrame:
        """``stability`` on a test file: ``Stability.frame()`` with the file's cell names, written as
        ``{species}_{tissue}_stability.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``.
        ``thin="reads"``: the file holds raw counts (``normalize`` required); its full table and gene names are thinned."""
        levels = _keep_levels(keep)
        if thin == "reads":
            if self._spec(normalize) is None:
                raise ValueError("thin=\"reads\" thins raw counts: the file needs a normalize spec")
            test, genes, index = self._read_counts_file(input_file)
        else:
            test, index = self._read_test(input_file, normalize)
            genes = normalize = None                        # _read_test has applied them
        out = self.stability(test, keep=levels, n_draws=n_draws, seed=seed, index=index, genes=genes, normalize=normalize, thin=thin)
        return self._save_frame(out.frame(), save_path, "stability")

    # ---------------------------------------------------------------------------------------------
    def panels(self, expr, panels=None, without=None, genes=None, normalize=None, renormalize: bool = False,
               index=None) -> PanelCalls:
        """Would the call survive when only a KNOWN, NAMED set of genes is measured?  The batch is classified once as given
        (``classify``'s call, bit for bit), then every cell is re-classified once per panel on the panel's genes alone - every
        layer in one launch per 64 panels (``wgnn_predict_rows_panels``), no masked matrix is built - into a ``PanelCalls``:
        ``agreement`` / ``by_type`` / ``confusion`` / ``lost`` / ``frame`` / ``summary`` on top.  ``expr``, ``genes`` and
        ``normalize`` as for ``classify``; ``index``: the cells' names (default ``range(B)``).

        ``panels`` maps a panel's name to the gene names to KEEP (a targeted assay: a probe panel, a qPCR set); ``without`` maps
        a name to the gene names to REMOVE (a confounder set: mitochondrial, ribosomal, cell-cycle genes - the panel is the
        complement).  At least one is needed, names are unique across both, the order is ``panels`` first.  With ``genes=`` given
        as names the gene names resolve against the caller's columns, else against the bundle's vocabulary; they are compared as
        ``str`` and go through the predictor's ``aliases``.  A name that resolves nowhere is no error: ``PanelCalls.missing``
        collects it.

        ``renormalize=False`` (the default) is the confounder question: the values as the model was given them, some genes taken
        away; a panel's call carries the bits of ``classify`` on the batch with the other columns removed.
        ``renormalize=True`` is the targeted-assay question: the batch holds raw integer COUNTS (``genes=`` and a ``normalize``
        spec are required, else ``ValueError``), a panel's library size is the cell's counts over the panel's columns of the
        CALLER's list, in the bundle or not, and the counts are log-normalised against it inside the kernel - the bits of
        ``classify(counts with the other columns zeroed, genes, normalize)``.  ``LogNormalize(library_size=)`` and merged
        columns (``duplicates="sum"``) raise ``ValueError``; a count that is no integer in [1, 2^24] raises ``WgnnError``.

        Cells are chunked so that the ``[cells x panels, H]`` intermediates of a deeper model stay under
        ``STABILITY_CHUNK_BYTES``.  The panels run on the fused kernels only: a bundle they cannot serve (hidden width above 256)
        raises ValueError, there is no graph route.  Argument errors are ValueError before anything is launched."""
        spec = None
        if renormalize:
            spec = self._count_spec(genes, normalize, "panels")
            if spec.library_size is not None:
                raise ValueError("renormalize=True takes a panel's own reads as its library size: LogNormalize(library_size=) does "
                                 "not apply")
        _check_index(index, self._n_cells(expr))
        self._require_fused("panels")
        columns, column_ids, groups = self._caller_columns(genes)
        names, _, member_genes, member_cols, missing = _resolve_panels(panels, without, self._gene2id, self.aliases, columns, column_ids)
        genes = self._resolved_genes(genes, normalize, columns, column_ids, groups)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._panels(expr, genes, normalize, spec, names, member_genes, member_cols, missing, index)

    def _caller_columns(self, genes):
        """``genes=`` of a call that resolves NAMED gene sets against it (``panels``, ``signatures``), resolved once: the caller's
        names (``None`` for a gene map), a column's bundle gene or -1 as a host vector (``None`` without ``genes=``: the sets
        then resolve against the bundle's vocabulary), and the columns ``_resolve_genes`` merged (``None`` without any)."""
        if genes is None:
            return None, None, None
        if isinstance(genes, (torch.Tensor, GeneMap)):
            ids = genes.ids if isinstance(genes, GeneMap) else genes
            return None, ids.detach().cpu().numpy(), None
        columns = [str(g) for g in genes]
        return (columns, *_resolve_genes(columns, self._gene2id, self.aliases, self.duplicates))

    def _resolved_genes(self, genes, normalize, columns, column_ids, groups):
        """``genes=`` as it goes on to ``align`` after ``_caller_columns``: names give way to the map made of them - the tensor, or
        the ``GeneMap`` when columns merge, which a batch without a normalize spec refuses as ``align`` does."""
        if columns is None:
            return genes
        if self.duplicates == "sum" and self._spec(normalize) is None:
            raise ValueError("duplicates=\"sum\" needs normalize=: the batch then holds log-values (see align)")
        return torch.from_numpy(column_ids).to(self.device) if groups is None else self.gene_map(columns, self.aliases, self.duplicates)

    def _panel_reads(self, batch, member_cols: np.ndarray) -> torch.Tensor:
        """int64 [B, P]: a cell's counts summed over each panel's columns of the caller's list.  Integer sums in fp64 are exact
        whatever their order; the rows (dense) or the entries (CSR) are taken in slices that keep the fp64 operand small."""
        dev = self.device
        M = torch.from_numpy(np.ascontiguousarray(member_cols.T)).to(dev).to(torch.float64)          # [n_cols, P]
        n_cols, P = M.shape
        budget = 64 * 1024 * 1024 // 8
        if isinstance(batch, torch.Tensor):
            B = int(batch.shape[0])
            lib = torch.empty((B, P), dtype=torch.float64, device=dev)
            step = max(1, budget // max(n_cols, 1))
            for r0 in range(0, B, step):
                lib[r0:r0 + step] = batch[r0:r0 + step].to(torch.float64) @ M
            return lib.to(torch.int64)
        rowptr, col, val = batch
        B = int(rowptr.shape[0]) - 1
        lib = torch.zeros((B, P), dtype=torch.float64, device=dev)
        rows = torch.repeat_interleave(torch.arange(B, device=dev), (rowptr[1:] - rowptr[:-1]).long(), output_size=int(col.shape[0]))
        step = max(1, budget // P)
        for e0 in range(0, int(col.shape[0]), step):
            sl = slice(e0, e0 + step)
            lib.index_add_(0, rows[sl], M[col[sl].long()] * val[sl].to(torch.float64)[:, None])
        return lib.to(torch.int64)

    def _panels(self, expr, genes, normalize, spec, names, member_genes, member_cols, missing, index):
        dev = self.device
        lib, mode_kw = None, {}
        if spec is not None:                               # renormalize: the panels run on the counts, the full call on the values
            cb = self._count_batch(expr, genes, spec, "panels")
            lib = self._panel_reads(cb.batch, member_cols)
            mode_kw = dict(scale=float(spec.scale_factor), threshold=float(self.threshold))
        else:
            cb = self._values_batch(self._device_csr(self._over_genes(expr, genes, normalize)))
        rowptr, col, raw = cb.csr
        B, P = int(rowptr.shape[0]) - 1, len(names)
        label = torch.empty((B, P), dtype=torch.int32, device=dev)
        prob = torch.empty((B, P), dtype=torch.float32, device=dev)
        entries = torch.empty((B, P), dtype=torch.int32, device=dev)
        for p0 in range(0, P, _ops.PANELS_PER_LAUNCH):
            p1 = min(P, p0 + _ops.PANELS_PER_LAUNCH)
            n_p = p1 - p0
            member = torch.from_numpy(_member_words(member_genes[p0:p1])).to(dev)
            step = self._cells_per_launch(n_p)
            for r0 in range(0, B, step):
                r1 = min(B, r0 + step)
                rows = functools.partial(_ops.predict_rows_panels, rowptr[r0:r1 + 1], col, raw, member=member, n_panels=n_p,
                                         check_cols=False, lib=None if lib is None else lib[r0:r1, p0:p1], **mode_kw)
                _, label[r0:r1, p0:p1], prob[r0:r1, p0:p1], entries[r0:r1, p0:p1] = self._layers(rows, want_entries=True)
        return PanelCalls(names=names, missing=missing, n_genes=member_genes.sum(axis=1).astype(np.int64),
                          n_columns=None if member_cols is None else member_cols.sum(axis=1).astype(np.int64),
                          label=cb.pred, max_prob=cb.max_prob, panel_label=label.cpu().numpy().astype(np.int64),
                          panel_prob=prob.cpu().numpy(), n_entries=entries.cpu().numpy().astype(np.int64),
                          n_reads=None if lib is None else lib.cpu().numpy(), renormalize=spec is not None,
                          **self._table_fields(B, index))

    def panels_file(self, input_file, panels=None, without=None, normalize=None, renormalize: bool = False,
                    save_path=None) -> pd.DataFrame:
        """``panels`` on a test file - its full table, its gene names as ``genes=`` and its cell names: ``PanelCalls.by_type()``,
        written as ``{species}_{tissue}_panels.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``;
        ``renormalize=True``: the file holds raw counts (a ``normalize`` spec is required)."""
        if renormalize and self._spec(normalize) is None:
            raise ValueError("renormalize=True re-normalises raw counts per panel: the file needs a normalize spec")
        matrix, genes, index = self._read_counts_file(input_file)
        out = self.panels(matrix, panels=panels, without=without, genes=genes, normalize=normalize, renormalize=renormalize,
                          index=index)
        return self._save_frame(out.by_type(), save_path, "panels")

    # ---------------------------------------------------------------------------------------------
    def signatures(self, expr, sets, genes=None, normalize=None, max_rank: int = 1500, expected: Optional[dict] = None,
                   index=None) -> SignatureScores:
        """Do the cells the model calls T cells express the marker genes you already trust?  The batch is classified once as
        given (``classify``'s call, bit for bit, either route), and on the same aligned batch - the values as the model sees
        them - every cell gets UCell's rank-based score (Andreatta & Carmona 2021) of every NAMED gene set: the genes are ranked
        within the cell's own row and the set's ranks go into a Mann-Whitney U, ``score = 1 - U / (n * max_rank)``.  A cell's
        ranks depend on its row alone and are invariant under any monotone per-cell normalisation; no control genes are drawn.
        The ranks are counted on the device in integers (``wgnn_rank_sets_rows``, 64 sets per launch, more sets in several
        launches) and finished on the host in fp64; ``include/wgnn.h`` has the definition.  Returns a ``SignatureScores``:
        ``best`` / ``own`` / ``concordant`` / ``by_type`` / ``discordant`` / ``frame`` / ``summary`` on top.  ``expr``, ``genes``
        and ``normalize`` as for ``classify``; ``index``: the cells' names (default ``range(B)``).

        ``sets`` maps a set's name to its gene names (``read_gmt`` reads a ``.gmt`` file into that).  With ``genes=`` given as
        names the gene names resolve against the caller's columns, else against the bundle's vocabulary; they are compared as
        ``str`` and go through the predictor's ``aliases``.  A name that resolves nowhere is no error:
        ``SignatureScores.missing`` collects it.  ``max_rank`` is UCell's ``maxRank``: ranks past it all count as
        ``max_rank + 1``.  ``expected`` maps a cell type of the bundle to the name of the set the caller expects for it.

        ``ValueError`` before anything is launched: no set, a set name used twice, a resolved set larger than ``max_rank``
        (UCell's own precondition), ``max_rank`` outside [1, 2^30], ``expected`` naming an unknown set or cell type.

        What this is not: there are no negative ("GENE-") signatures, no smoothing of the scores over neighbours and no null
        distribution; genes outside the bundle's vocabulary take no part, neither in the ranks nor in a set, whatever the
        caller's columns hold."""
        max_rank = int(max_rank)
        if not 1 <= max_rank <= _ops.RANK_SETS_MAX_RANK:
            raise ValueError(f"signatures: max_rank = {max_rank} must be in [1, 2^30]")
        if not sets:
            raise ValueError("signatures: pass at least one set (sets={name: gene names})")
        given = [str(k) for k in sets]
        twice = sorted({n for n in given if given.count(n) > 1})
        if twice:
            raise ValueError(f"signatures: the set name {twice[0]!r} is used twice")
        for name, gene_names in sets.items():
            if isinstance(gene_names, (str, bytes)):
                raise ValueError(f"signatures: {str(name)!r} must list gene names, got one string")
        _check_index(index, self._n_cells(expr))
        if genes is None:
            self._over_genes(expr, None, normalize)        # its refusal of normalize= without genes=, before the device is touched
        columns, column_ids, groups = self._caller_columns(genes)
        names, _, member_genes, _, missing = _resolve_panels(sets, None, self._gene2id, self.aliases, columns, column_ids)
        set_size = member_genes.sum(axis=1).astype(np.int64)
        if (set_size > max_rank).any():
            p = int(np.argmax(set_size > max_rank))
            raise ValueError(f"signatures: the set {names[p]!r} holds {int(set_size[p])} bundle genes, more than max_rank = {max_rank}")
        expected = None if expected is None else {str(t): str(s) for t, s in expected.items()}
        for cell_type, name in (expected or {}).items():
            if cell_type not in set(map(str, self.id2label)):
                raise ValueError(f"signatures: expected names the cell type {cell_type!r}, which the bundle does not hold")
            if name not in names:
                raise ValueError(f"signatures: expected names the set {name!r}, which sets= does not hold")
        genes = self._resolved_genes(genes, normalize, columns, column_ids, groups)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._signatures(expr, genes, normalize, names, member_genes, set_size, missing, max_rank, expected, index)

    def _signatures(self, expr, genes, normalize, names, member_genes, set_size, missing, max_rank, expected, index):
        dev, G = self.device, self.n_genes
        vb = self._values_batch(self._device_csr(self._over_genes(expr, genes, normalize)))
        rowptr, col, raw = vb.csr
        B, P = int(rowptr.shape[0]) - 1, len(names)
        rank2 = torch.empty((B, P), dtype=torch.int64, device=dev)
        present = torch.empty((B, P), dtype=torch.int32, device=dev)
        for p0 in range(0, P, _ops.SETS_PER_LAUNCH):
            p1 = min(P, p0 + _ops.SETS_PER_LAUNCH)
            member = torch.from_numpy(_member_words(member_genes[p0:p1])).to(dev)
            _ops.rank_sets_rows(rowptr, col, raw, member, p1 - p0, max_rank, G, check_cols=False,
                                out=(rank2[:, p0:p1], present[:, p0:p1]))
        deg = (rowptr[1:] - rowptr[:-1]).cpu().numpy().astype(np.int64)
        present = present.cpu().numpy().astype(np.int64)
        return SignatureScores(names=names, missing=missing, set_size=set_size,
                               score=_signature_scores(rank2.cpu().numpy(), present, deg, set_size, G, max_rank),
                               n_present=present, n_genes=deg, label=vb.pred, max_prob=vb.max_prob,
                               max_rank=max_rank, expected=expected, **self._table_fields(B, index))

    def signatures_file(self, data, sets, normalize=None, max_rank: int = 1500, expected: Optional[dict] = None,
                        save_path=None) -> pd.DataFrame:
        """``signatures`` on a test file - its full table, its gene names as ``genes=`` and its cell names:
        ``SignatureScores.frame()``, written as ``{species}_{tissue}_signatures.csv`` under ``save_path`` when given.  ``sets``:
        a ``{name: gene names}`` dict or the path of a ``.gmt`` file (``read_gmt``); ``normalize``: as for ``predict``."""
        if isinstance(sets, (str, os.PathLike)):
            sets = read_gmt(sets)
        matrix, genes, index = self._read_counts_file(data)
        out = self.signatures(matrix, sets, genes=genes, normalize=normalize, max_rank=max_rank, expected=expected, index=index)
        return self._save_frame(out.frame(), save_path, "signatures")

    # ---------------------------------------------------------------------------------------------
    def doublets(self, expr, genes, normalize=None, n_partners: int = 16, across: str = "types", seed: int = 0, index=None,
                 into: Optional[Doublets] = None) -> Doublets:
        """What does this model call a DOUBLET - two cells in one droplet, whose reads are the sum of both cells'?  Every cell
        of the batch is paired with ``n_partners`` other cells of the batch, the two cells' raw counts are added on the device
        and log-normalised against the sum of their library sizes (``wgnn_pair_rows_count`` / ``_fill``; the merged rows are
        stored, one chunk of pairs at a time under ``DOUBLETS_CHUNK_BYTES``), and the merged rows go through the predictor's own
        ``classify`` path - every layer, either route - so a pair's call is bit for bit ``classify`` of the host-summed count
        matrix.  Returns a ``Doublets``: ``pair_table`` / ``frame`` / ``caught`` / ``sinks`` / ``artifact_risk`` / ``dominance`` /
        ``summary`` on top.

        The batch holds raw integer COUNTS: ``genes=`` and a ``normalize`` spec are required exactly as
        ``stability(thin="reads")`` requires them (else ``ValueError``), a ``GeneMap`` with merged columns raises ``ValueError``,
        a count that is no integer in [1, 2^23] raises ``WgnnError`` naming the cell.  The genes may come in any order (the
        rows are sorted by bundle id when they are not; a pair's call follows the sorted row).  The real cells' call is
        ``classify``'s on the lognorm-aligned batch.  ``index``: the cells' names (default ``range(B)``).

        The partners, drawn on the device over the whole batch, are a pure function of ``(seed, cell, draw)``.  With ``key`` and
        ``mix64`` of ``include/wgnn.h`` (the dropout block), in uint64 with wrap-around:
        ``u = mix64((seed ^ cell * 0x9FB21C651E98DF25 ^ draw * 0xD6E8FEB86659FD93) + 0x9E3779B97F4A7C15)`` and ``k = u mod M``
        (the modulo bias is below 2^-32).  ``across="any"``: ``M = B - 1`` and the partner is ``k + (k >= cell)`` - any other
        cell.  ``across="types"`` (the default): the cells are ordered stably by (full call, index), -1 (unsure) being a group
        of its own; ``M = B`` minus the size of the cell's own group, and the partner is the ``k``-th cell of that order outside
        the group - so two cells of one call are never paired.  A batch with a single group raises ``ValueError`` (pass
        ``across="any"``).

        ``into``: an earlier ``Doublets`` of the same batch, seed and ``across``, to which ``n_partners`` FURTHER draws are
        appended (and which is returned): 8 and 8 more equal 16 at once.

        Out of scope: this characterises the model on doublets, it does not call real cells doublets - there is no kNN or
        embedding score here."""
        if across not in ("types", "any"):
            raise ValueError(f"across = {across!r}: pass \"types\" or \"any\"")
        n_partners = int(n_partners)
        if n_partners < 1:
            raise ValueError(f"n_partners = {n_partners} must be >= 1")
        spec = self._count_spec(genes, normalize, "doublets")
        B = self._n_cells(expr)
        if into is not None:
            into._require_same(B, self.id2label, seed, across)
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._doublets(expr, genes, spec, n_partners, across, int(seed), index, into)

    def _doublets(self, expr, genes, spec, n_partners, across, seed, index, into):
        dev = self.device
        cb = self._count_batch(expr, genes, spec, "doublets", pair_check="doublets adds two cells' counts in float32")
        (rowptr, col, cnt), lib = _ops.csr_rows_ascending(*cb.csr), cb.lib
        B, D = int(rowptr.shape[0]) - 1, n_partners
        draw0 = 0 if into is None else into.n_partners
        partner = _draw_partners(cb.label, D, seed, across, draw0)
        a = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(D)
        b = partner.reshape(-1).contiguous()
        # chunks of consecutive pairs whose merged rows (at most the two rows' lengths, 8 bytes per entry) fit the budget
        lens = (rowptr[1:] - rowptr[:-1]).long()
        bound = torch.cumsum((lens[a.long()] + lens[b.long()]) * 8, 0).cpu().numpy()
        draw_label = np.empty(B * D, np.int32)
        draw_prob = np.empty(B * D, np.float32)
        for q0, q1 in _byte_chunks(bound, DOUBLETS_CHUNK_BYTES):
            merged = _ops.pair_rows(rowptr, col, cnt, lib, a[q0:q1], b[q0:q1], scale=float(spec.scale_factor),
                                    threshold=float(self.threshold))
            draw_label[q0:q1], draw_prob[q0:q1] = self._classify_on_device(_Aligned(merged))[:2]
        partner, draw_label, draw_prob = partner.cpu().numpy(), draw_label.reshape(B, D), draw_prob.reshape(B, D)
        if into is None:
            return Doublets(label=cb.pred, max_prob=cb.max_prob, partner=partner, draw_label=draw_label, draw_prob=draw_prob,
                            seed=seed, across=across, **self._table_fields(B, index))
        into.partner = np.concatenate([into.partner, partner], axis=1)
        into.draw_label = np.concatenate([into.draw_label, draw_label], axis=1)
        into.draw_prob = np.concatenate([into.draw_prob, draw_prob], axis=1)
        return into

    def doublets_file(self, input_file, normalize="lognorm", n_partners: int = 16, across: str = "types", seed: int = 0,
                      save_path=None) -> pd.DataFrame:
        """``doublets`` on a test file of raw counts (its full table and gene names): ``Doublets.frame()``, written as
        ``{species}_{tissue}_doublets.csv`` under ``save_path`` when given."""
        matrix, genes, index = self._read_counts_file(input_file)
        out = self.doublets(matrix, genes, normalize=normalize, n_partners=n_partners, across=across, seed=seed, index=index)
        return self._save_frame(out.frame(), save_path, "doublets")

    # ---------------------------------------------------------------------------------------------
    def ambient(self, counts, genes, normalize=None, rho=(0.05, 0.1, 0.2), n_draws: int = 8, profile="batch", seed: int = 0,
                index=None, into: Optional[Ambient] = None) -> Ambient:
        """At which level of AMBIENT-RNA contamination does a call drift?  Every droplet also captures free-floating transcripts
        of lysed cells - the "soup", which looks like the sample's most abundant cell types - so a rare or shallow cell is
        pulled towards the dominant type.  Per level of ``rho`` and per draw, soup reads are drawn from ``profile`` and added
        to every cell's raw counts on the device, the contaminated row is log-normalised against the contaminated library size
        (``wgnn_soup_rows_count`` / ``_fill``; the rows are stored, one chunk of consecutive cells at a time under
        ``AMBIENT_CHUNK_BYTES``) and goes through the predictor's own ``classify`` path - every layer, either route - so a
        draw's call is bit for bit ``classify`` of the host-materialised contaminated count matrix.  Returns an ``Ambient``:
        ``agreement`` / ``mean_prob`` / ``flips_to`` / ``fragile`` / ``sinks`` / ``by_type`` / ``frame`` / ``summary`` on top.

        The batch holds raw integer COUNTS: ``genes=`` and a ``normalize`` spec are required exactly as ``doublets`` requires
        them (else ``ValueError``), a ``GeneMap`` with merged columns raises ``ValueError``, a count that is no integer in
        [1, 2^23] raises ``WgnnError`` naming the cell.  The genes may come in any order.  The call as given is ``classify``'s on
        the lognorm-aligned batch.  ``index``: the cells' names (default ``range(B)``).

        ``rho``: levels in [0, 1), sorted and de-duplicated: the share of the CONTAMINATED cell's reads that are soup, so a
        cell of ``lib`` reads takes ``n_add = floor(lib * rho / (1 - rho) + 0.5)`` soup reads (fp64); more than 2^23 of them
        raise ``WgnnError`` naming the cell.  The reads are a pure function of ``(seed, cell, draw, read)`` and NESTED: the
        reads added at 5 % are the first of those added at 10 %.

        ``profile``: ``"batch"`` - the batch's own column sums over ALL of the caller's columns, what SoupX falls back to
        without empty droplets - or one non-negative integer (at most 2^40) per entry of ``genes``, e.g. the summed counts of
        the run's empty droplets; columns outside the bundle fold into one bin whose reads only deepen the library.  A
        negative, fractional or non-finite weight, and a profile without any weight, raise ``ValueError``.  The profile itself
        is classified once (``soup_label`` / ``soup_prob``): what the model calls an empty droplet.

        ``into``: an earlier ``Ambient`` of the same batch, seed, levels and profile, to which ``n_draws`` FURTHER draws are
        appended (and which is returned): 4 and 4 more equal 8 at once.

        Out of scope: this characterises the model under contamination.  It does not estimate a sample's ``rho`` and does not
        decontaminate counts (SoupX, DecontX and CellBender do)."""
        levels = _rho_levels(rho)
        n_draws = int(n_draws)
        if n_draws < 1:
            raise ValueError(f"n_draws = {n_draws} must be >= 1")
        spec = self._count_spec(genes, normalize, "ambient")
        if into is not None and not isinstance(into, Ambient):
            raise ValueError("into: pass an earlier Ambient")
        B = self._n_cells(counts)
        if into is not None:
            into._require_same(levels, B, self.id2label, seed)
        _check_index(index, B)
        if not (isinstance(profile, str) and profile == "batch"):
            if isinstance(profile, str):
                raise ValueError(f"profile = {profile!r}: pass \"batch\" or one weight per entry of genes")
            profile = profile.detach().cpu().numpy() if isinstance(profile, torch.Tensor) else np.asarray(profile)
            if profile.ndim != 1 or not (np.issubdtype(profile.dtype, np.number) or profile.dtype == bool):
                raise ValueError("profile: pass \"batch\" or a vector with one weight per entry of genes")
            w = profile.astype(np.float64)
            if not np.isfinite(w).all() or (w < 0).any() or (w != np.floor(w)).any() or (w > 2.0 ** 40).any():
                raise ValueError("profile: every weight must be a non-negative integer of at most 2^40")
            if not (w > 0).any():
                raise ValueError("profile: no weight at all (an all-zero soup cannot be drawn from)")
            profile = profile.astype(np.int64)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._ambient(counts, genes, spec, levels, n_draws, profile, int(seed), index, into)

    def _soup_profile(self, profile, gmap, rowptr, col, cnt, lib):
        """The soup as ``(weights int64 [G] over the bundle's genes, the weight of everything outside it)`` on the device."""
        dev, G = self.device, self.n_genes
        if isinstance(profile, str):                       # "batch": one pooled group of every cell, the rest from the library sizes
            B = int(rowptr.shape[0]) - 1
            _, p_col, _, p_cnt, total, _ = _ops.pool_rows(rowptr, col, cnt, lib, torch.zeros(B, dtype=torch.int32, device=dev), 1,
                                                          threshold=0.0, n_genes=G)
            bundle = torch.zeros(G, dtype=torch.int64, device=dev)
            bundle[p_col.long()] = p_cnt
            return bundle, int(total[0]) - int(p_cnt.sum())
        if profile.shape[0] != gmap.shape[0]:
            raise ValueError(f"profile holds {profile.shape[0]} weights, the gene list {gmap.shape[0]} names")
        w = torch.from_numpy(profile).to(dev)
        inside = gmap >= 0
        bundle = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, gmap[inside].long(), w[inside])
        return bundle, int(w[~inside].sum())

    def _ambient(self, counts, genes, spec, levels, n_draws, profile, seed, index, into):
        dev, G, D, L = self.device, self.n_genes, n_draws, len(levels)
        cb = self._count_batch(counts, genes, spec, "ambient", pair_check="ambient adds soup reads to counts held in 32-bit slots")
        (rowptr, col, cnt), lib = cb.csr, cb.lib
        B = int(rowptr.shape[0]) - 1
        bundle, rest = self._soup_profile(profile, cb.gmap, rowptr, col, cnt, lib)
        W = int(bundle.sum()) + rest
        if W <= 0:
            raise ValueError("profile: no weight at all (an all-zero soup cannot be drawn from)")
        if W >= 2 ** 53:
            raise ValueError("profile: the weights add up to 2^53 or more (fp64 no longer holds the total exactly)")
        host_profile = (bundle.cpu().numpy(), int(rest))
        if into is not None and not (np.array_equal(into.profile[0], host_profile[0]) and int(into.profile[1]) == host_profile[1]):
            raise ValueError("into: the table was drawn from another soup profile")
        cdf = torch.zeros(G + 2, dtype=torch.int64, device=dev)
        torch.cumsum(torch.cat([bundle, torch.tensor([rest], dtype=torch.int64, device=dev)]), 0, out=cdf[1:])
        scale, thr = float(spec.scale_factor), float(self.threshold)
        # the soup itself: the profile as one pooled row against its own total
        nz = torch.nonzero(bundle).reshape(-1)
        s_ptr = torch.tensor([0, int(nz.shape[0])], dtype=torch.int64, device=dev)
        none_i32 = torch.zeros(0, dtype=torch.int32, device=dev)
        soup = _ops.pool_rows_grouped(torch.zeros(1, dtype=torch.int64, device=dev), none_i32, torch.zeros(0, dtype=torch.float32, device=dev),
                                      torch.zeros(2, dtype=torch.int64, device=dev), none_i32,
                                      torch.tensor([W], dtype=torch.int64, device=dev), G, scale, thr,
                                      seed=(s_ptr, nz.to(torch.int32), bundle[nz]))
        s_pred, s_prob, _, _ = self._classify_on_device(_Aligned(soup[:3]))
        draw0 = 0 if into is None else into.n_draws
        lens = (rowptr[1:] - rowptr[:-1]).long()
        draw_label = np.empty((B, L, D), np.int32)
        draw_prob = np.empty((B, L, D), np.float32)
        n_mapped = np.empty((B, L, D), np.int32)
        n_added = np.empty((B, L), np.int64)
        for li, k in enumerate(levels):
            n_add = torch.floor(lib.to(torch.float64) * (k / (1.0 - k)) + 0.5).to(torch.int64)
            over = torch.nonzero(n_add > _ops.SOUP_MAX_ADD)
            if over.numel():
                raise WgnnError(f"ambient: cell {int(over[0])} would take more than 2^23 soup reads at rho = {k:g}")
            n_added[:, li] = n_add.cpu().numpy()
            # chunks of consecutive cells whose contaminated rows (own entries + min(n_add, G) soup genes, 8 bytes each, per
            # draw) fit the budget
            bound = torch.cumsum((lens + torch.clamp(n_add, max=G)) * (8 * D), 0).cpu().numpy()
            for r0, r1 in _byte_chunks(bound, AMBIENT_CHUNK_BYTES, (2 ** 31 - 1) // D):
                o_rowptr, o_col, o_val, mapped = _ops.soup_rows(rowptr[r0:r1 + 1], col, cnt, lib[r0:r1], n_add[r0:r1], cdf, D, row0=r0,
                                                                draw0=draw0, seed=seed, scale=scale, threshold=thr)
                lab, prob = self._classify_on_device(_Aligned((o_rowptr, o_col, o_val)))[:2]
                draw_label[r0:r1, li], draw_prob[r0:r1, li] = lab.reshape(r1 - r0, D), np.asarray(prob).reshape(r1 - r0, D)
                n_mapped[r0:r1, li] = mapped.cpu().numpy().reshape(r1 - r0, D)
        if into is None:
            return Ambient(rho=levels, label=cb.pred, max_prob=cb.max_prob, draw_label=draw_label, draw_prob=draw_prob,
                           n_added=n_added, n_mapped=n_mapped, soup_label=int(s_pred[0]), soup_prob=float(np.asarray(s_prob)[0]),
                           profile=host_profile, seed=seed, **self._table_fields(B, index))
        into.draw_label = np.concatenate([into.draw_label, draw_label], axis=2)
        into.draw_prob = np.concatenate([into.draw_prob, draw_prob], axis=2)
        into.n_mapped = np.concatenate([into.n_mapped, n_mapped], axis=2)
        return into

    def ambient_file(self, data, normalize="lognorm", rho=(0.05, 0.1, 0.2), n_draws: int = 8, profile="batch", seed: int = 0,
                     save_path=None) -> pd.DataFrame:
        """``ambient`` on a test file of raw counts (its full table and gene names): ``Ambient.frame()``, written as
        ``{species}_{tissue}_ambient.csv`` under ``save_path`` when given."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.ambient(matrix, genes, normalize=normalize, rho=rho, n_draws=n_draws, profile=profile, seed=seed, index=index)
        return self._save_frame(out.frame(), save_path, "ambient")

    # ---------------------------------------------------------------------------------------------
    def smooth(self, counts, genes, neighbors, normalize=None, include_self: bool = True, index=None) -> Smoothed:
        """Calls on kNN-POOLED counts: every cell's raw counts are added to those of its nearest neighbours on the device, the
        pooled row is log-normalised against the pooled library size (``wgnn_hood_rows_count`` / ``_fill``: integer sums in
        LDS, exact in any order; the rows are stored, one chunk of consecutive cells at a time under ``SMOOTH_CHUNK_BYTES``) and
        goes through the predictor's own ``classify`` path - every layer, either route.  A pooled cell's call is therefore bit
        for bit ``classify(..., normalize="lognorm")`` of the host-summed count matrix ``(A + I) @ counts`` (``A @ counts`` with
        ``include_self=False``), ``A`` = the neighbour indicator.  This is one step of kNN smoothing (Wagner, Yan and Yanai),
        the idea behind metacells: a 600-read cell that half its marker genes dropped out of borrows depth from the cells
        around it, before any clustering.  Returns a ``Smoothed``: the call as given next to the pooled call, ``rescued`` /
        ``lost`` / ``changed`` / ``transitions`` / ``neighbor_agreement`` / ``by_type`` / ``frame`` / ``summary`` on top.

        The batch holds raw integer COUNTS: ``genes=`` and a ``normalize`` spec are required exactly as ``ambient`` requires
        them (else ``ValueError``), a ``GeneMap`` with merged columns raises ``ValueError``, a count that is no integer in
        [1, 2^23] raises ``WgnnError`` naming the cell.  The genes may come in any order.  The call as given is ``classify``'s on
        the lognorm-aligned batch.  ``index``: the cells' names (default ``range(B)``).

        ``neighbors``: the CALLER's graph - an integer ``[B, k]`` array or tensor of cell indices (-1 = no neighbour, so lists
        may be ragged), or a scipy sparse ``[B, B]`` matrix whose stored non-zero entries of row ``i`` are cell ``i``'s
        neighbours (``adata.obsp["connectivities"]``; the values are otherwise ignored).  A cell that is its own neighbour is
        dropped (``include_self`` says whether it takes part); an index outside ``[0, B)``, a neighbour listed twice for one
        cell and more than 255 neighbours raise ``ValueError``.  A cell without a neighbour keeps its own row (or, with
        ``include_self=False``, the empty row).

        Out of scope: this does not BUILD the graph - it runs no kNN and no embedding search - and it does not iterate: there
        is one pooling step over the counts as given.  Pooling across a type boundary blurs a rare cell into its neighbours'
        type; ``Smoothed.neighbor_agreement`` shows where a neighbourhood straddles two."""
        spec = self._count_spec(genes, normalize, "smooth")
        B = self._n_cells(counts)
        _check_index(index, B)
        hood_ptr, members = _neighbor_lists(neighbors, B, include_self)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._smooth(counts, genes, spec, hood_ptr, members, bool(include_self), index)

    def _smooth(self, counts, genes, spec, hood_ptr, members, include_self, index):
        dev, G, C = self.device, self.n_genes, self.n_classes
        cb = self._count_batch(counts, genes, spec, "smooth", pair_check="smooth adds up to 256 cells' counts in a 32-bit sum")
        (rowptr, col, cnt), lib = cb.csr, cb.lib
        B = int(rowptr.shape[0]) - 1
        lens = (rowptr[1:] - rowptr[:-1]).long().cpu().numpy()
        per_unit = lambda x: np.diff(np.concatenate([[0], np.cumsum(x[members])])[hood_ptr])      # a unit's sum over its members
        # chunks of consecutive cells whose pooled rows (at most min(G, the members' row lengths together) entries, 8 bytes each)
        # fit the budget
        bound = np.cumsum(np.minimum(per_unit(lens), G) * 8)
        d_ptr, d_members = torch.from_numpy(hood_ptr).to(dev), torch.from_numpy(members).to(dev)
        smooth_label, smooth_prob = np.empty(B, np.int64), np.empty(B, np.float32)
        kept, logits = np.empty(B, np.int64), []
        for r0, r1 in _byte_chunks(bound, SMOOTH_CHUNK_BYTES):
            pooled = _ops.hood_rows(rowptr, col, cnt, lib, d_ptr[r0:r1 + 1], d_members, G, scale=float(spec.scale_factor),
                                    threshold=float(self.threshold))
            smooth_label[r0:r1], smooth_prob[r0:r1], part, _ = self._classify_on_device(_Aligned(pooled[:3]))
            logits.append(torch.as_tensor(part))
            kept[r0:r1] = np.diff(pooled[0].cpu().numpy())
        return Smoothed(label=cb.pred, max_prob=cb.max_prob, smooth_label=smooth_label, smooth_prob=smooth_prob,
                        logits=torch.cat(logits) if logits else torch.zeros((0, C), dtype=torch.float32, device=dev),
                        n_neighbors=np.diff(hood_ptr) - (1 if include_self else 0), n_reads=per_unit(lib.cpu().numpy()),
                        n_genes=lens.astype(np.int64), smooth_n_genes=kept, hood_ptr=hood_ptr, members=members,
                        include_self=include_self, **self._table_fields(B, index))

    def smooth_file(self, data, neighbors_file, normalize="lognorm", include_self: bool = True, save_path=None) -> pd.DataFrame:
        """``smooth`` on a test file of raw counts (its full table and gene names) and a neighbours file laid out like the
        cell-type files - a CSV with a header line; the first column holds a cell's name, the further columns the names of its
        neighbours, empty fields allowed (ragged lists).  The cells may come in any order; a cell without a line has no
        neighbour.  A name that is not in the data file, and a cell with two lines, raise ``ValueError``.  Returns
        ``Smoothed.frame()``, written as ``{species}_{tissue}_smoothed.csv`` under ``save_path`` when given."""
        matrix, genes, index = self._read_counts_file(data)
        cells = [str(c) for c in index]
        at = {name: i for i, name in enumerate(cells)}
        if len(at) != len(cells):
            raise ValueError(f"{data}: a cell name occurs twice")
        table = pd.read_csv(neighbors_file, dtype=str, keep_default_na=False)
        lists = np.full((len(cells), max(table.shape[1] - 1, 0)), -1, np.int64)
        seen = set()
        for line in table.itertuples(index=False):
            names = [str(x).strip() for x in line]
            for name in names:
                if name and name not in at:
                    raise ValueError(f"{neighbors_file}: {name!r} is not a cell of {data}")
            if not names or not names[0]:
                raise ValueError(f"{neighbors_file}: a line without a cell name")
            if names[0] in seen:
                raise ValueError(f"{neighbors_file}: the cell {names[0]!r} has two lines")
            seen.add(names[0])
            lists[at[names[0]]] = [at[name] if name else -1 for name in names[1:]]
        out = self.smooth(matrix, genes, lists, normalize=normalize, include_self=include_self, index=index)
        return self._save_frame(out.frame(), save_path, "smoothed")

    # ---------------------------------------------------------------------------------------------
    def embed(self, expr, genes=None, normalize=None, space: str = "hidden") -> torch.Tensor:
        """What the model sees of a cell: float32 ``[B, D]`` on the device.  ``expr``, ``genes`` and ``normalize`` as for
        ``classify``.  ``space="hidden"``: the last layer's post-ReLU row - the vector the head reads, so that
        ``embed @ w_head.T + b_head`` are ``classify``'s logits up to rounding; ``D`` = the hidden width.  The layers run as in
        ``classify``'s fused route with the last launch headless, in chunks of consecutive cells under
        ``STABILITY_CHUNK_BYTES`` (a cell's row depends on its own entries alone: chunking changes no bit).
        ``space="features"``: the model's INPUT features of the cell, ``rownorm(X) . gene_feat`` (``CellGeneGraph.cell_features``
        on the device CSR) - no trained weight takes part, this is the unsupervised space; ``D`` = the bundle's dense width.

        Fused kernels only: a hidden width above 256 raises ``ValueError`` (there is no graph route)."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        self._require_fused("embed")
        with torch.cuda.device(self.device), torch.no_grad():
            vb = self._values_batch(self._device_csr(self._over_genes(expr, genes, normalize)), full_call=False)
            return self._embed(vb.csr, space)[:, :self.hidden if space == "hidden" else None]

    def _embed(self, csr, space: str) -> torch.Tensor:
        """``embed`` of a device CSR whose gene ids are known to be in range; the hidden space comes with its padding columns
        (zeros), ``[B, hidden_padded]``."""
        rowptr, col, raw = csr
        if space == "features":
            return CellGeneGraph.cell_features(rowptr, col, raw, self.gene_feat)
        B = int(rowptr.shape[0]) - 1
        out = torch.empty((B, self.hidden_padded), dtype=torch.float32, device=self.device)
        step = max(1, self._cells_per_launch(1))
        for r0 in range(0, B, step):
            part = rowptr[r0:min(B, r0 + step) + 1]

            def rows(table, alpha, bias, self_rows=None, **_head):        # every launch headless: the last h is the embedding
                return _ops.predict_rows(part, col, raw, table, alpha, bias, self_rows=self_rows, check_cols=False)

            out[r0:r0 + part.shape[0] - 1] = _ops._pad_cols(self._layers(rows), self.hidden_padded)
        return out

    def knn(self, expr, k: int = 15, genes=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
            index=None) -> NeighborGraph:
        """The exact k-nearest-neighbour graph of a batch among its OWN cells, in the model's space, built on the device: the
        batch is classified once (``classify``'s call, bit for bit), embedded (``embed``, ``space`` as there) and searched by
        ``wgnn_knn_rows`` - brute force over every ordered pair of cells in float32, the ``[B, B]`` distance matrix never
        stored, neighbours by ascending (squared distance, index) so that duplicate cells are listed in index order, the cell
        itself left out.  ``k`` in [1, 64].  ``metric="cosine"``: the rows are L2-normalised first
        (``torch.nn.functional.normalize``) and go through the same kernel - for unit rows ``1 - cos = d2 / 2``, the order
        is that of the cosine; an all-zero row stays zero, and its distances then mean nothing.  ``index``: the cells' names.

        Returns a ``NeighborGraph``; its ``indices`` are, as they come, the ``neighbors`` argument of ``smooth``, and
        ``to_scipy()`` is the layout of ``adata.obsp["distances"]``.  Two calls give the same bits.

        What this is not: no approximate index - the cost is ``O(B^2 D)``; no fuzzy-simplicial-set connectivities (UMAP's
        weights: ``umap`` builds them from these lists, ``graph=`` there takes this table) and no clustering (``kmeans``,
        ``louvain``); one batch only - no graph across calls (cells of several samples: ``bbknn`` lists neighbours per sample).
        A graph in ``space="hidden"`` is the classifier's own
        view: smoothing over it can confirm a wrong call; ``space="features"`` and ``Smoothed.neighbor_agreement()`` are the
        checks."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if metric not in KNN_METRICS:
            raise ValueError(f"metric = {metric!r}: pass one of {', '.join(map(repr, KNN_METRICS))}")
        if not 1 <= int(k) <= _ops.KNN_MAX_K:
            raise ValueError(f"k = {k} is outside [1, {_ops.KNN_MAX_K}]")
        self._require_fused("knn")
        _check_index(index, self._n_cells(expr))
        with torch.cuda.device(self.device), torch.no_grad():
            return self._knn(self._over_genes(expr, genes, normalize), int(k), space, metric, index)

    def _knn(self, expr, k, space, metric, index):
        vb = self._values_batch(self._device_csr(expr))
        rows = self._embed(vb.csr, space)
        if metric == "cosine":
            rows = F.normalize(rows, dim=1)
        idx, d2 = _ops.knn_rows(rows, k)
        B = int(rows.shape[0])
        return NeighborGraph(indices=idx.cpu().numpy().astype(np.int64), sq_distances=d2.cpu().numpy(), k=k, space=space,
                             metric=metric, label=vb.pred, max_prob=vb.max_prob, **self._table_fields(B, index))

    def knn_file(self, data, k: int = 15, normalize=None, space: str = "hidden", metric: str = "euclidean",
                 save_path=None) -> pd.DataFrame:
        """``knn`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  Returns one row per cell,
        ``cell`` then ``n0`` .. ``n{k-1}``: the cell's name and its neighbours' names, nearest first, empty where a list is
        short - the layout ``smooth_file`` reads as ``neighbors_file`` - written as ``{species}_{tissue}_neighbors.csv`` under
        ``save_path`` when given.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        graph = self.knn(matrix, k=k, genes=genes, normalize=normalize, space=space, metric=metric, index=index)
        cells = [str(c) for c in index]
        lists = [[cells[j] if j >= 0 else "" for j in row] for row in graph.indices]
        out = pd.DataFrame([[c] + row for c, row in zip(cells, lists)], columns=["cell"] + [f"n{j}" for j in range(graph.k)])
        return self._save_frame(out, save_path, "neighbors")

    def bbknn(self, expr, batch, k_within: int = 3, genes=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
              batch_names: Optional[Sequence[str]] = None, n_batches: Optional[int] = None, index=None) -> BatchGraph:
        """The batch-balanced kNN graph of a cohort of several samples (BBKNN, Polanski et al. 2020), built on the device: on a
        plain ``knn`` graph the cells of one sample list each other, and clusters, layouts and pseudotime split by sample before
        they split by biology; here every cell takes its ``k_within`` nearest cells in EACH batch separately and the union of
        those lists is the graph.  The batch is classified once and embedded exactly as ``knn`` does (``space`` and ``metric``
        as there), and searched by ``wgnn_knn_segments`` in one launch pair - exact brute force per batch, the rows left where
        they are, ``knn``'s distances bit for bit, ties by (squared distance, index) within a batch and across batches.
        ``batch``: one id or name per cell, resolved as ``annotate``'s ``clusters`` are (integer ids need ``batch_names`` or
        ``n_batches``; ``str`` names are factorised in sorted order) - every cell has a batch, -1 is refused.  At most 64
        batches, and ``n_batches * k_within <= 64``.  With a single batch the graph is ``knn(k=k_within)``'s.

        Returns a ``BatchGraph``.  It is a ``NeighborGraph`` with ``k = n_batches * k_within``: every ``graph=`` argument
        (``louvain``, ``leiden``, ``umap``, ``pseudotime``, ``paga``, ``diffmap``) takes it as it is, and ``smooth`` its
        ``indices``.  Two calls give the same bits.  Whether the repair is needed at all is what ``NeighborGraph.lisi`` over the
        batch ids says of a PLAIN ``knn`` graph; this graph is balanced by construction and its own batch LISI says nothing.

        What this is not: no ``trim`` of the lists; no approximate index - the cost is ``O(B^2 D)``; no correction of the
        embedding itself (no Harmony or MNN vectors: ``embed`` is unchanged); and no connectivities of its own - they are
        whatever the consumer builds from the lists, ``snn`` weights (``louvain``, ``leiden``) or the fuzzy graph (``umap``,
        ``diffmap``)."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if metric not in KNN_METRICS:
            raise ValueError(f"metric = {metric!r}: pass one of {', '.join(map(repr, KNN_METRICS))}")
        B, k_within = self._n_cells(expr), int(k_within)
        ids, names = _cluster_ids(batch, batch_names, n_batches, n_cells=B)
        if (ids < 0).any():
            raise ValueError("batch: every cell needs a batch, -1 is not taken")
        limit = min(_ops.SNN_MAX_K, _ops.FUZZY_MAX_K)
        if len(names) > _ops.KNN_SEGMENTS_MAX_SEGS or k_within < 1 or len(names) * k_within > limit:
            raise ValueError(f"{len(names)} batches with k_within = {k_within}: at most {_ops.KNN_SEGMENTS_MAX_SEGS} batches, "
                             f"k_within >= 1 and n_batches * k_within <= {limit}")
        self._require_fused("bbknn")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._bbknn(self._over_genes(expr, genes, normalize), ids, names, k_within, space, metric, index)

    def _bbknn(self, expr, ids, names, k_within, space, metric, index):
        vb = self._values_batch(self._device_csr(expr))
        rows = self._embed(vb.csr, space)
        if metric == "cosine":
            rows = F.normalize(rows, dim=1)
        lists = _ops.knn_segments(rows, torch.from_numpy(ids).to(self.device), len(names), k_within)
        B = int(rows.shape[0])
        return BatchGraph(indices=lists.merged_idx.cpu().numpy().astype(np.int64), sq_distances=lists.merged_d2.cpu().numpy(),
                          k=len(names) * k_within, space=space, metric=metric, label=vb.pred, max_prob=vb.max_prob,
                          batch=ids, batch_names=list(names), k_within=k_within,
                          by_batch_indices=lists.idx.cpu().numpy().astype(np.int64), by_batch_sq_distances=lists.d2.cpu().numpy(),
                          **self._table_fields(B, index))

    def bbknn_file(self, data, batch_file, k_within: int = 3, normalize=None, space: str = "hidden", metric: str = "euclidean",
                   save_path=None) -> pd.DataFrame:
        """``bbknn`` on a test file - its full table, its gene names as ``genes=`` and its cell names - and a batch file laid
        out like a clusters file (an index column, the cell's name, its batch's name; the cells in the data file's order, else
        ``ValueError``).  Returns ``knn_file``'s layout - ``cell`` then ``n0`` .. ``n{k-1}``, ``k = n_batches * k_within``,
        nearest first, empty where a list is short - which ``smooth_file`` reads as ``neighbors_file``; written as
        ``{species}_{tissue}_bbknn.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        batch = self._read_clusters_file(batch_file, data, index)
        graph = self.bbknn(matrix, batch, k_within=k_within, genes=genes, normalize=normalize, space=space, metric=metric, index=index)
        cells = [str(c) for c in index]
        lists = [[cells[j] if j >= 0 else "" for j in row] for row in graph.indices]
        out = pd.DataFrame([[c] + row for c, row in zip(cells, lists)], columns=["cell"] + [f"n{j}" for j in range(graph.k)])
        return self._save_frame(out, save_path, "bbknn")

    def harmony(self, expr, batch, n_clusters: Optional[int] = None, theta=2.0, sigma: float = 0.1, lamb: float = 1.0, k: Optional[int] = 15,
                compare: bool = True, n_blocks: int = 20, max_iter: int = 10, max_iter_cluster: int = 20, epsilon_cluster: float = 1e-5,
                epsilon: float = 1e-4, seed: int = 0, genes=None, normalize=None, space: str = "hidden",
                batch_names: Optional[Sequence[str]] = None, n_batches: Optional[int] = None, index=None) -> Harmonized:
        """The batch-corrected embedding of a cohort of several samples (Harmony, Korsunsky et al. 2019), computed on the device.
        ``bbknn`` repairs the graph; everything that reads ROWS - ``ops.kmeans_rows``, a plain ``knn`` graph, distances - still
        sees the sample before the biology.  Here the rows themselves are moved: the batch is classified once and embedded
        exactly as ``knn`` does (``space`` as there), and ``ops.harmony_rows`` takes soft clusters of the unit rows under a
        batch-diversity penalty (``theta``, a scalar or one value per batch; ``sigma`` the softness) and removes a per-cluster,
        per-batch ridge offset (``lamb``) from every cell, round by round until the objective settles - all in float64, in
        fixed summation orders: two calls give the same bits.  ``batch``: as ``bbknn`` takes it (-1 is refused); at most 64
        batches.  ``n_clusters`` defaults to ``min(round(B / 30), 100)``; the other keywords are ``ops.harmony_rows``'.

        ``k`` (1..64, default 15): the corrected unit rows are searched by ``wgnn_knn_rows`` and returned as ``graph`` - a
        ``NeighborGraph`` with ``metric="cosine"`` that knows the batches, so that ``graph.lisi("batch")`` says whether the
        samples now mix, and that ``louvain``, ``leiden``, ``umap``, ``pseudotime``, ``paga`` and ``diffmap`` take as ``graph=``
        (``smooth`` its ``indices``).  ``k=None`` skips it.  ``compare=True`` also searches the UNCORRECTED unit rows
        (``graph_before`` - ``knn(metric="cosine")``'s lists), which ``Harmonized.mixing()`` / ``summary()`` read against.

        Returns a ``Harmonized``.  A cell whose embedding is all zero or holds a non-finite value raises ``ValueError``.

        What this is not: one categorical covariate only; no ``tau`` (no discounting of small clusters); no per-batch automatic
        ``lamb``; the blocks are a fixed stride over the cells (``i mod n_blocks``), not a random order; ``kmeans`` /
        ``silhouette`` still embed from ``expr`` - ``ops.kmeans_rows(torch.from_numpy(h.coords).to(device), K)`` is the way for now;
        one batch of cells per call.  The comparison with harmonypy was not run: the formulas in ``include/wgnn.h`` and their
        numpy restatement are the contract."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if k is not None and not 1 <= int(k) <= _ops.KNN_MAX_K:
            raise ValueError(f"k = {k} is outside [1, {_ops.KNN_MAX_K}] (None: no graph)")
        B = self._n_cells(expr)
        ids, names = _cluster_ids(batch, batch_names, n_batches, n_cells=B)
        if (ids < 0).any():
            raise ValueError("batch: every cell needs a batch, -1 is not taken")
        if len(names) > _ops.HARMONY_MAX_BATCHES:
            raise ValueError(f"{len(names)} batches: at most {_ops.HARMONY_MAX_BATCHES}")
        self._require_fused("harmony")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            vb = self._values_batch(self._device_csr(self._over_genes(expr, genes, normalize)))
            full = self._embed(vb.csr, space)                          # the hidden space comes with its zero padding columns
            rows = full[:, :self.hidden].contiguous() if space == "hidden" else full
            run = _ops.harmony_rows(rows, torch.from_numpy(ids).to(self.device), len(names), n_clusters=n_clusters, theta=theta,
                                    sigma=sigma, lamb=lamb, n_blocks=n_blocks, max_iter=max_iter, max_iter_cluster=max_iter_cluster,
                                    epsilon_cluster=epsilon_cluster, epsilon=epsilon, seed=seed)
            coords = run.coords.to(torch.float32)
            fields = self._table_fields(B, index)

            def graph_of(x):
                idx, d2 = _ops.knn_rows(F.normalize(x, dim=1), int(k))
                return HarmonizedGraph(indices=idx.cpu().numpy().astype(np.int64), sq_distances=d2.cpu().numpy(), k=int(k),
                                       space=space, metric="cosine", label=vb.pred, max_prob=vb.max_prob, batch=ids,
                                       batch_names=list(names), **fields)

            R = run.R.cpu().numpy() if run.R is not None else np.zeros((B, 0), np.float64)
            return Harmonized(coords=coords.cpu().numpy(), embedding=rows.cpu().numpy(), cluster_prob=R,
                              cluster=R.argmax(axis=1).astype(np.int64) if R.shape[1] else np.zeros(B, np.int64),
                              centers=run.centers.cpu().numpy() if run.centers is not None else np.zeros((0, rows.shape[1])),
                              batch=ids, batch_names=list(names), objective=list(run.objective), n_iter=run.n_iter,
                              converged=run.converged, space=space, graph=None if k is None else graph_of(coords),
                              graph_before=graph_of(full) if k is not None and compare else None, label=vb.pred,
                              max_prob=vb.max_prob, **fields)

    def harmony_file(self, data, batch_file, normalize=None, space: str = "hidden", save_path=None, **harmony) -> pd.DataFrame:
        """``harmony`` on a test file - its full table, its gene names as ``genes=`` and its cell names - and a batch file laid
        out as ``bbknn_file`` reads it (an index column, the cell's name, its batch's name; the cells in the data file's order,
        else ``ValueError``).  Returns one row per cell, ``cell`` then ``h1`` .. ``hD``: the corrected coordinates, written as
        ``{species}_{tissue}_harmony.csv`` under ``save_path`` when given.  ``harmony``: the call's other keywords (``theta``,
        ``n_clusters``, ...; no graph is built).  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        batch = self._read_clusters_file(batch_file, data, index)
        harmony.update(k=None, compare=False)
        h = self.harmony(matrix, batch, genes=genes, normalize=normalize, space=space, index=index, **harmony)
        out = pd.DataFrame({"cell": [str(c) for c in index],
                            **{f"h{j + 1}": h.coords[:, j] for j in range(h.coords.shape[1])}})
        return self._save_frame(out, save_path, "harmony")

    # ---------------------------------------------------------------------------------------------
    def kmeans(self, expr, n_clusters: int, genes=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
               init="k-means++", max_iter: int = 100, seed: int = 0, index=None) -> KMeans:
        """k-means clusters of a batch in the model's space, cut on the device: the batch is classified once (``classify``'s
        call, bit for bit), embedded (``embed``, ``space`` as there) and clustered by ``ops.kmeans_rows`` - k-means++ seeding
        without a read-back between its rounds (``wgnn_kmeans_seed``), then Lloyd's iterations with ``wgnn_knn_rows`` (k = 1, the
        centres as candidates) as the assignment and a deterministic fp64 row sum (``wgnn_group_rows_reduce``) as the update.
        ``n_clusters`` in [1, 4096] and at most the number of cells; ``init``: ``"k-means++"`` (the draws are a hash of
        ``seed``) or a float32 ``[n_clusters, D]`` array of starting centres in the space's own width; ``max_iter`` >= 1.
        ``metric="cosine"``: the rows are L2-normalised first, as ``knn`` does; the centres are then the plain means of unit
        rows and are NOT re-normalised - this is Euclidean k-means on the unit sphere's points, not spherical k-means.
        ``index``: the cells' names.

        Returns a ``KMeans``; its ``cluster`` is, as it comes and with ``n_clusters=``, the ``clusters`` argument of
        ``annotate`` and ``pseudobulk`` and ``rank_genes``' ``groups`` - over-clustering into metacells for those is what this
        is for.  A cluster the iterations empty stays empty (its centre is left where it was).  Two calls give the same bits.

        What this is not: no Leiden or Louvain on the kNN graph; no ``n_init`` restarts - loop over ``seed`` and keep the
        lowest ``inertia``; no mini-batch mode and no ``tol`` - it stops on an unchanged assignment or on ``max_iter``; one
        batch only.  Fused kernels only, as ``embed``."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if metric not in KNN_METRICS:
            raise ValueError(f"metric = {metric!r}: pass one of {', '.join(map(repr, KNN_METRICS))}")
        B = self._n_cells(expr)
        if not 1 <= int(n_clusters) <= min(_ops.KMEANS_MAX_K, max(B, 1)):
            raise ValueError(f"n_clusters = {n_clusters} is outside [1, {min(_ops.KMEANS_MAX_K, B)}] (a batch of {B} cells)")
        if int(max_iter) < 1:
            raise ValueError(f"max_iter = {max_iter} must be >= 1")
        if isinstance(init, str) and init not in _ops.KMEANS_INITS:
            raise ValueError(f"init = {init!r}: pass \"k-means++\" or an array [n_clusters, D]")
        self._require_fused("kmeans")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._kmeans(self._over_genes(expr, genes, normalize), int(n_clusters), space, metric, init, int(max_iter),
                                int(seed), index)

    def _kmeans(self, expr, n_clusters, space, metric, init, max_iter, seed, index):
        vb = self._values_batch(self._device_csr(expr))
        rows = self._embed(vb.csr, space)[:, :self.hidden if space == "hidden" else None]       # embed's rows
        if metric == "cosine":
            rows = F.normalize(rows, dim=1)
        km =_ops.kmeans_rows(rows, n_clusters, init=init, max_iter=max_iter, seed=seed)
        trace = [float(v) for v in km.inertia_trace]
        return KMeans(cluster=km.label.cpu().numpy().astype(np.int64), sq_distance=km.d2.cpu().numpy(),
                      centers=km.centers.cpu().numpy(), size=km.size.cpu().numpy(),
                      seed_cells=None if km.seed_row is None else km.seed_row.cpu().numpy().astype(np.int64),
                      inertia=trace[-1], inertia_trace=trace, n_iter=km.n_iter, converged=km.converged, space=space,
                      metric=metric, label=vb.pred, max_prob=vb.max_prob, **self._table_fields(int(rows.shape[0]), index))

    def kmeans_file(self, data, n_clusters: int, normalize=None, space: str = "hidden", metric: str = "euclidean",
                    init="k-means++", max_iter: int = 100, seed: int = 0, save_path=None) -> pd.DataFrame:
        """``kmeans`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  Returns one row per cell:
        a running number, ``cell`` (its name) and ``cluster`` (its cluster's name, ``"c0000"``, ...) - with the header line the
        layout ``annotate_file`` and ``pseudobulk_file`` read as ``clusters_file`` - written as ``{species}_{tissue}_kmeans.csv``
        under ``save_path`` when given.  A cell whose embedding is not finite has no cluster: ``WgnnError``.  ``normalize``: as
        for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        km = self.kmeans(matrix, n_clusters, genes=genes, normalize=normalize, space=space, metric=metric, init=init,
                         max_iter=max_iter, seed=seed, index=index)
        if (km.cluster < 0).any():
            raise WgnnError(f"kmeans_file: {int((km.cluster < 0).sum())} cells have no finite embedding and no cluster")
        return self._save_frame(km.clusters_frame(), save_path, "kmeans")

    # ---------------------------------------------------------------------------------------------
    def louvain(self, expr, k: int = 15, resolution=1.0, weights: str = "snn", genes=None, normalize=None, space: str = "hidden",
                metric: str = "euclidean", graph=None, max_sweeps: int = 256, index=None) -> Communities:
        """Louvain communities of a batch's own kNN graph, cut on the device and in integers: the batch is classified once
        (``classify``'s call, bit for bit), searched as ``knn`` does (``k``, ``space``, ``metric`` as there), the lists made a
        symmetric graph with shared-neighbour weights (``ops.snn_graph``: ``weights="snn"``, or ``"unit"``) and clustered by
        ``ops.louvain_graph`` - a synchronous Louvain whose every gain is a 64-bit integer, so that the result depends on no
        accumulation order.  ``resolution`` (> 0) becomes ``Fraction(resolution).limit_denominator(64)``: higher = more, smaller
        communities.  ``graph``: an earlier ``NeighborGraph`` of the same batch, or a ``[B, k]`` index array (-1 = none), in
        place of the search - ``k``, ``space`` and ``metric`` are then the graph's own (an array keeps the arguments').
        ``index``: the cells' names.

        Returns a ``Communities``; its ``cluster`` is, as it comes and with ``n_clusters=``, the ``clusters`` argument of
        ``annotate`` / ``pseudobulk`` and the ``groups`` of ``rank_genes`` / ``silhouette``.  A cell without an edge (a NaN row,
        which ``knn`` lists nowhere) has community -1.  Two calls give the same bits.

        What this is not: it is Louvain, not Leiden - no refinement phase, a community can be internally disconnected; the
        weights are shared-neighbour counts, not Jaccard indices with pruning and not UMAP connectivities (``umap`` computes those, for its layout
        only: ``Layout.connectivities()``); no random restarts;
        one batch only (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table);
        a graph whose total weight ``M`` has ``M^2 max(num, den) >= 2^62`` is refused (about 10^8 edges of
        weight 16).  Fused kernels only, as ``embed``."""
        return self._graph_clusters("louvain", expr, k, resolution, weights, genes, normalize, space, metric, graph, max_sweeps, index)

    def _graph_clusters(self, method, expr, k, resolution, weights, genes, normalize, space, metric, graph, max_sweeps, index):
        """``louvain`` / ``leiden``: the checks, the graph and the cut named ``method``."""
        if weights not in _ops.SNN_WEIGHTS:
            raise ValueError(f"weights = {weights!r}: pass one of {', '.join(map(repr, _ops.SNN_WEIGHTS))}")
        if int(max_sweeps) < 1:
            raise ValueError(f"max_sweeps = {max_sweeps} must be >= 1")
        _ops.louvain_resolution(resolution)
        B = self._n_cells(expr)
        lists, k, space, metric = self._graph_lists(method, graph, B, k, space, metric, False)
        self._require_fused(method)
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._louvain(self._over_genes(expr, genes, normalize), k, resolution, weights, space, metric, lists,
                                 int(max_sweeps), index, method)

    def _louvain(self, expr, k, resolution, weights, space, metric, lists, max_sweeps, index, method="louvain"):
        vb = self._values_batch(self._device_csr(expr))
        B = int(vb.csr[0].shape[0]) - 1
        idx, _, _ = self._lists_on_device(vb, lists, k, space, metric)
        cut = _ops.leiden_graph if method == "leiden" else _ops.louvain_graph
        out = cut(*_ops.snn_graph(idx, weights), resolution=resolution, max_sweeps=max_sweeps)
        more = dict(method=method, refined_labels=[l.cpu().numpy() for l in out.refined_labels]) if method == "leiden" else {}
        cluster = out.cluster.cpu().numpy()
        return Communities(cluster=cluster, size=np.bincount(cluster[cluster >= 0], minlength=0).astype(np.int64),
                           modularity=out.modularity, resolution=out.resolution, weights=weights, levels=out.levels,
                           level_labels=[l.cpu().numpy() for l in out.level_labels], converged=out.converged, k=k, space=space,
                           metric=metric, label=vb.pred, max_prob=vb.max_prob, **more, **self._table_fields(B, index))

    def louvain_file(self, data, k: int = 15, resolution=1.0, weights: str = "snn", normalize=None, space: str = "hidden",
                     metric: str = "euclidean", max_sweeps: int = 256, save_path=None) -> pd.DataFrame:
        """``louvain`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  Returns one row per cell:
        a running number, ``cell`` (its name) and ``cluster`` (its community's name, ``"c0000"``, ...) - ``kmeans_file``'s layout,
        which ``annotate_file``, ``pseudobulk_file`` and ``silhouette_file`` read as ``clusters_file`` - written as
        ``{species}_{tissue}_louvain.csv`` under ``save_path`` when given.  A cell without an edge has no community:
        ``WgnnError``.  ``normalize``: as for ``predict``."""
        return self._graph_clusters_file("louvain", data, save_path, k=k, resolution=resolution, weights=weights, normalize=normalize,
                                         space=space, metric=metric, max_sweeps=max_sweeps)

    def _graph_clusters_file(self, method, data, save_path, **kw):
        """``louvain_file`` / ``leiden_file``: the cut named ``method`` on a test file, every cell in a community."""
        matrix, genes, index = self._read_counts_file(data)
        out = getattr(self, method)(matrix, genes=genes, index=index, **kw)
        if (out.cluster < 0).any():
            raise WgnnError(f"{method}_file: {int((out.cluster < 0).sum())} cells have no edge in the graph and no community")
        return self._save_frame(out.clusters_frame(), save_path, method)

    def leiden(self, expr, k: int = 15, resolution=1.0, weights: str = "snn", genes=None, normalize=None, space: str = "hidden",
               metric: str = "euclidean", graph=None, max_sweeps: int = 256, index=None) -> Communities:
        """Leiden communities of a batch's own kNN graph: ``louvain``'s arguments, graph and weights, cut by ``ops.leiden_graph`` - a
        deterministic, synchronous Leiden in 64-bit integers.  Between a level's moving phase and its aggregation a refinement
        rebuilds every community from singletons, and only what that refinement joined becomes a vertex of the next level; the
        last cut is split into its connected components.  So every community is connected on the graph that was cut, which
        ``louvain`` does not promise: a disconnected community is two populations under one name, and ``annotate`` /
        ``pseudobulk`` / ``rank_genes`` / ``silhouette`` would inherit the mistake.  Two calls give the same bits.

        Returns a ``Communities`` with ``method == "leiden"``, used downstream exactly as ``louvain``'s.

        What this is not: the published Leiden's randomised refinement (no theta, no random number); no CPM or other quality
        function than modularity; one pass, no repeated outer iterations - feeding a result back as the start partition is the
        obvious follow-up; it does not claim a higher modularity than ``louvain`` (measured: 0.99 to 1.005 of it).  The rest as
        ``louvain``: one batch only (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table)."""
        return self._graph_clusters("leiden", expr, k, resolution, weights, genes, normalize, space, metric, graph, max_sweeps, index)

    def leiden_file(self, data, k: int = 15, resolution=1.0, weights: str = "snn", normalize=None, space: str = "hidden",
                    metric: str = "euclidean", max_sweeps: int = 256, save_path=None) -> pd.DataFrame:
        """``leiden`` on a test file, as ``louvain_file``: one row per cell - a running number, ``cell`` and ``cluster`` - the layout
        ``annotate_file``, ``pseudobulk_file`` and ``silhouette_file`` read as ``clusters_file``, written as
        ``{species}_{tissue}_leiden.csv`` under ``save_path`` when given.  A cell without an edge has no community: ``WgnnError``."""
        return self._graph_clusters_file("leiden", data, save_path, k=k, resolution=resolution, weights=weights, normalize=normalize,
                                         space=space, metric=metric, max_sweeps=max_sweeps)

    # ---------------------------------------------------------------------------------------------
    def umap(self, expr, k: int = 15, min_dist: float = 0.1, spread: float = 1.0, a=None, b=None, n_epochs: Optional[int] = None,
             n_neg: int = 5, seed: int = 0, init="pca", genes=None, normalize=None, space: str = "hidden",
             metric: str = "euclidean", graph=None, index=None) -> Layout:
        """A 2-D layout of a batch from the fuzzy graph of its own kNN lists - the picture the calls and clusters are drawn on -
        without a host round trip: the batch is classified once (``classify``'s call, bit for bit), searched as ``knn`` does
        (``k``, ``space``, ``metric`` as there), the lists and their distances made UMAP's connectivities (``ops.fuzzy_graph``)
        and laid out by ``ops.layout_graph``: UMAP's attraction along the edges and repulsion from ``n_neg`` hashed draws per
        firing edge, applied synchronously - every epoch reads the positions of the one before, every sum has a fixed order.
        ``a`` / ``b``: the curve, by default ``ops.layout_curve(min_dist, spread)`` (a scipy fit on the host); ``n_epochs`` =
        None: 500 below 10 000 cells, 200 from there on.  ``graph``: an earlier ``NeighborGraph`` of the same batch in place of
        the search - ``k``, ``space`` and ``metric`` are then the graph's own; a bare index array is refused, distances are
        needed.  ``index``: the cells' names.

        ``init``: ``"pca"`` - the first two principal components of the searched rows, scaled to max-abs 10 - is the ONE step not
        run by this project's kernels: mean, ``[D, D]`` covariance and projection are framework operations in float64 on the
        device with ``numpy.linalg.eigh`` on the host in between (each axis' sign fixed by its largest component), so its bits
        follow the installed libraries; ``"hash"`` (uniform in [-10, 10) from ``seed``) and a ``[B, 2]`` array start from
        stated bits, and for them two calls give the same bits.

        Returns a ``Layout``.  A cell without an edge (a NaN row, which ``knn`` lists nowhere) keeps its start position - the
        origin under ``"pca"`` - and has ``placed`` False.

        What this is not: not umap-learn's order of updates - there (Hogwild SGD) an edge moves both ends at once and later
        edges see the move, here a firing edge moves each end once, from that end's own row, off the previous epoch's
        positions; no spectral init, no ``transform`` of new cells, no 3-D, no supervised mode; one batch only
        (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table).  Fused kernels
        only, as ``embed``."""
        B = self._n_cells(expr)
        lists, k, space, metric = self._graph_lists(
            "the layout", graph, B, k, space, metric, True, max_k=_ops.FUZZY_MAX_K,
            misfit=f"graph must be a NeighborGraph of this batch: [{B}, 1..{_ops.FUZZY_MAX_K}] lists and distances")
        if n_epochs is not None and not 1 <= int(n_epochs) <= _ops.LAYOUT_MAX_EPOCHS:
            raise ValueError(f"n_epochs = {n_epochs} is outside [1, {_ops.LAYOUT_MAX_EPOCHS}]")
        if not 0 <= int(n_neg) <= _ops.LAYOUT_MAX_NEG:
            raise ValueError(f"n_neg = {n_neg} is outside [0, {_ops.LAYOUT_MAX_NEG}]")
        if not 0 <= int(seed) < 2 ** 32:
            raise ValueError(f"seed = {seed} is outside [0, 2^32)")
        if a is None or b is None:
            fit = _ops.layout_curve(min_dist, spread)
            a, b = fit[0] if a is None else a, fit[1] if b is None else b
        a, b = float(a), float(b)
        if not (0.0 < a < float("inf") and 0.0 < b < float("inf")):
            raise ValueError(f"a = {a} and b = {b} must be positive and finite")
        start = init
        if not isinstance(init, str):
            start = np.asarray(init)
            if start.shape != (B, 2) or start.dtype.kind not in "fiu" or not np.isfinite(start).all():
                raise ValueError(f"init must be 'pca', 'hash' or a finite array [{B}, 2]")
            start = start.astype(np.float32)
        elif init not in ("pca", "hash"):
            raise ValueError(f"init = {init!r}: pass 'pca', 'hash' or an array [{B}, 2]")
        self._require_fused("umap")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._umap(self._over_genes(expr, genes, normalize), k, a, b, n_epochs, int(n_neg), int(seed), start,
                              space, metric, lists, index)

    def _umap(self, expr, k, a, b, n_epochs, n_neg, seed, start, space, metric, lists, index):
        vb = self._values_batch(self._device_csr(expr))
        B = int(vb.csr[0].shape[0]) - 1
        pca = isinstance(start, str) and start == "pca"
        idx, d2, rows = self._lists_on_device(vb, lists, k, space, metric, want_rows=pca)      # "pca" embeds the batch once
        fuzzy = _ops.fuzzy_graph(idx, d2)
        if isinstance(start, str):
            how, y0 = start, (self._pca_start(rows) if start == "pca" else "hash")
        else:
            how, y0 = "array", torch.as_tensor(start, device=self.device)
        out = _ops.layout_graph(fuzzy.rowptr, fuzzy.col, fuzzy.w, y0, n_epochs=n_epochs, a=a, b=b, n_neg=n_neg, seed=seed)
        rowptr = fuzzy.rowptr.cpu().numpy()
        return Layout(coords=out.y.cpu().numpy(), placed=rowptr[1:] > rowptr[:-1], rho=fuzzy.rho.cpu().numpy(),
                      sigma=fuzzy.sigma.cpu().numpy(), rowptr=rowptr, col=fuzzy.col.cpu().numpy(), weight=fuzzy.w.cpu().numpy(),
                      a=a, b=b, n_epochs=out.n_epochs, n_fired=out.n_fired, seed=seed, init=how, k=k, space=space, metric=metric,
                      label=vb.pred, max_prob=vb.max_prob, **self._table_fields(B, index))

    @staticmethod
    def _pca_start(rows: torch.Tensor) -> torch.Tensor:
        """``umap``'s ``init="pca"``: the finite rows' first two principal components in float64 (framework operations and a host
        ``eigh``), each axis' sign fixed by its largest component, scaled to max-abs 10; a non-finite row sits at the origin."""
        x = rows.double()
        ok = torch.isfinite(x).all(dim=1)
        y = torch.zeros((x.shape[0], 2), dtype=torch.float64, device=x.device)
        if int(ok.sum()) > 0:
            centred = x[ok] - x[ok].mean(dim=0)
            cov = (centred.T @ centred / centred.shape[0]).cpu().numpy()
            axes = np.linalg.eigh(cov)[1][:, ::-1][:, :2]
            axes = axes * np.where(axes[np.abs(axes).argmax(axis=0), np.arange(2)] < 0, -1.0, 1.0)
            y[ok] = centred @ torch.from_numpy(np.ascontiguousarray(axes)).to(x.device)
            top = float(y.abs().max())
            if top > 0:
                y = y * (10.0 / top)
        return y.float()

    def umap_file(self, data, k: int = 15, min_dist: float = 0.1, spread: float = 1.0, a=None, b=None,
                  n_epochs: Optional[int] = None, n_neg: int = 5, seed: int = 0, init="pca", normalize=None,
                  space: str = "hidden", metric: str = "euclidean", save_path=None) -> pd.DataFrame:
        """``umap`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  Returns one row per cell:
        ``cell`` (its name), ``x`` and ``y`` - written as ``{species}_{tissue}_umap.csv`` under ``save_path`` when
        given.  A cell without an edge is written at its start position.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.umap(matrix, k=k, min_dist=min_dist, spread=spread, a=a, b=b, n_epochs=n_epochs, n_neg=n_neg, seed=seed,
                        init=init, genes=genes, normalize=normalize, space=space, metric=metric, index=index)
        return self._save_frame(out.coords_frame(), save_path, "umap")

    # ---------------------------------------------------------------------------------------------
    def _graph_lists(self, what, graph, B, k, space, metric, need_distances, max_k=_ops.SNN_MAX_K, misfit=None):
        """``graph=`` of the calls on a kNN graph, and their ``space`` / ``metric`` / ``k`` checks: ``(lists | None, k, space,
        metric)`` - ``lists`` the host ``(indices, sq_distances | None)`` of an earlier ``NeighborGraph`` of this batch (or, where
        no distances are needed, of a bare ``[B, k]`` index array), whose own ``k`` / ``space`` / ``metric`` then replace the
        call's.  ``what``: who needs the distances, in that refusal; ``max_k``: the caller's limit of ``k``; ``misfit``: the
        caller's own words for lists or distances that are not this batch's."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if metric not in KNN_METRICS:
            raise ValueError(f"metric = {metric!r}: pass one of {', '.join(map(repr, KNN_METRICS))}")
        if not 1 <= int(k) <= max_k:
            raise ValueError(f"k = {k} is outside [1, {max_k}]")
        if graph is None:
            return None, int(k), space, metric
        if need_distances and not isinstance(graph, NeighborGraph):
            raise ValueError(f"graph must be a NeighborGraph: {what} needs the neighbours' distances, which a bare index array "
                             "does not carry")
        idx = np.asarray(graph.indices if isinstance(graph, NeighborGraph) else graph)
        if idx.ndim != 2 or idx.shape[0] != B or not 1 <= idx.shape[1] <= max_k or idx.dtype.kind not in "iu":
            raise ValueError(misfit or f"graph must be a NeighborGraph or an integer array [{B}, 1..{max_k}] of this batch")
        d2 = None
        if isinstance(graph, NeighborGraph):
            space, metric = graph.space, graph.metric
            d2 = np.asarray(graph.sq_distances)
            if need_distances and d2.shape != idx.shape:
                raise ValueError(misfit or f"graph must be a NeighborGraph of this batch: its distances are {d2.shape}, its lists "
                                 f"{idx.shape}")
        return (idx, d2), int(idx.shape[1]), space, metric

    def _lists_on_device(self, vb, lists, k, space, metric, want_rows=False):
        """``(idx, d2, rows)`` on the device: ``knn``'s search of the classified batch ``vb``, or the host ``lists`` of
        ``_graph_lists``.  ``rows``: the embedded rows that were, or would have been, searched - embedded once - when the search
        ran or ``want_rows``, else None."""
        rows = None
        if lists is None or want_rows:
            rows = self._embed(vb.csr, space)
            if metric == "cosine":
                rows = F.normalize(rows, dim=1)
        if lists is None:
            return (*_ops.knn_rows(rows, k), rows)
        idx = torch.as_tensor(lists[0].astype(np.int64), device=self.device)
        return idx, None if lists[1] is None else torch.as_tensor(lists[1].astype(np.float32), device=self.device), rows

    def pseudotime(self, expr, root, k: int = 15, genes=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
                   graph=None, max_rounds: Optional[int] = None, index=None) -> Pseudotime:
        """Order the cells of a batch along its own kNN graph: every cell's geodesic distance from ``root`` - the shortest path
        over the graph's edges, each as long as the two cells are apart in the searched space - without a host round trip.  The
        batch is classified once (``classify``'s call, bit for bit), searched as ``knn`` does (``k``, ``space``, ``metric`` as
        there), the lists and their distances made a symmetric graph of edge lengths (``ops.distance_graph``) and walked by
        ``ops.geodesic_rows``: a synchronous Bellman-Ford in float32, one individually rounded add per edge and round, so that two
        calls give the same bits.  This is Monocle 3's ``order_cells`` on a kNN graph, and what ``scipy.sparse.csgraph.dijkstra``
        would give on ``knn().to_scipy()`` made symmetric, up to one float32 rounding per hop.

        ``root``: a cell's position, a sequence of positions (the distance is then to the nearest of them), a cell's name when
        ``index`` is given, or ``{"type": "<a called type's name>"}`` - that type's most confident cell (the highest
        ``max_prob``, ties to the lowest position; ``ValueError`` if no cell has that call).  ``graph``: an earlier
        ``NeighborGraph`` of the same batch in place of the search - ``k``, ``space`` and ``metric`` are then the graph's own; a
        bare index array is refused, distances are needed.  ``max_rounds`` (None = the number of cells): a cap on the rounds;
        ``converged`` says whether it was hit.  ``index``: the cells' names.

        Returns a ``Pseudotime``.  A cell in another component than every root (a NaN row, which ``knn`` lists nowhere, among
        them) is not reached: ``distance`` +inf, ``pseudotime`` NaN.

        What this is not: geodesic distance, not diffusion pseudotime (scanpy's ``tl.dpt`` averages over all paths, this takes
        the shortest); no branch detection - ``paga`` and ``Abstraction.directed`` are the coarse view of the branches; the
        lengths are distances in the searched space, so ``space="hidden"`` orders the cells as the classifier sees them
        (``space="features"`` is the view no trained weight takes part in); one batch only
        (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table); the cost is ``O(rounds x edges)``
        where ``rounds`` is the hop diameter from the root, which reaches the number of cells on a chain.  Fused kernels only, as
        ``embed``."""
        B = self._n_cells(expr)
        lists, k, space, metric = self._graph_lists("pseudotime", graph, B, k, space, metric, True)
        if max_rounds is not None and int(max_rounds) < 0:
            raise ValueError(f"max_rounds = {max_rounds} must not be negative")
        self._require_fused("pseudotime")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._pseudotime(self._over_genes(expr, genes, normalize), root, k, space, metric, lists, max_rounds, index)

    def _root_cells(self, root, B, index, pred, max_prob) -> np.ndarray:
        """``pseudotime``'s ``root`` as checked positions, ascending."""
        if isinstance(root, dict):
            if set(root) != {"type"}:
                raise ValueError(f"root = {root!r}: a dict root is {{'type': <a called type's name>}}")
            names = [str(n) for n in self.id2label]
            if str(root["type"]) not in names:
                raise ValueError(f"root type {root['type']!r} is no cell type of this bundle")
            own = np.nonzero(np.asarray(pred, np.int64) == names.index(str(root["type"])))[0]
            if own.size == 0:
                raise ValueError(f"root type {root['type']!r}: no cell of the batch has that call")
            return own[[int(np.argmax(np.asarray(max_prob)[own]))]].astype(np.int64)        # the first of equal maxima
        if isinstance(root, str) or (index is not None and not isinstance(root, (int, np.integer))
                                     and np.ndim(root) == 0 and not isinstance(root, torch.Tensor)):
            if index is None:
                raise ValueError(f"root = {root!r} names a cell: pass index= with the cells' names")
            at = [i for i, c in enumerate(index) if c == root or str(c) == str(root)]
            if len(at) != 1:
                raise ValueError(f"root = {root!r} names {len(at)} cells of index")
            return np.asarray(at, np.int64)
        cells = root.detach().cpu().numpy() if isinstance(root, torch.Tensor) else np.asarray(root)
        if cells.dtype.kind not in "iu" or cells.ndim > 1 or cells.size == 0:
            raise ValueError(f"root = {root!r}: pass a cell's position, a non-empty sequence of positions, a cell's name with "
                             "index=, or {'type': name}")
        cells = np.unique(cells.reshape(-1).astype(np.int64))
        if cells[0] < 0 or cells[-1] >= B:
            raise ValueError(f"root position out of range [0, {B})")
        return cells

    def _pseudotime(self, expr, root, k, space, metric, lists, max_rounds, index):
        vb = self._values_batch(self._device_csr(expr))
        B = int(vb.csr[0].shape[0]) - 1
        cells = self._root_cells(root, B, index, vb.pred, vb.max_prob)
        idx, d2, _ = self._lists_on_device(vb, lists, k, space, metric)
        out = _ops.geodesic_rows(*_ops.distance_graph(idx, d2), torch.as_tensor(cells, device=self.device), max_rounds=max_rounds)
        distance = out.dist.cpu().numpy()
        return Pseudotime(distance=distance, pseudotime=_scaled_pseudotime(distance), pred=out.pred.cpu().numpy().astype(np.int64),
                          root=cells, reached=out.reached, rounds=out.rounds, converged=out.converged, k=k, space=space,
                          metric=metric, label=vb.pred, max_prob=vb.max_prob, **self._table_fields(B, index))

    def pseudotime_file(self, data, root, k: int = 15, normalize=None, space: str = "hidden", metric: str = "euclidean",
                        max_rounds: Optional[int] = None, save_path=None) -> pd.DataFrame:
        """``pseudotime`` on a test file - its full table, its gene names as ``genes=`` and its cell names (so ``root`` may name a
        cell).  Returns one row per cell: ``cell`` (its name) and ``pseudotime`` - empty where the cell was not reached, which is
        no error - written as ``{species}_{tissue}_pseudotime.csv`` under ``save_path`` when given.  ``normalize``: as for
        ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.pseudotime(matrix, root, k=k, genes=genes, normalize=normalize, space=space, metric=metric,
                              max_rounds=max_rounds, index=index)
        return self._save_frame(out.pseudotime_frame(), save_path, "pseudotime")

    def paga(self, expr, groups="predicted", k: int = 15, genes=None, normalize=None, space: str = "hidden",
             metric: str = "euclidean", graph=None, group_names: Optional[Sequence[str]] = None, n_groups: Optional[int] = None,
             index=None) -> Abstraction:
        """How do groups of cells hang together on the batch's own kNN graph?  The PAGA connectivity (Wolf et al. 2019) of every
        pair of groups: the batch is classified once (``classify``'s call, bit for bit), searched as ``knn`` does, and the
        directed list entries are counted per pair of groups on the device (``ops.group_edges``: integer counts); a pair's
        connectivity is the entries between the two groups over what a random wiring of the same out-degrees would put there,
        ``(e[a, b] + e[b, a]) (n - 1) / (es[a] ns[b] + es[b] ns[a])`` capped at 1 - one fp64 division of integers
        (``Abstraction`` has the tables).  This is scanpy's ``tl.paga`` connectivity, ``model="v1.2"``, as stated on the
        unit-weight directed kNN graph; the comparison with scanpy itself was not run.

        ``groups="predicted"``: the called types, unsure cells skipped; else one integer id per cell (-1 = skip) with
        ``group_names`` or ``n_groups``, as for ``silhouette`` - ``leiden``'s result feeds it as it comes:
        ``paga(expr, groups=lc.cluster, n_groups=lc.n_clusters, graph=g)``.  ``graph``: an earlier ``NeighborGraph`` of the same
        batch, or a ``[B, k]`` index array (counts need no distances), in place of the search.  At most 4096 groups.

        Returns an ``Abstraction``: ``tree`` / ``frame`` / ``centroids`` / ``directed`` / ``summary`` on top.

        What this is not: no connectivities of a weighted (UMAP) graph - every list entry counts 1; no ``model="v1.0"``; no
        thresholding or layout of the abstracted graph (``centroids`` puts the groups on a ``umap``); no transitions from RNA
        velocity - ``directed`` orients the pairs by ``pseudotime`` alone; one batch only
        (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table).  Fused kernels only, as ``embed``."""
        B = self._n_cells(expr)
        lists, k, space, metric = self._graph_lists("paga", graph, B, k, space, metric, False)
        self._require_fused("paga")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._paga(self._over_genes(expr, genes, normalize), groups, group_names, n_groups, k, space, metric, lists)

    def _paga(self, expr, groups, group_names, n_groups, k, space, metric, lists):
        predicted, names = self._group_names(groups, group_names, n_groups)
        K = len(names)
        if K > _ops.GROUP_EDGES_MAX_GROUPS:
            raise ValueError(f"{K} groups: paga takes at most {_ops.GROUP_EDGES_MAX_GROUPS}")
        device_csr = self._device_csr(expr)
        B = int(device_csr[0].shape[0]) - 1
        if not predicted:
            ids = self._group_ids(groups, B, K)
        vb = self._values_batch(device_csr)
        group = np.asarray(vb.pred if predicted else ids, np.int64)
        group = np.where(group >= 0, group, -1)
        idx, _, _ = self._lists_on_device(vb, lists, k, space, metric)
        out = _ops.group_edges(idx, torch.from_numpy(group).to(self.device), K)
        edges, size = out.edges.cpu().numpy(), out.size.cpu().numpy()
        out_edges, expected, conn = _paga_connectivities(edges, size)
        return Abstraction(edges=edges, size=size, out_edges=out_edges, connectivities=conn, expected=expected, group_names=names,
                           n_skipped=int((group < 0).sum()), group=group, k=k, space=space, metric=metric)

    def paga_file(self, data, clusters_file=None, k: int = 15, normalize=None, space: str = "hidden", metric: str = "euclidean",
                  save_path=None) -> pd.DataFrame:
        """``paga`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  ``clusters_file``: a
        clusters file laid out as ``annotate_file`` reads it - what ``kmeans_file`` / ``louvain_file`` / ``leiden_file`` write;
        ``None``: the predicted types.  Returns ``Abstraction.frame()``, written as ``{species}_{tissue}_paga.csv`` under
        ``save_path`` when given.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        kw = dict(k=k, genes=genes, normalize=normalize, space=space, metric=metric, index=index)
        if clusters_file is None:
            out = self.paga(matrix, **kw)
        else:
            ids, names = _cluster_ids(self._read_clusters_file(clusters_file, data, index), n_cells=len(index))
            out = self.paga(matrix, groups=ids, group_names=names, **kw)
        return self._save_frame(out.frame(), save_path, "paga")

    # ---------------------------------------------------------------------------------------------
    def diffmap(self, expr, n_comps: int = 15, k: int = 15, genes=None, normalize=None, space: str = "hidden",
                metric: str = "euclidean", graph=None, n_steps: Optional[int] = None, seed: int = 0, tol: float = 1e-8,
                index=None) -> DiffusionMap:
        """The diffusion map of a batch's own kNN graph - the leading eigenvectors of its density-normalised transition matrix,
        scanpy's ``tl.diffmap`` - without a host round trip of the graph: the batch is classified once (``classify``'s call, bit
        for bit), searched as ``knn`` does (``k``, ``space``, ``metric`` as there), the lists and their distances made UMAP's
        connectivities (``ops.fuzzy_graph``, the graph ``umap`` lays out), these made the symmetric transition matrix
        (``ops.diffusion_operator``) and its largest connected component (``ops.graph_components``; ties in size go to the
        component that holds the lowest cell) handed to ``ops.lanczos_graph``: a Lanczos iteration with full
        re-orthogonalisation and a fixed number of steps, every sum in a stated order, so that two calls give the same bits.
        The small tridiagonal problem is solved on the host (``ops.lanczos_ritz``: ``numpy.linalg.eigh``) and the eigenvectors
        are put together on the device (``ops.basis_combine``), each with the sign that makes its largest entry positive.

        ``n_comps`` in [2, 64] counts the stationary component 0, as scanpy does.  ``n_steps`` = None: 128 below 10 000 cells,
        256 from there on; at most 1024.  ``seed``: of the start vector.  ``tol``: what ``converged`` holds the residuals to.
        ``graph``: an earlier ``NeighborGraph`` of the same batch in place of the search - ``k``, ``space`` and ``metric`` are
        then the graph's own; a bare index array is refused, distances are needed.  ``index``: the cells' names.

        Returns a ``DiffusionMap``.  Fewer components than asked for (a small component, a breakdown) are reported, not raised;
        a cell outside the component (a NaN row, which ``knn`` lists nowhere, among them) has NaN coordinates.

        What this is not: no Gaussian-kernel connectivities (scanpy's ``method="gauss"``) - the weights are UMAP's; no restarts,
        so a residual above ``tol`` is reported (``converged`` False) and the caller raises ``n_steps``; one component, one batch
        (cells of several samples: ``bbknn`` lists neighbours per sample, and ``graph=`` takes its table);
        an eigenvalue within about ``tol`` of another gives a basis of that eigenspace, not scanpy's particular vectors; the
        comparison with scanpy itself was not run, the formulas of ``include/wgnn.h`` are the contract.  Fused kernels only, as
        ``embed``."""
        B = self._n_cells(expr)
        lists, k, space, metric = self._graph_lists(
            "the diffusion map", graph, B, k, space, metric, True, max_k=_ops.FUZZY_MAX_K,
            misfit=f"graph must be a NeighborGraph of this batch: [{B}, 1..{_ops.FUZZY_MAX_K}] lists and distances")
        n_comps, seed, tol = int(n_comps), int(seed), float(tol)
        if not 2 <= n_comps <= _ops.DIFFUSION_MAX_COMPS:
            raise ValueError(f"n_comps = {n_comps} is outside [2, {_ops.DIFFUSION_MAX_COMPS}]")
        if n_steps is not None and not 1 <= int(n_steps) <= _ops.LANCZOS_MAX_STEPS:
            raise ValueError(f"n_steps = {n_steps} is outside [1, {_ops.LANCZOS_MAX_STEPS}]")
        if not 0 <= seed < 2 ** 32:
            raise ValueError(f"seed = {seed} is outside [0, 2^32)")
        if not 0.0 <= tol < float("inf"):
            raise ValueError(f"tol = {tol} must be finite and not negative")
        self._require_fused("diffmap")
        _check_index(index, B)
        with torch.cuda.device(self.device), torch.no_grad():
            return self._diffmap(self._over_genes(expr, genes, normalize), n_comps, k, space, metric, lists, n_steps, seed, tol,
                                 index)

    def _diffmap(self, expr, n_comps, k, space, metric, lists, n_steps, seed, tol, index):
        vb = self._values_batch(self._device_csr(expr))
        B = int(vb.csr[0].shape[0]) - 1
        idx, d2, _ = self._lists_on_device(vb, lists, k, space, metric)
        fuzzy = _ops.fuzzy_graph(idx, d2)
        lowest = _ops.graph_components(fuzzy.rowptr, fuzzy.col)
        size = torch.bincount(lowest, minlength=B)
        mask = lowest == torch.nonzero(size == size.max())[0, 0] if B else lowest == 0      # the first of the largest
        op = _ops.diffusion_operator(fuzzy.rowptr, fuzzy.col, fuzzy.w)
        run = _ops.lanczos_graph(fuzzy.rowptr, fuzzy.col, op.t, op.z, mask, n_steps=n_steps, seed=seed)
        theta, S, res = _ops.lanczos_ritz(run.alpha, run.beta, run.n_run)
        n_found = min(n_comps, run.n_run + 1)
        on = mask.cpu().numpy()
        coords = _ops.basis_combine(run.V, S[:, :n_found - 1]).cpu().numpy()
        coords[~on] = np.nan
        residual = np.concatenate([[0.0], res[:n_found - 1]])
        return DiffusionMap(coords=coords, eigenvalues=np.concatenate([[1.0], theta[:n_found - 1]]), residual=residual,
                            converged=bool((residual <= tol).all()), tol=tol, n_steps=run.n_run, breakdown=run.breakdown,
                            in_component=on, n_components=int((size > 0).sum()), seed=seed, k=k, space=space, metric=metric,
                            label=vb.pred, max_prob=vb.max_prob, **self._table_fields(B, index))

    def diffmap_file(self, data, n_comps: int = 15, k: int = 15, normalize=None, space: str = "hidden", metric: str = "euclidean",
                     n_steps: Optional[int] = None, seed: int = 0, tol: float = 1e-8, save_path=None) -> pd.DataFrame:
        """``diffmap`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  Returns one row per cell:
        ``cell`` (its name), ``dc1``, ``dc2``, ... - empty where the cell lies outside the component, which is no error - written
        as ``{species}_{tissue}_diffmap.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.diffmap(matrix, n_comps=n_comps, k=k, genes=genes, normalize=normalize, space=space, metric=metric,
                           n_steps=n_steps, seed=seed, tol=tol, index=index)
        return self._save_frame(out.coords_frame(), save_path, "diffmap")

    def dpt(self, expr, root, n_dcs: int = 10, diffmap: Optional[DiffusionMap] = None, n_comps: int = 15, k: int = 15, genes=None,
            normalize=None, space: str = "hidden", metric: str = "euclidean", graph=None, n_steps: Optional[int] = None,
            seed: int = 0, tol: float = 1e-8, index=None) -> DiffusionPseudotime:
        """Order the cells of a batch by diffusion pseudotime (Haghverdi et al. 2016, scanpy's ``tl.dpt`` without branchings):
        every cell's distance from ``root`` in the diffusion map, ``sqrt(sum_l (lambda_l / (1 - lambda_l))^2 (y_l[root] -
        y_l[cell])^2)`` over the components ``l = 1 .. n_dcs - 1`` - the sum of the transition matrix's powers, which averages
        over every path of the graph where ``pseudotime`` takes the shortest, so that one spurious edge across a gap does not
        short-cut the order.  ``ops.diffusion_distance`` on the device, the sum sequential and every operation rounded on its
        own; ``lambda / (1 - lambda)`` is taken on the host in float64.

        ``root``: as ``pseudotime`` takes it - a cell's position, a sequence of positions (the distance is then to the nearest
        of them), a cell's name when ``index`` is given, or ``{"type": "<a called type's name>"}``; a root outside the
        component is a ``ValueError``.  ``n_dcs`` in [2, the components found] counts the stationary component, as ``n_comps``.
        ``diffmap``: an earlier ``DiffusionMap`` of this batch - nothing is classified or searched then, and the other
        arguments of ``diffmap`` are not read; else ``diffmap`` runs with them.

        Returns a ``DiffusionPseudotime``: ``distance`` and ``pseudotime`` are NaN for a cell outside the component.

        What this is not: no branch detection (scanpy's ``n_branchings``) - ``paga`` and ``Abstraction.directed``, which takes
        this table as it takes ``pseudotime``'s, are the coarse view of the branches; and what ``diffmap`` is not.  Fused kernels
        only, as ``embed``."""
        B = self._n_cells(expr)
        _check_index(index, B)
        if diffmap is None:
            diffmap = self.diffmap(expr, n_comps=n_comps, k=k, genes=genes, normalize=normalize, space=space, metric=metric,
                                   graph=graph, n_steps=n_steps, seed=seed, tol=tol, index=index)
        elif not isinstance(diffmap, DiffusionMap) or len(diffmap.in_component) != B:
            raise ValueError(f"diffmap must be a DiffusionMap of this batch of {B} cells")
        n_dcs = int(n_dcs)
        if not 2 <= n_dcs <= diffmap.n_found:
            raise ValueError(f"n_dcs = {n_dcs} is outside [2, {diffmap.n_found}] (the components found)")
        cells = self._root_cells(root, B, index, diffmap.label, diffmap.max_prob)
        outside = cells[~np.asarray(diffmap.in_component, bool)[cells]]
        if outside.size:
            raise ValueError(f"root cell(s) {outside.tolist()} lie outside the component the diffusion map was taken on")
        self._require_fused("dpt")
        lam = np.asarray(diffmap.eigenvalues, np.float64)[:n_dcs]
        with np.errstate(divide="ignore", invalid="ignore"):
            g = lam / (1.0 - lam)
        g[0] = 0.0                                                              # the stationary component is not read
        with torch.cuda.device(self.device), torch.no_grad():
            Y = torch.as_tensor(np.ascontiguousarray(np.asarray(diffmap.coords, np.float64)[:, :n_dcs]), device=self.device)
            distance = _ops.diffusion_distance(Y, g, torch.as_tensor(cells, device=self.device)).cpu().numpy()
        return DiffusionPseudotime(distance=distance, pseudotime=_scaled_pseudotime(distance), roots=cells, n_dcs=n_dcs,
                                   label=diffmap.label, max_prob=diffmap.max_prob,
                                   index=diffmap.index if index is None else index, id2label=list(diffmap.id2label),
                                   label_map=diffmap.label_map)

    def dpt_file(self, data, root, n_dcs: int = 10, n_comps: int = 15, k: int = 15, normalize=None, space: str = "hidden",
                 metric: str = "euclidean", n_steps: Optional[int] = None, seed: int = 0, tol: float = 1e-8,
                 save_path=None) -> pd.DataFrame:
        """``dpt`` on a test file - its full table, its gene names as ``genes=`` and its cell names (so ``root`` may name a cell).
        Returns one row per cell: ``cell`` (its name) and ``pseudotime`` - empty where the cell lies outside the component, which
        is no error - written as ``{species}_{tissue}_dpt.csv`` under ``save_path`` when given.  ``normalize``: as for
        ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.dpt(matrix, root, n_dcs=n_dcs, n_comps=n_comps, k=k, genes=genes, normalize=normalize, space=space,
                       metric=metric, n_steps=n_steps, seed=seed, tol=tol, index=index)
        return self._save_frame(out.pseudotime_frame(), save_path, "dpt")

    # ---------------------------------------------------------------------------------------------
    def silhouette(self, expr, groups="predicted", genes=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
                   group_names: Optional[Sequence[str]] = None, n_groups: Optional[int] = None, index=None) -> Silhouette:
        """How well are groups of cells separated in the model's space?  The exact silhouette (Rousseeuw 1987) of every cell,
        on the device: the batch is classified once (``classify``'s call, bit for bit), embedded (``embed``, ``space`` as there)
        and scored by ``wgnn_silhouette_rows`` - brute force over every ordered pair of cells, the ``[B, B]`` distance matrix
        never stored, a cell's distances summed per group in fp64 in a fixed order.  Per cell ``a`` is the mean distance to the
        other cells of its own group, ``b`` the lowest mean distance to another group (``nearest``) and ``score = (b - a) /
        max(a, b)``: near 1 the cell sits inside its group, below 0 it sits closer to ``nearest``.
        ``groups="predicted"``: the called types, unsure cells skipped; else one integer id per cell (-1 = skip) with
        ``group_names`` or ``n_groups``, as for ``rank_genes`` - ``kmeans``' result feeds it as it comes:
        ``silhouette(expr, groups=km.cluster, n_groups=K, space=km.space, metric=km.metric)``.  ``metric="cosine"``: the rows are
        L2-normalised first, as ``knn`` and ``kmeans`` do, and the distances are then EUCLIDEAN distances of unit rows,
        ``sqrt(2 (1 - cos))`` - not ``1 - cos``.  A cell whose embedding holds a non-finite value takes no part.  At most 4096
        groups; fewer than two non-empty groups raise ``ValueError``.  ``index``: the cells' names.

        Returns a ``Silhouette``: ``mean`` / ``by_group`` / ``misplaced`` / ``frame`` / ``summary`` on top.  Two calls give the
        same bits.  To choose ``n_clusters``, loop ``kmeans`` and this over K and keep the highest ``mean()`` - inertia falls
        with every K and cannot choose.

        In ``space="hidden"`` with ``groups="predicted"`` this is the classifier judging itself: the hidden rows are what the
        head separates, so the called types score high there by construction.  ``space="features"`` is the independent view -
        no trained weight takes part.

        What this is not: no sampling - the cost is exact ``O(B^2 D)``; no simplified (centroid) silhouette; one batch only;
        no automatic K sweep.  Fused kernels only, as ``embed``."""
        if space not in KNN_SPACES:
            raise ValueError(f"space = {space!r}: pass one of {', '.join(map(repr, KNN_SPACES))}")
        if metric not in KNN_METRICS:
            raise ValueError(f"metric = {metric!r}: pass one of {', '.join(map(repr, KNN_METRICS))}")
        self._require_fused("silhouette")
        _check_index(index, self._n_cells(expr))
        with torch.cuda.device(self.device), torch.no_grad():
            return self._silhouette(self._over_genes(expr, genes, normalize), groups, group_names, n_groups, space, metric, index)

    def _silhouette(self, expr, groups, group_names, n_groups, space, metric, index):
        predicted, names = self._group_names(groups, group_names, n_groups)
        K = len(names)
        if K > _ops.SILHOUETTE_MAX_GROUPS:
            raise ValueError(f"{K} groups: silhouette takes at most {_ops.SILHOUETTE_MAX_GROUPS}")
        device_csr = self._device_csr(expr)
        B = int(device_csr[0].shape[0]) - 1
        if not predicted:
            ids = self._group_ids(groups, B, K)
        vb = self._values_batch(device_csr)
        group = np.asarray(vb.pred if predicted else ids, np.int64)
        if len(set(group[group >= 0].tolist())) < 2:       # the host holds the ids: no read-back
            raise ValueError("silhouette needs at least two non-empty groups")
        rows = self._embed(vb.csr, space)[:, :self.hidden if space == "hidden" else None]       # embed's rows
        if metric == "cosine":
            rows = F.normalize(rows, dim=1)
        out = _ops.silhouette_rows(rows, torch.from_numpy(group).to(self.device), K)
        group = np.where(torch.isfinite(rows).all(dim=1).cpu().numpy(), group, -1)      # a row with a non-finite value took no part
        return Silhouette(a=out.a.cpu().numpy(), b=out.b.cpu().numpy(), score=out.score.cpu().numpy(),
                          nearest=out.nearest.cpu().numpy().astype(np.int64), group=group,
                          group_names=names, size=out.size.cpu().numpy(), n_skipped=int((group < 0).sum()), space=space,
                          metric=metric, label=vb.pred, max_prob=vb.max_prob, **self._table_fields(B, index))

    def silhouette_file(self, data, clusters_file=None, normalize=None, space: str = "hidden", metric: str = "euclidean",
                        save_path=None) -> pd.DataFrame:
        """``silhouette`` on a test file - its full table, its gene names as ``genes=`` and its cell names.  ``clusters_file``:
        a clusters file laid out as ``annotate_file`` reads it (an index column, the cell's name, its cluster's name; the
        cells in the data file's order, else ``ValueError``; the names compared as stripped ``str``, in sorted order) -
        ``kmeans_file``'s output is one; ``None``: the predicted types.  Returns ``Silhouette.frame()``, written as
        ``{species}_{tissue}_silhouette.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        kw = dict(genes=genes, normalize=normalize, space=space, metric=metric, index=index)
        if clusters_file is None:
            out = self.silhouette(matrix, **kw)
        else:
            ids, names = _cluster_ids(self._read_clusters_file(clusters_file, data, index), n_cells=len(index))
            out = self.silhouette(matrix, groups=ids, group_names=names, **kw)
        return self._save_frame(out.frame(), save_path, "silhouette")

    # ---------------------------------------------------------------------------------------------
    def pseudobulk(self, expr, genes, clusters, normalize=None, cluster_names: Optional[Sequence[str]] = None,
                   n_clusters: Optional[int] = None, into: Optional[Pseudobulk] = None) -> Pseudobulk:
        """One PROFILE per cluster, and the call on it: the raw counts of all cells of a cluster (a sample, a metacell) are
        added on the device (``wgnn_pool_rows_accumulate``: integer sums, exact in any order), the pooled row is log-normalised
        against the cluster's summed library size (``wgnn_pool_rows_count`` / ``_fill``) and goes through the predictor's own
        ``classify`` path - every layer, either route.  A cluster's call is therefore ``classify(..., normalize="lognorm")`` of
        the host-summed count row with one more column holding the reads outside the bundle; shallow cells whose own calls fall
        apart (``stability(thin="reads")``) are called together.  Returns a ``Pseudobulk``: the calls, the pooled value CSR and
        the pooled integer counts (``counts()``: what pseudobulk differential expression takes), ``frame`` / ``summary`` on top.

        The batch holds raw integer COUNTS: ``genes=`` and a ``normalize`` spec are required exactly as ``doublets`` requires
        them (else ``ValueError``), a ``GeneMap`` with merged columns raises ``ValueError``, a count that is no integer in
        [1, 2^23] raises ``WgnnError`` naming the cell.  The genes may come in any order.  ``clusters``, ``cluster_names`` and
        ``n_clusters`` as ``annotate`` takes them: one integer id per cell (-1 = skip), or one ``str`` name per cell - factorised
        in sorted order, or matched against ``into``'s names.  Choosing the clusters or metacells is the caller's.

        ``into``: an earlier ``Pseudobulk`` of the same bundle and cluster names; this batch is pooled ON TOP of it, the
        clusters are classified again, and ``into`` is returned: two halves of a cohort equal the whole, bit for bit.  It needs
        the predictor's ``threshold`` to be 0 (a pooled row that dropped entries cannot be added to)."""
        spec = self._count_spec(genes, normalize, "pseudobulk")
        if into is not None and not isinstance(into, Pseudobulk):
            raise ValueError("into: pass an earlier Pseudobulk")
        ids, names = _cluster_ids(clusters, cluster_names, n_clusters, into=into,
                                  n_cells=self._n_cells(expr))
        if into is not None:
            into._require_same(names, self.id2label, self.id2gene)
            if float(self.threshold) > 0:
                raise ValueError("into: needs a predictor threshold of 0 (entries at or below it were dropped from the profiles)")
        with torch.cuda.device(self.device), torch.no_grad():
            return self._pseudobulk(expr, genes, spec, ids, names, into)

    def _pseudobulk(self, expr, genes, spec, ids, names, into):
        dev = self.device
        cb = self._count_batch(expr, genes, spec, "pseudobulk", full_call=False,
                               pair_check="pseudobulk adds up to 256 cells' counts in a 32-bit partial sum")
        (rowptr, col, cnt), lib = cb.csr, cb.lib
        group = torch.from_numpy(ids.astype(np.int32)).to(dev)
        seed = None if into is None else (into.rowptr, into.col, into.cnt, torch.from_numpy(np.asarray(into.n_reads, np.int64)).to(dev),
                                          torch.from_numpy(np.asarray(into.n_cells, np.int64)).to(dev))
        p_rowptr, p_col, p_val, p_cnt, total, n_cells = _ops.pool_rows(
            rowptr, col, cnt, lib, group, len(names), scale=float(spec.scale_factor), threshold=float(self.threshold), seed=seed,
            n_genes=self.n_genes)
        pred, max_prob, logits, _ = self._classify_on_device(_Aligned((p_rowptr, p_col, p_val)))
        fields = dict(n_cells=n_cells.cpu().numpy(), n_reads=total.cpu().numpy(), n_genes=np.diff(p_rowptr.cpu().numpy()),
                      label=pred, max_prob=np.asarray(max_prob, np.float32), logits=logits, rowptr=p_rowptr, col=p_col, val=p_val,
                      cnt=p_cnt)
        if into is None:
            return Pseudobulk(names=list(names), id2label=list(self.id2label), id2gene=list(self.id2gene),
                              label_map=self._label_names(), **fields)
        for name, value in fields.items():
            setattr(into, name, value)
        return into

    def pseudobulk_file(self, input_file, clusters_file, normalize="lognorm", save_path=None) -> pd.DataFrame:
        """``pseudobulk`` on a test file of raw counts (its full table and gene names) and a clusters file laid out as
        ``annotate_file`` takes it (an index column, the cell's name, its cluster's name; the cells in the data file's order,
        else ``ValueError``): ``Pseudobulk.frame()``, written as ``{species}_{tissue}_pseudobulk.csv`` under ``save_path`` when
        given.  Cluster names are compared as stripped ``str`` and come in sorted order."""
        matrix, genes, index = self._read_counts_file(input_file)
        clusters = self._read_clusters_file(clusters_file, input_file, index)
        return self._save_frame(self.pseudobulk(matrix, genes, clusters, normalize=normalize).frame(), save_path, "pseudobulk")

    # ---------------------------------------------------------------------------------------------
    def explain(self, expr, top_k: int = 10, target="predicted", genes=None, normalize=None) -> "Attribution":
        """Which genes made the model say so: the target logit of every cell split, without approximation, into one share
        per expressed gene plus a bias share (``sum(scores of the cell) + base == logit``; ``include/wgnn.h``,
        ``wgnn_attrib_rows``).  ``expr`` as ``classify`` takes it.  ``target``: ``"predicted"`` (the arg max, also for a
        cell that comes out unsure), a class id, a label string, or one class id per cell.  ``top_k`` in 0..64: the
        highest-scoring genes per cell (0 = scores only).  Cells are independent, so there is no graph route.  ``genes``: as
        for ``classify``; the scores then follow ``align``'s entries (gene ids of the bundle, the caller's order).
        ``normalize``: as for ``align`` (needs ``genes``)."""
        with torch.cuda.device(self.device), torch.no_grad():
            return self._explain(self._over_genes(expr, genes, normalize), top_k, target)

    def _target_ids(self, target, n_cells: int) -> Optional[torch.Tensor]:
        """``explain``'s ``target`` as None (the predicted class) or an int32 device vector with one class per cell."""
        if isinstance(target, str):
            if target == "predicted":
                return None
            if target not in self.id2label:
                raise ValueError(f"target {target!r} is not a cell type of this bundle ({len(self.id2label)} types)")
            target = self.id2label.index(target)
        if isinstance(target, (int, np.integer)):
            ids = np.full(n_cells, int(target), np.int64)
        else:
            ids = (target.detach().cpu().numpy() if isinstance(target, torch.Tensor) else np.asarray(target)).astype(np.int64)
            if ids.shape != (n_cells,):
                raise ValueError(f"target lists {ids.shape} classes, the batch holds {n_cells} cells")
        if ids.size and (ids.min() < 0 or ids.max() >= self.n_classes):
            raise ValueError(f"target class out of range [0, {self.n_classes})")
        return torch.from_numpy(ids.astype(np.int32)).to(self.device)

    def _explain(self, expr, top_k, target):
        if not 0 <= int(top_k) <= 64:
            raise ValueError(f"top_k = {top_k} is outside [0, 64]")
        Hp, L = self.hidden_padded, self.n_layers
        if Hp > 256:
            raise WgnnError(f"explain: hidden width {self.hidden} > 256 is not built (WGNN_ERR_UNSUPPORTED)")
        if self.n_classes * Hp * 4 > _ops.HEAD_LDS_BYTES:
            raise WgnnError(f"explain: a [{self.n_classes}, {Hp}] head does not fit the kernel's LDS (WGNN_ERR_UNSUPPORTED)")
        rowptr, col, raw, checked, _ = self._device_csr(expr)
        if int(col.shape[0]) >= 2 ** 31:
            raise WgnnError("explain: nnz >= 2^31 (split the batch)")
        B = rowptr.shape[0] - 1
        tgt = self._target_ids(target, B)
        # forward below the last layer (h_1 .. h_{L-1}), then the last layer's head-mode launch
        hs = []
        for l in range(L - 1):
            self_rows = None if l == 0 else _ops.linear_fwd(hs[-1], self.self_weights[l])
            hs.append(_ops.predict_rows(rowptr, col, raw, self.tables[l], self.alpha, self.biases[l], self_rows=self_rows,
                                        check_cols=not checked and l == 0))
        self_rows = None if L == 1 else _ops.linear_fwd(hs[-1], self.self_weights[L - 1])
        scores, t_out, logit, base, label, v = _ops.attrib_rows(
            rowptr, col, raw, self.tables[L - 1], self.alpha, self.biases[L - 1], head=(self.w_head, self.b_head), target=tgt,
            self_rows=self_rows, unsure_threshold=self.unsure_threshold, want_direction=L > 1,
            check_cols=not checked and L == 1)
        if L > 1:
            deg = (rowptr[1:] - rowptr[:-1]).to(torch.float32)
            back = (self.alpha[self.n_genes + 1] / (deg + 1.0)).unsqueeze(1)
            widen = lambda t: t if t.shape[1] == Hp else F.pad(t, (0, Hp - t.shape[1]))      # the tables' padded width
            v = widen(v)
            for l in range(L - 1, 0, -1):                    # v_l = (h_l > 0) * (v_{l+1} . W_{l+1}) * alpha[G+1] / (deg + 1)
                v = widen(hs[l - 1] > 0) * _ops.linear_fwd(v.contiguous(), self.self_weights[l].t().contiguous()) * back
                base = base + (v * self.biases[l - 1]).sum(dim=1)
                _ops.attrib_rows(rowptr, col, raw, self.tables[l - 1], self.alpha, self.biases[l - 1], direction=v,
                                 scores=scores, accumulate=True, explicit_self=l > 1, check_cols=False)
        if int(top_k) > 0:
            top_genes, top_scores = _ops.rows_topk(rowptr, col, scores, int(top_k))
            top_genes, top_scores = top_genes.cpu().numpy().astype(np.int64), top_scores.cpu().numpy()
        else:
            top_genes, top_scores = np.zeros((B, 0), np.int64), np.zeros((B, 0), np.float32)
        return Attribution(label=label.cpu().numpy().astype(np.int64), target=t_out.cpu().numpy().astype(np.int64),
                           logit=logit.cpu().numpy(), base=base.cpu().numpy(), scores=scores, top_genes=top_genes,
                           top_scores=top_scores, id2gene=self.id2gene)

    # ---------------------------------------------------------------------------------------------
    def markers(self, expr, groups="predicted", target="predicted", into: Optional[MarkerTable] = None,
                group_names: Optional[Sequence[str]] = None, n_groups: Optional[int] = None, genes=None,
                normalize=None) -> MarkerTable:
        """Which genes drive each group of cells across a cohort: ``explain``'s per-entry scores summed per (group, gene)
        on the device (``wgnn_group_gene_reduce``: fp64, deterministic), nothing per-entry leaves the GPU.  ``expr`` as
        ``classify`` takes it.  ``groups="predicted"``: a cell's group is its label from the same launch (unsure cells are
        skipped), named by ``id2label``; else one integer id per cell (-1 = skip) with ``group_names`` or ``n_groups`` -
        clusters, true labels, conditions.  ``target`` as for ``explain``.  ``into``: an earlier table of the same bundle
        and grouping, which this batch is ADDED to (and which is returned): a cohort of any size streams through.
        ``genes``: as for ``classify``; ``normalize``: as for ``align`` (needs ``genes``)."""
        with torch.cuda.device(self.device), torch.no_grad():
            return self._markers(self._over_genes(expr, genes, normalize), groups, target, into, group_names, n_groups)

    def _group_names(self, groups, group_names, n_groups) -> Tuple[bool, List[str]]:
        """``groups=`` of ``markers`` / ``rank_genes``: whether the groups are the predicted types, and the groups' names."""
        predicted = isinstance(groups, str)
        if predicted:
            if groups != "predicted":
                raise ValueError(f"groups = {groups!r}: pass \"predicted\" or one integer id per cell")
            names = list(self.id2label)
        else:
            if group_names is not None:
                names = list(group_names)
                if n_groups is not None and int(n_groups) != len(names):
                    raise ValueError(f"n_groups = {n_groups} but {len(names)} group names")
            elif n_groups is not None:
                names = [str(i) for i in range(int(n_groups))]
            else:
                raise ValueError("groups given per cell need group_names or n_groups")
            if not names:
                raise ValueError("no groups")
        return predicted, names

    @staticmethod
    def _group_ids(groups, B: int, K: int) -> np.ndarray:
        """Groups given per cell as a checked host vector: one integer id in [-1, K) per cell of the batch."""
        ids = groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
        if ids.shape != (B,):
            raise ValueError(f"groups lists {ids.shape} ids, the batch holds {B} cells")
        if not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"groups must be integer ids, got {ids.dtype}")
        if ids.size and (ids.min() < -1 or ids.max() >= K):
            raise ValueError(f"group id out of range [-1, {K})")
        return ids

    def _markers(self, expr, groups, target, into, group_names, n_groups):
        predicted, names = self._group_names(groups, group_names, n_groups)
        if into is not None:
            into._require_same(names, self.n_genes, self.id2gene)
        rowptr, col, raw, _, _ = csr = self._device_csr(expr)
        B = rowptr.shape[0] - 1
        if not predicted:
            ids = self._group_ids(groups, B, len(names))
        att = self._explain(expr if isinstance(expr, _Aligned) else csr[:3] if csr[4] is None else csr[4], 0, target)
        group = att.label if predicted else ids.astype(np.int64)
        dev_group = torch.from_numpy(group.astype(np.int32)).to(self.device)
        out = None if into is None else (into.score_sum, into.expr_count)
        total, count = _ops.group_gene_reduce(rowptr, col, att.scores, dev_group, len(names), self.n_genes, out=out,
                                              accumulate=into is not None, check=False)
        table = into if into is not None else MarkerTable(
            group_names=names, id2gene=self.id2gene, n_cells=np.zeros(len(names), np.int64), n_skipped=0, score_sum=total,
            expr_count=count, base_sum=np.zeros(len(names)), logit_sum=np.zeros(len(names)))
        table._add_cells(group, att.base, att.logit)
        return table

    def _read_test(self, input_file, normalize=None):
        """A test file as a batch the kernels' routes take, and its cell names.  Without normalisation: ``_read_test_csr``'s
        host CSR, a cell's genes by ascending bundle id.  With it (``normalize``, else the predictor's default) the file
        holds raw counts: its full table and gene names go through ``align``, so the cell totals cover every gene of the
        file, and a cell's genes then come in the FILE's order - the results agree with the ascending-id route in everything
        but the last bits of a row sum (bit for bit when the file lists its bundle genes in the bundle's order)."""
        spec = self._spec(normalize)
        if spec is None and self.aliases is None and self.duplicates == "error":
            return _read_test_csr(input_file, self.file_type, self._gene2id, self.threshold)
        matrix, genes, index = self._read_counts_file(input_file)       # aliases / duplicates are align's: the file goes through it
        with torch.cuda.device(self.device), torch.no_grad():
            return _Aligned(self._align(matrix, genes, None, spec)), index

    def markers_files(self, files, top_k: int = 20, min_fraction: float = 0.0, save_path=None, normalize=None) -> pd.DataFrame:
        """``markers`` over test files streamed into one table (groups = the predicted types), as ``frame(top_k)`` with
        ``cell_type`` (and ``cell_subtype`` with a label map, as ``predict`` names them) in place of ``group``.  Written as
        ``{species}_{tissue}_markers.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``."""
        table = None
        for f in files:
            test, _ = self._read_test(f, normalize)
            table = self.markers(test, into=table)
        if table is None:
            raise ValueError("markers_files: no files")
        out = table.frame(top_k, min_fraction)
        return self._save_frame(self._typed_groups(out), save_path, "markers")

    # ---------------------------------------------------------------------------------------------
    def rank_genes(self, expr, groups="predicted", genes=None, normalize=None, group_names: Optional[Sequence[str]] = None,
                   n_groups: Optional[int] = None, index=None) -> GeneRanks:
        """Which genes are differentially expressed in the cells called type k, against the rest?  A Wilcoxon rank-sum
        (Mann-Whitney) test of every gene of the bundle for every group, on the aligned batch the model sees - what
        ``scanpy.tl.rank_genes_groups(method="wilcoxon")``, Seurat's ``FindAllMarkers`` and presto compute.  ``markers`` is not
        this: it sums the model's attribution scores; ``GeneRanks.compare`` sets the two side by side.  ``expr``, ``genes`` and
        ``normalize`` as for ``markers``.  ``groups="predicted"``: the batch is classified once (``classify``'s call, bit for
        bit, either route) and grouped by label, unsure cells skipped; else one integer id per cell (-1 = skip) with
        ``group_names`` or ``n_groups`` - clusters, true labels, conditions.  ``index``: the cells' names.

        One ``wgnn_rank_genes_groups`` launch counts every gene's tie-averaged ranks across the cells in integers and adds
        them per group, one ``wgnn_group_gene_reduce`` sums the values for the means; the host finishes U, z, p and the AUC
        in fp64 (``include/wgnn.h`` has the definition).  Returns a ``GeneRanks``: ``z`` / ``pvals`` / ``pvals_adj`` / ``auc``
        / ``logfc`` / ``top`` / ``frame`` / ``compare`` / ``summary`` on top.  At most 2^20 cells and 4096 groups.

        There is no ``into=``: ranks are not additive over batches - concatenate the batches first.  A PAIRWISE test needs no
        other call: pass ``groups`` with the cells of every other group at -1.

        What this is not: there are no covariates and no control of pseudoreplication (cells are not samples - with several
        donors feed ``pseudobulk().counts()`` to DESeq2 / edgeR), ``p`` is the normal approximation, and genes outside the
        bundle's vocabulary take no part."""
        _check_index(index, self._n_cells(expr))
        with torch.cuda.device(self.device), torch.no_grad():
            return self._rank_genes(self._over_genes(expr, genes, normalize), groups, group_names, n_groups, index)

    def _rank_genes(self, expr, groups, group_names, n_groups, index):
        predicted, names = self._group_names(groups, group_names, n_groups)
        K, G = len(names), self.n_genes
        device_csr = self._device_csr(expr)
        B = int(device_csr[0].shape[0]) - 1
        if not predicted:                                  # between the upload and the id check, where this refusal has always stood
            ids = self._group_ids(groups, B, K)
        vb = self._values_batch(device_csr, full_call=predicted)
        (rowptr, col, raw), label, max_prob = vb.csr, vb.pred, vb.max_prob
        group = np.asarray(label if predicted else ids, np.int64)
        dev_group = torch.from_numpy(group.astype(np.int32)).to(self.device)
        rank2, count, tie, _ = _ops.rank_genes_groups(rowptr, col, raw, dev_group, K, G, check=False)
        total, _ = _ops.group_gene_reduce(rowptr, col, raw, dev_group, K, G, check=False)
        n_cells = np.bincount(group[group >= 0], minlength=K).astype(np.int64)
        total = total.cpu().numpy()
        whole = np.zeros(G, np.float64)
        for k in range(K):                                 # ascending k: one addition order
            whole += total[k]
        n1 = n_cells[:, None].astype(np.float64)
        n2 = float(n_cells.sum()) - n1
        with np.errstate(invalid="ignore", divide="ignore"):
            mean, mean_rest = total / n1, (whole[None, :] - total) / n2
        return GeneRanks(group_names=names, id2gene=self.id2gene, n_cells=n_cells, n_skipped=int((group < 0).sum()),
                         rank2_sum=rank2.cpu().numpy(), expr_count=count.cpu().numpy(), tie_sum=tie.cpu().numpy(), mean=mean,
                         mean_rest=mean_rest, label=label, max_prob=max_prob, index=pd.RangeIndex(B) if index is None else index)

    def rank_genes_file(self, data, normalize=None, top_k: int = 20, save_path=None) -> pd.DataFrame:
        """``rank_genes`` on a test file - its full table, its gene names as ``genes=`` and its cell names - with the predicted
        types as groups: ``GeneRanks.frame(top_k)`` with ``cell_type`` (and ``cell_subtype`` with a label map, as ``predict``
        names them) in place of ``group``, written as ``{species}_{tissue}_rank_genes.csv`` under ``save_path`` when given.
        ``normalize``: as for ``predict``."""
        matrix, genes, index = self._read_counts_file(data)
        out = self.rank_genes(matrix, genes=genes, normalize=normalize, index=index).frame(top_k)
        return self._save_frame(self._typed_groups(out), save_path, "rank_genes")

    def predict(self, input_file, save_path=None, normalize=None) -> pd.DataFrame:
        """``DeepSortPredictor.predict`` on the resident bundle: same columns, label-map handling and output file name.
        ``normalize`` (``None`` = the predictor's default | ``"lognorm"`` | ``LogNormalize``): the file holds raw counts, which
        are log-normalised on the device over ALL of the file's genes (``align``); a cell's genes then come in the file's order,
        and the results agree with the ascending-id route in everything but the last bits of a row sum."""
        test, index = self._read_test(input_file, normalize)
        pred, _, _ = self.classify(test)
        return _prediction_frame(self.species, self.tissue, input_file, index, pred, self.id2label, self.bundle, save_path)

    def explain_file(self, input_file, top_k: int = 10, save_path=None, normalize=None) -> pd.DataFrame:
        """``explain`` on a test file, in long form: one row per (cell, rank) with the columns ``index``, ``cell_type`` (and
        ``cell_subtype`` with a label map, as ``predict`` names them), ``rank`` (1 = highest score), ``gene``, ``score``.
        Written as ``{species}_{tissue}_{stem}_genes.csv`` under ``save_path`` when given.  ``normalize``: as for ``predict``."""
        test, index = self._read_test(input_file, normalize)
        att = self.explain(test, top_k=top_k)
        cells = _prediction_frame(self.species, self.tissue, input_file, index, att.label, self.id2label, self.bundle, None)
        r, k = np.nonzero(att.top_genes >= 0)
        out = cells.iloc[r].reset_index(drop=True)
        out["rank"] = k + 1
        out["gene"] = [self.id2gene[g] for g in att.top_genes[r, k]]
        out["score"] = att.top_scores[r, k]
        return self._save_frame(out, save_path, f"{Path(input_file).stem}_genes")

    def predict_many(self, files, save_path=None, normalize=None) -> List[pd.DataFrame]:
        """One table per test file (``predict.py --test_dataset 1 2 3``), the bundle loaded once.  ``normalize``: as for
        ``predict``."""
        return [self.predict(f, save_path, normalize=normalize) for f in files]

    def default_map_file(self) -> Optional[Path]:
        root = self.bundle.root
        return next((f for f in (root / "map.xlsx", root.parent / "map" / self.species / "map.xlsx") if f.exists()), None)

    def evaluate(self, data_file, celltype_file, map_file=None, dataset_num=None, normalize=None):
        """The reference's evaluate mode (predict.py:90-121, its default): predictions scored against the true labels of
        ``celltype_file`` through ``map.xlsx`` (``get_map_dict``, preprocess.py:14-29).  Returns (correct, total, unsure,
        acc, DataFrame with an 'original label' column, predict.py:138-143).  ``normalize``: as for ``predict``."""
        map_file = Path(map_file) if map_file is not None else self.default_map_file()
        if map_file is None:
            raise FileNotFoundError(f"no map.xlsx next to the bundle under {self.bundle.root} (pass map_file)")
        num = int(dataset_num) if dataset_num is not None else dataset_number(data_file, self.tissue)
        map_dict = load_map_dict(map_file, self.tissue)
        if num not in map_dict:
            raise ValueError(f"dataset {num} of tissue {self.tissue!r} is not in {map_file}")
        ct = pd.read_csv(celltype_file, index_col=0)
        ct.columns = ['cell', 'type']                                       # preprocess.py:147-150
        truth = ct['type'].map(str.strip).tolist()
        test, index = self._read_test(data_file, normalize)
        if len(truth) != len(index):
            raise ValueError(f"{celltype_file} lists {len(truth)} cells, {data_file} holds {len(index)}")
        pred, _, _ = self.classify(test)
        correct, total, unsure, acc, _ = evaluate_predictions(pred, truth, self.id2label, map_dict[num])
        out = _prediction_frame(self.species, self.tissue, data_file, index, pred, self.id2label, self.bundle, None,
                                original=truth)
        return correct, total, unsure, acc, out
