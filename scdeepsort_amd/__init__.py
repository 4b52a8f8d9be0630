"""scdeepsort_amd - MI355X-native hot path of scDeepSort (weighted GraphSAGE aggregation).

Public surface mirrors the reference: ``GNN`` (models/gnn.py:28), ``DeepSortPredictor`` /
``DeepSortClassifier`` (docs/api.rst:6-130).  The arithmetic runs in ``libwgnn_hip.so``
(C ABI in ``include/wgnn.h``); importing this package does not load it, using any
operator does, and fails loudly when it is missing.
"""
from ._lib import WgnnError, DST_IS_GENE, NO_ALPHA, SRC_IS_GENE
from .graph import AggCsr, CellGeneGraph, Plan, build_plan
from .gnn import GNN, NodeUpdate
from .api import Abstraction, Ambient, Attribution, BatchGraph, ClusterCalls, Communities, Coverage, DeepSortClassifier, DeepSortPredictor, DiffusionMap, DiffusionPseudotime, Doublets, GeneMap, GeneRanks, Harmonized, KMeans, Layout, LogNormalize, MarkerTable, NeighborGraph, PanelCalls, Pseudobulk, Pseudotime, ResidentPredictor, SignatureScores, Silhouette, Smoothed, Stability, read_gmt
from .graphed import GraphedForward, GraphedShardedForward, GraphedTrainStep
from .ops import agg_bwd_alpha, agg_bwd_src, agg_fwd, cross_entropy_sum, linear_fwd, predict_rows, weighted_mean_aggregate
from .ops import align_rows, attrib_rows, basis_combine, coverage_rows, diffusion_distance, diffusion_operator, distance_graph, graph_components, lanczos_graph, lanczos_ritz, fuzzy_graph, geodesic_rows, group_class_reduce, group_edges, group_gene_reduce, hood_rows, kmeans_rows, kmeans_seed, group_rows_reduce, knn_rows, knn_segments, layout_curve, layout_graph, leiden_graph, louvain_graph, pair_rows, pool_rows, predict_rows_dropout, predict_rows_panels, predict_rows_thin, rank_genes_groups, rank_sets_rows, rows_topk, silhouette_rows, snn_graph, soup_rows
from .ops import harmony_apply, harmony_assign_block, harmony_fold, harmony_objective, harmony_ridge, harmony_rows, harmony_scores, weighted_group_reduce
from .sampler import DeviceSampler

__all__ = ["GNN", "NodeUpdate", "DeepSortClassifier", "DeepSortPredictor", "ResidentPredictor", "CellGeneGraph", "AggCsr", "Plan", "build_plan", "agg_fwd", "agg_bwd_src",
           "agg_bwd_alpha", "weighted_mean_aggregate", "linear_fwd", "predict_rows", "predict_rows_dropout", "predict_rows_thin", "predict_rows_panels", "rank_sets_rows", "rank_genes_groups", "pair_rows", "pool_rows", "soup_rows", "hood_rows", "knn_rows", "knn_segments", "kmeans_rows", "kmeans_seed", "group_rows_reduce", "silhouette_rows", "snn_graph", "louvain_graph", "leiden_graph", "fuzzy_graph", "layout_graph", "layout_curve", "distance_graph", "geodesic_rows", "group_edges", "graph_components", "diffusion_operator", "lanczos_graph", "lanczos_ritz", "basis_combine", "diffusion_distance", "harmony_rows", "harmony_scores", "harmony_assign_block", "harmony_fold", "weighted_group_reduce", "harmony_objective", "harmony_apply", "harmony_ridge", "attrib_rows", "rows_topk", "group_gene_reduce", "group_class_reduce", "align_rows", "coverage_rows", "Coverage", "Attribution", "MarkerTable", "ClusterCalls", "Stability", "Doublets", "Pseudobulk", "PanelCalls", "Ambient", "Smoothed", "SignatureScores", "GeneRanks", "NeighborGraph", "BatchGraph", "Harmonized", "KMeans", "Silhouette", "Communities", "Layout", "Pseudotime", "Abstraction", "DiffusionMap", "DiffusionPseudotime", "read_gmt", "LogNormalize", "GeneMap", "DeviceSampler", "GraphedForward", "GraphedShardedForward", "GraphedTrainStep", "cross_entropy_sum",
           "WgnnError", "SRC_IS_GENE", "DST_IS_GENE", "NO_ALPHA"]
__version__ = "0.4.0"
