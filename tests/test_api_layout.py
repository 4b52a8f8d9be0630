"""Where the host code of the package lives: the result tables in ``tables.py``, the predictor and its constants in ``api.py``,
every moved name still reachable through ``api``, and no import from ``tables`` back into ``api`` or ``ops``."""
import ast
import inspect

import scdeepsort_amd as sda
from scdeepsort_amd import api, tables

TABLES = ("Attribution", "MarkerTable", "ClusterCalls", "Coverage", "Stability", "Doublets", "Ambient", "Smoothed", "Pseudobulk",
          "PanelCalls", "SignatureScores", "GeneRanks")
SUMMARIES = ("CoverageSummary", "StabilitySummary", "DoubletsSummary", "AmbientSummary", "SmoothedSummary", "PseudobulkSummary",
             "PanelSummary", "SignatureSummary", "GeneRanksSummary")
HELPERS = ("_call_names", "_NamesCalls", "_check_index", "_cluster_ids", "_keep_levels", "_rho_levels", "_neighbor_lists",
           "SMOOTH_MAX_NEIGHBORS", "_signature_scores", "_rank_genes_stats", "_benjamini_hochberg")
STAY = ("ResidentPredictor", "_Aligned", "_CountBatch", "_COUNT_OPS", "LogNormalize", "GeneMap", "_resolve_genes", "_gene_map_ids",
        "_resolve_panels", "_member_words", "read_gmt", "_i64", "_lsr", "_mix64", "_draw_partners", "_byte_chunks",
        "RESIDENT_FUSED_MAX_WORK", "STABILITY_CHUNK_BYTES", "DOUBLETS_CHUNK_BYTES", "AMBIENT_CHUNK_BYTES", "SMOOTH_CHUNK_BYTES",
        "_predict_logits", "_classify", "_gene_features")


def test_every_exported_name_resolves():
    assert sda.__all__
    for name in sda.__all__:
        assert getattr(sda, name) is not None, name


def test_moved_names_are_the_same_objects_through_api():
    for name in TABLES + SUMMARIES + HELPERS:
        assert getattr(api, name) is getattr(tables, name), name
    for name in TABLES + SUMMARIES:
        assert getattr(tables, name).__module__ == "scdeepsort_amd.tables", name
    for name in TABLES:
        assert getattr(sda, name) is getattr(tables, name), name


def test_tables_imports_neither_api_nor_ops():
    tree = ast.parse(inspect.getsource(tables))
    for node in ast.walk(tree):                                   # imports inside functions included
        if isinstance(node, ast.Import):
            assert not any(a.name.split(".")[-1] in ("api", "ops") for a in node.names), ast.dump(node)
        elif isinstance(node, ast.ImportFrom):
            assert (node.module or "").split(".")[-1] not in ("api", "ops"), ast.dump(node)
            assert node.module or not any(a.name in ("api", "ops") for a in node.names), ast.dump(node)      # from . import api


def test_the_predictor_and_what_tests_patch_stay_in_api():
    assert api.ResidentPredictor.__module__ == "scdeepsort_amd.api"
    assert api.ResidentPredictor._cells_per_launch.__globals__ is vars(api)       # monkeypatch.setattr(api, "..._CHUNK_BYTES") reaches it
    for name in STAY:
        assert hasattr(api, name) and not hasattr(tables, name), name
