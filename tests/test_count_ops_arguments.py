"""The six ``ResidentPredictor`` entry points that take raw counts refuse the same arguments, each in its own words, before the
device is touched (``_count_spec`` / ``_check_index``)."""
import numpy as np
import pytest
import torch

from scdeepsort_amd import api

BATCH, GENES = np.zeros((5, 7), np.float32), [f"g{i}" for i in range(7)]

# entry point -> (the call, the clause of its own that both count refusals carry)
CALLS = {
    "stability": (lambda rp, genes, **kw: rp.stability(BATCH, genes=genes, thin="reads", **kw), "thin=\"reads\""),
    "panels": (lambda rp, genes, **kw: rp.panels(BATCH, panels={"a": ["g1"]}, genes=genes, renormalize=True, **kw), "renormalize=True"),
    "doublets": (lambda rp, genes, **kw: rp.doublets(BATCH, genes, **kw), "doublets"),
    "ambient": (lambda rp, genes, **kw: rp.ambient(BATCH, genes, **kw), "ambient"),
    "smooth": (lambda rp, genes, **kw: rp.smooth(BATCH, genes, np.full((5, 1), -1), **kw), "smooth"),
    "pseudobulk": (lambda rp, genes, **kw: rp.pseudobulk(BATCH, genes, ["a", "b", "a", "b", "a"], **kw), "pseudobulk"),
}


class Fake(api.ResidentPredictor):                                  # no bundle and no device: a launch would be an AttributeError
    def __init__(self):
        self.hidden_padded, self.n_classes, self.id2label = 12, 3, ["T0", "T1", "T2"]
        self.normalize, self.duplicates, self.aliases = None, "error", None


@pytest.mark.parametrize("op", list(CALLS))
def test_count_taking_calls_refuse_alike(op):
    call, clause = CALLS[op]
    rp = Fake()
    ids = torch.zeros(7, dtype=torch.int32)
    merged = api.GeneMap(ids=ids, col_group=ids, group_ptr=torch.tensor([0, 2], dtype=torch.int32),
                         group_cols=torch.tensor([0, 1], dtype=torch.int32), n_groups=1, n_merged_columns=2)
    with pytest.raises(ValueError, match="genes=") as e:
        call(rp, None, normalize="lognorm")
    assert clause in str(e.value)
    with pytest.raises(ValueError, match="normalize") as e:
        call(rp, GENES)
    assert clause in str(e.value)
    with pytest.raises(ValueError, match="merged") as e:
        call(rp, merged, normalize="lognorm")
    assert clause in str(e.value)
    rp.duplicates = "sum"
    with pytest.raises(ValueError, match="merged") as e:
        call(rp, GENES, normalize="lognorm")
    assert clause in str(e.value)
    rp.duplicates = "error"
    if op != "pseudobulk":                                          # pseudobulk returns clusters: it takes no index
        with pytest.raises(ValueError, match="index names 1 cells, the batch holds 5"):
            call(rp, GENES, normalize="lognorm", index=["a"])
