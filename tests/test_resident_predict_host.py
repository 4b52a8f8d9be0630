"""CPU checks of the resident predictor: argument validation of ``wgnn_predict_rows`` (no launch), the loud failure without
a GPU, the evaluate mode's map reader and counting (reference predict.py:90-121, preprocess.py:14-29)."""
import ctypes as C
import zipfile

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import _lib, api


def test_predict_rows_validation_returns_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)      # fake, aligned, never dereferenced: validation happens first

    def call(rowptr=one, col=one, raw=one, B=4, table=one, ld=8, G=10, H=8, alpha=one, bias=one, self_rows=None, ld_self=0,
             out=one, ld_out=8, w_head=None, b_head=one, C_=3, logits=None, ld_logits=0, label=one, max_prob=one, flags=0):
        return lib.wgnn_predict_rows(rowptr, col, raw, B, table, ld, G, H, alpha, bias, self_rows, ld_self, out, ld_out,
                                     w_head, b_head, C_, 0.5, logits, ld_logits, label, max_prob, flags, None)

    assert call(B=0) == 0                                   # empty batch: a no-op
    for k in ("rowptr", "col", "raw", "table", "alpha", "bias"):
        assert call(**{k: None}) == -1, k
    assert call(out=None) == -1                             # no head and no output
    assert call(B=-1) == -1 and call(B=2 ** 31) == -1
    assert call(G=0) == -1 and call(H=0) == -1
    assert call(flags=_lib.FLAG_RELU) == -1                 # only WGNN_FLAG_ROWPTR_I64
    assert call(flags=_lib.FLAG_ROWPTR_I64, B=0) == 0
    assert call(H=6, ld=8) == -2                            # H % 4
    assert b"multiple of 4" in lib.wgnn_last_error_string(-2)
    assert call(H=260, ld=260, ld_out=260) == -3            # H > 256
    assert b"H > 256" in lib.wgnn_last_error_string(-3)
    assert call(ld=4) == -2 and call(ld_out=6) == -2
    assert call(self_rows=one, ld_self=4) == -2
    assert call(table=C.c_void_p(20)) == -2                 # not 16-byte aligned
    # a fused head: C * H * 4 <= 64 KiB, and it needs its bias, label and max_prob
    assert call(w_head=one, out=None, B=0) == 0
    assert call(w_head=one, out=None, H=256, ld=256, C_=64, B=0) == 0
    assert call(w_head=one, out=None, H=256, ld=256, C_=65) == -3
    assert b"64 KiB" in lib.wgnn_last_error_string(-3)
    assert call(w_head=one, b_head=None) == -1 and call(w_head=one, label=None) == -1 and call(w_head=one, max_prob=None) == -1
    assert call(w_head=one, C_=0) == -1
    assert call(w_head=one, logits=one, ld_logits=2) == -1  # ld_logits < C
    # the detail is handed out once; the generic text (other entry points' callers rely on it) stays in front of it
    assert call(H=260, ld=260, ld_out=260) == -3
    first = lib.wgnn_last_error_string(-3)
    assert b"2^31" in first and b"H > 256" in first
    assert lib.wgnn_last_error_string(-3) == b"unsupported dtype, feature width (D <= 1024 required) or nnz >= 2^31 (shard the cell axis)"


def test_ops_predict_rows_refuses_cpu_tensors():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(sda.WgnnError):
        sda.predict_rows(rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), torch.zeros(3, 8), torch.ones(5), torch.zeros(8))


def test_resident_predictor_fails_loudly_without_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(sda.WgnnError):
        sda.ResidentPredictor("mouse", "Testis", model_path=tmp_path)


def _write_xlsx(path, rows, sheet="Sheet1"):
    """One-sheet .xlsx written with zipfile: strings as inline strings, ints as number cells (as Excel stores `num`)."""
    from xml.sax.saxutils import escape
    body = []
    for r, row in enumerate(rows, 1):
        cells = []
        for c, v in enumerate(row):
            ref = f"{chr(65 + c)}{r}"
            if v is None:
                continue
            if isinstance(v, int):
                cells.append(f'<c r="{ref}"><v>{v}</v></c>')
            else:
                cells.append(f'<c r="{ref}" t="inlineStr"><is><t>{escape(v)}</t></is></c>')
        body.append(f'<row r="{r}">{"".join(cells)}</row>')
    ns = 'xmlns="http://schemas.openxmlformats.org/spreadsheetml/2006/main"'
    rns = 'xmlns:r="http://schemas.openxmlformats.org/officeDocument/2006/relationships"'
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("xl/workbook.xml", f'<?xml version="1.0"?><workbook {ns} {rns}><sheets><sheet name="{sheet}" sheetId="1" '
                                      f'r:id="rId1"/></sheets></workbook>')
        z.writestr("xl/_rels/workbook.xml.rels", '<?xml version="1.0"?><Relationships xmlns="http://schemas.openxmlformats.org/'
                   'package/2006/relationships"><Relationship Id="rId1" Type="http://schemas.openxmlformats.org/officeDocument/'
                   '2006/relationships/worksheet" Target="worksheets/sheet1.xml"/></Relationships>')
        z.writestr("xl/worksheets/sheet1.xml", f'<?xml version="1.0"?><worksheet {ns}><sheetData>{"".join(body)}</sheetData></worksheet>')


MAP_ROWS = [["Tissue", "num", "Test Datasets", "Celltype", "Training dataset cell type"],
            ["Testis", 199, "mouse_Testis199_data.csv", "Sertoli cell", "Sertoli cell"],
            ["Testis", 199, "mouse_Testis199_data.csv", "Spermatogonia", "Spermatogonia"],
            ["Testis", 199, "mouse_Testis199_data.csv", "Spermatogonia", "Preleptotene spermatogonia"],
            ["Blood", 768, "mouse_Blood768_data.csv", "Basophil", "Basophil"],
            ["Testis", 2584, "mouse_Testis2584_data.csv", "Leydig cell", "Leydig cell"]]


def test_map_xlsx_reader_matches_handwritten_dict(tmp_path):
    _write_xlsx(tmp_path / "map.xlsx", MAP_ROWS)
    got = api.load_map_dict(tmp_path / "map.xlsx", "Testis")
    assert got == {199: {"Sertoli cell": {"Sertoli cell"}, "Spermatogonia": {"Spermatogonia", "Preleptotene spermatogonia"}},
                   2584: {"Leydig cell": {"Leydig cell"}}}
    assert api.load_map_dict(tmp_path / "map.xlsx", "Blood") == {768: {"Basophil": {"Basophil"}}}
    assert api.load_map_dict(tmp_path / "map.xlsx", "Lung") == {}


def _reference_counting(prob, truth, id2label, unsure_rate, map_for_num):
    """predict.py:104-118, restated literally over softmax rows."""
    total = prob.shape[0]
    unsure_num, correct = 0, 0
    predict_label = []
    for pred, t_label in zip(prob, truth):
        pred_label = id2label[pred.argmax().item()]
        if pred.max().item() < unsure_rate / len(id2label):
            unsure_num += 1
            predict_label.append('unsure')
        else:
            if pred_label in map_for_num[t_label]:
                correct += 1
            predict_label.append(pred_label)
    return correct, total, unsure_num, correct / total, predict_label


def test_evaluate_counting_matches_reference_restatement():
    rng = np.random.default_rng(3)
    id2label = ["Sertoli cell", "Spermatogonia", "Preleptotene spermatogonia", "Leydig cell"]
    mapping = {"Sertoli cell": {"Sertoli cell"}, "Spermatogonia": {"Spermatogonia", "Preleptotene spermatogonia"},
               "Leydig cell": {"Leydig cell"}}
    logits = torch.from_numpy(rng.normal(0, 1.5, (200, 4)).astype(np.float32))
    truth = [list(mapping)[i] for i in rng.integers(0, 3, 200)]
    pred, prob = api._classify(logits, 2.0)
    want = _reference_counting(prob, truth, id2label, 2.0, mapping)
    got = api.evaluate_predictions(pred, truth, id2label, mapping)
    assert got == want
    assert 0 < want[2] < 200 and 0 < want[0]                  # both unsure and correct cells occur
    with pytest.raises(ValueError, match="Macrophage"):
        api.evaluate_predictions([0], ["Macrophage"], id2label, mapping)


def test_dataset_number_parsing():
    assert api.dataset_number("test/mouse/mouse_Testis199_data.csv", "Testis") == 199
    assert api.dataset_number("mouse_Bone_marrow47_data.csv.gz", "Bone_marrow") == 47
    assert api.dataset_number("/x/human_Lung6022_data.gz", "Lung") == 6022
    with pytest.raises(ValueError):
        api.dataset_number("mouse_Testis_data.csv", "Testis")
