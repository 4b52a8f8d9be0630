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


@pytest.fixture(scope="module")
def generic():
    """The generic text of each code: what wgnn_last_error_string says when no call has failed with it."""
    lib = _lib.lib()
    texts = {}
    for code in (-1, -2, -3):
        for _ in range(8):                                                # drop the details earlier tests left unasked
            texts[code] = lib.wgnn_last_error_string(code)
        assert b" - wgnn_" not in texts[code]
    return texts


# ------------------------------------------------------------------------------------------------
# the refusals of wgnn_predict_rows_dropout / wgnn_predict_rows_thin / wgnn_attrib_rows: the code and the check that
# wgnn_last_error_string names, one perturbed argument per row (the cases test_{stability,thin,attrib}_reference.py assert
# already are not repeated).  Fake pointers: 16 is aligned; 24 is 8- but not 16-byte aligned, 20 is 4- but not 8-byte
# aligned, 18 is not 4-byte aligned.  None of them is dereferenced: validation returns first.
# ------------------------------------------------------------------------------------------------
_ROW = ("rowptr", "col", "raw", "n_rows", "table", "ld_table", "n_genes", "H", "alpha", "bias", "self_rows", "ld_self")
_DRAW = ("n_draws", "row0", "draw0", "seed", "keep", "out", "ld_out", "w_head", "b_head", "n_classes", "unsure_threshold",
         "votes", "ld_votes", "unsure", "empty", "conf_sum", "draw_label", "draw_prob")
_ORDER = {      # the arguments in the order include/wgnn.h declares them
    "wgnn_predict_rows_dropout": _ROW + _DRAW + ("flags", "stream"),
    "wgnn_predict_rows_thin": _ROW + ("rest", "scale", "threshold") + _DRAW + ("draw_reads", "draw_entries", "flags", "stream"),
    "wgnn_attrib_rows": _ROW + ("w_head", "b_head", "n_classes", "target", "unsure_threshold", "label_out", "direction", "ld_dir",
                                "score", "target_out", "logit_out", "base_out", "dir_out", "ld_dir_out", "flags", "stream"),
}
_P = 16
_ROW_OK = dict(rowptr=_P, col=_P, raw=_P, n_rows=4, table=_P, ld_table=8, n_genes=10, H=8, alpha=_P, bias=_P, self_rows=None,
               ld_self=0, flags=0, stream=None)
_DRAW_OK = dict(_ROW_OK, n_draws=2, row0=0, draw0=0, seed=7, keep=0.5, out=_P, ld_out=8, w_head=None, b_head=None, n_classes=0,
                unsure_threshold=0.5, votes=None, ld_votes=0, unsure=None, empty=None, conf_sum=None, draw_label=None,
                draw_prob=None)
_DRAW_HEAD = dict(out=None, ld_out=0, w_head=_P, b_head=_P, n_classes=3, votes=_P, ld_votes=3, unsure=_P, empty=_P, conf_sum=_P)
_BASE = {       # a call every check lets through: (without a head | in direction mode, the changes that give it a head)
    "wgnn_predict_rows_dropout": (_DRAW_OK, _DRAW_HEAD),
    "wgnn_predict_rows_thin": (dict(_DRAW_OK, rest=_P, scale=1e4, threshold=0.0, draw_reads=None, draw_entries=None), _DRAW_HEAD),
    "wgnn_attrib_rows": (dict(_ROW_OK, bias=None, w_head=None, b_head=None, n_classes=0, target=None, unsure_threshold=0.5,
                              label_out=None, direction=_P, ld_dir=8, score=_P, target_out=None, logit_out=None, base_out=None,
                              dir_out=None, ld_dir_out=0),
                         dict(bias=_P, w_head=_P, b_head=_P, n_classes=3, direction=None, ld_dir=0, target_out=_P, logit_out=_P,
                              base_out=_P)),
}
_DROPOUT, _THIN, _ATTRIB = _ORDER
_DRAWS = (_DROPOUT, _THIN)
_ALL = (_DROPOUT, _THIN, _ATTRIB)
_ACC = 256          # WGNN_STABILITY_ACCUMULATE == WGNN_THIN_ACCUMULATE == WGNN_ATTRIB_ACCUMULATE


def _refusals():
    """(entry, head, perturbed arguments, return code, fragment of the detail)"""
    rows = []

    def add(entries, head, change, code, word):
        rows.extend((e, head, change, code, word) for e in entries)

    for head in (False, True):
        for p in ("rowptr", "col", "raw", "table", "alpha"):
            add(_ALL, head, {p: None}, -1, b"are required")
        add(_ALL, head, dict(n_rows=-1), -1, b"n_rows must be in [0, 2^31)")
        add(_ALL, head, dict(n_genes=0), -1, b"n_genes must be positive")
        add(_ALL, head, dict(H=0), -1, b"H must be positive")
        add(_ALL, head, dict(ld_table=4), -2, b"ld_table must be >= H and a multiple of 4")
        add(_ALL, head, dict(ld_table=10), -2, b"ld_table must be >= H and a multiple of 4")
        add(_DRAWS, head, dict(table=24), -2, b"table and bias must be 16-byte aligned")
        add(_DRAWS, head, dict(bias=24), -2, b"table and bias must be 16-byte aligned")
        add(_DRAWS, head, dict(bias=None), -1, b"are required")
        add(_DRAWS, head, dict(self_rows=_P, ld_self=4), -2, b"self_rows: ld_self >= H")
        add(_DRAWS, head, dict(self_rows=_P, ld_self=10), -2, b"self_rows: ld_self >= H")
        add(_DRAWS, head, dict(self_rows=24, ld_self=8), -2, b"self_rows: ld_self >= H")
        add(_DRAWS, head, dict(n_rows=2 ** 31 - 1, n_draws=2), -1, b"n_rows * n_draws must be < 2^31")
        add((_THIN,), head, dict(n_draws=-3), -1, b"n_draws must be >= 1")
        add((_THIN,), head, dict(draw_reads=20, draw_entries=18), -2, b"draw_reads and draw_entries must be 4-byte aligned")
        add((_THIN,), head, dict(rest=24), 0, None)                       # 8-byte alignment is all `rest` needs
    # without a head
    add(_DRAWS, False, dict(ld_out=4), -2, b"out: ld_out >= H")
    add(_DRAWS, False, dict(ld_out=10), -2, b"out: ld_out >= H")
    add(_DRAWS, False, dict(out=24), -2, b"out: ld_out >= H")
    add(_DRAWS, False, dict(H=256, ld_table=256, ld_out=256, n_classes=65), 0, None)     # n_classes is not read
    # with a head
    add(_DRAWS, True, dict(b_head=None), -1, b"a head needs b_head, votes, unsure, empty and conf_sum")
    add((_THIN,), True, dict(unsure=None), -1, b"a head needs b_head, votes, unsure, empty and conf_sum")
    add((_THIN,), True, dict(empty=None), -1, b"a head needs b_head, votes, unsure, empty and conf_sum")
    add(_ALL, True, dict(n_classes=0), -1, b"n_classes must be positive")
    add(_DRAWS, True, dict(H=256, ld_table=256, n_classes=65, ld_votes=65), -3, b"the head needs C*H*4 <= 64 KiB")
    add(_DRAWS, True, dict(H=256, ld_table=256, n_classes=64, ld_votes=64), 0, None)
    add((_ATTRIB,), True, dict(H=256, ld_table=256, n_classes=64), 0, None)
    add(_ALL, True, dict(w_head=24), -2, b"w_head must be 16-byte aligned")
    add(_DRAWS, True, dict(conf_sum=24), 0, None)
    add(_DRAWS, True, dict(conf_sum=20), -2, b"conf_sum must be 8-byte aligned")
    for p in ("votes", "unsure", "empty", "draw_label", "draw_prob"):
        add(_DRAWS, True, {p: 18}, -2, b"votes, unsure, empty, draw_label and draw_prob must be 4-byte aligned")
        add(_DRAWS, True, {p: 20}, 0, None)
    add(_DRAWS, True, dict(ld_votes=2), -1, b"ld_votes must be >= n_classes")
    add(_DRAWS, True, dict(flags=_ACC), 0, None)
    add(_DRAWS, True, dict(flags=_ACC | _lib.FLAG_ROWPTR_I64), 0, None)
    add((_THIN,), True, dict(flags=512), -1, b"only WGNN_FLAG_ROWPTR_I64 and WGNN_THIN_ACCUMULATE are valid flags")
    # wgnn_attrib_rows' own rules
    add((_ATTRIB,), False, dict(score=None), -1, b"rowptr, col, raw, table, alpha and score are required")
    add((_ATTRIB,), True, dict(score=None), -1, b"rowptr, col, raw, table, alpha and score are required")
    add((_ATTRIB,), False, dict(flags=_lib.FLAG_RELU), -1, b"valid flags: WGNN_FLAG_ROWPTR_I64, WGNN_ATTRIB_ACCUMULATE")
    add((_ATTRIB,), False, dict(H=6), -2, b"H must be a multiple of 4 (zero-pad the table, bias, head and direction)")
    add((_ATTRIB,), False, dict(H=260, ld_table=260, ld_dir=260), -3, b"H > 256 is not built")
    add((_ATTRIB,), False, dict(table=24), -2, b"table must be 16-byte aligned")
    add((_ATTRIB,), True, dict(table=24), -2, b"table must be 16-byte aligned")
    add((_ATTRIB,), False, dict(direction=None), -1, b"give either a head (w_head) or a direction")
    add((_ATTRIB,), True, dict(direction=_P, ld_dir=8), -1, b"give either a head (w_head) or a direction")
    for p in ("bias", "b_head", "target_out", "logit_out", "base_out"):
        add((_ATTRIB,), True, {p: None}, -1, b"a head needs bias, b_head, target_out, logit_out and base_out")
    for f in (_lib.ATTRIB_ACCUMULATE, _lib.ATTRIB_EXPLICIT_SELF):
        add((_ATTRIB,), True, dict(flags=f), -1, b"head mode overwrites score and takes its self rule from self_rows")
        add((_ATTRIB,), False, dict(flags=f), 0, None)
    add((_ATTRIB,), True, dict(bias=24), -2, b"bias must be 16-byte aligned")
    add((_ATTRIB,), False, dict(bias=24), 0, None)                        # direction mode does not read the bias
    add((_ATTRIB,), True, dict(self_rows=_P, ld_self=4), -2, b"self_rows: ld_self >= H")
    add((_ATTRIB,), True, dict(self_rows=_P, ld_self=10), -2, b"self_rows: ld_self >= H")
    add((_ATTRIB,), True, dict(self_rows=24, ld_self=8), -2, b"self_rows: ld_self >= H")
    add((_ATTRIB,), False, dict(self_rows=24, ld_self=4), 0, None)        # nor the self rows
    add((_ATTRIB,), True, dict(H=256, ld_table=256, n_classes=65), -3, b"the head needs C*H*4 <= 64 KiB")
    add((_ATTRIB,), True, dict(dir_out=_P, ld_dir_out=4), -2, b"dir_out: ld_dir_out >= H")
    add((_ATTRIB,), True, dict(dir_out=_P, ld_dir_out=10), -2, b"dir_out: ld_dir_out >= H")
    add((_ATTRIB,), True, dict(dir_out=24, ld_dir_out=8), -2, b"dir_out: ld_dir_out >= H")
    add((_ATTRIB,), False, dict(ld_dir=4), -2, b"direction: ld_dir >= H")
    add((_ATTRIB,), False, dict(ld_dir=10), -2, b"direction: ld_dir >= H")
    add((_ATTRIB,), False, dict(direction=24), -2, b"direction: ld_dir >= H")
    return rows


def _refusal_id(row):
    entry, head, change, code, _ = row
    return f"{entry[5:]}-{'head' if head else 'nohead'}-{','.join(f'{k}={v}' for k, v in change.items())}->{code}"


@pytest.mark.parametrize("row", _refusals(), ids=_refusal_id)
def test_resident_row_entries_refuse_with_code_and_detail_without_gpu(row, generic):
    entry, head, change, code, word = row
    lib = _lib.lib()
    base, with_head = _BASE[entry]
    kw = {**base, **(with_head if head else {}), **change}
    # an accepted call must not reach a launch: it runs on an empty batch (n_rows == 0 returns after every check)
    if code == 0:
        kw["n_rows"] = 0
    assert set(kw) == set(_ORDER[entry])
    assert getattr(lib, entry)(*(kw[k] for k in _ORDER[entry])) == code
    if code:
        msg = lib.wgnn_last_error_string(code)
        assert entry.encode() + b": " in msg and word in msg, msg
        assert lib.wgnn_last_error_string(code) == generic[code]         # handed out once


@pytest.mark.parametrize("entry", _ALL)
@pytest.mark.parametrize("head", (False, True))
def test_resident_row_entries_accept_an_empty_batch_without_gpu(entry, head):
    base, with_head = _BASE[entry]
    kw = {**base, **(with_head if head else {}), "n_rows": 0}
    assert getattr(_lib.lib(), entry)(*(kw[k] for k in _ORDER[entry])) == 0


def test_last_error_detail_is_that_of_the_last_failing_call_whatever_the_entry(generic):
    """``wgnn_predict_rows`` refused with -3 and nobody asks; then ``wgnn_attrib_rows`` refused with -3: the string is the second
    call's, once, then the generic text.  A call that passes forgets an unasked detail too."""
    lib = _lib.lib()
    p = C.c_void_p(_P)
    predict = lambda H: lib.wgnn_predict_rows(p, p, p, 4, p, H, 10, H, p, p, None, 0, p, H, None, None, 0, 0.5, None, 0, None, None, 0, None)
    base, with_head = _BASE[_ATTRIB]
    attrib = lambda **kw: lib.wgnn_attrib_rows(*({**base, **with_head, **kw}[k] for k in _ORDER[_ATTRIB]))
    assert predict(260) == -3
    assert attrib(H=260, ld_table=260) == -3
    msg = lib.wgnn_last_error_string(-3)
    assert b" - wgnn_attrib_rows: H > 256 is not built" in msg and b"wgnn_predict_rows" not in msg
    assert lib.wgnn_last_error_string(-3) == generic[-3]
    assert predict(260) == -3
    assert attrib(n_rows=0) == 0
    assert lib.wgnn_last_error_string(-3) == generic[-3]


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
