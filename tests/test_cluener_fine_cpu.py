"""cluener_fine: CLUENER with its ten native entity types (24 BIO labels),
from the spec through the loaders to a CPU forward/backward."""
import json

import torch

from chinesener_amd.data.datasets import (CLS_TAG, PAD_TAG, SEP_TAG, get_spec,
                                          load_data)

from conftest import make_tiny_batch, make_tiny_params

TYPES = ["address", "book", "company", "game", "government", "movie",
         "name", "organization", "position", "scene"]


def test_spec_has_24_labels_in_native_order():
    spec = get_spec("cluener_fine")
    assert spec.label_size == 24
    assert spec.entity_types == TYPES
    expect = [PAD_TAG, "O"]
    for t in TYPES:
        expect += [f"B-{t}", f"I-{t}"]
    expect += [CLS_TAG, SEP_TAG]
    assert [spec.idx2tag[i] for i in range(24)] == expect
    base = get_spec("cluener")
    assert (spec.max_seq_len, spec.n_train, spec.n_valid, spec.n_test) == \
        (base.max_seq_len, base.n_train, base.n_valid, base.n_test)


def test_cluener_itself_is_untouched():
    spec = get_spec("cluener")
    assert spec.label_size == 10
    assert spec.entity_types == ["LOC", "PER", "ORG"]


def test_jsonl_loads_fine_and_collapsed(tmp_path):
    #        0 1 2 3 4 5 6 7
    text = "我读红楼梦在市府"
    rec = {"text": text,
           "label": {"book": {text[2:5]: [[2, 4]]},
                     "scene": {text[5]: [[5, 5]]},
                     "government": {text[6:8]: [[6, 7]]}}}
    for name in ("cluener_fine", "cluener"):
        d = tmp_path / name
        d.mkdir()
        (d / "train.json").write_text(
            json.dumps(rec, ensure_ascii=False) + "\n", encoding="utf-8")
    sents, tags = load_data("cluener_fine", str(tmp_path / "cluener_fine"),
                            "train")
    assert sents == [text]
    assert tags == [["O", "O", "B-book", "I-book", "I-book", "B-scene",
                     "B-government", "I-government"]]
    # the collapsed dataset reads the same file as before
    sents, tags = load_data("cluener", str(tmp_path / "cluener"), "train")
    assert sents == [text]
    assert tags == [["O"] * 6 + ["B-ORG", "I-ORG"]]


def test_synthetic_fallback_covers_all_ten_types(tmp_path):
    spec = get_spec("cluener_fine")
    sents, tags = load_data("cluener_fine", str(tmp_path / "absent"), "train")
    assert len(sents) == len(tags) > 0
    seen = set()
    for s, ts in zip(sents, tags):
        assert len(s) == len(ts)
        for t in ts:
            assert t in spec.tag2idx
            if t != "O":
                seen.add(t[2:])
    assert seen == set(TYPES)


def test_nerdataset_batch_labels_below_24(tmp_path):
    from chinesener_amd.data.loader import NerDataset
    pipe = NerDataset(str(tmp_path), "cluener_fine", 4, 1, "bilstm_crf")
    assert pipe.params["label_size"] == 24
    batch = next(iter(pipe.iter_batches("valid", shuffle=False)))
    assert int(batch["label_ids"].max()) < 24
    assert int(batch["label_ids"].min()) >= 0


def test_bilstm_crf_cpu_forward_backward_at_24_labels():
    from chinesener_amd.models import build_model
    torch.manual_seed(0)
    model = build_model("bilstm_crf",
                        make_tiny_params("bilstm_crf", label_size=24))
    batch = make_tiny_batch("bilstm_crf", label_size=24)
    out = model(batch)
    assert torch.isfinite(out.loss)
    out.loss.backward()
    trans = [p for p in model.parameters() if tuple(p.shape) == (24, 24)]
    assert trans and all(p.grad is not None for p in trans)
    with torch.no_grad():
        pred = model.eval()(batch, compute_pred=True).pred_ids
    assert int(pred.max()) < 24
