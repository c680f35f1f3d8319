"""GPU serving with constrained decoding: the captured PREDICT graph decodes
with the constrained Viterbi kernel under the constraint_tags static input
and returns (pred_ids, path_score). The kernel has no atomics, so replay and
eager agree bit for bit."""
import numpy as np
import pytest
import torch

from chinesener_amd.data.constraints import bio_transition_words, span_words

from conftest import make_tiny_params
from test_gpu_serving import _cuda, _export_bert

pytestmark = pytest.mark.gpu

L = 32
TAGS = make_tiny_params("bert_bilstm_crf")["tag2idx"]     # 10 tags


def _feats(rng, batch):
    feats = {"token_ids": rng.integers(1, 2000, (batch, L)),
             "segment_ids": np.zeros((batch, L), dtype=np.int64),
             "mask": np.ones((batch, L), dtype=np.int64)}
    feats["mask"][batch - 1, 20:] = 0
    return feats


def _hints(batch):
    words = np.zeros((batch, L), dtype=np.int64)
    words[0] = span_words([("ORG", 2, 5), ("PER", 9, 10)], L, TAGS, offset=1)
    return words


def _check_hints(pred):
    assert pred[0, 3] == TAGS["B-ORG"]
    assert (pred[0, 4:6] == TAGS["I-ORG"]).all()
    assert pred[0, 6] != TAGS["I-ORG"]
    assert pred[0, 10] == TAGS["B-PER"] and pred[0, 11] != TAGS["I-PER"]


def test_constrained_graph_matches_eager(tmp_path):
    _cuda()
    name = _export_bert(tmp_path)
    from chinesener_amd.serve.engine import InferenceEngine
    bio = bio_transition_words(TAGS)
    eng = InferenceEngine(name, str(tmp_path), batch_sizes=(1, 4),
                          max_seq_len=L, use_graph=True, constraints=True,
                          trans_allowed=bio)
    eng.warmup()
    assert set(eng._graphs) == {1, 4}
    assert "constraint_tags" in eng._graphs[1].static_in
    rng = np.random.default_rng(0)
    for batch in (4, 3, 1):      # 3 pads to the bucket of 4
        feats = _feats(rng, batch)
        hinted = dict(feats, constraint_tags=_hints(batch))
        got = eng.predict_constrained(hinted)
        assert set(got) == {"pred_ids", "path_score"}
        _check_hints(got["pred_ids"])
        assert np.isfinite(got["path_score"]).all()
        assert (got["pred_ids"][feats["mask"] == 0] == 0).all()
        # the request after a hinted one is plain: none of the first one's
        # words may be left in the static buffer
        plain = eng.predict_constrained(feats)
        dev = {k: torch.as_tensor(v).cuda() for k, v in feats.items()}
        dev["constraint_tags"] = torch.zeros_like(dev["mask"])
        with torch.no_grad():
            want = eng.model(dev, constrained=True)
        np.testing.assert_array_equal(plain["pred_ids"],
                                      want.pred_ids.cpu().numpy())
        np.testing.assert_array_equal(plain["path_score"],
                                      want.path_score.cpu().numpy())
        np.testing.assert_array_equal(eng.predict(feats), plain["pred_ids"])
        assert (plain["path_score"] >= got["path_score"]).all()
        # and the hinted request against eager too
        dev["constraint_tags"] = torch.as_tensor(
            hinted["constraint_tags"]).cuda()
        with torch.no_grad():
            want = eng.model(dev, constrained=True)
        np.testing.assert_array_equal(got["pred_ids"],
                                      want.pred_ids.cpu().numpy())
        np.testing.assert_array_equal(got["path_score"],
                                      want.path_score.cpu().numpy())
