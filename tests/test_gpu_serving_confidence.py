"""GPU serving with confidence: the captured PREDICT graph also runs the
CRF path-posterior kernel and returns (pred_ids, span_a, span_b). No atomics
anywhere on the path, so replay and eager agree bit for bit."""
import numpy as np
import pytest

from test_gpu_serving import _cuda, _export_bert

pytestmark = pytest.mark.gpu


def _feats(rng, batch):
    feats = {"token_ids": rng.integers(1, 2000, (batch, 64)),
             "segment_ids": np.zeros((batch, 64), dtype=np.int64),
             "mask": np.ones((batch, 64), dtype=np.int64)}
    feats["mask"][batch - 1, 40:] = 0
    return feats


def test_confidence_graph_matches_eager(tmp_path):
    _cuda()
    name = _export_bert(tmp_path)
    from chinesener_amd.serve.engine import InferenceEngine
    eng_graph = InferenceEngine(name, str(tmp_path), batch_sizes=(1, 4),
                                max_seq_len=64, use_graph=True,
                                confidence=True)
    eng_eager = InferenceEngine(name, str(tmp_path), max_seq_len=64,
                                use_graph=False, confidence=True)
    eng_plain = InferenceEngine(name, str(tmp_path), batch_sizes=(1, 4),
                                max_seq_len=64, use_graph=True)
    eng_graph.warmup()
    eng_plain.warmup()
    assert set(eng_graph._graphs) == {1, 4}
    rng = np.random.default_rng(0)
    for batch in (4, 3, 1):      # 3 pads to the bucket of 4
        feats = _feats(rng, batch)
        got = eng_graph.predict_scored(feats)
        want = eng_eager.predict_scored(feats)
        assert set(got) == {"pred_ids", "span_a", "span_b"}
        for k in got:
            assert got[k].shape == (batch, 64)
            np.testing.assert_array_equal(got[k], want[k])
        assert got["span_a"].dtype == np.float64
        valid = feats["mask"] == 1
        assert (got["span_a"][~valid] == 0).all()
        assert (got["span_b"][~valid] == 0).all()
        tok = (got["span_a"] + got["span_b"])[valid]   # token marginals
        assert np.isfinite(tok).all() and (tok <= 1e-3).all()
        # the plain call, on either engine, decodes the same tags
        np.testing.assert_array_equal(eng_graph.predict(feats),
                                      got["pred_ids"])
        np.testing.assert_array_equal(eng_plain.predict(feats),
                                      got["pred_ids"])
    with pytest.raises(RuntimeError, match="confidence=True"):
        eng_plain.predict_scored(_feats(rng, 1))
