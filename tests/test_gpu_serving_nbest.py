"""GPU serving with n-best decoding: the captured PREDICT graph also runs
the list-Viterbi kernel and the path posterior of its k paths, and returns
(pred_ids, nbest_paths, nbest_scores, nbest_logp). No atomics anywhere on
the path, so replay and eager agree bit for bit."""
import numpy as np
import pytest

from test_gpu_serving import _cuda, _export_bert

pytestmark = pytest.mark.gpu

L = 32
NBEST_KEYS = ("nbest_paths", "nbest_scores", "nbest_logp")


def _feats(rng, batch):
    feats = {"token_ids": rng.integers(1, 2000, (batch, L)),
             "segment_ids": np.zeros((batch, L), dtype=np.int64),
             "mask": np.ones((batch, L), dtype=np.int64)}
    feats["mask"][batch - 1, 20:] = 0
    return feats


def test_nbest_graph_matches_eager(tmp_path):
    _cuda()
    name = _export_bert(tmp_path)
    from chinesener_amd.serve.engine import InferenceEngine
    eng_graph = InferenceEngine(name, str(tmp_path), batch_sizes=(1, 4),
                                max_seq_len=L, use_graph=True, nbest=4)
    eng_eager = InferenceEngine(name, str(tmp_path), max_seq_len=L,
                                use_graph=False, nbest=4)
    eng_plain = InferenceEngine(name, str(tmp_path), batch_sizes=(1, 4),
                                max_seq_len=L, use_graph=True)
    eng_both = InferenceEngine(name, str(tmp_path), batch_sizes=(4,),
                               max_seq_len=L, use_graph=True,
                               confidence=True, nbest=4)
    for eng in (eng_graph, eng_plain, eng_both):
        eng.warmup()
    assert set(eng_graph._graphs) == {1, 4}
    rng = np.random.default_rng(0)
    for batch in (4, 3, 1):      # 3 pads to the bucket of 4
        feats = _feats(rng, batch)
        got = eng_graph.predict_nbest(feats)
        want = eng_eager.predict_nbest(feats)
        assert set(got) == {"pred_ids"} | set(NBEST_KEYS)
        for key in got:
            np.testing.assert_array_equal(got[key], want[key])
        assert got["nbest_paths"].shape == (batch, 4, L)
        assert got["nbest_logp"].dtype == np.float64
        valid = feats["mask"] == 1
        assert (got["nbest_paths"][~np.broadcast_to(
            valid[:, None, :], got["nbest_paths"].shape)] == 0).all()
        assert np.isfinite(got["nbest_logp"]).all()
        assert (np.exp(got["nbest_logp"]).sum(1) <= 1 + 1e-3).all()
        assert (np.diff(got["nbest_scores"], axis=1) <= 0).all()
        # the plain call, on either engine, decodes the same tags
        np.testing.assert_array_equal(eng_graph.predict(feats),
                                      got["pred_ids"])
        np.testing.assert_array_equal(eng_plain.predict(feats),
                                      got["pred_ids"])
        # combined with confidence: the same n-best, plus the span scores,
        # whose whole-row value is the best path's probability
        both = eng_both.predict_nbest(feats, k=2, scored=True)
        assert set(both) == {"pred_ids", "span_a", "span_b"} | set(NBEST_KEYS)
        np.testing.assert_array_equal(both["pred_ids"], got["pred_ids"])
        for key in NBEST_KEYS:
            np.testing.assert_array_equal(both[key], got[key][:, :2])
        scored = eng_both.predict_scored(feats)
        np.testing.assert_array_equal(scored["span_a"], both["span_a"])
        # rank 0 is pred_ids unless the two best scores tie (bound 1e-3)
        gap = got["nbest_scores"][:, 0] - got["nbest_scores"][:, 1]
        clear = gap > 1e-3
        np.testing.assert_array_equal(got["nbest_paths"][clear, 0],
                                      got["pred_ids"][clear])
        last = feats["mask"].sum(1) - 1
        seq = scored["span_a"][:, 0] + scored["span_b"][np.arange(batch), last]
        np.testing.assert_allclose(got["nbest_logp"][clear, 0], seq[clear],
                                   atol=1e-3, rtol=0)
    with pytest.raises(RuntimeError, match="nbest"):
        eng_plain.predict_nbest(_feats(rng, 1))
    with pytest.raises(RuntimeError, match="nbest=4"):
        eng_graph.predict_nbest(_feats(rng, 1), k=5)
