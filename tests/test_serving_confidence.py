"""Serving with entity confidence, on CPU with a tiny exported bilstm_crf:
engine.predict_scored, the gRPC option, MicroBatcher coalescing of scored
and plain callers, and InferHelper.infer_scored. The hipGraph side is in
test_gpu_serving_confidence.py."""
import threading

import numpy as np
import pytest
import torch

from test_serving import _export_tiny, _free_port


def _feats(rng, batch, seq=32):
    return {"token_ids": rng.integers(1, 200, (batch, seq)),
            "mask": np.ones((batch, seq), dtype=np.int64)}


def _engine(tmp_path, confidence, **kw):
    from chinesener_amd.serve.engine import InferenceEngine
    # device="cpu": this file is the CPU side (the direct model call below
    # feeds CPU tensors), also on a machine that has a GPU
    return InferenceEngine("bilstm_crf", str(tmp_path), use_graph=False,
                           max_seq_len=32, confidence=confidence,
                           device="cpu", **kw)


def test_engine_predict_scored_matches_model(tmp_path):
    _export_tiny(tmp_path)
    eng = _engine(tmp_path, confidence=True)
    plain = _engine(tmp_path, confidence=False)
    rng = np.random.default_rng(0)
    feats = _feats(rng, 3)
    feats["mask"][1, 20:] = 0
    feats["mask"][2, 1:] = 0
    out = eng.predict_scored(feats)
    assert set(out) == {"pred_ids", "span_a", "span_b"}
    with torch.no_grad():
        direct = eng.model({k: torch.as_tensor(v) for k, v in feats.items()},
                           compute_conf=True)
    assert torch.equal(torch.from_numpy(out["pred_ids"]), direct.pred_ids)
    assert out["span_a"].dtype == np.float64
    assert torch.equal(torch.from_numpy(out["span_a"]), direct.span_scores[0])
    assert torch.equal(torch.from_numpy(out["span_b"]), direct.span_scores[1])
    # the plain call is the same on both engines
    pred = eng.predict(feats)
    assert isinstance(pred, np.ndarray)
    np.testing.assert_array_equal(pred, plain.predict(feats))
    np.testing.assert_array_equal(pred, out["pred_ids"])
    with pytest.raises(RuntimeError, match="confidence=True"):
        plain.predict_scored(feats)


def test_grpc_confidence_option(tmp_path):
    import grpc
    _export_tiny(tmp_path)
    from chinesener_amd.serve import rpc
    from chinesener_amd.serve.client import PredictionClient
    from chinesener_amd.serve.server import serve
    assert "options" not in rpc.make_predict_request("m", {})
    port, port_plain = _free_port(), _free_port()
    server = serve(["bilstm_crf"], str(tmp_path), port=port, wait=False,
                   use_graph=False, confidence=True)
    plain_server = serve(["bilstm_crf"], str(tmp_path), port=port_plain,
                         wait=False, use_graph=False)
    try:
        feats = _feats(np.random.default_rng(1), 2)
        client = PredictionClient(port=port)
        scored = client.predict("bilstm_crf", feats,
                                options={"confidence": True})
        assert set(scored["outputs"]) == {"pred_ids", "span_a", "span_b"}
        assert scored["outputs"]["span_a"].shape == (2, 32)
        assert scored["outputs"]["span_a"].dtype == np.float64
        resp = client.predict("bilstm_crf", feats)
        assert set(resp["outputs"]) == {"pred_ids"}
        assert set(resp) == {"outputs", "model_spec", "latency_ms"}
        np.testing.assert_array_equal(resp["outputs"]["pred_ids"],
                                      scored["outputs"]["pred_ids"])
        client.close()

        plain_client = PredictionClient(port=port_plain)
        resp2 = plain_client.predict("bilstm_crf", feats)
        assert set(resp2["outputs"]) == {"pred_ids"}
        np.testing.assert_array_equal(resp2["outputs"]["pred_ids"],
                                      resp["outputs"]["pred_ids"])
        with pytest.raises(grpc.RpcError) as ei:
            plain_client.predict("bilstm_crf", feats,
                                 options={"confidence": True})
        assert ei.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        plain_client.close()
    finally:
        server.stop(0)
        plain_server.stop(0)


def test_micro_batcher_mixes_scored_and_plain(tmp_path):
    _export_tiny(tmp_path)
    from chinesener_amd.serve.engine import MicroBatcher
    eng = _engine(tmp_path, confidence=True, batch_sizes=(1, 4, 8))
    batcher = MicroBatcher(eng, window_ms=15.0)
    rng = np.random.default_rng(2)
    reqs = [_feats(rng, int(rng.integers(1, 3))) for _ in range(10)]
    want = [eng.predict_scored(r) for r in reqs]
    n0 = eng.n_requests
    results = [None] * len(reqs)
    errs = []
    barrier = threading.Barrier(len(reqs))

    def worker(i):
        try:
            barrier.wait()
            if i % 2:
                results[i] = batcher.predict_scored(reqs[i])
            else:
                results[i] = batcher.predict(reqs[i])
        except Exception as e:
            errs.append((i, e))

    threads = [threading.Thread(target=worker, args=(i,))
               for i in range(len(reqs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    try:
        assert not errs, errs
        for i, (got, exp) in enumerate(zip(results, want)):
            if i % 2:
                assert set(got) == {"pred_ids", "span_a", "span_b"}
                np.testing.assert_array_equal(got["pred_ids"], exp["pred_ids"])
                # The coalesced batch runs the fp32 encoder at another batch
                # size, and the CPU GEMMs then round differently: logits move
                # by a few fp32 ulp (<= 1e-6 at |logit| < 8). A span score
                # sums at most 2*L = 64 such terms, hence 1e-4; the scoring
                # itself is fp64 and adds nothing to it.
                for k in ("span_a", "span_b"):
                    np.testing.assert_allclose(got[k], exp[k], atol=1e-4,
                                               rtol=0)
            else:
                assert isinstance(got, np.ndarray)
                np.testing.assert_array_equal(got, exp["pred_ids"])
        assert eng.n_requests - n0 < len(reqs)      # they did coalesce
        with pytest.raises(RuntimeError, match="confidence=True"):
            MicroBatcher(_engine(tmp_path, confidence=False)) \
                .predict_scored(reqs[0])
    finally:
        batcher.close()


def test_infer_helper_scored(tmp_path):
    model, params, _ = _export_tiny(tmp_path, vocab_size=None)
    # random weights rarely decode an entity: push the B-/I- tags (ids >= 2)
    # up and export that as the newest version
    from chinesener_amd.serve.export import export_model
    with torch.no_grad():
        model.logits.bias[:2] -= 4.0
    export_model(model, "bilstm_crf", params, export_root=str(tmp_path),
                 version=2 ** 40)
    port = _free_port()
    from chinesener_amd.serve.server import serve
    server = serve(["bilstm_crf"], str(tmp_path), port=port, wait=False,
                   use_graph=False, confidence=True)
    try:
        import inference
        helper = inference.InferHelper("bilstm_crf", "msra", port=port,
                                       max_seq_len=32)
        sentence = "北京大学的张三去了上海"
        plain = helper.infer(sentence)
        scored = helper.infer_scored(sentence)
        assert isinstance(scored, list) and scored
        regrouped = {}
        for e in scored:
            assert set(e) == {"type", "text", "start", "end", "confidence"}
            assert 0.0 < e["confidence"] <= 1.0
            assert 0 <= e["start"] <= e["end"] < len(sentence)
            regrouped.setdefault(e["type"], set()).add(e["text"])
        assert regrouped == plain
    finally:
        server.stop(0)
