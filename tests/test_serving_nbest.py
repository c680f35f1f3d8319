"""Serving with n-best decoding, on CPU with a tiny exported bilstm_crf:
engine.predict_nbest, the gRPC option, MicroBatcher coalescing of plain,
scored and nbest callers, InferHelper.infer_nbest, and the model-level
compute_nbest switch. The hipGraph side is in test_gpu_serving_nbest.py."""
import threading

import numpy as np
import pytest
import torch

from chinesener_amd.models import build_model

from conftest import make_tiny_batch, make_tiny_params
from test_serving import _export_tiny, _free_port


def _feats(rng, batch, seq=32):
    return {"token_ids": rng.integers(1, 200, (batch, seq)),
            "mask": np.ones((batch, seq), dtype=np.int64)}


def _engine(tmp_path, **kw):
    from chinesener_amd.serve.engine import InferenceEngine
    # device="cpu": this file is the CPU side, also on a machine with a GPU
    return InferenceEngine("bilstm_crf", str(tmp_path), use_graph=False,
                           max_seq_len=32, device="cpu", **kw)


def test_engine_predict_nbest_matches_model(tmp_path):
    _export_tiny(tmp_path)
    eng = _engine(tmp_path, nbest=4)
    plain = _engine(tmp_path)
    rng = np.random.default_rng(0)
    feats = _feats(rng, 3)
    feats["mask"][1, 20:] = 0
    feats["mask"][2, 1:] = 0
    out = eng.predict_nbest(feats)
    assert set(out) == {"pred_ids", "nbest_paths", "nbest_scores",
                        "nbest_logp"}
    with torch.no_grad():
        direct = eng.model({k: torch.as_tensor(v) for k, v in feats.items()},
                           compute_nbest=4)
    assert direct.span_scores is None
    assert torch.equal(torch.from_numpy(out["pred_ids"]), direct.pred_ids)
    for key, want in zip(("nbest_paths", "nbest_scores", "nbest_logp"),
                         direct.nbest):
        assert torch.equal(torch.from_numpy(out[key]), want), key
    assert out["nbest_paths"].shape == (3, 4, 32)
    assert out["nbest_scores"].dtype == np.float32
    assert out["nbest_logp"].dtype == np.float64
    assert (out["nbest_logp"] <= 1e-9).all()
    assert (np.exp(out["nbest_logp"]).sum(1) <= 1 + 1e-9).all()
    # rank 0 is the decoded path (random weights: no exact ties)
    np.testing.assert_array_equal(out["nbest_paths"][:, 0], out["pred_ids"])
    # a smaller k is a prefix
    two = eng.predict_nbest(feats, k=2)
    assert two["nbest_paths"].shape == (3, 2, 32)
    np.testing.assert_array_equal(two["nbest_paths"], out["nbest_paths"][:, :2])
    np.testing.assert_array_equal(two["nbest_logp"], out["nbest_logp"][:, :2])
    # the plain call is the same on both engines
    pred = eng.predict(feats)
    assert isinstance(pred, np.ndarray)
    np.testing.assert_array_equal(pred, plain.predict(feats))
    np.testing.assert_array_equal(pred, out["pred_ids"])
    with pytest.raises(RuntimeError, match="nbest"):
        plain.predict_nbest(feats)
    with pytest.raises(RuntimeError, match="nbest=4"):
        eng.predict_nbest(feats, k=5)
    with pytest.raises(RuntimeError, match="confidence=True"):
        eng.predict_scored(feats)
    with pytest.raises(RuntimeError, match="confidence=True"):
        eng.predict_nbest(feats, scored=True)
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            _engine(tmp_path, nbest=bad)


def test_engine_confidence_and_nbest_combine(tmp_path):
    _export_tiny(tmp_path)
    both = _engine(tmp_path, confidence=True, nbest=3)
    conf = _engine(tmp_path, confidence=True)
    nb = _engine(tmp_path, nbest=3)
    feats = _feats(np.random.default_rng(3), 2)
    feats["mask"][1, 9:] = 0
    scored = both.predict_scored(feats)
    want = conf.predict_scored(feats)
    assert set(scored) == {"pred_ids", "span_a", "span_b"}
    for key in want:
        np.testing.assert_array_equal(scored[key], want[key])
    got = both.predict_nbest(feats)
    want_nb = nb.predict_nbest(feats)
    for key in want_nb:
        np.testing.assert_array_equal(got[key], want_nb[key])
    allof = both.predict_nbest(feats, k=2, scored=True)
    assert set(allof) == {"pred_ids", "span_a", "span_b", "nbest_paths",
                          "nbest_scores", "nbest_logp"}
    np.testing.assert_array_equal(allof["span_a"], want["span_a"])
    np.testing.assert_array_equal(allof["nbest_paths"],
                                  want_nb["nbest_paths"][:, :2])
    # the best path's probability is the whole-row span score
    rows = np.arange(2)
    last = feats["mask"].sum(1) - 1
    seq = scored["span_a"][:, 0] + scored["span_b"][rows, last]
    np.testing.assert_allclose(got["nbest_logp"][:, 0], seq, atol=1e-12)


def test_grpc_nbest_option(tmp_path):
    import grpc
    _export_tiny(tmp_path)
    from chinesener_amd.serve.client import PredictionClient
    from chinesener_amd.serve.server import serve
    port, port_plain = _free_port(), _free_port()
    server = serve(["bilstm_crf"], str(tmp_path), port=port, wait=False,
                   use_graph=False, nbest=4)
    plain_server = serve(["bilstm_crf"], str(tmp_path), port=port_plain,
                         wait=False, use_graph=False)
    try:
        feats = _feats(np.random.default_rng(1), 2)
        client = PredictionClient(port=port)
        resp = client.predict("bilstm_crf", feats)
        assert set(resp["outputs"]) == {"pred_ids"}
        nb = client.predict("bilstm_crf", feats, options={"nbest": 3})
        assert set(nb["outputs"]) == {"pred_ids", "nbest_paths",
                                      "nbest_scores", "nbest_logp"}
        assert nb["outputs"]["nbest_paths"].shape == (2, 3, 32)
        assert nb["outputs"]["nbest_logp"].shape == (2, 3)
        assert nb["outputs"]["nbest_logp"].dtype == np.float64
        np.testing.assert_array_equal(nb["outputs"]["pred_ids"],
                                      resp["outputs"]["pred_ids"])
        with pytest.raises(grpc.RpcError) as ei:
            client.predict("bilstm_crf", feats, options={"nbest": 5})
        assert ei.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        with pytest.raises(grpc.RpcError) as ei:
            client.predict("bilstm_crf", feats, options={"confidence": True})
        assert ei.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        client.close()

        plain_client = PredictionClient(port=port_plain)
        resp2 = plain_client.predict("bilstm_crf", feats)
        np.testing.assert_array_equal(resp2["outputs"]["pred_ids"],
                                      resp["outputs"]["pred_ids"])
        with pytest.raises(grpc.RpcError) as ei:
            plain_client.predict("bilstm_crf", feats, options={"nbest": 2})
        assert ei.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        assert "--nbest" in ei.value.details()
        plain_client.close()
    finally:
        server.stop(0)
        plain_server.stop(0)


def test_micro_batcher_mixes_plain_scored_and_nbest(tmp_path):
    _export_tiny(tmp_path)
    from chinesener_amd.serve.engine import FastPredict, MicroBatcher
    eng = _engine(tmp_path, confidence=True, nbest=4, batch_sizes=(1, 4, 8))
    batcher = MicroBatcher(eng, window_ms=15.0)
    assert batcher.nbest == 4 and batcher.confidence
    rng = np.random.default_rng(2)
    reqs = [_feats(rng, int(rng.integers(1, 3))) for _ in range(12)]
    want = [eng.predict_nbest(r, scored=True) for r in reqs]
    ks = [None, 2, 4]
    n0 = eng.n_requests
    results = [None] * len(reqs)
    errs = []
    barrier = threading.Barrier(len(reqs))

    def worker(i):
        try:
            barrier.wait()
            if i % 3 == 0:
                results[i] = batcher.predict(reqs[i])
            elif i % 3 == 1:
                results[i] = batcher.predict_scored(reqs[i])
            else:
                results[i] = batcher.predict_nbest(reqs[i], ks[(i // 3) % 3])
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
            if i % 3 == 0:
                assert isinstance(got, np.ndarray)
                np.testing.assert_array_equal(got, exp["pred_ids"])
                continue
            np.testing.assert_array_equal(got["pred_ids"], exp["pred_ids"])
            # The coalesced batch runs the fp32 encoder at another batch
            # size and the CPU GEMMs then round differently: logits move by
            # a few fp32 ulp (<= 1e-6 at |logit| < 8). A path score or a
            # span score sums at most 2*L = 64 such terms, hence 1e-4 (the
            # figure test_serving_confidence.py derives).
            if i % 3 == 1:
                assert set(got) == {"pred_ids", "span_a", "span_b"}
                for key in ("span_a", "span_b"):
                    np.testing.assert_allclose(got[key], exp[key], atol=1e-4,
                                               rtol=0)
                continue
            k = ks[(i // 3) % 3] or 4
            assert set(got) == {"pred_ids", "nbest_paths", "nbest_scores",
                                "nbest_logp"}
            assert got["nbest_paths"].shape == exp["nbest_paths"][:, :k].shape
            np.testing.assert_allclose(got["nbest_scores"],
                                       exp["nbest_scores"][:, :k], atol=1e-4,
                                       rtol=0)
            np.testing.assert_allclose(got["nbest_logp"],
                                       exp["nbest_logp"][:, :k], atol=1e-4,
                                       rtol=0)
            # the best path is pred_ids; lower ranks may swap where two
            # scores are closer than that rounding
            np.testing.assert_array_equal(got["nbest_paths"][:, 0],
                                          got["pred_ids"])
        assert eng.n_requests - n0 < len(reqs)      # they did coalesce
        with pytest.raises(RuntimeError, match="nbest"):
            MicroBatcher(_engine(tmp_path)).predict_nbest(reqs[0])
        with pytest.raises(RuntimeError, match="nbest=4"):
            batcher.predict_nbest(reqs[0], 6)
        fast = FastPredict(eng).predict_nbest(reqs[0], 2)
        np.testing.assert_array_equal(fast["nbest_paths"],
                                      want[0]["nbest_paths"][:, :2])
    finally:
        batcher.close()


def test_infer_helper_nbest(tmp_path):
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
                   use_graph=False, nbest=4)
    try:
        import inference
        helper = inference.InferHelper("bilstm_crf", "msra", port=port,
                                       max_seq_len=32)
        sentence = "北京大学的张三去了上海"
        plain = helper.infer(sentence)
        out = helper.infer_nbest(sentence, 4)
        assert set(out) == {"alternatives", "entities"}
        alts = out["alternatives"]
        assert [a["rank"] for a in alts] == [0, 1, 2, 3]
        probs = [a["prob"] for a in alts]
        assert all(0.0 < p <= 1.0 for p in probs) and sum(probs) <= 1 + 1e-9
        assert probs == sorted(probs, reverse=True)
        regrouped = {}
        for e in alts[0]["entities"]:
            assert set(e) == {"type", "text", "start", "end"}
            regrouped.setdefault(e["type"], set()).add(e["text"])
        assert regrouped == plain                 # rank 0 is infer()'s answer
        assert out["entities"]
        for e in out["entities"]:
            assert set(e) == {"type", "text", "start", "end", "support"}
            assert 0.0 < e["support"] <= 1.0
            assert 0 <= e["start"] <= e["end"] < len(sentence)
        assert len(helper.infer_nbest(sentence, 2)["alternatives"]) == 2
    finally:
        server.stop(0)


@pytest.mark.parametrize("name", ["bilstm_crf", "bert_crf", "bert_ce",
                                  "bert_bilstm_crf_mtl"])
def test_models_compute_nbest(name):
    torch.manual_seed(0)
    mtl = "mtl" in name
    params = make_tiny_params(name)
    model = build_model(name, params).eval()
    batch = make_tiny_batch(name, batch_size=3, seq_len=16, mtl=mtl)
    batch.pop("label_ids", None)
    k = 3
    with torch.no_grad():
        plain = model(batch, compute_pred=True)
        nb = model(batch, compute_nbest=k)
        both = model(batch, compute_conf=True, compute_nbest=k)
        neither = model(batch)
    assert plain.nbest is None and neither.nbest is None
    assert neither.pred_ids is None and nb.span_scores is None
    assert torch.equal(nb.pred_ids, plain.pred_ids)
    assert torch.equal(both.pred_ids, plain.pred_ids)
    paths, scores, logp = nb.nbest
    assert paths.shape == (3, k, 16) and paths.dtype == torch.long
    assert scores.shape == (3, k) and scores.dtype == torch.float32
    assert logp.shape == (3, k) and logp.dtype == torch.float64
    for got, want in zip(both.nbest, nb.nbest):
        assert torch.equal(got, want)
    assert both.span_scores is not None
    mask = batch["mask"].bool()
    assert torch.count_nonzero(paths[~mask[:, None, :].expand_as(paths)]) == 0
    assert torch.equal(paths[:, 0], plain.pred_ids)
    assert torch.isfinite(logp).all() and (logp <= 1e-9).all()
    assert (torch.exp(logp).sum(1) <= 1 + 1e-9).all()
    if name == "bert_ce":  # independent tokens: logp is the score itself
        torch.testing.assert_close(logp, scores.double(), atol=1e-5, rtol=0)
    if mtl:  # each row carries its own task's tower
        with torch.no_grad():
            flipped = dict(batch, task_ids=1 - batch["task_ids"])
            other = model(flipped, compute_nbest=k).nbest
        assert not torch.equal(other[1], scores)


def test_mrc_nbest_decodes_the_text_region():
    """MRC rows are [CLS] query [SEP] text and text_mask selects the text,
    which is no prefix of the row: the n-best paths must cover exactly the
    positions that pred_ids covers."""
    torch.manual_seed(0)
    model = build_model("mrc_bio", make_tiny_params("mrc_bio")).eval()
    B, L, k = 3, 16, 4
    start = torch.tensor([6, 9, 4])             # query lengths incl. CLS/SEP
    end = torch.tensor([16, 13, 5])             # text of 10, 4 and 1 tokens
    pos = torch.arange(L)[None, :]
    text_mask = ((pos >= start[:, None]) & (pos < end[:, None])).long()
    batch = {"token_ids": torch.randint(4, 200, (B, L)),
             "mask": (pos < end[:, None]).long(),
             "segment_ids": (pos >= start[:, None]).long(),
             "text_mask": text_mask}
    with torch.no_grad():
        plain = model(batch, compute_pred=True)
        out = model(batch, compute_nbest=k)
    paths, scores, logp = out.nbest
    assert paths.shape == (B, k, L) and logp.shape == (B, k)
    assert torch.equal(out.pred_ids, plain.pred_ids)
    assert torch.equal(paths[:, 0], plain.pred_ids)
    outside = (text_mask == 0)[:, None, :].expand_as(paths)
    assert torch.count_nonzero(paths[outside]) == 0
    # logp of a path = sum of its log-softmax values over the text region
    lsm = torch.log_softmax(out.logits.double(), -1)
    chosen = lsm.gather(2, paths.transpose(1, 2)).transpose(1, 2)  # [B,k,L]
    want = (chosen * text_mask[:, None, :]).sum(2)
    present = torch.isfinite(logp)
    # row 2 has one text token and 3 labels: 3 paths, the 4th rank absent
    assert present.tolist() == [[True] * 4, [True] * 4, [True] * 3 + [False]]
    # fp32 log-softmax and fp32 scores against the fp64 sum: <= 10 terms of
    # magnitude < 4, 1e-5 is 40 ulp of the largest
    torch.testing.assert_close(logp[present], want[present], atol=1e-5, rtol=0)
    torch.testing.assert_close(scores[present].double(), want[present],
                               atol=1e-5, rtol=0)
    assert (scores[:, 1:] <= scores[:, :-1]).all()
    # distinct paths per row
    for b in range(B):
        rows = {tuple(p.tolist()) for p, ok in zip(paths[b], present[b]) if ok}
        assert len(rows) == int(present[b].sum())
