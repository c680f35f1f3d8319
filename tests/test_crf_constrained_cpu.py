"""Constrained CRF decoding on the CPU: the reference against path
enumeration, its properties, the constraint builders, the models'
constrained=True switch and the serving API on the eager engine. The HIP
kernel is in test_gpu_crf_constrained.py."""
import itertools
import threading

import numpy as np
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.data import constraints as cons
from chinesener_amd.data import partial
from chinesener_amd.data.datasets import get_spec
from chinesener_amd.models import build_model
from chinesener_amd.ops import reference as ref

from conftest import make_tiny_batch, make_tiny_params
from test_serving import _export_tiny, _free_port

NINF = float("-inf")
TAGS = make_tiny_params("bilstm_crf")["tag2idx"]


def _mask(lens, L):
    return (torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]).long()


def _singletons(path):
    return ops.allowed_from_tags(path, torch.ones_like(path, dtype=torch.bool),
                                 0)


def _score(em, trans, path, n):
    s = sum(em[t, path[t]] for t in range(n))
    return s + sum(trans[path[t], path[t + 1]] for t in range(n - 1))


# ------------------------------------------------------------- reference
@pytest.mark.parametrize("T,L,seed", [(4, 6, 0), (3, 5, 1), (4, 1, 2),
                                      (3, 6, 3)])
def test_reference_matches_enumeration(T, L, seed):
    g = torch.Generator().manual_seed(seed)
    B = 48
    em = torch.randn(B, L, T, generator=g, dtype=torch.double)
    trans = torch.randn(T, T, generator=g, dtype=torch.double)
    allowed = torch.randint(0, 1 << T, (B, L), generator=g)
    tallowed = torch.randint(0, 1 << T, (T,), generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    pred, score = ref.crf_decode_constrained(em, allowed, _mask(lens, L),
                                             trans, tallowed)
    sets = ref.allowed_sets(allowed, T)
    tsets = ref.transition_sets(tallowed, T)
    feasible = infeasible = 0
    for b in range(B):
        n = int(lens[b])
        best = None
        for path in itertools.product(range(T), repeat=n):
            if not all(sets[b, t, path[t]] for t in range(n)):
                continue
            if not all(tsets[path[t], path[t + 1]] for t in range(n - 1)):
                continue
            s = _score(em[b], trans, path, n)
            if best is None or s > best[0]:
                best = (s, path)
        if best is None:
            infeasible += 1
            assert score[b].item() == NINF
            assert torch.count_nonzero(pred[b]) == 0
        else:
            feasible += 1
            assert abs(score[b].item() - best[0].item()) < 1e-9
            assert tuple(pred[b, :n].tolist()) == best[1]
            assert torch.count_nonzero(pred[b, n:]) == 0
    assert feasible > 0
    if L > 1:
        assert infeasible > 0       # both kinds of row were checked


@pytest.mark.parametrize("integers", [False, True])
def test_open_words_equal_crf_decode(integers):
    g = torch.Generator().manual_seed(5)
    B, L, T = 9, 12, 5
    if integers:    # tie-heavy
        em = torch.randint(-2, 3, (B, L, T), generator=g).float()
        trans = torch.randint(-2, 3, (T, T), generator=g).float()
    else:
        em = torch.randn(B, L, T, generator=g)
        trans = torch.randn(T, T, generator=g)
    mask = _mask([12, 1, 5, 12, 7, 2, 3, 11, 12], L)
    want = ref.crf_decode(em, mask, trans)
    for words in (torch.zeros(B, L, dtype=torch.int64),
                  torch.full((B, L), -1, dtype=torch.int64),
                  torch.full((B, L), 1 << 40, dtype=torch.int64)):
        pred, score = ref.crf_decode_constrained(em, words, mask, trans)
        assert torch.equal(pred, want)
        for b in range(B):
            n = int(mask[b].sum())
            torch.testing.assert_close(
                score[b], _score(em[b], trans, want[b].tolist(), n),
                atol=1e-4, rtol=0)
    assert ops.crf_viterbi_constrained(
        em, torch.zeros(B, L, dtype=torch.int64), mask, trans)[0].equal(want)


def test_singletons_return_that_path():
    g = torch.Generator().manual_seed(6)
    B, L, T = 4, 7, 64
    em = torch.randn(B, L, T, generator=g, dtype=torch.double)
    trans = torch.randn(T, T, generator=g, dtype=torch.double)
    path = torch.randint(0, T, (B, L), generator=g)
    path[0, 3] = 63                              # the sign bit
    lens = [7, 4, 1, 6]
    mask = _mask(lens, L)
    pred, score = ref.crf_decode_constrained(em, _singletons(path), mask,
                                             trans)
    assert torch.equal(pred, path * mask)
    for b in range(B):
        torch.testing.assert_close(
            score[b], _score(em[b], trans, path[b].tolist(), lens[b]))
    # the only forbidden tag is 63
    em[:, :, 63] += 100.0
    words = torch.full((B, L), (1 << 63) - 1, dtype=torch.int64)
    pred, score = ref.crf_decode_constrained(em, words, mask, trans)
    assert (pred != 63).all() and torch.isfinite(score).all()


def test_rows_are_independent_and_lens():
    g = torch.Generator().manual_seed(7)
    B, L, T = 6, 8, 4
    em = torch.randn(B, L, T, generator=g)
    trans = torch.randn(T, T, generator=g)
    allowed = torch.randint(0, 1 << T, (B, L), generator=g)
    tallowed = torch.randint(1, 1 << T, (T,), generator=g)
    mask = _mask([0, 1, L, 3, L, 0], L)
    pred, score = ref.crf_decode_constrained(em, allowed, mask, trans,
                                             tallowed)
    for b in range(B):
        p1, s1 = ref.crf_decode_constrained(
            em[b:b + 1], allowed[b:b + 1], mask[b:b + 1], trans, tallowed)
        assert torch.equal(pred[b], p1[0]) and torch.equal(score[b], s1[0])
    for b in (0, 5):                             # empty rows
        assert score[b].item() == NINF and torch.count_nonzero(pred[b]) == 0
    # a row of one position: the best allowed emission, no transition used
    s = ref.allowed_sets(allowed[1, 0], T)
    want = torch.where(s, em[1, 0], torch.full((T,), NINF)).max()
    assert score[1] == want
    # an infeasible pair of singletons
    words = torch.zeros(1, L, dtype=torch.int64)
    words[0, 2], words[0, 3] = 1 << 1, 1 << 2
    ta = torch.full((T,), -1, dtype=torch.int64)
    ta[1] = ~(1 << 2)
    p, s = ref.crf_decode_constrained(em[:1], words, _mask([L], L), trans, ta)
    assert s.item() == NINF and torch.count_nonzero(p) == 0


# -------------------------------------------------------------- builders
def test_bio_transition_words_msra():
    t2i = get_spec("msra").tag2idx
    words = cons.bio_transition_words(t2i)
    assert words.dtype == np.int64 and words.shape == (max(t2i.values()) + 1,)
    iloc = 1 << t2i["I-LOC"]
    for src in ("O", "[CLS]", "B-PER", "I-PER", "B-ORG"):
        assert not int(words[t2i[src]]) & iloc, src
    for src in ("B-LOC", "I-LOC"):
        assert int(words[t2i[src]]) & iloc, src
    for src in t2i:     # everything that is not an I- tag stays allowed
        for dst in ("O", "B-LOC", "B-PER", "[SEP]"):
            assert int(words[t2i[src]]) & (1 << t2i[dst])
    # a tagset without B-/I- tags: all ones
    bies = {"[PAD]": 0, "B": 1, "I": 2, "E": 3, "S": 4, "[CLS]": 5, "[SEP]": 6}
    assert (cons.bio_transition_words(bies) == -1).all()


def test_bio_transition_words_bit_63():
    t2i = {"[PAD]": 0, "O": 1}
    for k in range(31):
        t2i[f"B-T{k}"] = 2 + 2 * k
        t2i[f"I-T{k}"] = 3 + 2 * k
    assert t2i["I-T30"] == 63
    words = cons.bio_transition_words(t2i)
    assert words[t2i["B-T30"]] < 0 and words[t2i["I-T30"]] < 0   # bit 63 set
    assert words[t2i["O"]] > 0 and words[t2i["B-T29"]] > 0
    sw = cons.span_words([("T30", 1, 3)], 4, t2i)
    assert sw[2] == -(1 << 63) and sw[1] == 1 << 62
    assert sw[3] == partial.as_int64(partial.open_bits(t2i) & ~(1 << 63))
    fw = cons.forbid_types(np.zeros(2, dtype=np.int64), ["T30"], t2i)
    assert (fw == partial.as_int64(
        partial.open_bits(t2i) & ~(3 << 62))).all()


def test_span_words():
    open_ = partial.open_bits(TAGS)
    w = cons.span_words([("ORG", 0, 4), ("PER", 6, 7)], 9, TAGS)
    assert w.dtype == np.int64 and w.shape == (9,)
    assert w[0] == 1 << TAGS["B-ORG"]
    assert (w[1:4] == 1 << TAGS["I-ORG"]).all()
    assert w[4] == open_ & ~(1 << TAGS["I-ORG"])        # the entity ends here
    assert w[5] == 0
    assert w[6] == 1 << TAGS["B-PER"]
    assert w[7] == open_ & ~(1 << TAGS["I-PER"])
    assert w[8] == 0
    # offset shifts everything; a span up to the end has no "ends here" word
    w = cons.span_words([("LOC", 5, 7)], 8, TAGS, offset=1)
    assert w[6] == 1 << TAGS["B-LOC"] and w[7] == 1 << TAGS["I-LOC"]
    assert (w[:6] == 0).all()
    # adjacent spans: the second one's B- word wins over "ends here"
    w = cons.span_words([("LOC", 0, 2), ("PER", 2, 3)], 4, TAGS)
    assert w[2] == 1 << TAGS["B-PER"]
    assert (cons.span_words([], 5, TAGS) == 0).all()
    for bad in ([("LOC", 0, 3), ("PER", 2, 4)],        # overlap
                [("GPE", 0, 1)],                       # unknown type
                [("LOC", 3, 6)], [("LOC", -1, 2)], [("LOC", 2, 2)]):
        with pytest.raises(ValueError):
            cons.span_words(bad, 5, TAGS)
    with pytest.raises(ValueError):
        cons.span_words([("LOC", 3, 5)], 5, TAGS, offset=1)


def test_forbid_types():
    open_ = partial.open_bits(TAGS)
    w = cons.span_words([("ORG", 1, 3)], 6, TAGS)
    f = cons.forbid_types(w, ["PER", "LOC"], TAGS)
    drop = sum(1 << TAGS[t] for t in ("B-PER", "I-PER", "B-LOC", "I-LOC"))
    assert (f[1:4] == w[1:4]).all()              # hinted positions stay
    assert (f[[0, 4, 5]] == open_ & ~drop).all()
    assert (w[[0, 4, 5]] == 0).all()             # the input is not modified
    with pytest.raises(ValueError):
        cons.forbid_types(w, ["GPE"], TAGS)


# ---------------------------------------------------------------- models
@pytest.mark.parametrize("name", ["bilstm_crf", "bert_bilstm_crf",
                                  "transformer_crf_bichar"])
def test_model_constrained_forward(name):
    torch.manual_seed(0)
    model = build_model(name, make_tiny_params(name)).eval()
    batch = make_tiny_batch(name)
    batch.pop("label_ids")
    mask = batch["mask"]
    with torch.no_grad():
        free = model(batch, compute_pred=True)
        assert free.path_score is None
        zero = dict(batch, constraint_tags=torch.zeros_like(mask))
        out = model(zero, constrained=True)
        assert torch.equal(out.pred_ids, free.pred_ids)
        assert out.path_score.shape == (mask.shape[0],)
        assert torch.isfinite(out.path_score).all()
        assert out.span_scores is None and out.nbest is None
        # every singleton is honoured
        g = torch.Generator().manual_seed(2)
        known = (torch.rand(mask.shape, generator=g) < 0.4) & (mask == 1)
        want = torch.randint(1, 8, mask.shape, generator=g)
        hinted = dict(batch, constraint_tags=ops.allowed_from_tags(
            want, known, 0))
        out = model(hinted, constrained=True, compute_conf=True)
        assert torch.equal(out.pred_ids[known], want[known])
        assert torch.isfinite(out.path_score).all()
        a, b = ref.crf_path_posterior(out.logits, mask,
                                      model.crf.transitions, out.pred_ids)
        torch.testing.assert_close(out.span_scores[0], a)
        torch.testing.assert_close(out.span_scores[1], b)
        with pytest.raises(KeyError, match="constraint_tags"):
            model(batch, constrained=True)
        with pytest.raises(ValueError, match="nbest"):
            model(zero, constrained=True, compute_nbest=2)
        # the training key is not the decoding key
        part = dict(batch, allowed_tags=hinted["constraint_tags"])
        assert torch.equal(model(part, compute_pred=True).pred_ids,
                           free.pred_ids)


@pytest.mark.parametrize("name", ["bert_bilstm_crf_mtl", "bert_ce",
                                  "mrc_bio"])
def test_other_heads_reject_constrained(name):
    torch.manual_seed(0)
    model = build_model(name, make_tiny_params(name)).eval()
    batch = make_tiny_batch(name, mtl=name.endswith("mtl"))
    batch["constraint_tags"] = torch.zeros_like(batch["mask"])
    with pytest.raises(ValueError, match="constrained"):
        model(batch, constrained=True)


def test_bio_transitions_remove_ill_formed_rows():
    torch.manual_seed(0)
    model = build_model("bilstm_crf", make_tiny_params("bilstm_crf")).eval()
    keys_before = set(model.state_dict())
    with torch.no_grad():        # make O -> I-ORG and B-PER -> I-LOC attractive
        model.crf.transitions.zero_()
        model.crf.transitions[TAGS["O"], TAGS["I-ORG"]] = 6.0
        model.crf.transitions[TAGS["B-PER"], TAGS["I-LOC"]] = 6.0
        model.crf.transitions[TAGS["I-ORG"], TAGS["B-PER"]] = 3.0
    batch = make_tiny_batch("bilstm_crf", batch_size=6)
    batch.pop("label_ids")
    # position 0 has no predecessor: its word closes the I- tags, the
    # transition words do the rest
    no_i = partial.open_bits(TAGS) & ~sum(
        1 << i for t, i in TAGS.items() if t.startswith("I-"))
    batch["constraint_tags"] = torch.zeros_like(batch["mask"])
    batch["constraint_tags"][:, 0] = no_i
    idx2tag = {v: k for k, v in TAGS.items()}

    def ill_formed(pred):
        bad = 0
        for row, m in zip(pred.tolist(), batch["mask"].tolist()):
            tags = [idx2tag[i] for i, keep in zip(row, m) if keep]
            for t, tag in enumerate(tags):
                if tag.startswith("I-"):
                    prev = tags[t - 1] if t else "O"
                    bad += prev not in (f"B-{tag[2:]}", f"I-{tag[2:]}")
        return bad

    with torch.no_grad():
        free = model(batch, constrained=True)
        assert ill_formed(free.pred_ids) > 0     # else this shows nothing
        model.crf.constrain_transitions(cons.bio_transition_words(TAGS))
        out = model(batch, constrained=True)
        assert ill_formed(out.pred_ids) == 0
        assert torch.isfinite(out.path_score).all()
        assert (out.path_score <= free.path_score).all()
        # free decoding is untouched, and so is the checkpoint
        plain = model(batch, compute_pred=True).pred_ids
        assert ill_formed(plain) > 0
        assert set(model.state_dict()) == keys_before
        model.crf.constrain_transitions(None)
        assert torch.equal(model(batch, constrained=True).pred_ids,
                           free.pred_ids)
    with pytest.raises(ValueError):
        model.crf.constrain_transitions(np.zeros(3, dtype=np.int64))


def test_complete_annotations_keeps_annotated_tags():
    torch.manual_seed(0)
    model = build_model("bilstm_crf", make_tiny_params("bilstm_crf")).train()
    batch = make_tiny_batch("bilstm_crf")
    g = torch.Generator().manual_seed(1)
    known = (torch.rand(batch["mask"].shape, generator=g) < 0.5)
    batch["allowed_tags"] = ops.allowed_from_tags(
        batch["label_ids"], known, partial.open_bits(TAGS))
    pred, score = partial.complete_annotations(model, batch)
    live = known & (batch["mask"] == 1)
    assert torch.equal(pred[live], batch["label_ids"][live])
    assert torch.isfinite(score).all()
    assert model.training                        # mode restored
    sets = ref.allowed_sets(batch["allowed_tags"], 10)
    inside = sets.gather(2, pred[:, :, None]).squeeze(2)
    assert inside[batch["mask"] == 1].all()
    with pytest.raises(KeyError):
        partial.complete_annotations(model, make_tiny_batch("bilstm_crf"))


# --------------------------------------------------------------- serving
# the exported tiny model has 7 labels
STAGS = {"[PAD]": 0, "O": 1, "B-ORG": 2, "I-ORG": 3, "B-PER": 4, "I-PER": 5,
         "[SEP]": 6}


def _feats(rng, batch, seq=32):
    return {"token_ids": rng.integers(1, 200, (batch, seq)),
            "mask": np.ones((batch, seq), dtype=np.int64)}


def _engine(tmp_path, **kw):
    from chinesener_amd.serve.engine import InferenceEngine
    return InferenceEngine("bilstm_crf", str(tmp_path), use_graph=False,
                           max_seq_len=32, device="cpu", **kw)


def _hints(batch, seq=32):
    words = np.zeros((batch, seq), dtype=np.int64)
    words[0] = cons.span_words([("ORG", 2, 5), ("PER", 9, 10)], seq, STAGS)
    return words


def _check_hints(pred):
    assert pred[0, 2] == STAGS["B-ORG"]
    assert (pred[0, 3:5] == STAGS["I-ORG"]).all()
    assert pred[0, 5] != STAGS["I-ORG"]
    assert pred[0, 9] == STAGS["B-PER"] and pred[0, 10] != STAGS["I-PER"]


def test_engine_predict_constrained(tmp_path):
    _export_tiny(tmp_path)
    eng = _engine(tmp_path, constraints=True)
    plain = _engine(tmp_path)
    assert eng.out_keys == ("pred_ids", "path_score")
    rng = np.random.default_rng(0)
    feats = _feats(rng, 3)
    feats["mask"][1, 20:] = 0
    hinted = dict(feats, constraint_tags=_hints(3))
    out = eng.predict_constrained(hinted)
    assert set(out) == {"pred_ids", "path_score"}
    assert out["path_score"].dtype == np.float32
    assert np.isfinite(out["path_score"]).all()
    _check_hints(out["pred_ids"])
    # a plain request on a constraints engine is free decoding
    want = plain.predict(feats)
    np.testing.assert_array_equal(eng.predict(feats), want)
    free = eng.predict_constrained(feats)
    np.testing.assert_array_equal(free["pred_ids"], want)
    assert (free["path_score"] >= out["path_score"]).all()
    np.testing.assert_array_equal(out["pred_ids"][1:], want[1:])
    # refusals
    with pytest.raises(RuntimeError, match="constraints=True"):
        plain.predict(hinted)
    with pytest.raises(RuntimeError, match="constraints=True"):
        plain.predict_constrained(feats)
    with pytest.raises(RuntimeError, match="confidence=True"):
        eng.predict_constrained(hinted, scored=True)
    with pytest.raises(ValueError, match="nbest"):
        _engine(tmp_path, constraints=True, nbest=2)
    # with confidence: the span scores of the constrained path
    both = _engine(tmp_path, constraints=True, confidence=True)
    scored = both.predict_constrained(hinted, scored=True)
    assert set(scored) == {"pred_ids", "path_score", "span_a", "span_b"}
    np.testing.assert_array_equal(scored["pred_ids"], out["pred_ids"])
    # BIO transitions applied once at construction
    bio = _engine(tmp_path, constraints=True,
                  trans_allowed=cons.bio_transition_words(STAGS))
    assert bio.model.crf.trans_allowed is not None
    assert "crf.trans_allowed" not in bio.model.state_dict()
    _check_hints(bio.predict_constrained(hinted)["pred_ids"])


def test_microbatcher_coalesces_hinted_and_plain(tmp_path):
    _export_tiny(tmp_path)
    from chinesener_amd.serve.engine import FastPredict, MicroBatcher
    eng = _engine(tmp_path, constraints=True)
    rng = np.random.default_rng(1)
    f_hint = dict(_feats(rng, 2), constraint_tags=_hints(2))
    f_plain = _feats(rng, 1)
    want_hint = eng.predict_constrained(f_hint)
    want_plain = eng.predict(f_plain)
    base = eng.n_requests
    # dispatches as soon as both requests (3 rows) are queued
    mb = MicroBatcher(eng, max_batch=3, window_ms=5000.0)
    try:
        got = {}
        barrier = threading.Barrier(2)

        def hinted():
            barrier.wait()
            got["hint"] = mb.predict_constrained(f_hint)

        def plain():
            barrier.wait()
            got["plain"] = mb.predict(f_plain)

        threads = [threading.Thread(target=f) for f in (hinted, plain)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(30)
        assert eng.n_requests == base + 1        # one replay for both
        for key in want_hint:
            np.testing.assert_array_equal(got["hint"][key], want_hint[key])
        np.testing.assert_array_equal(got["plain"], want_plain)
        _check_hints(got["hint"]["pred_ids"])
    finally:
        mb.close()
    fp = FastPredict(eng).predict_constrained(f_hint)
    np.testing.assert_array_equal(fp["pred_ids"], want_hint["pred_ids"])
    mb_plain = MicroBatcher(_engine(tmp_path), window_ms=0.1)
    try:
        with pytest.raises(RuntimeError, match="constraints=True"):
            mb_plain.predict_constrained(f_plain)
        with pytest.raises(RuntimeError, match="constraints=True"):
            mb_plain.predict(f_hint)
    finally:
        mb_plain.close()


def test_grpc_constraint_tags(tmp_path):
    import grpc
    _export_tiny(tmp_path)
    from chinesener_amd.serve.client import PredictionClient
    from chinesener_amd.serve.server import serve
    port, port_plain = _free_port(), _free_port()
    server = serve(["bilstm_crf"], str(tmp_path), port=port, wait=False,
                   use_graph=False, constraints=True,
                   trans_allowed=cons.bio_transition_words(STAGS))
    plain_server = serve(["bilstm_crf"], str(tmp_path), port=port_plain,
                         wait=False, use_graph=False)
    try:
        feats = _feats(np.random.default_rng(2), 2)
        hinted = dict(feats, constraint_tags=_hints(2))
        client = PredictionClient(port=port)
        resp = client.predict("bilstm_crf", hinted)
        assert set(resp["outputs"]) == {"pred_ids", "path_score"}
        _check_hints(resp["outputs"]["pred_ids"])
        assert set(client.predict("bilstm_crf", feats)["outputs"]) == {
            "pred_ids"}
        client.close()
        plain_client = PredictionClient(port=port_plain)
        with pytest.raises(grpc.RpcError) as ei:
            plain_client.predict("bilstm_crf", hinted)
        assert ei.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        assert "--constraints" in ei.value.details()
        plain_client.close()
    finally:
        server.stop(0)
        plain_server.stop(0)


def test_infer_helper_constrained(tmp_path):
    _export_tiny(tmp_path, vocab_size=None)
    port = _free_port()
    from chinesener_amd.serve.server import serve
    # the 7-label export knows the O, LOC and PER tags of the msra map; with
    # well-formed BIO enforced, a hinted entity is not glued to a neighbour
    known = {t: i for t, i in get_spec("msra").tag2idx.items() if i < 7}
    server = serve(["bilstm_crf"], str(tmp_path), port=port, wait=False,
                   use_graph=False, constraints=True,
                   trans_allowed=cons.bio_transition_words(known))
    try:
        import inference
        helper = inference.InferHelper("bilstm_crf", "msra", port=port,
                                       max_seq_len=32)
        sentence = "北京大学的张三去了上海"
        out = helper.infer_constrained(sentence, [("PER", 5, 7),
                                                  ("LOC", 9, 11)])
        assert set(out) == {"entities", "feasible", "path_score"}
        assert out["feasible"] and np.isfinite(out["path_score"])
        assert "张三" in out["entities"]["PER"]
        assert "上海" in out["entities"]["LOC"]
        none = helper.infer_constrained(sentence, forbid=["PER", "LOC"])
        assert none["feasible"]
        assert not none["entities"].get("PER")
        assert not none["entities"].get("LOC")
        words = helper.constraint_words(len(sentence), [("LOC", 0, 2)],
                                        ["PER"])
        assert words.shape == (1, 32) and words.dtype == np.int64
        assert words[0, 0] == 1 << 2 and words[0, 1] == 1 << 3
        assert (words[0, len(sentence):] == 0).all()     # padding: unknown
        with pytest.raises(ValueError):
            helper.infer_constrained(sentence, [("GPE", 0, 2)])
    finally:
        server.stop(0)
