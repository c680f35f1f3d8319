"""CRF path posterior on CPU: the fp64 reference against brute-force
enumeration, its row handling and identities, entity scoring, and the
model-level compute_conf switch."""
import itertools
import math

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.eval import decode_prediction, decode_prediction_scored
from chinesener_amd.models import build_model
from chinesener_amd.ops import reference as ref

from conftest import make_tiny_batch, make_tiny_params


def _rand(B, L, T, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    # fp64 values that fp32 holds exactly: ref.crf_log_likelihood rounds its
    # emissions to fp32, and the identity test compares against it at 1e-8
    em = torch.randn(B, L, T, generator=g).double()
    trans = torch.randn(T, T, generator=g, dtype=torch.float64)
    path = torch.randint(0, T, (B, L), generator=g)
    lens = torch.tensor(lens if lens is not None else [L] * B)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return em, trans, path, mask, lens


def _brute_span_logp(em, trans, path):
    """{(s, e): log P(y_s..y_e = path_s..path_e | x)} for one full-length
    row by enumerating every tag sequence."""
    L, T = em.shape
    scores = {}
    for y in itertools.product(range(T), repeat=L):
        sc = em[0, y[0]].item()
        for t in range(1, L):
            sc += trans[y[t - 1], y[t]].item() + em[t, y[t]].item()
        scores[y] = sc
    log_z = torch.logsumexp(torch.tensor(list(scores.values()),
                                         dtype=torch.float64), 0).item()
    p = path.tolist()
    out = {}
    for s in range(L):
        for e in range(s, L):
            hit = [sc for y, sc in scores.items()
                   if list(y[s:e + 1]) == p[s:e + 1]]
            out[(s, e)] = torch.logsumexp(
                torch.tensor(hit, dtype=torch.float64), 0).item() - log_z
    return out


@pytest.mark.parametrize("T,L", [(3, 5), (4, 4)])
def test_reference_matches_enumeration(T, L):
    em, trans, path, mask, _ = _rand(1, L, T, seed=T * 10 + L)
    a, b = ref.crf_path_posterior(em, mask, trans, path)
    assert a.dtype == torch.float64
    brute = _brute_span_logp(em[0], trans, path[0])
    for (s, e), want in brute.items():
        got = (a[0, s] + b[0, e]).item()
        assert abs(got - want) <= 1e-10, (s, e, got, want)


def test_reference_row_handling():
    L, T = 6, 5
    em, trans, path, mask, lens = _rand(4, L, T, seed=1, lens=[0, 1, 2, L])
    a, b = ref.crf_path_posterior(em, mask, trans, path)
    assert torch.count_nonzero(a[mask == 0]) == 0
    assert torch.count_nonzero(b[mask == 0]) == 0
    assert torch.count_nonzero(a[0]) == 0 and torch.count_nonzero(b[0]) == 0
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    # each row equals the same row evaluated alone at its own length
    for r in range(1, 4):
        n = int(lens[r])
        a1, b1 = ref.crf_path_posterior(em[r:r + 1, :n], mask[r:r + 1, :n],
                                        trans, path[r:r + 1, :n])
        torch.testing.assert_close(a[r, :n], a1[0], atol=1e-12, rtol=0)
        torch.testing.assert_close(b[r, :n], b1[0], atol=1e-12, rtol=0)
    assert (a[mask == 1] >= -1e-12).all() and (b[mask == 1] <= 1e-12).all()


def test_reference_single_tag_is_certain():
    em, trans, path, mask, _ = _rand(3, 7, 1, seed=2, lens=[7, 3, 1])
    a, b = ref.crf_path_posterior(em, mask, trans, path)
    torch.testing.assert_close(a, torch.zeros_like(a), atol=1e-12, rtol=0)
    torch.testing.assert_close(b, torch.zeros_like(b), atol=1e-12, rtol=0)


def test_reference_identities():
    B, L, T = 4, 33, 21
    em, trans, path, mask, lens = _rand(B, L, T, seed=3, lens=[33, 17, 2, 9])
    a, b = ref.crf_path_posterior(em, mask, trans, path)
    # whole-sequence span == path log-likelihood
    ll = ref.crf_log_likelihood(em, path, mask, trans)
    assert ll.dtype == torch.float64
    seq = a[:, 0] + b[torch.arange(B), lens - 1]
    torch.testing.assert_close(seq, ll, atol=1e-8, rtol=0)
    # nested spans are monotone: a wider span is never more probable
    for r in range(B):
        n = int(lens[r])
        logp = a[r, :n, None] + b[r, None, :n]          # [s, e]
        for s in range(n):
            for e in range(s, n):
                if s + 1 <= e:
                    assert logp[s, e] <= logp[s + 1, e] + 1e-8
                    assert logp[s, e] <= logp[s, e - 1] + 1e-8
                assert logp[s, e] <= 1e-8


def test_reference_clamps_path_ids():
    B, L, T = 2, 9, 6
    em, trans, path, mask, _ = _rand(B, L, T, seed=4, lens=[9, 5])
    bad = path.clone()
    bad[0, 2], bad[0, 5], bad[1, 1] = -3, T + 5, T + 5
    a, b = ref.crf_path_posterior(em, mask, trans, bad)
    a2, b2 = ref.crf_path_posterior(em, mask, trans, bad.clamp(0, T - 1))
    assert torch.equal(a, a2) and torch.equal(b, b2)


def test_op_dispatches_to_reference_without_grad():
    em, trans, path, mask, _ = _rand(2, 8, 5, seed=5, lens=[8, 3])
    em32 = em.float().requires_grad_()
    tr32 = trans.float().requires_grad_()
    a, b = ops.crf_path_posterior(em32, mask, tr32, path)
    assert a.dtype == torch.float64 and not a.requires_grad
    assert not b.requires_grad
    ra, rb = ref.crf_path_posterior(em32, mask, tr32, path)
    assert torch.equal(a, ra) and torch.equal(b, rb)
    pred, a2, b2 = ops.crf_decode_scored(em32, mask, tr32)
    assert torch.equal(pred, ops.crf_viterbi(em32, mask, tr32))
    ra2, _ = ref.crf_path_posterior(em32, mask, tr32, pred)
    assert torch.equal(a2, ra2)


# ------------------------------------------------------------ entity scoring
def test_decode_prediction_scored_hand_cases():
    tokens = list("甲乙丙丁戊己庚辛")
    #          0      1        2        3    4        5        6    7
    tags = ["I-LOC", "I-LOC", "B-PER", "O", "B-ORG", "I-PER", "O", "B-LOC"]
    n = len(tokens)
    span_a = [0.1 * (t + 1) for t in range(n)]
    span_b = [-0.2 * (t + 1) for t in range(n)]
    ents = decode_prediction_scored(tokens, tags, span_a, span_b)
    assert [(e["type"], e["text"], e["start"], e["end"]) for e in ents] == [
        ("LOC", "甲乙", 0, 1),            # I- without a B- opens a span
        ("PER", "丙", 2, 2),
        ("ORG", "戊己[ERROR]", 4, 5),      # type mismatch inside the span
        ("LOC", "辛", 7, 7),              # entity at the last token
    ]
    for e in ents:
        want = math.exp(min(0.0, span_a[e["start"]] + span_b[e["end"]]))
        assert e["confidence"] == pytest.approx(want, abs=1e-15)
        assert 0.0 < e["confidence"] <= 1.0
    # [CLS] offset: the score row is shifted by one against the tokens
    sa, sb = [9.0] + span_a, [9.0] + span_b
    shifted = decode_prediction_scored(tokens, tags, sa, sb, offset=1)
    assert shifted == ents
    # a positive sum (rounding) is capped at probability 1
    one = decode_prediction_scored(["甲"], ["B-LOC"], [0.5], [-0.25])
    assert one[0]["confidence"] == 1.0


@pytest.mark.parametrize("tags", [
    ["I-LOC", "I-LOC", "B-PER", "O", "B-ORG", "I-PER", "O", "B-LOC"],
    ["O"] * 8,
    ["B-LOC", "B-LOC", "I-LOC", "I-PER", "I-PER", "O", "I-ORG", "I-ORG"],
    ["B-PER", "I-PER", "I-PER", "I-PER", "I-PER", "I-PER", "I-PER", "I-PER"],
])
def test_decode_prediction_scored_surfaces_match_plain(tags):
    tokens = ["北", "京", "##大", "[UNK]", "的", "张", "三", "去"]
    zeros = [0.0] * len(tokens)
    scored = decode_prediction_scored(tokens, tags, zeros, zeros)
    plain = decode_prediction(tokens, tags)
    regrouped = {}
    for e in scored:
        regrouped.setdefault(e["type"], []).append(e["text"])
    assert regrouped == plain


# -------------------------------------------------------------------- models
@pytest.mark.parametrize("name", ["bilstm_crf", "bert_crf", "bert_ce",
                                  "bert_bilstm_crf_mtl"])
def test_models_compute_conf(name):
    torch.manual_seed(0)
    mtl = "mtl" in name
    params = make_tiny_params(name)
    model = build_model(name, params).eval()
    batch = make_tiny_batch(name, batch_size=3, seq_len=16, mtl=mtl)
    batch.pop("label_ids", None)
    with torch.no_grad():
        plain = model(batch, compute_pred=True)
        conf = model(batch, compute_conf=True)
        neither = model(batch)
    assert plain.span_scores is None and neither.span_scores is None
    assert neither.pred_ids is None
    assert torch.equal(conf.pred_ids, plain.pred_ids)
    a, b = conf.span_scores
    assert a.shape == (3, 16) and b.shape == (3, 16)
    assert a.dtype == torch.float64 and b.dtype == torch.float64
    mask = batch["mask"].bool()
    assert torch.count_nonzero(a[~mask]) == 0
    assert torch.count_nonzero(b[~mask]) == 0
    # token marginals of the decoded tags are probabilities
    tok = (a + b)[mask]
    assert (tok <= 1e-9).all() and torch.isfinite(tok).all()


def test_token_head_scores_are_token_probability_products():
    g = torch.Generator().manual_seed(6)
    logits = torch.randn(2, 7, 5, generator=g)
    mask = (torch.arange(7)[None, :] < torch.tensor([7, 4])[:, None]).long()
    pred = logits.argmax(-1) * mask
    a, b = ops.token_path_scores(logits, mask, pred)
    lp = torch.log_softmax(logits.double(), -1).gather(
        2, pred[:, :, None]).squeeze(2)
    for r, n in ((0, 7), (1, 4)):
        for s in range(n):
            for e in range(s, n):
                want = lp[r, s:e + 1].sum()
                assert abs((a[r, s] + b[r, e]) - want) < 1e-12
    assert torch.count_nonzero(a[mask == 0]) == 0
