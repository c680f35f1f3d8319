"""N-best CRF decoding on CPU: ops.reference.crf_nbest against full
enumeration (order and tie rule included), its row handling, the op, and
eval.decode_prediction_nbest with the support <= strict <= confidence
sandwich around the strict BIO entity posterior."""
import itertools
import math

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.eval import (decode_prediction_nbest,
                                 decode_prediction_scored)
from chinesener_amd.eval.predict_utils import _bio_groups
from chinesener_amd.ops import reference as ref

NINF = float("-inf")


def _rand(B, L, T, seed, lens=None, quarter=False):
    g = torch.Generator().manual_seed(seed)
    if quarter:  # multiples of 0.25 in [-1, 1]: every sum is exact
        em = torch.randint(-4, 5, (B, L, T), generator=g).double() / 4
        trans = torch.randint(-4, 5, (T, T), generator=g).double() / 4
    else:
        em = torch.randn(B, L, T, generator=g, dtype=torch.float64)
        trans = torch.randn(T, T, generator=g, dtype=torch.float64)
    lens = torch.tensor(lens if lens is not None else [L] * B)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return em, trans, mask, lens


def _score(em, trans, y):
    """The path score in the reference's association order."""
    sc = em[0, y[0]]
    for t in range(1, len(y)):
        sc = (sc + trans[y[t - 1], y[t]]) + em[t, y[t]]
    return sc.item()


def _enumerate(em, trans, n):
    """[(score, path)] of every tag path of one row of length n, ranked by
    score descending and, among equal scores, in the order the stated rule
    gives: the list Viterbi's ties resolve to the lexicographically smallest
    REVERSED path (last tag first, then the one before, ...), because each
    step prefers the lower predecessor and the final step the lower tag."""
    T = em.shape[1]
    rows = [(_score(em, trans, y), y)
            for y in itertools.product(range(T), repeat=n)]
    rows.sort(key=lambda r: (-r[0], r[1][::-1]))
    return rows


def _check_row(paths, scores, em, trans, n, k, exact_order):
    """One row of a crf_nbest result against enumeration."""
    L = em.shape[0]
    if n <= 0:
        assert (scores == NINF).all() and torch.count_nonzero(paths) == 0
        return
    rows = _enumerate(em, trans, n)
    have = min(k, len(rows))
    assert (scores[have:] == NINF).all()
    assert torch.count_nonzero(paths[have:]) == 0
    assert torch.count_nonzero(paths[:, n:]) == 0
    for r in range(have):
        assert scores[r].item() == pytest.approx(rows[r][0], abs=1e-12)
        got = tuple(paths[r, :n].tolist())
        if exact_order:
            assert got == rows[r][1], (r, got, rows[r])
        else:
            assert _score(em, trans, got) == pytest.approx(rows[r][0],
                                                           abs=1e-12)


def test_reference_matches_enumeration():
    em, trans, mask, _ = _rand(1, 5, 3, seed=35)
    paths, scores = ref.crf_nbest(em, mask, trans, 8)
    assert paths.shape == (1, 8, 5) and paths.dtype == torch.long
    assert scores.shape == (1, 8) and scores.dtype == torch.float64
    _check_row(paths[0], scores[0], em[0], trans, 5, 8, exact_order=True)


def test_reference_fewer_paths_than_k():
    em, trans, mask, _ = _rand(1, 2, 2, seed=22)
    paths, scores = ref.crf_nbest(em, mask, trans, 8)
    assert torch.isfinite(scores[0, :4]).all()
    assert (scores[0, 4:] == NINF).all()
    _check_row(paths[0], scores[0], em[0], trans, 2, 8, exact_order=True)


def test_reference_ragged_batch_with_empty_row():
    L, T, k = 5, 3, 8
    lens = [5, 0, 1, 3, 2]
    em, trans, mask, _ = _rand(len(lens), L, T, seed=7, lens=lens)
    paths, scores = ref.crf_nbest(em, mask, trans, k)
    for b, n in enumerate(lens):
        _check_row(paths[b], scores[b], em[b], trans, n, k, exact_order=True)
    # each row equals the same row decoded alone at its own length
    for b, n in enumerate(lens):
        if n:
            p1, s1 = ref.crf_nbest(em[b:b + 1, :n], mask[b:b + 1, :n], trans, k)
            assert torch.equal(paths[b, :, :n], p1[0])
            assert torch.equal(scores[b], s1[0])


@pytest.mark.parametrize("T,L,k,seed", [(3, 5, 8, 1), (3, 5, 4, 2),
                                        (4, 4, 8, 3), (2, 6, 8, 4)])
def test_reference_tie_rule(T, L, k, seed):
    """Exact sums tie often; the result must be the enumeration sorted by
    the stated order."""
    lens = [L, L - 1, 2]
    em, trans, mask, _ = _rand(3, L, T, seed=seed, lens=lens, quarter=True)
    paths, scores = ref.crf_nbest(em, mask, trans, k)
    tied = 0
    for b, n in enumerate(lens):
        _check_row(paths[b], scores[b], em[b], trans, n, k, exact_order=True)
        fin = scores[b][torch.isfinite(scores[b])]
        tied += int((fin[1:] == fin[:-1]).sum())
    assert tied > 0
    # and fp32 gives the same answer: the sums are exact there too
    p32, s32 = ref.crf_nbest(em.float(), mask, trans.float(), k)
    assert s32.dtype == torch.float32
    assert torch.equal(p32, paths) and torch.equal(s32.double(), scores)


def test_reference_k1_is_crf_decode():
    B, L, T = 6, 17, 9
    em, trans, mask, _ = _rand(B, L, T, seed=8, lens=[17, 1, 9, 2, 16, 5])
    em, trans = em.float(), trans.float()
    paths, scores = ref.crf_nbest(em, mask, trans, 1)
    assert torch.equal(paths[:, 0], ref.crf_decode(em, mask, trans))
    # a longer list keeps the shorter one as its prefix
    p4, s4 = ref.crf_nbest(em, mask, trans, 4)
    assert torch.equal(p4[:, :1], paths) and torch.equal(s4[:, :1], scores)
    with pytest.raises(ValueError):
        ref.crf_nbest(em, mask, trans, 0)


def test_op_on_cpu():
    B, L, T, k = 3, 6, 4, 5
    lens = [6, 0, 1]
    em, trans, mask, _ = _rand(B, L, T, seed=9, lens=lens)
    em32 = em.float().requires_grad_()
    tr32 = trans.float().requires_grad_()
    paths, scores, logp = ops.crf_nbest(em32, mask, tr32, k)
    assert paths.shape == (B, k, L) and paths.dtype == torch.long
    assert scores.dtype == torch.float32 and logp.dtype == torch.float64
    assert not scores.requires_grad and not logp.requires_grad
    rp, rs = ref.crf_nbest(em32.detach(), mask, tr32.detach(), k)
    assert torch.equal(paths, rp) and torch.equal(scores, rs)
    # logp = score - logZ on present ranks, -inf on absent ones
    assert (logp[1] == NINF).all() and (logp[2, T:] == NINF).all()
    rows = _enumerate(em32.detach().double()[0], tr32.detach().double(), 6)
    log_z = torch.logsumexp(
        torch.tensor([r[0] for r in rows], dtype=torch.float64), 0).item()
    for r in range(k):
        assert logp[0, r].item() == pytest.approx(rows[r][0] - log_z, abs=1e-9)
    # a row of length 1 with T tags: its T paths carry the whole mass
    assert torch.exp(logp[2, :T]).sum().item() == pytest.approx(1.0, abs=1e-9)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            ops.crf_nbest(em32, mask, tr32, bad)


def test_token_nbest_logp_is_the_score():
    g = torch.Generator().manual_seed(10)
    logits = torch.randn(2, 7, 5, generator=g)
    mask = (torch.arange(7)[None, :] < torch.tensor([7, 4])[:, None]).long()
    paths, scores, logp = ops.token_nbest(logits, mask, 4)
    assert torch.equal(paths[:, 0], logits.argmax(-1) * mask)
    torch.testing.assert_close(logp, scores.double(), atol=1e-5, rtol=0)
    assert (scores[:, 1:] <= scores[:, :-1]).all()


# ---------------------------------------------------------- entity decoding
def test_decode_prediction_nbest_hand_cases():
    tokens = list("甲乙丙丁戊")
    paths = [
        ["B-LOC", "I-LOC", "O", "B-PER", "O"],
        ["B-LOC", "I-LOC", "O", "O", "O"],
        ["[PAD]"] * 5,                                  # absent rank
        ["B-LOC", "I-PER", "O", "B-PER", "I-PER"],      # [ERROR] span
        ["O", "B-LOC", "O", "B-PER", "O"],
    ]
    logp = [math.log(0.4), math.log(0.25), NINF, math.log(0.125),
            math.log(0.0625)]
    out = decode_prediction_nbest(tokens, paths, logp)
    alts = out["alternatives"]
    assert [a["rank"] for a in alts] == [0, 1, 3, 4]      # absent one skipped
    assert [a["prob"] for a in alts] == pytest.approx([0.4, 0.25, 0.125,
                                                       0.0625])
    assert alts[0]["entities"] == [
        {"type": "LOC", "text": "甲乙", "start": 0, "end": 1},
        {"type": "PER", "text": "丁", "start": 3, "end": 3}]
    assert alts[2]["entities"][0]["text"] == "甲乙[ERROR]"
    ents = out["entities"]
    assert [(e["type"], e["start"], e["end"]) for e in ents] == [
        ("LOC", 0, 1), ("PER", 3, 3), ("PER", 3, 4), ("LOC", 1, 1)]
    sup = {(e["type"], e["start"], e["end"]): e["support"] for e in ents}
    assert sup[("LOC", 0, 1)] == pytest.approx(0.65)   # not the [ERROR] one
    assert sup[("PER", 3, 3)] == pytest.approx(0.4625)
    assert sup[("PER", 3, 4)] == pytest.approx(0.125)
    assert sup[("LOC", 1, 1)] == pytest.approx(0.0625)
    for e in ents:
        assert set(e) == {"type", "text", "start", "end", "support"}
    # [CLS] offset, and a rounding overshoot capped at 1
    shifted = decode_prediction_nbest(
        tokens, [["[CLS]"] + p + ["[SEP]"] for p in paths], logp, offset=1)
    assert shifted == out
    one = decode_prediction_nbest(["甲"], [["B-LOC"], ["B-LOC"]], [0.0, -0.1])
    assert one["entities"][0]["support"] == 1.0
    # the same span opened with I- is another tag sequence: not counted
    two = decode_prediction_nbest(
        list("甲乙"), [["B-LOC", "I-LOC"], ["I-LOC", "I-LOC"]],
        [math.log(0.5), math.log(0.25)])
    assert [e["support"] for e in two["entities"]] == pytest.approx([0.5])
    assert len(two["alternatives"]) == 2
    assert decode_prediction_nbest(tokens, paths[2:3], [NINF]) == {
        "alternatives": [], "entities": []}


def test_support_strict_confidence_sandwich():
    """support (n-best mass, k=8) <= strict BIO entity posterior (by
    enumerating all 5**6 paths) <= confidence (path posterior), for every
    entity of the best path. Strict: the path carries the decoded tags on
    start..end and BIO grouping delimits exactly that entity there.

    Each inequality has 1e-9 of slack for fp64 rounding: where the entity
    cannot be extended (it ends the row) strict and confidence are the same
    number computed two ways, and they differ in the last bits."""
    idx2tag = {0: "O", 1: "B-PER", 2: "I-PER", 3: "B-LOC", 4: "I-LOC"}
    T, L, k = 5, 6, 8
    tokens = list("甲乙丙丁戊己")
    checked = 0
    for seed in (11, 12, 13):
        em, trans, mask, _ = _rand(1, L, T, seed=seed)
        em = em * 2
        paths, scores, logp = ops.crf_nbest(em.float(), mask, trans.float(), k)
        pred, span_a, span_b = ops.crf_decode_scored(em.float(), mask,
                                                     trans.float())
        assert torch.equal(paths[0, 0], pred[0])
        tag_paths = [[idx2tag[i] for i in p.tolist()] for p in paths[0]]
        nb = decode_prediction_nbest(tokens, tag_paths, logp[0].tolist())
        scored = decode_prediction_scored(tokens, tag_paths[0],
                                          span_a[0].tolist(),
                                          span_b[0].tolist())
        # strict posterior of every well-formed entity, by enumeration
        em32, tr32 = em.float().double()[0], trans.float().double()
        mass = {}
        best = paths[0, 0].tolist()
        all_scores = torch.tensor(
            [_score(em32, tr32, y)
             for y in itertools.product(range(T), repeat=L)],
            dtype=torch.float64)
        log_z = torch.logsumexp(all_scores, 0).item()
        for y, sc in zip(itertools.product(range(T), repeat=L),
                         all_scores.tolist()):
            p = math.exp(sc - log_z)
            for etype, s, e, err in _bio_groups([idx2tag[i] for i in y]):
                if not err and list(y[s:e + 1]) == best[s:e + 1]:
                    mass[(etype, s, e)] = mass.get((etype, s, e), 0.0) + p
        support = {(e["type"], e["start"], e["end"]): e["support"]
                   for e in nb["entities"]}
        for ent in scored:
            if ent["text"].endswith("[ERROR]"):
                continue
            key = (ent["type"], ent["start"], ent["end"])
            strict = mass[key]
            assert support[key] <= strict + 1e-9
            assert strict <= ent["confidence"] + 1e-9
            assert support[key] > 0.0
            checked += 1
    assert checked > 0


def test_token_nbest_is_position_wise():
    """Any mask, not only a prefix: the result is that of the selected
    positions decoded on their own, put back where they were."""
    g = torch.Generator().manual_seed(14)
    B, L, T, k = 3, 9, 4, 5
    logits = torch.randn(B, L, T, generator=g)
    mask = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 0, 0],
                         [1, 0, 1, 0, 1, 1, 0, 0, 1],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0]])
    paths, scores, logp = ops.token_nbest(logits, mask, k)
    assert torch.count_nonzero(paths[(mask == 0)[:, None, :].expand_as(paths)]) == 0
    assert (scores[2] == NINF).all() and (logp[2] == NINF).all()
    for b in range(2):
        sel = mask[b].bool()
        n = int(sel.sum())
        alone = ops.token_nbest(logits[b:b + 1, sel],
                                torch.ones(1, n, dtype=torch.long), k)
        assert torch.equal(paths[b][:, sel], alone[0][0])
        assert torch.equal(scores[b], alone[1][0])
        assert torch.equal(logp[b], alone[2][0])
    assert torch.equal(paths[:, 0], logits.argmax(-1) * mask)
    # a prefix mask goes through unchanged
    pm = (torch.arange(L)[None, :] < torch.tensor([9, 4, 1])[:, None]).long()
    lp = torch.log_softmax(logits, -1)
    direct = ops.crf_nbest(lp, pm, torch.zeros(T, T), k)
    for got, want in zip(ops.token_nbest(logits, pm, k), direct):
        assert torch.equal(got, want)
