"""Partial-annotation CRF on the CPU: the reference against brute-force path
enumeration, the allowed-word helpers, the feature builder and the model
wiring."""
import itertools

import numpy as np
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.data import partial
from chinesener_amd.data.datasets import get_spec, load_data
from chinesener_amd.data.loader import _to_tensors
from chinesener_amd.data.preprocess import get_instance
from chinesener_amd.ops import reference as ref

from conftest import make_tiny_batch, make_tiny_params


def _case(T, L, seed):
    """B = 3 rows of length 1, 2 and L with random allowed words (stray bits
    >= T and all-zero words included)."""
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(3, L, T, dtype=torch.float64, generator=g)
    trans = torch.randn(T, T, dtype=torch.float64, generator=g)
    lens = torch.tensor([1, 2, L])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    allowed = torch.randint(0, 1 << (T + 2), (3, L), generator=g)
    return em, trans, lens, mask, allowed


def _brute_force(em, trans, lens, allowed):
    """(ll [B], d ll / d em [B,L,T], d ll / d trans [B,T,T]) by enumerating
    every path: marginals under the constrained minus under the free
    distribution."""
    B, L, T = em.shape
    ll = torch.zeros(B, dtype=torch.float64)
    d_em = torch.zeros_like(em)
    d_tr = torch.zeros(B, T, T, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        sets = []
        for t in range(n):
            s = [j for j in range(T) if (int(allowed[b, t]) >> j) & 1]
            sets.append(s or list(range(T)))
        paths = list(itertools.product(range(T), repeat=n))
        score = torch.stack([
            sum(em[b, t, y[t]] for t in range(n))
            + sum(trans[y[t - 1], y[t]] for t in range(1, n)) for y in paths])
        inside = torch.tensor([all(y[t] in sets[t] for t in range(n))
                               for y in paths])
        p_free = torch.softmax(score, 0)
        p_con = torch.softmax(score.masked_fill(~inside, -float("inf")), 0)
        ll[b] = (torch.logsumexp(score[inside], 0) - torch.logsumexp(score, 0))
        for y, pf, pc in zip(paths, p_free, p_con):
            for t in range(n):
                d_em[b, t, y[t]] += pc - pf
                if t > 0:
                    d_tr[b, y[t - 1], y[t]] += pc - pf
    return ll, d_em, d_tr


@pytest.mark.parametrize("T,L", [(3, 5), (4, 4), (3, 1), (4, 2)])
def test_reference_matches_path_enumeration(T, L):
    em, trans, lens, mask, allowed = _case(T, L, seed=10 * T + L)
    lens = lens.clamp(max=L)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    em.requires_grad_()
    trans.requires_grad_()
    ll = ref.crf_partial_log_likelihood(em, allowed, mask, trans,
                                        dtype=torch.float64)
    ll_bf, d_em_bf, d_tr_bf = _brute_force(em.detach(), trans.detach(), lens,
                                           allowed)
    torch.testing.assert_close(ll.detach(), ll_bf, atol=1e-12, rtol=1e-12)
    assert (ll <= 1e-12).all()
    # per-row weights separate the rows' transition gradients
    for b in range(3):
        d_em, d_tr = torch.autograd.grad(ll[b], (em, trans), retain_graph=True,
                                         allow_unused=True)
        if d_tr is None:                # L = 1: no transition is scored
            d_tr = torch.zeros_like(trans)
        torch.testing.assert_close(d_em[b], d_em_bf[b], atol=1e-12, rtol=1e-10)
        torch.testing.assert_close(d_tr, d_tr_bf[b], atol=1e-12, rtol=1e-10)
        assert torch.count_nonzero(d_em[b, int(lens[b]):]) == 0


def test_singletons_match_crf_log_likelihood():
    g = torch.Generator().manual_seed(3)
    B, L, T = 4, 7, 6
    em = torch.randn(B, L, T, generator=g)
    trans = torch.randn(T, T, generator=g)
    lens = torch.tensor([1, 2, 7, 4])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    tags = torch.randint(0, T, (B, L), generator=g)
    allowed = ops.allowed_from_tags(tags, torch.ones(B, L, dtype=torch.bool), 0)
    ll = ops.crf_partial_nll(em, allowed, mask, trans)
    gold = ref.crf_log_likelihood(em, tags, mask, trans)
    torch.testing.assert_close(ll, gold, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("word", ["open", "zero", "stray"])
def test_open_rows_are_zero(word):
    B, L, T = 3, 6, 5
    g = torch.Generator().manual_seed(4)
    em = torch.randn(B, L, T, generator=g, requires_grad=True)
    trans = torch.randn(T, T, generator=g, requires_grad=True)
    mask = (torch.arange(L)[None, :] < torch.tensor([6, 1, 3])[:, None]).long()
    value = {"open": (1 << T) - 1, "zero": 0, "stray": -1 << T}[word]
    allowed = torch.full((B, L), value, dtype=torch.int64)
    ll = ops.crf_partial_nll(em, allowed, mask, trans)
    assert torch.count_nonzero(ll) == 0
    d_em, d_tr = torch.autograd.grad(ll.sum(), (em, trans))
    assert torch.count_nonzero(d_em) == 0 and torch.count_nonzero(d_tr) == 0


def test_empty_row_is_zero():
    g = torch.Generator().manual_seed(5)
    em = torch.randn(2, 4, 3, generator=g, requires_grad=True)
    trans = torch.randn(3, 3, generator=g, requires_grad=True)
    mask = torch.tensor([[0, 0, 0, 0], [1, 1, 1, 0]])
    allowed = torch.tensor([[1, 2, 4, 1], [1, 2, 4, 1]])
    ll = ref.crf_partial_log_likelihood(em, allowed, mask, trans)
    assert ll[0] == 0 and ll[1] < 0
    d_em, = torch.autograd.grad(ll.sum(), em)
    assert torch.count_nonzero(d_em[0]) == 0


def test_allowed_from_tags_sets_bit_63():
    tags = torch.tensor([[63, 0, 62, 5]])
    known = torch.tensor([[True, True, True, False]])
    words = ops.allowed_from_tags(tags, known, (1 << 64) - 1)
    assert words.dtype == torch.int64
    assert words.tolist() == [[-2 ** 63, 1, 1 << 62, -1]]
    # the reference reads bit 63 back as tag 63, and only that
    sets = ref.allowed_sets(words, 64)
    assert sets[0, 0].nonzero().flatten().tolist() == [63]
    assert sets[0, 3].all()
    assert ops.allowed_from_tags(tags, known, -2 ** 63)[0, 3] == -2 ** 63
    # a T = 64 row of tag-63 singletons is the gold-path likelihood
    g = torch.Generator().manual_seed(6)
    em = torch.randn(1, 3, 64, generator=g)
    trans = torch.randn(64, 64, generator=g)
    t63 = torch.full((1, 3), 63)
    mask = torch.ones(1, 3, dtype=torch.long)
    ll = ops.crf_partial_nll(
        em, ops.allowed_from_tags(t63, torch.ones(1, 3, dtype=torch.bool), 0),
        mask, trans)
    torch.testing.assert_close(ll, ref.crf_log_likelihood(em, t63, mask, trans),
                               atol=1e-5, rtol=1e-5)


def test_open_bits_and_mask_annotations():
    spec = get_spec("msra_partial")
    assert partial.open_bits(spec.tag2idx) == 0b0011111110
    assert partial.as_int64(1 << 63) == -2 ** 63
    tags = [["O", "B-PER", "I-PER", "O", "B-LOC", "I-LOC", "I-LOC", "O"]] * 50
    out = partial.mask_annotations(tags, entity_keep=0.5, o_keep=0.3, seed=1)
    kept = dropped = 0
    for src, new in zip(tags, out):
        assert len(new) == len(src)
        for lo, hi in ((1, 3), (4, 7)):       # an entity stays or goes whole
            span = new[lo:hi]
            assert span == src[lo:hi] or span == ["?"] * (hi - lo)
            kept += span == src[lo:hi]
            dropped += span != src[lo:hi]
        assert all(n in (s, "?") for s, n in zip(src, new))
    assert kept > 0 and dropped > 0
    assert partial.mask_annotations(tags, 1.0, 1.0) == [list(t) for t in tags]


def test_distant_tags():
    ents = {"PER": ["张三", "张三丰"], "LOC": ["北京"]}
    assert partial.distant_tags("张三丰去北京了", ents) == [
        "B-PER", "I-PER", "I-PER", "?", "B-LOC", "I-LOC", "?"]
    assert partial.distant_tags("无", {}) == ["?"]


@pytest.mark.parametrize("tok", ["char", "bert"])
def test_build_seq_feature_words(tok):
    spec = get_spec("msra_partial")
    t2i = spec.tag2idx
    proc = get_instance(tok, 8, t2i, unknown_tag=spec.unknown_tag)
    feat = proc.build_seq_feature("甲乙丙丁", ["B-PER", "?", "O", "?"])
    words = feat["allowed_tags"]
    assert words.dtype == np.int64 and words.shape == (8,)
    free = partial.open_bits(t2i)
    body = [1 << t2i["B-PER"], free, 1 << t2i["O"], free]
    if tok == "bert":
        want = [1 << t2i["[CLS]"]] + body + [1 << t2i["[SEP]"]]
    else:
        want = body
    want = want + [1 << t2i["[PAD]"]] * (8 - len(want))
    assert words.tolist() == want
    # label_ids: O as a placeholder at '?'
    off = 1 if tok == "bert" else 0
    assert feat["label_ids"][off:off + 4].tolist() == [
        t2i["B-PER"], t2i["O"], t2i["O"], t2i["O"]]
    # every sample of the dataset has the key, fully labelled ones too
    full = proc.build_seq_feature("甲乙", ["O", "B-LOC"])
    assert "allowed_tags" in full
    assert np.count_nonzero(full["allowed_tags"] == free) == 0
    batch = _to_tensors(proc.stack([feat, full]), np.arange(2))
    assert batch["allowed_tags"].dtype == torch.int64


def test_dataset_without_unknown_tag_has_no_new_key():
    spec = get_spec("msra")
    assert spec.unknown_tag is None
    proc = get_instance("char", 8, spec.tag2idx, unknown_tag=spec.unknown_tag)
    feat = proc.build_seq_feature("甲乙", ["O", "B-LOC"])
    assert sorted(feat) == ["label_ids", "mask", "seq_len", "token_ids"]
    # and '?' is still a sentence to drop there
    with pytest.raises(KeyError):
        proc.build_seq_feature("甲乙", ["O", "?"])


def test_partial_datasets_registered():
    for name, base in (("msra_partial", "msra"),
                       ("cluener_fine_partial", "cluener_fine")):
        spec = get_spec(name)
        assert spec.unknown_tag == partial.UNKNOWN_TAG
        assert spec.tag2idx == get_spec(base).tag2idx
        sents, tags = load_data(name, f"no-such-dir/{name}", "train")
        flat = [t for row in tags[:50] for t in row]
        assert "?" in flat and set(flat) - {"?"} <= set(spec.tag2idx)
        v_sents, v_tags = load_data(name, f"no-such-dir/{name}", "valid")
        assert (v_sents, v_tags) == load_data(base, f"no-such-dir/{base}",
                                              "valid")
        assert all(t != "?" for row in v_tags for t in row)
    assert get_spec("cluener_fine_partial").label_size == 24


def _partial_batch(batch):
    """make_tiny_batch plus allowed_tags: about half the positions open."""
    g = torch.Generator().manual_seed(1)
    known = torch.rand(batch["label_ids"].shape, generator=g) < 0.5
    known |= batch["mask"] == 0
    batch = dict(batch)
    batch["allowed_tags"] = ops.allowed_from_tags(batch["label_ids"], known,
                                                  0b0011111110)
    return batch


def test_bilstm_crf_loss_is_the_partial_loss():
    torch.manual_seed(0)
    from chinesener_amd.models import build_model
    model = build_model("bilstm_crf", make_tiny_params("bilstm_crf")).eval()
    full = make_tiny_batch("bilstm_crf")
    batch = _partial_batch(full)
    out = model(batch)
    want = -ref.crf_partial_log_likelihood(
        out.logits, batch["allowed_tags"], batch["mask"],
        model.crf.transitions).sum() / batch["token_ids"].shape[0]
    torch.testing.assert_close(out.loss, want, atol=1e-5, rtol=1e-5)
    assert out.loss < model(full).loss      # fewer constraints, smaller loss
    out.loss.backward()
    assert model.crf.transitions.grad.abs().sum() > 0

    # all singletons: the label_ids loss
    single = dict(full)
    single["allowed_tags"] = ops.allowed_from_tags(
        full["label_ids"], torch.ones_like(full["label_ids"], dtype=torch.bool),
        0)
    torch.testing.assert_close(model(single).loss, model(full).loss,
                               atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["bert_bilstm_crf_mtl", "bert_ce"])
def test_other_heads_reject_partial_labels(name):
    torch.manual_seed(0)
    from chinesener_amd.models import build_model
    model = build_model(name, make_tiny_params(name)).eval()
    batch = make_tiny_batch(name, mtl=name.endswith("mtl"))
    assert torch.isfinite(model(batch).loss)
    with pytest.raises(ValueError, match="allowed_tags"):
        model(_partial_batch(batch))
