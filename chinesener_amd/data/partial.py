"""Partially annotated training data: tag sequences in which some positions
carry the unknown tag ``?`` instead of a gold tag.

A dataset whose ``DatasetSpec.unknown_tag`` is set has its features built
with one extra array, ``allowed_tags`` (int64 [L]): per position the set of
tags the annotation permits, one bit per tag id (``BasicProc
.build_seq_feature``). The CRF models train on it with the partial-annotation
loss (``ops.crf_partial_nll``): the likelihood of all paths that agree with
what was annotated, which leaves the unannotated positions to the model
instead of teaching it ``O`` there.

Helpers here produce such tag sequences: ``mask_annotations`` thins a full
annotation out (for experiments and the synthetic corpus), ``distant_tags``
tags a sentence from an entity dictionary (``augment.build_entity_dict``)
and leaves everything the dictionary did not match unknown.
"""
from __future__ import annotations

import random
from typing import Dict, List, Sequence

from ..eval.entity_eval import extract_spans
from .datasets import CLS_TAG, PAD_TAG, SEP_TAG
from .trie import Trie

UNKNOWN_TAG = "?"


def as_int64(bits: int) -> int:
    """A 64-bit pattern as the signed value an int64 array holds (bit 63 is
    the sign bit, so tag id 63 is ``-2**63``)."""
    bits &= (1 << 64) - 1
    return bits - (1 << 64) if bits >= 1 << 63 else bits


def open_bits(tag2idx: Dict[str, int]) -> int:
    """The allowed-tag word of an unknown position: every tag except [PAD],
    [CLS] and [SEP] (unsigned bit pattern)."""
    bits = 0
    for tag, idx in tag2idx.items():
        if tag not in (PAD_TAG, CLS_TAG, SEP_TAG):
            assert 0 <= idx < 64, "allowed-tag words hold at most 64 tags"
            bits |= 1 << idx
    return bits


def mask_annotations(tags: Sequence[Sequence[str]], entity_keep: float,
                     o_keep: float, seed: int = 1234) -> List[List[str]]:
    """Turn full annotations into partial ones. Every entity span is kept
    whole with probability `entity_keep` or replaced whole by ``?``; every
    position outside an entity keeps its tag with probability `o_keep`."""
    rng = random.Random(seed)
    out: List[List[str]] = []
    for sent in tags:
        sent = list(sent)
        new = [t if rng.random() < o_keep else UNKNOWN_TAG for t in sent]
        for _, start, end in extract_spans(sent):
            keep = rng.random() < entity_keep
            for i in range(start, end):
                new[i] = sent[i] if keep else UNKNOWN_TAG
        out.append(new)
    return out


def distant_tags(sentence: str, entity_dict: Dict[str, List[str]]) -> List[str]:
    """Distant supervision from an entity dictionary {type: [surface, ...]}:
    forward maximum matching over a trie of the surfaces, ``B-``/``I-`` on
    the matches and ``?`` everywhere else (a dictionary miss says nothing
    about a position). A surface listed under several types takes the first
    type in dictionary order."""
    surface2type: Dict[str, str] = {}
    for typ, surfaces in entity_dict.items():
        for s in surfaces:
            if s:
                surface2type.setdefault(s, typ)
    trie = Trie(surface2type)
    longest = max((len(s) for s in surface2type), default=1)
    out = [UNKNOWN_TAG] * len(sentence)
    i = 0
    while i < len(sentence):
        words = trie.prefixes(sentence, i, longest)
        if not words:
            i += 1
            continue
        typ = surface2type[words[-1]]
        end = i + len(words[-1])
        out[i] = f"B-{typ}"
        for j in range(i + 1, end):
            out[j] = f"I-{typ}"
        i = end
    return out


def complete_annotations(model, features):
    """Pseudo-labels for self-training on a partially annotated dataset:
    decode `features` (a batch that carries ``allowed_tags``) under its own
    annotation, so every annotated position keeps its tag and the model
    fills in the rest. Returns ``(pred_ids long [B,L], path_score f32 [B])``;
    a row whose annotation admits no path under the model's transition
    constraints has score -inf and a zero row. Needs a single-task CRF
    model."""
    import torch

    if "allowed_tags" not in features:
        raise KeyError("complete_annotations: the batch has no 'allowed_tags'")
    feats = {k: v for k, v in features.items()
             if k not in ("label_ids", "allowed_tags")}
    feats["constraint_tags"] = features["allowed_tags"]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model(feats, constrained=True)
    finally:
        model.train(was_training)
    return out.pred_ids, out.path_score
