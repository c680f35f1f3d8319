"""Prediction post-processing: strip special tokens, ids→tags, BIO→entity
decode (reference tools/predict_utils.py:6-60 and tools/infer_utils.py:76-118
behaviour, re-implemented)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

SPECIAL_TAGS = ("[PAD]", "[CLS]", "[SEP]")


def fix_tokens(tokens: Sequence[str]) -> List[str]:
    """Clean wordpiece artifacts for display: strip '##' continuation
    prefixes and map '[UNK]' to a placeholder char (reference
    tools/infer_utils.py:102-118)."""
    out = []
    for tok in tokens:
        if tok.startswith("##"):
            tok = tok[2:]
        if tok == "[UNK]":
            tok = "?"
        out.append(tok)
    return out


def process_prediction(row: Dict, idx2tag: Dict[int, str],
                       tokens: Optional[Sequence[str]] = None) -> Dict:
    """One predict-pkl row (pred_ids, label_ids, mask arrays) → real-token
    tag sequences with [CLS]/[SEP]/[PAD] stripped (reference
    tools/predict_utils.py:39-60)."""
    pred_ids = list(row["pred_ids"])
    label_ids = list(row["label_ids"])
    mask = list(row.get("mask", [1] * len(pred_ids)))
    pred_tags, label_tags, kept_tokens = [], [], []
    for i, (p, y, m) in enumerate(zip(pred_ids, label_ids, mask)):
        if not m:
            continue
        ytag = idx2tag.get(int(y), "O")
        if ytag in SPECIAL_TAGS:
            continue
        ptag = idx2tag.get(int(p), "O")
        pred_tags.append("O" if ptag in SPECIAL_TAGS else ptag)
        label_tags.append(ytag)
        if tokens is not None and i < len(tokens):
            kept_tokens.append(tokens[i])
    out = {"pred_tags": pred_tags, "label_tags": label_tags}
    if tokens is not None:
        out["tokens"] = fix_tokens(kept_tokens)
    return out


def _bio_groups(tags: Sequence[str]):
    """BIO grouping shared by the entity decoders: yields (type, start, end,
    error) per span, end inclusive. A B- opens a span, an I- continues the
    open one (or opens one when none is open), anything else closes it; an
    I- of another type stays in the span and sets its error flag."""
    cur_type, start, end, err = None, 0, 0, False
    for i, tag in enumerate(tags):
        if tag.startswith("B-"):
            if cur_type is not None:
                yield cur_type, start, end, err
            cur_type, start, end, err = tag[2:], i, i, False
        elif tag.startswith("I-"):
            if cur_type is None:
                cur_type, start, end, err = tag[2:], i, i, False
            else:
                if tag[2:] != cur_type:
                    err = True
                end = i
        else:
            if cur_type is not None:
                yield cur_type, start, end, err
            cur_type = None
    if cur_type is not None:
        yield cur_type, start, end, err


def _surface(toks: Sequence[str], start: int, end: int, err: bool) -> str:
    return "".join(toks[start:end + 1]) + ("[ERROR]" if err else "")


def decode_prediction(tokens: Sequence[str], tags: Sequence[str]) -> Dict[str, List[str]]:
    """BIO tag sequence + tokens → {entity_type: [surface, ...]}; a B/I
    type mismatch inside one span marks the surface with '[ERROR]'
    (reference tools/predict_utils.py:6-36)."""
    entities: Dict[str, List[str]] = {}
    toks = fix_tokens(tokens)
    n = min(len(toks), len(tags))
    for etype, start, end, err in _bio_groups(tags[:n]):
        entities.setdefault(etype, []).append(_surface(toks, start, end, err))
    return entities


def decode_prediction_scored(tokens: Sequence[str], tags: Sequence[str],
                             span_a: Sequence[float], span_b: Sequence[float],
                             offset: int = 0) -> List[Dict]:
    """decode_prediction's spans, in order of appearance, each with its
    confidence: [{"type", "text", "start", "end", "confidence"}] with
    start/end token indices into ``tokens`` (end inclusive) and

        confidence = exp(min(0, span_a[start+offset] + span_b[end+offset]))

    span_a/span_b are one row of the model's span_scores; ``offset`` is the
    shift between ``tokens`` and that row (1 when the row starts with
    [CLS]). The confidence is the posterior that tokens start..end carry
    exactly the decoded tags; it does not also require the entity to stop
    at ``end``, so it is an upper bound on the strict BIO entity's."""
    toks = fix_tokens(tokens)
    n = min(len(toks), len(tags))
    out = []
    for etype, start, end, err in _bio_groups(tags[:n]):
        logp = float(span_a[start + offset]) + float(span_b[end + offset])
        out.append({"type": etype, "text": _surface(toks, start, end, err),
                    "start": start, "end": end,
                    "confidence": math.exp(min(0.0, logp))})
    return out


def decode_prediction_nbest(tokens: Sequence[str],
                            tag_paths: Sequence[Sequence[str]],
                            logp: Sequence[float], offset: int = 0) -> Dict:
    """The n best taggings of one sentence as entity lists, and what they
    say together about each entity.

    ``tag_paths[r]`` is the tag sequence of rank r over one model row and
    ``logp[r]`` its log posterior (one row of the model's nbest paths, ids
    mapped to tags, and nbest_logp); ``offset`` is the shift between
    ``tokens`` and that row (1 when the row starts with [CLS]). Ranks the
    row does not have (logp = -inf) are skipped.

    Returns {"alternatives": [{"rank", "prob", "entities": [{"type", "text",
    "start", "end"}]}], "entities": [{"type", "text", "start", "end",
    "support"}]}: the alternatives in rank order with prob = exp(min(0,
    logp)), then every distinct well-formed entity in order of first
    appearance (rank, then position) with

        support = min(1, sum of prob over the alternatives that contain
                         exactly this (type, start, end) with no error flag)

    start/end index ``tokens``, end inclusive. The alternatives are
    distinct paths, so their probabilities add, and each one that holds the
    entity holds it as a strict BIO entity: support is a lower bound on the
    strict entity posterior (decode_prediction_scored's confidence is an
    upper bound). Spans with a B/I type mismatch ('[ERROR]' surface) are
    listed in their alternative but earn no support. Neither does a span
    that opens with I- where the entity's first (best-ranked) occurrence
    opens with B-, or the other way round: it is the same (type, start,
    end) but another tag sequence, which the confidence does not cover, so
    counting it could lift support above that upper bound."""
    toks = fix_tokens(tokens)
    alternatives, support, first, opening = [], {}, {}, {}
    for rank, (path, lp) in enumerate(zip(tag_paths, logp)):
        lp = float(lp)
        if lp == -math.inf or math.isnan(lp):
            continue
        tags = list(path)[offset:offset + len(toks)]
        prob = math.exp(min(0.0, lp))
        ents = []
        for etype, start, end, err in _bio_groups(tags):
            ent = {"type": etype, "text": _surface(toks, start, end, err),
                   "start": start, "end": end}
            ents.append(ent)
            if not err:
                key = (etype, start, end)
                first.setdefault(key, ent)
                if opening.setdefault(key, tags[start][:2]) == tags[start][:2]:
                    support[key] = support.get(key, 0.0) + prob
        alternatives.append({"rank": rank, "prob": prob, "entities": ents})
    entities = [dict(ent, support=min(1.0, support[key]))
                for key, ent in first.items()]
    return {"alternatives": alternatives, "entities": entities}


def extract_entity(tokens: Sequence[str], tags: Sequence[str]) -> Dict[str, set]:
    """Like decode_prediction but deduplicated per type (reference
    tools/infer_utils.py:76-99 returns {type: {surfaces}})."""
    ents = decode_prediction(tokens, tags)
    return {t: set(v) for t, v in ents.items()}


def bio_extract_entity(text: str, tags: Sequence[str]) -> List[str]:
    """Span surfaces from a BIO sequence over raw text characters
    (reference mrc/evaluation.py:8-24)."""
    spans, start = [], None
    for i, tag in enumerate(list(tags) + ["O"]):
        inside = i < len(text) and tag != "O"
        if tag.startswith("B-") or (inside and start is None):
            if start is not None:
                spans.append(text[start:i])
            start = i
        elif not inside and start is not None:
            spans.append(text[start:i])
            start = None
    return spans
