"""Builders for constrained decoding (``ops.crf_viterbi_constrained``,
``forward(..., constrained=True)``): the allowed-transition words of a
tagset and the per-position allowed-tag words of what a caller knows about a
sentence. All words are int64 bit patterns, bit j = tag id j, in the
encoding of the partial-annotation loss (``data/partial.py``).

    words = span_words([("ORG", 0, 4)], len(sentence), tag2idx, offset=1)
    words = forbid_types(words, ["PER"], tag2idx)
    crf.constrain_transitions(bio_transition_words(tag2idx))
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

from .partial import as_int64, open_bits

ALL_BITS = (1 << 64) - 1


def bio_transition_words(tag2idx: Dict[str, int]) -> np.ndarray:
    """int64 [T]: word i holds the tags that may follow tag i under BIO.
    ``X -> I-Y`` is allowed only for X in {B-Y, I-Y}; everything else is
    allowed. A tagset without ``B-``/``I-`` tags (the ``bies`` CWS set) gives
    all-ones words. T = max id + 1."""
    size = max(tag2idx.values()) + 1
    assert size <= 64, "allowed-transition words hold at most 64 tags"
    inside = {tag[2:]: idx for tag, idx in tag2idx.items()
              if tag.startswith("I-")}
    all_i = 0
    for idx in inside.values():
        all_i |= 1 << idx
    words = [ALL_BITS & ~all_i] * size
    for tag, idx in tag2idx.items():
        if tag[:2] in ("B-", "I-") and tag[2:] in inside:
            words[idx] |= 1 << inside[tag[2:]]
    return np.array([as_int64(w) for w in words], dtype=np.int64)


def span_words(spans: Iterable[Tuple[str, int, int]], length: int,
               tag2idx: Dict[str, int], offset: int = 0) -> np.ndarray:
    """int64 [length] allowed-tag words from entity hints ``(type, start,
    end)``, end exclusive, in token positions; `offset` is added to both
    (1 for a leading [CLS]). ``B-type`` is the only tag at the start,
    ``I-type`` the only one on the rest of the span. The position after a
    span, unless it is hinted itself or past the end, gets every open tag
    but ``I-type``, so the entity ends where the hint says. All other
    positions are 0: nothing known. Overlapping spans, unknown types and
    spans outside ``[0, length)`` raise ValueError."""
    hinted = np.zeros(length, dtype=bool)
    bits = [0] * length
    ends = []
    for typ, start, end in spans:
        b, i = tag2idx.get(f"B-{typ}"), tag2idx.get(f"I-{typ}")
        if b is None or (i is None and end - start > 1):
            raise ValueError(f"span_words: unknown entity type {typ!r}")
        s, e = start + offset, end + offset
        if not 0 <= s < e <= length:
            raise ValueError(
                f"span_words: span {(typ, start, end)} outside the sentence "
                f"(length {length}, offset {offset})")
        if hinted[s:e].any():
            raise ValueError(
                f"span_words: span {(typ, start, end)} overlaps another")
        hinted[s:e] = True
        bits[s] = 1 << b
        for t in range(s + 1, e):
            bits[t] = 1 << i
        if i is not None:
            ends.append((e, i))
    rest = open_bits(tag2idx)
    for e, i in ends:
        if e < length and not hinted[e]:
            bits[e] = rest & ~(1 << i)
    return np.array([as_int64(w) for w in bits], dtype=np.int64)


def forbid_types(words: Sequence[int], types: Iterable[str],
                 tag2idx: Dict[str, int]) -> np.ndarray:
    """Every position of `words` that is still open (0) becomes every open
    tag minus the ``B-``/``I-`` tags of `types`; hinted positions stay.
    Unknown types raise ValueError."""
    drop = 0
    for typ in types:
        ids = [tag2idx[t] for t in (f"B-{typ}", f"I-{typ}") if t in tag2idx]
        if not ids:
            raise ValueError(f"forbid_types: unknown entity type {typ!r}")
        for idx in ids:
            drop |= 1 << idx
    out = np.array(words, dtype=np.int64, copy=True)
    out[out == 0] = as_int64(open_bits(tag2idx) & ~drop)
    return out
