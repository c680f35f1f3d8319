#!/usr/bin/env python3
"""Interactive gRPC inference client — reference inference.py parity:

  python chinesener_amd/serve/server.py --model bert_bilstm_crf   # terminal 1
  python inference.py --model bert_bilstm_crf                     # terminal 2
  输入: 北京大学的张三去了上海 → {'LOC': {'上海'}, 'ORG': {'北京大学'}, 'PER': {'张三'}}

InferHelper builds features online with the SAME L1 proc used at
training preprocess time (reference inference.py:33-99,
base_preprocess.py:176-187: fake labels, task_ids=1 for mtl), sends a
Predict RPC with retry/backoff, and decodes pred_ids → entities."""
from __future__ import annotations

import argparse
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chinesener_amd.data.constraints import forbid_types, span_words
from chinesener_amd.data.datasets import get_spec
from chinesener_amd.data.preprocess import extract_prefix_surfix, get_instance
from chinesener_amd.eval import (decode_prediction_nbest,
                                 decode_prediction_scored, extract_entity)
from chinesener_amd.serve.client import PredictionClient, timer
from chinesener_amd.serve import rpc


class InferHelper:
    def __init__(self, model_name: str, data: str = "msra",
                 host: str = "127.0.0.1", port: int = rpc.DEFAULT_PORT,
                 max_seq_len: int | None = None, version: int | None = None):
        self.model_name = model_name
        spec = get_spec(data)
        self.max_seq_len = max_seq_len or spec.max_seq_len
        self.idx2tag = spec.idx2tag
        self.tag2idx = spec.tag2idx
        enhance, tok_type = extract_prefix_surfix(model_name)
        self.proc = get_instance(tok_type, self.max_seq_len, spec.tag2idx,
                                 enhance)
        self.is_mtl = "mtl" in model_name or "adv" in model_name
        self.client = PredictionClient(host, port)
        self.version = version

    def make_feature(self, sentence: str) -> dict:
        feat = self.proc.build_seq_feature(sentence)  # fake 'O' labels inside
        feats = {k: v[None, ...] for k, v in feat.items()}
        if self.is_mtl:
            # NER task is id 1 in the mtl pair (reference inference.py:70-71)
            feats["task_ids"] = np.ones_like(feats["token_ids"])
        return feats

    @timer
    def infer(self, sentence: str):
        feats = self.make_feature(sentence)
        resp = self.client.predict(self.model_name, feats, self.version)
        pred_ids = resp["outputs"]["pred_ids"][0]
        tokens = self.proc.tokenizer.tokenize(sentence)
        offset = 1 if self.proc.is_bert else 0  # skip [CLS]
        tags = [self.idx2tag.get(int(i), "O")
                for i in pred_ids[offset:offset + len(tokens)]]
        return extract_entity(tokens, tags)

    @timer
    def infer_scored(self, sentence: str):
        """infer()'s entities in order of appearance, each as {"type",
        "text", "start", "end", "confidence"}; the server must run with
        --confidence. The confidence is the model's posterior that the
        span's tokens carry exactly the decoded tags."""
        feats = self.make_feature(sentence)
        resp = self.client.predict(self.model_name, feats, self.version,
                                   options={"confidence": True})
        out = resp["outputs"]
        tokens = self.proc.tokenizer.tokenize(sentence)
        offset = 1 if self.proc.is_bert else 0  # skip [CLS]
        tags = [self.idx2tag.get(int(i), "O")
                for i in out["pred_ids"][0][offset:offset + len(tokens)]]
        return decode_prediction_scored(tokens, tags, out["span_a"][0],
                                        out["span_b"][0], offset=offset)

    @timer
    def infer_nbest(self, sentence: str, k: int):
        """The k best taggings of the sentence as {"alternatives": [{"rank",
        "prob", "entities"}], "entities": [{"type", "text", "start", "end",
        "support"}]} (eval.decode_prediction_nbest); the server must run
        with --nbest K, K >= k. support is the probability mass of the
        alternatives that contain the entity exactly, a lower bound on its
        posterior."""
        feats = self.make_feature(sentence)
        resp = self.client.predict(self.model_name, feats, self.version,
                                   options={"nbest": int(k)})
        out = resp["outputs"]
        tokens = self.proc.tokenizer.tokenize(sentence)
        offset = 1 if self.proc.is_bert else 0  # skip [CLS]
        tag_paths = [[self.idx2tag.get(int(i), "O") for i in path]
                     for path in out["nbest_paths"][0]]
        return decode_prediction_nbest(tokens, tag_paths,
                                       out["nbest_logp"][0], offset=offset)

    def constraint_words(self, n_tokens: int, spans=(), forbid=()
                         ) -> np.ndarray:
        """int64 [1, max_seq_len] allowed-tag words of a sentence of
        n_tokens tokens: span_words for the hints, forbid_types for the
        rest of the tokens; [CLS], [SEP] and the padding stay 0 (nothing
        known)."""
        offset = 1 if self.proc.is_bert else 0
        n = min(n_tokens, self.max_seq_len - 2 * offset)
        inner = span_words(spans, n, self.tag2idx)
        if forbid:
            inner = forbid_types(inner, forbid, self.tag2idx)
        words = np.zeros((1, self.max_seq_len), dtype=np.int64)
        words[0, offset:offset + n] = inner
        return words

    @timer
    def infer_constrained(self, sentence: str, spans=(), forbid=()):
        """infer() under what the caller knows: `spans` are (type, start,
        end) hints in token positions, end exclusive, that the tagging must
        contain; `forbid` are entity types it must not contain outside the
        hints. Returns {"entities": infer()'s dict, "feasible": bool,
        "path_score": float}; feasible is False (and entities empty) when no
        tagging satisfies the constraints. The server must run with
        --constraints."""
        feats = self.make_feature(sentence)
        tokens = self.proc.tokenizer.tokenize(sentence)
        feats["constraint_tags"] = self.constraint_words(len(tokens), spans,
                                                         forbid)
        resp = self.client.predict(self.model_name, feats, self.version)
        out = resp["outputs"]
        score = float(out["path_score"][0])
        offset = 1 if self.proc.is_bert else 0  # skip [CLS]
        tags = [self.idx2tag.get(int(i), "O")
                for i in out["pred_ids"][0][offset:offset + len(tokens)]]
        feasible = score > float("-inf")
        return {"entities": extract_entity(tokens, tags) if feasible else {},
                "feasible": feasible, "path_score": score}


def _parse_hint(text: str):
    try:
        typ, start, end = text.rsplit(":", 2)
        return typ, int(start), int(end)
    except ValueError:
        raise argparse.ArgumentTypeError(
            f"hint must be TYPE:START:END, got {text!r}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert_bilstm_crf")
    ap.add_argument("--data", default="msra")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=rpc.DEFAULT_PORT)
    ap.add_argument("--text", default=None,
                    help="one-shot inference instead of the REPL")
    ap.add_argument("--confidence", action="store_true",
                    help="print each entity with its confidence (server "
                         "started with --confidence)")
    ap.add_argument("--nbest", type=int, default=0, metavar="K",
                    help="print the K best taggings with their probabilities "
                         "and each entity's support (server started with "
                         "--nbest K or more); not together with --confidence")
    ap.add_argument("--hint", action="append", default=[], type=_parse_hint,
                    metavar="TYPE:START:END",
                    help="an entity the tagging must contain, in token "
                         "positions with END exclusive; repeatable (server "
                         "started with --constraints)")
    ap.add_argument("--forbid", action="append", default=[], metavar="TYPE",
                    help="an entity type the tagging must not contain; "
                         "repeatable (server started with --constraints)")
    args = ap.parse_args(argv)
    constrained = bool(args.hint or args.forbid)
    if constrained and args.nbest > 0:
        ap.error("--hint/--forbid cannot be combined with --nbest")
    if constrained and args.confidence:
        ap.error("--hint/--forbid cannot be combined with --confidence")
    if args.nbest > 0 and args.confidence:
        ap.error("--nbest and --confidence print different things; "
                 "give one of them")
    logging.basicConfig(level=logging.INFO)
    helper = InferHelper(args.model, args.data, args.host, args.port)
    infer = helper.infer_scored if args.confidence else helper.infer
    if args.nbest > 0:
        def infer(text, k=args.nbest):
            return helper.infer_nbest(text, k)
    if constrained:
        def infer(text):
            return helper.infer_constrained(text, args.hint, args.forbid)
    if args.text:
        print(infer(args.text))
        return 0
    while True:  # reference inference.py:110-115 interactive loop
        try:
            text = input("输入文本: ").strip()
        except (EOFError, KeyboardInterrupt):
            break
        if not text or text in ("q", "quit", "exit"):
            break
        print(infer(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
