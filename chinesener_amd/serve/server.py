"""gRPC prediction server (the reference's TF-Serving docker role,
server.sh:1-5): loads exported models from ./serving_model/{name}/{ver}/,
captures the hipGraph inference engine, replays recorded warmup requests
at startup, then serves unary Predict RPCs on port 8500."""
from __future__ import annotations

import argparse
import logging
import os
import pickle
import sys
import time
from concurrent import futures
from typing import Dict

import grpc

from ..config import EXPORT_DIR
from . import rpc
from .engine import InferenceEngine, MicroBatcher
from .export import latest_version_dir

log = logging.getLogger("chinesener_amd.serve")

WARMUP_FILE = os.path.join("assets.extra", "serving_warmup_requests")


def load_warmup(model_dir: str):
    path = os.path.join(model_dir, WARMUP_FILE)
    if not os.path.exists(path):
        return []
    with open(path, "rb") as f:
        return pickle.load(f)


class PredictionServicer:
    def __init__(self, engines: Dict[str, InferenceEngine]):
        self.engines = engines

    def predict(self, request_bytes: bytes, context) -> bytes:
        try:
            req = rpc.loads(request_bytes)
            name = req["model_spec"]["name"]
        except Exception as e:
            context.abort(grpc.StatusCode.INVALID_ARGUMENT,
                          f"malformed request: {e}")
        engine = self.engines.get(name)
        if engine is None:
            # context.abort raises; no code runs after it
            context.abort(grpc.StatusCode.NOT_FOUND,
                          f"model '{name}' not loaded "
                          f"(loaded: {sorted(self.engines)})")
        options = req.get("options") or {}
        scored = bool(options.get("confidence"))
        if scored and not engine.confidence:
            context.abort(grpc.StatusCode.FAILED_PRECONDITION,
                          f"model '{name}' is served without confidence; "
                          "start the server with --confidence")
        try:
            k = int(options.get("nbest") or 0)
        except (TypeError, ValueError):
            context.abort(grpc.StatusCode.INVALID_ARGUMENT,
                          f"option nbest must be an integer, got "
                          f"{options.get('nbest')!r}")
        if k < 0:
            context.abort(grpc.StatusCode.INVALID_ARGUMENT,
                          f"option nbest must be >= 0, got {k}")
        if k > engine.nbest:
            context.abort(grpc.StatusCode.FAILED_PRECONDITION,
                          f"model '{name}' is served with nbest="
                          f"{engine.nbest}, the request asks for {k}; "
                          f"start the server with --nbest {k} or more")
        try:
            hinted = "constraint_tags" in req["inputs"]
        except Exception as e:
            context.abort(grpc.StatusCode.INVALID_ARGUMENT,
                          f"malformed request: {e}")
        if hinted and not getattr(engine, "constraints", False):
            context.abort(grpc.StatusCode.FAILED_PRECONDITION,
                          f"model '{name}' is served without constraints; "
                          "start the server with --constraints")
        if hinted and k:
            context.abort(grpc.StatusCode.INVALID_ARGUMENT,
                          "constraint_tags cannot be combined with option "
                          "nbest")
        try:
            t0 = time.perf_counter()
            if hinted:
                outputs = engine.predict_constrained(req["inputs"], scored)
            elif k:
                outputs = engine.predict_nbest(req["inputs"], k, scored)
            elif scored:
                outputs = engine.predict_scored(req["inputs"])
            else:
                outputs = {"pred_ids": engine.predict(req["inputs"])}
            ms = (time.perf_counter() - t0) * 1000
            return rpc.dumps({"outputs": outputs,
                              "model_spec": req["model_spec"],
                              "latency_ms": ms})
        except Exception as e:  # surface as INTERNAL with the message
            log.exception("predict failed")
            context.abort(grpc.StatusCode.INTERNAL, str(e))


def build_server(engines: Dict[str, InferenceEngine], port: int,
                 max_workers: int = 4) -> grpc.Server:
    servicer = PredictionServicer(engines)
    handler = grpc.method_handlers_generic_handler(
        rpc.SERVICE,
        {rpc.METHOD: grpc.unary_unary_rpc_method_handler(
            servicer.predict,
            request_deserializer=None, response_serializer=None)})
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=max_workers))
    server.add_generic_rpc_handlers((handler,))
    server.add_insecure_port(f"[::]:{port}")
    return server


def serve(model_names, export_root: str = EXPORT_DIR,
          port: int = rpc.DEFAULT_PORT, wait: bool = True,
          use_graph=None, batch_sizes=(1, 4, 8), max_workers: int = 4,
          batching: bool = True, window_ms: float = 0.3,
          confidence: bool = False, nbest: int = 0,
          constraints: bool = False, trans_allowed=None):
    engines = {}
    for name in model_names:
        eng = InferenceEngine(name, export_root, batch_sizes=batch_sizes,
                              use_graph=use_graph, confidence=confidence,
                              nbest=nbest, constraints=constraints,
                              trans_allowed=trans_allowed)
        warm = load_warmup(latest_version_dir(name, export_root))
        eng.warmup(warm)
        log.info("loaded %s (%d warmup requests replayed)", name, len(warm))
        # micro-batching: coalesce concurrent clients into one replay
        # (the engine itself serializes under a lock; see MicroBatcher)
        engines[name] = MicroBatcher(eng, window_ms=window_ms) if batching else eng
    server = build_server(engines, port, max_workers=max_workers)
    server.start()
    log.info("serving %s on :%d", sorted(engines), port)
    if wait:
        server.wait_for_termination()
    return server


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True,
                    help="comma-separated exported model names")
    ap.add_argument("--export_root", default=EXPORT_DIR)
    ap.add_argument("--port", type=int, default=rpc.DEFAULT_PORT)
    ap.add_argument("--no_graph", action="store_true",
                    help="disable hipGraph capture (debug)")
    ap.add_argument("--no_batching", action="store_true",
                    help="disable concurrent-request micro-batching")
    ap.add_argument("--confidence", action="store_true",
                    help="also compute span scores, for requests that ask "
                         "for entity confidences")
    ap.add_argument("--nbest", type=int, default=0, metavar="K",
                    help="also compute the K best tag paths (1..8), for "
                         "requests with options={'nbest': k}, k <= K")
    ap.add_argument("--constraints", action="store_true",
                    help="decode under the allowed-tag words a request "
                         "carries as inputs['constraint_tags'] (answered "
                         "with pred_ids and path_score); not with --nbest")
    ap.add_argument("--structure", choices=["bio"], default=None,
                    help="with --constraints: allow only well-formed BIO "
                         "transitions; needs --data for the tag map")
    ap.add_argument("--data", default=None, metavar="NAME",
                    help="dataset whose tag map --structure uses (the "
                         "export carries none)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    trans_allowed = None
    if args.structure:
        if not (args.constraints and args.data):
            ap.error("--structure needs --constraints and --data NAME")
        from ..data.constraints import bio_transition_words
        from ..data.datasets import get_spec
        trans_allowed = bio_transition_words(get_spec(args.data).tag2idx)
    serve(args.model.split(","), args.export_root, args.port,
          use_graph=False if args.no_graph else None,
          batching=not args.no_batching, confidence=args.confidence,
          nbest=args.nbest, constraints=args.constraints,
          trans_allowed=trans_allowed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
