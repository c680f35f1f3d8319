"""hipGraph-captured inference engine.

The reference serves a frozen SavedModel through TF-Serving
(server.sh:1-5, export signature tools/train_utils.py:173-185). The
MI355X-native equivalent loads the exported state_dict and captures the
whole PREDICT path — embedding → BERT encoder → BiLSTM → logits →
CRF Viterbi — into a hipGraph (torch.cuda.CUDAGraph on ROCm *is*
hipGraphLaunch under the hood) per supported batch size, so a request
replays one pre-built graph: zero launch latency for ~100 small kernels.

Batch shapes are fixed at capture time; warmup requests (warmup.py,
mirroring the reference's TF-Serving warmup records) establish them.
Requests are padded up to the nearest captured batch size.

With ``confidence=True`` the same path also runs the CRF path-posterior
kernel (token-softmax heads: a cumulative log-softmax) and the captured
outputs are (pred_ids, span_a, span_b): log P(tokens s..e carry the
decoded tags) = span_a[s] + span_b[e], see ops.crf_path_posterior.

With ``nbest=K`` (1..8) it also runs the n-best CRF decode and the captured
outputs gain (nbest_paths [B,K,L], nbest_scores [B,K], nbest_logp [B,K]),
see ops.crf_nbest. The two switches are independent and combine; pred_ids
is the Viterbi decode on every engine.

With ``constraints=True`` the decode is the constrained Viterbi kernel
(ops.crf_viterbi_constrained): ``constraint_tags`` (int64 [batch, L]
allowed-tag words, data.constraints builds them) becomes one more static
input whose zero default means "nothing known", so hinted and plain requests
replay the same graph, and the outputs gain path_score [B]. ``trans_allowed``
(int64 [T], e.g. data.constraints.bio_transition_words) is applied once to
the model's CRF. Not combinable with nbest.
"""
from __future__ import annotations

import logging
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..config import EXPORT_DIR
from .export import load_exported

log = logging.getLogger("chinesener_amd.serve")

# feature dtypes the models consume (see data/preprocess.py feature build)
_INT_KEYS = ("token_ids", "segment_ids", "mask", "label_ids", "task_ids",
             "softword_ids", "softlexicon_ids", "bichar_ids",
             "constraint_tags")

# Captured-graph inputs a request may legitimately omit: an all-zeros
# value is their semantic default (segment 0 = single-sentence BERT
# input; padding-id word-enhance features). token_ids/mask (and task_ids
# for mtl/adv routing) must always be supplied.
_DEFAULTABLE_KEYS = frozenset({
    "segment_ids", "softword_ids", "ex_softword_ids",
    "softlexicon_ids", "softlexicon_weights", "bichar_ids",
})


# a constraints engine may also omit the allowed-tag words: all-zero words
# say nothing about any position, which is free decoding
_CONSTRAINT_KEY = "constraint_tags"

NBEST_MAX = 8
_CONF_KEYS = ("span_a", "span_b")
_NBEST_KEYS = ("nbest_paths", "nbest_scores", "nbest_logp")


def _need_nbest(name: str, have: int, k: Optional[int]) -> int:
    """The k a predict_nbest call gets, or the RuntimeError it deserves."""
    if not have:
        raise RuntimeError(
            f"engine for '{name}' was built without nbest; predict_nbest "
            "needs InferenceEngine(..., nbest=K)")
    k = have if k is None else int(k)
    if not 1 <= k <= have:
        raise RuntimeError(
            f"engine for '{name}' was built with nbest={have}; "
            f"predict_nbest(k={k}) needs 1 <= k <= {have}")
    return k


def _nbest_view(full: Dict[str, np.ndarray], k: int, lo: int = 0,
                hi: Optional[int] = None, scored: bool = False
                ) -> Dict[str, np.ndarray]:
    """Rows lo:hi of a full result as predict_nbest returns them."""
    out = {"pred_ids": full["pred_ids"][lo:hi]}
    for key in _NBEST_KEYS:
        out[key] = full[key][lo:hi, :k]
    if scored:
        for key in _CONF_KEYS:
            out[key] = full[key][lo:hi]
    return out


def _need_confidence(name: str, have: bool):
    if not have:
        raise RuntimeError(
            f"engine for '{name}' was built without confidence=True;"
            " predict_scored needs InferenceEngine(..., confidence=True)")


def _need_constraints(name: str, have: bool):
    if not have:
        raise RuntimeError(
            f"engine for '{name}' was built without constraints=True; "
            "constraint_tags and predict_constrained need "
            "InferenceEngine(..., constraints=True)")


def _constrained_view(full: Dict[str, np.ndarray], lo: int = 0,
                      hi: Optional[int] = None, scored: bool = False
                      ) -> Dict[str, np.ndarray]:
    """Rows lo:hi of a full result as predict_constrained returns them."""
    keys = ("pred_ids", "path_score") + (_CONF_KEYS if scored else ())
    return {k: full[k][lo:hi] for k in keys}


class _CapturedGraph:
    def __init__(self, graph, static_in: Dict[str, torch.Tensor],
                 static_out: Tuple[torch.Tensor, ...]):
        self.graph = graph
        self.static_in = static_in
        self.static_out = static_out


class InferenceEngine:
    """Runs PREDICT for one exported model. GPU: hipGraph replay per
    batch-size bucket; CPU (tests): eager no_grad."""

    def __init__(self, name: str, export_root: str = EXPORT_DIR,
                 version: Optional[int] = None,
                 batch_sizes: Sequence[int] = (1, 4, 8),
                 max_seq_len: Optional[int] = None,
                 use_graph: Optional[bool] = None,
                 device: Optional[str] = None,
                 confidence: bool = False,
                 nbest: int = 0,
                 constraints: bool = False,
                 trans_allowed=None):
        self.name = name
        self.confidence = bool(confidence)
        self.nbest = int(nbest)
        self.constraints = bool(constraints)
        if not 0 <= self.nbest <= NBEST_MAX:
            raise ValueError(
                f"nbest must be between 0 and {NBEST_MAX}, got {nbest}")
        if self.constraints and self.nbest:
            raise ValueError(
                "constraints=True cannot be combined with nbest: n-best "
                "under constraints is not available")
        if trans_allowed is not None and not self.constraints:
            raise ValueError("trans_allowed needs constraints=True")
        self.out_keys = (("pred_ids",)
                         + (_CONF_KEYS if self.confidence else ())
                         + (_NBEST_KEYS if self.nbest else ())
                         + (("path_score",) if self.constraints else ()))
        self.device = device or ("cuda" if torch.cuda.is_available() else "cpu")
        self.model, self.params = load_exported(name, export_root,
                                                device=self.device,
                                                version=version)
        self.bf16 = (self.device.startswith("cuda")
                     and self.params.get("dtype", "bf16") == "bf16")
        if self.bf16:
            # pure-bf16 inference (fused bf16 attention/LN/GELU kernels)
            from ..train.precision import convert_bf16_mixed
            convert_bf16_mixed(self.model)
        self.model.eval()
        self.max_seq_len = max_seq_len or self.params.get("max_seq_len", 150)
        self.batch_sizes = sorted(batch_sizes)
        self.use_graph = (use_graph if use_graph is not None
                          else self.device.startswith("cuda"))
        self._graphs: Dict[int, _CapturedGraph] = {}
        self._DEFAULTABLE = _DEFAULTABLE_KEYS
        if self.constraints:
            self._DEFAULTABLE = _DEFAULTABLE_KEYS | {_CONSTRAINT_KEY}
            crf = getattr(self.model, "crf", None)
            if crf is None:
                raise ValueError(
                    f"model '{name}' has no single-task CRF head; "
                    "constraints=True needs one")
            if trans_allowed is not None:
                crf.constrain_transitions(trans_allowed)
        self.n_requests = 0
        self._lock = threading.Lock()

    # ---------------------------------------------------------- capture
    def _example_features(self, batch: int) -> Dict[str, torch.Tensor]:
        """Static input buffers for one bucket, shaped like the exported
        model's feature schema (word-enhance keys included when the model
        name demands them, reference base_preprocess.py:22-33)."""
        L = self.max_seq_len
        feats = {
            "token_ids": torch.ones(batch, L, dtype=torch.long),
            "segment_ids": torch.zeros(batch, L, dtype=torch.long),
            "mask": torch.ones(batch, L, dtype=torch.long),
        }
        name = self.name
        if "softword" in name and "ex_softword" not in name:
            feats["softword_ids"] = torch.zeros(batch, L, dtype=torch.long)
        if "ex_softword" in name:
            feats["ex_softword_ids"] = torch.zeros(batch, L, 5)
        if "softlexicon" in name:
            feats["softlexicon_ids"] = torch.zeros(batch, L, 40, dtype=torch.long)
            feats["softlexicon_weights"] = torch.zeros(batch, L, 40)
        if "bichar" in name:
            feats["bichar_ids"] = torch.zeros(batch, L, dtype=torch.long)
        if "mtl" in name or "adv" in name:
            feats["task_ids"] = torch.ones(batch, L, dtype=torch.long)
        if self.constraints:
            feats[_CONSTRAINT_KEY] = torch.zeros(batch, L, dtype=torch.long)
        out = {}
        for k, v in feats.items():
            if v.is_floating_point() and self.bf16:
                v = v.to(torch.bfloat16)
            out[k] = v.to(self.device)
        return out

    def _forward(self, feats: Dict[str, torch.Tensor]
                 ) -> Tuple[torch.Tensor, ...]:
        """The tensors named by self.out_keys: pred_ids, then span_a and
        span_b on a confidence engine, then the nbest triple on an nbest
        engine or path_score on a constraints engine."""
        if self.constraints:
            out = self.model(feats, compute_pred=True,
                             compute_conf=self.confidence, constrained=True)
            conf = tuple(out.span_scores) if self.confidence else ()
            return (out.pred_ids,) + conf + (out.path_score,)
        if not (self.confidence or self.nbest):
            return (self.model(feats, compute_pred=True).pred_ids,)
        if not self.nbest:
            out = self.model(feats, compute_pred=True, compute_conf=True)
            return (out.pred_ids,) + tuple(out.span_scores)
        out = self.model(feats, compute_pred=True,
                         compute_conf=self.confidence,
                         compute_nbest=self.nbest)
        conf = tuple(out.span_scores) if self.confidence else ()
        return (out.pred_ids,) + conf + tuple(out.nbest)

    @torch.no_grad()
    def _capture(self, batch: int) -> _CapturedGraph:
        static_in = self._example_features(batch)
        # two eager warmup passes on a side stream (allocator steady-state)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._forward(static_in)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = self._forward(static_in)
        log.info("hipGraph captured for %s batch=%d L=%d", self.name, batch,
                 self.max_seq_len)
        return _CapturedGraph(graph, static_in, static_out)

    def warmup(self, requests: Optional[List[Dict[str, np.ndarray]]] = None):
        """Capture all batch buckets (optionally driven by recorded warmup
        requests, whose batch sizes define the buckets — the reference's
        assets.extra/tf_serving_warmup_requests role)."""
        if requests:
            sizes = sorted({r["token_ids"].shape[0] for r in requests})
            self.batch_sizes = sorted(set(self.batch_sizes) | set(sizes))
        if self.use_graph:
            for b in self.batch_sizes:
                if b not in self._graphs:
                    self._graphs[b] = self._capture(b)
        if requests:
            for r in requests:
                self.predict(r)

    # ---------------------------------------------------------- predict
    def _bucket(self, batch: int) -> Optional[int]:
        for b in self.batch_sizes:
            if b >= batch:
                return b
        return None

    @torch.no_grad()
    def predict(self, features: Dict[str, np.ndarray]) -> np.ndarray:
        """features: numpy arrays [B, ...] (as built by
        data.preprocess.BasicProc.build_seq_feature, stacked).
        Returns pred_ids [B, L].

        Serialized per engine: the gRPC server runs a thread pool and the
        hipGraph static input/output buffers are shared state — without
        the lock two in-flight requests would overwrite each other."""
        with self._lock:
            return self._predict(features)[0]

    @torch.no_grad()
    def predict_scored(self, features: Dict[str, np.ndarray]
                       ) -> Dict[str, np.ndarray]:
        """predict() plus the span scores of the decoded tags:
        {"pred_ids" [B,L], "span_a" [B,L] f64, "span_b" [B,L] f64}. For
        tokens s..e of a row, exp(span_a[s] + span_b[e]) is the posterior
        that they carry exactly the decoded tags (an upper bound on the
        strict BIO entity's, which would also need the entity to stop at
        e); eval.decode_prediction_scored turns it into per-entity
        confidences. Needs an engine built with confidence=True."""
        _need_confidence(self.name, self.confidence)
        full = self.predict_full(features)
        return {k: full[k] for k in ("pred_ids",) + _CONF_KEYS}

    @torch.no_grad()
    def predict_nbest(self, features: Dict[str, np.ndarray],
                      k: Optional[int] = None, scored: bool = False
                      ) -> Dict[str, np.ndarray]:
        """predict() plus the k best tag paths of every row, best first:
        {"pred_ids" [B,L], "nbest_paths" [B,k,L], "nbest_scores" [B,k] f32,
        "nbest_logp" [B,k] f64}; exp(nbest_logp) is the posterior of the
        whole path. Ranks a row does not have hold -inf and a zero path.
        pred_ids is what predict() returns; rank 0 equals it except under
        exact score ties. k defaults to the engine's nbest and may not
        exceed it. Needs an engine built with nbest=K. scored=True adds
        predict_scored's span_a/span_b from the same replay (the engine
        then needs confidence=True as well)."""
        k = _need_nbest(self.name, self.nbest, k)
        if scored:
            _need_confidence(self.name, self.confidence)
        return _nbest_view(self.predict_full(features), k, scored=scored)

    @torch.no_grad()
    def predict_constrained(self, features: Dict[str, np.ndarray],
                            scored: bool = False) -> Dict[str, np.ndarray]:
        """Decode under features["constraint_tags"] (int64 [B,L] allowed-tag
        words, 0 = nothing known; absent = all zero) and the engine's
        trans_allowed: {"pred_ids" [B,L], "path_score" [B] f32}. path_score
        is the unnormalised score of the returned path, -inf (and a zero
        row) where the constraints admit no path. scored=True adds
        span_a/span_b, the unconstrained model's posterior of the returned
        path (the engine then needs confidence=True as well). Needs an
        engine built with constraints=True."""
        _need_constraints(self.name, self.constraints)
        if scored:
            _need_confidence(self.name, self.confidence)
        return _constrained_view(self.predict_full(features), scored=scored)

    @torch.no_grad()
    def predict_full(self, features: Dict[str, np.ndarray]
                     ) -> Dict[str, np.ndarray]:
        """Everything this engine computes per request, by name
        (self.out_keys)."""
        with self._lock:
            return dict(zip(self.out_keys, self._predict(features)))

    def _predict(self, features: Dict[str, np.ndarray]
                 ) -> Tuple[np.ndarray, ...]:
        self.n_requests += 1
        if _CONSTRAINT_KEY in features:
            _need_constraints(self.name, self.constraints)
        batch = features["token_ids"].shape[0]
        tensors = {}
        for k, v in features.items():
            if k == "label_ids":
                continue  # PREDICT path never consumes labels
            a = np.asarray(v)
            t = torch.as_tensor(a)
            if k in _INT_KEYS or a.dtype.kind in "iu":
                t = t.long()
            else:
                t = t.to(torch.bfloat16) if self.bf16 else t.float()
            tensors[k] = t

        bucket = self._bucket(batch) if self.use_graph else None
        if bucket is not None and bucket in self._graphs:
            g = self._graphs[bucket]
            # Zero EVERY captured buffer first: the graph consumes all of
            # them, and a key absent from this request must not silently
            # retain the previous request's data (cross-request leakage).
            missing = [k for k in g.static_in
                       if k not in tensors and k not in self._DEFAULTABLE]
            if missing:
                raise KeyError(
                    f"request for model '{self.name}' is missing required "
                    f"feature(s) {missing}; captured graph consumes "
                    f"{sorted(g.static_in)}")
            for k, buf in g.static_in.items():
                buf.zero_()
                t = tensors.get(k)
                if t is None:
                    continue  # defaultable key: zeros are its default
                sl = [slice(0, s) for s in t.shape]
                buf[tuple(sl)].copy_(t.to(self.device), non_blocking=True)
            g.graph.replay()
            torch.cuda.synchronize()
            return tuple(o[:batch].cpu().numpy() for o in g.static_out)

        # eager path (CPU, or batch larger than any bucket)
        dev = {k: t.to(self.device) for k, t in tensors.items()}
        if self.constraints and _CONSTRAINT_KEY not in dev:
            dev[_CONSTRAINT_KEY] = torch.zeros_like(dev["token_ids"])
        return tuple(o.cpu().numpy() for o in self._forward(dev))


class MicroBatcher:
    """Concurrency layer over InferenceEngine (VERDICT weak #6: the
    engine serializes requests under one lock because hipGraph static
    buffers are shared). Instead of queueing N clients for N replays,
    concurrent requests are coalesced into ONE padded batch replayed
    once: p99 under k concurrent clients stays ~1 replay + window
    instead of k replays.

    predict() blocks the calling thread until its rows are ready, so the
    gRPC handler uses it as a drop-in engine replacement."""

    def __init__(self, engine: InferenceEngine, max_batch: Optional[int] = None,
                 window_ms: float = 0.3):
        self.engine = engine
        self.max_batch = max_batch or max(engine.batch_sizes)
        self.window = window_ms / 1000.0
        self._cv = threading.Condition()
        self._queue: list = []          # (features, slot, event)
        self._stop = False
        self._worker = threading.Thread(target=self._run, daemon=True)
        self._worker.start()

    # engine API passthrough used by the server
    @property
    def name(self):
        return self.engine.name

    @property
    def confidence(self):
        return self.engine.confidence

    @property
    def nbest(self):
        return self.engine.nbest

    @property
    def constraints(self):
        return self.engine.constraints

    def warmup(self, requests=None):
        return self.engine.warmup(requests)

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._worker.join(timeout=2.0)

    def predict(self, features: Dict[str, np.ndarray]) -> np.ndarray:
        return self._submit(features, scored=False)

    def predict_scored(self, features: Dict[str, np.ndarray]
                       ) -> Dict[str, np.ndarray]:
        """Engine.predict_scored through the batcher. Scored and plain
        requests of one signature share a replay; each caller gets back
        what it asked for."""
        _need_confidence(self.name, self.engine.confidence)
        return self._submit(features, scored=True)

    def predict_nbest(self, features: Dict[str, np.ndarray],
                      k: Optional[int] = None, scored: bool = False
                      ) -> Dict[str, np.ndarray]:
        """Engine.predict_nbest through the batcher. Plain, scored and
        nbest requests of one signature share one replay of everything the
        engine computes; each caller gets back what it asked for."""
        k = _need_nbest(self.name, self.engine.nbest, k)
        if scored:
            _need_confidence(self.name, self.engine.confidence)
        return self._submit(features, scored=scored, nbest=k)

    def predict_constrained(self, features: Dict[str, np.ndarray],
                            scored: bool = False) -> Dict[str, np.ndarray]:
        """Engine.predict_constrained through the batcher. Hinted and plain
        requests of one signature share a replay (a plain one rides along
        with all-zero words); each caller gets back what it asked for."""
        _need_constraints(self.name, self.engine.constraints)
        if scored:
            _need_confidence(self.name, self.engine.confidence)
        return self._submit(features, scored=scored, constrained=True)

    def _submit(self, features: Dict[str, np.ndarray], scored: bool,
                nbest: int = 0, constrained: bool = False):
        if _CONSTRAINT_KEY in features:
            _need_constraints(self.name, self.engine.constraints)
        elif self.engine.constraints:
            # before _sig is taken, so hinted and plain requests coalesce
            features = dict(features)
            features[_CONSTRAINT_KEY] = np.zeros(
                np.asarray(features["token_ids"]).shape, dtype=np.int64)
        ev = threading.Event()
        slot: Dict[str, object] = {"scored": scored, "nbest": nbest,
                                   "constrained": constrained}
        with self._cv:
            self._queue.append((features, slot, ev))
            self._cv.notify()
        ev.wait()
        if "err" in slot:
            raise slot["err"]  # type: ignore[misc]
        return slot["out"]     # type: ignore[return-value]

    # ------------------------------------------------------------ worker
    @staticmethod
    def _sig(features) -> tuple:
        return tuple(sorted((k, tuple(np.asarray(v).shape[1:]))
                            for k, v in features.items()))

    def _take_compatible(self) -> list:
        """Pop a prefix-compatible group (same keys + trailing shapes)
        totalling <= max_batch rows. Leaves incompatible requests queued
        for the next cycle."""
        group, rows, sig = [], 0, None
        rest = []
        for item in self._queue:
            f = item[0]
            n = int(np.asarray(f["token_ids"]).shape[0])
            s = self._sig(f)
            if sig is None:
                sig = s
            if s == sig and rows + n <= self.max_batch:
                group.append(item)
                rows += n
            else:
                rest.append(item)
        if not group and self._queue:
            # an oversize request (batch > max_batch) can never fill a
            # group: dispatch it alone (the engine's eager path handles
            # batches beyond the largest captured bucket)
            group = [self._queue[0]]
            rest = self._queue[1:]
        self._queue = rest
        return group

    def _run(self):
        while True:
            with self._cv:
                while not self._queue and not self._stop:
                    self._cv.wait(0.25)
                if self._stop:
                    pending = self._queue
                    self._queue = []
                    for _, slot, ev in pending:
                        slot["err"] = RuntimeError("batcher stopped")
                        ev.set()
                    return
                deadline = time.perf_counter() + self.window
                while (sum(int(np.asarray(f["token_ids"]).shape[0])
                           for f, _, _ in self._queue) < self.max_batch):
                    remaining = deadline - time.perf_counter()
                    if remaining <= 0:
                        break
                    self._cv.wait(remaining)
                batch = self._take_compatible()
            if not batch:
                continue
            try:
                merged = {k: np.concatenate(
                    [np.asarray(f[k]) for f, _, _ in batch])
                    for k in batch[0][0]}
                if (self.engine.constraints
                        or any(slot["nbest"] for _, slot, _ in batch)):
                    full = self.engine.predict_full(merged)  # the superset
                elif any(slot["scored"] for _, slot, _ in batch):
                    full = self.engine.predict_scored(merged)
                else:
                    full = {"pred_ids": self.engine.predict(merged)}
                i = 0
                for f, slot, ev in batch:
                    n = int(np.asarray(f["token_ids"]).shape[0])
                    if slot["constrained"]:
                        slot["out"] = _constrained_view(full, i, i + n,
                                                        slot["scored"])
                    elif slot["nbest"]:
                        slot["out"] = _nbest_view(full, slot["nbest"], i,
                                                  i + n, slot["scored"])
                    elif slot["scored"]:
                        slot["out"] = {k: full[k][i:i + n]
                                       for k in ("pred_ids",) + _CONF_KEYS}
                    else:
                        slot["out"] = full["pred_ids"][i:i + n]
                    i += n
            except Exception as e:
                for _, slot, ev in batch:
                    slot["err"] = e
            finally:
                for _, slot, ev in batch:
                    ev.set()


class FastPredict:
    """Reference FastPredict parity (tools/fast_predict.py:10-38): the
    reference holds an Estimator.predict generator open to avoid graph
    reload per call; here the captured hipGraph engine IS that persistent
    predictor — this thin alias keeps the familiar API."""

    def __init__(self, engine: InferenceEngine):
        self.engine = engine

    def predict(self, features):
        return self.engine.predict(features)

    def predict_scored(self, features):
        return self.engine.predict_scored(features)

    def predict_nbest(self, features, k=None, scored=False):
        return self.engine.predict_nbest(features, k, scored)

    def predict_constrained(self, features, scored=False):
        return self.engine.predict_constrained(features, scored)
