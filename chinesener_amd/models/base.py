"""Model base types: every graph is an nn.Module whose forward takes the
feature dict and returns ModelOutput — the torch analog of the
reference's ``build_graph(features, labels, params, is_training) ->
(loss, pred_ids[, task_ids])`` contract (model/bert_bilstm_crf.py:8-34,
model/bert_bilstm_crf_mtl.py:8-66)."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn


class ModelOutput(NamedTuple):
    loss: Optional[torch.Tensor]
    pred_ids: Optional[torch.Tensor] = None
    task_ids: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    # (span_a, span_b), fp64 [B,L]: log P(tags s..e as decoded) =
    # span_a[s] + span_b[e]; filled only with compute_conf=True
    span_scores: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    # (paths long [B,k,L], scores f32 [B,k], logp f64 [B,k]): the k best tag
    # paths, best first; filled only with compute_nbest=k > 0
    nbest: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
    # f32 [B]: unnormalised score of pred_ids, -inf on a row whose constraints
    # admit no path; filled only with constrained=True
    path_score: Optional[torch.Tensor] = None


class NerModel(nn.Module):
    """Base: holds resolved params; subclasses implement forward()."""

    def __init__(self, params: Dict):
        super().__init__()
        self.params = dict(params)

    def reject_partial_labels(self, features) -> None:
        """For the heads that cannot train on partial annotations: a batch
        of a partially annotated dataset is an error, not a silent fall back
        to its placeholder label_ids."""
        if "allowed_tags" in features:
            raise ValueError(
                f"{type(self).__name__}: the batch carries 'allowed_tags' "
                "(a partially annotated dataset), which only the single-task "
                "CRF models train on")

    def reject_constrained(self, constrained: bool) -> None:
        """For the heads without constrained decoding."""
        if constrained:
            raise ValueError(
                f"{type(self).__name__}: constrained=True is only available "
                "on the single-task CRF models")

    def forward(self, features: Dict[str, torch.Tensor],
                compute_pred: bool = False,
                compute_conf: bool = False,
                compute_nbest: int = 0,
                constrained: bool = False) -> ModelOutput:
        """compute_conf=True implies decoding and also fills
        ModelOutput.span_scores (see ops.crf_path_posterior).
        compute_nbest=k > 0 implies decoding and also fills
        ModelOutput.nbest with the k best paths (see ops.crf_nbest).
        pred_ids stays the Viterbi decode; rank 0 of nbest equals it except
        under exact score ties.
        constrained=True (single-task CRF models) decodes under
        features["constraint_tags"], int64 [B,L] allowed-tag words with 0 =
        nothing known, and the transitions CRF.constrain_transitions set:
        pred_ids becomes that path and path_score its score. With
        compute_conf the span scores are the unconstrained model's posterior
        of the returned path. Not combinable with compute_nbest."""
        raise NotImplementedError


class GradReverse(torch.autograd.Function):
    """Gradient reversal (reference FlipGradientBuilder,
    tools/train_utils.py:47-63): identity forward, -lambda * grad backward."""

    @staticmethod
    def forward(ctx, x, lam: float):
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return -ctx.lam * g, None


def flip_gradient(x: torch.Tensor, lam: float = 1.0) -> torch.Tensor:
    return GradReverse.apply(x, lam)
