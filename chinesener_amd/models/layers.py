"""Shared layer library (parity with reference tools/layer.py).

BiLSTM (:10-41), multi-kernel CNN (:44-60), CRF layer (:112-149) live
here as nn.Modules composed from the ops layer; the BERT encoder is in
bert.py, transformer encoders in transformer.py.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class BiLSTM(nn.Module):
    """Bidirectional LSTM with the reference's DropoutWrapper semantics
    (output keep-prob; activation tanh/relu selectable —
    tools/layer.py:10-41, model/bilstm_crf.py:48-52)."""

    def __init__(self, input_size: int, hidden_size: int, activation: str = "tanh",
                 keep_prob: float = 0.8, cell_clip: float = None):
        super().__init__()
        self.hidden_size = hidden_size
        self.activation = activation
        # relu cells are unbounded; clip the cell state like TF's
        # LSTMCell(cell_clip=...) to keep the recurrence stable
        self.cell_clip = (10.0 if activation == "relu" else 0.0) \
            if cell_clip is None else cell_clip
        self.dropout = nn.Dropout(1.0 - keep_prob)

        # TF LSTMCell defaults the reference builds on: glorot-uniform
        # kernels, zero bias with forget-gate bias 1.0 — keeps the (relu)
        # recurrence away from the exponential-growth regime over L=150
        # steps (a uniform 1/sqrt(h) init sits near the stability cliff).
        def w(*shape):
            t = torch.empty(*shape)
            nn.init.xavier_uniform_(t)
            return nn.Parameter(t)

        def b():
            t = torch.zeros(4 * hidden_size)
            t[hidden_size:2 * hidden_size] = 1.0  # forget gate (i,f,g,o)
            return nn.Parameter(t)
        self.w_ih_f, self.w_hh_f, self.b_f = w(input_size, 4 * hidden_size), \
            w(hidden_size, 4 * hidden_size), b()
        self.w_ih_b, self.w_hh_b, self.b_b = w(input_size, 4 * hidden_size), \
            w(hidden_size, 4 * hidden_size), b()

    def forward(self, x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        out = ops.bilstm(x, self.w_ih_f, self.w_hh_f, self.b_f,
                         self.w_ih_b, self.w_hh_b, self.b_b, lens,
                         self.activation, cell_clip=self.cell_clip)
        return self.dropout(out)


class MultiKernelCNN(nn.Module):
    """Per-kernel conv1d SAME + dropout, concat filters
    (reference cnn_layer, tools/layer.py:44-60).

    torch ``padding='same'`` is bit-identical to TF SAME at stride 1 for
    every kernel size incl. even ones — both put the extra zero on the
    RIGHT (total k-1, left (k-1)//2) — verified by
    tests/test_ops_reference.py::test_conv1d_same_matches_tf_same."""

    def __init__(self, input_size: int, filters: int = 128,
                 kernel_sizes: List[int] = (2, 3, 4), keep_prob: float = 0.8):
        super().__init__()
        self.convs = nn.ModuleList([
            nn.Conv1d(input_size, filters, k, padding="same")
            for k in kernel_sizes])
        self.dropout = nn.Dropout(1.0 - keep_prob)
        self.output_size = filters * len(kernel_sizes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:   # [B,L,E]
        if x.is_cuda and x.dtype == torch.bfloat16:
            # SAME conv1d as pad + unfold + linear: the unfolded GEMM is
            # K-major NT, so it rides the in-tree MFMA GEMM / hipBLASLt
            # measured dispatch like every other linear
            outs = []
            for c in self.convs:
                k = c.kernel_size[0]
                left = (k - 1) // 2
                xp = F.pad(x, (0, 0, left, (k - 1) - left))     # [B,L+k-1,E]
                u = xp.unfold(1, k, 1)                          # [B,L,E,k]
                u = u.transpose(2, 3).reshape(x.shape[0], x.shape[1], -1)
                w = c.weight.permute(0, 2, 1).reshape(c.weight.shape[0], -1)
                y = ops.linear(u.contiguous(), w.contiguous(), c.bias)
                outs.append(self.dropout(torch.relu(y)))
            return torch.cat(outs, dim=-1)
        xt = x.transpose(1, 2)
        outs = [self.dropout(torch.relu(c(xt))) for c in self.convs]
        return torch.cat(outs, dim=1).transpose(1, 2)


class CRF(nn.Module):
    """Linear-chain CRF head (reference crf_layer/crf_decode,
    tools/layer.py:112-149): loss over the full padded length including
    CLS/SEP (seq_len counts them, comment :121)."""

    def __init__(self, num_tags: int):
        super().__init__()
        self.num_tags = num_tags
        # near-zero init: with the reference's crf diff-LR x500, a
        # strong random transition prior locks borderline seeds into the
        # all-O basin before the encoder learns anything
        self.transitions = nn.Parameter(
            torch.empty(num_tags, num_tags).uniform_(-0.01, 0.01))
        # allowed-transition words of decode_constrained (None = all): not
        # persistent, so checkpoints and exports do not change
        self.register_buffer("trans_allowed", None, persistent=False)

    def constrain_transitions(self, words) -> None:
        """Set (or with None clear) the allowed-transition words constrained
        decoding uses: int64 [num_tags], bit j of word i = transition i -> j
        allowed (data.constraints.bio_transition_words builds the BIO ones).
        Free decoding, the losses and the posteriors are not affected."""
        if words is not None:
            words = torch.as_tensor(words, dtype=torch.int64).to(
                self.transitions.device).reshape(-1)
            if words.numel() != self.num_tags:
                raise ValueError(
                    f"constrain_transitions: {words.numel()} words for "
                    f"{self.num_tags} tags")
        self.trans_allowed = words

    def neg_log_likelihood(self, emissions, tags, mask) -> torch.Tensor:
        """Sum of -log p(tags | emissions) over the batch."""
        ll = ops.crf_nll(emissions.float(), tags, mask, self.transitions)
        return -ll.sum()

    def partial_neg_log_likelihood(self, emissions, allowed, mask
                                   ) -> torch.Tensor:
        """Sum over the batch of -log p(the paths inside the allowed sets |
        emissions): the partial-annotation loss. allowed is int64 [B,L],
        one bit per permitted tag id (ops.crf_partial_nll)."""
        ll = ops.crf_partial_nll(emissions.float(), allowed, mask,
                                 self.transitions)
        return -ll.sum()

    def loss(self, emissions, features) -> torch.Tensor:
        """The batch's summed training loss: the partial-annotation loss
        when the features carry "allowed_tags" (a partially annotated
        dataset), else neg_log_likelihood of "label_ids"."""
        if "allowed_tags" in features:
            return self.partial_neg_log_likelihood(
                emissions, features["allowed_tags"], features["mask"])
        return self.neg_log_likelihood(emissions, features["label_ids"],
                                       features["mask"])

    def decode(self, emissions, mask) -> torch.Tensor:
        return ops.crf_viterbi(emissions.float(), mask, self.transitions)

    def decode_scored(self, emissions, mask):
        """(pred, (span_a, span_b)): decode()'s tags plus the fp64 [B,L]
        posterior arrays of that path, log P(tags s..e as decoded) =
        span_a[s] + span_b[e]. It is the posterior of exactly these tags on
        s..e, hence an upper bound on the strict BIO entity's."""
        pred, span_a, span_b = ops.crf_decode_scored(
            emissions.float(), mask, self.transitions)
        return pred, (span_a, span_b)

    def decode_nbest(self, emissions, mask, k: int):
        """(paths long [B,k,L], scores f32 [B,k], logp f64 [B,k]): the k
        best tag paths, best first, their unnormalised scores and log
        posteriors (ops.crf_nbest). Ranks a row does not have get -inf and
        a zero path. Rank 0 is decode()'s path except under exact score
        ties."""
        return ops.crf_nbest(emissions.float(), mask, self.transitions, k)

    def decode_constrained(self, emissions, mask, allowed):
        """(pred long [B,L], score f32 [B]): the best path inside the
        allowed-tag words (int64 [B,L], the words of the partial-annotation
        loss; 0 = nothing known) that uses only the transitions set with
        constrain_transitions. score is that path's unnormalised score; a
        row whose constraints admit no path gets -inf and a zero row
        (ops.crf_viterbi_constrained)."""
        return ops.crf_viterbi_constrained(emissions.float(), allowed, mask,
                                           self.transitions,
                                           self.trans_allowed)

    def predict(self, emissions, mask, compute_pred: bool,
                compute_conf: bool, *, nbest: int = 0, allowed=None):
        """The (pred, span_scores, nbest) triple a model's forward returns:
        pred is decode()'s (None unless anything is asked for), span_scores
        is filled with compute_conf, nbest is decode_nbest(..., nbest) or
        None when nbest is 0.

        With `allowed` (int64 [B,L] words) the decode is decode_constrained
        and a fourth item, its path score [B], is returned. span_scores are
        then crf_path_posterior of the constrained path: the unconstrained
        model's posterior of what was returned, not a posterior conditioned
        on the constraints. N-best under constraints is not available."""
        if allowed is not None:
            if nbest > 0:
                raise ValueError(
                    "constrained decoding cannot be combined with n-best")
            pred, score = self.decode_constrained(emissions, mask, allowed)
            conf = None
            if compute_conf:
                conf = ops.crf_path_posterior(emissions.float(), mask,
                                              self.transitions, pred)
            return pred, conf, None, score
        if compute_conf:
            pred, conf = self.decode_scored(emissions, mask)
        else:
            want = compute_pred or nbest > 0
            pred, conf = (self.decode(emissions, mask) if want else None), None
        best = self.decode_nbest(emissions, mask, nbest) if nbest > 0 else None
        return pred, conf, best

    def outputs(self, emissions, features, compute_pred: bool,
                compute_conf: bool, compute_nbest: int = 0,
                constrained: bool = False) -> dict:
        """predict() as the ModelOutput fields of a single-task CRF model:
        pred_ids, span_scores, nbest and path_score. constrained=True decodes
        under features["constraint_tags"]."""
        if not constrained:
            pred, conf, best = self.predict(
                emissions, features["mask"], compute_pred, compute_conf,
                nbest=compute_nbest)
            return dict(pred_ids=pred, span_scores=conf, nbest=best)
        if compute_nbest > 0:
            raise ValueError(
                "constrained=True cannot be combined with compute_nbest > 0")
        if "constraint_tags" not in features:
            raise KeyError(
                "constrained=True needs features['constraint_tags'] (int64 "
                "[B,L] allowed-tag words, 0 = nothing known)")
        pred, conf, _, score = self.predict(
            emissions, features["mask"], True, compute_conf,
            allowed=features["constraint_tags"])
        return dict(pred_ids=pred, span_scores=conf, path_score=score)


class TokenEmbedding(nn.Module):
    """Char/word embedding, optionally initialized from a pretrained matrix
    carried in data params (reference base_preprocess.py:223-226) and
    optionally frozen (bichar pretrained constant, bilstm_crf_bichar.py)."""

    def __init__(self, vocab_size: int, dim: int,
                 pretrained: Optional[torch.Tensor] = None, freeze: bool = False,
                 padding_idx: int = 0):
        super().__init__()
        self.emb = nn.Embedding(vocab_size, dim, padding_idx=padding_idx)
        if pretrained is not None:
            with torch.no_grad():
                self.emb.weight.copy_(torch.as_tensor(pretrained))
        if freeze:
            self.emb.weight.requires_grad_(False)

    def forward(self, ids):
        return self.emb(ids)
