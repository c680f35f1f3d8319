"""Pure-torch fp32 reference implementations of every custom op.

These are (a) the CPU execution path, (b) the ground truth the HIP
kernels are tested against (numerics tests compare the gfx950 kernels to
these in fp32 — SURVEY.md §4 implication (a)). All are differentiable so
autograd provides backward on the reference path.

Shapes follow SURVEY.md §2.6: B=batch, L=seq len, H=hidden, T=labels.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

NEG_INF = -1e30


# ------------------------------------------------------------- layernorm
def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-12) -> torch.Tensor:
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def add_layernorm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor,
                  bias: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """Fused residual-add + LayerNorm (post-LN, as BERT and the reference's
    add_and_norm_layer, tools/transformer/modules.py:58-65)."""
    return F.layer_norm(x + residual, (x.shape[-1],), weight, bias, eps)


# ------------------------------------------------------------- bias gelu
def bias_gelu(x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BERT's gelu after a bias add — tanh approximation, the form
    google-research BERT / the reference's bert_base actually computes."""
    if bias is not None:
        x = x + bias
    return F.gelu(x, approximate="tanh")


# ------------------------------------------------------------- attention
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              mask: Optional[torch.Tensor] = None,
              scale: Optional[float] = None,
              p_drop: float = 0.0, training: bool = False) -> torch.Tensor:
    """Scaled dot-product attention. q,k,v: [B,H,L,D]; mask: [B,L] (1=keep).

    Matches BERT attention and the reference's
    scaled_dot_product_attention + normalize_attention
    (tools/transformer/modules.py:101-130): additive large-negative mask
    on padded KEY positions, softmax over the key axis.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    scores = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask is not None:
        key_mask = mask[:, None, None, :].to(scores.dtype)
        scores = scores + (1.0 - key_mask) * NEG_INF
    # softmax in at least fp32; fp64 inputs stay fp64 (the fp64 oracle of
    # the tiled-attention tests)
    acc = scores if scores.dtype == torch.float64 else scores.float()
    probs = torch.softmax(acc, dim=-1).to(q.dtype)
    if training and p_drop > 0:
        probs = F.dropout(probs, p_drop, training)
    return torch.matmul(probs, v)


def attention_tiled(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    lens: torch.Tensor, scale: float, tile_q: int,
                    tile_k: int, keep: float = 1.0,
                    keep_mask: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """CPU model of csrc/attention_tiled.hip forward: the tile-by-tile
    online-softmax recurrence, in the dtype of q. q,k,v [B,H,L,D]; lens
    [B] (>= 1); keep_mask bool [B,H,L,L] (True = kept) when keep < 1.

    Per (batch, query block): running row max m, running row sum l and an
    O accumulator over the key tiles below lens[b]; key tiles wholly at
    or beyond lens[b] are skipped; masked keys inside a tile contribute
    exactly 0. Dropout multiplies the un-normalised tile probabilities
    that feed P.V, l sums the undropped ones, and 1/(l*keep) is applied
    once at the end. Returns (out [B,H,L,D], lse [B,H,L])."""
    B, H, L, D = q.shape
    out = torch.zeros_like(q)
    lse = q.new_zeros(B, H, L)
    for b in range(B):
        kend = min(int(lens[b]), L)
        for q0 in range(0, L, tile_q):
            q1 = min(q0 + tile_q, L)
            qt = q[b, :, q0:q1]                              # [H,tq,D]
            m = q.new_full((H, q1 - q0), NEG_INF)
            l = q.new_zeros(H, q1 - q0)
            o = q.new_zeros(H, q1 - q0, D)
            for k0 in range(0, kend, tile_k):
                k1 = min(k0 + tile_k, L)
                s = torch.matmul(qt, k[b, :, k0:k1].transpose(-1, -2)) * scale
                valid = torch.arange(k0, k1, device=q.device) < kend
                s = torch.where(valid, s, torch.full_like(s, NEG_INF))
                m_new = torch.maximum(m, s.max(-1).values)
                alpha = torch.exp(m - m_new)
                p = torch.where(valid, torch.exp(s - m_new[..., None]),
                                torch.zeros_like(s))
                l = l * alpha + p.sum(-1)
                if keep < 1.0:
                    p = p * keep_mask[b, :, q0:q1, k0:k1].to(p.dtype)
                o = o * alpha[..., None] + torch.matmul(p, v[b, :, k0:k1])
                m = m_new
            out[b, :, q0:q1] = o / (l * keep)[..., None]
            lse[b, :, q0:q1] = m + torch.log(l)
    return out, lse


def attention_tiled_bwd(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor,
                        v: torch.Tensor, out: torch.Tensor, lse: torch.Tensor,
                        lens: torch.Tensor, scale: float, tile_q: int,
                        tile_k: int, keep: float = 1.0,
                        keep_mask: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU model of csrc/attention_tiled.hip backward: two sweeps that
    each recompute P = exp(S*scale - lse) and dP = dO V^T per tile.

    Sweep 1 (per key block, looping over query tiles) accumulates
    dV += P'^T dO and dK += dS^T Q; key blocks wholly at or beyond
    lens[b] are written as zeros. Sweep 2 (per query block, looping over
    key tiles below lens[b]) accumulates dQ += dS K. With the dropout
    mask M: P' = P*M/keep, dS = P*(dP*M/keep - delta)*scale, and
    delta = rowsum(dO*O) per query tile. Returns (dq, dk, dv)."""
    B, H, L, D = q.shape
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)

    def tile(b, q0, q1, k0, k1, kend):
        s = torch.matmul(q[b, :, q0:q1],
                         k[b, :, k0:k1].transpose(-1, -2)) * scale
        valid = torch.arange(k0, k1, device=q.device) < kend
        p = torch.where(valid, torch.exp(s - lse[b, :, q0:q1, None]),
                        torch.zeros_like(s))
        dp = torch.matmul(dout[b, :, q0:q1], v[b, :, k0:k1].transpose(-1, -2))
        pd = p
        if keep < 1.0:
            mk = keep_mask[b, :, q0:q1, k0:k1].to(p.dtype) / keep
            pd = p * mk
            dp = dp * mk
        delta = (dout[b, :, q0:q1] * out[b, :, q0:q1]).sum(-1, keepdim=True)
        return pd, p * (dp - delta) * scale

    for b in range(B):
        kend = min(int(lens[b]), L)
        # sweep 1: dK/dV per key block
        for k0 in range(0, L, tile_k):
            k1 = min(k0 + tile_k, L)
            if k0 >= kend:
                continue                      # rows stay exactly zero
            dk_acc = q.new_zeros(H, k1 - k0, D)
            dv_acc = q.new_zeros(H, k1 - k0, D)
            for q0 in range(0, L, tile_q):
                q1 = min(q0 + tile_q, L)
                pd, ds = tile(b, q0, q1, k0, k1, kend)
                dv_acc = dv_acc + torch.matmul(pd.transpose(-1, -2),
                                               dout[b, :, q0:q1])
                dk_acc = dk_acc + torch.matmul(ds.transpose(-1, -2),
                                               q[b, :, q0:q1])
            dk[b, :, k0:k1] = dk_acc
            dv[b, :, k0:k1] = dv_acc
        # sweep 2: dQ per query block
        for q0 in range(0, L, tile_q):
            q1 = min(q0 + tile_q, L)
            dq_acc = q.new_zeros(H, q1 - q0, D)
            for k0 in range(0, kend, tile_k):
                k1 = min(k0 + tile_k, L)
                _, ds = tile(b, q0, q1, k0, k1, kend)
                dq_acc = dq_acc + torch.matmul(ds, k[b, :, k0:k1])
            dq[b, :, q0:q1] = dq_acc
    return dq, dk, dv


def tener_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    u: torch.Tensor, vb: torch.Tensor, rel: torch.Tensor,
                    mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TENER relative attention (reference tools/transformer/tener.py:12-74).

    q,k,v: [B,H,L,D]; u,vb: per-head biases [H,D]; rel: sinusoidal table
    [2L, D] covering offsets [-L, L). Unscaled scores; the shift trick is
    replaced by direct indexing R[L-1+(j-i)].
    attn[b,h,i,j] = (q+u)·k + (q+vb)·R[j-i]   (no key projection upstream)
    """
    B, H, L, D = q.shape
    ac = torch.matmul(q + u[None, :, None, :], k.transpose(-1, -2))   # [B,H,L,L]
    # BD term: (q+vb) @ rel^T gives [B,H,L,2L]; gather offset j-i+L-1
    bd_full = torch.matmul(q + vb[None, :, None, :], rel.transpose(0, 1))  # [B,H,L,2L]
    idx = (torch.arange(L, device=q.device)[None, :]
           - torch.arange(L, device=q.device)[:, None]) + (L - 1)     # [L,L]
    bd = bd_full.gather(-1, idx.expand(B, H, L, L))
    scores = ac + bd
    if mask is not None:
        key_mask = mask[:, None, None, :].to(scores.dtype)
        scores = scores + (1.0 - key_mask) * NEG_INF
    # softmax in at least fp32; fp64 inputs stay fp64 (the fp64 oracle of
    # the TENER edge tests)
    acc = scores if scores.dtype == torch.float64 else scores.float()
    probs = torch.softmax(acc, dim=-1).to(q.dtype)
    return torch.matmul(probs, v)


def _bf16_rt(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 and back: one bf16 store of the kernel."""
    return x.to(torch.bfloat16).to(torch.float64)


def tener_attention_model(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                          u: torch.Tensor, vb: torch.Tensor,
                          rel: torch.Tensor, mask: Optional[torch.Tensor],
                          dout: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                     torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rounding model of csrc/tener.hip and its wrapper
    ops.functional.tener_attention: fp64 arithmetic with a bf16 round-trip
    wherever the kernel or the wrapper stores bf16. Shapes as in
    tener_attention; dout [B,H,L,D] is the upstream gradient. Returns
    (out, dq, dk, dv, du, dvb) in fp64; every value is bf16-exact.

    Rounding points (file:line at the time of writing):
      inputs   q, k, v, u, vb, rel, dout to bf16  (functional.py, the
               .to(bfloat16) casts of the wrapper; exact for bf16 inputs)
      qu, qv   bf16(q+u), bf16(q+vb): the wrapper's bf16 adds
      BD       qv R^T rounded to bf16 before the gather, forward
               tener.hip:99-100 and again in the backward's recompute
               tener.hip:260-261
      lse      stored fp32, tener.hip:167 (the only fp32 point modelled)
      P        softmax rounded to bf16 before P V, tener.hip:159
      out      bf16, tener.hip:187-188
      delta    rowsum(dout * out) from the bf16 out and dout,
               tener.hip:232-234 (fp32 sum, not rounded here)
      P (bwd)  exp(s - lse) rounded to bf16, tener.hip:286-288
      dS       P (dP - delta) rounded to bf16, tener.hip:345-346
      dv       P^T dO to bf16, tener.hip:319-320
      dk       dS^T qu to bf16, tener.hip:377-378
      dqu      dS K to bf16, tener.hip:415-416
      dqv      dBD R to bf16, tener.hip:453-454 (dBD is dS scattered,
               no further rounding)
      dq       bf16(dqu + dqv): autograd's bf16 accumulation of the two
               uses of q in the wrapper
      du, dvb  bf16 of the sum of dqu (dqv) over batch and rows: the
               reduction autograd forms over the wrapper's broadcast
    Not modelled: fp32 accumulation order inside the MFMAs, __expf,
    __logf, __frcp_rn, and the fp32 add of the AC and BD terms.

    Key columns at or beyond a row's length score -1e30 as in the kernel;
    an item of length 0 therefore gets the kernel's uniform 1/Lpad rows
    in the forward (Lpad = L rounded up to 32) and zero gradients."""
    B, H, L, D = q.shape
    r = _bf16_rt
    q_, k_, v_, do = (r(t.detach().double()) for t in (q, k, v, dout))
    u_, vb_, rel_ = (r(t.detach().double()) for t in (u, vb, rel))
    dev = q.device
    lens = (mask.long().sum(1) if mask is not None
            else torch.full((B,), L, dtype=torch.long, device=dev))
    lpad = ((L + 31) // 32) * 32
    qu = r(q_ + u_[None, :, None, :])
    qv = r(q_ + vb_[None, :, None, :])
    ar = torch.arange(L, device=dev)
    idx = ((ar[None, :] - ar[:, None]) + (L - 1)).expand(B, H, L, L)
    valid = (ar[None, :] < lens[:, None])[:, None, None, :]        # [B,1,1,L]

    bd_full = r(torch.matmul(qv, rel_.transpose(0, 1)))            # [B,H,L,2L]
    s = torch.matmul(qu, k_.transpose(-1, -2)) + bd_full.gather(-1, idx)
    s = torch.where(valid, s, torch.full_like(s, NEG_INF))
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    # an empty item: every column, the Lpad - L padded ones too, counts 1
    pad_cols = (lens == 0).double()[:, None, None, None] * (lpad - L)
    denom = e.sum(-1, keepdim=True) + pad_cols
    lse = (mx + torch.log(denom)).float().double()
    out = r(torch.matmul(r(e / denom), v_))

    delta = (do * out).sum(-1, keepdim=True)
    p = r(torch.where(valid, torch.exp(s - lse), torch.zeros_like(s)))
    dv = r(torch.matmul(p.transpose(-1, -2), do))
    dp = torch.matmul(do, v_.transpose(-1, -2))
    ds = r(p * (dp - delta))
    dk = r(torch.matmul(ds.transpose(-1, -2), qu))
    dqu = r(torch.matmul(ds, k_))
    dbd = torch.zeros_like(bd_full).scatter(-1, idx, ds)
    dqv = r(torch.matmul(dbd, rel_))
    return (out, r(dqu + dqv), dk, dv, r(dqu.sum((0, 2))),
            r(dqv.sum((0, 2))))


def sinusoidal_table(length: int, dim: int, device=None,
                     dtype=torch.float32) -> torch.Tensor:
    """Sinusoidal position table [length, dim] (reference modules.py:177-197)."""
    pos = torch.arange(length, device=device, dtype=torch.float32)[:, None]
    i = torch.arange(dim, device=device, dtype=torch.float32)[None, :]
    angle = pos / torch.pow(10000.0, (2 * (i // 2)) / dim)
    table = torch.where(i.long() % 2 == 0, torch.sin(angle), torch.cos(angle))
    return table.to(dtype)


def relative_table(seq_len: int, dim: int, device=None,
                   dtype=torch.float32) -> torch.Tensor:
    """Relative-position table over offsets [-L, L) as TENER uses
    (tener.py sinusoid over [-L, L))."""
    pos = torch.arange(-seq_len, seq_len, device=device, dtype=torch.float32)[:, None]
    i = torch.arange(dim, device=device, dtype=torch.float32)[None, :]
    angle = pos / torch.pow(10000.0, (2 * (i // 2)) / dim)
    table = torch.where(i.long() % 2 == 0, torch.sin(angle), torch.cos(angle))
    return table.to(dtype)


# ------------------------------------------------------------------- crf
def crf_log_likelihood(emissions: torch.Tensor, tags: torch.Tensor,
                       mask: torch.Tensor, transitions: torch.Tensor
                       ) -> torch.Tensor:
    """Per-sequence log-likelihood [B]. emissions [B,L,T] (fp32), tags [B,L],
    mask [B,L] (1 on real incl CLS/SEP as reference counts them,
    tools/layer.py:121), transitions [T,T] trans[i,j] = score(i -> j)."""
    B, L, T = emissions.shape
    emissions = emissions.float()
    mask = mask.to(torch.bool)
    score = emissions[:, 0].gather(1, tags[:, :1]).squeeze(1)
    alpha = emissions[:, 0]                                   # [B,T]
    for t in range(1, L):
        m = mask[:, t]
        # gold path score
        step = (transitions[tags[:, t - 1], tags[:, t]]
                + emissions[:, t].gather(1, tags[:, t:t + 1]).squeeze(1))
        score = score + step * m.to(score.dtype)
        # partition forward
        next_alpha = torch.logsumexp(
            alpha[:, :, None] + transitions[None, :, :], dim=1) + emissions[:, t]
        alpha = torch.where(m[:, None], next_alpha, alpha)
    log_z = torch.logsumexp(alpha, dim=1)
    return score - log_z


def allowed_sets(allowed: torch.Tensor, num_tags: int) -> torch.Tensor:
    """bool [..., T]: the allowed-tag set each int64 word of `allowed` stands
    for. Bit j < T set = tag j allowed; bits >= T are ignored; a word with no
    bit below T set means "nothing known" and stands for all T tags."""
    shifts = torch.arange(num_tags, device=allowed.device)
    # an arithmetic shift of a negative word still leaves bit j in bit 0
    bits = ((allowed.long().unsqueeze(-1) >> shifts) & 1).bool()
    return bits | ~bits.any(dim=-1, keepdim=True)


def crf_partial_log_likelihood(emissions: torch.Tensor, allowed: torch.Tensor,
                               mask: torch.Tensor, transitions: torch.Tensor,
                               dtype: torch.dtype = torch.float32
                               ) -> torch.Tensor:
    """Partial-annotation (fuzzy) CRF log-likelihood [B]:

        ll[b] = log sum_{y: y_t in S_t} exp score(y) - log sum_y exp score(y)

    over t < n_b, where n_b = mask[b].sum() (the mask is read as a length,
    as in every CRF op here) and S_t is the set allowed[b,t] encodes
    (allowed_sets). ll <= 0; one tag per position is crf_log_likelihood; all
    tags everywhere gives exactly 0. A row with n_b = 0 gives 0. Plain torch,
    differentiable by autograd: d ll / d emissions = P_S(y_t=j) - P(y_t=j).

    Transitions that leave an allowed set without a finite-score path
    (-1e4-style hard constraints) give a finite but meaningless value."""
    B, L, T = emissions.shape
    e = emissions.to(dtype)
    trans = transitions.to(dtype)
    lens = mask.long().sum(1)
    neg = torch.full((), -1e30, dtype=dtype, device=e.device)

    def log_z(open_):                       # open_: bool [B,L,T]
        alpha = torch.where(open_[:, 0], e[:, 0], neg)
        for t in range(1, L):
            nxt = torch.logsumexp(alpha[:, :, None] + trans[None], dim=1)
            nxt = torch.where(open_[:, t], nxt + e[:, t], neg)
            alpha = torch.where((t < lens)[:, None], nxt, alpha)
        return torch.logsumexp(alpha, dim=1)

    sets = allowed_sets(allowed, T)
    ll = log_z(sets) - log_z(torch.ones_like(sets))
    # a row with no closed tag inside its length is the free sum itself: 0,
    # and (through where) exactly zero gradients, not two that nearly cancel
    inside = torch.arange(L, device=e.device)[None, :] < lens[:, None]
    constrained = (~sets.all(dim=-1) & inside).any(dim=1)
    return torch.where(constrained, ll, torch.zeros_like(ll))


def crf_decode(emissions: torch.Tensor, mask: torch.Tensor,
               transitions: torch.Tensor) -> torch.Tensor:
    """Viterbi decode -> [B,L] best tag ids (padded positions keep tag of
    last real step, then zeroed)."""
    B, L, T = emissions.shape
    emissions = emissions.float()
    mask = mask.to(torch.bool)
    history = []
    alpha = emissions[:, 0]
    for t in range(1, L):
        scores = alpha[:, :, None] + transitions[None, :, :]    # [B,T,T]
        best, idx = scores.max(dim=1)
        next_alpha = best + emissions[:, t]
        keep = mask[:, t][:, None]
        alpha = torch.where(keep, next_alpha, alpha)
        history.append((idx, mask[:, t]))
    lens = mask.long().sum(1)                                   # [B]
    best_last = alpha.argmax(dim=1)                             # [B]
    out = torch.zeros(B, L, dtype=torch.long, device=emissions.device)
    cur = best_last.clone()
    out[:, L - 1] = cur
    batch_idx = torch.arange(B, device=emissions.device)
    for t in range(L - 2, -1, -1):
        idx, _ = history[t]                 # transition t -> t+1 backpointers
        within = (t + 1) < lens             # step back only inside the sequence
        prev = idx[batch_idx, cur]
        cur = torch.where(within, prev, cur)
        out[:, t] = cur
    # positions beyond len -> 0 ([PAD])
    pos = torch.arange(L, device=emissions.device)[None, :]
    return out * (pos < lens[:, None]).long()


def transition_sets(trans_allowed: Optional[torch.Tensor], num_tags: int,
                    device=None) -> torch.Tensor:
    """bool [T,T]: cell [i,j] = transition i -> j allowed, from one int64
    word per source tag (bit j of word i). Bits >= T are ignored. Unlike the
    position words there is no "empty means all" rule: a tag whose word has
    no bit below T set is terminal. None = everything allowed."""
    if trans_allowed is None:
        return torch.ones(num_tags, num_tags, dtype=torch.bool, device=device)
    shifts = torch.arange(num_tags, device=trans_allowed.device)
    return ((trans_allowed.long().unsqueeze(-1) >> shifts) & 1).bool()


def crf_decode_constrained(emissions: torch.Tensor, allowed: torch.Tensor,
                           mask: torch.Tensor, transitions: torch.Tensor,
                           trans_allowed: Optional[torch.Tensor] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Viterbi under constraints: (pred long [B,L], score [B]), the best tag
    path over the len = mask.sum(1) real positions among the paths that stay
    inside the sets `allowed` encodes (allowed_sets: int64 [B,L], bit j = tag
    j allowed, bits >= T ignored, no bit below T = all tags) and use only
    the transitions `trans_allowed` permits (transition_sets: int64 [T], bit
    j of word i = i -> j allowed, None = all). Computed in the dtype of
    ``emissions`` (pass ``.double()`` for fp64).

    Arithmetic and tie rule are crf_decode's: delta[t][j] = max_i(delta[t-1]
    [i] + trans[i][j]) + e[t][j], first maximum in index order per step and
    for the final tag. Masking is a select: forbidden transitions are NEG =
    -1e30 cells, and a tag that is closed at t or whose best predecessor
    term is not above NEG/2 is reset to exactly NEG, so nothing accumulates
    on NEG. Contract: real path scores stay above -1e29.

    score is the returned path's unnormalised score. A row without a path
    (len 0, or an infeasible constraint set) gets score -inf and an all-zero
    pred row; positions >= len are 0."""
    B, L, T = emissions.shape
    e = emissions.detach()
    dev = e.device
    neg = torch.full((), -1e30, dtype=e.dtype, device=dev)
    half = -0.5e30
    tr = torch.where(transition_sets(trans_allowed, T, dev).to(dev),
                     transitions.detach().to(e.dtype), neg)
    sets = allowed_sets(allowed, T)                              # [B,L,T]
    lens = mask.long().sum(1)                                    # [B]
    delta = torch.where(sets[:, 0], e[:, 0], neg)                # [B,T]
    history = []
    for t in range(1, L):
        best, idx = (delta[:, :, None] + tr[None]).max(dim=1)    # over i
        nxt = torch.where(sets[:, t] & (best > half), best + e[:, t], neg)
        delta = torch.where((t < lens)[:, None], nxt, delta)
        history.append(idx)
    score, cur = delta.max(dim=1)
    feasible = (score > half) & (lens > 0)
    out = torch.zeros(B, L, dtype=torch.long, device=dev)
    out[:, L - 1] = cur
    bi = torch.arange(B, device=dev)
    for t in range(L - 2, -1, -1):
        prev = history[t][bi, cur]          # transition t -> t+1 backpointers
        cur = torch.where((t + 1) < lens, prev, cur)
        out[:, t] = cur
    pos = torch.arange(L, device=dev)[None, :]
    keep = (pos < lens[:, None]) & feasible[:, None]
    score = torch.where(feasible, score,
                        torch.full_like(score, float("-inf")))
    return out * keep.long(), score


def crf_path_posterior(emissions: torch.Tensor, mask: torch.Tensor,
                       transitions: torch.Tensor, path: torch.Tensor,
                       dtype: torch.dtype = torch.float64
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Log-posterior of a tag path under the CRF, as two [B,L] arrays:

        log P(y_s..y_e = path_s..path_e | x) = span_a[s] + span_b[e]

    for every 0 <= s <= e < len, with

        span_a[t] = alpha_t(p_t) - C_t           (>= 0)
        span_b[t] = beta_t(p_t) + C_t - logZ     (<= 0)

    where alpha/beta are the log forward/backward messages and C_t the score
    of the path prefix 0..t. s == e is the token marginal of the path tag;
    s = 0, e = len-1 the sequence probability. Cells at t >= len, and rows
    with len == 0, hold 0; path ids are clamped to [0, T-1].

    The score says that positions s..e carry exactly these tags. Under BIO
    it does not also say that the entity stops at e, so it is an upper bound
    on the posterior of the strict entity.

    Plain recurrences in ``dtype`` (no running offsets): the ground truth
    for the HIP kernel."""
    B, L, T = emissions.shape
    em = emissions.detach().to(dtype)
    tr = transitions.detach().to(dtype)
    lens = mask.long().sum(1)                                    # [B]
    p = path.long().clamp(0, T - 1)
    pos = torch.arange(L, device=em.device)
    valid = pos[None, :] < lens[:, None]                         # [B,L]
    alphas = [em[:, 0]]
    for t in range(1, L):
        alphas.append(torch.logsumexp(
            alphas[-1][:, :, None] + tr[None, :, :], dim=1) + em[:, t])
    alphas = torch.stack(alphas, dim=1)                          # [B,L,T]
    zero = torch.zeros(B, T, dtype=dtype, device=em.device)
    betas = [zero] * L                     # beta_t = 0 for every t >= len-1
    beta = zero
    for t in range(L - 2, -1, -1):
        nxt = torch.logsumexp(
            tr[None, :, :] + (em[:, t + 1] + beta)[:, None, :], dim=2)
        beta = torch.where(((t + 1) < lens)[:, None], nxt, zero)
        betas[t] = beta
    betas = torch.stack(betas, dim=1)                            # [B,L,T]
    last = (lens - 1).clamp(min=0)
    log_z = torch.logsumexp(
        alphas[torch.arange(B, device=em.device), last], dim=1)  # [B]
    x_p = em.gather(2, p[:, :, None]).squeeze(2)                 # [B,L]
    inc = x_p.clone()
    inc[:, 1:] = inc[:, 1:] + tr[p[:, :-1], p[:, 1:]]
    c = torch.cumsum(inc * valid.to(dtype), dim=1)               # C_t
    a_p = alphas.gather(2, p[:, :, None]).squeeze(2)
    b_p = betas.gather(2, p[:, :, None]).squeeze(2)
    zeros = torch.zeros_like(c)
    span_a = torch.where(valid, a_p - c, zeros)
    span_b = torch.where(valid, b_p + c - log_z[:, None], zeros)
    return span_a, span_b


def crf_nbest(emissions: torch.Tensor, mask: torch.Tensor,
              transitions: torch.Tensor, k: int
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best tag paths of every row (list Viterbi):
    (paths [B,k,L] long, scores [B,k]), best first, computed in the dtype of
    ``emissions`` (pass ``.double()`` for fp64).

    scores[b,r] is the unnormalised score of the r-th best path: its
    emissions plus the transitions along it over the len = mask.sum(1) real
    positions.

    Order, which also settles exact ties: for tag j at step t the candidates
    (delta[t-1][i][r] + trans[i][j]) over predecessor i and rank r are ranked
    by value descending, then i ascending, then r ascending; the first k are
    kept and emis[t][j] is added afterwards (the association order of
    crf_decode and the Viterbi kernels). The final ranking over (j, r) is by
    value descending, then j, then r. Both are a stable descending sort over
    the tag-major flattening.

    A row has min(k, T**len) paths: ranks beyond that, and every rank of a
    row with len <= 0, get score -inf and an all-zero path. Positions >= len
    are 0."""
    B, L, T = emissions.shape
    k = int(k)
    if k < 1:
        raise ValueError(f"crf_nbest: k must be >= 1, got {k}")
    em = emissions.detach()
    tr = transitions.detach().to(em.dtype)
    dev = em.device
    lens = mask.long().sum(1)                                    # [B]
    ninf = float("-inf")
    delta = em.new_full((B, T, k), ninf)                         # [B,T,k]
    delta[:, :, 0] = em[:, 0]
    history = []
    for t in range(1, L):
        # [B, (i,r), j]: predecessor-major, so a stable sort breaks ties by
        # i and then r
        cand = (delta[:, :, :, None] + tr[None, :, None, :]).reshape(
            B, T * k, T)
        vals, idx = torch.sort(cand, dim=1, descending=True, stable=True)
        nxt = vals[:, :k].transpose(1, 2) + em[:, t][:, :, None]
        delta = torch.where((t < lens)[:, None, None], nxt, delta)
        history.append(idx[:, :k])                               # [B,k,T]
    fin, fidx = torch.sort(delta.reshape(B, T * k), dim=1, descending=True,
                           stable=True)
    scores = fin[:, :k]
    cur_j, cur_r = fidx[:, :k] // k, fidx[:, :k] % k             # [B,k]
    paths = torch.zeros(B, k, L, dtype=torch.long, device=dev)
    bi = torch.arange(B, device=dev)[:, None]
    for t in range(L - 1, 0, -1):
        within = (t < lens)[:, None]
        paths[:, :, t] = torch.where(within, cur_j, torch.zeros_like(cur_j))
        code = history[t - 1][bi, cur_r, cur_j]                  # (i, r) at t-1
        cur_j = torch.where(within, code // k, cur_j)
        cur_r = torch.where(within, code % k, cur_r)
    paths[:, :, 0] = cur_j
    present = torch.isfinite(scores) & (lens > 0)[:, None]
    scores = torch.where(present, scores, torch.full_like(scores, ninf))
    return paths * present[:, :, None].long(), scores


# ------------------------------------------------------------------ lstm
def lstm_forward(x: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
                 b: torch.Tensor, lens: torch.Tensor, reverse: bool = False,
                 activation: str = "tanh",
                 state_dropout: Optional[torch.Tensor] = None,
                 cell_clip: float = 0.0) -> torch.Tensor:
    """Single-direction LSTM over padded [B,L,E] -> [B,L,h].

    Gate order i,f,g,o (torch convention). `activation` applies to the
    cell candidate and output squash (reference supports tanh/relu,
    model/bilstm_crf.py:52 vs bert_bilstm_crf.py:42). Outputs at t>=len
    are zero (like dynamic_rnn with seq_len). state_dropout: [B,h]
    keep-mask/scale applied to h between steps (DropoutWrapper state
    keep-prob semantics, tools/layer.py:20-24).
    """
    B, L, E = x.shape
    h4 = w_hh.shape[1]
    h = h4 // 4
    act = torch.tanh if activation == "tanh" else torch.relu
    gates_x = x @ w_ih + b                                      # [B,L,4h]
    hs = x.new_zeros(B, L, h)
    ht = x.new_zeros(B, h)
    ct = x.new_zeros(B, h)
    steps = range(L - 1, -1, -1) if reverse else range(L)
    for t in steps:
        g = gates_x[:, t] + ht @ w_hh
        i, f, gc, o = g.split(h, dim=-1)
        i, f, o = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o)
        c_new = f * ct + i * act(gc)
        if cell_clip > 0:
            # TF LSTMCell cell_clip: bounds the relu recurrence
            c_new = c_new.clamp(-cell_clip, cell_clip)
        h_new = o * act(c_new)
        valid = (t < lens).to(x.dtype)[:, None]                 # [B,1]
        ct = valid * c_new + (1 - valid) * ct
        h_out = h_new * valid
        if state_dropout is not None:
            h_new = h_new * state_dropout
        ht = valid * h_new + (1 - valid) * ht
        hs[:, t] = h_out
    return hs


def bilstm_forward(x, w_ih_f, w_hh_f, b_f, w_ih_b, w_hh_b, b_b, lens,
                   activation="tanh", state_dropout=None,
                   cell_clip: float = 0.0) -> torch.Tensor:
    fw = lstm_forward(x, w_ih_f, w_hh_f, b_f, lens, False, activation,
                      state_dropout, cell_clip)
    bw = lstm_forward(x, w_ih_b, w_hh_b, b_b, lens, True, activation,
                      state_dropout, cell_clip)
    return torch.cat([fw, bw], dim=-1)


# ----------------------------------------------------------- softlexicon
def softlexicon_fuse(table: torch.Tensor, ids: torch.Tensor,
                     weights: torch.Tensor) -> torch.Tensor:
    """SoftLexicon gather-scale-reduce: table [V,E],
    ids/weights [B,L,40] (4 roles x 10 slots) -> [B,L,4*E]
    (weighted sum within each role group, concat groups)."""
    B, L, K = ids.shape
    R, S = 4, K // 4
    E = table.shape[1]
    emb = F.embedding(ids.long(), table)                       # [B,L,40,E]
    w = weights.to(emb.dtype).unsqueeze(-1)                    # [B,L,40,1]
    fused = (emb * w).view(B, L, R, S, E).sum(dim=3)           # [B,L,4,E]
    return fused.reshape(B, L, R * E)


# ---------------------------------------------------------------- losses
def masked_cross_entropy(logits: torch.Tensor, labels: torch.Tensor,
                         mask: torch.Tensor) -> torch.Tensor:
    """Mean CE over real tokens (reference tools/loss.py:5-16)."""
    T = logits.shape[-1]
    # at least fp32; fp64 logits stay fp64 (the fp64 oracle of the tests)
    lg = logits.reshape(-1, T)
    lg = lg if lg.dtype == torch.float64 else lg.float()
    loss = F.cross_entropy(lg, labels.reshape(-1), reduction="none")
    m = mask.reshape(-1).to(loss.dtype)
    return (loss * m).sum() / m.sum().clamp(min=1.0)


def dice_loss(logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor,
              idx_skip: Tuple[int, ...], alpha: float = 0.1,
              gamma: float = 1.0) -> torch.Tensor:
    """Dice/DSC loss (reference tools/loss.py:19-46): per-tag soft dice over
    real tokens, summed over tags excluding O/[PAD]/[CLS]/[SEP] (idx_skip),
    with focal-style (1-p)^alpha down-weight and gamma smoothing."""
    T = logits.shape[-1]
    probs = torch.softmax(logits.float(), dim=-1)
    m = mask.to(probs.dtype).reshape(-1, 1)
    probs = probs.reshape(-1, T)
    y = F.one_hot(labels.reshape(-1), T).to(probs.dtype)
    # vectorized over tags (the per-tag python loop launched ~50 tiny
    # kernels per call and cost 2.6 ms fwd+bwd on GPU; this form is a
    # handful of [R,T] passes, same math)
    p = probs * (1 - probs) ** alpha * m
    g = y * m
    num = 2 * (p * g).sum(0) + gamma
    den = p.sum(0) + g.sum(0) + gamma
    dsc = 1 - num / den                     # [T]
    keep = torch.ones(T, dtype=torch.bool, device=logits.device)
    for t in idx_skip:
        keep[t] = False
    return dsc[keep].sum()


def crf_partition_scan(emissions: torch.Tensor, mask: torch.Tensor,
                       transitions: torch.Tensor) -> torch.Tensor:
    """log Z via an ASSOCIATIVE parallel scan (Blelchel-style prefix
    product in the log semiring) — the round-3 blueprint for a
    depth-log(L) CRF forward kernel (docs/ROADMAP.md; the sequential
    scan kernel is latency-bound at ~6.8k cycles/step).

    Formulation: define per-step matrices
        M_t[i, j] = transitions[i, j] + emissions[t, j]   (t >= 1)
    masked steps use the identity of the (max,+/logsumexp) semiring
    (diag 0, off-diag -inf). Then
        alpha_L = alpha_0 (*) M_1 (*) ... (*) M_{L-1}
    with (A (*) B)[i, k] = logsumexp_j(A[i, j] + B[j, k]), which is
    associative — the matrix chain reduces pairwise in log2(L) rounds.
    Returns log Z [B] (bitwise-equivalent math to the sequential
    forward up to fp reduction order; tested against
    crf_log_likelihood)."""
    B, L, T = emissions.shape
    em = emissions.float()
    neg = torch.finfo(torch.float32).min / 4
    eye = torch.full((T, T), neg, device=em.device)
    eye.fill_diagonal_(0.0)
    if L == 1:
        return torch.logsumexp(em[:, 0], dim=1)
    # M[t] for t = 1..L-1, shape [B, L-1, T, T]
    m = mask[:, 1:].to(torch.bool)
    mats = transitions[None, None] + em[:, 1:, None, :]
    mats = torch.where(m[:, :, None, None], mats, eye[None, None])

    def combine(a, b):
        # [*, T, T] (*) [*, T, T] in the log semiring
        return torch.logsumexp(a[..., :, :, None] + b[..., None, :, :],
                               dim=-2)

    chain = mats
    while chain.shape[1] > 1:
        n = chain.shape[1]
        even = chain[:, 0:n - 1:2]
        odd = chain[:, 1:n:2]
        merged = combine(even, odd)
        if n % 2 == 1:                      # carry the unpaired tail
            merged = torch.cat([merged, chain[:, -1:]], dim=1)
        chain = merged
    total = chain[:, 0]                     # [B, T, T]
    alpha0 = em[:, 0]
    return torch.logsumexp(
        torch.logsumexp(alpha0[:, :, None] + total, dim=1), dim=1)
