"""Off-GPU, ops.linear_dropout_add_layernorm is literally
dropout_add_layernorm(linear(x)): same values, same grads, same RNG use."""
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.models.bert import BertLayer


def _run(f, leaves, seed):
    ts = [t.clone().requires_grad_() for t in leaves]
    torch.manual_seed(seed)
    y = f(*ts)
    y.float().pow(2).sum().backward()
    return y.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("training,p", [(True, 0.1), (True, 0.0), (False, 0.1)])
def test_cpu_op_equals_composition(tiny_bert_config, training, p):
    cfg = tiny_bert_config
    torch.manual_seed(0)
    layer = BertLayer(cfg)
    H, Fi = cfg.hidden_size, cfg.intermediate_size
    for lin, lw, lb, k_in in ((layer.attn_out, layer.ln1_w, layer.ln1_b, H),
                              (layer.ffn_out, layer.ln2_w, layer.ln2_b, Fi)):
        leaves = [torch.randn(3, 16, k_in), lin.weight.detach(),
                  lin.bias.detach() + 0.1 * torch.randn(H),
                  torch.randn(3, 16, H), lw.detach() + 0.1 * torch.randn(H),
                  lb.detach() + 0.1 * torch.randn(H)]

        def fused(x, w, b, r, g, beta):
            return ops.linear_dropout_add_layernorm(x, w, b, r, g, beta,
                                                    cfg.layer_norm_eps, p,
                                                    training)

        def composed(x, w, b, r, g, beta):
            return ops.dropout_add_layernorm(ops.linear(x, w, b), r, g, beta,
                                             cfg.layer_norm_eps, p, training)

        y1, g1 = _run(fused, leaves, 7)
        y2, g2 = _run(composed, leaves, 7)
        assert torch.equal(y1, y2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


def test_cpu_bert_layer_uses_composition_math(tiny_bert_config):
    """BertLayer.forward through the new op equals the spelled-out
    sublayer chain with the same seed."""
    cfg = tiny_bert_config
    torch.manual_seed(1)
    layer = BertLayer(cfg).train()
    x = torch.randn(2, 16, cfg.hidden_size)
    mask = torch.ones(2, 16, dtype=torch.long)
    lens = mask.sum(1)
    torch.manual_seed(11)
    got = layer(x, mask, lens)

    torch.manual_seed(11)
    B, L, H = x.shape
    qkv = ops.linear(x, layer.qkv.weight, layer.qkv.bias) \
        .reshape(B, L, 3, layer.n_heads, layer.head_dim)
    ctx = ops.attention_qkv(qkv, mask=mask, lens=lens,
                            p_drop=layer.p_attn_drop,
                            training=True).reshape(B, L, H)
    a = ops.linear(ctx, layer.attn_out.weight, layer.attn_out.bias)
    h = ops.dropout_add_layernorm(a, x, layer.ln1_w, layer.ln1_b, layer.eps,
                                  layer.p_drop, True)
    f = ops.bias_gelu(ops.linear(h, layer.ffn_in.weight), layer.ffn_in_bias)
    f = ops.linear(f, layer.ffn_out.weight, layer.ffn_out.bias)
    want = ops.dropout_add_layernorm(f, h, layer.ln2_w, layer.ln2_b,
                                     layer.eps, layer.p_drop, True)
    assert torch.equal(got, want)
