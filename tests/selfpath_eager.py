"""TEST INFRASTRUCTURE -- plain-torch restatement of the SelAttention primitive (SelfPath), any dtype, any device.  Written from the
formulae, for the GPU machine where no reference tree exists:

    res = PReLU(conv(x))                        Conv2d(32, 32, 3, pad 1, bias); ONE slope for both activations
    tok = res as [B, N = H W, 32]
    qkv = tok W_qkv^T                           [B, N, 192 heads]: q | k | v column blocks, head hd at 64 hd inside each
    o   = softmax(q k^T / 8) v                  per (batch, head) over all N keys
    v1  = o W_out^T + b_out
    ln  = LayerNorm_32(v1), eps 1e-5
    out = PReLU(conv2(ln as [B, 32, H, W]))
"""
import torch
import torch.nn.functional as F


def prelu(z, a):
    return torch.where(z >= 0, z, a * z)


def attention_core(qkv, heads):
    """qkv [B, N, 192 heads] -> (out [B, N, 64 heads], lse [B, heads, N]) with the N x N scores materialised."""
    B, N, _ = qkv.shape
    q, k, v = (qkv[..., i * 64 * heads:(i + 1) * 64 * heads].reshape(B, N, heads, 64).permute(0, 2, 1, 3) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * 0.125
    lse = torch.logsumexp(s, dim=-1)
    o = torch.matmul(torch.exp(s - lse[..., None]), v)
    return o.permute(0, 2, 1, 3).reshape(B, N, 64 * heads), lse


def scores(qkv, heads):
    B, N, _ = qkv.shape
    q, k = (qkv[..., i * 64 * heads:(i + 1) * 64 * heads].reshape(B, N, heads, 64).permute(0, 2, 1, 3) for i in range(2))
    return torch.matmul(q, k.transpose(-1, -2)) * 0.125


def selfpath(x, sd, heads, taps=None):
    """x [B,32,H,W]; sd: the ten state_dict tensors in x's dtype / device.  taps (dict): receives z1, tok, qkv, o, lse, v1, ln, z2."""
    B, C, H, W = x.shape
    a = sd["prelu.weight"]
    z1 = F.conv2d(x, sd["conv.weight"], sd["conv.bias"], padding=1)
    tok = prelu(z1, a).flatten(2).transpose(1, 2)
    qkv = tok @ sd["cross_attn.to_qkv.weight"].t()
    o, lse = attention_core(qkv, heads)
    v1 = o @ sd["cross_attn.to_out.0.weight"].t() + sd["cross_attn.to_out.0.bias"]
    ln = F.layer_norm(v1, (C,), sd["norm1.weight"], sd["norm1.bias"], 1e-5)
    z2 = F.conv2d(ln.reshape(B, H, W, C).permute(0, 3, 1, 2), sd["conv2.weight"], sd["conv2.bias"], padding=1)
    if taps is not None:
        taps.update(z1=z1, tok=tok, qkv=qkv, o=o, lse=lse, v1=v1, ln=ln, z2=z2)
    return prelu(z2, a)


def state(sd_numpy, dtype, device="cpu"):
    return {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in sd_numpy.items()}
