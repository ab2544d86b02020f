"""CPU comparand of the layout model (not imported by the package): the architecture written out in plain torch operations with the
dropout masks as explicit inputs, the weighted loss, the accuracy statistics, a deterministic name-keyed parameter fill and seeded input
builders.  Written from the documented behaviour of ``nn.TransformerEncoderLayer`` (post-norm, ReLU, eps 1e-5, batch_first=False) and of
the reference's layout training script; any dtype.

Shapes: boxes (N, W, 4); the SEQUENCE axis of the encoder is N, the batch axis is W (see ocrs_models_amd/layout.py).
Mask shapes per (layer, site): site 0 (W * 4, N, N) = (word * 4 + head, query, key); sites 1 and 3 (N * W, 256); site 2 (N * W, 1024).
"""
from __future__ import annotations

import math
import zlib
from collections import OrderedDict

import numpy as np
import torch

D, H, FF, LAYERS, CLASSES = 256, 4, 1024, 6, 2
CASES = {"lay1": {"N": 16, "W": 50, "seed": 31}, "lay2": {"N": 1, "W": 7, "seed": 32}, "lay3": {"N": 5, "W": 33, "seed": 33}}
POS_WEIGHT = 10.0


def param_specs():
    """(name, shape) in the state-dict order of the reference's LayoutModel"""
    out = []
    for i in range(LAYERS):
        p = f"encode.layers.{i}."
        out += [(p + "self_attn.in_proj_weight", (3 * D, D)), (p + "self_attn.in_proj_bias", (3 * D,)), (p + "self_attn.out_proj.weight", (D, D)),
                (p + "self_attn.out_proj.bias", (D,)), (p + "linear1.weight", (FF, D)), (p + "linear1.bias", (FF,)), (p + "linear2.weight", (D, FF)),
                (p + "linear2.bias", (D,)), (p + "norm1.weight", (D,)), (p + "norm1.bias", (D,)), (p + "norm2.weight", (D,)), (p + "norm2.bias", (D,))]
    out += [("classify.weight", (CLASSES, D)), ("classify.bias", (CLASSES,))]
    return out


def fill_params(seed: int, dtype=torch.float32):
    """Deterministic, keyed by the tensor's name: weights uniform in +-1/sqrt(fan_in), LayerNorm gains near (not equal to) 1, non-zero biases
    -- every gradient path carries signal.  Values are drawn in float64 and rounded to fp32 first, so every dtype sees the same numbers."""
    P = OrderedDict()
    for name, shape in param_specs():
        r = np.random.RandomState((zlib.crc32(name.encode()) + 7919 * seed) % 2147483647)
        u = r.uniform(-1.0, 1.0, shape)
        if name.endswith("weight") and len(shape) == 2:
            v = u / math.sqrt(shape[1])
        elif "norm" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * u
        else:
            v = 0.1 * u
        P[name] = torch.from_numpy(v.astype(np.float32)).to(dtype)
    return P


def make_inputs(N: int, W: int, seed: int):
    """boxes (N, W, 4) fp32 with coordinates in [0, 2000), a tenth of them exact .5 values (round-half-even matters), targets (N, W, 2) with
    7-9 % positives, and a zero-padded tail of rows per page (boxes and targets 0), as the dataset pads pages to a fixed word count."""
    r = np.random.RandomState(seed + 5000)
    boxes = r.uniform(0.0, 1999.0, (N, W, 4))
    half = r.uniform(0, 1, (N, W, 4)) < 0.1
    boxes = np.where(half, np.floor(boxes) + 0.5, boxes).astype(np.float32)
    rate = r.uniform(0.07, 0.09)
    target = (r.uniform(0, 1, (N, W, 2)) < rate).astype(np.float32)
    for n in range(N):
        n_words = W - int(r.randint(0, max(W // 4, 1) + 1))
        boxes[n, n_words:] = 0.0
        target[n, n_words:] = 0.0
    return torch.from_numpy(boxes), torch.from_numpy(target)


def angle_rates():
    j = torch.arange(32, dtype=torch.float32)
    return 1 / (10_000 ** (j / 32))


def embed(boxes: torch.Tensor) -> torch.Tensor:
    """fp32: round half to even, angle = float(p) * rate rounded once to fp32, [sin(32) | cos(32)] per coordinate"""
    N, W, _ = boxes.shape
    pos = torch.round(boxes.float()).to(torch.int32).to(torch.float32).unsqueeze(-1)
    ang = pos * angle_rates()
    return torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(N, W, 4 * 64)


def embed64(boxes: torch.Tensor) -> torch.Tensor:
    """the same angles (fp32 product) with sine and cosine evaluated in float64: the comparand of the device's libm"""
    N, W, _ = boxes.shape
    pos = torch.round(boxes.float()).to(torch.int32).to(torch.float32).unsqueeze(-1)
    ang = (pos * angle_rates()).double()
    return torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(N, W, 4 * 64)


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _drop(x, masks, key, p, shape):
    if masks is None or p == 0:
        return x
    return x * masks[key].reshape(shape).to(x.dtype) * (1.0 / (1.0 - p))


def attention(q, k, v, mask=None, p=0.0):
    """q, k, v (S, W, 256) -> (S, W, 256): per (word, head) softmax(q k^T / 8) v over the sequence axis S"""
    S, W, _ = q.shape
    sp = lambda t: t.reshape(S, W, H, D // H).permute(1, 2, 0, 3)  # (W, H, S, 64)
    qh, kh, vh = sp(q), sp(k), sp(v)
    pr = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D // H), -1)
    if mask is not None and p > 0:
        pr = pr * mask.reshape(W, H, S, S).to(pr.dtype) * (1.0 / (1.0 - p))
    return (pr @ vh).permute(2, 0, 1, 3).reshape(S, W, D)


def encoder(P, x, masks=None, p=0.0):
    N, W, _ = x.shape
    for i in range(LAYERS):
        pre = f"encode.layers.{i}."
        qkv = x @ P[pre + "self_attn.in_proj_weight"].T + P[pre + "self_attn.in_proj_bias"]
        att = attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], None if masks is None else masks.get((i, 0)), p)
        a = att @ P[pre + "self_attn.out_proj.weight"].T + P[pre + "self_attn.out_proj.bias"]
        x = layer_norm(x + _drop(a, masks, (i, 1), p, (N, W, D)), P[pre + "norm1.weight"], P[pre + "norm1.bias"])
        h = torch.relu(x @ P[pre + "linear1.weight"].T + P[pre + "linear1.bias"])
        h = _drop(h, masks, (i, 2), p, (N, W, FF))
        f = h @ P[pre + "linear2.weight"].T + P[pre + "linear2.bias"]
        x = layer_norm(x + _drop(f, masks, (i, 3), p, (N, W, D)), P[pre + "norm2.weight"], P[pre + "norm2.bias"])
    return x


def forward(P, boxes, masks=None, p=0.0, return_probs=False):
    """logits (N, W, 2) in the dtype of P; the embedding is always evaluated in fp32 and cast"""
    dtype = next(iter(P.values())).dtype
    x = encoder(P, embed(boxes).to(dtype), masks, p)
    y = x @ P["classify.weight"].T + P["classify.bias"]
    return torch.sigmoid(y) if return_probs else y


def weighted_loss(pred, target, pos_weight=POS_WEIGHT):
    """BCE with logits, positive class weight, mean over all elements"""
    t = target.to(pred.dtype)
    lw = 1 + (pos_weight - 1) * t
    return ((1 - t) * pred + lw * (torch.log1p(torch.exp(-pred.abs())) + torch.clamp(-pred, min=0))).mean()


def counts(prob, target):
    """[tp0, pp0, tg0, tp1, pp1, tg1] from probabilities thresholded at 0.5"""
    out = []
    for c in (0, 1):
        pp, tg = prob[..., c] >= 0.5, target[..., c] != 0
        out += [int((pp & tg).sum()), int(pp.sum()), int(tg.sum())]
    return out


def ratios(cnt):
    """the four fp32 ratios (start precision, start recall, end precision, end recall); 0 / 0 = NaN"""
    f = np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        return [float(f(cnt[0]) / f(cnt[1])), float(f(cnt[0]) / f(cnt[2])), float(f(cnt[3]) / f(cnt[4])), float(f(cnt[3]) / f(cnt[5]))]


class Stats:
    """running sums of the four ratios (Python floats), means on read"""

    def __init__(self):
        self.sums = [0.0] * 4
        self.updates = 0

    def update(self, prob, target):
        self.updates += 1
        for i, v in enumerate(ratios(counts(prob, target))):
            self.sums[i] += v

    def means(self):
        return [s / self.updates for s in self.sums]


def adam_steps(P, boxes, target, steps, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8):
    """plain Adam on the comparand (no dropout): returns the parameters after `steps` updates"""
    P = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in P.items())
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    s = {k: torch.zeros_like(v) for k, v in P.items()}
    for t in range(1, steps + 1):
        loss = weighted_loss(forward(P, boxes), target)
        grads = torch.autograd.grad(loss, list(P.values()))
        with torch.no_grad():
            for (k, v), g in zip(P.items(), grads):
                m[k].mul_(b1).add_(g, alpha=1 - b1)
                s[k].mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = (s[k].sqrt() / math.sqrt(1 - b2**t)).add_(eps)
                v.addcdiv_(m[k], denom, value=-lr / (1 - b1**t))
    return OrderedDict((k, v.detach()) for k, v in P.items())
