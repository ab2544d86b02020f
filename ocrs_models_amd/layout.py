"""LayoutModel (sinusoidal box encoding -> 6-layer post-norm transformer encoder -> Linear(256, 2)) with the reference's constructor /
forward signature and state-dict keys (ocrs_models/models.py:271-406), executed by the gfx950 kernels of libocrs_hip.so.

The batch-axis quirk is part of the contract: the reference builds ``nn.TransformerEncoderLayer`` with torch's default
``batch_first=False`` and feeds it ``(N, W, 256)``, so the SEQUENCE axis is N (the pages of the batch) and the batch axis is W: a word
attends to the word with the same index on the other pages, not to the words of its own page.  Checkpoints of the reference were trained
that way; this module reproduces it (attention = W * 4 independent problems of sequence length N per layer).

Arithmetic
  * all storage fp32 (train_layout.py runs without autocast).  Linear layers: exact-fp32 MFMA by default (parity mode); split-bf16 x3
    (``ocrs_gemm_x3[p]`` / ``ocrs_wgrad_gemm_x3``, fp32-class) when called under ``torch.autocast("cuda", dtype=torch.bfloat16)``.
    Embedding, attention, LayerNorm and the loss are exact fp32 in both.
  * dropout (``model.dropout_p``, default 0.1 = torch's default the reference inherits; four sites per layer) is counter-based: the seed of a
    step is drawn from torch's CPU generator (``torch.manual_seed`` fixes a run), masks are regenerated in the backward.  Eval mode and
    ``dropout_p = 0`` skip it.
"""
from __future__ import annotations

import warnings

import torch
from torch import nn

from ._lib import lib, ptr
from .models import _check_versions
from .packs import EMPTY as EMPTY_PACKS, cached_table, dgrad_row, fwd_row

D_MODEL, N_HEADS, D_FF, N_LAYERS, N_CLASSES = 256, 4, 1024, 6, 2
LDL = 32  # row pitch of the padded classify output / gradient (the GEMM entry points want K % 32 == 0)
MAX_SEQ = 128
SITE_ATTN, SITE_PROJ, SITE_RELU, SITE_FF = 0, 1, 2, 3


def site_code(layer: int, site: int) -> int:
    """the `site` argument of the dropout-aware entry points (include/ocrs_hip.h)"""
    return 4 * layer + site


def angle_rates() -> torch.Tensor:
    """The 32 angle rates of positional_encoding(length, 64), by the reference's own fp32 expression (models.py:286-292)."""
    depth = 32
    depths = torch.arange(depth).unsqueeze(0) / depth
    return (1 / (10_000**depths)).reshape(depth).contiguous()


_rates_cache: dict = {}
_loss_ws_cache: dict = {}


def _rates(dev):
    t = _rates_cache.get(dev)
    if t is None:
        t = _rates_cache[dev] = angle_rates().to(dev)
    return t


def encode_bbox_positions_aten(boxes: torch.Tensor) -> torch.Tensor:
    """encode_bbox_positions(boxes, 64) (models.py:298-318) per element instead of through a table of max_coord + 1 rows: the same bits on
    the CPU, no data-dependent shape (and no host synchronisation).  Stock ATen operators only (export.AtenGraph uses it)."""
    N, W, D = boxes.shape
    pos = boxes.round().int().to(torch.float32).unsqueeze(-1)
    ang = pos * angle_rates().to(boxes.device)
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(N, W, D * 64)


class SinPositionalEncoding(nn.Module):
    """models.py:321-337 (parameter-free)."""

    def __init__(self, d_model: int):
        super().__init__()
        self.d_model = d_model

    def forward(self, boxes):
        return encode_bbox_positions_aten(boxes)


_ORDER = ["classify."] + [f"encode.layers.{i}.{part}" for i in reversed(range(N_LAYERS))
                          for part in ("norm2.", "linear2.", "linear1.", "norm1.", "self_attn.out_proj.", "self_attn.in_proj_")]


class _LayoutRun:
    packs = EMPTY_PACKS  # this step's weight-fragment packs (prepack)

    def __init__(self, mod, boxes, names, params, train, x3, p_drop, seed):
        self.L = lib()
        self.mod = mod
        self.names = names
        self.P = dict(zip(names, params))
        self.train = train
        self.x3 = x3
        self.dev = boxes.device
        self.boxes = boxes
        self.N, self.W = boxes.shape[0], boxes.shape[1]
        self.R = self.N * self.W
        self.p = float(p_drop) if train else 0.0
        self.seed = seed
        self.frag = (1, 2) if x3 else (0, 0)  # (fragment dtype, pack mode): pre-split hi / lo bf16 planes for the pipelined x3 GEMM, or exact fp32

    def empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    # ---- weights ------------------------------------------------------------------------------------------------------
    def _linear_names(self):
        out = []
        for i in range(N_LAYERS):
            pre = f"encode.layers.{i}."
            out += [pre + "self_attn.in_proj_weight", pre + "self_attn.out_proj.weight", pre + "linear1.weight", pre + "linear2.weight"]
        return out

    def pack_rows(self, need_dgrad):
        """A[m][k] = W[m][k] for the forward, A[m][k] = W[k][m] for the input gradients (layer 0's in_proj has none: the embedding has no
        parameters).  classify (2 x 256) is packed in parity mode only; in x3 mode it runs on ocrs_gemm_x3 from the master layout."""
        rows = []
        for n in self._linear_names() + ([] if self.x3 else ["classify.weight"]):
            rows.append(fwd_row(self.P[n], *self.frag))
            if need_dgrad and not n.startswith("encode.layers.0.self_attn.in_proj"):
                rows.append(dgrad_row(self.P[n], *self.frag))
        return rows

    def prepack(self, need_dgrad):
        """All weight-fragment packs of the step in one launch (packs.py); the table is cached while the parameters stay put."""
        key = (self.frag, need_dgrad, tuple(p.data_ptr() for p in self.P.values()))
        self.packs = cached_table(self.mod, key, lambda: self.pack_rows(need_dgrad), self.dev)
        self.packs.launch()

    def linear(self, x, ldx, w, bias, relu=False, ldo=None):
        """out [R][ldo] = x [R][K] @ w[M][K]^T + bias"""
        L, R = self.L, self.R
        M, K = w.shape
        ldo = ldo or M
        out = self.empty(R, ldo)
        row = fwd_row(w, *self.frag)
        if self.x3:
            wpk = self.packs.get(row)
            if wpk is not None and L.gemm_x3p_supported(ldx, K, ldo, M, R):
                L.gemm_x3p(ptr(x), ldx, K, ptr(wpk), ptr(bias), ptr(out), ldo, M, R)
            else:
                L.gemm_x3(ptr(x), ldx, K, ptr(w), K, 0, ptr(bias), ptr(out), ldo, M, R, 0)
            return out, False
        L.conv_igemm(ptr(x), ldx, ptr(self.packs[row]), ptr(out), ldo, ptr(bias), 1 if relu else 0, None, K, M, 1, 1, R, 1, R, 1, 1, 0, 0, 0)
        return out, relu

    def linear_dgrad(self, g, ldg, w):
        """dx [R][K] = g [R][ldg] (first M columns; the others zero) @ w[M][K]"""
        L, R = self.L, self.R
        M, K = w.shape
        out = self.empty(R, K)
        row = dgrad_row(w, *self.frag)
        if self.x3:
            wpk = self.packs.get(row)
            if wpk is not None and ldg == M and L.gemm_x3p_supported(ldg, M, K, K, R):
                L.gemm_x3p(ptr(g), ldg, M, ptr(wpk), None, ptr(out), K, K, R)
            else:
                L.gemm_x3(ptr(g), ldg, ldg, ptr(w), K, 1, None, ptr(out), K, K, R, M if M != ldg else 0)
            return out
        L.conv_igemm(ptr(g), ldg, ptr(self.packs[row]), ptr(out), K, None, 0, None, ldg, K, 1, 1, R, 1, R, 1, 1, 0, 0, 0)
        return out

    def wgrad(self, g, ldg, M, x, K, dW):
        """dW [M][K] += g^T x: deterministic two-stage reductions (workspace from the caching allocator)"""
        L, R = self.L, self.R
        if self.x3:
            ws = self.empty(L.wgrad_gemm_x3_ws_floats(M, K, R))
            L.wgrad_gemm_x3(ptr(g), ldg, M, ptr(x), K, K, ptr(dW), ptr(ws), R)
        else:
            ws = self.empty(L.wgrad_gather_ws_floats(M, K, 1, R, 0))
            L.wgrad_gather(ptr(g), ldg, M, None, ptr(x), K, K, ptr(dW), ptr(ws), 1, 1, R, 1, R, 1, 0, 0, 1, 1, 0)

    def bias_grad(self, g, ldg, C, db):
        L = self.L
        Cr = (C + 3) // 4 * 4
        ws = self.empty(L.layout_col_sum_ws_floats(Cr, self.R))
        L.layout_col_sum(ptr(g), ldg, Cr, C, ptr(db), ptr(ws), self.R)

    # ---- forward ------------------------------------------------------------------------------------------------------
    def forward(self):
        L, P, R, N, W, p, seed = self.L, self.P, self.R, self.N, self.W, self.p, self.seed
        if not L.layout_attn_supported(N):
            raise RuntimeError(f"LayoutModel: the batch size is the attention sequence length (batch_first=False, models.py:385-388) and the fused "
                               f"attention kernel covers 1 <= N <= {MAX_SEQ}; got N = {N}")
        if W > 65535:
            raise RuntimeError(f"LayoutModel: at most 65535 words per page, got {W}")
        self.prepack(self.train)
        x = self.empty(R, D_MODEL)
        L.layout_embed(ptr(self.boxes), ptr(_rates(self.dev)), ptr(x), R)
        self.acts = []
        for i in range(N_LAYERS):
            pre = f"encode.layers.{i}."
            qkv, _ = self.linear(x, D_MODEL, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"])
            att = self.empty(R, D_MODEL)
            L.layout_attn_fwd(ptr(qkv), ptr(att), N, W, p, seed, site_code(i, SITE_ATTN))
            a, _ = self.linear(att, D_MODEL, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"])
            x1 = self.empty(R, D_MODEL)
            st1 = self.empty(R, 2) if self.train else None
            L.layout_ln_fwd(ptr(x), ptr(a), ptr(P[pre + "norm1.weight"]), ptr(P[pre + "norm1.bias"]), ptr(x1), ptr(st1), R, 1e-5, p, seed,
                            site_code(i, SITE_PROJ))
            h, relu_done = self.linear(x1, D_MODEL, P[pre + "linear1.weight"], P[pre + "linear1.bias"], relu=True)
            if not relu_done or p > 0:
                L.layout_relu_drop_fwd(ptr(h), R * D_FF, 0 if relu_done else 1, p, seed, site_code(i, SITE_RELU))
            f, _ = self.linear(h, D_FF, P[pre + "linear2.weight"], P[pre + "linear2.bias"])
            x2 = self.empty(R, D_MODEL)
            st2 = self.empty(R, 2) if self.train else None
            L.layout_ln_fwd(ptr(x1), ptr(f), ptr(P[pre + "norm2.weight"]), ptr(P[pre + "norm2.bias"]), ptr(x2), ptr(st2), R, 1e-5, p, seed,
                            site_code(i, SITE_FF))
            if self.train:
                self.acts.append(dict(x=x, qkv=qkv, att=att, a=a, x1=x1, st1=st1, h=h, f=f, st2=st2))
            x = x2
        self.xf = x if self.train else None
        logits, _ = self.linear(x, D_MODEL, P["classify.weight"], P["classify.bias"], ldo=LDL)
        out = self.empty(N, W, N_CLASSES)
        L.layout_head_out(ptr(logits), LDL, ptr(out), R, 1 if self.mod.return_probs else 0)
        self.out = out if (self.train and self.mod.return_probs) else None
        return out

    # ---- backward -----------------------------------------------------------------------------------------------------
    def backward(self, g):
        L, P, R, N, W, p, seed = self.L, self.P, self.R, self.N, self.W, self.p, self.seed
        # flat gradient buffer in backward-completion order, as the other two models keep it (data-parallel buckets = contiguous ranges)
        flat = torch.zeros(sum(q.numel() for q in P.values()), dtype=torch.float32, device=self.dev)
        G, off, stage_end = {}, 0, {}
        for stage in _ORDER:
            for k in self.names:
                if k.startswith(stage) and k not in G:
                    n = P[k].numel()
                    G[k] = flat[off:off + n].view_as(P[k])
                    off += n
            stage_end[stage] = off
        assert off == flat.numel(), "parameter ordering table is incomplete"
        bucketer = getattr(self.mod, "_grad_bucketer", None)
        done = [0]

        def stage_done(stage):
            # called behind the stage's last gradient launch: every launch writes its own outputs (k_lay_colsum owns its partials, no deferral
            # window), so the range is final in stream order and a data-parallel bucket may go out
            if bucketer is not None and stage_end[stage] > done[0]:
                bucketer.ready(flat, done[0], stage_end[stage])
            done[0] = max(done[0], stage_end[stage])
        g = g.contiguous().float()
        if self.out is not None:  # return_probs: d sigmoid
            g = g * self.out * (1 - self.out)
        dlog = self.empty(R, LDL)
        L.layout_head_grad_in(ptr(g), ptr(dlog), LDL, R)
        self.wgrad(dlog, LDL, N_CLASSES, self.xf, D_MODEL, G["classify.weight"])
        self.bias_grad(dlog, LDL, N_CLASSES, G["classify.bias"])
        stage_done("classify.")
        dy1, dy2 = self.linear_dgrad(dlog, LDL, P["classify.weight"]), None
        self.xf = None
        lnws = self.empty(L.layout_ln_bwd_ws_floats(R))
        for i in reversed(range(N_LAYERS)):
            pre = f"encode.layers.{i}."
            A = self.acts.pop()
            ds2 = self.empty(R, D_MODEL)
            df = self.empty(R, D_MODEL) if p > 0 else ds2
            L.layout_ln_bwd(ptr(dy1), ptr(dy2), ptr(A["x1"]), ptr(A["f"]), ptr(A["st2"]), ptr(P[pre + "norm2.weight"]), ptr(ds2),
                            ptr(df) if p > 0 else None, ptr(G[pre + "norm2.weight"]), ptr(G[pre + "norm2.bias"]), ptr(lnws), R, p, seed,
                            site_code(i, SITE_FF))
            stage_done(pre + "norm2.")
            self.wgrad(df, D_MODEL, D_MODEL, A["h"], D_FF, G[pre + "linear2.weight"])
            self.bias_grad(df, D_MODEL, D_MODEL, G[pre + "linear2.bias"])
            stage_done(pre + "linear2.")
            dh = self.linear_dgrad(df, D_MODEL, P[pre + "linear2.weight"])
            L.layout_relu_drop_bwd(ptr(dh), ptr(A["h"]), ptr(dh), R * D_FF, p)
            self.wgrad(dh, D_FF, D_FF, A["x1"], D_MODEL, G[pre + "linear1.weight"])
            self.bias_grad(dh, D_FF, D_FF, G[pre + "linear1.bias"])
            stage_done(pre + "linear1.")
            dx1 = self.linear_dgrad(dh, D_FF, P[pre + "linear1.weight"])
            ds1 = self.empty(R, D_MODEL)
            da = self.empty(R, D_MODEL) if p > 0 else ds1
            L.layout_ln_bwd(ptr(ds2), ptr(dx1), ptr(A["x"]), ptr(A["a"]), ptr(A["st1"]), ptr(P[pre + "norm1.weight"]), ptr(ds1),
                            ptr(da) if p > 0 else None, ptr(G[pre + "norm1.weight"]), ptr(G[pre + "norm1.bias"]), ptr(lnws), R, p, seed,
                            site_code(i, SITE_PROJ))
            stage_done(pre + "norm1.")
            self.wgrad(da, D_MODEL, D_MODEL, A["att"], D_MODEL, G[pre + "self_attn.out_proj.weight"])
            self.bias_grad(da, D_MODEL, D_MODEL, G[pre + "self_attn.out_proj.bias"])
            stage_done(pre + "self_attn.out_proj.")
            datt = self.linear_dgrad(da, D_MODEL, P[pre + "self_attn.out_proj.weight"])
            dqkv = self.empty(R, 3 * D_MODEL)
            L.layout_attn_bwd(ptr(A["qkv"]), ptr(datt), ptr(dqkv), N, W, p, seed, site_code(i, SITE_ATTN))
            self.wgrad(dqkv, 3 * D_MODEL, 3 * D_MODEL, A["x"], D_MODEL, G[pre + "self_attn.in_proj_weight"])
            self.bias_grad(dqkv, 3 * D_MODEL, 3 * D_MODEL, G[pre + "self_attn.in_proj_bias"])
            stage_done(pre + "self_attn.in_proj_")
            if i > 0:  # (the embedding has no parameters and the boxes need no gradient)
                dy1, dy2 = ds1, self.linear_dgrad(dqkv, 3 * D_MODEL, P[pre + "self_attn.in_proj_weight"])
        if bucketer is not None:
            bucketer.finish(flat)
        self.flat = flat
        return [G[k] for k in self.names]


class _LayoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boxes, mod, names, x3, p_drop, seed, *params):
        run = _LayoutRun(mod, boxes, names, [q.detach() for q in params], mod.training, x3, p_drop, seed)
        ctx.run = run
        ctx.params = params
        ctx.versions = [q._version for q in params]
        return run.forward()

    @staticmethod
    def backward(ctx, g):
        _check_versions(ctx)
        grads = ctx.run.backward(g)
        ctx.run = None  # free the saved activations
        return (None, None, None, None, None, None, *grads)


class LayoutModel(nn.Module):
    """Text layout analysis model (reference: ocrs_models/models.py:340-406).

    ``forward(x: (N, W, 4)) -> (N, W, 2)`` logits (or probabilities with ``return_probs=True``) for ``[line_start, line_end]``.
    Preconditions: box coordinates are >= 0 (the reference's dataset asserts it; its table lookup would fail otherwise) and below 2^24;
    1 <= N <= 128 (N is the attention sequence length, see the module docstring).  ``dropout_p`` (default 0.1) is the dropout probability of all
    four sites of every encoder layer in training mode.
    """

    last_seed = None  # the dropout seed of the latest training forward (tests fetch the masks the kernels used through it)

    def __init__(self, return_probs=False, pos_embedding="sin"):
        super().__init__()
        self.d_embed = D_MODEL
        self.return_probs = return_probs
        if pos_embedding == "mlp":
            raise NotImplementedError('LayoutModel(pos_embedding="mlp") is not built: only the "sin" encoding the reference trains with runs on the '
                                      'HIP path')
        if pos_embedding != "sin":
            raise ValueError(f"unknown pos_embedding {pos_embedding!r}")
        self.embed = SinPositionalEncoding(D_MODEL)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (torch's note that nested tensors need batch_first=True)
            layer = nn.TransformerEncoderLayer(d_model=D_MODEL, nhead=N_HEADS, dim_feedforward=D_FF)
            self.encode = nn.TransformerEncoder(layer, num_layers=N_LAYERS)
        self.classify = nn.Linear(D_MODEL, N_CLASSES)
        self.dropout_p = 0.1

    @staticmethod
    def _x3():
        return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("ocrs_models_amd.LayoutModel runs on MI355X only (no CPU path); move the model and input to 'cuda'")
        if x.dim() != 3 or x.shape[2] != 4 or x.shape[0] < 1 or x.shape[1] < 1:
            raise RuntimeError(f"expected (N, W, 4) word boxes, got {tuple(x.shape)}")
        lib()
        x = x.contiguous().float()
        names = [n for n, _ in self.named_parameters()]
        params = [q for _, q in self.named_parameters()]
        for q in params:
            if q.dtype != torch.float32 or not q.is_contiguous() or not q.is_cuda:
                raise RuntimeError("parameters must be contiguous fp32 CUDA tensors")
        p = float(self.dropout_p) if self.training else 0.0
        if not 0.0 <= p < 1.0:
            raise RuntimeError(f"dropout_p must be in [0, 1), got {p}")
        seed = 0
        if p > 0:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())  # CPU generator: no device synchronisation
            self.last_seed = seed
        x3 = self._x3()
        with torch.autocast("cuda", enabled=False):
            if torch.is_grad_enabled() and any(q.requires_grad for q in params):
                return _LayoutFn.apply(x, self, names, x3, p, seed, *params)
            return _LayoutRun(self, x, names, [q.detach() for q in params], self.training, x3, p, seed).forward()


def dropout_mask(shape, p: float, seed: int, layer: int, site: int, device="cuda") -> torch.Tensor:
    """The uint8 keep-mask (1 = kept) a kernel used at (layer, site) for a step's seed, in the site's element order: SITE_ATTN
    (W * 4, N, N) = (word * 4 + head, query, key); SITE_PROJ / SITE_FF (N * W, 256); SITE_RELU (N * W, 1024)."""
    mask = torch.empty(shape, dtype=torch.uint8, device=device)
    lib().layout_dropout_mask(ptr(mask), mask.numel(), float(p), int(seed), site_code(layer, site))
    return mask


def loss_workspace(dev):
    """the loss launch's workspace (arrival counter + per-workgroup partials), zeroed once per device"""
    ws = _loss_ws_cache.get(dev)
    if ws is None:
        ws = _loss_ws_cache[dev] = torch.zeros(lib().layout_loss_ws_bytes(), dtype=torch.uint8, device=dev)
    return ws
