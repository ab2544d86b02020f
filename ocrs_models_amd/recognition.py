"""RecognitionModel (CRNN: conv backbone -> 2-layer BiGRU -> Linear + LogSoftmax) with the reference's constructor /
forward signature and state-dict keys (ocrs_models/models.py:146-268), executed by the gfx950 kernels of libocrs_hip.so.

Layout / dtype policy
  * conv activations NHWC, fp32 or bf16 (bf16 when called under ``torch.autocast(dtype=torch.bfloat16)`` like
    train_rec.py:118 does, or with ``act_dtype=torch.bfloat16``); MFMA accumulation, BatchNorm statistics fp32.
  * the GRU always runs in fp32 (models.py:264-266), on exact-fp32 MFMA; so do the Linear and LogSoftmax here.
  * output: log-probs (W//4 + 1, B, n_classes) fp32.
"""
from __future__ import annotations

import math

import os

import torch
from torch import nn

from ._lib import DT, lib, ptr
from .models import _check_versions, _identity_tr
from .packs import EMPTY as EMPTY_PACKS, PackRow, cached_table, conv_dgrad_row, conv_row, dgrad_row, fwd_row

_coef_cache: dict = {}


def _unit_coef(C, device):
    key = (C, device)
    t = _coef_cache.get(key)
    if t is None:
        t = torch.zeros(3, C, dtype=torch.float32, device=device)
        t[0] = 1.0
        _coef_cache[key] = t
    return t


class _GruRec:
    """What a GRU layer's backward needs from its forward (both directions stacked; x: the layer's input [T][N][I])."""

    __slots__ = ("layer", "x", "I", "w_ih", "w_hh", "out", "saved")

    def __init__(self, layer, x, I, w_ih, w_hh, out, saved):
        self.layer, self.x, self.I, self.w_ih, self.w_hh, self.out, self.saved = layer, x, I, w_ih, w_hh, out, saved


class _RecRun:
    """One forward (and later backward) pass of the recognition network on the current stream."""

    # per-pass state, declared here with its value between passes (immutable defaults: a run the op tests drive stage by stage reads them too):
    packs = EMPTY_PACKS  # this step's weight-fragment packs (prepack); empty outside a full forward
    _arena, _arena_off = None, 0  # the fp64 accumulator arena (stat)
    _side, _keep = None, ()  # inside backward(): the side stream (None: single stream) and the tensors its launches still read (on_side)
    G = None  # inside backward(): gradient views by parameter name

    def __init__(self, P, Bf, dev, dtype, N, H, W, train=True, mod=None, x=None):
        """P / Bf: parameters / buffers by state-dict name (P in the module's parameter order); mod / x: the module and the input crops of a
        whole-network pass (forward / backward need them; the op tests drive single stages without)."""
        self.L = lib()
        self.P, self.Bf, self.names = P, Bf, list(P)
        self.dev, self.dtype, self.dt, self.N, self.H, self.W, self.train = dev, dtype, DT[dtype], N, H, W, train
        self.mod, self.x = mod, x
        # split-bf16 GEMMs for the fp32 GRU weight gradients in throughput mode, the projections on the pipelined kernel (rec_gemm.hip)
        self.x3 = os.environ.get("OCRS_GRU_X3", "1") != "0"
        # recurrence as one persistent launch per layer and pass (csrc/rec_gru_seq.hip) when all its workgroups can be resident; its matrix
        # products follow the projection GEMMs' arithmetic: exact fp32 MFMA in parity mode, split-bf16 x3 in throughput mode
        self.gru_seq = bool(self.L.gru_seq_supported(N)) and not _GRU_SEQ_OFF.get(dev, False)
        self.gru_exact = 0 if self.dt == 1 and self.x3 else 1

    @property
    def ncls(self):
        return self.P["output.0.weight"].shape[0]

    # ---- helpers -------------------------------------------------------------------------------
    def empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.dev)

    def seq_sync(self):
        """arrival counters (zeroed by the entry point) and exchange workspace of one persistent GRU launch"""
        nsync, nws = self.L.gru_seq_sync_words(self.N), self.L.gru_seq_ws_floats(self.N)
        buf = torch.empty(nsync + nws, dtype=torch.int32, device=self.dev)  # one allocation: the entry point initialises both with one fill
        return buf[:nsync], buf[nsync:].view(torch.float32)

    def stat(self, C):
        """zeroed fp64 [2][C] accumulator (BatchNorm batch sums / their backward counterparts): a slice of ONE zero-filled arena per step"""
        n = 2 * C
        if self._arena is None or self._arena_off + n > self._arena.numel():
            self._arena = torch.zeros(2 * 2 * (64 + 3 * 128), dtype=torch.float64, device=self.dev)
            self._arena_off = 0
        self._arena_off += n
        return self._arena[self._arena_off - n:self._arena_off]

    def on_side(self, fn, *keep):
        """fn() on the backward's side stream, behind what the caller's stream holds so far; `keep` (fn's operands) and the workspace fn may
        return stay referenced until the caller's stream has waited for the side stream.  Single stream: just fn()."""
        if self._side is None:
            return fn()
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            out = fn()
        self._keep.extend(keep if out is None else (*keep, out))
        return out

    def pack(self, src, K, M, K2, s1, s2, sm, dt=None, offset=0):
        """MFMA weight fragments of one layout: from this step's multi-pack buffer (prepack) or, when the table does not hold it, packed here."""
        return self.packs.fetch(PackRow(src, self.dt if dt is None else dt, 0, K, M, K2, s1, s2, sm, offset), self.dev)

    _CONVS = ("conv.3.weight", "conv.7.weight", "conv.9.weight", "conv.13.weight", "conv.15.weight", "conv.19.weight")

    def pack_rows(self):
        """The packs of a step: the conv layers (forward + input-gradient layouts) in the activation dtype, and the Linear layers of the mode."""
        P, rows = self.P, []
        for name in self._CONVS:
            rows.append(conv_row(P[name], self.dt))
            if self.train:
                rows.append(conv_dgrad_row(P[name], self.dt))
        wout = P["output.0.weight"]
        if not self.use_x3(512, self.ncls, 0):
            # parity mode: the output layer in both layouts, exact fp32 (the GRU projection weights are NOT here: linear() packs them with
            # one ocrs_pack_frags each per step)
            rows.append(fwd_row(wout, 0))
            if self.train:
                rows.append(dgrad_row(wout, 0))
        else:
            # throughput mode, pipelined split-bf16 GEMM (csrc/rec_gemm.hip): the GRU input-projection weights pre-split into hi / lo bf16
            # fragment planes (pack mode 2), forward and -- training -- input-gradient layouts; the output layer's input gradient likewise
            # (its forward has a ragged M = n_classes and stays on k_gemm_x3, straight from the master layout)
            for layer in (0, 1):
                w_ih = RecognitionModel._gru_stacked(layer, P)[0]
                rows.append(fwd_row(w_ih, 1, 2))
                if self.train:
                    rows.append(dgrad_row(w_ih, 1, 2))
            if self.train:
                rows.append(dgrad_row(wout, 1, 2))
        return rows

    def prepack(self):
        """All weight-fragment packs of the step in one launch per fragment dtype (packs.py); the table is built once per module / mode and
        reused while the parameter storage stays in place."""
        key = (self.dt, self.train, self.x3, tuple(p.data_ptr() for p in self.P.values()))
        self.packs = cached_table(self.mod, key, self.pack_rows, self.dev)
        self.packs.launch()

    def bn(self, prefix, gstat, count, C, lo):
        P, Bf = self.P, self.Bf
        tr = self.empty(3, C, dtype=torch.float32)
        saved = self.empty(2, C, dtype=torch.float32)
        if self.train:
            self.L.bn_finalize(ptr(gstat), count, C, ptr(P[f"{prefix}.weight"]), ptr(P[f"{prefix}.bias"]), 1e-5, 0.1, ptr(tr), ptr(saved),
                               ptr(Bf[f"{prefix}.running_mean"]), ptr(Bf[f"{prefix}.running_var"]), ptr(Bf[f"{prefix}.num_batches_tracked"]), lo)
        else:
            rstd = torch.rsqrt(Bf[f"{prefix}.running_var"] + 1e-5)
            tr[0] = P[f"{prefix}.weight"] * rstd
            tr[1] = P[f"{prefix}.bias"] - Bf[f"{prefix}.running_mean"] * tr[0]
            tr[2] = lo
        return tr, saved

    def conv(self, x, w, bias, relu, stats, Hi, Wi, pad, Ho=None, Wo=None):
        co, ci, kh, kw = w.shape
        Ho, Wo = Ho or Hi, Wo or Wi
        out = self.empty(self.N, Ho, Wo, co)
        gstat = self.stat(co) if stats else None
        wpk = self.packs.fetch(conv_row(w, self.dt), self.dev)
        self.L.conv_igemm(ptr(x), ci, ptr(wpk), ptr(out), co, ptr(bias), 1 if relu else 0, ptr(gstat), ci, co, self.N, Hi, Wi, Ho, Wo, kh, kw, pad, pad,
                          self.dt)
        return out, gstat

    def use_x3(self, K, M, km=1):
        return self.dt == 1 and self.x3 and K % 32 == 0 and (M % 4 == 0 or not km)

    def gemm(self, x, ldx, K, wpk, bias, M, ldo, rows):
        """fp32 GEMM: out[rows][ldo] = x[rows][K] @ W^T (+bias), W given as packed fragments (K, M)."""
        out = self.empty(rows, ldo, dtype=torch.float32)
        self.L.conv_igemm(ptr(x), ldx, ptr(wpk), ptr(out), ldo, ptr(bias), 0, None, K, M, 1, 1, rows, 1, rows, 1, 1, 0, 0, 0)
        return out

    def linear(self, x, ldx, K, w, ldw, km, bias, M, ldo, rows, kw=0):
        """fp32 out[rows][ldo] = x[rows][K] @ A^T (+ bias) with A[m][k] = w[m][k] (km = 0) or w[k][m] (km = 1), w's row pitch ldw; kw (0: K):
        the k extent w really has -- x's columns [kw, K) are zero.  w is the whole matrix: its shape says the same as (M, kw or K, ldw).  The one place that picks the kernel: throughput mode runs split-bf16
        (csrc/rec_gemm.hip::k_gemm_x3), on the pipelined kernel where this step's prepack pre-split the weight and the shape is taken, else
        straight from the master layout; parity mode runs exact fp32 on packed fragments."""
        L = self.L
        assert (M, kw or K, ldw) == ((w.shape[1], w.shape[0]) if km else tuple(w.shape)) + (w.shape[1],)  # (the packed routes read w.shape)
        row_of = dgrad_row if km else fwd_row
        if not self.use_x3(K, M, km):
            return self.gemm(x, ldx, K, self.packs.fetch(row_of(w, 0), self.dev), bias, M, ldo, rows)
        out = self.empty(rows, ldo, dtype=torch.float32)
        wpk = self.packs.get(row_of(w, 1, 2))
        if wpk is not None and L.gemm_x3p_supported(ldx, K, ldo, M, rows):
            L.gemm_x3p(ptr(x), ldx, K, ptr(wpk), ptr(bias), ptr(out), ldo, M, rows)
        else:
            L.gemm_x3(ptr(x), ldx, K, ptr(w), ldw, km, ptr(bias), ptr(out), ldo, M, rows, kw)
        return out

    # ---- forward -------------------------------------------------------------------------------
    def forward(self):
        L, P, N, H, W = self.L, self.P, self.N, self.H, self.W
        if H != 64:
            raise RuntimeError(f"RecognitionModel expects input height 64 (models.py:153), got {H}")
        if W < 4:
            raise RuntimeError(f"input width must be at least 4 (two floor-mode 2x2 max-pools, models.py:187,199), got {W}")
        # any width: nn.MaxPool2d floors (the last odd column is in no window), exactly as the kernels' W // 2 -> W // 4 below
        S = self
        self.prepack()
        S.a0 = self.empty(N, 32, W // 2, 32)
        L.conv0_fwd(ptr(self.x), ptr(P["conv.0.weight"]), ptr(P["conv.0.bias"]), ptr(S.a0), N, H, W, self.dt)
        H1, W1 = 32, W // 2
        S.z3, gs = self.conv(S.a0, P["conv.3.weight"], None, False, True, H1, W1, 1)
        S.tr3, S.sv3 = self.bn("conv.4", gs, N * H1 * W1, 64, 0.0)
        H2, W2 = 16, W // 4
        S.a3 = self.empty(N, H2, W2, 64)
        L.act_pool_fwd(ptr(S.z3), ptr(S.tr3), ptr(S.a3), 64, N, H1, W1, 2, 2, self.dt)
        S.a7, _ = self.conv(S.a3, P["conv.7.weight"], P["conv.7.bias"], True, False, H2, W2, 1)
        S.z9, gs = self.conv(S.a7, P["conv.9.weight"], None, False, True, H2, W2, 1)
        S.tr9, S.sv9 = self.bn("conv.10", gs, N * H2 * W2, 128, 0.0)
        S.a9 = self.empty(N, 8, W2, 128)
        L.act_pool_fwd(ptr(S.z9), ptr(S.tr9), ptr(S.a9), 128, N, H2, W2, 2, 1, self.dt)
        S.a13, _ = self.conv(S.a9, P["conv.13.weight"], P["conv.13.bias"], True, False, 8, W2, 1)
        S.z15, gs = self.conv(S.a13, P["conv.15.weight"], None, False, True, 8, W2, 1)
        S.tr15, S.sv15 = self.bn("conv.16", gs, N * 8 * W2, 128, 0.0)
        S.a15 = self.empty(N, 4, W2, 128)
        L.act_pool_fwd(ptr(S.z15), ptr(S.tr15), ptr(S.a15), 128, N, 8, W2, 2, 1, self.dt)
        T = W2 + 1
        S.z19, gs = self.conv(S.a15, P["conv.19.weight"], None, False, True, 4, W2, 1, Ho=5, Wo=T)
        S.tr19, S.sv19 = self.bn("conv.20", gs, N * 5 * T, 128, -math.inf)
        S.seq = self.empty(T, N, 128, dtype=torch.float32)
        L.avgpool_fwd(ptr(S.z19), ptr(S.tr19), ptr(S.seq), 128, N, 5, T, self.dt)
        S.T, S.W2 = T, W2
        # ---- 2-layer bidirectional GRU, fp32 ----
        rows = T * N
        S.gru = []
        xin, I = S.seq, 128
        for layer in (0, 1):
            w_ih, w_hh, b_ih, b_hh = RecognitionModel._gru_stacked(layer, P)  # (1536, I), (2, 768, 256), (1536,), (1536,): both directions
            gi = self.linear(xin, I, I, w_ih, I, 0, b_ih, 1536, 1536, rows)  # W_ih [1536][I]
            out = self.empty(T, N, 512, dtype=torch.float32)
            saved = self.empty(T, N, 2, 4, 256, dtype=torch.float32) if self.train else None
            if self.gru_seq:
                sync, xws = self.seq_sync()  # (kept alive across the call: a temporary would be freed -- and its block re-used -- before the launch)
                L.gru_seq_fwd(ptr(gi), ptr(w_hh), ptr(b_hh), ptr(out), ptr(saved), T, N, ptr(sync), ptr(_gru_err(self.dev)), ptr(xws), self.gru_exact)
            else:
                nfl = 8 * 48 * 64 * 8
                whh_pk = torch.empty(2 * nfl, dtype=torch.float32, device=self.dev)
                for d in (0, 1):
                    L.pack_frags(w_hh.data_ptr() + 4 * d * 768 * 256, 0, 256, 768, 256, 0, 1, 256, whh_pk.data_ptr() + 4 * d * nfl, 0)
                L.gru_layer_fwd(ptr(gi), ptr(whh_pk), ptr(b_hh), ptr(out), ptr(saved), T, N)
            S.gru.append(_GruRec(layer, xin, I, w_ih, w_hh, out, saved))
            xin, I = out, 512
        # ---- Linear + LogSoftmax (fp32) ----
        C = self.ncls
        S.ldl = (C + 31) // 32 * 32
        logits = self.linear(xin, 512, 512, P["output.0.weight"], 512, 0, P["output.0.bias"], C, S.ldl, rows)
        S.lp = self.empty(T, N, C, dtype=torch.float32)
        L.log_softmax_fwd(ptr(logits), ptr(S.lp), rows, C, S.ldl, 0)
        return S.lp

    # ---- backward ------------------------------------------------------------------------------
    def conv_bwd(self, name, dz, xin, Hz, Wz, Hx, Wx, pad, need_dx=True):
        """dz: gradient w.r.t. the conv output [N][Hz][Wz][Cout]; accumulates dW, returns dx [N][Hx][Wx][Cin]."""
        L, w = self.L, self.P[name]
        co, ci, kh, kw = w.shape

        def wgrad_now():
            if kh == 3 and kw == 3 and pad == 1 and co <= 128:
                ws = self.empty(L.conv3x3_wgrad_ws_floats(co, ci, self.N, Hz, Wz), dtype=torch.float32)
                L.conv3x3_wgrad(ptr(dz), co, ptr(xin), ci, ptr(self.G[name]), ptr(ws), self.N, Hz, Wz, self.dt)
                return ws
            self.wgrad(dz, co, co, xin, ci, ci, self.G[name], self.N, Hz, Wz, Hx, Wx, pad, pad, kh, kw, self.dt)
            return None
        if not need_dx:
            wgrad_now()
            return None
        # The weight gradient hangs off dz and nothing downstream in the backward reads it: it runs on the side stream next to the dgrad and the
        # HBM-bound BatchNorm / pooling backward kernels of the next layer (matrix-core work next to streaming work).  Its operands and workspace
        # stay referenced until the main stream has waited for the side stream (end of the backward, or the DDP stage report).
        self.on_side(wgrad_now, dz, xin)
        dx = self.empty(self.N, Hx, Wx, ci)
        L.conv_igemm(ptr(dz), co, ptr(self.packs.fetch(conv_dgrad_row(w, self.dt), self.dev)), ptr(dx), ci, None, 0, None, co, ci, self.N, Hz, Wz, Hx, Wx, kh, kw,
                     kh - 1 - pad, kw - 1 - pad, self.dt)
        return dx

    def wgrad(self, A, ldA, CA, B, ldB, CB, dW, N, hA, wA, HB, WB, padh, padw, KH, KW, dt):
        """dW += A^T (gathered) B with the deterministic two-stage flush (workspace from the caching allocator)."""
        L = self.L
        a_ptr = A if isinstance(A, int) else ptr(A)
        b_ptr = B if isinstance(B, int) else ptr(B)
        if (dt == 0 and self.dt == 1 and self.x3 and KH * KW == 1 and padw == 0 and N == 1 and (hA, wA) == (HB, WB) and ldA >= (CA + 3) // 4 * 4
                and CB % 4 == 0 and ldA % 4 == 0 and ldB % 4 == 0):
            # throughput (autocast) mode: the fp32 GRU weight gradients as split-bf16 (bf16x3) GEMMs -- ~1e-5 relative per product, fp32
            # accumulation; parity mode (self.dt == 0) keeps the exact-fp32 MFMA kernel.
            # A row (t, n) pairs with B row (t - padh, n) (the h_{t-1} / h_{t+1} operand of the recurrent weights): a plain GEMM over the
            # overlapping rows after shifting one of the two base pointers by |padh| * wA rows.
            shift = padh * wA
            P = hA * wA - abs(shift)
            if shift > 0:
                a_ptr += 4 * shift * ldA
            elif shift < 0:
                b_ptr += 4 * (-shift) * ldB
            ws = self.empty(L.wgrad_gemm_x3_ws_floats(CA, CB, P), dtype=torch.float32)
            L.wgrad_gemm_x3(a_ptr, ldA, CA, b_ptr, ldB, CB, ptr(dW), ptr(ws), P)
            return
        ws = self.empty(L.wgrad_gather_ws_floats(CA, CB, KH * KW, N * hA * wA, dt), dtype=torch.float32)
        L.wgrad_gather(a_ptr, ldA, CA, None, b_ptr, ldB, CB, ptr(dW), ptr(ws), N, hA, wA, HB, WB, 1, padh, padw, KH, KW, dt)

    def gru_wgrads(self, gl, dgi, dgh):
        """dW_ih += dgi^T x and, per direction, dW_hh += dgh^T h_{t -+ 1} of GRU layer gl (both directions' W_ih gradients are one stacked view:
        adjacent in the flat buffer, see `order` in _backward)"""
        T, N, G = self.T, self.N, self.G
        self.wgrad(dgi, 1536, 1536, gl.x, gl.I, gl.I, G[f"gru.weight_ih_l{gl.layer}"], 1, 1, T * N, 1, T * N, 0, 0, 1, 1, 0)
        for d, sfx in enumerate((f"_l{gl.layer}", f"_l{gl.layer}_reverse")):
            self.wgrad(dgh.data_ptr() + 4 * d * 768, 1536, 768, gl.out.data_ptr() + 4 * d * 256, 512, 256, G["gru.weight_hh" + sfx], 1, T, N, T, N,
                       1 if d == 0 else -1, 0, 1, 1, 0)

    def bn_pool_bwd(self, prefix, g, z, tr, saved, C, H, W, PH, PW):
        L = self.L
        gsum = self.stat(C)
        L.rec_bn_reduce(ptr(g), ptr(z), ptr(tr), ptr(saved), ptr(gsum), C, self.N, H, W, PH, PW, self.dt)
        coef = self.empty(3, C, dtype=torch.float32)
        L.bn_bwd_finalize(ptr(gsum), self.N * H * W, C, ptr(self.P[f"{prefix}.weight"]), ptr(saved), ptr(coef), ptr(self.G[f"{prefix}.weight"]),
                          ptr(self.G[f"{prefix}.bias"]))
        dz = self.empty(self.N, H, W, C)
        L.dz_apply(ptr(g), ptr(z), ptr(tr), ptr(coef), ptr(dz), C, self.N, H, W, PH, PW, self.dt, None)
        return dz

    def relu_bwd(self, g, a, C, H, W, dbias):
        """gradient through a ReLU (dz = g where a > 0) and, in the same pass, the conv's bias gradient (column sums of dz)"""
        dz = self.empty(self.N, H, W, C)
        self.L.dz_apply(ptr(g), ptr(a), ptr(_identity_tr(C, self.dev)), ptr(_unit_coef(C, self.dev)), ptr(dz), C, self.N, H, W, 1, 1, self.dt, ptr(dbias))
        return dz

    def backward(self, g_lp):
        try:
            return self._backward(g_lp)
        finally:
            self.L.bwd_defer_flush()  # (a no-op after a complete backward; after an exception it leaves the library's deferral mode)

    def _backward(self, g_lp):
        L, P, N, S = self.L, self.P, self.N, self
        T, W2, W = S.T, S.W2, self.W
        rows = T * N
        C = self.ncls
        # flat gradient buffer in backward-completion order (DP buckets = contiguous ranges)
        order = ["output.", "gru.weight_ih_l1", "gru.weight_hh_l1", "gru.bias_ih_l1", "gru.bias_hh_l1", "gru.weight_ih_l0", "gru.weight_hh_l0",
                 "gru.bias_ih_l0", "gru.bias_hh_l0", "conv.20.", "conv.19.", "conv.16.", "conv.15.", "conv.13.", "conv.10.", "conv.9.", "conv.7.",
                 "conv.4.", "conv.3.", "conv.0."]
        flat = torch.zeros(sum(p.numel() for p in P.values()), dtype=torch.float32, device=self.dev)
        self.G, off, stage_end = {}, 0, {}
        for stage in order:
            for k in self.names:
                if k.startswith(stage) and k not in self.G:
                    n = P[k].numel()
                    self.G[k] = flat[off:off + n].view_as(P[k])
                    off += n
            stage_end[stage] = off
        assert off == flat.numel(), "parameter ordering table is incomplete"
        bucketer = getattr(self.mod, "_grad_bucketer", None)
        done = [0]

        main = torch.cuda.current_stream()
        self._side, self._keep = (_rec_side_stream(self.dev) if _REC_OVERLAP else None), []
        # Deferred second stage (ocrs_bwd_defer_begin / _flush, round 5): the launches that used to end in cross-block float atomics (bias column sums,
        # the first layer's weight gradient, the GRU bias sums) write per-block partials into the library's workspace and queue a fixed-order column
        # sum; ONE launch at the end of the backward runs them all -- the step's gradients are bit-reproducible.  Not with a gradient bucketer (a
        # stage's gradients must be complete when it is reported).
        deferring = bucketer is None
        if deferring:
            L.bwd_defer_begin(None, 0)

        def join_side():
            if self._side is not None and self._keep:
                main.wait_stream(self._side)
                self._keep.clear()

        def stage_done(stage):
            if bucketer is not None and stage_end[stage] > done[0]:
                join_side()  # (DDP: a stage's gradients are final when they are reported)
                bucketer.ready(flat, done[0], stage_end[stage])
            done[0] = max(done[0], stage_end[stage])

        G = self.G
        g_lp = g_lp.contiguous().float()
        dlog = self.empty(rows, S.ldl, dtype=torch.float32)
        L.log_softmax_bwd(ptr(S.lp), ptr(g_lp), ptr(dlog), rows, C, S.ldl, 0)
        top = S.gru[1].out
        self.wgrad(dlog, S.ldl, C, top, 512, 512, G["output.0.weight"], 1, 1, rows, 1, rows, 0, 0, 1, 1, 0)
        L.col_sum(ptr(dlog), S.ldl, C, ptr(G["output.0.bias"]), rows, 0)
        dout = self.linear(dlog, S.ldl, S.ldl, P["output.0.weight"], 512, 1, None, 512, 512, rows, kw=C)  # dlog's columns [C, ldl) are zero
        stage_done("output.")
        dhz = self.empty(2, 2, N, 256, dtype=torch.float32)
        held = []
        for layer in (1, 0):
            gl = S.gru[layer]
            I = gl.I
            dgi = self.empty(rows, 1536, dtype=torch.float32)
            dgh = self.empty(rows, 1536, dtype=torch.float32)
            if self.gru_seq:
                sync, xws = self.seq_sync()
                L.gru_seq_bwd(ptr(dout), ptr(gl.saved), ptr(gl.out), ptr(gl.w_hh), ptr(dgi), ptr(dgh), T, N, ptr(sync),
                              ptr(_gru_err(self.dev)), ptr(xws), self.gru_exact, ptr(G[f"gru.bias_ih_l{layer}"]), ptr(G[f"gru.bias_hh_l{layer}"]))
            else:
                nfl = 24 * 16 * 64 * 8
                whhT = torch.empty(2 * nfl, dtype=torch.float32, device=self.dev)
                for d in (0, 1):
                    L.pack_frags(gl.w_hh.data_ptr() + 4 * d * 768 * 256, 0, 768, 256, 768, 0, 256, 1, whhT.data_ptr() + 4 * d * nfl, 0)
                L.gru_layer_bwd(ptr(dout), ptr(gl.saved), ptr(gl.out), ptr(whhT), ptr(dgi), ptr(dgh), ptr(dhz), T, N)
            # The weight gradients.  With a side stream, layer 0's run there next to the conv backward that follows.  Layer 1's must not run under
            # layer 0's persistent recurrence (its hand-offs suffer from streaming neighbours: measured slower): they are queued on the side
            # stream BEHIND that recurrence, together with layer 0's -- except with a bucketer, which reports layer 1's stage before layer 0 runs.
            if layer == 1 and self._side is not None and bucketer is None:
                held.append((gl, dgi, dgh))
                self._keep.extend((dgi, dgh, gl.x, gl.out))
            elif layer == 1:
                self.gru_wgrads(gl, dgi, dgh)
            else:
                def wgrads_now():
                    for args in held + [(gl, dgi, dgh)]:
                        self.gru_wgrads(*args)
                self.on_side(wgrads_now, dgi, dgh, gl.x, gl.out)
            if not self.gru_seq:  # (the persistent launch accumulates the bias gradients itself)
                L.col_sum(ptr(dgi), 1536, 1536, ptr(G[f"gru.bias_ih_l{layer}"]), rows, 0)
                L.col_sum(ptr(dgh), 1536, 1536, ptr(G[f"gru.bias_hh_l{layer}"]), rows, 0)
            dout = self.linear(dgi, 1536, 1536, gl.w_ih, I, 1, None, I, I, rows)  # dx = dgi W_ih: W(m, k) = W_ih[k][m]
            stage_done(f"gru.bias_hh_l{layer}")
        dseq = dout  # [T][N][128] fp32
        # ---- conv.20 (BN, no ReLU) + AvgPool ----
        gsum = self.stat(128)
        L.avgpool_bn_reduce(ptr(dseq), ptr(S.z19), ptr(S.sv19), ptr(gsum), 128, N, 5, T, self.dt)
        coef = self.empty(3, 128, dtype=torch.float32)
        L.bn_bwd_finalize(ptr(gsum), N * 5 * T, 128, ptr(P["conv.20.weight"]), ptr(S.sv19), ptr(coef), ptr(G["conv.20.weight"]), ptr(G["conv.20.bias"]))
        dz19 = self.empty(N, 5, T, 128)
        L.avgpool_dz(ptr(dseq), ptr(S.z19), ptr(coef), ptr(dz19), 128, N, 5, T, self.dt)
        g15 = self.conv_bwd("conv.19.weight", dz19, S.a15, 5, T, 4, W2, 1)
        stage_done("conv.19.")
        dz15 = self.bn_pool_bwd("conv.16", g15, S.z15, S.tr15, S.sv15, 128, 8, W2, 2, 1)
        g13 = self.conv_bwd("conv.15.weight", dz15, S.a13, 8, W2, 8, W2, 1)
        stage_done("conv.15.")
        dz13 = self.relu_bwd(g13, S.a13, 128, 8, W2, G["conv.13.bias"])
        g9 = self.conv_bwd("conv.13.weight", dz13, S.a9, 8, W2, 8, W2, 1)
        stage_done("conv.13.")
        dz9 = self.bn_pool_bwd("conv.10", g9, S.z9, S.tr9, S.sv9, 128, 16, W2, 2, 1)
        g7 = self.conv_bwd("conv.9.weight", dz9, S.a7, 16, W2, 16, W2, 1)
        stage_done("conv.9.")
        dz7 = self.relu_bwd(g7, S.a7, 128, 16, W2, G["conv.7.bias"])
        g3 = self.conv_bwd("conv.7.weight", dz7, S.a3, 16, W2, 16, W2, 1)
        stage_done("conv.7.")
        dz3 = self.bn_pool_bwd("conv.4", g3, S.z3, S.tr3, S.sv3, 64, 32, W // 2, 2, 2)
        g0 = self.conv_bwd("conv.3.weight", dz3, S.a0, 32, W // 2, 32, W // 2, 1)
        stage_done("conv.3.")
        L.conv0_bwd(ptr(self.x), ptr(P["conv.0.weight"]), ptr(P["conv.0.bias"]), ptr(g0), ptr(G["conv.0.weight"]), ptr(G["conv.0.bias"]), N, self.H,
                    W, self.dt)
        join_side()
        self._side, self._keep = None, ()
        if deferring:
            L.bwd_defer_flush()  # (behind the join: partials written on the side stream are complete in main-stream order)
        stage_done("conv.0.")
        if bucketer is not None:
            bucketer.finish(flat)
        return [G[k] for k in self.names]


def _adjacent(a, b):
    """b starts where a ends, inside ONE storage (tensors that merely happen to be neighbours in the allocator's pool do not count)"""
    return (a.is_contiguous() and b.is_contiguous() and b.data_ptr() == a.data_ptr() + 4 * a.numel()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


_GRU_ERR = {}      # device -> (device error word of the persistent GRU launches, pinned host copy)
_GRU_SEQ_OFF = {}  # device -> True once a persistent launch timed out there: this process uses the per-step kernels from then on


def _gru_err_entry(dev):
    ent = _GRU_ERR.get(dev)
    if ent is None:
        ent = _GRU_ERR[dev] = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32).pin_memory())
    return ent


def _gru_err_reset(dev):
    """A timeout was observed: clear the word (device and host copy) and route this process to the per-step kernels (rec_gru.hip) -- a
    transient stall (another process or stream holding the CUs the resident grid needs) must not end the training process."""
    ent = _gru_err_entry(dev)
    # every poll copy queued so far (e.g. the failed step's backward poll) must have landed before the host word is cleared, or it would
    # set the word again and the next forward would report the same failure twice; the device word is cleared in stream order first
    ent[0].zero_()
    torch.cuda.current_stream(dev).synchronize()
    ent[1].zero_()
    _GRU_SEQ_OFF[dev] = True


def _gru_err(dev):
    """The error word the persistent GRU launches raise when a wait times out (ocrs_gru_seq_fwd / _bwd: outputs incomplete).  Training checks
    it WITHOUT a device synchronisation: every forward and every backward queue a copy of the word into pinned host memory, every forward
    looks at the host copy first.  A failure is reported ONCE, one step late (the step whose launch timed out produced incomplete gradients:
    the caller should discard / repeat it), the word is cleared and later forwards run on the per-step kernels.  Inference (no autograd)
    checks synchronously and repeats the forward itself (RecognitionModel.forward)."""
    ent = _gru_err_entry(dev)
    if int(ent[1][0]) != 0:
        _gru_err_reset(dev)
        raise RuntimeError("a persistent GRU launch (ocrs_gru_seq_fwd/_bwd) timed out waiting for its peer workgroups: the results of the previous "
                           "step are incomplete and the optimizer step that followed it has ALREADY been applied -- restore the last checkpoint (or accept one step "
                           "taken with incomplete gradients) before continuing.  The error word was cleared and this process now uses the per-step GRU "
                           "kernels (csrc/rec_gru.hip); later steps are not affected")
    return ent[0]


def _gru_err_poll(dev):
    ent = _GRU_ERR.get(dev)
    if ent is not None:
        ent[1].copy_(ent[0], non_blocking=True)


def _new_run(mod, x, names, params, dtype):
    P = dict(zip(names, (p.detach() for p in params)))
    return _RecRun(P, dict(mod.named_buffers()), x.device, dtype, x.shape[0], x.shape[2], x.shape[3], mod.training, mod, x)


class _RecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, names, dtype, *params):
        run = ctx.run = _new_run(mod, x, names, params, dtype)
        ctx.params = params
        ctx.versions = [p._version for p in params]
        out = run.forward()
        if run.gru_seq:
            _gru_err_poll(run.dev)  # (a timed-out forward launch is seen at the next forward even if no backward follows)
        return out

    @staticmethod
    def backward(ctx, g):
        _check_versions(ctx)
        grads = ctx.run.backward(g)
        _gru_err_poll(ctx.run.dev)
        ctx.run = None  # free the saved activations (and break the output -> grad_fn -> ctx -> run cycle)
        return (None, None, None, None, *grads)


# the conv and GRU weight gradients of the backward on a side stream (False: everything on the caller's stream -- bench.py's per-launch
# roofline, tools/prof_crnn.py)
_REC_OVERLAP = True
_REC_SIDE = {}


def _rec_side_stream(dev):
    st = _REC_SIDE.get(dev)
    if st is None:
        st = _REC_SIDE[dev] = torch.cuda.Stream(device=dev)
    return st


class RecognitionModel(nn.Module):
    """Text recognition CRNN (reference: ocrs_models/models.py:146-268).

    ``forward(x: (B,1,64,W)) -> (W//4 + 1, B, len(alphabet)+1)`` log-probabilities (fp32)."""

    def __init__(self, alphabet: str, act_dtype: torch.dtype | None = None):
        super().__init__()
        n_classes = len(alphabet) + 1
        self.conv = nn.Sequential(
            nn.Conv2d(1, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(32, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(),
            nn.Conv2d(128, 128, 3, padding=1, bias=False), nn.BatchNorm2d(128), nn.ReLU(), nn.MaxPool2d((2, 1)),
            nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(),
            nn.Conv2d(128, 128, 3, padding=1, bias=False), nn.BatchNorm2d(128), nn.ReLU(), nn.MaxPool2d((2, 1)),
            nn.Conv2d(128, 128, (2, 2), padding=1, bias=False), nn.BatchNorm2d(128), nn.AvgPool2d((4, 1)),
        )
        self.gru = nn.GRU(128, 256, bidirectional=True, num_layers=2)
        self.output = nn.Sequential(nn.Linear(512, n_classes), nn.LogSoftmax(dim=2))
        self.act_dtype = act_dtype

    def _gru_flatten(self):
        """Re-home the forward and reverse direction's GRU parameters of each layer into adjacent halves of a common buffer (what
        nn.GRU.flatten_parameters does for its library), ONCE: the kernels take both directions as one stacked tensor, which is then a view --
        no per-step concatenation.  Parameters that were re-allocated since (``.to()``, ``.data = ...``) are re-homed at the next forward."""
        for layer in (0, 1):
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                pa, pb = getattr(self.gru, f"{kind}_l{layer}"), getattr(self.gru, f"{kind}_l{layer}_reverse")
                if not _adjacent(pa, pb):
                    with torch.no_grad():
                        buf = torch.stack([pa.detach(), pb.detach()], 0).contiguous()
                        pa.data, pb.data = buf[0], buf[1]

    @staticmethod
    def _gru_stacked(layer, P):
        """(w_ih (1536, I), w_hh (2, 768, 256), b_ih (1536,), b_hh (1536,)): both directions of one layer as views (see _gru_flatten)"""
        out = []
        for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            a, b = P[f"gru.{kind}_l{layer}"], P[f"gru.{kind}_l{layer}_reverse"]
            if not _adjacent(a, b):
                raise RuntimeError("GRU parameters of the two directions are not adjacent (RecognitionModel._gru_flatten was bypassed)")
            st = torch.as_strided(a, (2,) + tuple(a.shape), (a.numel(),) + tuple(a.stride()))
            out.append(st if kind == "weight_hh" else st.reshape((2 * a.shape[0],) + tuple(a.shape[1:])))
        return out

    def _act_dtype(self):
        if self.act_dtype is not None:
            return self.act_dtype
        if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
            return torch.bfloat16
        return torch.float32

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("ocrs_models_amd.RecognitionModel runs on MI355X only (no CPU path); move the model and input to 'cuda'")
        if x.dim() != 4 or x.shape[1] != 1:
            raise RuntimeError(f"expected (B,1,64,W) input, got {tuple(x.shape)}")
        x = x.contiguous().float()
        self._gru_flatten()
        names = [n for n, _ in self.named_parameters()]
        params = [p for _, p in self.named_parameters()]
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("parameters must be contiguous fp32")
        dtype = self._act_dtype()
        with torch.autocast("cuda", enabled=False):
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                return _RecFn.apply(x, self, names, dtype, *params)
            run = _new_run(self, x, names, params, dtype)
            out = run.forward()
            if run.gru_seq and not self._gru_seq_ok(run):
                # inference / validation: a timed-out persistent launch left `out` incomplete -- one synchronous check per call is cheap here;
                # repeat this forward on the per-step kernels instead of returning wrong log-probabilities
                _gru_err_reset(x.device)
                out = _new_run(self, x, names, params, dtype).forward()
            return out

    @staticmethod
    def _gru_seq_ok(run):
        try:
            run.L.gru_seq_status(ptr(_gru_err_entry(run.dev)[0]))
            return True
        except RuntimeError:
            return False
