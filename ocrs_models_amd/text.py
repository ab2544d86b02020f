"""Host-side sequence/text contract of the recognition train step, same behaviour as the reference's helpers:

* ``DEFAULT_ALPHABET``, ``encode_text``, ``decode_text``, ``ctc_greedy_decode_text``  (datasets/hiertext.py:133-137, datasets/util.py:113-177)
* ``round_up``, ``ctc_input_and_target_compatible``, ``collate_samples``           (train_rec.py:220-304)
* ``RecognitionAccuracyStats``                                                     (train_rec.py:20-82) -- arg-max and the CTC collapse run
  on the GPU (``ocrs_ctc_greedy_decode``), only the already-collapsed label rows come back for the Levenshtein distance.
* ``DeviceRecognitionAccuracyStats``, ``edit_distance_device``                       the same stats with nothing left on the host
  (``ocrs_ctc_cer_update`` / ``ocrs_edit_distance``, csrc/rec_cer.hip): edit distances and both sums on the GPU, one host sync per read.
* ``transform_image``                                                              (datasets/util.py:27-35)
* ``beam_decode_spans``, ``ctc_align_spans``                                         CTC prefix beam search next to the greedy rule of
  datasets/util.py:147-177, and the forced alignment that gives its labelling spans (``ocrs_ctc_beam_decode`` / ``ocrs_ctc_align_spans``,
  csrc/ctc_beam.hip)
* ``CharLM``, ``LMGain``                                                             a character n-gram model counted on the host and its
  gain table on the device, which ``lm=`` of the beam decoders fuses into the ranking (``ocrs_ctc_beam_decode_lm``)
"""
from __future__ import annotations

import string

import numpy as np
import torch

from ._lib import lib, ptr

DEFAULT_ALPHABET = (
    " " + string.digits + "".join(chr(c) for c in range(33, 127) if not chr(c).isalnum()) + "€" + string.ascii_uppercase + string.ascii_lowercase
)


def transform_image(img: torch.Tensor) -> torch.Tensor:
    """8-bit greyscale CHW -> float CHW in [-0.5, 0.5]."""
    return img.float() / 255.0 - 0.5


def encode_text(text: str, alphabet, unknown_char: str) -> torch.Tensor:
    alphabet = list(alphabet)
    unk = alphabet.index(unknown_char)
    return torch.tensor([(alphabet.index(ch) if ch in alphabet else unk) + 1 for ch in text], dtype=torch.int32)


def decode_text(x, alphabet) -> str:
    if isinstance(x, torch.Tensor):
        x = x.tolist()
    return "".join(alphabet[c - 1] for c in x if c > 0)


def ctc_greedy_decode_text(x, alphabet) -> str:
    """Host version for a single label sequence (repeat test before the blank test)."""
    if isinstance(x, torch.Tensor):
        x = x.tolist()
    out, last = [], None
    for c in x:
        if c == last:
            continue
        last = c
        if c != 0:
            out.append(alphabet[c - 1])
    return "".join(out)


class _Decode:
    """Result handle of greedy_decode_batch_async: the collapsed labels are on their way into pinned host memory."""

    def __init__(self, host, event, amax, N, T):
        self.host, self.event, self.amax, self.N, self.T = host, event, amax, N, T

    def result(self):
        """list of N collapsed label lists (waits for the copy only, not for work queued after it)"""
        self.event.synchronize()
        N, T = self.N, self.T
        labels_h, lens_h = self.host[:N * T].view(N, T).tolist(), self.host[N * T:].tolist()
        return [row[:n] for row, n in zip(labels_h, lens_h)]


_DECODE_SIDE = True  # greedy decode on a side stream (tools/prof_crnn.py turns it off for single-stream traces)
_DECODE_STREAMS = {}


def _decode_stream(dev):
    st = _DECODE_STREAMS.get(dev)
    if st is None:
        st = _DECODE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return st


def greedy_decode_batch_async(log_probs: torch.Tensor, input_lengths) -> _Decode:
    """(T,N,C) log-probs on the GPU -> handle; arg-max + collapse run on the device, ONE non-blocking copy brings labels | lengths to the
    host.  A caller that queues more GPU work (the backward pass) before asking for ``result()`` overlaps the host-side part with it."""
    lp = log_probs.contiguous().float()
    T, N, C = lp.shape
    dev = lp.device
    il = torch.as_tensor(input_lengths, dtype=torch.int64)
    if not il.is_cuda:
        il = il.pin_memory().to(dev, non_blocking=True)
    # The decode depends on the log-probs only: on a side stream it runs next to the CTC loss / the start of the backward instead of in front
    # of them (arg-max + collapse + copies are ~40 us of small launches).  result() waits for the event recorded on that stream.
    main = torch.cuda.current_stream(dev)
    side = _decode_stream(dev) if _DECODE_SIDE and not torch.cuda.is_current_stream_capturing() else main
    if side is not main:
        side.wait_stream(main)
        lp.record_stream(side)
        il.record_stream(side)
    with torch.cuda.stream(side):
        amax = torch.empty(N, T, dtype=torch.int32, device=dev)
        buf = torch.zeros(N * T + N, dtype=torch.int32, device=dev)  # labels | lens
        lib().ctc_greedy_decode(ptr(lp), ptr(il), ptr(amax), ptr(buf), buf.data_ptr() + 4 * N * T, T, N, C)
        host = torch.empty(N * T + N, dtype=torch.int32, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
    return _Decode(host, ev, amax, N, T)


def greedy_decode_batch(log_probs: torch.Tensor, input_lengths):
    """(T,N,C) log-probs on the GPU -> list of N collapsed label lists (arg-max + collapse on the device, one D2H copy)."""
    h = greedy_decode_batch_async(log_probs, input_lengths)
    return h.result(), h.amax


def span_arrays(rows: int, ld: int, device):
    """The output arrays of ``ocrs_ctc_decode_spans`` for ``rows`` samples at a row pitch of ``ld``, as views of ONE int32 device buffer
    ``labels | t0 | t1 | peak | lens`` (so that one copy brings all of them to the host) -> ``(buf, labels, t0, t1, peak, lens)``; ``peak`` is
    the float32 view of its part.  Not initialised: entries of a row from its length on are never written."""
    buf = torch.empty(4 * rows * ld + rows, dtype=torch.int32, device=device)
    return (buf, *span_views(buf, rows, ld))


def span_views(buf: torch.Tensor, rows: int, ld: int):
    """The one statement of the span buffer's layout: a flat int32 buffer ``labels | t0 | t1 | peak | lens`` for ``rows`` samples at a row
    pitch of ``ld``, on the device or its copy on the host -> the views ``(labels, t0, t1, peak, lens)``; the first four are (rows, ld),
    ``peak`` the float32 view of its part, ``lens`` (rows,).  Nothing is copied: the views alias ``buf``."""
    cells = rows * ld
    part = buf[:4 * cells].view(4, rows, ld)
    return part[0], part[1], part[2], part[3].view(torch.float32), buf[4 * cells:]


def span_lengths(lens: torch.Tensor) -> list[int]:
    """``lens`` of ``span_views`` on the host as a list; -1, a beam row without any labelling of finite mass, reads as an empty row"""
    return [max(n, 0) for n in lens.tolist()]


class _DecodeSpans:
    """Result handle of greedy_decode_spans_async: the span arrays on the device, and on their way into pinned host memory."""

    def __init__(self, arrays, host, event, N, ld, amax):
        (self.buf, self.labels, self.t0, self.t1, self.peak, self.lens), self.host, self.event, self.N, self.ld, self.amax = arrays, host, event, N, ld, amax

    def result(self):
        """list of N dicts ``labels``, ``t0``, ``t1`` (int lists) and ``peak`` (float list), one entry per character (waits for the copy only)"""
        self.event.synchronize()
        *part, lens = span_views(self.host, self.N, self.ld)
        labels, t0, t1, peak = (p.tolist() for p in part)
        return [{"labels": labels[i][:n], "t0": t0[i][:n], "t1": t1[i][:n], "peak": peak[i][:n]} for i, n in enumerate(span_lengths(lens))]


def greedy_decode_spans_async(log_probs: torch.Tensor, input_lengths, out=None, row0: int = 0):
    """``greedy_decode_batch_async`` that keeps where every character came from (``ocrs_ctc_decode_spans``): (T,N,C)
    log-probs on the GPU -> per character its label, the first and last time step of the run it was collapsed from and the largest
    log-prob of its class over that run.  Labels and lengths are exactly those of ``greedy_decode_batch_async``.

    ``out=None``: new arrays (pitch T) and a handle whose ``result()`` waits for ONE non-blocking copy of all of them.  ``out`` = the tuple of
    ``span_arrays`` shared by the chunks of a page: sample n writes row ``row0 + n``, nothing is copied and None is returned -- the caller
    copies the buffer once, after its last chunk.  Runs on the current stream."""
    lp = log_probs.contiguous().float()
    if lp.dim() != 3 or not lp.is_cuda:
        raise RuntimeError("greedy_decode_spans: expected (T,N,C) log-probs on the GPU (no CPU path)")
    T, N, C = lp.shape
    if T < 1 or C < 1:
        raise RuntimeError("greedy_decode_spans: expected at least one time step and one class")
    dev = lp.device
    il = torch.as_tensor(input_lengths, dtype=torch.int64)
    if not il.is_cuda:
        il = il.pin_memory().to(dev, non_blocking=True) if il.numel() else il.to(dev)
    il = il.contiguous()
    if il.numel() != N:
        raise RuntimeError(f"greedy_decode_spans: {il.numel()} input lengths for {N} samples")
    own = out is None
    if own:
        out, row0 = span_arrays(N, T, dev), 0
    _, labels, t0, t1, peak, lens = out
    rows, ld = labels.shape
    if ld < T or row0 < 0 or row0 + N > rows or lens.numel() != rows:
        raise RuntimeError(f"greedy_decode_spans: rows {row0}..{row0 + N} of pitch {T} do not fit span arrays of {rows} rows of pitch {ld}")
    amax = torch.empty(N, T, dtype=torch.int32, device=dev)
    amax_lp = torch.empty(N, T, dtype=torch.float32, device=dev)
    if N:
        lib().ctc_decode_spans(ptr(lp), ptr(il), ptr(amax), ptr(amax_lp), T, N, C, int(row0), ld, ptr(labels), ptr(t0), ptr(t1), ptr(peak), ptr(lens))
    if not own:
        return None
    host = torch.empty(out[0].numel(), dtype=torch.int32, pin_memory=True)
    host.copy_(out[0], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return _DecodeSpans(out, host, ev, N, T, amax)


def greedy_decode_spans(log_probs: torch.Tensor, input_lengths):
    """(T,N,C) log-probs on the GPU -> list of N dicts ``labels``, ``t0``, ``t1``, ``peak``, one entry per character (one D2H copy)."""
    return greedy_decode_spans_async(log_probs, input_lengths).result()


BEAM_MAX_WIDTH, BEAM_MAX_CLASSES = 64, 256  # what ocrs_ctc_beam_decode supports (csrc/ctc_beam.hip)


class _BeamSpans(_DecodeSpans):
    """Result handle of beam_decode_spans_async: the span arrays and the scores on the device, and on their way into pinned host memory."""

    def __init__(self, arrays, host, event, N, ld, scores, scores_host, lm_scores=None, lm_scores_host=None):
        super().__init__(arrays, host, event, N, ld, None)
        self.scores, self.scores_host, self.lm_scores, self.lm_scores_host = scores, scores_host, lm_scores, lm_scores_host

    def result(self):
        """list of N dicts ``labels``, ``t0``, ``t1``, ``peak`` as ``greedy_decode_spans`` returns them, plus ``score``, the log-mass of the
        labelling, and with a language model ``lm_score``, the sum of its gains (waits for the copies only)"""
        out = super().result()
        for d, s in zip(out, self.scores_host.tolist()):
            d["score"] = s
        if self.lm_scores_host is not None:
            for d, s in zip(out, self.lm_scores_host.tolist()):
                d["lm_score"] = s
        return out


LM_MAX_ORDER = 3  # what ocrs_ctc_beam_decode_lm supports (csrc/ctc_beam.hip)


class LMGain:
    """A gain table of DESIGN.md §19 on a device: ``table`` float32 of shape ``(C,) * order``, ``table[ctx..., c]`` the credit for appending
    label c after the last ``order - 1`` labels (padded on the left with 0).  Entries are finite or -inf; NaN and +inf are refused here."""

    def __init__(self, table, device=None):
        t = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
        if not 1 <= t.ndim <= LM_MAX_ORDER or t.shape != (t.shape[0],) * t.ndim or t.shape[0] < 2:
            raise RuntimeError(f"LMGain: expected a table of shape (C,) * order with C >= 2 and order in 1..{LM_MAX_ORDER}, got {t.shape}")
        if np.isnan(t).any() or (t == np.inf).any():
            raise RuntimeError("LMGain: the table holds NaN or +inf (entries must be finite or -inf)")
        self.order, self.C = t.ndim, t.shape[0]
        self.table = torch.from_numpy(t).to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)


def witten_bell(counts: np.ndarray) -> np.ndarray:
    """float64 counts ``n[ctx..., c]`` of shape ``(C,) * order`` -> float64 P(c | ctx) of the same shape by interpolated Witten-Bell smoothing
    (DESIGN.md §19): with n(ctx) the count of ctx, d(ctx) its number of distinct followers and ctx' the context without its oldest label,
    P_k(c | ctx) = (n(ctx, c) + d(ctx) P_{k-1}(c | ctx')) / (n(ctx) + d(ctx)) where n(ctx) > 0, else P_{k-1}(c | ctx'); P_0 = 1 / (C - 1) for
    c >= 1 and 0 for the blank.  The counts of a shorter context are the sums over the oldest label."""
    n = np.asarray(counts, dtype=np.float64)
    C = n.shape[0]
    levels = [n]
    while levels[0].ndim > 1:
        levels.insert(0, levels[0].sum(axis=0))
    p = np.full(C, 1.0 / (C - 1))
    p[0] = 0.0
    for nk in levels:
        tot, d = nk.sum(axis=-1, keepdims=True), (nk > 0).sum(axis=-1, keepdims=True).astype(np.float64)
        back = np.broadcast_to(p, nk.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.where(tot > 0, (nk + d * back) / (tot + d), back)
    return p


class CharLM:
    """Character n-gram language model over the recogniser's labels: ``log_probs`` float32 of shape ``(C,) * order``,
    ``log_probs[ctx..., c] = log P(c | ctx)`` with the context padded on the left with 0 (the blank: start of line); every row sums to 1
    over c = 1..C-1 and column 0 is -inf.  Counted and smoothed on the host in numpy float64, a one-off whose result is reproducible bit
    for bit; ``gain`` puts the table the beam search reads on the device."""

    def __init__(self, log_probs, alphabet=None, order: int | None = None):
        lp = np.ascontiguousarray(np.asarray(log_probs, dtype=np.float32))
        if not 1 <= lp.ndim <= LM_MAX_ORDER or lp.shape != (lp.shape[0],) * lp.ndim or (order is not None and order != lp.ndim):
            raise RuntimeError(f"CharLM: expected log-probs of shape (C,) * order with order in 1..{LM_MAX_ORDER}, got {lp.shape}")
        if alphabet is not None and len(alphabet) + 1 != lp.shape[0]:
            raise RuntimeError(f"CharLM: {lp.shape[0]} classes for an alphabet of {len(alphabet)} characters")
        self.log_probs, self.alphabet, self.order = lp, None if alphabet is None else "".join(alphabet), lp.ndim
        self._gains = {}

    @staticmethod
    def count(rows, lengths, n_classes: int, order: int = 3) -> np.ndarray:
        """float64 n-gram counts of shape ``(n_classes,) * order`` over the lines ``rows[i, :lengths[i]]``, each padded on the left with
        ``order - 1`` zeros"""
        if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= LM_MAX_ORDER:
            raise RuntimeError(f"CharLM: order must be an integer in 1..{LM_MAX_ORDER}, got {order!r}")
        C = int(n_classes)
        if C < 2:
            raise RuntimeError("CharLM: expected at least two classes (the blank and one label)")
        rows = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        lengths = lengths.cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
        rows = rows.astype(np.int64).reshape(len(lengths), -1) if len(lengths) else np.zeros((0, 1), dtype=np.int64)
        lengths = np.minimum(lengths.astype(np.int64), rows.shape[1])
        valid = np.arange(rows.shape[1])[None, :] < lengths[:, None]
        if ((rows < 1) | (rows >= C))[valid].any():
            raise RuntimeError(f"CharLM: labels must lie in 1..{C - 1}")
        padded = np.concatenate([np.zeros((rows.shape[0], order - 1), dtype=np.int64), np.where(valid, rows, 0)], axis=1)
        flat = np.zeros(valid.shape, dtype=np.int64)
        for k in range(order):
            flat = flat * C + padded[:, k:k + rows.shape[1]]
        return np.bincount(flat[valid], minlength=C ** order).astype(np.float64).reshape((C,) * order)

    @classmethod
    def from_labels(cls, rows, lengths, n_classes: int, order: int = 3, alphabet=None):
        """the model of already encoded lines (``rows`` (N, L) labels in 1..n_classes-1, ``lengths`` (N,)), such as the device line store's"""
        with np.errstate(divide="ignore"):
            return cls(np.log(witten_bell(cls.count(rows, lengths, n_classes, order))).astype(np.float32), alphabet)

    @classmethod
    def from_texts(cls, texts, alphabet=DEFAULT_ALPHABET, order: int = 3, unknown_char: str = "?"):
        """the model of text lines, encoded with ``encode_text``"""
        enc = [encode_text(t, alphabet, unknown_char).numpy() for t in texts]
        rows = np.zeros((len(enc), max([len(e) for e in enc], default=0) or 1), dtype=np.int64)
        for i, e in enumerate(enc):
            rows[i, :len(e)] = e
        return cls.from_labels(rows, np.asarray([len(e) for e in enc], dtype=np.int64), len(alphabet) + 1, order, alphabet)

    def save(self, path: str) -> None:
        """one .npz: the table, the alphabet (empty: none) and the order"""
        with open(path, "wb") as f:
            np.savez(f, log_probs=self.log_probs, alphabet=np.asarray(self.alphabet or ""), order=np.asarray(self.order, dtype=np.int64))

    @classmethod
    def load(cls, path: str):
        with np.load(path, allow_pickle=False) as z:
            alphabet = str(z["alphabet"][()])
            return cls(z["log_probs"], alphabet or None, int(z["order"]))

    def gain(self, weight: float = 1.0, bonus: float = 0.0, device=None) -> LMGain:
        """The table the beam search adds per appended label: ``float32(weight * log P + bonus)``, computed in float64 (column 0, which is
        never read, stays -inf).  ``weight`` scales the model against the recogniser, ``bonus`` pays every label for the probability mass a
        longer text loses.  Cached per (weight, bonus, device); NaN or +inf (a negative weight on a forbidden transition) is refused."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        key = (float(weight), float(bonus), str(dev))
        if key not in self._gains:
            with np.errstate(invalid="ignore"):
                g = (float(weight) * self.log_probs.astype(np.float64) + float(bonus)).astype(np.float32)
            g[..., 0] = -np.inf
            self._gains[key] = LMGain(g, dev)
        return self._gains[key]


def _span_args(who: str, log_probs, input_lengths):
    """the argument checks shared by the decoders that fill span arrays -> (lp, il, T, N, C, dev)"""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3 or not log_probs.is_cuda:
        raise RuntimeError(f"{who}: expected (T,N,C) log-probs on the GPU (no CPU path)")
    lp = log_probs.contiguous().float()
    T, N, C = lp.shape
    if T < 1 or C < 1:
        raise RuntimeError(f"{who}: expected at least one time step and one class")
    dev = lp.device
    il = torch.as_tensor(input_lengths, dtype=torch.int64)
    if not il.is_cuda:
        il = il.pin_memory().to(dev, non_blocking=True) if il.numel() else il.to(dev)
    il = il.contiguous()
    if il.numel() != N:
        raise RuntimeError(f"{who}: {il.numel()} input lengths for {N} samples")
    return lp, il, T, N, C, dev


def _check_beam_width(who: str, beam_width):
    if isinstance(beam_width, bool) or not isinstance(beam_width, int) or not 1 <= beam_width <= BEAM_MAX_WIDTH:
        raise RuntimeError(f"{who}: beam_width must be an integer in 1..{BEAM_MAX_WIDTH}, got {beam_width!r}")


def _align_into(lp, il, T, N, C, row0, ld, labels, lens, t0, t1, peak):
    """one ocrs_ctc_align_spans launch over rows row0 .. row0 + N of the span arrays"""
    ws = torch.empty(lib().ctc_align_ws_bytes(T, N, min(ld, T)), dtype=torch.uint8, device=lp.device)
    lib().ctc_align_spans(ptr(lp), ptr(il), T, N, C, int(row0), ld, ptr(labels), ptr(lens), ptr(t0), ptr(t1), ptr(peak), ptr(ws), ws.numel())


def _check_lm(who: str, lm, C=None):
    if not isinstance(lm, LMGain):
        raise RuntimeError(f"{who}: lm must be an LMGain (CharLM.gain(...)), got {type(lm).__name__}")
    if C is not None and lm.C != C:
        raise RuntimeError(f"{who}: the language model has {lm.C} classes, the log-probs {C}")


def beam_decode_spans_async(log_probs: torch.Tensor, input_lengths, beam_width: int, out=None, row0: int = 0, scores: torch.Tensor | None = None,
                            lm: LMGain | None = None, lm_scores: torch.Tensor | None = None):
    """``greedy_decode_spans_async`` for the best labelling under CTC prefix beam search with ``beam_width`` prefixes (DESIGN.md §18,
    ``ocrs_ctc_beam_decode``) and the spans of its forced alignment (``ocrs_ctc_align_spans``): the same span arrays, the same ``out`` /
    ``row0`` contract.  ``scores``: float32 device tensor with one entry per row of ``out`` that receives the labelling's log-mass at
    ``row0 + n`` (required with ``out``; without it a new one is made and copied with the arrays).  One beam launch and one align launch on
    the current stream.
    ``lm`` (``ocrs_ctc_beam_decode_lm``): the gain table of a language model on the log-probs' device; the prefixes are ranked
    by log-mass + gains, ``scores`` keeps its meaning and ``lm_scores``, under the rules of ``scores``, receives the gains of the labelling.
    None: the plain beam, the launches and bytes it has always had."""
    who = "beam_decode_spans"
    _check_beam_width(who, beam_width)
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise RuntimeError(f"{who}: expected (T,N,C) log-probs on the GPU (no CPU path)")
    if not 2 <= log_probs.shape[2] <= BEAM_MAX_CLASSES:
        raise RuntimeError(f"{who}: {log_probs.shape[2]} classes, supported are 2..{BEAM_MAX_CLASSES}")
    if lm is not None:
        _check_lm(who, lm, log_probs.shape[2])
    elif lm_scores is not None:
        raise RuntimeError(f"{who}: lm_scores without lm")
    lp, il, T, N, C, dev = _span_args(who, log_probs, input_lengths)
    if lm is not None and lm.table.device != dev:
        raise RuntimeError(f"{who}: the language model's table is on {lm.table.device}, the log-probs on {dev}")
    own = out is None
    if own:
        out, row0 = span_arrays(N, T, dev), 0
        scores = torch.empty(N, dtype=torch.float32, device=dev)
        lm_scores = None if lm is None else torch.empty(N, dtype=torch.float32, device=dev)
    _, labels, t0, t1, peak, lens = out
    rows, ld = labels.shape
    if ld < T or row0 < 0 or row0 + N > rows or lens.numel() != rows:
        raise RuntimeError(f"{who}: rows {row0}..{row0 + N} of pitch {T} do not fit span arrays of {rows} rows of pitch {ld}")
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.numel() == rows):
        raise RuntimeError(f"{who}: scores must be a contiguous float32 device tensor with one entry per row ({rows})")
    if lm is not None and not (isinstance(lm_scores, torch.Tensor) and lm_scores.is_cuda and lm_scores.dtype == torch.float32 and lm_scores.is_contiguous()
                               and lm_scores.numel() == rows):
        raise RuntimeError(f"{who}: lm_scores must be a contiguous float32 device tensor with one entry per row ({rows})")
    if N:
        ws = torch.empty(lib().ctc_beam_ws_bytes(T, N, beam_width), dtype=torch.uint8, device=dev)
        if lm is None:
            lib().ctc_beam_decode(ptr(lp), ptr(il), T, N, C, beam_width, int(row0), ld, ptr(labels), ptr(lens), ptr(scores), ptr(ws), ws.numel())
        else:
            lib().ctc_beam_decode_lm(ptr(lp), ptr(il), T, N, C, beam_width, ptr(lm.table), lm.order, int(row0), ld, ptr(labels), ptr(lens), ptr(scores),
                                     ptr(lm_scores), ptr(ws), ws.numel())
        _align_into(lp, il, T, N, C, row0, ld, labels, lens, t0, t1, peak)
    if not own:
        return None
    host = torch.empty(out[0].numel(), dtype=torch.int32, pin_memory=True)
    host.copy_(out[0], non_blocking=True)
    scores_host = torch.empty(N, dtype=torch.float32, pin_memory=True)
    scores_host.copy_(scores, non_blocking=True)
    lm_host = None
    if lm is not None:
        lm_host = torch.empty(N, dtype=torch.float32, pin_memory=True)
        lm_host.copy_(lm_scores, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return _BeamSpans(out, host, ev, N, T, scores, scores_host, lm_scores, lm_host)


def beam_decode_spans(log_probs: torch.Tensor, input_lengths, beam_width: int, lm: LMGain | None = None):
    """(T,N,C) log-probs on the GPU -> list of N dicts ``labels``, ``t0``, ``t1``, ``peak`` (one entry per character) and ``score``; with
    ``lm`` also ``lm_score``."""
    return beam_decode_spans_async(log_probs, input_lengths, beam_width, lm=lm).result()


def ctc_align_spans(log_probs: torch.Tensor, input_lengths, labels, label_lengths):
    """Forced alignment of given labellings (``ocrs_ctc_align_spans``): ``labels`` (N, L) label rows and ``label_lengths``
    (N,) -> the tuple of ``span_arrays`` (pitch max(T, L)) with ``t0`` / ``t1`` / ``peak`` of every character on the best alignment path;
    ``lens`` is -1 where the labelling has no alignment of finite score.  One launch, no synchronisation."""
    who = "ctc_align_spans"
    lp, il, T, N, C, dev = _span_args(who, log_probs, input_lengths)
    lab = _labels_to_device(dev, labels)
    ll, = _lengths_to_device(dev, label_lengths)
    if lab.shape[0] != N or ll.numel() != N:
        raise RuntimeError(f"{who}: {lab.shape[0]} label rows and {ll.numel()} label lengths for {N} samples")
    L = lab.shape[1]
    out = span_arrays(N, max(T, L), dev)
    _, o_labels, t0, t1, peak, lens = out
    o_labels[:, :L] = lab
    lens.copy_(ll.clamp(max=L).to(torch.int32))
    if N:
        _align_into(lp, il, T, N, C, 0, max(T, L), o_labels, lens, t0, t1, peak)
    return out


def levenshtein(a, b) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


class RecognitionAccuracyStats:
    def __init__(self, alphabet=DEFAULT_ALPHABET):
        self.total_chars = 0
        self.char_errors = 0
        self.alphabet = list(alphabet)

    def update(self, targets, target_lengths, preds, pred_lengths):
        """targets [batch, seq]; preds [seq, batch, class] log-probs; lengths per sample."""
        assert len(target_lengths) == targets.size(0) and len(pred_lengths) == preds.size(1)
        self.update_async(targets, target_lengths, preds, pred_lengths)()

    def update_async(self, targets, target_lengths, preds, pred_lengths):
        """Queue the device part of ``update`` (arg-max, CTC collapse, copy to the host) and return the function that finishes it.  Calling that
        AFTER the backward pass and the optimizer step have been queued keeps the edit-distance work on the host off the GPU's critical path
        (the reference's loop blocks on it between forward and backward, train_rec.py:123)."""
        assert len(target_lengths) == targets.size(0) and len(pred_lengths) == preds.size(1)
        handle = greedy_decode_batch_async(preds, pred_lengths)
        rows, ntarget = targets.tolist(), int(sum(int(v) for v in target_lengths))

        def finish():
            for y, labels in zip(rows, handle.result()):
                want = decode_text(y, self.alphabet)
                got = "".join(self.alphabet[c - 1] for c in labels)
                self.char_errors += levenshtein(want, got)
            self.total_chars += ntarget

        return finish

    def char_error_rate(self) -> float:
        return self.char_errors / self.total_chars

    def stats_dict(self) -> dict:
        return {"char_error_rate": self.char_error_rate()}


def _lengths_to_device(dev, *lengths):
    """per-sample lengths (lists or tensors) -> int64 device tensors; host ones go over together in ONE pinned non-blocking copy"""
    ts = [torch.as_tensor(v, dtype=torch.int64).reshape(-1) for v in lengths]
    host = [i for i, t in enumerate(ts) if not t.is_cuda]
    if host:
        up = torch.cat([ts[i] for i in host]).pin_memory().to(dev, non_blocking=True)
        o = 0
        for i in host:
            n = ts[i].numel()
            ts[i], o = up[o:o + n], o + n
    return [t.to(dev).contiguous() for t in ts]


def _labels_to_device(dev, x):
    """(N, L) label rows -> contiguous int32 on the device (a host tensor: one pinned non-blocking copy)"""
    x = torch.as_tensor(x)
    if x.dim() != 2:
        raise RuntimeError("label rows must be (N, L)")
    if not x.is_cuda:
        x = x.to(torch.int32).contiguous().pin_memory().to(dev, non_blocking=True)
    return x.to(dev, torch.int32).contiguous()


def alphabet_codes(alphabet):
    """class id -> id of the first class with the same character (0 = blank stays 0): the table the device kernels compare through.  None
    when all characters are distinct (identity)."""
    first, codes = {}, [0]
    for i, ch in enumerate(alphabet):
        codes.append(first.setdefault(ch, i + 1))
    return codes if len(first) < len(codes) - 1 else None


def edit_distance_device(a, a_len, b, b_len, codes=None) -> torch.Tensor:
    """Levenshtein distance (unit costs, exactly ``levenshtein``) of N pairs of label rows on the GPU: ``a`` (N, pa) and ``b`` (N, pb) int32
    device tensors, the first ``a_len[i]`` / ``b_len[i]`` entries of row i count.  ``codes``: optional int32 device table, labels inside it
    are compared through it (two ids with the same code are equal).  Returns int32 (N,) on the device; nothing is synchronised."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda and isinstance(b, torch.Tensor) and b.is_cuda):
        raise RuntimeError("ocrs_models_amd edit distances run on MI355X only (no CPU path)")
    dev = a.device
    a, b = _labels_to_device(dev, a), _labels_to_device(dev, b)
    N, pa, pb = a.shape[0], a.shape[1], b.shape[1]
    al, bl = _lengths_to_device(dev, a_len, b_len)
    if b.shape[0] != N or al.numel() != N or bl.numel() != N:
        raise RuntimeError(f"a, b and their lengths must have the same batch size {N}")
    dist = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return dist
    if codes is not None:
        codes = codes.to(dev, torch.int32).contiguous()
    ws = torch.empty(lib().edit_distance_ws_bytes(N, pa), dtype=torch.uint8, device=dev)
    lib().edit_distance(ptr(a), ptr(al), pa, ptr(b), ptr(bl), pb, ptr(codes), 0 if codes is None else codes.numel(), ptr(ws), ptr(dist), N)
    return dist


class DeviceRecognitionAccuracyStats:
    """``RecognitionAccuracyStats`` with nothing left on the host: arg-max, CTC collapse, target compaction, edit distances and both sums
    run in ``ocrs_ctc_cer_update`` (two launches, no copy back, no synchronisation; capturable in a graph).  The counters live in ``state``,
    one int64[2] device tensor (char_errors, total_chars) that a data-parallel caller can all-reduce; reading ``char_errors``,
    ``total_chars``, ``char_error_rate()`` or ``stats_dict()`` is the one host synchronisation.

    Both quirks of the host class are kept: every zero of the whole padded target row is dropped (``decode_text``) whatever
    ``target_lengths`` says, and ``total_chars`` adds the lengths as given."""

    device_resident = True  # train_rec.train_step hands such stats the uploaded targets and the length tensors

    def __init__(self, alphabet=DEFAULT_ALPHABET):
        self.alphabet = list(alphabet)
        self._codes_host = alphabet_codes(self.alphabet)
        self._codes = None
        self.state = None   # created on the device of the first update
        self.last_dist = None  # int32 (N,) edit distances of the latest update (device)

    def update(self, targets, target_lengths, preds, pred_lengths):
        """targets [batch, seq] (host or device); preds [seq, batch, class] log-probs on the GPU; lengths per sample (lists or tensors)."""
        self.update_async(targets, target_lengths, preds, pred_lengths)

    def update_async(self, targets, target_lengths, preds, pred_lengths):
        """Queue the whole update on the current stream; the returned finisher has nothing left to do."""
        if not (isinstance(preds, torch.Tensor) and preds.is_cuda):
            raise RuntimeError("ocrs_models_amd accuracy stats run on MI355X only (no CPU path)")
        assert len(target_lengths) == targets.size(0) and len(pred_lengths) == preds.size(1)
        lp = preds.contiguous().float()
        T, N, C = lp.shape
        dev = lp.device
        if C != len(self.alphabet) + 1:
            raise RuntimeError(f"log-probs have {C} classes, the alphabet has {len(self.alphabet)} characters + blank")
        if self.state is None:
            self.state = torch.zeros(2, dtype=torch.int64, device=dev)
            if self._codes_host is not None:
                self._codes = torch.tensor(self._codes_host, dtype=torch.int32).to(dev)
        if N == 0:
            return _nothing
        tg = _labels_to_device(dev, targets)
        il, tl = _lengths_to_device(dev, pred_lengths, target_lengths)
        Lp = tg.shape[1]
        nbytes = lib().ctc_cer_ws_bytes(T, N, Lp)
        if nbytes <= 0:
            raise RuntimeError(f"unsupported shape for the device accuracy stats: T={T}, N={N}, target pitch {Lp}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dist = torch.empty(N, dtype=torch.int32, device=dev)
        lib().ctc_cer_update(ptr(lp), ptr(il), ptr(tg), ptr(tl), ptr(self._codes), ptr(ws), ptr(self.state), ptr(dist), T, N, C, Lp)
        self.last_dist = dist
        return _nothing

    def _read(self):
        return (0, 0) if self.state is None else tuple(self.state.tolist())

    @property
    def char_errors(self) -> int:
        return self._read()[0]

    @property
    def total_chars(self) -> int:
        return self._read()[1]

    def char_error_rate(self) -> float:
        errors, total = self._read()
        return errors / total

    def stats_dict(self) -> dict:
        return {"char_error_rate": self.char_error_rate()}


def _nothing():
    return None


def round_up(val: int, unit: int) -> int:
    """Reference quirk kept: an exact multiple is bumped a full unit (round_up(256, 256) == 512)."""
    return (val // unit + 1) * unit


def ctc_input_and_target_compatible(input_len: int, target) -> bool:
    t = target.tolist() if isinstance(target, torch.Tensor) else list(target)
    need = max(1, len(t)) + sum(1 for i in range(1, len(t)) if t[i - 1] == t[i])
    return input_len >= need


def line_output_width(line_height: int, line_width: int, output_height: int = 64) -> int:
    """Width rule of hiertext.py:288-292: scale with the height, at least 10 (never zero-width), at most 800 (bounds batch memory)."""
    return min(800, max(10, int(output_height * (line_width / line_height))))


def collate_plan(widths, text_seqs, pad_to: int | None = None):
    """The batch rule of train_rec.py:248-304 without the pixels, for every collate of this package: per-sample image widths and
    ``text_seq``s -> (padded width, kept positions, {"text_seq", "text_len", "image_width"} host tensors of the kept samples).  The widths
    are bucketed over every sample (``round_up`` quirk included), then the samples the CTC loss cannot align are dropped.
    ``pad_to`` (extension for the data-parallel path, default None = the reference's behaviour): pad the width at least to this bucket width,
    so that every rank of a step runs the same sequence length (sampler.WidthBucketedDistributedSampler)."""
    wmax = round_up(max(widths), 256)
    if pad_to is not None:
        wmax = max(wmax, int(pad_to))
    lmax = round_up(max(t.shape[0] for t in text_seqs), 64)
    keep = [k for k, t in enumerate(text_seqs) if ctc_input_and_target_compatible(widths[k] // 4, t)]
    n = len(keep)
    text = torch.zeros(n, lmax, dtype=torch.int32)
    tl = torch.zeros(n, dtype=torch.int64)
    iw = torch.zeros(n, dtype=torch.int64)
    for i, k in enumerate(keep):
        L = text_seqs[k].shape[0]
        text[i, :L] = text_seqs[k]
        tl[i], iw[i] = L, widths[k]
    return wmax, keep, {"text_seq": text, "text_len": tl, "image_width": iw}


def collate_samples(samples: list[dict], pad_to: int | None = None) -> dict:
    """list of {'image': (1,64,w) float, 'text_seq': (L,) int32} -> padded batch dict (train_rec.py:248-304); ``pad_to``: see ``collate_plan``."""
    wmax, keep, meta = collate_plan([s["image"].shape[-1] for s in samples], [s["text_seq"] for s in samples], pad_to)
    image = torch.zeros(len(keep), 1, samples[keep[0]]["image"].shape[1] if keep else 64, wmax, dtype=torch.float32)
    for i, k in enumerate(keep):
        image[i, :, :, :samples[k]["image"].shape[-1]] = samples[k]["image"]
    return {"image": image, **meta}
