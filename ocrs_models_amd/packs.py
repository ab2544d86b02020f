"""The per-step weight-fragment pack table of the three model drivers (models.py::_DetRun, recognition.py::_RecRun, layout.py::_LayoutRun).

A run lists the packs of its step as ``PackRow``s (its ``pack_rows()``); ``PackTable`` lays them out in one buffer and writes the int64 tables
``ocrs_pack_frags_multi`` reads; ``cached_table`` keeps the table on the module while the parameter storage stays in place.  A layer asks the
table with the SAME ``PackRow``: ``row.key()`` is the only lookup key and holds every field that changes the packed bytes.
"""
from __future__ import annotations

from types import MappingProxyType
from typing import NamedTuple

import torch

from ._lib import lib, ptr


class PackRow(NamedTuple):
    """One ocrs_pack_frags job: A[m][k] = src[offset + (k / K2) * s1 + (k % K2) * s2 + m * sm] (mode 0 / 2; include/ocrs_hip.h), packed as
    MFMA A-operand fragments of dtype code dt.  mode 2: pre-split hi / lo bf16 planes (twice the bytes)."""
    src: torch.Tensor
    dt: int
    mode: int
    K: int
    M: int
    K2: int
    s1: int
    s2: int
    sm: int
    offset: int = 0  # elements (fp32) into src

    def src_ptr(self):
        return self.src.data_ptr() + 4 * self.offset

    def key(self):
        return (self.src_ptr(), self.dt, self.mode, self.K, self.M, self.K2, self.s1, self.s2, self.sm)


def fwd_row(w, dt, mode=0):
    """A[m][k] = W[m][k], W [M][K] row-major: a Linear / 1x1 conv forward"""
    M, K = w.shape[0], w.shape[1]
    return PackRow(w, dt, mode, K, M, K, 0, 1, K)


def dgrad_row(w, dt, mode=0):
    """A[m][k] = W[k][m], W [K][M] row-major: the input gradient of the same layer"""
    K, M = w.shape[0], w.shape[1]
    return PackRow(w, dt, mode, K, M, K, 0, M, 1)


def conv_row(w, dt):
    """W[cout][cin][kh][kw] -> A[m = cout][k = (tap, cin)]"""
    co, ci, kh, kw = w.shape
    nt = kh * kw
    return PackRow(w, dt, 0, nt * ci, co, ci, 1, nt, ci * nt)


def conv_dgrad_row(w, dt):
    """A[m = cin][k = (tap', cout)] = W[cout][cin][ntaps - 1 - tap']"""
    co, ci, kh, kw = w.shape
    nt = kh * kw
    return PackRow(w, dt, 0, nt * co, ci, co, -1, ci * nt, nt, nt - 1)


def _nbytes(row, frag_bytes):
    return frag_bytes(row.K, row.M, row.dt) * (2 if row.mode == 2 else 1)


def pack_one(row, device):
    """The fragments of one row by a single ocrs_pack_frags launch."""
    L = lib()
    out = torch.empty(_nbytes(row, L.pack_frags_bytes), dtype=torch.uint8, device=device)
    L.pack_frags(row.src_ptr(), row.mode, row.K, row.M, row.K2, row.s1, row.s2, row.sm, ptr(out), row.dt)
    return out


class PackTable:
    """rows -> one uint8 buffer (each pack at a 256-byte offset), the views into it by row key, and per fragment dtype (ascending) the device
    table int64 [n][9] = {src, out, mode, K, M, K2, s1, s2, sm} of its rows in the given order.  frag_bytes(K, M, dt): ocrs_pack_frags_bytes."""

    def __init__(self, rows, device, frag_bytes=None):
        rows = list(rows)
        sizes = [_nbytes(r, frag_bytes or lib().pack_frags_bytes) for r in rows]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + (n + 255) // 256 * 256)
        self.buf = torch.empty(offs[-1], dtype=torch.uint8, device=device)
        tables = []  # (device table, its row count, max_frag_threads, dt)
        for dt in sorted({r.dt for r in rows}):
            sel = [(r, o) for r, o in zip(rows, offs) if r.dt == dt]
            table = torch.tensor([[r.src_ptr(), self.buf.data_ptr() + o, r.mode, r.K, r.M, r.K2, r.s1, r.s2, r.sm] for r, o in sel],
                                 dtype=torch.int64).to(device)
            tables.append((table, len(sel), max(((r.K + 31) // 32) * ((r.M + 15) // 16) * 64 for r, _ in sel), dt))
        self.tables = tuple(tables)
        # (plain containers of tensors: a module that carries a cached table still deep-copies and pickles)
        self.views = {r.key(): self.buf[o:o + n] for r, o, n in zip(rows, offs, sizes)}

    def launch(self):
        for table, n, max_frag_threads, dt in self.tables:
            lib().pack_frags_multi(ptr(table), n, max_frag_threads, dt)

    def get(self, row):
        return self.views.get(row.key())

    def __getitem__(self, row):  # (a miss is a KeyError: for routes that have no unpacked alternative)
        return self.views[row.key()]

    def fetch(self, row, device):
        """the pack of row: from the table or, for a row it does not hold (outside a full forward), packed here"""
        hit = self.views.get(row.key())
        return hit if hit is not None else pack_one(row, device)


EMPTY = PackTable((), "cpu")  # a run's table outside a full forward: every lookup misses; shared by all runs, hence immutable
EMPTY.views = MappingProxyType({})


def cached_table(mod, key, build_rows, device, frag_bytes=None):
    """mod._pack_cache = (key, table): the table of build_rows(), rebuilt when key (mode switches + parameter addresses) changes"""
    cache = getattr(mod, "_pack_cache", None)
    if cache is None or cache[0] != key:
        cache = mod._pack_cache = (key, PackTable(build_rows(), device, frag_bytes))
    return cache[1]
