"""Record the reference's WebLayout items for the fixture pages (BUILD container only; imports the reference through tools/ref_import.py).

    python tools/gen_weblayout_goldens.py

Reads tests/golden/weblayout/*.json, writes tests/golden/weblayout.npz.  One entry per (file, normalize_coords, padded_size, mode), keyed by
``key()`` below and independent of the directory order: an fp32 array (W, 6) = the item's input (W, 4) next to its labels (W, 2).  Modes:
``fixed`` = randomize=False; ``s<seed>j<max_jitter>`` = randomize=True with ``torch.manual_seed(seed)`` called immediately before that one
``__getitem__``.  Only these recorded outputs and the JSON inputs are committed.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PAGES = os.path.join(ROOT, "tests", "golden", "weblayout")
OUT = os.path.join(ROOT, "tests", "golden", "weblayout.npz")

NORMALIZE = (False, True)
PADDED = (None, 1, 16, 64)
SEEDS = (0, 1234)
JITTERS = (10, 25)


def modes():
    return [("fixed", None, None)] + [(f"s{s}j{j}", s, j) for s in SEEDS for j in JITTERS]


def key(name, normalize, padded, mode):
    return f"{name}|n{int(normalize)}|p{padded}|{mode}"


def main():
    from ref_import import import_reference

    import_reference()
    from ocrs_models.datasets.web_layout import WebLayout

    out = {}
    names = sorted(f for f in os.listdir(PAGES) if f.endswith(".json"))
    for name in names:
        for normalize in NORMALIZE:
            for padded in PADDED:
                for mode, seed, jitter in modes():
                    ds = WebLayout(PAGES, randomize=seed is not None, padded_size=padded, normalize_coords=normalize,
                                   **({} if jitter is None else {"max_jitter": jitter}))
                    ds._files = [name]  # (the split rule is tested on its own; every page is recorded)
                    if seed is not None:
                        torch.manual_seed(seed)
                    x, y = ds[0]
                    out[key(name, normalize, padded, mode)] = torch.cat([x, y], dim=1).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"{len(out)} items of {len(names)} pages -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
