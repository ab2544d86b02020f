"""Build the character language model of DESIGN.md §19 from a dataset's line texts, on the host:

    python -m ocrs_models_amd.char_lm hiertext DATA_DIR OUT.npz [--order N] [--max-images N]

counts the character n-grams (N = 1..3, default 3) of the HierText training split's text lines -- the lines ``HierTextRecognition`` selects
(``datasets.hiertext_text_lines``: the lines file, generated from the annotations if it is missing, and its ``--max-images`` cut; the crops
are not read, so a line that the store would drop for an empty crop still counts), encoded with ``text.encode_text`` over
``DEFAULT_ALPHABET`` -- smooths them by interpolated Witten-Bell (``text.CharLM``) and writes the model as one ``.npz`` that
``text.CharLM.load`` and ``eval_detection --lm`` read.  Counting and smoothing are numpy float64 on the host: no GPU is used.
"""
from __future__ import annotations

import json
from argparse import ArgumentParser

from .datasets import hiertext_text_lines
from .text import DEFAULT_ALPHABET, LM_MAX_ORDER, CharLM


def hiertext_texts(root_dir: str, max_images=None) -> list:
    """the texts of the training split's lines, in the lines file's order"""
    return [json.loads(line)["text"] for line in hiertext_text_lines(root_dir, True, max_images)[3]]


def main(argv=None):
    parser = ArgumentParser(description="Build a character n-gram language model for the beam search's lm= keyword.")
    parser.add_argument("dataset", choices=["hiertext"])
    parser.add_argument("data_dir")
    parser.add_argument("out", help="the .npz file to write")
    parser.add_argument("--order", type=int, default=3, metavar="N", help=f"n-gram order, 1..{LM_MAX_ORDER} (default 3)")
    parser.add_argument("--max-images", type=int, default=None, metavar="N", help="use only the first N lines of the lines file")
    args = parser.parse_args(argv)
    if not 1 <= args.order <= LM_MAX_ORDER:
        parser.error(f"--order must be in 1..{LM_MAX_ORDER}")
    texts = hiertext_texts(args.data_dir, args.max_images)
    model = CharLM.from_texts(texts, DEFAULT_ALPHABET, args.order)
    model.save(args.out)
    print(json.dumps({"lines": len(texts), "characters": sum(len(t) for t in texts), "order": model.order, "classes": model.log_probs.shape[0],
                      "out": args.out}))


if __name__ == "__main__":
    main()
