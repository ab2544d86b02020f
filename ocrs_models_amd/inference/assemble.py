"""Result assembly: host lists and a ``Decoded`` record -> the result dicts of the drivers.  Pure list work; nothing here touches the GPU."""
from __future__ import annotations


def assemble_results(rec, words: list, lines=None, reading=None, chain=None) -> list[dict]:
    """``rec``: the ``decode.Decoded`` of the crops (quad order); ``words``: the word quads as lists.  Without ``lines`` one dict per word.
    ``lines`` = ``(line quads, word_order, line_offsets)`` as host lists cut to the line count: one dict per line, line l holding the words
    ``word_order[line_offsets[l]:line_offsets[l + 1]]`` in chain order.  ``reading`` = ``(line_order, new_block, page_offs)`` (with ``lines``):
    the dicts in reading order -- position k holds line ``line_order[k]`` -- each with ``"block"``, counted from 0 on every page, the lines
    of page p being the positions ``page_offs[p]:page_offs[p + 1]``.  ``chain`` = ``(knots, line_dims)`` (with ``lines``; chain crops,
    DESIGN.md §21): the ``[L, R]`` knots of the word at every chain position and ``[S, H]`` of every line; line dicts gain ``"spine"``, the
    2n knots of their words in chain order, and ``"height"``, H.

    Keys, in this order (the dicts are printed as JSON lines): ``quad``, ``text``, for lines ``words``, ``spine``, ``height``; with characters ``char_quads``,
    ``char_log_probs``; ``log_prob`` and ``lm_score`` where the record has them; with characters, for lines, ``word_chars`` and
    ``word_texts``; ``block`` last."""
    if lines is None:
        quads, members = words, None
    else:
        quads, word_order, offs = lines
        members = [word_order[a:b] for a, b in zip(offs, offs[1:])]
    out = []
    for i, quad in enumerate(quads):
        d = {"quad": quad, "text": rec.texts[i]}
        if members is not None:
            d["words"] = [words[w] for w in members[i]]
        if chain is not None:
            d["spine"] = [pt for pair in chain[0][offs[i]:offs[i + 1]] for pt in pair]
            d["height"] = chain[1][i][1]
        if rec.chars is not None:
            d.update(rec.chars[i])
        if rec.log_probs is not None:
            d["log_prob"] = rec.log_probs[i]
        if rec.lm_scores is not None:
            d["lm_score"] = rec.lm_scores[i]
        if rec.word_ranges is not None:
            d["word_chars"] = [rec.word_ranges[w] for w in members[i]]
            d["word_texts"] = [d["text"][a:b] for a, b in d["word_chars"]]
        out.append(d)
    if reading is None:
        return out
    line_order, new_block, page_offs = reading
    read = []
    for a, b in zip(page_offs, page_offs[1:]):
        block = -1
        for k in range(a, b):
            block += 1 if (new_block[k] or k == a) else 0
            read.append({**out[line_order[k]], "block": block})
    return read
