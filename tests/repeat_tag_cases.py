"""Unbounded repetition in thinking tags — ``+``, ``*`` and ``{m,}`` after one element — tag sets,
tables and generators shared by tests/test_repeat_tags.py (CPU) and tests/test_gpu_repeat_tags.py
(GPU) (``repeat=True``, ``runtime.native_repeat_tags``, with ``classes``, ``variants`` and
``extended``).

A row's open-ended element — "this element, once or more" — is listed with a ``+`` after it
(``_qmx.tagset_rows``).  U+0663 (ARABIC-INDIC DIGIT THREE) is a digit in every Unicode version,
U+00A0 a space, 思 an uncased letter.
"""
from __future__ import annotations

import random
from typing import List, Sequence

KW = dict(classes=True, variants=True, extended=True, repeat=True)
MIXED_KW = dict(classes=True, unicode=True, mixed=True, variants=True, extended=True, repeat=True)
OFF_KW = dict(classes=True, variants=True, extended=True)
ROWS = 4  # kRepeatRows (qmx_text.h)

D3, NBSP = "٣", " "

NEEDS = "tag needs regex semantics: "
GROUP = "tag repeats a group without a bound (runs with --impl python): "
OVERLAP = ("tag repeats an element that also accepts what can follow the run, so the run's end depends on the "
           "regex's backtracking (runs with --impl python): ")
EMPTY_ROW = "tag has an empty alternative: "
CLASS_FIRST = "tag has an alternative that begins with a class: "
TOO_MANY = "thinking tags expand to more than 16 rows: "
SAME_PATTERN = "two thinking tags give the same pattern under different source texts: "
TOO_LONG = "unsupported tag length: "


def _rows(stem: str, x: str, lo: int, hi: int, tail: str = "") -> List[str]:
    """stem + x * n + tail for n = hi ... lo, the longest open-ended at its last copy"""
    return [stem + x * n + ("+" if n == hi else "") + tail for n in range(hi, lo - 1, -1)]


# (tag, its rows in priority order, six characters drawn from it for the determinism sweep)
ACCEPTED = [
    ("step\\d+", _rows("step", "\\d", 1, 4), "step19"),
    ("think\\s*", _rows("think", "\\s", 0, 4), "thinK "),
    ("thought_\\d+", _rows("thought_", "\\d", 1, 4), "tho_g7"),
    ("hm+", _rows("h", "m", 1, 4), "hmHM x"),
    ("a\\d+[a-z]+", [r + s for r in _rows("a", "\\d", 1, 4) for s in _rows("", "[a-z]", 1, 4)], "a1zA9_"),
    ("v\\d+\\.\\d+", [r + s for r in _rows("v", "\\d", 1, 4, "\\.") for s in _rows("", "\\d", 1, 4)], "v12.V-"),
    ("step\\d{2,}", _rows("step", "\\d", 2, 5), "steP05"),
    ("a{2,}b", _rows("", "a", 2, 5, "b"), "abAB c"),
    ("s\\d+", _rows("s", "\\d", 1, 4), "sS07 x"),
    ("x[ab]*y?", [r + y for r in _rows("x", "[ab]", 0, 4) for y in ("y", "")], "xabyAY"),
    ("n[^0-9x]+x", _rows("n", "[^0-9x]", 1, 4, "x"), "nN1a x"),
    ("a{0,}b", _rows("", "a", 0, 3, "b"), "abAB c"),
]

# (tag, message with the key on); with the key off every one of them is NEEDS + tag
REFUSED = [
    ("(ab)+", GROUP), ("(ab)*", GROUP), ("(?:a|b){2,}", GROUP), ("x(a\\d+)+", GROUP), ("(a?)*", GROUP),
    ("é+", NEEDS), ("a思*", NEEDS),
    ("a+?", NEEDS), ("a*?", NEEDS), ("a{2,}?", NEEDS), ("a++", NEEDS), ("a+*", NEEDS), ("a+{2}", NEEDS), ("a*+", NEEDS),
    ("a{2,}{2}", NEEDS), ("a{2,}+", NEEDS), ("a{62,}", NEEDS), ("a{,}", NEEDS), ("+a", NEEDS), ("a|*", NEEDS),
    ("think.*", OVERLAP), ("a.+b", OVERLAP), ("a.+", OVERLAP), ("a\\d+5", OVERLAP), ("\\w+_x", OVERLAP), ("\\d+\\w+", OVERLAP),
    ("a\\d+\\d", OVERLAP), ("am+m", OVERLAP), ("am+M", OVERLAP), ("a[a-c]+(x|c)", OVERLAP), ("a\\d+(x|\\w)?", OVERLAP),
    ("a[^b]+", OVERLAP), ("n[^\\d]+\\d", OVERLAP), ("a\\w+[^x]", OVERLAP), ("a\\s*\\w", OVERLAP), ("x(a\\d+){2}1", OVERLAP),
    ("\\d+x", CLASS_FIRST), ("a*", EMPTY_ROW), ("\\s*", CLASS_FIRST), ("[ab]+x", CLASS_FIRST),
    ("a\\d+[a-z]+x*", TOO_MANY), ("a{59,}", TOO_LONG), ("a" * 46 + "\\w+", TOO_LONG),
]

# the issue's differential sets: (tags, keywords, stems, what a run is made of)
DIFF_SETS = [
    (["think", "step\\d+"], KW, ["step", "think", "STEP", "Step"], "0123456789"),
    (["think\\s*"], KW, ["think", "THINK", "thin"], " \n\t "),
    (["hm+", "h\\d+"], KW, ["h", "H", "hm", "HM"], "mM0123456789"),
    (["v\\d+\\.\\d+"], KW, ["v", "V", "v1."], "0123456789."),
    (["思\\d+"], MIXED_KW, ["思", "思1"], "0123456789"),
]
MAX_RUN = 12


def _name(rng: random.Random, stems: Sequence[str], run: str) -> str:
    body = "".join(rng.choice(run) for _ in range(rng.randint(0, MAX_RUN)))
    if body and rng.random() < 0.12:  # a non-ASCII digit (or space) inside the run
        k = rng.randrange(len(body))
        body = body[:k] + (NBSP if " " in run else D3) + body[k + 1:]
    return rng.choice(list(stems)) + body


def diff_text(rng: random.Random, n: int, stems: Sequence[str], run: str) -> str:
    """n pieces: opens and closes of a stem and a run of 0-12 run characters (an ARABIC-INDIC digit
    among them), right closes (the last open's name again, maybe in another ASCII case), wrong
    closes, tag heads without their '>', the delimiters and plain text.  Nesting comes from the
    order; no piece but a name holds a run character, so no run passes MAX_RUN + a stem."""
    out, opened = [], []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            opened.append(_name(rng, stems, run))
            out.append("<" + opened[-1] + ">")
        elif r < 0.5 and opened:
            name = opened.pop(rng.randrange(len(opened)))
            out.append("</" + (name.upper() if rng.random() < 0.3 else name) + ">")
        elif r < 0.62:
            out.append("</" + _name(rng, stems, run) + ">")
        elif r < 0.72:
            out.append(rng.choice(["<", "</"]) + _name(rng, stems, run))
        elif r < 0.9:
            out.append(rng.choice(["<", ">", "/", "\n", " ", "</", ">>", "x", "-"]))
        else:
            out.append(rng.choice(["<think>", "</think>", "<think", "text", "<" + stems[0] + "\\d+>", "<" + stems[0] + "\\"]))
    return "".join(out)


# ---------------------------------------------------------------- GPU streams
GPU_TAGS = ["think", "step\\d+"]


def clean_pieces(rng: random.Random, n: int, stem: str = "step", max_digits: int = ROWS) -> List[str]:
    """Pieces of a stream of ["think", stem + "\\d+"] whose runs have 1 to max_digits digits: whole
    opens and closes in any ASCII case (nesting comes from the order), near misses, plain runs and
    heads followed by plain text."""
    out = []
    for _ in range(n):
        name = stem + "".join(rng.choice("0123456789") for _ in range(rng.randint(1, max_digits)))
        r = rng.random()
        if r < 0.2:
            name = name.upper()
        elif r < 0.3:
            name = rng.choice(["think", "THINK", stem, stem + "x", stem[:-1] + "1", stem + "1x"])
        if r < 0.75:
            out.append(("<" if rng.random() < 0.55 else "</") + name + ">")
        elif r < 0.9:
            out.append("".join(rng.choice("abxyz. \n") for _ in range(rng.randint(1, 12))))
        else:
            src = rng.choice(["<", "</"]) + rng.choice([name, stem + "\\d+"]) + ">"
            out.append(src[:rng.randint(1, len(src) - 1)] + " plain text")
    return out
