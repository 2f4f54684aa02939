"""Class thinking tags ('.', bracket classes, escaped punctuation): tag sets and generators
shared by tests/test_class_tags.py (CPU) and tests/test_gpu_class_tags.py (GPU).

The element tables used to build inputs come from Python's ``re`` itself, never from the
native parser, so a generator cannot inherit a parser bug.
"""
from __future__ import annotations

import random
import re
from typing import List, Sequence

# the first seven run everywhere; the last one ('.' can swallow the '>' of the shorter tag) is
# for the ambiguous-window tests only
TAG_SETS = [
    ["a.b"],
    ["think", "t[0-9]"],
    ["x[^y]z", "xb"],
    ["r\\.s", "think", "th.nk", "reason[a-z]"],
    ["a[.]b", "a.b", "q[^a-z]"],
    ["abcdefghijklm.op[0-9]rs", "abcdefghijklmnop.", "think"],  # class positions inside and past byte 16
    ["t[0-9][0-9]", "note\\.x", "n[a-c-]te"],
    ["a.", "a"],
]
CLEAN_SETS = TAG_SETS[:7]
AMBIGUOUS_SET = TAG_SETS[7]

PLAIN = "abxyzt5. \n"
# uncased non-ASCII only: Python's IGNORECASE folds a few code points onto ASCII letters and
# compares cased non-ASCII captures case-insensitively; the native path does neither (README,
# "Semantics decisions")
WIDE = ["日", "→", "😀", "\u00a0", "\u2028"]

_ELEM = re.compile(r"\\.|\[\^?(?:\\.|[^\]\\])+\]|.", re.S)


def elements(tag: str) -> List[str]:
    """The tag's elements as regex source strings (one code point each)."""
    out = _ELEM.findall(tag)
    assert "".join(out) == tag
    return out


def is_class(elem: str) -> bool:
    return elem == "." or elem.startswith("[")


def accepted_ascii(elem: str, flags: int = 0) -> List[str]:
    return [chr(b) for b in range(128) if re.fullmatch(elem, chr(b), re.I | flags)]


def instance(rng: random.Random, tag: str, wide_p: float = 0.0) -> str:
    """A text the tag matches: class elements drawn from their own table, restricted to
    printable ASCII without '<' and '>' (or, with probability wide_p where the element
    accepts them, an uncased non-ASCII code point), in random case."""
    out = []
    for el in elements(tag):
        if not is_class(el):
            c = el[-1]
        elif wide_p and rng.random() < wide_p and re.fullmatch(el, "日", re.I):
            c = rng.choice(WIDE)
        else:
            c = rng.choice([c for c in accepted_ascii(el) if " " <= c <= "~" and c not in "<>"])
        out.append(c.upper() if rng.random() < 0.5 else c.lower())
    return "".join(out)


def plain_run(rng: random.Random, lo: int = 0, hi: int = 12) -> str:
    return "".join(rng.choice(PLAIN) for _ in range(rng.randint(lo, hi)))


def clean_pieces(rng: random.Random, tags: Sequence[str], n: int) -> List[str]:
    """Pieces of a clean stream: plain runs, well-formed open and close tags, and proper
    prefixes of a tag's source text followed by at least 8 plain bytes.  No candidate '<' of
    the concatenation is suspect (the tests assert that with the shared suspect function)."""
    out = []
    for _ in range(n):
        r = rng.random()
        tag = rng.choice(list(tags))
        if r < 0.4:
            out.append(plain_run(rng, 1, 12))
        elif r < 0.8:
            out.append(("<" if rng.random() < 0.55 else "</") + instance(rng, tag) + ">")
        else:
            src = ("<" if rng.random() < 0.5 else "</") + tag + ">"
            out.append(src[:rng.randint(1, len(src) - 1)] + plain_run(rng, 8, 12))
    return out


def fuzz_pieces(rng: random.Random, tags: Sequence[str], n: int) -> List[str]:
    """Adversarial pieces: instantiated tags with uncased non-ASCII at accepting positions,
    partial prefixes (of the source text and of instances), stray '<', '>', '/', newlines."""
    out = []
    for _ in range(n):
        r = rng.random()
        tag = rng.choice(list(tags))
        if r < 0.3:
            out.append(("<" if rng.random() < 0.55 else "</") + instance(rng, tag, 0.3) + ">")
        elif r < 0.45:
            src = rng.choice(["<", "</"]) + (tag if rng.random() < 0.5 else instance(rng, tag, 0.3)) + ">"
            out.append(src[:rng.randint(1, len(src))])
        elif r < 0.6:
            body = instance(rng, tag, 0.3)
            out.append(body[rng.randint(0, len(body)):] + ">")
        elif r < 0.8:
            out.append(rng.choice(["<", "<", ">", "/", "\n", "</", ">>", "<<"]))
        elif r < 0.9:
            out.append(rng.choice(WIDE))
        else:
            out.append(plain_run(rng, 1, 5))
    return out


def split_chars(rng: random.Random, text: str, lo: int = 1, hi: int = 40) -> List[str]:
    out, i = [], 0
    while i < len(text):
        k = rng.randint(lo, hi)
        out.append(text[i:i + k])
        i += k
    return out
