"""Variable-width thinking tags ('?', '|', groups): tag sets and generators shared by
tests/test_variant_tags.py (CPU) and tests/test_gpu_variant_tags.py (GPU)
(``variants=True``, ``runtime.native_variant_tags``, with ``classes``).

The expansion used to build inputs (``expand``) is a parser of its own, written against the
grammar of the README ("Variable-width thinking tags") and checked against Python's ``re``
where it is used — never the native parser, so a generator cannot inherit a parser bug.  Class positions are filled from ASCII;
the *ambiguous* fillers put '<', '>', '/', a newline or an uncased non-ASCII character there.
Never emitted: the Kelvin sign, long s and U+0130 (Python folds them onto ASCII letters, the
native matchers do not) and a cased non-ASCII character at a class position.
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import class_tag_cases as C

KW = dict(classes=True, variants=True)
MIXED_KW = dict(classes=True, unicode=True, mixed=True, variants=True)

MAX_ROWS = 16
MAX_SRC = 61

# (tag, its rows in priority order)
ROW_TABLE = [
    ("thoughts?", ["thoughts", "thought"]),
    ("think(ing)?", ["thinking", "think"]),
    ("a(b|c)?d", ["abd", "acd", "ad"]),
    ("a?b?c", ["abc", "ac", "bc", "c"]),
    ("x|y(?:z)?", ["x", "yz", "y"]),
    ("t[0-9]?", ["t[0-9]", "t"]),
    ("reason(?:ing)?", ["reasoning", "reason"]),
    ("step[0-9]?|phase", ["step[0-9]", "step", "phase"]),
    ("a(b(c|d)?|e)f", ["abcf", "abdf", "abf", "aef"]),
    ("(a|a)b", ["ab"]),
    ("th.nk(s)?", ["th.nks", "th.nk"]),
    ("r\\.s?", ["r\\.s", "r\\."]),
]

# the sets of the GPU tests' clean streams: no tag of a set puts '<', '>' or a non-ASCII byte
# on a class position that accepts it
CLEAN_SETS = [["think(ing)?", "thoughts?"], ["t[0-9]?", "reason(?:ing)?"], ["step[0-9]?|phase"]]
# the optional element on bytes 15/16 of the matcher's 16-byte window ("<" + 14 letters + o? + p)
EDGE_TAG = "abcdefghijklmno?p"
MIXED_SET = ["réflexions?", "思(考)?"]


# ---------------------------------------------------------------- the expansion
class _P:
    def __init__(self, s: str):
        self.s, self.i = s, 0

    def peek(self) -> str:
        return self.s[self.i] if self.i < len(self.s) else ""


def _dedup(rows):
    out = []
    for r in rows:
        if r not in out:
            out.append(r)
    return out


def _alt(p: _P) -> List[Tuple[str, ...]]:
    rows = list(_seq(p))
    while p.peek() == "|":
        p.i += 1
        rows += _seq(p)
    return _dedup(rows)


def _seq(p: _P) -> List[Tuple[str, ...]]:
    rows: List[Tuple[str, ...]] = [()]
    while p.peek() not in ("", "|", ")"):
        if p.peek() == "(":
            p.i += 1
            if p.s.startswith("?:", p.i):
                p.i += 2
            atom = _alt(p)
            assert p.peek() == ")", p.s
            p.i += 1
        else:
            m = C._ELEM.match(p.s, p.i)
            p.i = m.end()
            atom = [(m.group(0),)]
        if p.peek() == "?":
            p.i += 1
            atom = _dedup(atom + [()])
        rows = _dedup([a + b for a in rows for b in atom])
    return rows


def expand(tag: str) -> List[Tuple[str, ...]]:
    """The tag's rows in regex priority order, each a tuple of element source strings (present
    before absent, left alternative before right, the leftmost choice most significant)."""
    p = _P(tag)
    rows = _alt(p)
    assert p.i == len(tag), tag
    return rows


def row_text(row: Sequence[str]) -> str:
    return "".join(e.lower() if len(e) == 1 else e for e in row)


def set_ok(tags: Sequence[str]) -> bool:
    """Inside the subset by this module's own expansion: at most 16 rows, none empty, each
    beginning with a literal, no two equal rows under different source texts, sources of at
    most 61 bytes."""
    seen = {}
    n = 0
    for t in dict.fromkeys(x.lower() for x in tags):
        if len(t.encode()) > MAX_SRC:
            return False
        for r in expand(t):
            if not r or C.is_class(r[0]):
                return False
            key = row_text(r)
            if seen.setdefault(key, t) != t:
                return False
            n += 1
    return 0 < n <= MAX_ROWS


# ---------------------------------------------------------------- random tags
LETTERS = "abtx"


def _rand_expr(rng: random.Random, depth: int, first: bool) -> str:
    """A concatenation of 1-3 atoms; `first`: it begins the tag, so it begins with a letter that
    is not optional (every row non-empty and literal-first by construction)."""
    out = []
    for k in range(rng.randint(1, 3)):
        lead = first and k == 0
        r = rng.random()
        if lead or r < 0.5:
            atom = rng.choice(LETTERS)
        elif r < 0.6:
            atom = "."
        elif r < 0.7:
            atom = "[0-9]"
        elif depth < 2:
            alts = [_rand_expr(rng, depth + 1, False) for _ in range(rng.randint(1, 2))]
            atom = ("(" if rng.random() < 0.5 else "(?:") + "|".join(alts) + ")"
        else:
            atom = rng.choice(LETTERS)
        if not lead and rng.random() < 0.4:
            atom += "?"
        out.append(atom)
    return "".join(out)


def random_tag(rng: random.Random) -> str:
    """A tag of the grammar: literals, '.', '[0-9]', '?', '|', capturing and '(?:' groups nested
    two deep; every top-level alternative begins with a mandatory letter."""
    return "|".join(_rand_expr(rng, 0, True) for _ in range(1 if rng.random() < 0.7 else 2))


def random_set(rng: random.Random) -> List[str]:
    """One or two tags, inside the subset by construction (set_ok of this module's expansion)."""
    while True:
        tags = [random_tag(rng) for _ in range(rng.randint(1, 2))]
        if set_ok(tags):
            return tags


# ---------------------------------------------------------------- texts
AMBIGUOUS = ["<", ">", "/", "\n"] + C.WIDE


def row_instance(rng: random.Random, row: Sequence[str], ambiguous: Sequence[str] = (), p: float = 0.0) -> str:
    out = []
    for el in row:
        if not C.is_class(el):
            c = el[-1]
        elif ambiguous and rng.random() < p:
            out.append(rng.choice(list(ambiguous)))
            continue
        else:
            c = rng.choice([c for c in C.accepted_ascii(el) if " " <= c <= "~" and c not in "<>"])
        out.append(c.upper() if rng.random() < 0.5 else c.lower())
    return "".join(out)


def near_miss(name: str) -> str:
    """The name with its last character changed, or one more, or one fewer."""
    return name[:-1] + "~" if len(name) > 1 else name + "~"


def fuzz_text(rng: random.Random, tags: Sequence[str], rows: Sequence[Sequence[str]], n: int) -> str:
    """n pieces: opens and closes of row instances in both cases (some with '<', '>', '/', a
    newline or a non-ASCII character at a class position), near misses, prefixes of a source
    text and of an instance, stray punctuation, plain runs."""
    out = []
    for _ in range(n):
        r = rng.random()
        row = rng.choice(list(rows))
        lead = "<" if rng.random() < 0.55 else "</"
        if r < 0.4:
            out.append(lead + row_instance(rng, row, AMBIGUOUS, 0.15) + ">")
        elif r < 0.5:
            out.append(lead + near_miss(row_instance(rng, row)) + ">")
        elif r < 0.65:
            src = lead + (rng.choice(list(tags)) if rng.random() < 0.5 else row_instance(rng, row)) + ">"
            out.append(src[:rng.randint(1, len(src))])
        elif r < 0.8:
            out.append(rng.choice(["<", "<", ">", "/", "\n", "</", ">>", "s>", "ing>"]))
        else:
            out.append(C.plain_run(rng, 1, 6))
    return "".join(out)


def all_rows(tags: Sequence[str]) -> List[Tuple[str, ...]]:
    return [r for t in tags for r in expand(t)]


def clean_form(rng: random.Random, rows: Sequence[Sequence[str]]) -> str:
    """A whole open or close of a row: lower, upper or mixed case, or a near miss."""
    name = row_instance(rng, rng.choice(list(rows)))
    r = rng.random()
    name = name.lower() if r < 0.3 else name.upper() if r < 0.55 else name if r < 0.85 else near_miss(name.lower())
    return ("<" if rng.random() < 0.55 else "</") + name + ">"


def clean_pieces(rng: random.Random, tags: Sequence[str], n: int, extra: Optional[Sequence[str]] = None) -> List[str]:
    """Pieces of a clean stream: plain runs, whole tag forms of every row, and proper prefixes
    of a tag's source text or of an instance followed by at least 8 plain bytes."""
    rows = all_rows(tags)
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            out.append(C.plain_run(rng, 1, 12))
        elif r < 0.8:
            out.append(clean_form(rng, rows))
        elif extra and r < 0.85:
            out.append(rng.choice(list(extra)))
        else:
            name = rng.choice(list(tags)) if rng.random() < 0.5 else row_instance(rng, rng.choice(rows))
            src = ("<" if rng.random() < 0.5 else "</") + name + ">"
            out.append(src[:rng.randint(1, len(src) - 1)] + C.plain_run(rng, 8, 12))
    return out
