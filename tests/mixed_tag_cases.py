"""Shared inputs of the mixed thinking tag tests (tests/test_mixed_tags.py on the CPU,
tests/test_gpu_mixed_tags.py on the GPU): tag sets that hold class elements and non-ASCII
literals together (``mixed=True``, ``runtime.native_mixed_tags``), and text generators.

The generators build on ``unicode_tag_cases`` (case mixing, look-alikes, alphabets, streams)
and ``class_tag_cases`` (a tag's elements and the texts it matches, taken from Python's ``re``).
Class positions are filled from ASCII; the separate *ambiguous* fillers put a non-ASCII
character, '<' or '>' there.  Never emitted: the Kelvin sign, long s and U+0130 (Python folds
them onto ASCII letters, the native matchers do not), and a cased non-ASCII character at a
class position that is not one of the set's own pair characters (the native strip compares
such a capture byte for byte).
"""
from __future__ import annotations

import random
from typing import List, Sequence

import class_tag_cases as C
import unicode_tag_cases as U

KW = dict(classes=True, unicode=True, mixed=True)

# one 16-tag set: U.SIXTEEN with four tags replaced by class or mixed tags (the opens of the 16
# tags are one MFMA column block, their closes the other: both hold class and pair tags).  A
# class position comes after literals no other tag shares, so a whole tag of the set never puts
# '>' or a non-ASCII byte on another tag's class position.
SIXTEEN = list(U.SIXTEEN)
SIXTEEN[1], SIXTEEN[6], SIXTEEN[9], SIXTEEN[15] = "reas.n", "plan[!?]", "考え.", "ÿz[0-9]"

TAG_SETS = [
    ["th.nk", "思考"],                           # class plus uncased, no fold table
    ["think", "réflexion", "t[0-9]"],            # class and pair in separate tags
    ["réfl.xion", "思[0-9]", "é.", "think"],     # both in one tag, a non-ASCII first element
    ["abcdefghijklmn.я"],                        # class position on byte 15 of the open, я on 16-17
    ["abcdefghijklm思[0-9]"],                    # 思 across the 16-byte window edge
    ["r.flexion", "réflexion"],                  # list order
    ["réflexion", "r.flexion"],
    SIXTEEN,
]
LONG_SETS = TAG_SETS[3:5]

# uncased only (as class_tag_cases.WIDE), plus '<' and '>'
AMBIGUOUS = C.WIDE + ["<", ">"]


def pair_chars(tags: Sequence[str]) -> List[str]:
    """The set's own pair characters, both members."""
    pairs, _ = U.case_rule()
    out = []
    for t in tags:
        for el in C.elements(t):
            if not C.is_class(el) and ord(el[-1]) >= 0x80 and ord(el[-1]) in pairs:
                out += [el[-1].lower(), el[-1].upper()]
    return sorted(set(out))


def instance(rng: random.Random, tag: str, ambiguous: Sequence[str] = (), p: float = 0.0) -> str:
    """A text the tag may match: literals in random case (through ``str.upper``: the pair's
    other member), class positions one accepted printable ASCII byte that is neither '<' nor
    '>' — or, with probability p, one of `ambiguous` (whether the element accepts it or not)."""
    out = []
    for el in C.elements(tag):
        if not C.is_class(el):
            c = el[-1]
            out.append(c.upper() if rng.random() < 0.5 else c.lower())
        elif ambiguous and rng.random() < p:
            out.append(rng.choice(list(ambiguous)))
        else:
            c = rng.choice([c for c in C.accepted_ascii(el) if " " <= c <= "~" and c not in "<>"])
            out.append(c.upper() if rng.random() < 0.5 else c.lower())
    return "".join(out)


def lookalike(t: str) -> str:
    """U.lookalike, but "é" becomes "÷": the same lead byte and uncased — "è" on the class
    position of "r.flexion" would be a cased capture that is no pair character of the set."""
    return t.replace("é", "÷", 1) if "é" in t else U.lookalike(t)


def tag_form(rng: random.Random, tags: Sequence[str], ambiguous: Sequence[str] = (), p: float = 0.0) -> str:
    """An open or a close of a tag of the set: an instance, or (one in seven) a look-alike."""
    t = rng.choice(list(tags))
    name = instance(rng, t, ambiguous, p)
    if rng.random() < 0.15:
        name = lookalike(name.lower())
    return ("<" if rng.random() < 0.55 else "</") + name + ">"


def alphabet(tags: Sequence[str]) -> List[str]:
    """As U.alphabet, of one lower-case instance per tag: the engine's wide alphabet, the
    instances in both cases, look-alikes, opens cut after every byte — and the source texts
    "<tag>" cut after every byte."""
    import engine_harness as H

    rng = random.Random(len(tags))
    inst = [instance(rng, t).lower() for t in tags]
    out = list(H.wide_alphabet(inst))
    for t in inst:
        out += [f"<{t.upper()}>", f"</{t.upper()}>", f"<{t}>", f"</{t}>", f"<{lookalike(t)}>", f"</{lookalike(t)}>",
                f"<{lookalike(t).upper()}>"]
    for t in [i.upper() for i in inst] + list(tags):
        raw = f"<{t}>".encode()
        out += [raw[:k].decode("utf-8", "ignore") for k in range(1, len(raw))]
    return out


def pieces(rng: random.Random, tags: Sequence[str], n: int, alpha: Sequence[str], ambiguous: Sequence[str] = (),
           p: float = 0.0) -> List[str]:
    """n pieces: a quarter tag forms (class positions from ASCII, or `ambiguous` with
    probability p), the rest drawn from the alphabet."""
    return [tag_form(rng, tags, ambiguous, p) if rng.random() < 0.25 else rng.choice(list(alpha)) for _ in range(n)]


def ambiguous_for(tags: Sequence[str]) -> List[str]:
    return AMBIGUOUS + pair_chars(tags)


# ---------------------------------------------------------------- clean streams (GPU)
# Tag sets whose own tags never put '>' or a non-ASCII byte on each other's class positions
# (in the list-order sets "<réflexion>" itself is suspect against "r.flexion")
CLEAN_SETS = TAG_SETS[:5] + [SIXTEEN]
ORDER_SETS = TAG_SETS[5:7]


def clean_form(rng: random.Random, tags: Sequence[str]) -> str:
    """A whole open or close: an instance in lower, upper or mixed case (class positions one
    ASCII byte), or a look-alike of one."""
    name = instance(rng, rng.choice(list(tags)))
    r = rng.random()
    name = name.lower() if r < 0.25 else name.upper() if r < 0.55 else name if r < 0.85 else lookalike(name.lower())
    return ("<" if rng.random() < 0.55 else "</") + name + ">"


def clean_pieces(rng: random.Random, tags: Sequence[str], n: int) -> List[str]:
    """Pieces of a clean stream: plain ASCII runs, non-ASCII characters, whole tag forms, and
    proper prefixes of a tag's source text or of an instance (cut on a character) followed by
    at least 8 plain ASCII bytes — so no class position ever holds '<', '>' or a non-ASCII byte."""
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            out.append(C.plain_run(rng, 1, 12))
        elif r < 0.4:
            out.append(rng.choice([" 思", "é", "я ", "😀", "É"]))
        elif r < 0.8:
            out.append(clean_form(rng, tags))
        else:
            t = rng.choice(list(tags))
            src = ("<" if rng.random() < 0.5 else "</") + (t if rng.random() < 0.5 else instance(rng, t)) + ">"
            out.append(src[:rng.randint(1, len(src) - 1)] + C.plain_run(rng, 8, 12))
    return out
