"""Extended thinking tags — the shorthands ``\\d``, ``\\w``, ``\\s`` and counted repetition —
tag sets, tables and generators shared by tests/test_extended_tags.py (CPU) and
tests/test_gpu_extended_tags.py (GPU) (``extended=True``, ``runtime.native_extended_tags``, with
``classes`` and ``variants``).

Non-ASCII characters used outside the Unicode sweep are stable across Unicode versions: U+0663
(ARABIC-INDIC DIGIT THREE) and U+FF13 (FULLWIDTH DIGIT THREE) are digits and word characters,
U+00A0 and U+3000 are spaces, é is a cased letter, 思 an uncased one.
"""
from __future__ import annotations

import random
from typing import List, Sequence

import class_tag_cases as C

KW = dict(classes=True, variants=True, extended=True)
MIXED_KW = dict(classes=True, unicode=True, mixed=True, variants=True, extended=True)
OFF_KW = dict(classes=True, variants=True)

D3, FW3, NBSP, IDSP = "٣", "３", " ", "　"

NEEDS = "tag needs regex semantics: "
UPPER = ("tag holds \\D, \\W or \\S: the reference's streaming filter compiles the lowercased tag (\\d, \\w, \\s) "
         "and its final strip the tag as written, so the two disagree (runs with --impl python): ")
EMPTY_REPEAT = "tag repeats a group that can match the empty string (runs with --impl python): "
EMPTY_ROW = "tag has an empty alternative: "
CLASS_FIRST = "tag has an alternative that begins with a class: "
TOO_MANY = "thinking tags expand to more than 16 rows: "
SAME_PATTERN = "two thinking tags give the same pattern under different source texts: "
TOO_LONG = "unsupported tag length: "

# (tag, its rows in priority order) — accepted with the key on
ROW_TABLE = [
    ("step\\d", ["step\\d"]),
    ("a\\d{1,2}", ["a\\d\\d", "a\\d"]),
    ("(a|b){1,2}", ["aa", "ab", "a", "ba", "bb", "b"]),
    ("a{0}b", ["b"]),
    ("h[1-6]{2}", ["h[1-6][1-6]"]),
    ("h[1-6]{1,2}", ["h[1-6][1-6]", "h[1-6]"]),
    ("t\\d?", ["t\\d", "t"]),
    ("a{1}", ["a"]),
    ("ab{,2}", ["abb", "ab", "a"]),
    ("thought_\\d{1,2}", ["thought_\\d\\d", "thought_\\d"]),
    ("phase\\s\\d", ["phase\\s\\d"]),
    ("a[\\d_]", ["a[\\d_]"]),
    ("a[a-f\\d]", ["a[a-f\\d]"]),
    ("a[^\\w]", ["a[^\\w]"]),
    ("a[\\d-]", ["a[\\d-]"]),
    ("a\\w\\s", ["a\\w\\s"]),
    ("x(?:ab|c){2}", ["xabab", "xabc", "xcab", "xcc"]),
    ("(?:a|ab){1,2}", ["aa", "aab", "a", "aba", "abab", "ab"]),
    ("a{3}", ["aaa"]),
    ("a{2,3}b", ["aaab", "aab"]),
]

# (tag, message with the key on); with the key off every one of them is NEEDS + tag
REFUSED = [
    ("a[\\d-z]", NEEDS), ("a[a-\\d]", NEEDS),
    ("\\dx", CLASS_FIRST), ("\\w{2}", CLASS_FIRST), ("[\\d_]a", CLASS_FIRST), ("a|\\sb", CLASS_FIRST),
    ("a\\D", UPPER), ("a\\W", UPPER), ("a\\S", UPPER), ("a[\\D]", UPPER), ("a[^\\W]", UPPER), ("a[x\\S]", UPPER),
    ("a\\b", NEEDS), ("a\\B", NEEDS), ("\\Aa", NEEDS), ("a\\Z", NEEDS), ("a\\t", NEEDS), ("a\\n", NEEDS),
    ("a\\x41", NEEDS), ("a\\u0041", NEEDS), ("(a)\\1", NEEDS),
    ("a{2,}", NEEDS), ("a{3,2}", NEEDS), ("a{2}?", NEEDS), ("a{2}+", NEEDS), ("a{2}{2}", NEEDS), ("a{2}*", NEEDS),
    ("a{", NEEDS), ("a{x}", NEEDS), ("a{ 1}", NEEDS), ("a{}", NEEDS), ("a{,}", NEEDS), ("a{1,2", NEEDS), ("a{62}", NEEDS),
    ("a{1,62}", NEEDS), ("{2}a", NEEDS), ("a\\d*", NEEDS), ("a\\d+", NEEDS), ("a\\d{1,2}?", NEEDS),
    ("(a?){2}", EMPTY_REPEAT), ("(a|){1,2}", EMPTY_REPEAT), ("(?:a?b?){0}", EMPTY_REPEAT),
    ("a{,2}", EMPTY_ROW), ("a{0}", EMPTY_ROW), ("\\d{0}", EMPTY_ROW),
    ("a{1,61}", TOO_MANY), ("a(b|c){5}", TOO_MANY), ("a\\d{1,17}", TOO_MANY), ("ab{,16}", TOO_MANY),
    ("a" * 59 + "\\d{2}", NEEDS),           # a source text of 64 bytes
    ("a" * 46 + "\\d{4}", TOO_LONG),        # "</" + 46 + 4 * 4 + ">" = 65 bytes: a shorthand class counts 4
]

# the GPU tests' clean streams and the fuzz sets of the issue
CLEAN_SET = ["step\\d", "t\\d?", "h[1-6]{1,2}", "sec\\d{1,3}"]
FUZZ_SET = ["step\\d", "t\\d?", "h[1-6]{1,2}", "sec\\s\\d{1,3}", "n[\\w-]{2}"]
MIXED_SET = ["思\\d", "réfl\\w{1,2}"]
EDGE_TAG = "abcdefghijklmn\\d{1,2}"

FUZZ_ALPHABET = list("0123456789") + list("abehnpstcABEHNPSTC") + ["_", " ", "\n", "-", D3, FW3, NBSP, IDSP, "é", "É", "思",
                                                                     "<", "<", ">", ">", "/", "</"]
FUZZ_WORDS = ["<step", "</step", "<t", "</t", "<h", "</h", "<sec", "</sec", "<n", "</n", "<sec ", "<step1>", "</step1>",
              "<t>", "</t>", "<h12>", "<sec 12>", "</sec 12>", "<n_-", "<step" + D3 + ">", "</step" + D3 + ">",
              "<t" + FW3 + ">", "<sec" + NBSP + "7>", "<sec" + IDSP + D3 + "1>", "<né思>", "</né思>", "<step\\d>", "<t\\d?>",
              "<h[1-6]{1,2}>", "<step\\", "<sec\\s\\d{1,"]
MIXED_WORDS = ["<思", "</思", "<réfl", "</réfl", "<RÉFL", "<思7>", "</思7>", "<思" + D3 + ">", "</思" + D3 + ">", "<réflx>",
               "</RÉFLX>", "<réfl思1>", "</réfl思1>", "<réfl_>", "<思\\d>", "<réfl\\w{1,2}>", "<réfl" + FW3, "<思" + FW3 + ">"]


def fuzz_text(rng: random.Random, n: int, words: Sequence[str] = FUZZ_WORDS) -> str:
    """n pieces of the fuzz alphabet: tag heads, whole tags, source texts and single characters.
    Never a cased non-ASCII letter in a block that closes in another case (é and É stand apart)."""
    return "".join(rng.choice(words) if rng.random() < 0.45 else rng.choice(FUZZ_ALPHABET) for _ in range(n))


# ---------------------------------------------------------------- clean streams (GPU)
def _clean_names(rng: random.Random) -> List[str]:
    d = lambda: rng.choice("0123456789")  # noqa: E731
    h = lambda: rng.choice("123456")  # noqa: E731
    return ["step" + d(), "t" + d(), "t", "h" + h(), "h" + h() + h(), "sec" + d(), "sec" + d() + d(), "sec" + d() + d() + d()]


def clean_form(rng: random.Random) -> str:
    """A whole open or close of a row of CLEAN_SET in lower, upper or mixed case, or a near miss
    (a letter where a digit belongs, one digit too many, a digit outside [1-6])."""
    name = rng.choice(_clean_names(rng))
    r = rng.random()
    if r < 0.3:
        name = name.upper()
    elif r < 0.5:
        name = "".join(c.upper() if rng.random() < 0.5 else c for c in name)
    elif r < 0.62:
        name = rng.choice(["stepx", "step12", "step", "h7", "h123", "h", "sec", "sec1234", "secx", "tx", "t12", "ste1"])
    return ("<" if rng.random() < 0.55 else "</") + name + ">"


def clean_pieces(rng: random.Random, n: int, extra: Sequence[str] = ()) -> List[str]:
    """Pieces of a clean stream of CLEAN_SET: plain runs, whole forms of every row, plain "<t>" and
    "</t>", and proper prefixes of a source text or of an instance followed by plain bytes."""
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.25:
            out.append(C.plain_run(rng, 1, 12))
        elif r < 0.7:
            out.append(clean_form(rng))
        elif r < 0.8:
            out.append(rng.choice(["<t>", "</t>", "<T>", "</T>"]))
        elif extra and r < 0.88:
            out.append(rng.choice(list(extra)))
        else:
            name = rng.choice(CLEAN_SET) if rng.random() < 0.5 else rng.choice(_clean_names(rng))
            src = ("<" if rng.random() < 0.5 else "</") + name + ">"
            out.append(src[:rng.randint(1, len(src) - 1)] + C.plain_run(rng, 8, 12))
    return out
