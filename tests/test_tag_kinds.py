"""The three kinds of native tag set — literal, class ('.', "[...]", escapes), pair (a cased
non-ASCII character) — as one value per filter, stripper and engine.

Every instance owns its tables: any number of distinct tag sets can be built in one process,
and two instances with different tables never see each other's.  Compared with the python
oracle (``quorum_amd/ops/reference.py``).
"""
import random
import threading

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.native import NativeEngine

import engine_harness as H

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _ext():
    return native.require()


def _filtered(f, text):
    return f.feed(text.encode()).decode()


# ---------------------------------------------------------------- no cap on distinct tag sets
@pytest.mark.parametrize("kind", ["class", "pair"])
def test_300_distinct_tag_sets_in_one_process(kind):
    """300 distinct class tag sets and 300 distinct pair tag sets: each builds, each one's
    StreamFilter and Stripper agree with the oracle on a short text that holds its tag."""
    ext = _ext()
    keep = []  # (every set stays alive to the end: none can stand in for another)
    for i in range(300):
        if kind == "class":
            tags, kw, text = [f"a{i}."], dict(classes=True), f"x<a{i}Q>h</A{i}q>y<a{i}>z"
        else:
            tags, kw, text = [f"é{i}"], dict(unicode=True), f"x<É{i}>h</é{i}>y<e{i}>z"
        f, s = ext.StreamFilter(tags, **kw), ext.Stripper(tags, **kw)
        keep.append((f, s))
        assert _filtered(f, text) == ref.ThinkingTagFilter(tags).feed(text) == f"xy<{'a' if kind == 'class' else 'e'}{i}>z", (i, tags)
        assert s.strip(text.encode()).decode() == ref.strip_thinking_tags(text, tags), (i, tags)
    # the first sets still run their own tables after the last was built
    for i in (0, 1, 254, 255):
        f = keep[i][0]
        text = f"<a{i}Z>q</a{i}z>w" if kind == "class" else f"<é{i}>q</É{i}>w"
        assert _filtered(f, text) == "w", i


# ---------------------------------------------------------------- kinds
KINDS = [
    (["think"], dict(), "literal"),
    (["think", "思考"], dict(unicode=True), "literal"),
    (["réflexion"], dict(unicode=True), "pair"),
    (["th.nk"], dict(classes=True), "class"),
    (["note\\.x"], dict(classes=True), "class"),  # an escape only: no class table
    (["think", "th.nk"], dict(classes=True), "class"),
]


@pytest.mark.parametrize("tags,kw,kind", KINDS)
def test_tagset_has_classes_table(tags, kw, kind):
    kw = dict(dict(classes=False), **kw)
    assert _ext().tagset_has_classes(tags, **kw) == (kind != "literal")


@pytest.mark.parametrize("tags,kw,kind", KINDS)
def test_tagset_kind_table(tags, kw, kind):
    ext = _ext()
    assert ext.tagset_kind(tags, **kw) == kind
    assert ext.tagset_has_classes(tags, **dict(dict(classes=False), **kw)) == (kind != "literal")


def test_tagset_kind_defaults_refuse_like_the_parser():
    ext = _ext()
    assert ext.tagset_kind(["think"]) == "literal"
    for tags in (["th.nk"], ["réflexion"]):
        with pytest.raises(ValueError, match="regex semantics"):
            ext.tagset_kind(tags)


# ---------------------------------------------------------------- the Kelvin sign
KELVIN = "THIN\u212a"


def test_kelvin_sign_lowercases_to_ascii():
    """"THIN\\u212a".lower() is "think": the tag reaches the extension as ASCII, on the plain
    path, and runs as ["think"] does."""
    text = "a<think>b</think>c"
    assert native.strip_fn([KELVIN])(text, True) == native.strip_fn(["think"])(text, True) == "ac"
    rng = random.Random(0)
    streams = [[H.event_bytes(rng, text), b"data: [DONE]\n\n"]]
    res = [H.run_engine(NativeEngine("cpu", tags), streams, [True], [True], H.EveryRound())
           for tags in ([KELVIN], ["think"])]
    assert res[0] == res[1]
    assert res[0][0][0][2] == "ac"


# ---------------------------------------------------------------- independent tables
def test_two_class_tag_sets_fed_alternately_from_two_threads():
    """["th.nk"] and ["th[0-9]nk"], one StreamFilter each, a thread each, fed in turn with the
    same text split at every byte: each equals the oracle of its own tag set fed the same
    pieces, which is its own one-piece result wherever the cut is not inside "<thX" | "nk>"
    (outside a block the reference holds back the tag's source text only, so "<thX" is
    released there before the rest arrives)."""
    ext = _ext()
    text = "<thXnk>a</thXnk>b<th1nk>c</th1nk>d"
    raw = text.encode()
    sets = [["th.nk"], ["th[0-9]nk"]]
    whole = [_filtered(ext.StreamFilter(t, classes=True), text) for t in sets]
    assert whole == [ref.ThinkingTagFilter(t).feed(text) for t in sets] == ["bd", "<thXnk>a</thXnk>bd"]
    # splits: byte by byte, then every cut into two pieces
    plans = [[raw[i:i + 1] for i in range(len(raw))]] + [[raw[:k], raw[k:]] for k in range(1, len(raw))]
    turn = threading.Barrier(2)
    got = [[], []]

    def run(w):
        for plan in plans:
            f = ext.StreamFilter(sets[w], classes=True)
            out = b""
            for piece in plan:
                turn.wait(timeout=30)
                out += f.feed(piece)
            got[w].append(out.decode())

    threads = [threading.Thread(target=run, args=(w,)) for w in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    for w in (0, 1):
        want = []
        for plan in plans:
            py = ref.ThinkingTagFilter(sets[w])
            want.append("".join(py.feed(piece.decode()) for piece in plan))
        assert got[w] == want, (sets[w], got[w])
        # (plan 0 is byte by byte; plan k cuts after byte k: inside "<thX|n|k|>", "<th1|n|k|>")
        cut_open = [k for k, x in enumerate(want) if x != whole[w]]
        assert cut_open == ([0, 4, 5, 6, 21, 22, 23] if w == 0 else [0, 21, 22, 23]), (sets[w], want)
