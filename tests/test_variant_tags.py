"""Variable-width thinking tags — '?', '|' and groups — on the native C++ engine
(``variants=True``, ``runtime.native_variant_tags``, with ``classes``).

The reference joins ``thinking_tags`` unescaped into one regex, so ``thoughts?``,
``think(ing)?`` and ``think|reason`` are tags there.  Such a tag has the matches of the ordered
alternation of its fixed-width expansions, its *rows*; the native parser yields them in the
regex's priority order and every row runs as one entry of a class tag set whose source text is
the whole tag.  These tests pin the rows, every refusal and the key off, and the filter / strip
/ engine semantics and the kernels' suspect rule against the python oracle
(``quorum_amd/ops/reference.py``, the real ``re``).

``a?b?`` has the expansions ab, a, b *and the empty one* ("<>" is a tag of ``<(a?b?)>`` in
``re``), so it is refused like ``a?`` for its empty row, not accepted as ab, a, b; ``a?b?c``
(abc, ac, bc, c) is the accepted case of two optional elements in a row.
"""
import random
import re

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import native_tag_ok
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import variant_tag_cases as V

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")

NEEDS = "tag needs regex semantics: "


def _ext():
    return native.require()


def _err(tags, **kw):
    return _ext().tagset_error(list(tags), **kw)


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("tag,rows", V.ROW_TABLE)
def test_rows_in_priority_order(tag, rows):
    assert native.tagset_rows([tag], **V.KW) == [(r, 0) for r in rows]
    assert [V.row_text(r) for r in V.expand(tag)] == rows  # the generators' own expansion agrees
    assert native.tagset_kind([tag], **V.KW) == "class"
    assert native_tag_ok([tag], classes=True, variants=True)


def test_rows_follow_the_tag_list():
    got = native.tagset_rows(["think", "T[0-9]?", "Thoughts?", "th.nk"], **V.KW)
    assert got == [("think", 0), ("t[0-9]", 1), ("t", 1), ("thoughts", 2), ("thought", 2), ("th.nk", 3)]
    assert _ext().tagset_size(["think", "t[0-9]?", "thoughts?", "th.nk"], **V.KW) == 6
    # a tag without '?', '|' or a group is what it is with the key off
    for tags in (["think"], ["th.nk", "t[0-9]"], ["r\\.s"]):
        assert native.tagset_rows(tags, **V.KW) == native.tagset_rows(tags, classes=True)
        assert native.tagset_kind(tags, **V.KW) == native.tagset_kind(tags, classes=True)
    # the same tag twice (in any case) is one tag
    assert native.tagset_rows(["thoughts?", "THOUGHTS?"], **V.KW) == [("thoughts", 0), ("thought", 0)]


def test_expansion_equals_the_tag_in_re():
    """The fact the feature rests on, for this file's table: the tag and the ordered alternation
    of its rows have the same matches under ``re`` (streaming spans and the strip)."""
    rng = random.Random(5)
    for tag, rows in V.ROW_TABLE:
        alt = "|".join(rows)
        for _ in range(60):
            text = V.fuzz_text(rng, [tag], V.expand(tag), rng.randint(1, 10))
            for pat in ("<(%s)>", "</(%s)>"):
                a, b = re.compile(pat % tag, re.I), re.compile(pat % alt, re.I)
                assert [m.span() for m in a.finditer(text)] == [m.span() for m in b.finditer(text)], (tag, text)
            assert ref.strip_thinking_tags(text, [tag]) == ref.strip_thinking_tags(text, [alt]), (tag, text)


# ---------------------------------------------------------------- refusals
REFUSED = [
    (["a?"], "tag has an empty alternative: a?"),
    (["a?b?"], "tag has an empty alternative: a?b?"),
    (["a|"], "tag has an empty alternative: a|"),
    (["(a)?"], "tag has an empty alternative: (a)?"),
    ([".?a"], "tag has an alternative that begins with a class: .?a"),
    (["a|[0-9]b"], "tag has an alternative that begins with a class: a|[0-9]b"),
    (["a(b|c)(d|e)(f|g)(h|i)(j|k)"], "thinking tags expand to more than 16 rows: a(b|c)(d|e)(f|g)(h|i)(j|k)"),
    (["a(b|c)(d|e)(f|g)", "x(b|c)(d|e)(f|g)", "y"], "thinking tags expand to more than 16 rows: y"),
    (["ab?c", "ac"], "two thinking tags give the same pattern under different source texts: ab?c, ac"),
    (["ac", "ab?c"], "two thinking tags give the same pattern under different source texts: ac, ab?c"),
    (["th(is|at)", "th(at|em)"], "two thinking tags give the same pattern under different source texts: "
                                 "th(is|at), th(at|em)"),
]
STILL_NEEDS_REGEX = ["a??", "a?+", "a?*", "a?{2}", "a*", "a+", "a{2}", "(?=a)b", "(?P<n>a)", "(?i)a", "(a", "a)", "a(",
                     "^a?", "a?$", "a\\d?", "?a", "a(?", "(" * 100 + "a" + ")" * 100, "(" * 61]


@pytest.mark.parametrize("tags,msg", REFUSED)
def test_refusals_have_their_own_message(tags, msg):
    assert _err(tags, **V.KW) == msg
    assert not native_tag_ok(tags, classes=True, variants=True)
    for make in (lambda: _ext().StreamFilter(tags, **V.KW), lambda: _ext().Stripper(tags, **V.KW),
                 lambda: NativeEngine("cpu", tags, **V.KW), lambda: native.strip_fn(tags, **V.KW)):
        with pytest.raises(ValueError, match=re.escape(msg)):
            make()


def test_sixteen_rows_fit():
    tags = ["a(b|c)(d|e)(f|g)", "x(b|c)(d|e)(f|g)"]
    assert _err(tags, **V.KW) == "" and _ext().tagset_size(tags, **V.KW) == 16
    # groups nest as deep as the 61 bytes of a source text allow
    assert native.tagset_rows(["(" * 30 + "a" + ")" * 30], **V.KW) == [("a", 0)]
    # duplicates within one tag are dropped before they count
    assert native.tagset_rows(["(a|a)(b|b)(c|c)(d|d)(e|e)x"], **V.KW) == [("abcdex", 0)]


@pytest.mark.parametrize("tag", STILL_NEEDS_REGEX)
def test_still_refused_with_the_existing_message(tag):
    assert _err(["think", tag], **V.KW) == NEEDS + tag
    assert not native_tag_ok(["think", tag], classes=True, variants=True)


def test_limits_of_source_and_row():
    ok, long = "a" * 59 + "b?", "a" * 60 + "b?"
    assert _err([ok], **V.KW) == "" and _err([long], **V.KW) == NEEDS + long
    # "</" + longest match + ">" within 64 bytes: a wide class element counts 4
    # (3 + 1 + 4 * 14 + 4 = 64; one more optional letter makes the longest row 65)
    fits, over = "a" + "." * 14 + "bcd?e?", "a" + "." * 14 + "bcd?e?f?"
    assert _err([fits], **V.KW) == "", _err([fits], **V.KW)
    assert _err([over], **V.KW) == "unsupported tag length: " + over


def test_key_off_answers_are_todays():
    """variants off (the default), and variants on without classes: today's message through
    every constructor."""
    ext = _ext()
    tags_off = [t for t, _ in V.ROW_TABLE] + [next(x for x in t if set(x) & set("?|(")) for t, _ in REFUSED] + [V.EDGE_TAG]
    makers = (lambda t, **kw: ext.StreamFilter(t, **kw), lambda t, **kw: ext.Stripper(t, **kw),
              lambda t, **kw: ext.CpuEngine(t, **kw), lambda t, **kw: NativeEngine("cpu", t, **kw),
              lambda t, **kw: native.strip_fn(t, **kw))
    for tag in tags_off:
        for kw in ({}, {"classes": True}, {"variants": True}, {"classes": True, "unicode": True, "mixed": True},
                   {"unicode": True, "mixed": True, "variants": True}):
            assert _err(["think", tag], **kw) == NEEDS + tag, (tag, kw)
            assert not native_tag_ok(["think", tag], **kw)
        for make in makers:
            with pytest.raises(ValueError, match=re.escape(NEEDS + tag)):
                make(["think", tag], classes=True)


def test_kind():
    assert native.tagset_kind(["think(ing)?"], **V.KW) == "class"
    assert native.tagset_kind(["think(ing)?"], **V.MIXED_KW) == "class"
    assert native.tagset_kind(["réflexions?"], **V.MIXED_KW) == "mixed"
    assert native.tagset_kind(["思(考)?"], **V.MIXED_KW) == "mixed"
    assert native.tagset_kind(["think", "思考"], **V.MIXED_KW) == "literal"
    assert native.tagset_kind(["think", "réflexion"], **V.MIXED_KW) == "pair"
    assert native.tagset_rows(V.MIXED_SET, **V.MIXED_KW) == [("réflexions", 0), ("réflexion", 0), ("思考", 1),
                                                             ("思", 1)]
    # a non-ASCII variable-width tag needs the mixed key: the existing mixing message
    mixing = "class tags and non-ASCII tags do not mix in one tag set (runs with --impl python)"
    assert _err(["réflexions?"], classes=True, unicode=True, variants=True) == mixing
    assert _err(["think(ing)?", "思考"], classes=True, unicode=True, variants=True) == mixing
    assert _err(["réflexions?"], **V.KW) == NEEDS + "réflexions?"


def test_make_engine_flag_and_cache():
    from quorum_amd.ops.engine import PyEngine, make_engine

    tags = ["Think(ing)?", "thoughts?"]
    assert isinstance(make_engine("cpu", tags, classes=True), PyEngine)
    assert isinstance(make_engine("cpu", tags, variants=True), PyEngine)
    eng = make_engine("cpu", tags, classes=True, variants=True)
    assert isinstance(eng, NativeEngine) and eng.variants
    assert make_engine("cpu", tags, classes=True, variants=True) is eng
    a = make_engine("cpu", ["think"], classes=True, variants=True)
    assert a is not make_engine("cpu", ["think"], classes=True)
    assert isinstance(make_engine("cpu", ["a*"], classes=True, variants=True), PyEngine)


# ---------------------------------------------------------------- differential fuzz against re
def _feed_both(tags, chunks, kw):
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **kw)
    for ch in chunks:
        got, want = nat.feed(ch.encode()).decode(), py.feed(ch)
        assert got == want, (tags, chunks, ch, got, want)
    assert nat.flush().decode() == py.flush(), (tags, chunks)


FUZZ_PARTS, FUZZ_SETS, FUZZ_TEXTS = 8, 250, 20  # 2,000 sets x 20 texts


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_filter_and_strip_fuzz_against_re(part):
    """Seeded random tag sets inside the subset by construction (every one asserted accepted,
    none skipped), texts of instances in both cases, near misses and '<' '>' '/' newlines and
    non-ASCII at class positions, cut at random: every ``feed`` output and ``flush`` of the C++
    StreamFilter equal ThinkingTagFilter's, strip_fn equals strip_thinking_tags."""
    for k in range(FUZZ_SETS):
        rng = random.Random(1_000_003 * part + k)
        tags = V.random_set(rng)
        assert native.tagset_ok(tags, **V.KW), (tags, _err(tags, **V.KW))
        rows = V.all_rows(tags)
        assert [r for r, _ in native.tagset_rows(tags, **V.KW)] == \
            [V.row_text(r) for t in dict.fromkeys(x.lower() for x in tags) for r in V.expand(t)], tags
        strip = native.strip_fn(tags, **V.KW)
        for _ in range(FUZZ_TEXTS):
            text = V.fuzz_text(rng, tags, rows, rng.randint(1, 12))
            _feed_both(tags, _split(rng, text), V.KW)
            assert strip(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)


def _split(rng, text):
    return V.C.split_chars(rng, text, 1, rng.choice([1, 3, 8, 40]))


def test_mixed_family_fuzz_against_re():
    """réflexions? and 思(考)? under the four keys: a mixed tag set, the text folded as it is read."""
    tags = V.MIXED_SET
    assert native.tagset_ok(tags, **V.MIXED_KW)
    strip = native.strip_fn(tags, **V.MIXED_KW)
    names = ["réflexions", "réflexion", "RÉFLEXIONS", "RÉFLEXION", "Réflexion", "思考", "思", "réflexionz", "思考考",
             "reflexion"]
    pieces = [f"{lead}{n}>" for n in names for lead in ("<", "</")] + \
        ["<", ">", "/", "\n", "s>", "考>", "x", " é ", "<réflexions?>", "<思(考)?>", "<réflexion", "</réfl", "<思(",
         "<RÉ"]
    for seed in range(1500):
        rng = random.Random(seed)
        text = "".join(rng.choice(pieces) for _ in range(rng.randint(1, 12)))
        _feed_both(tags, _split(rng, text), V.MIXED_KW)
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), text


@pytest.mark.parametrize("seed", range(40))
def test_cpu_engine_matches_python(seed):
    """PyStream (the python engine) against the C++ engine over random batches of SSE streams."""
    rng = random.Random(seed)
    tags = V.random_set(rng) if seed % 4 else V.CLEAN_SETS[seed // 4 % 3]
    rows = V.all_rows(tags)
    raw = []
    for _ in range(4):
        parts = [H.event_bytes(rng, V.fuzz_text(rng, tags, rows, rng.randint(0, 6))) for _ in range(rng.randint(1, 10))]
        raw.append(b"".join(parts) + b"data: [DONE]\n\n")
    streams = [H.split_random(rng, r, rng.choice([3, 17, 64, 400])) for r in raw]
    filt = [rng.random() < 0.7 for _ in range(4)]
    ts = rng.randint(0, 10**9)
    py = H.run_engine(H.python_engine(tags), streams, filt, [True] * 4, random.Random(ts))
    nat = H.run_engine(NativeEngine("cpu", tags, **V.KW), streams, filt, [True] * 4, random.Random(ts))
    assert py == nat, (tags, raw)


# ---------------------------------------------------------------- holdback: split at every byte
SPLIT_TEXTS = ["<think(ing)?>", "<thinking>", "<think>", "</thinking>"]


@pytest.mark.parametrize("text", SPLIT_TEXTS)
@pytest.mark.parametrize("pre", ["", "<T>"])
def test_split_at_every_byte(text, pre):
    """The source text itself, both opens and a close, fed in two parts split after every byte,
    outside and inside a block: the oracle's output per feed."""
    tags = ["think(ing)?", "t"]
    for k in range(1, len(text)):
        py, f = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **V.KW)
        for ch in (pre, text[:k], text[k:], "x</t>!<"):
            assert f.feed(ch.encode()).decode() == py.feed(ch), (text, pre, k, ch)


def test_source_text_is_held_and_an_expansion_is_not():
    tags = ["think(ing)?"]

    def feeds(chunks):
        py, f = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **V.KW)
        out = [py.feed(c) for c in chunks]
        assert [f.feed(c.encode()).decode() for c in chunks] == out, chunks
        return out

    src = "<think(ing)?>"
    for k in range(1, len(src)):  # the source is held at every split outside a block
        assert feeds(["a" + src[:k]]) == ["a"], k
    # "<thinki" is no prefix of the source text: released, so "<thinki" + "ng>" is text there ...
    assert feeds(["a<thinki", "ng>b"]) == ["a<thinki", "ng>b"]
    assert feeds(["a<think(ing", ")?>b"]) == ["a", "<think(ing)?>b"]
    # ... but a tag inside a block (a class-aware prefix of a row is kept)
    assert feeds(["<think>", "x<thinki", "ng>y</thinking>z</think>w"]) == ["", "", "w"]
    assert feeds(["a<thin", "k>b</think>c"]) == ["a", "c"]


# ---------------------------------------------------------------- strip
def _strip(tags, text, kw=V.KW):
    want = ref.strip_thinking_tags(text, tags)
    assert native.strip_fn(tags, **kw)(text, True) == want, (tags, text)
    return want


def test_strip_close_is_the_captured_text():
    assert _strip(["thoughts?"], "<thoughts>a</thought>b</thoughts>c") == "c"
    assert _strip(["thoughts?"], "<thought>a</thoughts>b") == "<thought>a</thoughts>b"
    assert _strip(["thoughts?"], "<THOUGHTS>a</thoughts>") == ""
    assert _strip(["t[0-9]?"], "<t>a</t7>b</t>c<t7>d</t>e</T7>f") == "cf"
    assert _strip(["think|reason(?:ing)?"], "<reason>a</reasoning>b</think>c</reason>d") == "d"
    assert _strip(["réflexions?"], "<RÉFLEXION>a</réflexions>b</réflexion>c", V.MIXED_KW) == "c"


# ---------------------------------------------------------------- the kernels' suspect rule
def test_suspect_rule_for_variant_sets():
    cs = native.class_suspects
    for text in (b"<t>", b"<t7>", b"<t>>", "<t日>".encode(), b"</t>x<t>y</T>", b"<t<t>"):
        assert cs(["t[0-9]?"], text, variants=True) == 0 == cs(["t[0-9]?"], text, strip=True, variants=True), text
    # a byte the class accepts stays suspect
    assert cs(["a.?"], b"<a>x", variants=True) == 1
    assert cs(["a.?"], "<a日>x".encode(), variants=True) == 1
    assert cs(["t[^0-9]?"], b"<t>", variants=True) == 1
    assert cs(["t[^0-9]?"], b"<t7>", variants=True) == 0
    # mixed: the same rule in mixed_candidate
    assert cs(["é[0-9]?"], "<é>x<É>".encode(), unicode=True, mixed=True, variants=True) == 0
    assert cs(["é.?"], "<é>x".encode(), unicode=True, mixed=True, variants=True) == 1


def test_suspect_rule_is_gated():
    """Without a variable-width tag in the set the rule is today's, key on or off."""
    cs = native.class_suspects
    assert cs(["t[0-9]", "t"], b"<t>") == 1
    assert cs(["t[0-9]", "t"], b"<t>", variants=True) == 1
    assert cs(["é[0-9]", "é"], "<é>".encode(), unicode=True, mixed=True) == 1
    assert cs(["é[0-9]", "é"], "<é>".encode(), unicode=True, mixed=True, variants=True) == 1
    with pytest.raises(ValueError, match="tag needs regex semantics"):
        cs(["t[0-9]?"], b"<t>")


# ---------------------------------------------------------------- config + server
def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_variant_tags is False
    on = {"native_regex_tags": True, "native_variant_tags": True}
    assert RuntimeConfig.from_config({"runtime": on}).native_variant_tags is True
    with pytest.raises(ValueError, match="native_variant_tags must be true or false"):
        RuntimeConfig.from_config({"runtime": dict(on, native_variant_tags="yes")})
    for rt in ({"native_variant_tags": True}, {"native_variant_tags": True, "native_unicode_tags": True}):
        with pytest.raises(ValueError, match="native_variant_tags needs runtime.native_regex_tags"):
            RuntimeConfig.from_config({"runtime": rt})


def variant_server_scenario(tags=("think(ing)?", "thoughts?"), keys=None):
    """One streamed session (the shape of tests/test_unicode_tags.py's): both rows of both tags in
    lower and upper case, tags split over events (one after "<thinki", which the reference
    releases), a close of the other row, a near miss, the source text, an unclosed open."""
    from conftest import cfg_parallel, sse_chunk

    import test_native_server as T

    s1 = [sse_chunk({"role": "assistant"}), sse_chunk({"content": "A <THINKING>hid"}),
          sse_chunk({"content": "den</thinking> B <thou"}), sse_chunk({"content": "ghts>x</thought>y</THOUGHTS> C <thinki"}),
          sse_chunk({"content": "ng>kept</thinking> <thinkin>k</thinkin> D <think(ing)?>"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    s2 = [sse_chunk({"content": "<think>t<thinking>u</think>v</thinking>E <Thought>w</thoughts>F</THOUGHT> G<thoughts"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, hide_final_think=True, thinking_tags=list(tags)))
    cfg["runtime"] = dict(keys if keys is not None else {"native_regex_tags": True, "native_variant_tags": True})
    return (cfg, {"b1.test": ("stream", 200, T.split7(s1)), "b2.test": ("stream", 200, s2)},
            {"messages": T.MSG, "stream": True}, T.AUTH)


def test_native_config_key_on_and_off():
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    cfg = variant_server_scenario()[0]
    d = native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tag_variants"] is True and d["tag_classes"] is True and d["tag_mixed"] is False
    assert d["tags"] == ["think(ing)?", "thoughts?"]
    off = dict(cfg, runtime={"native_regex_tags": True})
    with pytest.raises(NativeUnsupported) as e:
        native_config(off, "127.0.0.1", 1, "cpu", 0, 1)
    assert str(e.value) == "thinking_tags ['think(ing)?', 'thoughts?'] need regex semantics: run with --impl python"


def test_native_server_variant_tags_match_python():
    import test_native_server as T

    T._compare(variant_server_scenario(), "variant_tags", None)
