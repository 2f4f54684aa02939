"""Class thinking tags on the native C++ engine ('.', bracket classes, escaped punctuation).

The reference joins ``thinking_tags`` unescaped into a regex alternation, so ``th.nk`` or
``t[0-9]`` is a pattern.  With ``classes=True`` (``runtime.native_regex_tags``) the native
engines run that fixed-width part of the regex language exactly; these tests pin the parser,
the element tables and the filter / strip semantics against Python's ``re`` and the python
oracle (``quorum_amd/ops/reference.py``).
"""
import random
import re

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import native_tag_ok
from quorum_amd.ops.native import NativeEngine

import class_tag_cases as C
import engine_harness as H

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _ext():
    return native.require()


# ---------------------------------------------------------------- parser
ACCEPTED = ["a.b", "t[0-9]", "x[^y]z", "r\\.s", "a[.]b", "q[^a-z]", "n[a-c-]te", "a[-x]", "a[^-x]", "a[\\]\\\\\\^\\-\\[]",
            "a\\*\\+\\?\\{\\}\\[\\]\\|\\(\\)\\^\\$\\-\\\\", "a[Z-a]", "A[A-C]", "a[ !#%&',:;=@_`~]", "a[a^]", "a[|]",
            "abcdefghijklm.op[0-9]rs", "a" + "." * 15, "a" * 31 + "[b-d]" * 6, "a-b", "think"]
REFUSED = ["a|b", "x*", "q?", "th(ink)", ".b", "[x]y", "a\\d", "[]a]", "é", "a[]a]", "a[^]a]", "a[a--]", "a[a&&b]",
           "a[a~~b]", "a[a||b]", "a[[:alpha:]]", "a[\\w]", "a[\\d]", "a+", "a{2}", "^a", "a$", "a[b", "a]", "a\\", "a[c-a]",
           "a[a-c-e]", "a[<]", "a[>]", "a[/]", "a<", "a\\<", "a[é]", "a\\n", "a[\\n]", "\\", "a[]",
           "a" + "." * 16,  # byte bound 3 + 1 + 16 * 4 = 68 > 64
           "a[^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b][^b]"]


def test_parser_accepts():
    ext = _ext()
    for tag in ACCEPTED:
        ext.StreamFilter(["think", tag], classes=True)
        ext.Stripper([tag], classes=True)
        assert ext.tagset_ok([tag], True), tag
        assert native_tag_ok(["think", tag], classes=True), tag
        re.compile(tag)  # (and it is a pattern Python compiles)


def test_parser_refuses():
    ext = _ext()
    for tag in REFUSED:
        with pytest.raises(ValueError, match="regex semantics|unsupported tag length"):
            ext.StreamFilter(["think", tag], classes=True)
        assert not ext.tagset_ok(["think", tag], True), tag
        assert not native_tag_ok(["think", tag], classes=True), tag
    with pytest.raises(ValueError, match="too many thinking tags"):
        ext.StreamFilter([f"t{i}." for i in range(17)], classes=True)
    assert ext.tagset_ok([f"t{i}." for i in range(16)], True)
    # more distinct class definitions than the tables hold
    many = ["a" + "".join(f"[{chr(97 + i)}{chr(97 + j)}]" for j in range(i + 1, i + 9)) for i in range(5)]
    assert ext.tagset_ok(many[:4], True)
    with pytest.raises(ValueError, match="too many tag classes"):
        ext.StreamFilter(many, classes=True)


def test_defaults_refuse_every_class_tag():
    """classes=False (the default): everything with a metacharacter is refused as before,
    with the same message — by the parser, the engines and native_tag_ok."""
    ext = _ext()
    for tag in ACCEPTED + REFUSED:
        literal = native_tag_ok([tag])
        assert literal == (tag in ("a-b", "think")), tag
        if literal:
            continue
        assert not native_tag_ok(["think", tag], classes=False)
        assert not ext.tagset_ok(["think", tag])
        for make in (lambda t: ext.StreamFilter(["think", t]), lambda t: ext.Stripper(["think", t]),
                     lambda t: ext.CpuEngine(["think", t]), lambda t: NativeEngine("cpu", ["think", t]),
                     lambda t: native.strip_fn(["think", t])):
            with pytest.raises(ValueError, match="regex semantics|unsupported tag length"):
                make(tag)


def test_make_engine_flag_and_cache():
    from quorum_amd.ops.engine import PyEngine, make_engine

    tags = ["think", "th.nk"]
    assert isinstance(make_engine("cpu", tags), PyEngine)
    eng = make_engine("cpu", tags, classes=True)
    assert isinstance(eng, NativeEngine) and eng.classes
    assert make_engine("cpu", tags, classes=True) is eng
    lit = make_engine("cpu", ["think"])
    assert make_engine("cpu", ["think"], classes=True) is not lit  # the flag is part of the key
    assert isinstance(make_engine("cpu", ["think", "x*"], classes=True), PyEngine)


# ---------------------------------------------------------------- element tables
ELEMENTS = [".", "[A-C]", "[^k]", "[Z-a]", "[0-9]", "[^y]", "[a-z]", "[^a-z]", "[.]", "[a-c-]", "[-x]", "[^-x]", "[a^]",
            "[\\]\\\\\\^\\-\\[]", "[ !#%&',:;=@_`~]", "[|*+?(){}$.]", "\\.", "\\*", "\\\\", "\\-", "\\[", "\\]", "\\|",
            "k", "K", "-", "_", " "]


@pytest.mark.parametrize("elem", ELEMENTS)
def test_element_tables_exhaustive(elem):
    """Every element form, every ASCII byte: the streaming filter's match equals
    re.fullmatch(elem, chr(b), re.I), the final strip's the same with re.S."""
    ext = _ext()
    tag = "q" + elem
    filt_rx, strip_rx = re.compile(f"<q{elem}>", re.I), re.compile(f"<q{elem}>", re.I | re.S)
    strip = native.strip_fn([tag], classes=True)
    for b in range(128):
        ch = chr(b)
        f = ext.StreamFilter([tag], classes=True)
        out = f.feed(f"<q{ch}>x".encode()).decode()
        want = bool(filt_rx.fullmatch(f"<q{ch}>"))
        assert (out == "") == want, (elem, b, out)
        if not want and ch not in "<":  # (a '<' is held back as a possible tag start)
            assert out == f"<q{ch}>x", (elem, b, out)
        text = f"<q{ch}>y</q{ch}>z"
        got = strip(text, True)
        assert got == ref.strip_thinking_tags(text, [tag]), (elem, b, got)
        assert (got == "z") == bool(strip_rx.fullmatch(f"<q{ch}>")) or ch in "<>/", (elem, b, got)
    for ch in C.WIDE:  # the one flag: does the element accept non-ASCII code points?
        f = ext.StreamFilter([tag], classes=True)
        assert (f.feed(f"<q{ch}>x".encode()).decode() == "") == bool(filt_rx.fullmatch(f"<q{ch}>")), (elem, ch)


# ---------------------------------------------------------------- differential fuzz
def _feed_both(tags, text, chunks):
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, classes=True)
    for ch in chunks:
        got, want = nat.feed(ch.encode()).decode(), py.feed(ch)
        assert got == want, (tags, text, ch, got, want)
        assert nat is not None
    return py


@pytest.mark.parametrize("ti", range(len(C.TAG_SETS)))
def test_filter_and_strip_fuzz(ti):
    """>= 2,000 seeded cases per tag set: the native StreamFilter equals the oracle after
    every feed (random splits of 1-40 characters), the native strip equals the oracle's."""
    tags = C.TAG_SETS[ti]
    strip = native.strip_fn(tags, classes=True)
    for seed in range(2200):
        rng = random.Random(seed * 131 + ti)
        text = "".join(C.fuzz_pieces(rng, tags, rng.randint(1, 14)))
        _feed_both(tags, text, C.split_chars(rng, text, 1, rng.choice([3, 8, 40])))
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)


@pytest.mark.parametrize("ti", range(len(C.CLEAN_SETS)))
def test_clean_generator_has_no_suspect_candidate(ti):
    """The clean generator of the GPU tests never produces a candidate the kernels would hand
    to the host path (the shared suspect function) — and its streams are filtered exactly."""
    ext = _ext()
    tags = C.CLEAN_SETS[ti]
    for seed in range(700):
        rng = random.Random(seed * 17 + ti)
        text = "".join(C.clean_pieces(rng, tags, rng.randint(1, 30)))
        assert ext.class_suspects(tags, text.encode()) == 0, (tags, text)
        assert ext.class_suspects(tags, text.encode(), strip=True) == 0, (tags, text)
        _feed_both(tags, text, C.split_chars(rng, text, 1, 40))


def test_suspect_rule():
    ext = _ext()
    for tags, text, n in [(["th.nk"], "<th日nk>x</th日nk>y", 2), (["th.nk"], "<th<nk>z", 1), (["th.nk"], "<th>nk>z", 1),
                          (["a.", "a"], "<a>>x</a>>y", 2), (["th.nk"], "<thXnk>a</thYnk>b<th", 0),
                          (["th.nk"], "<tX<nk>", 0), (["think"], "<th<nk>", 0), (["t[0-9]"], "<t日>", 1)]:
        assert ext.class_suspects(tags, text.encode()) == n, (tags, text)


# ---------------------------------------------------------------- hand cases
def _filter_chunks(tags, chunks):
    f = _ext().StreamFilter(tags, classes=True)
    py = ref.ThinkingTagFilter(tags)
    out = []
    for ch in chunks:
        got = f.feed(ch.encode()).decode()
        assert got == py.feed(ch), (tags, chunks, ch)
        out.append(got)
    return out


def test_hand_filter_vs_strip_newline():
    """A dot takes no newline in the streaming filter (no DOTALL) and takes one in the strip."""
    text, tags = "<aXb>h</a\nb></aYb>y", ["a.b"]
    assert _filter_chunks(tags, [text]) == ["y"]
    assert native.strip_fn(tags, classes=True)(text, True) == ref.strip_thinking_tags(text, tags) == "<aXb>h</a\nb></aYb>y"
    text2 = "<a\nb>h</a\nb>y"
    assert _filter_chunks(tags, [text2]) == [text2]
    assert native.strip_fn(tags, classes=True)(text2, True) == ref.strip_thinking_tags(text2, tags) == "y"


def test_hand_backreference():
    """The strip's close is the open's captured text, not any match of the pattern."""
    text, tags = "<aXb>h</aYb>q</axb>y", ["a.b"]
    assert native.strip_fn(tags, classes=True)(text, True) == ref.strip_thinking_tags(text, tags) == "y"
    assert _filter_chunks(tags, [text]) == ["q</axb>y"]  # the filter's close is any match


def test_hand_dot_swallows_close_bracket():
    tags = ["a.", "a"]
    strip = native.strip_fn(tags, classes=True)
    for text in ["<a>>x</a>>y", "<A>></A>", "<A>>x</A>"]:
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), text
        _filter_chunks(tags, [text])
        _filter_chunks(tags, list(text))
    assert strip("<A>>x</A>", True) == ""  # the second alternative finds its close
    assert strip("<a>>x</a>>y", True) == "y"


@pytest.mark.parametrize("depth", [0, 1])
def test_hand_holdback_is_source_prefix(depth):
    """Outside a block the reference holds what is a prefix of the tag's source text: "<a."
    completes with "b>", "<aX" was released and does not.  Inside a block the whole buffer is
    kept, so both complete."""
    tags = ["a.b"]
    pre = ["<a1b>"] if depth else []
    got = _filter_chunks(tags, pre + ["<a.", "b>", "t"])
    assert got[len(pre):] == ["", "", ""]
    got = _filter_chunks(tags, pre + ["<aX", "b>", "t"])
    assert got[len(pre):] == (["", "", ""] if depth else ["<aX", "b>", "t"])


def test_hand_wide_code_point_split_at_every_byte():
    """<a日b> fed in two parts split after every byte, code point bytes included, outside
    and inside a block: the same final state as the oracle fed whole characters."""
    ext = _ext()
    tags = ["a.b"]
    raw = "<a日b>".encode()
    for pre in ("", "<a1b>"):
        for k in range(1, len(raw)):
            f = ext.StreamFilter(tags, classes=True)
            out = f.feed(pre.encode()) + f.feed(raw[:k]) + f.feed(raw[k:]) + f.feed(b"</a-b>!")
            # bytes 3..5 cut the code point: no str split lands there, and outside a block a
            # held "<a" + partial bytes is no prefix of the source text, so it is released
            whole = k <= 2 or k >= 5
            if pre or whole:
                py = ref.ThinkingTagFilter(tags)
                parts = [pre, raw[:k].decode(), raw[k:].decode()] if whole else [pre, raw.decode()]
                want = "".join(py.feed(p) for p in parts + ["</a-b>!"])
                assert out.decode() == want, (pre, k)
            else:
                assert out == raw + b"</a-b>!", (pre, k)


def test_case_and_escape_cases():
    for tags, text in [(["A[A-C]"], "<ab>x</aB>y<aD>"), (["a[Z-a]"], "<a`>1</A`>2<aZ>3</az>4<aA>5</aa>6<ab>"),
                       (["r\\.s"], "<r.s>x</R.S>y<rXs>"), (["q[^K]"], "<qk>a<qj>b</qJ>c"),
                       (["t[0-9]", "think"], "<T5>a<think>b</think>c</t5>d</t7>e")]:
        assert native.strip_fn(tags, classes=True)(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)
    # the streaming oracle lowercases its tags, which "[Z-a]" does not survive: the others
    for tags, text in [(["A[A-C]"], "<ab>x</aB>y<aD>"), (["r\\.s"], "<r.s>x</R.S>y<rXs>"), (["q[^K]"], "<qk>a<qj>b</qJ>c")]:
        _filter_chunks(tags, list(text))


# ---------------------------------------------------------------- whole engine
@pytest.mark.parametrize("seed", range(40))
def test_cpu_engine_matches_python_class_tags(seed):
    rng = random.Random(seed)
    tags = C.TAG_SETS[seed % len(C.TAG_SETS)]
    raw = []
    for _ in range(4):
        gen = C.fuzz_pieces if rng.random() < 0.5 else C.clean_pieces
        parts = [H.event_bytes(rng, "".join(gen(rng, tags, rng.randint(0, 4)))) for _ in range(rng.randint(1, 12))]
        raw.append(b"".join(parts) + b"data: [DONE]\n\n")
    streams = [H.split_random(rng, r, rng.choice([3, 17, 64, 400])) for r in raw]
    filt, emit = [True] * 4, [True] * 4
    ts = rng.randint(0, 10**9)
    py = H.run_engine(H.python_engine(tags), streams, filt, emit, random.Random(ts))
    nat = H.run_engine(NativeEngine("cpu", tags, classes=True), streams, filt, emit, random.Random(ts))
    assert py == nat, (tags, raw)


# ---------------------------------------------------------------- config + server
def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_regex_tags is False
    assert RuntimeConfig.from_config({"runtime": {"native_regex_tags": True}}).native_regex_tags is True
    with pytest.raises(ValueError, match="native_regex_tags"):
        RuntimeConfig.from_config({"runtime": {"native_regex_tags": "yes"}})


def test_native_config_key_on_and_off():
    from conftest import cfg_parallel
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    import test_native_server as T

    tags = ["think", "th.nk"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, thinking_tags=tags))
    with pytest.raises(NativeUnsupported, match="need regex semantics: run with --impl python"):
        native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)
    on = dict(cfg, runtime={"native_regex_tags": True})
    d = native_config(on, "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tags"] == tags and d["tag_classes"] is True
    assert native_config(cfg_parallel(2, block=T.CONCAT), "127.0.0.1", 1, "cpu", 0, 1)["tag_classes"] is False
    out = dict(cfg_parallel(2, block=dict(T.CONCAT, thinking_tags=["think", "th(ink)"])), runtime={"native_regex_tags": True})
    with pytest.raises(NativeUnsupported, match="need regex semantics: run with --impl python"):
        native_config(out, "127.0.0.1", 1, "cpu", 0, 1)


def class_server_scenario():
    """One streamed session with ["think", "th.nk"]: split tags, a class tag, a tag whose first
    part was released (no tag), a non-ASCII code point at the class position."""
    from conftest import cfg_parallel, sse_chunk

    import test_native_server as T

    s1 = [sse_chunk({"role": "assistant"}), sse_chunk({"content": "A <thXnk>hid"}), sse_chunk({"content": "den</th-nk> B <th"}),
          sse_chunk({"content": ".nk>x</THINK>y</th.nk> C <thQ"}), sse_chunk({"content": "nk>kept</thQnk> <th日nk>w</th日nk> D"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    s2 = [sse_chunk({"content": "<think>t</think>E <thynk>u</thYnk>F</th1nk> <th\nnk>"}), sse_chunk({}, finish="stop"),
          b"data: [DONE]\n\n"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, hide_final_think=True, thinking_tags=["think", "th.nk"]))
    cfg["runtime"] = {"native_regex_tags": True}
    return (cfg, {"b1.test": ("stream", 200, T.split7(s1)), "b2.test": ("stream", 200, s2)},
            {"messages": T.MSG, "stream": True}, T.AUTH)


def test_native_server_class_tags_match_python():
    import test_native_server as T

    T._compare(class_server_scenario(), "class_tags", None)
