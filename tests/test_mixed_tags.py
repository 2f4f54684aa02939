"""Class and non-ASCII thinking tags in one tag set, and in one tag, on the native C++ engine
(``mixed=True``, ``runtime.native_mixed_tags``, with ``classes`` and ``unicode``).

The reference joins ``thinking_tags`` into one Python regex under IGNORECASE, so
``["th.nk", "思考"]`` or ``réfl.xion`` are tags there.  With the three keywords on the native
engines take them as a *mixed* tag set: the class tag sets' rules, the text folded as it is
read.  These tests pin the parser (what is accepted, every limit, what stays refused, the key
off), and the filter / strip / engine semantics against the python oracle
(``quorum_amd/ops/reference.py``).
"""
import json
import random

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import native_tag_ok
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import mixed_tag_cases as M
import unicode_tag_cases as U

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")

ON = (True, True, True)  # classes, unicode, mixed — positionally, as the bindings take them


def _ext():
    return native.require()


# ---------------------------------------------------------------- parser
def test_accepted_sets_are_mixed():
    ext = _ext()
    for tags in M.TAG_SETS:
        assert ext.tagset_error(tags, *ON) == "", tags
        assert ext.tagset_kind(tags, *ON) == "mixed", tags
        assert ext.tagset_has_classes(tags, *ON)
        assert native_tag_ok(tags, classes=True, unicode=True, mixed=True)
    for tag in ("réfl.xion", "思[0-9]", "é.", "é\\.x.", "я[^a]"):
        assert ext.tagset_kind([tag], *ON) == "mixed", tag
    assert ext.tagset_size(["RÉFL.XION", "réfl.xion", "思考"], *ON) == 2


def test_other_kinds_keep_their_kind_with_the_key_on():
    ext = _ext()
    for tags, kind in ((["think"], "literal"), (["think", "思考"], "literal"), (["th.nk", "think"], "class"),
                       (["think", "réflexion"], "pair"), (["r\\.s"], "class")):
        assert ext.tagset_kind(tags, *ON) == kind == ext.tagset_kind(tags, True, True), tags
    assert not ext.tagset_has_classes(["think", "思考"], *ON)


def test_limits_keep_their_messages():
    ext = _ext()
    # 16 tags after lowercasing through the pair table
    sixteen = [f"é{i}." for i in range(16)]
    assert ext.tagset_ok(sixteen + [t.upper() for t in sixteen], *ON)
    assert "too many thinking tags" in ext.tagset_error(sixteen + ["é16."], *ON)
    # 61 bytes of tag source
    ok, long = "é" * 28 + "[0-9]", "é" * 28 + "a[0-9]"
    assert len(ok.encode()) == 61 and len(long.encode()) == 62
    assert ext.tagset_ok([ok], *ON)
    # (a tag with a class element past the limit has the class tags' message of today)
    assert ext.tagset_error(["a" * 57 + "[0-9]"], True) == "tag needs regex semantics: " + "a" * 57 + "[0-9]"
    assert ext.tagset_error([long], *ON) == "tag needs regex semantics: " + long
    assert "unsupported tag length" in ext.tagset_error(["é" * 31, "th.nk"], *ON)
    # "</" + match + ">" within 64 bytes: a non-ASCII literal counts its UTF-8 length, a wide
    # class element 4 — 3 + 3 * 14 + 4 * 4 + 3 = 64, one more dot is 68
    fits, over = "思" * 14 + "....abc", "思" * 14 + "....." + "ab"
    assert ext.tagset_ok([fits], *ON), ext.tagset_error([fits], *ON)
    assert "unsupported tag length" in ext.tagset_error([over], *ON)
    # 32 classes, 32 pair characters
    cls = [f"é[{chr(33 + k)}]" for k in range(33) if chr(33 + k) not in "<>/[]\\^-"]
    assert len(cls) >= 17
    many = ["é" + "".join(f"[{chr(97 + k)}{chr(97 + j)}]" for j in range(k + 1, k + 12)) for k in range(3)]
    assert sum(t.count("[") for t in many) == 33
    assert "too many tag classes" in ext.tagset_error(many, *ON)
    ps = "àáâãäæçèéêëìíîïðñòóôõöøùúûüýþÿяю"
    assert ext.tagset_ok([ps[:16] + ".", ps[16:]], *ON)
    assert "too many case-pair characters" in ext.tagset_error([ps[:16] + ".", ps[16:], "ạ"], *ON)


def test_still_refused_with_the_key_on():
    ext = _ext()
    for tag, msg in (("a[é]", "tag needs regex semantics"), ("a[a-é]", "tag needs regex semantics"),
                     ("ω.", "without a simple case pair"), (".é", "tag needs regex semantics"),
                     ("[é]a", "tag needs regex semantics"), ("th(ink)", "tag needs regex semantics"),
                     ("é+", "tag needs regex semantics"), ("é|a", "tag needs regex semantics"),
                     ("é\\d", "tag needs regex semantics"), ("^é.", "tag needs regex semantics")):
        assert msg in ext.tagset_error(["think", tag], *ON), tag
        assert not native_tag_ok(["think", tag], classes=True, unicode=True, mixed=True)


NO_MIX_SETS = (["th.nk", "思考"], ["réflexion", "t[0-9]"], ["思考", "r\\.s"])
NO_MIX_TAGS = ("a[é]", "é.", "思[0-9]")


def test_key_off_answers_are_todays():
    """mixed off (the default), and mixed on without both other keys: the two refusals of
    tests/test_unicode_tags.py::test_no_mixing_with_class_tags, through every constructor."""
    ext = _ext()
    makers = (lambda t, **kw: ext.StreamFilter(t, **kw), lambda t, **kw: ext.Stripper(t, **kw),
              lambda t, **kw: ext.CpuEngine(t, **kw), lambda t, **kw: NativeEngine("cpu", t, **kw),
              lambda t, **kw: native.strip_fn(t, **kw))
    for tags in NO_MIX_SETS:
        assert ext.tagset_error(tags, True, True) == ext.tagset_error(tags, True, True, False) == \
            "class tags and non-ASCII tags do not mix in one tag set (runs with --impl python)"
        assert not native_tag_ok(tags, classes=True, unicode=True)
        for make in makers:
            with pytest.raises(ValueError, match="do not mix in one tag set"):
                make(tags, classes=True, unicode=True)
    for tag in NO_MIX_TAGS:
        assert ext.tagset_error([tag], True, True) == "tag needs regex semantics: " + tag
        for make in makers:
            with pytest.raises(ValueError, match="tag needs regex semantics"):
                make([tag], classes=True, unicode=True)
        # the key alone means nothing
        assert ext.tagset_error([tag], True, False, True) == "tag needs regex semantics: " + tag
        assert ext.tagset_error([tag], False, True, True) == "tag needs regex semantics: " + tag
    assert "do not mix" not in ext.tagset_error(NO_MIX_SETS[0], True, False, True)
    assert ext.tagset_error(NO_MIX_SETS[0], True, False, True) != ""


def test_make_engine_flag_and_cache():
    from quorum_amd.ops.engine import PyEngine, make_engine

    tags = ["think", "Réfl.xion"]
    assert isinstance(make_engine("cpu", tags, classes=True, unicode=True), PyEngine)
    eng = make_engine("cpu", tags, classes=True, unicode=True, mixed=True)
    assert isinstance(eng, NativeEngine) and eng.mixed
    assert make_engine("cpu", tags, classes=True, unicode=True, mixed=True) is eng
    a = make_engine("cpu", ["think"], classes=True, unicode=True, mixed=True)
    assert a is not make_engine("cpu", ["think"], classes=True, unicode=True)
    assert isinstance(make_engine("cpu", ["think", "a[é]"], classes=True, unicode=True, mixed=True), PyEngine)


# ---------------------------------------------------------------- filter / strip vs the oracle
def _feed_both(tags, chunks):
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, *ON)
    for ch in chunks:
        got, want = nat.feed(ch.encode("utf-8", "surrogatepass")).decode("utf-8", "surrogatepass"), py.feed(ch)
        assert got == want, (tags, chunks, ch, got, want)
    return py


def _split_chars(rng, text, lo, hi):
    out, i = [], 0
    while i < len(text):
        k = rng.randint(lo, hi)
        out.append(text[i:i + k])
        i += k
    return out


@pytest.mark.parametrize("ti", range(len(M.TAG_SETS)))
def test_filter_and_strip_fuzz(ti):
    """Random texts, the ambiguous fillers included (the C++ engine is exact): the streaming
    filter in random chunks and the strip equal the oracle's."""
    tags = M.TAG_SETS[ti]
    alpha, amb = M.alphabet(tags), M.ambiguous_for(tags)
    strip = native.strip_fn(tags, **M.KW)
    for seed in range(400):
        rng = random.Random(seed * 131 + ti)
        text = "".join(M.pieces(rng, tags, rng.randint(1, 14), alpha, amb, rng.choice([0.0, 0.3])))
        _feed_both(tags, _split_chars(rng, text, 1, rng.choice([1, 3, 8, 40])))
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)


SPLIT_CASES = [("<RÉFL0XION>x</réfl0xion>y", ["réfl.xion"]), ("<思7>x</思7>y", ["思[0-9]"])]


@pytest.mark.parametrize("text,tags", SPLIT_CASES)
@pytest.mark.parametrize("pre", ["", "<T>"])
def test_content_split_at_every_byte(text, tags, pre):
    """The content fed in two parts split after every byte, code point bytes included, outside
    and inside a block: the output equals the oracle's."""
    tags = tags + ["t"]
    raw = text.encode()
    for k in range(1, len(raw)):
        # (the class rules: outside a block a split decides what is held, so the oracle gets the
        # same split — at the start of the character that byte k cuts, which has not arrived yet)
        kc = len(raw[:k].decode("utf-8", "ignore"))
        py = ref.ThinkingTagFilter(tags)
        want = py.feed(pre) + py.feed(text[:kc]) + py.feed(text[kc:]) + py.feed("</t>!<")
        f = _ext().StreamFilter(tags, *ON)
        out = f.feed(pre.encode()) + f.feed(raw[:k]) + f.feed(raw[k:]) + f.feed(b"</t>!<")
        assert out.decode() == want, (text, pre, k)


@pytest.mark.parametrize("text,tags", SPLIT_CASES)
@pytest.mark.parametrize("escaped", [False, True])
@pytest.mark.parametrize("pre", ["", "<t>"])
def test_upstream_split_at_every_byte(text, tags, escaped, pre):
    """The raw upstream (one content event, its tag characters as UTF-8 or JSON-escaped) split
    at every byte: the C++ engine equals the oracle."""
    tags = tags + ["t"]
    body = json.dumps(text)[1:-1] if escaped else text
    if escaped:
        assert body.isascii() and "\\u" in body
    ev = ('data: {"choices": [{"index": 0, "delta": {"content": "%s"}}]}\n\n' % body).encode()
    head = ('data: {"choices": [{"index": 0, "delta": {"content": "%s"}}]}\n\n' % pre).encode() if pre else b""
    raw = head + ev + b'data: {"choices": [{"index": 0, "delta": {"content": "</t>!"}}]}\n\ndata: [DONE]\n\n'
    want = H.run_engine(H.python_engine(tags), [[raw]], [True], [True], H.EveryRound())
    cpu = NativeEngine("cpu", tags, **M.KW)
    for k0 in range(len(head) + 1, len(head) + len(ev), 6):
        streams = [[raw[:k], raw[k:]] for k in range(k0, min(k0 + 6, len(head) + len(ev)))]
        n = len(streams)
        got = H.run_engine(cpu, streams, [True] * n, [True] * n, H.EveryRound(), indices=[0] * n)
        assert got[0] == [want[0][0]] * n, (text, escaped, pre, k0)


@pytest.mark.parametrize("seed", range(120))
def test_cpu_engine_matches_python_mixed_tags(seed):
    """PyStream (the python engine) against the C++ engine over random batches."""
    rng = random.Random(seed)
    tags = M.TAG_SETS[seed % len(M.TAG_SETS)]
    alpha, amb = M.alphabet(tags), M.ambiguous_for(tags)
    raw = []
    for _ in range(4):
        parts = [H.event_bytes(rng, "".join(M.pieces(rng, tags, rng.randint(0, 6), alpha, amb, 0.2)))
                 for _ in range(rng.randint(1, 12))]
        raw.append(b"".join(parts) + b"data: [DONE]\n\n")
    streams = [H.split_random(rng, r, rng.choice([3, 17, 64, 400])) for r in raw]
    filt = [rng.random() < 0.7 for _ in range(4)]
    ts = rng.randint(0, 10**9)
    py = H.run_engine(H.python_engine(tags), streams, filt, [True] * 4, random.Random(ts))
    nat = H.run_engine(NativeEngine("cpu", tags, **M.KW), streams, filt, [True] * 4, random.Random(ts))
    assert py == nat, (tags, raw)


# ---------------------------------------------------------------- the rules, one by one
def _filter(tags, chunks):
    """The oracle's output per chunk (asserted equal to the C++ filter's)."""
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, *ON)
    out = []
    for ch in chunks:
        want = py.feed(ch)
        assert nat.feed(ch.encode()).decode() == want, (tags, chunks, ch)
        out.append(want)
    return out


def _strip(tags, text):
    want = ref.strip_thinking_tags(text, tags)
    assert native.strip_fn(tags, **M.KW)(text, True) == want, (tags, text)
    return want


def test_rule_source_text_holdback_outside_a_block():
    # the source text "<réfl.xion>" is held, folded: "<RÉ" + "FL" stays back
    assert _filter(["réfl.xion"], ["a<RÉ", "FL", "0XION>h", "</réfl0xion>b"]) == ["a", "", "", "b"]
    assert _filter(["réfl.xion"], ["a<RÉFL.", "XION>h</réfl.xion>b"]) == ["a", "b"]
    # "<réfl0" is no prefix of the source text: released, and the tag with it
    assert _filter(["réfl.xion"], ["a<réfl0", "xion>b"]) == ["a<réfl0", "xion>b"]
    # a character cut short is a prefix of its folded self (bytes through the C++ filter)
    f = _ext().StreamFilter(["réfl.xion"], *ON)
    up = "<RÉ".encode()
    assert f.feed(b"a" + up[:-1]) == b"a" and f.feed(up[-1:] + "FL.XION>x".encode()) == b""


def test_rule_class_aware_prefix_inside_a_block():
    assert _filter(["思[0-9]", "t"], ["<t>", "x<思", "7>y</思", "7>z</t>w"]) == ["", "", "", "w"]
    assert _filter(["réfl.xion"], ["<réfl0xion>a</RÉFL", "1XION>b"]) == ["", "b"]


def test_rule_list_order():
    for tags in (["r.flexion", "réflexion"], ["réflexion", "r.flexion"]):
        assert _strip(tags, "<réflexion>a</réflexion>b<rEflexion>c</reflexion>d") == "bd"
        assert _strip(tags, "<RÉFLEXION>a</rxflexion>b</réflexion>c") == "c"
        _filter(tags, ["<RÉFLEXION>a</rxflexion>b</réflexion>c"])


def test_rule_dot_and_newline():
    # streaming: a dot takes no newline; the strip's dot does
    assert _filter(["é.", "t"], ["a<é\n>b"]) == ["a<é\n>b"]
    assert _strip(["é.", "t"], "a<é\n>b</É\n>c") == "ac"


def test_rule_close_is_the_captured_text():
    assert _strip(["思[0-9]"], "<思7>q</思8>r</思7>s") == "s"
    assert _strip(["思[0-9]"], "<思7>x</思8>") == "<思7>x</思8>"
    assert _strip(["réfl.xion"], "<réfl0xion>1</RÉFL0XION>2") == "2"
    assert _strip(["réfl.xion"], "<RÉFL0XION>x</réfl0xion>y") == "y"
    assert _strip(["réfl.xion"], "<réflAxion>1</RÉFLaXION>2") == "2"
    # the set's own pair character at a class position folds too
    assert _strip(["réfl.xion"], "<réflÉxion>1</réfléxion>2") == "2"


def test_rule_wide_class_element_takes_one_code_point():
    assert _strip(["th.nk", "思考"], "<th日nk>x</TH日NK>y") == "y"
    assert _filter(["th.nk", "思考"], ["<th" + "é" + "nk>x"]) == [""]
    assert _filter(["th[a-z]nk", "思考"], ["<th" + "é" + "nk>x"]) == ["<thénk>x"]
    assert _filter(["思[0-9]", "t"], ["<思é>x"]) == ["<思é>x"]


# ---------------------------------------------------------------- config + server
def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_mixed_tags is False
    both = {"native_regex_tags": True, "native_unicode_tags": True}
    assert RuntimeConfig.from_config({"runtime": dict(both, native_mixed_tags=True)}).native_mixed_tags is True
    with pytest.raises(ValueError, match="native_mixed_tags"):
        RuntimeConfig.from_config({"runtime": dict(both, native_mixed_tags="yes")})
    for rt in ({"native_mixed_tags": True}, {"native_mixed_tags": True, "native_regex_tags": True},
               {"native_mixed_tags": True, "native_unicode_tags": True}):
        with pytest.raises(ValueError, match="native_regex_tags.*native_unicode_tags"):
            RuntimeConfig.from_config({"runtime": rt})


ALL_KEYS = {"native_regex_tags": True, "native_unicode_tags": True, "native_mixed_tags": True}


def mixed_server_scenario(tags=("think", "réfl.xion", "思考")):
    """tests/test_unicode_tags.py's streamed session (its <RÉFLEXION> is the tag réfl.xion here)
    with the three keys on."""
    import test_unicode_tags as TU

    cfg, up, body, auth = TU.unicode_server_scenario(tags)
    cfg["runtime"] = dict(ALL_KEYS)
    return cfg, up, body, auth


def test_native_config_key_on_and_off():
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    cfg = mixed_server_scenario()[0]
    d = native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tag_mixed"] is True and d["tag_unicode"] is True and d["tag_classes"] is True
    assert d["tags"] == ["think", "réfl.xion", "思考"]
    off = dict(cfg, runtime={"native_regex_tags": True, "native_unicode_tags": True})
    with pytest.raises(NativeUnsupported, match="need regex semantics: run with --impl python"):
        native_config(off, "127.0.0.1", 1, "cpu", 0, 1)


def test_native_server_mixed_tags_match_python():
    import test_native_server as T

    T._compare(mixed_server_scenario(), "mixed_tags", None)
