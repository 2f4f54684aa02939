"""Non-ASCII thinking tags on the native C++ engine (``unicode=True``,
``runtime.native_unicode_tags``).

The reference joins ``thinking_tags`` into a Python regex, so ``思考`` or ``réflexion`` is a tag
there, matched under IGNORECASE.  With the keyword on the native engines take tags whose
non-ASCII characters are uncased or one of a simple case pair, and fold the text as they read
it.  These tests pin the case rule against ``unicodedata``, the parser's limits, and the filter
/ strip / engine semantics against the python oracle (``quorum_amd/ops/reference.py``).
"""
import json
import random

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import native_tag_ok
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import unicode_tag_cases as U

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _ext():
    return native.require()


# ---------------------------------------------------------------- the rule
def test_rule_sweep():
    """Every assigned code point: what the extension accepts is inside the rule, and a pair's
    partner is the rule's partner.  (The table may only ever err by refusing.)"""
    ext = _ext()
    pairs, refused = U.case_rule()
    assert len(pairs) % 2 == 0 and all(pairs[pairs[c]] == c for c in pairs)
    n_pairs = 0
    for cp in range(0x80, 0x110000):
        if not U.category_ok(cp):
            continue
        kind, partner = ext.unicode_tag_char(cp)
        if kind == 2:
            continue
        assert cp not in refused, hex(cp)
        if kind == 1:
            assert pairs.get(cp) == partner, (hex(cp), hex(partner))
            n_pairs += 1
        else:
            assert cp not in pairs, hex(cp)  # (an "uncased" answer for a pair would not fold)
    assert n_pairs > 2000  # (Unicode 13: 2,490)


def test_rule_examples():
    ext = _ext()
    for ch in U.MUST_ACCEPT:
        assert native_tag_ok([ch], unicode=True), ch
        assert native_tag_ok(["think", "a" + ch], unicode=True), ch
        ext.StreamFilter([ch], unicode=True)
    for ch in U.MUST_REFUSE:
        assert not native_tag_ok([ch], unicode=True), hex(ord(ch))
        assert not native_tag_ok(["think", "a" + ch + "b"], unicode=True), hex(ord(ch))
    assert not native_tag_ok(["é"], unicode=True)  # decomposed: tags must be precomposed
    assert ext.unicode_tag_char(0x10428) == (1, 0x10400) and ext.unicode_tag_char(0x10400) == (1, 0x10428)
    assert ext.unicode_tag_char(ord("é")) == (1, ord("É")) and ext.unicode_tag_char(ord("思")) == (0, ord("思"))
    assert ext.unicode_tag_char(0x212A)[0] == 2  # Kelvin sign


def test_pairs_match_under_re_ignorecase():
    """Every accepted pair is a pair to ``re`` too, and folds with ``str.lower`` (the holdback)."""
    import re

    ext = _ext()
    pairs, _ = U.case_rule()
    for cp, other in pairs.items():
        if ext.unicode_tag_char(cp)[0] != 1:
            continue
        assert re.fullmatch(chr(cp), chr(other), re.I), hex(cp)
        assert chr(cp).lower() == chr(other).lower(), hex(cp)


# ---------------------------------------------------------------- parser limits
def test_length_limit():
    ext = _ext()
    for tag in ("思" * 20 + "a", "a" * 61, "é" * 30 + "a"):  # 61 bytes
        assert len(tag.encode()) == 61
        assert ext.tagset_ok([tag], False, True), tag
        assert native_tag_ok([tag], unicode=True)
    for tag in ("思" * 20 + "ab", "a" * 62, "é" * 31):  # 62 bytes
        assert len(tag.encode()) == 62
        assert "unsupported tag length" in ext.tagset_error([tag], False, True), tag
        assert not native_tag_ok([tag], unicode=True)


def test_tag_count_after_lowercasing():
    ext = _ext()
    assert ext.tagset_size(["É", "é"], False, True) == 1
    assert ext.tagset_size(["RÉFLEXION", "réflexion", "Réflexion", "思考"], False, True) == 2
    sixteen = [f"é{i}" for i in range(16)]
    assert ext.tagset_ok(sixteen + [t.upper() for t in sixteen], False, True)
    assert "too many thinking tags" in ext.tagset_error(sixteen + ["é16"], False, True)


def test_pair_count_limit():
    ext = _ext()
    ps = "àáâãäæçèéêëìíîïðñòóôõöøùúûüýþÿяю"  # 32 pair characters
    assert len(set(ps)) == 32 and all(ext.unicode_tag_char(ord(c))[0] == 1 for c in ps)
    assert ext.tagset_ok([ps[:16], ps[16:]], False, True)
    assert ext.tagset_ok([ps[:16], ps[16:].upper(), ps[:16].upper(), "思考"], False, True)
    assert "too many case-pair characters" in ext.tagset_error([ps[:16], ps[16:], "ạ"], False, True)


def test_no_mixing_with_class_tags():
    ext = _ext()
    for tags in (["th.nk", "思考"], ["réflexion", "t[0-9]"], ["思考", "r\\.s"]):
        assert "do not mix" in ext.tagset_error(tags, True, True), tags
        assert not native_tag_ok(tags, classes=True, unicode=True)
    for tag in ("a[é]", "é.", "思[0-9]"):
        assert "regex semantics" in ext.tagset_error([tag], True, True), tag
    assert ext.tagset_ok(["th.nk", "think"], True, True) and ext.tagset_ok(["思考", "think"], True, True)


def test_keyword_off_refuses_every_non_ascii_tag():
    """unicode=False (the default): today's refusal with today's message, everywhere."""
    ext = _ext()
    for tag in U.MUST_ACCEPT + U.MUST_REFUSE + ["réflexion", "思考"]:
        for classes in (False, True):
            assert not native_tag_ok(["think", tag], classes=classes)
            assert not native_tag_ok(["think", tag], classes=classes, unicode=False)
            assert not ext.tagset_ok(["think", tag], classes)
            assert ext.tagset_error(["think", tag], classes, False) == "tag needs regex semantics: " + tag
        for make in (lambda t: ext.StreamFilter(["think", t]), lambda t: ext.Stripper(["think", t]),
                     lambda t: ext.CpuEngine(["think", t]), lambda t: NativeEngine("cpu", ["think", t]),
                     lambda t: native.strip_fn(["think", t]), lambda t: ext.StreamFilter(["think", t], classes=True)):
            with pytest.raises(ValueError, match="tag needs regex semantics"):
                make(tag)


def test_make_engine_flag_and_cache():
    from quorum_amd.ops.engine import PyEngine, make_engine

    tags = ["think", "Réflexion"]
    assert isinstance(make_engine("cpu", tags), PyEngine)
    eng = make_engine("cpu", tags, unicode=True)
    assert isinstance(eng, NativeEngine) and eng.unicode
    assert make_engine("cpu", tags, unicode=True) is eng
    assert make_engine("cpu", ["think"], unicode=True) is not make_engine("cpu", ["think"])
    assert isinstance(make_engine("cpu", ["think", "ω"], unicode=True), PyEngine)
    ext = _ext()
    assert ext.tagset_has_classes(tags, False, True) and not ext.tagset_has_classes(["think", "思考"], False, True)


# ---------------------------------------------------------------- filter / strip vs the oracle
def _feed_both(tags, chunks):
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, unicode=True)
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


@pytest.mark.parametrize("ti", range(len(U.TAG_SETS)))
def test_filter_and_strip_fuzz(ti):
    tags = U.TAG_SETS[ti]
    alpha = U.alphabet(tags)
    strip = native.strip_fn(tags, unicode=True)
    for seed in range(600):
        rng = random.Random(seed * 131 + ti)
        text = "".join(U.pieces(rng, tags, rng.randint(1, 14), alpha))
        _feed_both(tags, _split_chars(rng, text, 1, rng.choice([1, 3, 8, 40])))
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)


def test_hand_cases():
    strip = native.strip_fn(["é", "思考"], unicode=True)
    for text in ["<é>x</É>y", "<É>x</é>y", " a<思考>q</思考>b<é> ", "<è>x</è>y", "<思考>x</思耂>y</思考>z", "<É>x</È>y</É>z"]:
        assert strip(text, True) == ref.strip_thinking_tags(text, ["é", "思考"]), text
    assert strip("<é>x</É>y", True) == "y"
    _feed_both(["réflexion"], ["a<RÉFLEXION>x</Réflexion>y", "<RÈFLEXION>", "<réflexion", ">z"])
    _feed_both(["я"], ["<Я>", "x</я>", "y<Ю>", "<я", ">", "</Я", ">w"])


@pytest.mark.parametrize("text,tags", [("<思考>x</思考>y", ["思考"]), ("<RÉFLEXION>x</réflexion>y", ["réflexion"]),
                                       ("<\U00010400X>x</\U00010428x>y", ["\U00010428x"])])
@pytest.mark.parametrize("pre", ["", "<T>"])
def test_content_split_at_every_byte(text, tags, pre):
    """The content fed in two parts split after every byte, code point bytes included, outside
    and inside a block: the output equals the oracle's over the whole text."""
    tags = tags + ["t"]
    raw = text.encode()
    py = ref.ThinkingTagFilter(tags)
    want = py.feed(pre) + py.feed(text) + py.feed("</t>!<")
    for k in range(1, len(raw)):
        f = _ext().StreamFilter(tags, unicode=True)
        out = f.feed(pre.encode()) + f.feed(raw[:k]) + f.feed(raw[k:]) + f.feed(b"</t>!<")
        assert out.decode() == want, (text, pre, k)


def _escaped(s):
    return json.dumps(s)[1:-1]


@pytest.mark.parametrize("text,tags", [("<思考>x</思考>y", ["思考"]), ("<RÉFLEXION>x</réflexion>y", ["réflexion"]),
                                       ("<\U00010400X>x</\U00010428x>y", ["\U00010428x"])])
@pytest.mark.parametrize("escaped", [False, True])
@pytest.mark.parametrize("pre", ["", "<t>"])
def test_upstream_split_at_every_byte(text, tags, escaped, pre):
    """The raw upstream (one content event, its tag characters as UTF-8 or JSON-escaped:
    \\u601d, \\u00c9, \\ud801\\udc00) split at every byte: the C++ engine equals the oracle."""
    tags = tags + ["t"]
    body = _escaped(text) if escaped else text
    if escaped:
        assert body.isascii() and "\\u" in body
    ev = ('data: {"choices": [{"index": 0, "delta": {"content": "%s"}}]}\n\n' % body).encode()
    head = ('data: {"choices": [{"index": 0, "delta": {"content": "%s"}}]}\n\n' % pre).encode() if pre else b""
    raw = head + ev + b'data: {"choices": [{"index": 0, "delta": {"content": "</t>!"}}]}\n\ndata: [DONE]\n\n'
    want = H.run_engine(H.python_engine(tags), [[raw]], [True], [True], H.EveryRound())
    cpu = NativeEngine("cpu", tags, unicode=True)
    for k0 in range(len(head) + 1, len(head) + len(ev), 6):
        streams = [[raw[:k], raw[k:]] for k in range(k0, min(k0 + 6, len(head) + len(ev)))]
        n = len(streams)
        got = H.run_engine(cpu, streams, [True] * n, [True] * n, H.EveryRound(), indices=[0] * n)
        assert got[0] == [want[0][0]] * n, (text, escaped, pre, k0)


# ---------------------------------------------------------------- whole engine
@pytest.mark.parametrize("seed", range(150))
def test_cpu_engine_matches_python_unicode_tags(seed):
    rng = random.Random(seed)
    tags = U.TAG_SETS[seed % len(U.TAG_SETS)]
    alpha = U.alphabet(tags)
    raw = []
    for _ in range(4):
        parts = [H.event_bytes(rng, "".join(U.pieces(rng, tags, rng.randint(0, 6), alpha))) for _ in range(rng.randint(1, 12))]
        raw.append(b"".join(parts) + b"data: [DONE]\n\n")
    streams = [H.split_random(rng, r, rng.choice([3, 17, 64, 400])) for r in raw]
    filt = [rng.random() < 0.7 for _ in range(4)]
    emit = [True] * 4
    ts = rng.randint(0, 10**9)
    py = H.run_engine(H.python_engine(tags), streams, filt, emit, random.Random(ts))
    nat = H.run_engine(NativeEngine("cpu", tags, unicode=True), streams, filt, emit, random.Random(ts))
    assert py == nat, (tags, raw)


# ---------------------------------------------------------------- config + server
def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_unicode_tags is False
    assert RuntimeConfig.from_config({"runtime": {"native_unicode_tags": True}}).native_unicode_tags is True
    with pytest.raises(ValueError, match="native_unicode_tags"):
        RuntimeConfig.from_config({"runtime": {"native_unicode_tags": "yes"}})


def unicode_server_scenario(tags=("think", "réflexion", "思考")):
    """One streamed session: tags in lower, upper and mixed case, split over events, a
    look-alike, an unclosed open."""
    from conftest import cfg_parallel, sse_chunk

    import test_native_server as T

    s1 = [sse_chunk({"role": "assistant"}), sse_chunk({"content": "A <RÉFLEXION>hid"}), sse_chunk({"content": "den</réflexion> B <Ré"}),
          sse_chunk({"content": "flexion>x</THINK>y</RÉFLEXION> C <rèflexion>kept</rèflexion> <思"}),
          sse_chunk({"content": "考>w</思考> D <思耂>"}), sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    s2 = [sse_chunk({"content": "<think>t</think>E <Réflexion>u</réFLEXION>F</réflexion> <RÉFLEXION"}), sse_chunk({}, finish="stop"),
          b"data: [DONE]\n\n"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, hide_final_think=True, thinking_tags=list(tags)))
    cfg["runtime"] = {"native_unicode_tags": True}
    return (cfg, {"b1.test": ("stream", 200, T.split7(s1)), "b2.test": ("stream", 200, s2)},
            {"messages": T.MSG, "stream": True}, T.AUTH)


def test_native_config_key_on_and_off():
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    cfg = unicode_server_scenario()[0]
    d = native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tag_unicode"] is True and d["tag_classes"] is False and d["tags"] == ["think", "réflexion", "思考"]
    off = dict(cfg, runtime={})
    with pytest.raises(NativeUnsupported, match="need regex semantics: run with --impl python"):
        native_config(off, "127.0.0.1", 1, "cpu", 0, 1)
    bad = unicode_server_scenario(("think", "ω"))[0]
    with pytest.raises(NativeUnsupported, match="need regex semantics: run with --impl python"):
        native_config(bad, "127.0.0.1", 1, "cpu", 0, 1)


def test_native_server_unicode_tags_match_python():
    import test_native_server as T

    T._compare(unicode_server_scenario(), "unicode_tags", None)
