"""Unbounded repetition in thinking tags — ``+``, ``*`` and ``{m,}`` after one element — on the
native C++ engine (``repeat=True``, ``runtime.native_repeat_tags``, with ``classes``, ``variants`` and
``extended``).

Such a quantifier expands into 4 rows beyond its minimum count (``kRepeatRows``) and the longest
row is open-ended at its last copy: the exact host walk takes the rest of the run there.  The
parser refuses a repeated element that shares a character with what can follow the run — there the
regex backtracks into the run and the rows are not the tag.  These tests pin the parser (every
accepted and refused form, the key off), the rows, the filter and the strip against the python
oracle (``quorum_amd/ops/reference.py``), the 64-byte bound, and the overlap rule by enumeration
against ``re``.
"""
import itertools
import random
import re

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import native_tag_ok
from quorum_amd.ops.native import NativeEngine

import class_tag_cases as C
import engine_harness as H
import repeat_tag_cases as X

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _ext():
    return native.require()


def _err(tags, **kw):
    return _ext().tagset_error(list(tags), **kw)


# ---------------------------------------------------------------- 1: the parser's table
@pytest.mark.parametrize("tag,rows,_alphabet", X.ACCEPTED)
def test_accepted_forms_and_their_rows(tag, rows, _alphabet):
    assert _err([tag], **X.KW) == ""
    assert native.tagset_rows([tag], **X.KW) == [(r, 0) for r in rows]
    assert native.tagset_kind([tag], **X.KW) == "class"
    assert native_tag_ok([tag], **X.KW)
    # the key off: today's refusal, verbatim (this is the test that fails without the feature)
    assert _err([tag], **X.OFF_KW) == X.NEEDS + tag
    assert not native_tag_ok([tag], **X.OFF_KW)


@pytest.mark.parametrize("tag,msg", X.REFUSED)
def test_refused_forms_and_their_messages(tag, msg):
    kw = X.MIXED_KW if any(ord(c) >= 0x80 for c in tag) else X.KW
    assert _err(["think", tag], **kw) == msg + tag
    assert not native_tag_ok(["think", tag], **kw)
    for make in (lambda: _ext().StreamFilter([tag], **kw), lambda: _ext().Stripper([tag], **kw),
                 lambda: NativeEngine("cpu", [tag], **kw), lambda: native.strip_fn([tag], **kw)):
        with pytest.raises(ValueError, match=re.escape(msg + tag)):
            make()
    off = dict(kw, repeat=False)
    for k in (off, dict(off, extended=False, repeat=True), dict(off, variants=False, repeat=True)):
        assert _err(["think", tag], **k) == X.NEEDS + tag, k


def test_rows_equal_the_tag_in_re():
    """A check of this file's expectation table, not of the native code: with the open-ended element
    written as re's ``+``, the ordered alternation of the rows has the tag's matches."""
    rng = random.Random(5)
    for tag, rows, alphabet in X.ACCEPTED:
        alt = "|".join(rows)
        a, b = re.compile("<(%s)>" % tag, re.I), re.compile("<(%s)>" % alt, re.I)
        for _ in range(300):
            text = "<" + "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 9))) + ">"
            assert bool(a.fullmatch(text)) == bool(b.fullmatch(text)), (tag, text)


def test_row_limits_hold():
    two = ["step\\d+", "thought_\\d+"]  # two numbered tags are 8 rows
    assert _err(["think"] + two, **X.KW) == "" and _ext().tagset_size(["think"] + two, **X.KW) == 9
    full = ["a\\d+[a-z]+"]
    assert _ext().tagset_size(full, **X.KW) == 16
    assert _err(full + ["x"], **X.KW) == X.TOO_MANY + "x"  # 17 rows
    assert _err(["s\\d+", "s\\d{4,5}"], **X.KW) == ""  # (an open-ended row is no closed one: same_row)
    assert _err(["s\\d{1,4}", "s\\d\\d"], **X.KW) == X.SAME_PATTERN + "s\\d{1,4}, s\\d\\d"
    assert _err(["s\\d+", "s\\d\\d"], **X.KW) == X.SAME_PATTERN + "s\\d+, s\\d\\d"
    assert _err(["s\\d+", "s\\d{3,}"], **X.KW) == X.SAME_PATTERN + "s\\d+, s\\d{3,}"  # (s\d\d\d, closed, in both)
    assert _err(["a" * 59 + "\\d+"], **X.KW) == X.NEEDS + "a" * 59 + "\\d+"  # a source text of 62 bytes
    assert _err(["a{58,}"], **X.KW) == "" and native.tagset_rows(["a{58,}"], **X.KW)[0] == ("a" * 61 + "+", 0)


def test_kind_mixed_sets_and_the_key_off():
    assert native.tagset_kind(["think", "step\\d+"], **X.KW) == "class"
    assert native.tagset_kind(["思\\d+"], **X.MIXED_KW) == "mixed"
    assert native.tagset_rows(["思\\d+"], **X.MIXED_KW) == [("思\\d\\d\\d\\d+", 0), ("思\\d\\d\\d", 0), ("思\\d\\d", 0), ("思\\d", 0)]
    no_mixed = dict(X.KW, unicode=True)
    assert _err(["思\\d+"], **no_mixed) == "class tags and non-ASCII tags do not mix in one tag set (runs with --impl python)"
    # tags without an unbounded quantifier are what they are with the key off
    for tags in (["think"], ["th.nk", "t[0-9]?"], ["think(ing)?"], ["step\\d{1,2}", "a\\w\\s"]):
        assert native.tagset_rows(tags, **X.KW) == native.tagset_rows(tags, **X.OFF_KW)
        assert native.tagset_kind(tags, **X.KW) == native.tagset_kind(tags, **X.OFF_KW)
        for text in (b"<t>", b"<step12>x</step1>", "<t٣><step1٣>".encode(), b"<a_ >"):
            assert (native.class_suspects(tags, text, variants=True, extended=True, repeat=True)
                    == native.class_suspects(tags, text, variants=True, extended=True))


# ---------------------------------------------------------------- 2: differential against the oracle
def _feed_both(tags, chunks, kw):
    py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **kw)
    for ch in chunks:
        got, want = nat.feed(ch.encode()).decode(), py.feed(ch)
        assert got == want, (tags, chunks, ch, got, want)
    assert nat.flush().decode() == py.flush(), (tags, chunks)


@pytest.mark.parametrize("k", range(len(X.DIFF_SETS)))
def test_filter_and_strip_against_the_oracle(k):
    tags, kw, stems, run = X.DIFF_SETS[k]
    assert native.tagset_ok(tags, **kw), _err(tags, **kw)
    strip = native.strip_fn(tags, **kw)
    longest = 0
    for seed in range(500):
        rng = random.Random(1000 * k + seed)
        text = X.diff_text(rng, rng.randint(1, 16), stems, run)
        longest = max([longest] + [len(m) for m in re.findall("[%s%s%s]+" % (re.escape(run), X.D3, X.NBSP), text)])
        _feed_both(tags, C.split_chars(rng, text, 1, rng.choice([1, 2, 5, 9, 40])), kw)
        assert strip(text, True) == ref.strip_thinking_tags(text, tags), (tags, text)
    # (runs stay far from the 61-byte bound, so the oracle is exact for every generated text; and
    # they pass the rows' 4 copies, so the open-ended walk was run)
    assert X.ROWS < longest <= 3 * X.MAX_RUN, longest


@pytest.mark.parametrize("seed", range(16))
def test_cpu_engine_matches_python(seed):
    """PyStream (the python engine) against the C++ engine over batches of SSE streams."""
    rng = random.Random(seed)
    tags, kw, stems, run = X.DIFF_SETS[seed % len(X.DIFF_SETS)]
    raw = []
    for _ in range(4):
        parts = [H.event_bytes(rng, X.diff_text(rng, rng.randint(0, 6), stems, run)) for _ in range(rng.randint(1, 10))]
        raw.append(b"".join(parts) + b"data: [DONE]\n\n")
    streams = [H.split_random(rng, r, rng.choice([3, 17, 64, 400])) for r in raw]
    filt = [rng.random() < 0.7 for _ in range(4)]
    ts = rng.randint(0, 10**9)
    py = H.run_engine(H.python_engine(tags), streams, filt, [True] * 4, random.Random(ts))
    nat = H.run_engine(NativeEngine("cpu", tags, **kw), streams, filt, [True] * 4, random.Random(ts))
    assert py == nat, (tags, raw)


def _feeds(tags, chunks, kw=X.KW):
    py, f = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **kw)
    out = [py.feed(c) for c in chunks]
    assert [f.feed(c.encode()).decode() for c in chunks] == out, chunks
    return out


def test_holdback_outside_and_inside_a_block():
    tags = ["think", "step\\d+"]
    # outside a block the SOURCE text is held, an instance is not: released, and no tag later
    assert _feeds(tags, ["a<step\\d"]) == ["a"]
    assert _feeds(tags, ["a<step\\d", "+>b"]) == ["a", "<step\\d+>b"]
    assert _feeds(tags, ["a<step1", "2>b"]) == ["a<step1", "2>b"]
    # inside a block a prefix of a row is kept, inside the open-ended run too
    assert _feeds(tags, ["<think>", "x<step1", "2>y</step12>z</think>w"]) == ["", "", "w"]
    assert _feeds(tags, ["<think>", "x<step1234", "567", "8>y</step12345", "678>z</think>w"]) == ["", "", "", "", "w"]
    assert _feeds(tags, ["<think>", "x<step1234", "x>y</think>w"]) == ["", "", "w"]
    for text in ("<step\\d+>", "<step7>", "<step1234567>", "</step12" + X.D3 + "4567>", "<step" + X.D3 * 6 + ">"):
        for pre in ("", "<think>"):
            for k in range(1, len(text)):
                _feeds(tags, [pre, text[:k], text[k:], "x</step7>!</think>?<"])


def test_strip_close_is_the_captured_text():
    def strip(tags, text, kw=X.KW):
        want = ref.strip_thinking_tags(text, tags)
        assert native.strip_fn(tags, **kw)(text, True) == want, (tags, text)
        return want

    assert strip(["step\\d+"], "<step12>a</step1>b</step12>c") == "c"
    assert strip(["step\\d+"], "<step12345>a</step1234>b</step123456>c</step12345>d") == "d"
    assert strip(["step\\d+"], "<step12345>a</step1234>b") == "<step12345>a</step1234>b"
    assert strip(["step\\d+"], "<STEP7>x</step7>y") == "y"
    assert strip(["step\\d+"], "<step1٣345>a</step1٣345>b") == "b"
    assert strip(["think\\s*"], "<think>a</think >b</think>c<think \n>d</THINK \n>e") == "ce"
    assert strip(["hm+", "h\\d+"], "<hmmmmmm>a</hmm>b</HMMMMMM>c<h123456>d</h123456>e<hm1>") == "ce<hm1>"
    assert strip(["v\\d+\\.\\d+"], "<v1.23456>a</v1.2345>b</v1.23456>c<v12345.6>d</v12345.6>e<v1.>") == "ce<v1.>"
    assert strip(["思\\d+"], "<思12345>a</思1234>b</思12345>c<思x>", X.MIXED_KW) == "c<思x>"


# ---------------------------------------------------------------- 3: the 64-byte bound
def test_a_match_is_at_most_61_bytes():
    """"</" + match + ">" is at most 64 bytes, the holdback's size: ``<step`` + 57 digits + ``>`` is
    a tag on both sides, one digit more is a tag in ``re`` and text natively — the third documented
    difference from the python implementation."""
    tags = ["think", "step\\d+"]
    strip = native.strip_fn(tags, **X.KW)
    fits, over = "step" + "7" * 57, "step" + "7" * 58
    assert len("</" + fits + ">") == 64
    for cut in (1, 9, 30, 63, 200):
        text = "<think>a<%s>b</think>c</%s>d</think>e" % (fits, fits)
        _feed_both(tags, [text[i:i + cut] for i in range(0, len(text), cut)], X.KW)
    text = "p<%s>x</%s>y" % (fits, fits)
    assert strip(text, True) == ref.strip_thinking_tags(text, tags) == "py"
    # one digit more
    for cut in (1, 9, 30, 63, 200):
        text = "<think>a<%s>b</think>c" % over
        py, nat = ref.ThinkingTagFilter(tags), _ext().StreamFilter(tags, **X.KW)
        chunks = [text[i:i + cut] for i in range(0, len(text), cut)]
        want = "".join(py.feed(c) for c in chunks) + py.flush()
        got = b"".join(nat.feed(c.encode()) for c in chunks) + nat.flush()
        assert want == "" and got.decode() == "c", (cut, want, got)
    text = "p<%s>x</%s>y" % (over, over)
    assert ref.strip_thinking_tags(text, tags) == "py" and strip(text, True) == text
    # a follower after the run counts too, and so does a character of several bytes
    strip = native.strip_fn(["v\\d+\\.\\d+"], **X.KW)
    for name, tag in (("v" + "1" * 58 + ".5", True), ("v" + "1" * 58 + ".55", False), ("v1." + "5" * 57 + X.D3, False),
                      ("v1." + "5" * 56 + X.D3, True)):
        text = "p<%s>x</%s>y" % (name, name)
        assert len(name.encode()) <= 61 if tag else len(name.encode()) > 61
        assert ref.strip_thinking_tags(text, ["v\\d+\\.\\d+"]) == "py"
        assert strip(text, True) == ("py" if tag else text), name


# ---------------------------------------------------------------- 4: determinism, by enumeration
@pytest.mark.parametrize("tag,_rows,alphabet", X.ACCEPTED)
def test_every_short_string_matches_as_in_re(tag, _rows, alphabet):
    """Every string up to length 7 over six characters drawn from the tag: the native match of
    "<" + s + ">" is ``re.fullmatch`` under IGNORECASE.  One strip per length: an item is
    "<s>#</s>;", removed exactly when "<s>" is an open (its close repeats the capture)."""
    assert len(set(alphabet)) == 6 and not set(alphabet) & set("<>/#;")
    pat = re.compile(tag, re.I)
    strip = native.strip_fn([tag], **X.KW)
    matched = 0
    for n in range(8):
        names = ["".join(p) for p in itertools.product(alphabet, repeat=n)]
        text = "^" + "".join("<%s>#</%s>;" % (s, s) for s in names) + "$"
        want = "^" + "".join(";" if pat.fullmatch(s) else "<%s>#</%s>;" % (s, s) for s in names) + "$"
        matched += sum(1 for s in names if pat.fullmatch(s))
        assert strip(text, True) == want, (tag, n)
    assert matched > 0 or tag == "thought_\\d+", tag  # (its shortest match has 9 characters: the refusals only)


# ---------------------------------------------------------------- the kernels' suspect rule, on the host
def test_suspect_rule_for_open_ended_rows():
    cs = lambda tags, text, **kw: native.class_suspects(tags, text, variants=True, extended=True, repeat=True, **kw)  # noqa: E731
    tags = ["think", "step\\d+"]
    for text in (b"<step1>", b"</step12>", b"<step123>x</STEP1234>", b"<step>", b"<stepx>", b"<step1x>", b"<step1234", b"<step1234 5>",
                 b"<think>"):
        assert cs(tags, text) == 0 == cs(tags, text, strip=True), text
    for text in (b"<step12345>", b"</step12345>", b"<step12345", b"<step12345x>", "<step1234٣>".encode(), "<step12٣>".encode()):
        assert cs(tags, text) == 1 == cs(tags, text, strip=True), text
    # '*' with no copy, and a run of spaces past the rows
    assert cs(["think\\s*"], b"<think></think ><think    >") == 0
    assert cs(["think\\s*"], b"<think     >") == 1
    # a repeated literal: its open-ended copy is a class of one letter
    assert cs(["hm+"], b"<hm><hmmmm></HMMMM>") == 0 and cs(["hm+"], b"<hmmmmm>") == 1
    # a follower after the run
    assert cs(["v\\d+\\.\\d+"], b"<v1234.1234>") == 0
    assert cs(["v\\d+\\.\\d+"], b"<v12345.1>") == 1 and cs(["v\\d+\\.\\d+"], b"<v1.12345>") == 1
    mk = dict(unicode=True, mixed=True)
    assert cs(["思\\d+"], "<思1234>x</思12>".encode(), **mk) == 0 and cs(["思\\d+"], "<思12345>".encode(), **mk) == 1


# ---------------------------------------------------------------- config + server
KEYS = {"native_regex_tags": True, "native_variant_tags": True, "native_extended_tags": True, "native_repeat_tags": True}


def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_repeat_tags is False
    assert RuntimeConfig.from_config({"runtime": KEYS}).native_repeat_tags is True
    with pytest.raises(ValueError, match="native_repeat_tags must be true or false"):
        RuntimeConfig.from_config({"runtime": dict(KEYS, native_repeat_tags="yes")})
    for missing in ("native_regex_tags", "native_variant_tags", "native_extended_tags"):
        rt = {k: v for k, v in KEYS.items() if k != missing}
        with pytest.raises(ValueError) as e:
            RuntimeConfig.from_config({"runtime": rt})
        if missing == "native_extended_tags":
            assert str(e.value) == ("runtime.native_repeat_tags needs runtime.native_regex_tags, "
                                    "runtime.native_variant_tags and runtime.native_extended_tags all true")


def test_make_engine_flag_and_cache():
    from quorum_amd.ops.engine import PyEngine, make_engine

    tags = ["Think", "step\\d+"]
    assert isinstance(make_engine("cpu", tags, **X.OFF_KW), PyEngine)
    assert isinstance(make_engine("cpu", tags, classes=True, variants=True, repeat=True), PyEngine)
    eng = make_engine("cpu", tags, **X.KW)
    assert isinstance(eng, NativeEngine) and eng.repeat
    assert make_engine("cpu", tags, **X.KW) is eng
    assert make_engine("cpu", ["think"], **X.KW) is not make_engine("cpu", ["think"], **X.OFF_KW)
    assert isinstance(make_engine("cpu", ["think.*"], **X.KW), PyEngine)


def repeat_server_scenario(tags=("think", "step\\d+")):
    """One streamed session: runs inside and beyond the rows in both cases, a tag split over events
    inside its run, a close of another run, a near miss, the source text, a non-ASCII digit in a
    run, an unclosed open."""
    from conftest import cfg_parallel, sse_chunk

    import test_native_server as T

    s1 = [sse_chunk({"role": "assistant"}), sse_chunk({"content": "A <STEP1>hid"}),
          sse_chunk({"content": "den</step1> B <ste"}), sse_chunk({"content": "p123"}),
          sse_chunk({"content": "456>x</step12345>y</STEP123456> C <step"}),
          sse_chunk({"content": "7>gone</step7> <stepx>k</stepx> D <step\\d+> <step1٣2>h</step1٣2> E"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    s2 = [sse_chunk({"content": "<think>t<step31>u</think>v</step31>F <Step1234>w</step1234> G<step4"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, hide_final_think=True, thinking_tags=list(tags)))
    cfg["runtime"] = dict(KEYS)
    return (cfg, {"b1.test": ("stream", 200, T.split7(s1)), "b2.test": ("stream", 200, s2)},
            {"messages": T.MSG, "stream": True}, T.AUTH)


def test_native_config_key_on_and_off():
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    cfg = repeat_server_scenario()[0]
    d = native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tag_repeat"] is True and d["tag_extended"] is True and d["tag_variants"] is True and d["tag_classes"] is True
    assert d["tags"] == ["think", "step\\d+"]
    off = dict(cfg, runtime={k: v for k, v in KEYS.items() if k != "native_repeat_tags"})
    with pytest.raises(NativeUnsupported) as e:
        native_config(off, "127.0.0.1", 1, "cpu", 0, 1)
    assert str(e.value) == "thinking_tags ['think', 'step\\\\d+'] need regex semantics: run with --impl python"


def test_native_server_repeat_tags_match_python():
    import test_native_server as T

    T._compare(repeat_server_scenario(), "repeat_tags", None)
