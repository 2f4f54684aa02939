"""GPU: runs of any length in repeated thinking tags (``runs=True``, ``runtime.native_run_tags``) on the
HIP engine.

With the key the class kernels take a run of ASCII copies past an open-ended row themselves: the
candidate walk has a cursor of its own, a token's byte length is kept per candidate in LDS, and the
finalize compares a close with the text its open captured over the open's own length.  Such a stream
stays on the GPU; a non-ASCII byte in a run, or a '<' / '>' the repeated class accepts, still moves it
to the host path.  Every case asserts HIP == the C++ CPU engine == the python oracle, byte for byte;
every "stays on the GPU" case first asserts, through the kernels' rule on the host
(``class_suspects(..., runs=True)``), that its input has no suspect candidate.
"""
import json
import random

import pytest

from quorum_amd.ops import native, reference as ref
from quorum_amd.ops.engine import FinalizeRequest
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import repeat_tag_cases as X

pytestmark = pytest.mark.gpu

ENG = dict(max_slots=64, content_cap=1 << 16)
KW = dict(X.KW, runs=True)
MIXED_KW = dict(X.MIXED_KW, runs=True)
TAGS = X.GPU_TAGS


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _hip(tags, kw=KW, **more):
    return NativeEngine("hip", tags, device=0, **dict(ENG, **kw, **more))


def _cpu(tags, kw=KW):
    return NativeEngine("cpu", tags, **kw)


def _stats(eng):
    return dict(eng._e.kernel_stats())


def _content(raw: bytes) -> str:
    return "".join(json.loads(ev[6:])["choices"][0]["delta"]["content"]
                   for ev in raw.decode().split("\n\n") if ev.startswith("data: {"))


def _suspects(tags, raw, kw=KW) -> int:
    """Streams of `raw` with a suspect candidate: the kernels' rule on the host, over the whole
    content, streaming and strip tables."""
    kw = {k: v for k, v in kw.items() if k != "classes"}
    return sum((native.class_suspects(tags, _content(r).encode(), **kw) +
                native.class_suspects(tags, _content(r).encode(), strip=True, **kw)) > 0 for r in raw)


def _stream(rng, pieces, per_event=3):
    parts, i = [], 0
    while i < len(pieces):
        k = rng.randint(1, per_event)
        parts.append(H.event_bytes(rng, "".join(pieces[i:i + k])))
        i += k
    return b"".join(parts) + b"data: [DONE]\n\n"


def _events(rng, texts):
    return b"".join(H.event_bytes(rng, t) for t in texts) + b"data: [DONE]\n\n"


def _ev(t):
    return b"data: " + json.dumps({"choices": [{"index": 0, "delta": {"content": t}}]}, ensure_ascii=False).encode() + b"\n\n"


def _three_way(tags, hip, streams, rng_of, filt=True, kw=KW, oracle=True):
    n = len(streams)
    want = H.run_engine(_cpu(tags, kw), streams, [filt] * n, [True] * n, rng_of())
    if oracle:
        assert H.run_engine(H.python_engine(tags), streams, [filt] * n, [True] * n, rng_of()) == want, tags
    got = H.run_engine(hip, streams, [filt] * n, [True] * n, rng_of())
    assert got == want, tags
    return got


def _assert_all_on_gpu(st):
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0 and st["fin_items"] >= 2, st


def _clean_runs(tags, hip, stem, kw=KW, chunks=(3, 17, 64)):
    for chunk in chunks:
        for seed in range(2):
            rng = random.Random(10 * chunk + seed)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 8 if chunk == 3 else 25), stem, max_digits=12)) for _ in range(4)]
            assert _suspects(tags, raw, kw) == 0, (chunk, seed)  # the generator's own condition
            assert _suspects(tags, raw, {k: v for k, v in kw.items() if k != "runs"}) > 0  # (without the key they leave the GPU)
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts), kw=kw)


def _dirty_runs(tags, hip, stem, kw=KW):
    """The four streams of tests/test_gpu_repeat_tags.py::_dirty_runs — a run of five digits in an open,
    a close, a nested block and cut over two events — stay on the GPU; a fifth with a non-ASCII digit
    in its run is the one that leaves it."""
    rng = random.Random(21)
    s = stem
    dirty = [["a <%s12345>hid" % s, "den</%s12345> b" % s, " tail"], ["<%s1>x</%s12345>y</%s1> z" % (s, s, s)],
             ["p <think>q<%s123" % s, "45>r</%s12345>s</think>t" % s], ["<%s98765>" % s.upper(), "u</%s98765> v<%s7>" % (s, s)]]
    wide = [["a <%s12%s45>hid" % (s, X.D3), "den</%s12%s45> b" % (s, X.D3)]]
    raw = [_events(rng, d) for d in dirty + wide] + [_stream(rng, X.clean_pieces(rng, 20, stem, max_digits=12)) for _ in range(3)]
    assert _suspects(tags, raw[:4], kw) == 0 and _suspects(tags, raw[4:5], kw) == 1 and _suspects(tags, raw[5:], kw) == 0
    streams = [H.split_random(rng, r, 64) for r in raw]
    _three_way(tags, hip, streams, lambda: random.Random(2), kw=kw)
    st = _stats(hip)
    assert st["class_escalations"] == 1 and st["escalations"] == 1, st


# ---------------------------------------------------------------- 1: clean streams with long runs
@pytest.mark.parametrize("kfast", [None, "15", "0"])
def test_clean_streams_with_long_runs_stay_on_the_gpu(kfast, monkeypatch):
    """Streams of think and step\\d+ with runs of 1 to 12 digits — opens, closes, nested, in any ASCII
    case, near misses and partial tags — in chunks of 3, 17 and 64 bytes, 2 seeds: nothing is
    escalated and every finalize is on the GPU."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    assert native.tagset_kind(TAGS, **KW) == "class"
    hip = _hip(TAGS)
    _clean_runs(TAGS, hip, "step")
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 2: the streams that left the GPU
def test_five_digits_stay_on_the_gpu():
    _dirty_runs(TAGS, _hip(TAGS), "step")


# ---------------------------------------------------------------- 3: holdback at a tile end
@pytest.mark.parametrize("depth", [1, 0])
def test_holdback_at_a_tile_end(depth):
    """A tile ends inside a run longer than the rows: after "<step12345" (the next tile brings ">",
    "6>" or "x"), after "</step12345", and "<step" + 57 digits cut after 1, 5, 33, 62 and 63 bytes of
    the tag.  Inside a block the tail is held and the next tile decides the tag; outside one the
    instance is released, as the reference's source-text holdback does.  Nothing is escalated and the
    bytes are the oracle's."""
    pre = ["<think>"] if depth else []
    head = b"".join(_ev(t) for t in pre)
    end = _ev("</think>z" if depth else "z") + b"data: [DONE]\n\n"
    long_tag = "<step" + "7" * 57 + ">"
    assert len(long_tag) == 63
    streams = [
        [head + _ev("a<step12345"), _ev(">x</step12345>y") + end],
        [head + _ev("a<step12345"), _ev("6>x</step123456>y") + end],
        [head + _ev("a<step12345"), _ev("x>y") + end],
        [head + _ev("a<step12345>x</step12345"), _ev(">y") + end],
    ] + [[head + _ev("a" + long_tag[:k]), _ev(long_tag[k:] + "x</step" + "7" * 57 + ">y") + end] for k in (1, 5, 33, 62, 63)]
    raw = [b"".join(s) for s in streams]
    assert _suspects(TAGS, raw) == 0
    hip = _hip(TAGS)
    _three_way(TAGS, hip, streams, H.EveryRound)
    st = _stats(hip)
    assert st["class_escalations"] == 0 and st["escalations"] == 0, st
    # one digit more is text natively and a tag in `re` (the documented difference): decided on the GPU,
    # equal to the CPU engine
    over = "<step" + "7" * 58 + ">"
    streams = [[head + _ev("a" + over[:k]), _ev(over[k:] + "x</step" + "7" * 58 + ">y") + end] for k in (5, 33, 63, 64)]
    assert _suspects(TAGS, [b"".join(s) for s in streams]) == 0
    _three_way(TAGS, hip, streams, H.EveryRound, oracle=False)
    st = _stats(hip)
    assert st["class_escalations"] == 0 and st["escalations"] == 0, st


# ---------------------------------------------------------------- 4: window edge
def test_long_run_on_the_window_edge():
    """``abcdefghijklm\\d+``: with "<" the stem fills 14 bytes of the matcher's 16-byte window, so runs
    of 5 to 12 digits straddle its end and lie past it.  Opens and closes in both cases, near misses
    and partial tags, filtered and unfiltered."""
    stem = "abcdefghijklm"
    tags = [stem + "\\d+"]
    runs = ["12345", "123456", "7654321", "12345678", "123456789", "1234567890", "12345678901", "123456789012"]
    forms = [b + (stem.upper() if up else stem) + r + ">" for r in runs for b in ("<", "</") for up in (False, True)]
    near = ["<%s>" % stem, "<%s12345x>" % stem, "</%s123456x>" % stem, "</%s>" % stem, "<%s12345" % stem, "<%s1234567" % stem,
            "<%s\\d+>" % stem, "</abcdefghijkmm123456>", "<%s12345 6>" % stem]
    plain = lambda rng: "".join(rng.choice("abxyz. \n") for _ in range(rng.randint(1, 9)))  # noqa: E731
    # (unfiltered, the whole text reaches the finalize, whose captures are as long as their runs: there
    # every open is followed by its own close, in either case, so no open is left pending for the host)
    blocks = ["<%s>%s</%s>" % (a + r, body, b + r) for r in runs for a in (stem, stem.upper()) for b in (stem, stem.upper())
              for body in ("x", "</%s%s0>" % (stem, r), "</%s>" % (stem + r[:-1]))]
    hip = _hip(tags)
    for chunk in (17, 400):
        for seed in range(2):
            rng = random.Random(77 * chunk + seed)
            pieces = [rng.choice(forms) if rng.random() < 0.5 else rng.choice(near) if rng.random() < 0.6
                      else plain(rng) for _ in range(rng.randint(4, 25))]
            raw = [_stream(rng, pieces) for _ in range(3)]
            assert _suspects(tags, raw) == 0
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts))
            pieces = [rng.choice(blocks) if rng.random() < 0.5 else rng.choice(near) if rng.random() < 0.6
                      else plain(rng) for _ in range(rng.randint(4, 25))]
            raw = [_stream(rng, pieces) for _ in range(3)]
            assert _suspects(tags, raw) == 0
            streams = [H.split_random(rng, r, chunk) for r in raw]
            _three_way(tags, hip, streams, lambda: random.Random(ts), filt=False)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 5: two open-ended positions
@pytest.mark.parametrize("tags,texts", [
    (["v\\d+\\.\\d+"], ["a<v12345.678901>hid</v12345.678901>b", "<V1.23456>x</v1.23456>y <v12345.>k <v12345x6>l</v12345.678901>",
                        "<think>", "p<v123456.7>q<v1.2>r</v1.2>s</V123456.7>t"]),
    (["a\\d+[a-z]+"], ["a<A123456ABCDEFG>hid</a123456abcdefg>b", "<a1b>x</a1b>y <a123456>k <a12345b6>l", "<a12345bcdefgh>m</a12345bcdefg>n</A12345BCDEFGH>o"]),
])
def test_two_open_ended_positions(tags, texts):
    rng = random.Random(5)
    raw = [_events(rng, [t[:len(t) // 2], t[len(t) // 2:]]) for t in texts]
    assert _suspects(tags, raw) == 0
    hip = _hip(tags)
    for chunk in (17, 64):
        _three_way(tags, hip, [H.split_random(rng, r, chunk) for r in raw], lambda: random.Random(3))
        _three_way(tags, hip, [H.split_random(rng, r, chunk) for r in raw], lambda: random.Random(3), filt=False)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 6: whitespace and accepted delimiters
def test_whitespace_runs_and_accepted_delimiters():
    """think\\s* with 5 to 9 spaces, a newline among them, stays on the GPU.  n[^0-9x]+x: "<nabcdefx>"
    stays on the GPU, "<nab<cdx>" — a '<' the repeated class accepts, inside the run — moves exactly
    that stream to the host."""
    rng = random.Random(6)
    tags = ["think\\s*"]
    texts = [["a<think     >x", "</think     >b"], ["<THINK   \n  >c</think   \n  >d", "</think>e"], ["a<think \n       >x</think>y</think \n       >b"],
             ["<think>p<think      >q</think      >r</think>s"]]
    raw = [_events(rng, d) for d in texts]
    assert _suspects(tags, raw) == 0
    hip = _hip(tags)
    _three_way(tags, hip, [H.split_random(rng, r, 64) for r in raw], lambda: random.Random(3))
    _assert_all_on_gpu(_stats(hip))
    tags = ["n[^0-9x]+x"]
    hip = _hip(tags)
    raw = [_events(rng, ["a<nabcdefx>hid", "den</nabcdefx>b <NABCDEFX>c</nabcdefx>d"])]
    assert _suspects(tags, raw) == 0
    _three_way(tags, hip, [H.split_random(rng, r, 64) for r in raw], lambda: random.Random(3))
    _assert_all_on_gpu(_stats(hip))
    raw += [_events(rng, ["a<nab<cdx>hid", "den</nab<cdx>b"])]
    assert _suspects(tags, raw) == 1
    _three_way(tags, hip, [H.split_random(rng, r, 64) for r in raw], lambda: random.Random(3))
    st = _stats(hip)
    assert st["class_escalations"] == 1 and st["escalations"] == 1, st


# ---------------------------------------------------------------- 7: more than 64 candidates in a tile
def test_more_than_64_candidates_in_one_tile():
    """70 tags <stepN> / </stepN> with runs of 5 to 12 digits in one event: the tile has more than 64
    candidates, so the tokens are compacted four candidates per thread (the second branch)."""
    rng = random.Random(7)
    names = ["step" + "".join(rng.choice("0123456789") for _ in range(5 + i % 8)) for i in range(35)]
    text = "".join("<%s>h%d</%s>k%d " % (n.upper() if i % 3 == 0 else n, i, n, i) for i, n in enumerate(names))
    assert text.count("<") == 70
    # (the second stream cuts a 71st tag over two events inside a block, where the tail is held; outside a
    # block an open tag cut by an event boundary is the host's, with or without the key)
    raw = [_ev("<think>" + text + "</think>tail") + _ev(text) + b"data: [DONE]\n\n",
           _ev("<think>" + text + "<step123456") + _ev(">x</step123456></think>y") + b"data: [DONE]\n\n"]
    assert _suspects(TAGS, raw) == 0
    hip = _hip(TAGS)
    for filt in (True, False):
        _three_way(TAGS, hip, [[r] for r in raw], lambda: random.Random(1), filt=filt)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 8: finalize
def test_finalize_compares_the_captured_run():
    """The close of an open with a run is the close with the same run: a shorter one, a different one
    of the same length and the close of another row are passed over, on the GPU.  An open whose own
    close never comes gives the oracle's bytes on either path."""
    hip, cpu = _hip(TAGS), _cpu(TAGS)
    rng = random.Random(4)
    texts = ["<step12345>x</step12345>y", "<step12345>a</step1234>b</step12345>c", "<step12345>a</step12346>b</step12345>c",
             "<STEP123456>x</step123456>", "<step12345>x", "<step12345>a</step1234>b"]
    want = ["y", "c", "c", "", "<step12345>x", None]
    kw = {k: v for k, v in KW.items() if k != "classes"}
    assert all(native.class_suspects(TAGS, t.encode(), strip=True, **kw) == 0 for t in texts)
    res = {}
    for name, eng in (("hip", hip), ("cpu", cpu)):
        slots = [eng.open(i, False, True) for i in range(len(texts))]
        for s, t in zip(slots, texts):
            eng.feed(s, H.event_bytes(rng, t) + b"data: [DONE]\n\n")
            eng.finish(s)
        for _ in range(20):
            if not eng.has_work():
                break
            eng.tick(H.CREATED)
        assert [eng.text(s) for s in slots] == texts
        fins, out = {}, []
        for slot in slots:
            before = _stats(hip) if name == "hip" else None
            fid = eng.submit_finalize(FinalizeRequest([slot], True, "texts"))
            for _ in range(10):
                if not eng.has_work():
                    break
                fins.update(dict(eng.tick(H.CREATED)[1]))
            out.append((fins[fid], before, _stats(hip) if name == "hip" else None))
        res[name] = out
    oracle = [[ref.strip_thinking_tags(t, TAGS)] for t in texts]
    assert [o[0] for o in oracle[:5]] == want[:5]
    assert [o[0] for o in res["hip"]] == [o[0] for o in res["cpu"]] == oracle
    for _, b, a in res["hip"][:5]:
        assert a["class_fin_host"] == b["class_fin_host"] == 0 and a["fin_host"] == b["fin_host"], (b, a)
        assert a["fin_items"] == b["fin_items"] + 1, (b, a)


# ---------------------------------------------------------------- 9: mixed
def test_mixed_set_long_runs():
    """思\\d+ (a mixed tag set: ``mixed_candidate`` / ``mixed_walk``) behaves as step\\d+ does."""
    tags = ["think", "思\\d+"]
    assert native.tagset_kind(tags, **MIXED_KW) == "mixed"
    hip = _hip(tags, MIXED_KW)
    _clean_runs(tags, hip, "思", MIXED_KW, chunks=(17, 64))
    _assert_all_on_gpu(_stats(hip))
    _dirty_runs(tags, _hip(tags, MIXED_KW), "思", MIXED_KW)


# ---------------------------------------------------------------- 10: class grid
def test_class_grid(ext):
    """One engine posts its ticks and fused finalizes into a door of a class grid made for the set
    with ``runs=True``: equal outputs, nothing escalated, ``grid_classes`` 1."""
    grid = native.make_grid(TAGS, 0, 2, 4, **KW)
    try:
        assert grid.stats()["grid_classes"] == 1
        eng = _hip(TAGS, grid=grid, door=0)
        for chunk in (17, 400):  # two runs of ticks
            rng = random.Random(chunk)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 25), max_digits=12)) for _ in range(4)]
            assert _suspects(TAGS, raw) == 0
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(TAGS, eng, streams, lambda: random.Random(ts))
        st = _stats(eng)
        _assert_all_on_gpu(st)
        assert st["grid_ticks"] >= 2, st
        st = grid.stats()
        assert st["grid_classes"] == 1 and st["grid_launches"] >= 1, st
    finally:
        grid.stop()


# ---------------------------------------------------------------- 11: server
def run_server_scenario(tags=("think", "step\\d+")):
    """One streamed session with runs of 5 to 8 digits in both cases: a tag split over events inside
    its run, a close of another run, a near miss, the source text, an unclosed open."""
    from conftest import cfg_parallel, sse_chunk

    import test_native_server as T

    s1 = [sse_chunk({"role": "assistant"}), sse_chunk({"content": "A <STEP12345>hid"}),
          sse_chunk({"content": "den</step12345> B <ste"}), sse_chunk({"content": "p123"}),
          sse_chunk({"content": "456>x</step12345>y</STEP123456> C <step"}),
          sse_chunk({"content": "7654321>gone</step7654321> <step12345x>k</step12345x> D <step\\d+> E"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    s2 = [sse_chunk({"content": "<think>t<step31415926>u</think>v</step31415926>F <Step123456>w</step123456> G<step45678"}),
          sse_chunk({}, finish="stop"), b"data: [DONE]\n\n"]
    cfg = cfg_parallel(2, block=dict(T.CONCAT, hide_final_think=True, thinking_tags=list(tags)))
    cfg["runtime"] = {"native_regex_tags": True, "native_variant_tags": True, "native_extended_tags": True,
                      "native_repeat_tags": True, "native_run_tags": True}
    return (cfg, {"b1.test": ("stream", 200, T.split7(s1)), "b2.test": ("stream", 200, s2)},
            {"messages": T.MSG, "stream": True}, T.AUTH)


def test_native_server_hip_run_tags(ext, monkeypatch):
    """The native server on the HIP engine with ("think", "step\\d+") and the five keys on: loop ticks on
    a class grid, the response equal to the python implementation's, every stream and final equal to
    the shadow CPU oracle."""
    import test_native_server as T

    scn = run_server_scenario()
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "run_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
