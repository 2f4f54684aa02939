"""GPU: unbounded repetition in thinking tags (``+``, ``*``, ``{m,}`` after one element;
``repeat=True``, ``runtime.native_repeat_tags``) on the HIP engine.

Such a quantifier expands into rows, 4 beyond its minimum count (``kRepeatRows``), so the set runs
on the class kernels and a run within the rows is decided there.  The longest row is open-ended:
where its copies have matched and the next byte is one more of the repeated class, the token's
length is not the row's — the candidate is suspect (``class_candidate`` / ``mixed_candidate``), the
holdback's prefix walk sends the tile to the host (``kWalkHost``), and the exact host walk decides
the stream.  Every case asserts HIP == the C++ CPU engine == the python oracle, byte for byte.
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

KW = dict(max_slots=64, content_cap=1 << 16)
TAGS = X.GPU_TAGS


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _hip(tags, kw=X.KW, **more):
    return NativeEngine("hip", tags, device=0, **dict(KW, **kw, **more))


def _cpu(tags, kw=X.KW):
    return NativeEngine("cpu", tags, **kw)


def _stats(eng):
    return dict(eng._e.kernel_stats())


def _content(raw: bytes) -> str:
    return "".join(json.loads(ev[6:])["choices"][0]["delta"]["content"]
                   for ev in raw.decode().split("\n\n") if ev.startswith("data: {"))


def _suspects(tags, raw, kw=X.KW) -> int:
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


def _three_way(tags, hip, streams, rng_of, filt=True, kw=X.KW):
    n = len(streams)
    want = H.run_engine(H.python_engine(tags), streams, [filt] * n, [True] * n, rng_of())
    assert H.run_engine(_cpu(tags, kw), streams, [filt] * n, [True] * n, rng_of()) == want, tags
    got = H.run_engine(hip, streams, [filt] * n, [True] * n, rng_of())
    assert got == want, tags
    return got


def _assert_all_on_gpu(st):
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0 and st["fin_items"] >= 2, st


def _clean_runs(tags, hip, stem, kw=X.KW, chunks=(3, 17, 64)):
    for chunk in chunks:
        for seed in range(2):
            rng = random.Random(10 * chunk + seed)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 8 if chunk == 3 else 25), stem)) for _ in range(4)]
            assert _suspects(tags, raw, kw) == 0, (chunk, seed)  # the generator's own condition
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts), kw=kw)


def _dirty_runs(tags, hip, stem, kw=X.KW):
    """4 of 8 streams hold a run of five digits, in an open, a close, a nested block and cut over
    two events: exactly those leave the GPU."""
    rng = random.Random(21)
    s = stem
    dirty = [["a <%s12345>hid" % s, "den</%s12345> b" % s, " tail"], ["<%s1>x</%s12345>y</%s1> z" % (s, s, s)],
             ["p <think>q<%s123" % s, "45>r</%s12345>s</think>t" % s], ["<%s98765>" % s.upper(), "u</%s98765> v<%s7>" % (s, s)]]
    raw = [_events(rng, d) for d in dirty] + [_stream(rng, X.clean_pieces(rng, 20, stem)) for _ in range(4)]
    flagged = _suspects(tags, raw, kw)
    assert flagged == 4 and _suspects(tags, raw[4:], kw) == 0
    streams = [H.split_random(rng, r, 64) for r in raw]
    _three_way(tags, hip, streams, lambda: random.Random(2), kw=kw)
    st = _stats(hip)
    assert st["class_escalations"] == flagged and st["escalations"] == flagged, st


# ---------------------------------------------------------------- 1: runs within the rows
@pytest.mark.parametrize("kfast", [None, "15", "0"])
def test_clean_streams_stay_on_the_gpu(kfast, monkeypatch):
    """Streams of think and step\\d+ with runs of 1 to 4 digits — opens, closes, nested, in any
    ASCII case, near misses and partial tags — in chunks of 3, 17 and 64 bytes, 2 seeds: the rows
    decide every one of them, nothing is escalated and every finalize is on the GPU."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    assert native.tagset_kind(TAGS, **X.KW) == "class"
    hip = _hip(TAGS)
    _clean_runs(TAGS, hip, "step")
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 2: a run longer than the rows
def test_five_digits_go_to_the_host():
    _dirty_runs(TAGS, _hip(TAGS), "step")


# ---------------------------------------------------------------- 3: holdback at a tile end
@pytest.mark.parametrize("depth", [1, 0])
def test_holdback_at_a_tile_end(depth):
    """A tile ends after "<step12" (held inside a block; the next tile's '>' makes it a tag, on the
    GPU), after "<step1234" with '>' next (the same, at the open-ended row's last copy), after
    "<step1234" with '5' next (held, then suspect: the host) and after "</step12".  Outside a
    block the instance is released, as the reference's source-text holdback does.  The oracle's
    bytes; the streams that leave the GPU are the ones the host mirror flags."""
    pre = ["<think>"] if depth else []
    head = b"".join(_ev(t) for t in pre)
    end = _ev("</think>z" if depth else "z") + b"data: [DONE]\n\n"
    streams = [
        [head + _ev("a<step12"), _ev(">x</step12>y") + end],
        [head + _ev("a<step1234"), _ev(">x</step1234>y") + end],
        [head + _ev("a<step1234"), _ev("5>x</step12345>y") + end],
        [head + _ev("a<step12>x</step12"), _ev(">y") + end],
    ]
    raw = [b"".join(s) for s in streams]
    assert [_suspects(TAGS, [r]) for r in raw] == [0, 0, 1, 0]
    hip = _hip(TAGS)
    _three_way(TAGS, hip, streams, H.EveryRound)
    st = _stats(hip)
    assert st["class_escalations"] == 1 and st["escalations"] == 1, st


# ---------------------------------------------------------------- 4: window edge
def test_run_on_the_window_edge():
    """``abcdefghijklm\\d+``: with "<" the stem fills 14 bytes of the matcher's 16-byte window, so
    runs of 1 to 4 digits and their '>' straddle its end, and the closes' lie past it.  Every form,
    near misses and partial tags, filtered and unfiltered."""
    stem = "abcdefghijklm"
    tags = [stem + "\\d+"]
    assert [r for r, _ in native.tagset_rows(tags, **X.KW)] == [stem + "\\d" * 4 + "+", stem + "\\d" * 3, stem + "\\d" * 2, stem + "\\d"]
    # (one capture per row, so every close of a row is the close of every open of it: the
    # unfiltered runs' finalizes stay on the GPU too)
    runs = ["7", "42", "123", "1234"]
    forms = [b + (stem.upper() if up else stem) + r + ">" for r in runs for b in ("<", "</") for up in (False, True)]
    near = ["<%s>" % stem, "<%sx>" % stem, "</%s4x>" % stem, "</%s>" % stem, "<%s4" % stem, "<%s123" % stem,
            "<%s1234>x</%s123>y</%s1234>" % (stem.upper(), stem, stem), "<%s\\d+>" % stem, "</abcdefghijkmm42>", "<%s12 34>" % stem]
    plain = lambda rng: "".join(rng.choice("abxyz. \n") for _ in range(rng.randint(1, 9)))  # noqa: E731
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
            _three_way(tags, hip, streams, lambda: random.Random(ts), filt=False)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 5: finalize
def test_finalize_on_the_gpu_and_on_the_host():
    """<step12>a</step1>b</step12>c: the close of another row is passed over — "c", on the GPU;
    <STEP7>x</step7> strips on the GPU; <step12345>x</step12345>y has a run longer than the rows:
    finalized on the host."""
    hip, cpu = _hip(TAGS), _cpu(TAGS)
    rng = random.Random(4)
    texts = ["<step12>a</step1>b</step12>c", "<STEP7>x</step7>", "<step12345>x</step12345>y"]
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
    assert oracle == [["c"], [""], ["y"]]
    assert [o[0] for o in res["hip"]] == [o[0] for o in res["cpu"]] == oracle
    (_, b0, a0), (_, b1, a1), (_, b2, a2) = res["hip"]
    for b, a in ((b0, a0), (b1, a1)):
        assert a["class_fin_host"] == b["class_fin_host"] == 0 and a["fin_host"] == b["fin_host"], (b, a)
        assert a["fin_items"] == b["fin_items"] + 1, (b, a)
    assert a2["class_fin_host"] == 1 and a2["fin_host"] == b2["fin_host"] + 1, (b2, a2)


# ---------------------------------------------------------------- 6: '*' with no copy
def test_star_with_zero_copies():
    """think\\s*: "<think>" (the row without a copy: the '>' lies on the \\s of the longer rows, a
    mismatch of those, not a suspect) and "<think >" are decided on the GPU; five spaces are a
    run longer than the rows and go to the host."""
    tags = ["think\\s*"]
    rng = random.Random(6)
    on_gpu = [["a<think>x", "</think>b <THINK>c</think >d</think>e"], ["a<think >x</think >b", "<think  \n >y</THINK  \n >z"]]
    host = [["a<think     >x</think     >b"]]
    hip = _hip(tags)
    raw = [_events(rng, d) for d in on_gpu]
    assert _suspects(tags, raw) == 0
    _three_way(tags, hip, [H.split_random(rng, r, 64) for r in raw], lambda: random.Random(3))
    _assert_all_on_gpu(_stats(hip))
    raw = [_events(rng, d) for d in host]
    assert _suspects(tags, raw) == 1
    _three_way(tags, hip, [H.split_random(rng, r, 64) for r in raw], lambda: random.Random(3))
    st = _stats(hip)
    assert st["class_escalations"] == 1 and st["escalations"] == 1, st


# ---------------------------------------------------------------- 7: mixed
def test_mixed_set_clean_and_dirty():
    """思\\d+ (a mixed tag set: ``mixed_candidate`` / ``mixed_walk``) behaves as step\\d+ does: runs of
    1 to 4 digits stay on the GPU, five digits go to the host."""
    tags = ["think", "思\\d+"]
    assert native.tagset_kind(tags, **X.MIXED_KW) == "mixed"
    hip = _hip(tags, X.MIXED_KW)
    _clean_runs(tags, hip, "思", X.MIXED_KW, chunks=(17, 64))
    _assert_all_on_gpu(_stats(hip))
    _dirty_runs(tags, _hip(tags, X.MIXED_KW), "思", X.MIXED_KW)


# ---------------------------------------------------------------- 8: class grid
def test_class_grid(ext):
    """One engine posts its ticks and fused finalizes into a door of a class grid made for the set
    with ``repeat=True``: equal outputs, nothing escalated, ``grid_classes`` 1."""
    grid = native.make_grid(TAGS, 0, 2, 4, **X.KW)
    try:
        assert grid.stats()["grid_classes"] == 1
        eng = _hip(TAGS, grid=grid, door=0)
        for chunk in (17, 400):  # two runs of ticks
            rng = random.Random(chunk)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 25))) for _ in range(4)]
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


# ---------------------------------------------------------------- 9: server
def test_native_server_hip_repeat_tags(ext, monkeypatch):
    """The native server on the HIP engine with ("think", "step\\d+") and the four keys on: loop
    ticks on a class grid (/metrics: qmx_grid_classes 1), the response equal to the python
    implementation's, every stream and final equal to the shadow CPU oracle."""
    import httpx
    import test_native_server as T
    import test_repeat_tags as TR
    from live_upstream import native_server

    scn = TR.repeat_server_scenario()
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "repeat_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
    with native_server(scn[0], engine="hip") as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    assert len(lines) == 1 and lines[0].startswith("qmx_grid_classes 1"), lines
