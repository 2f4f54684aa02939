"""GPU: extended thinking tags (``\\d``, ``\\w``, ``\\s``, counted repetition; ``extended=True``,
``runtime.native_extended_tags``) on the HIP engine.

A shorthand is a class element and a counted repetition expands into rows, so such a set runs on
the class kernels (``qmx_ctick_kernel`` / a ``HipGrid(classes=True)``).  A shorthand's class
accepts some code points >= 0x80, and which ones only the host's tables say: such a byte at a
shorthand position makes the candidate suspect — for a set with a variable-width tag too, where
a class without a shorthand takes it as a mismatch — and the stream goes to the host path.
Every case asserts HIP == the C++ CPU engine == the python oracle, byte for byte.
"""
import json
import random

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.engine import FinalizeRequest
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import extended_tag_cases as X

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)
D3 = X.D3


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


# ---------------------------------------------------------------- 1: clean ASCII streams
@pytest.mark.parametrize("kfast", [None, "15", "0"])
def test_clean_streams_stay_on_the_gpu(kfast, monkeypatch):
    """Streams of every row of step\\d, t\\d?, h[1-6]{1,2}, sec\\d{1,3} in mixed case, near misses
    and partial tags, chunks of 3, 17 and 64 bytes, 2 seeds: nothing escalated, every finalize on
    the GPU.  The '>' of a plain "<t>" lies on the \\d of the row ``t\\d``: a mismatch, not a suspect."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    tags = X.CLEAN_SET
    assert native.tagset_kind(tags, **X.KW) == "class"
    hip = _hip(tags)
    plain_t = 0
    for chunk in (3, 17, 64):
        for seed in range(2):
            rng = random.Random(10 * chunk + seed)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 8 if chunk == 3 else 25))) for _ in range(4)]
            for r in raw:
                assert _suspects(tags, [r]) == 0, (chunk, seed, r)  # the generator's own condition
            plain_t += sum(_content(r).lower().count("<t>") + _content(r).lower().count("</t>") for r in raw)
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts))
    assert plain_t >= 20, plain_t
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 2: a non-ASCII digit at a shorthand position
def test_non_ascii_digit_goes_to_the_host():
    """4 streams with <step٣>...</step٣> and <t٣> beside 4 clean ones: the streams the host
    mirror flags are the escalated ones, exactly, and every output is the oracle's."""
    tags = X.CLEAN_SET
    rng = random.Random(21)
    dirty = [["a <step%s>hid" % D3, "den</step%s> b" % D3, " tail"], ["<STEP%s>x</step%s>" % (D3, D3), "y <t%s> z" % D3],
             ["p <t%s>q" % D3, "</t%s>r" % D3, "<step1>s</step1>"], ["<t>in<step%s>n</step%s>er</t>" % (D3, D3), " out"]]
    raw = [_events(rng, d) for d in dirty] + [_stream(rng, X.clean_pieces(rng, 20)) for _ in range(4)]
    flagged = _suspects(tags, raw)
    assert flagged == 4 and _suspects(tags, raw[4:]) == 0
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    _three_way(tags, hip, streams, lambda: random.Random(2))
    st = _stats(hip)
    assert st["class_escalations"] == flagged and st["escalations"] == flagged, st


# ---------------------------------------------------------------- 3: holdback at a tile end
@pytest.mark.parametrize("depth", [1, 0])
def test_holdback_at_a_tile_end(depth):
    """"<step٣>" cut after "<step", inside ٣ (a cut of the event's bytes: the event is whole a tick
    later) and after ٣, inside and outside a block, and "<step1>" cut after "<step" beside them.
    The oracle's bytes; the streams that leave the GPU are the ones the host mirror flags — a
    byte >= 0x80 at the shorthand's position, wherever the tile ended."""
    tags = ["step\\d", "t\\d?"]
    pre = ["<t>"] if depth else []
    tail = ["x</step%s>y" % D3, "</t>z" if depth else "z"]

    def ev(t):
        return b"data: " + json.dumps({"choices": [{"index": 0, "delta": {"content": t}}]}, ensure_ascii=False).encode() + b"\n\n"

    head = b"".join(ev(t) for t in pre)
    rest = b"".join(ev(t) for t in tail) + b"data: [DONE]\n\n"
    whole = ev("a<step%s>" % D3)
    k = whole.index(D3.encode())
    streams = [
        [head + ev("a<step"), ev(D3 + ">") + rest],                      # after "<step"
        [head + whole[:k + 1], whole[k + 1:] + rest],                    # after 1 byte of ٣
        [head + ev("a<step" + D3), ev(">") + rest],                      # after the whole ٣
        [head + ev("a<step"), ev("1>") + ev("x</step1>y") + b"".join(ev(t) for t in tail[1:]) + b"data: [DONE]\n\n"],
    ]
    raw = [b"".join(s) for s in streams]
    flagged = _suspects(tags, raw)
    assert flagged == 3 and _suspects(tags, raw[3:]) == 0
    hip = _hip(tags)
    _three_way(tags, hip, streams, H.EveryRound)
    st = _stats(hip)
    assert st["class_escalations"] == flagged and st["escalations"] == flagged, st


# ---------------------------------------------------------------- 4: window edge
def test_counted_class_on_the_window_edge():
    """``abcdefghijklmn\\d{1,2}``: rows of 16 and 15 elements, the digits on bytes 15/16 of the
    matcher's 16-byte window.  Both forms, near misses and the close forms, whose tail compare
    lies past the window."""
    tags = [X.EDGE_TAG]
    assert native.tagset_rows(tags, **X.KW) == [("abcdefghijklmn\\d\\d", 0), ("abcdefghijklmn\\d", 0)]
    # (one capture per row, so every close of a row is the close of every open of it: the
    # unfiltered runs' finalizes stay on the GPU too)
    forms = ["<abcdefghijklmn42>", "</ABCDEFGHIJKLMN42>", "<abcdefghijklmn7>", "</abcdefghijklmn7>", "<ABCDEFGHIJKLMN42>"]
    near = ["<abcdefghijklmn>", "<abcdefghijklmnx>", "<abcdefghijklmn123>", "</abcdefghijklmn4x>", "</abcdefghijklmn>",
            "<abcdefghijklmn4", "<ABCDEFGHIJKLMN42>x</abcdefghijklmn4>y</ABCDEFGHIJKLMN42>", "<abcdefghijklmn\\d{1,2}>",
            "</abcdefghijklmm42>"]
    hip = _hip(tags)
    for chunk in (17, 400):
        for seed in range(2):
            rng = random.Random(77 * chunk + seed)
            pieces = [rng.choice(forms) if rng.random() < 0.5 else rng.choice(near) if rng.random() < 0.6
                      else X.C.plain_run(rng, 1, 9) for _ in range(rng.randint(4, 25))]
            raw = [_stream(rng, pieces) for _ in range(3)]
            assert _suspects(tags, raw) == 0
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts))
            _three_way(tags, hip, streams, lambda: random.Random(ts), filt=False)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- 5: finalize
@pytest.mark.parametrize("tags,stem", [(["step\\d"], "step"), (["t[0-9]"], "t")])
def test_finalize_on_the_gpu_and_on_the_host(tags, stem):
    """<step1>a</step2>b</step1>c: the first close of the row is not the open's captured text, the
    finalize of a class set made with the key on goes on to the row's next close — "c", on the GPU.
    That holds for every class set made with the key on, a plain ``t[0-9]`` too (with the key off
    such a finalize goes to the host: tests/test_gpu_class_tags.py).
    <step٣>a</step٣>b has a byte >= 0x80 at the class position: finalized on the host."""
    hip, cpu = _hip(tags), _cpu(tags)
    rng = random.Random(4)
    texts = ["<%s1>a</%s2>b</%s1>c" % (stem, stem, stem), "<%s%s>a</%s%s>b" % (stem, D3, stem, D3)]
    res = {}
    for name, eng in (("hip", hip), ("cpu", cpu)):
        slots = [eng.open(i, False, True) for i in range(2)]
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
    from quorum_amd.ops import reference as ref
    oracle = [[ref.strip_thinking_tags(t, tags)] for t in texts]
    assert oracle == [["c"], ["b"] if stem == "step" else [texts[1]]]  # (٣ is a \d, not a [0-9])
    assert [o[0] for o in res["hip"]] == [o[0] for o in res["cpu"]] == oracle
    (_, b0, a0), (_, b1, a1) = res["hip"]
    assert a0["class_fin_host"] == b0["class_fin_host"] == 0 and a0["fin_host"] == b0["fin_host"], (b0, a0)
    assert a0["fin_items"] == b0["fin_items"] + 1, (b0, a0)
    assert a1["class_fin_host"] == 1 and a1["fin_host"] == b1["fin_host"] + 1, (b1, a1)


# ---------------------------------------------------------------- 6: class grid
def test_class_grid(ext):
    """One engine posts its ticks into a class grid made for the set with ``extended=True``:
    equal outputs, nothing escalated, ``grid_classes`` 1."""
    tags = X.CLEAN_SET
    grid = native.make_grid(tags, 0, 2, 4, **X.KW)
    try:
        assert grid.stats()["grid_classes"] == 1
        eng = _hip(tags, grid=grid, door=0)
        for chunk in (17, 400):  # two runs of ticks
            rng = random.Random(chunk)
            raw = [_stream(rng, X.clean_pieces(rng, rng.randint(1, 25))) for _ in range(4)]
            assert _suspects(tags, raw) == 0
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, eng, streams, lambda: random.Random(ts))
        st = _stats(eng)
        _assert_all_on_gpu(st)
        assert st["grid_ticks"] >= 2, st
        st = grid.stats()
        assert st["grid_classes"] == 1 and st["grid_launches"] >= 1, st
    finally:
        grid.stop()


# ---------------------------------------------------------------- server
def test_native_server_hip_extended_tags(ext, monkeypatch):
    """The native server on the HIP engine with ("think", "step\\d{1,2}") and the three keys on:
    loop ticks on a class grid (/metrics: qmx_grid_classes 1), the response equal to the python
    implementation's, every stream and final equal to the shadow CPU oracle."""
    import httpx
    import test_extended_tags as TX
    import test_native_server as T
    from live_upstream import native_server

    scn = TX.extended_server_scenario()
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "extended_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
    with native_server(scn[0], engine="hip") as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    assert len(lines) == 1 and lines[0].startswith("qmx_grid_classes 1"), lines
