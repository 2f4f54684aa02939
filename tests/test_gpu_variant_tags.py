"""GPU: variable-width thinking tags ('?', '|', groups; ``variants=True``,
``runtime.native_variant_tags``) on the HIP engine.

A set with such a tag is of the class kind (``qmx_ctick_kernel`` / a ``HipGrid(classes=True)``):
every row — a fixed-width expansion of a tag — is one entry of the set, the byte matchers find
the rows without a class element, the shared walk the others, the first in list order wins.  The
suspect rule of such a set takes '<', '>' or a byte >= 0x80 at a class position that does not
accept it as a mismatch of that row (the '>' of a plain "<t>" on the class of the row ``t[0-9]``),
so only a byte a class accepts sends a stream to the host.  Every case asserts HIP == the C++
CPU engine == the python oracle, byte for byte (SSE, flags, content, finals).
"""
import json
import random

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import variant_tag_cases as V

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _hip(tags, kw=V.KW, **more):
    return NativeEngine("hip", tags, device=0, **dict(KW, **kw, **more))


def _cpu(tags, kw=V.KW):
    return NativeEngine("cpu", tags, **kw)


def _stats(eng):
    return dict(eng._e.kernel_stats())


def _assert_all_on_gpu(st, fin=True):
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0, st
    if fin:
        assert st["fin_items"] >= 2, st


def _content(raw: bytes) -> str:
    return "".join(json.loads(ev[6:])["choices"][0]["delta"]["content"]
                   for ev in raw.decode().split("\n\n") if ev.startswith("data: {"))


def _suspects(tags, raw, kw=V.KW) -> int:
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


def _three_way(tags, hip, streams, rng_of, filt=True, kw=V.KW):
    n = len(streams)
    want = H.run_engine(H.python_engine(tags), streams, [filt] * n, [True] * n, rng_of())
    assert H.run_engine(_cpu(tags, kw), streams, [filt] * n, [True] * n, rng_of()) == want, tags
    got = H.run_engine(hip, streams, [filt] * n, [True] * n, rng_of())
    assert got == want, tags
    return got


# ---------------------------------------------------------------- clean streams
@pytest.mark.parametrize("kfast", [None, "15", "0"])
@pytest.mark.parametrize("ti", range(len(V.CLEAN_SETS)))
def test_clean_streams_stay_on_the_gpu(ti, kfast, monkeypatch):
    """Clean streams of every row of every tag, in lower, upper and mixed case, near misses and
    partial tags, in chunks of 3, 17, 64 and 400 bytes, 4 seeds: nothing escalated, every
    finalize on the GPU.  The streams of ``t[0-9]?`` hold plain "<t>" and "</t>", whose '>' lies
    on the class position of the row ``t[0-9]``: the case the variant suspect rule exists for."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    tags = V.CLEAN_SETS[ti]
    assert native.tagset_kind(tags, **V.KW) == "class"
    hip = _hip(tags)
    plain_t = 0
    for chunk in (3, 17, 64, 400):
        for seed in range(4):
            rng = random.Random(10000 * ti + 10 * chunk + seed)
            raw = [_stream(rng, V.clean_pieces(rng, tags, rng.randint(1, 8 if chunk == 3 else 25))) for _ in range(4)]
            assert _suspects(tags, raw) == 0, (tags, chunk, seed)  # the generator's own condition
            plain_t += sum(_content(r).lower().count("<t>") + _content(r).lower().count("</t>") for r in raw)
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts))
    if ti == 1:
        assert plain_t >= 20, plain_t
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- window edge
def test_optional_element_on_the_window_edge():
    """``abcdefghijklmno?p``: the optional element sits on bytes 15/16 of the matcher's 16-byte
    window.  Both forms, near misses and the close forms, whose tail compare lies past the window."""
    tags = [V.EDGE_TAG]
    assert native.tagset_rows(tags, **V.KW) == [("abcdefghijklmnop", 0), ("abcdefghijklmnp", 0)]
    near = ["<abcdefghijklmnoq>", "<abcdefghijklmnq>", "<abcdefghijklmnoop>", "</abcdefghijklmno>", "<abcdefghijklmn>",
            "</abcdefghijklmnpp>", "<ABCDEFGHIJKLMNOP>x</abcdefghijklmnp>y</ABCDEFGHIJKLMNOP>", "<abcdefghijklmno?p>"]
    hip = _hip(tags)
    for chunk in (17, 400):
        for seed in range(3):
            rng = random.Random(77 * chunk + seed)
            raw = [_stream(rng, V.clean_pieces(rng, tags, rng.randint(4, 25), extra=near)) for _ in range(4)]
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            _three_way(tags, hip, streams, lambda: random.Random(ts))
            _three_way(tags, hip, streams, lambda: random.Random(ts), filt=False)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- dense tiles
@pytest.mark.parametrize("ti", range(len(V.CLEAN_SETS)))
def test_dense_tiles(ti):
    """5, 63, 64 and min(MAX_CAND, 200) '<' in one tile: across the step from the VALU pair
    matcher to the MFMA matcher, with rows that are prefixes of one another."""
    lim = native.require().kernel_limits()
    tags = V.CLEAN_SETS[ti]
    rows = V.all_rows(tags)
    rng = random.Random(ti)
    raw = []
    for k in (5, 63, 64, min(lim["MAX_CAND"], 200)):
        text = "".join(V.clean_form(rng, rows) + V.C.plain_run(rng, 0, 3) for _ in range(k))
        raw.append(H.event_bytes(rng, text) + b"data: [DONE]\n\n")
    assert all(len(r) <= lim["TILE_MAX"] for r in raw)
    assert _suspects(tags, raw) == 0
    hip = _hip(tags)
    _three_way(tags, hip, [[r] for r in raw], H.EveryRound)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- holdback
def _split_streams(text, pre):
    """One stream per split point of `text`: [pre,] text[:k], text[k:], "z" — an event each."""
    rng = random.Random(0)
    out = []
    for k in range(1, len(text)):
        evs = ([pre] if pre else []) + [text[:k], text[k:], "z"]
        out.append([H.event_bytes(rng, e) for e in evs] + [b"data: [DONE]\n\n"])
    return out


@pytest.mark.parametrize("same_tile", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("text,released", [("<think(ing)?>", 0), ("<thinking>", 3), ("<think>", 0), ("</thinking>", 0)])
def test_split_at_every_byte(text, released, depth, same_tile):
    """The source text, both opens and a close split at every byte, outside and inside a block,
    the parts in separate ticks and in one tile: the python oracle's output.  Outside a block
    the reference holds a prefix of the SOURCE text "<think(ing)?>": "<thinki", "<thinkin" and
    "<thinking" were released, so "<thinking>" cut there is no tag — with both parts in one
    tile those three streams are decided by the host path; "<think>" has no such cut."""
    tags = ["think(ing)?"]
    streams = _split_streams(text, "<think>" if depth else "")
    if same_tile:
        streams = [[b"".join(s)] for s in streams]
    hip = _hip(tags)
    for i in range(0, len(streams), 6):
        batch = streams[i:i + 6]
        n = len(batch)
        want = H.run_engine(H.python_engine(tags), batch, [True] * n, [True] * n, H.EveryRound())
        assert H.run_engine(_cpu(tags), batch, [True] * n, [True] * n, H.EveryRound()) == want, (text, depth, i)
        got = H.run_engine(hip, batch, [True] * n, [True] * n, H.EveryRound())
        assert got == want, (text, depth, i)
    st = _stats(hip)
    if same_tile and depth == 0:
        # (an escalated stream's content lives on the host: so does a finalize that reads it)
        assert st["class_escalations"] == released and st["escalations"] == released, st
    else:
        assert st["escalations"] == 0 and st["class_escalations"] == 0 and st["fin_host"] == 0, st
    assert st["class_fin_host"] == 0, st


# ---------------------------------------------------------------- ambiguous windows
@pytest.mark.parametrize("tags,texts", [(["a.?"], ["<a>x y", "<A>>z</a>>"]), (["t[^0-9]?"], ["<t> y"])])
def test_ambiguous_streams_go_to_the_host(tags, texts):
    """A '>' at a class position that accepts it ('.', a negated class) stays suspect: the host
    path decides the stream — the oracle's bytes, one escalation per such stream — and a clean
    sibling on the same engine stays on the GPU."""
    rng = random.Random(1)
    row0 = [V.all_rows(tags)[0]]  # (the row with the class element: "<a>" itself is suspect against "a.")
    sib = _stream(rng, [p for _ in range(20) for p in (V.clean_form(rng, row0), V.C.plain_run(rng, 1, 8))])
    raw = [H.event_bytes(rng, t[:3]) + H.event_bytes(rng, t[3:]) + H.event_bytes(rng, " tail") + b"data: [DONE]\n\n"
           for t in texts] + [sib]
    assert _suspects(tags, raw) == len(texts) and _suspects(tags, [sib]) == 0
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    _three_way(tags, hip, streams, lambda: random.Random(2))
    st = _stats(hip)
    assert st["escalations"] == len(texts) and st["class_escalations"] == len(texts), st


# ---------------------------------------------------------------- finalize
def test_unfiltered_streams_finalize_on_the_gpu():
    """Streams that are not filtered keep their tags for the finalize's strip.  A close of the
    other row is not the open's close: <thoughts>a</thought>b</thoughts>c is "c".  In
    <thought>a</thoughts>b the row ``thought`` has no close in the text at all, so the interval
    selection never takes the open: the text is kept, on the GPU (fin_host == 0) — no open is
    left pending, which is what would send a finalize to the host."""
    rng = random.Random(9)
    tags = ["thoughts?", "t[0-9]?"]
    texts = ["<thoughts>a</thought>b</thoughts>c", "<thought>a</thoughts>b", "p <THOUGHTS>a</thoughts> q",
             "<t>a</t7>b</T>c<t7>d</t>e</t7>f", "<thought>never closes <t>x</t>y"]
    raw = [H.event_bytes(rng, t[:5]) + H.event_bytes(rng, t[5:]) + b"data: [DONE]\n\n" for t in texts]
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    got = _three_way(tags, hip, streams, lambda: random.Random(5), filt=False)
    assert got[2] == ["c", "<thought>a</thoughts>b", "p  q", "cf", "<thought>never closes y"]
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- mixed
def test_mixed_variant_set():
    """``réflexions?`` under the four keys is a mixed tag set: <RÉFLEXION> and <réflexions> in
    one stream, both rows folded as they are read."""
    tags = ["réflexions?"]
    assert native.tagset_kind(tags, **V.MIXED_KW) == "mixed"
    rng = random.Random(4)
    texts = ["a<RÉFLEXION>x</réflexion>b<réflexions>y</RÉFLEXIONS>c",
             "<réflexions>1</réflexion>2</RÉFLEXIONS>3 <Réflexion",
             "<réflexionz>kept</réflexionz> <RÉFLEXIONS>gone</réflexions>!"]
    raw = [H.event_bytes(rng, t[:7]) + H.event_bytes(rng, t[7:]) + b"data: [DONE]\n\n" for t in texts]
    assert _suspects(tags, raw, V.MIXED_KW) == 0
    hip = _hip(tags, V.MIXED_KW)
    for filt in (True, False):
        for chunk in (5, 400):
            streams = [H.split_random(rng, r, chunk) for r in raw]
            got = _three_way(tags, hip, streams, lambda: random.Random(chunk), filt=filt, kw=V.MIXED_KW)
            if not filt:
                assert got[2] == ["abc", "3 <Réflexion", "<réflexionz>kept</réflexionz> !"]
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- class grid
def test_class_grid_doors(ext):
    """Two door engines on a two-door class grid: equal to the CPU engine, nothing escalated,
    every finalize in the grid."""
    tags = ["think(ing)?", "t[0-9]?"]
    grid = native.make_grid(tags, 0, 2, 4, **V.KW)
    try:
        assert grid.stats()["grid_classes"] == 1
        cpu = _cpu(tags)
        engs = [_hip(tags, grid=grid, door=d) for d in range(2)]
        for d, eng in enumerate(engs):
            for chunk in (17, 400):
                rng = random.Random(100 * d + chunk)
                raw = [_stream(rng, V.clean_pieces(rng, tags, rng.randint(1, 25))) for _ in range(4)]
                assert _suspects(tags, raw) == 0
                streams = [H.split_random(rng, r, chunk) for r in raw]
                ts = rng.randint(0, 10**9)
                want = H.run_engine(cpu, streams, [True] * 4, [True] * 4, random.Random(ts))
                assert H.run_engine(eng, streams, [True] * 4, [True] * 4, random.Random(ts)) == want, (d, chunk)
        for eng in engs:
            st = _stats(eng)
            _assert_all_on_gpu(st)
            assert st["grid_ticks"] > 0, st
        st = grid.stats()
        assert st["grid_classes"] == 1 and st["grid_doors"] == 2 and st["grid_launches"] >= 1, st
    finally:
        grid.stop()


def test_grid_pairing(ext):
    """A set with a variable-width tag is of the class kind even when all its rows are literals:
    refused on a literal grid, accepted on a class grid."""
    lit = ext.HipGrid(0, 2)
    cls = ext.HipGrid(0, 2, classes=True)
    try:
        with pytest.raises(ValueError, match="tick lanes"):
            _hip(["thoughts?"], grid=lit, door=0)
        _hip(["thoughts?"], grid=cls, door=0)
    finally:
        lit.stop()
        cls.stop()


# ---------------------------------------------------------------- server
def test_native_server_hip_variant_tags_on_loop_ticks(ext, monkeypatch):
    """The native server on the HIP engine with ("think(ing)?", "thoughts?") and the key on,
    verify mode, the default tick mode: loop ticks on a class grid (/metrics: qmx_grid_classes
    1), a streaming concatenate response equal to the python implementation's, every stream and
    final equal to the shadow CPU oracle.  With the key off the config is refused with today's text."""
    import httpx
    import test_native_server as T
    import test_variant_tags as TV
    from live_upstream import native_server
    from quorum_amd.runtime.native_server import NativeUnsupported, native_config

    scn = TV.variant_server_scenario()
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "variant_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
    with native_server(scn[0], engine="hip") as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    assert len(lines) == 1 and lines[0].startswith("qmx_grid_classes 1"), lines
    off = dict(scn[0], runtime={"native_regex_tags": True})
    with pytest.raises(NativeUnsupported) as e:
        native_config(off, "127.0.0.1", 1, "hip", 0, 1)
    assert str(e.value) == "thinking_tags ['think(ing)?', 'thoughts?'] need regex semantics: run with --impl python"
