"""GPU: mixed thinking tag sets (``mixed=True``, ``runtime.native_mixed_tags``) on the HIP engine.

A tag set with a class element and a non-ASCII literal is of the class kind: it runs
``qmx_ctick_kernel`` / a ``HipGrid(classes=True)``.  The byte matchers find the tags they can
decide; a tag with a class element or a pair character comes from one walk that folds the text
and tells a class marker from a UTF-8 byte by the tag's bitmap.  A candidate whose class
position holds '<', '>' or a non-ASCII byte is suspect and its stream goes to the host path,
as for class tag sets.  Every case compares byte for byte with the C++ CPU engine (SSE, flags,
content, finals) or the python oracle.
"""
import json
import random

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import mixed_tag_cases as M

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _hip(tags, **kw):
    return NativeEngine("hip", tags, device=0, **dict(KW, **M.KW, **kw))


def _cpu(tags):
    return NativeEngine("cpu", tags, **M.KW)


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


def _suspects(ext, tags, raw) -> int:
    """Streams of `raw` with a suspect candidate: the kernels' rule (qmx_text.h mixed_candidate)
    on the host, over the whole content, streaming and strip tables."""
    n = 0
    for r in raw:
        text = _content(r).encode()
        n += (ext.class_suspects(tags, text, False, True, True) + ext.class_suspects(tags, text, True, True, True)) > 0
    return n


def _batch(tags, seed):
    """4-6 streams, every chunk a whole event: sparse streams of events with 1-3 '<', dense
    ones of events with 6-40 '<' (the MFMA matcher), and clean-piece streams in random chunks
    (partial tags, look-alikes).  -> (chunk lists, raw streams)"""
    rng = random.Random(seed)
    streams, raw = [], []
    for _ in range(2):  # sparse
        evs = [H.event_bytes(rng, "".join(M.clean_form(rng, tags) + rng.choice(["x", " 思", "é", ""])
                                          for _ in range(rng.randint(1, 3)))) for _ in range(rng.randint(2, 8))]
        streams.append(evs + [b"data: [DONE]\n\n"])
    for _ in range(2):  # dense
        evs = [H.event_bytes(rng, "".join(M.clean_form(rng, tags) + rng.choice(["", "y", "я "])
                                          for _ in range(rng.randint(6, 40)))) for _ in range(rng.randint(1, 3))]
        streams.append(evs + [b"data: [DONE]\n\n"])
    raw = [b"".join(s) for s in streams]
    for _ in range(rng.randint(0, 2)):
        r = M.U.stream(rng, M.clean_pieces(rng, tags, rng.randint(1, 30)))
        raw.append(r)
        streams.append(H.split_random(rng, r, rng.choice([17, 64, 400])))
    return streams, raw


def _differential(ext, tags, hip, cpu, seed):
    streams, raw = _batch(tags, seed)
    assert _suspects(ext, tags, raw) == 0, (tags, seed)  # the generators' own condition
    n = len(streams)
    want = H.run_engine(cpu, streams, [True] * n, [True] * n, H.EveryRound())
    got = H.run_engine(hip, streams, [True] * n, [True] * n, H.EveryRound())
    assert got == want, (tags, seed)
    ts = seed + 7
    want = H.run_engine(cpu, streams, [True] * n, [True] * n, random.Random(ts))
    got = H.run_engine(hip, streams, [True] * n, [True] * n, random.Random(ts))
    assert got == want, (tags, seed, "random ticks")


# ---------------------------------------------------------------- clean differential
@pytest.mark.parametrize("kfast", [None, "15", "0"])
@pytest.mark.parametrize("door", [False, True])
@pytest.mark.parametrize("ti", range(len(M.CLEAN_SETS)))
def test_clean_streams_on_the_class_kernels(ext, ti, door, kfast, monkeypatch):
    """Clean streams — tags in lower, upper and mixed case, look-alikes, partial tags, sparse
    and dense tiles: a launch per tick (qmx_ctick_kernel) and a door of a class grid match the
    CPU engine, nothing escalated, every finalize on the GPU."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    if not door:
        monkeypatch.setenv("QMX_PERSISTENT", "0")
    tags = M.CLEAN_SETS[ti]
    assert ext.tagset_kind(tags, True, True, True) == "mixed"
    grid = native.make_grid(tags, 0, 2, 4, **M.KW) if door else None
    try:
        if grid is not None:
            assert grid.stats()["grid_classes"] == 1
        hip = _hip(tags, grid=grid, door=0) if grid is not None else _hip(tags)
        cpu = _cpu(tags)
        for seed in range(6):
            _differential(ext, tags, hip, cpu, 1000 * ti + seed)
        st = _stats(hip)
        _assert_all_on_gpu(st)
        if grid is not None:
            assert st["grid_ticks"] > 0, st
    finally:
        if grid is not None:
            grid.stop()


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
@pytest.mark.parametrize("text,tags,released", [("<ABCDEFGHIJKLMN7Я>", M.LONG_SETS[0], 2),
                                                 ("<abcdefghijklm思5>", M.LONG_SETS[1], 1)])
def test_long_tag_split_at_every_character(text, tags, released, depth, same_tile):
    """A tag whose class position and non-ASCII literal lie at and past the 16-byte window,
    split at every character, outside and inside a block, both parts in one tick and in two:
    the python oracle's output.  Outside a block a first part that is no prefix of the source
    text ("<…n7", "<…n7Я"; "<…思5") was released by the reference, so the tag is none: with
    both parts in one tick such a stream is decided by the host path, as for class tags."""
    streams = _split_streams(text, "<" + text[1:-1].lower() + ">" if depth else "")
    if same_tile:
        streams = [[b"".join(s)] for s in streams]
    hip = _hip(tags)
    for i in range(0, len(streams), 6):
        batch = streams[i:i + 6]
        n = len(batch)
        want = H.run_engine(H.python_engine(tags), batch, [True] * n, [True] * n, H.EveryRound())
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
@pytest.mark.parametrize("tags,texts", [
    (["réfl.xion", "思[0-9]", "é.", "think"], ["<réfléxion>x</RÉFLÉXION>y", "<réfl<xion>z", "<é>>x</é>>y", "<思é>q"]),
    (["th.nk", "思考"], ["<th<nk>z", "<th思nk>x</th思nk>y", "<th>nk>z"]),
    (["r.flexion", "réflexion"], ["a<RÉFLEXION>x</réflexion>y"]),
    (["réflexion", "r.flexion"], ["a<RÉFLEXION>x</réflexion>y"]),
])
def test_ambiguous_streams_go_to_the_host(ext, tags, texts):
    """A candidate whose class position holds '<', '>' or a non-ASCII byte is decided by the
    host path: the C++ engine's (and the oracle's) output, one escalation per such stream, the
    clean sibling on the same engine stays on the GPU."""
    rng = random.Random(1)
    # (the sibling uses the first tag with a class element: "<réflexion>" is suspect against "r.flexion")
    sib = M.U.stream(rng, M.clean_pieces(rng, [t for t in tags if "." in t or "[" in t][:1], 20))
    raw = [H.event_bytes(rng, t[:3]) + H.event_bytes(rng, t[3:]) + H.event_bytes(rng, " tail") + b"data: [DONE]\n\n"
           for t in texts] + [sib]
    assert _suspects(ext, tags, raw) == len(texts) and _suspects(ext, tags, [sib]) == 0
    n = len(raw)
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    want = H.run_engine(_cpu(tags), streams, [True] * n, [True] * n, random.Random(2))
    assert want == H.run_engine(H.python_engine(tags), streams, [True] * n, [True] * n, random.Random(2))
    got = H.run_engine(hip, streams, [True] * n, [True] * n, random.Random(2))
    assert got == want
    st = _stats(hip)
    assert st["escalations"] == len(texts) and st["class_escalations"] == len(texts), st


# ---------------------------------------------------------------- finalize
FIN_TAGS = ["réfl.xion", "思[0-9]", "é.", "think"]


def test_unfiltered_streams_finalize_on_the_gpu():
    """Streams that are not filtered keep their tags for the finalize's strip: a close in the
    other case is its open's close (<RÉFL0XION>x</réfl0xion>), a close of the same tag with
    another capture is passed over when the right one follows (<思7>1</思8>2</思7>3), an open
    that never closes is text."""
    rng = random.Random(9)
    texts = ["a <RÉFL0XION>x</réfl0xion> b", "<思7>1</思8>2</思7>3", "<réfl1xion>never closes <think>t</THINK>u",
             "<é1>x</É1>y <É?>z</é?> w", "p<think>x</think>q <réfl.xion>"]
    raw = [H.event_bytes(rng, t[:5]) + H.event_bytes(rng, t[5:]) + b"data: [DONE]\n\n" for t in texts]
    n = len(raw)
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(FIN_TAGS)
    res = [H.run_engine(e, streams, [False] * n, [True] * n, random.Random(5))
           for e in (H.python_engine(FIN_TAGS), _cpu(FIN_TAGS), hip)]
    assert res[0] == res[1] == res[2]
    assert res[2][2] == ["a  b", "3", "<réfl1xion>never closes u", "y  w", "pq <réfl.xion>"]
    _assert_all_on_gpu(_stats(hip))


def test_finalize_close_that_is_not_the_captured_text():
    """<思7>x</思8> with no later </思7>: the close is not the text the open captured, so the
    block stays text on the oracle, the C++ engine and the HIP engine (whose finalize leaves an
    open without its close to the host path: both requests of the run, counted as class ones)."""
    rng = random.Random(3)
    raw = [H.event_bytes(rng, "<思7>x</思8> y") + b"data: [DONE]\n\n"]
    hip = _hip(FIN_TAGS)
    res = [H.run_engine(e, [raw], [False], [True], H.EveryRound())
           for e in (H.python_engine(FIN_TAGS), _cpu(FIN_TAGS), hip)]
    assert res[0] == res[1] == res[2]
    assert res[2][2] == ["<思7>x</思8> y"]
    st = _stats(hip)
    assert st["escalations"] == 0 and st["fin_host"] == st["class_fin_host"] == 2, st


# ---------------------------------------------------------------- plumbing
def test_grid_pairing(ext):
    """A mixed tag set is of the class kind: refused on a literal grid, accepted on a class grid."""
    lit = ext.HipGrid(0, 2)
    cls = ext.HipGrid(0, 2, classes=True)
    try:
        with pytest.raises(ValueError, match="tick lanes"):
            _hip(["th.nk", "思考"], grid=lit, door=0)
        _hip(["th.nk", "思考"], grid=cls, door=0)
        _hip(["réfl.xion"], grid=cls, door=1)
    finally:
        lit.stop()
        cls.stop()


def test_two_engines_keep_their_own_tables():
    """Two engines with different mixed tag sets in one process, both made before either runs."""
    text = "<réfl0xion>a</RÉFL0XION>b<réflAxion>c</réflaxion>d"
    sets = [["réfl.xion", "思考"], ["réfl[0-9]xion", "思考"]]
    hips = [_hip(t) for t in sets]
    rng = random.Random(9)
    streams = [[H.event_bytes(rng, text) + b"data: [DONE]\n\n"]]
    for tags, hip, content in zip(sets, hips, ["bd", "b<réflAxion>c</réflaxion>d"]):
        want = H.run_engine(_cpu(tags), streams, [True], [True], H.EveryRound())
        got = H.run_engine(hip, streams, [True], [True], H.EveryRound())
        assert got == want, tags
        assert got[0][0][1:] == (1, content) and got[2] == [content], (tags, got)
        st = _stats(hip)
        assert st["escalations"] == 0 and st["fin_host"] == 0 and st["fin_items"] >= 1, st


def test_native_server_hip_mixed_tags_on_loop_ticks(ext, monkeypatch):
    """The native server on the HIP engine with ("think", "réfl.xion", "思考"), the three keys
    on, verify mode and the default tick mode: loop ticks on a class grid (/metrics:
    qmx_grid_classes 1), equal to the FastAPI app, every stream and final equal to the shadow
    CPU oracle."""
    import httpx
    import test_mixed_tags as TM
    import test_native_server as T
    from live_upstream import native_server

    scn = TM.mixed_server_scenario()
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "mixed_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
    with native_server(scn[0], engine="hip") as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    assert len(lines) == 1 and lines[0].startswith("qmx_grid_classes 1"), lines
