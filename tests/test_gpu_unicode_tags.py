"""GPU: non-ASCII thinking tags (``unicode=True``, ``runtime.native_unicode_tags``) on the HIP engine.

A tag set whose non-ASCII characters are all uncased is a literal tag set: it runs the literal
kernels (``qmx_tick_kernel``, ``qmx_tick_persistent``, a literal ``HipGrid``), whose matchers
compare bytes.  A tag set with a cased character (a pair tag set) is of the class kind: it
runs ``qmx_ctick_kernel`` / a ``HipGrid(classes=True)``, where the text is folded as it is read
— ``<RÉFLEXION>`` matches in place, nothing goes to the host path.  Every case compares byte
for byte with the C++ CPU engine (SSE, flags, content, finals) and asserts that nothing was
escalated or finalized on the host.
"""
import random

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import unicode_tag_cases as U

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _hip(tags, **kw):
    return NativeEngine("hip", tags, device=0, unicode=True, **dict(KW, **kw))


def _cpu(tags):
    return NativeEngine("cpu", tags, unicode=True)


def _stats(eng):
    return dict(eng._e.kernel_stats())


def _assert_all_on_gpu(st, fin=True):
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0, st
    if fin:
        assert st["fin_items"] >= 2, st


def _kfast(monkeypatch, kfast):
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)


def _tag_forms(rng, tags):
    """A tag of the set in lower, upper or mixed case, open or close, or a look-alike."""
    t = rng.choice(tags)
    r = rng.random()
    name = t.lower() if r < 0.25 else t.upper() if r < 0.55 else U.mixed_case(rng, t) if r < 0.85 else U.lookalike(t)
    if rng.random() < 0.15:
        name = name.upper()
    return ("<" if rng.random() < 0.55 else "</") + name + ">"


def _batch(tags, seed):
    """4-6 streams, every chunk a whole event (a tick per event with H.EveryRound): sparse
    streams of events with 1-3 '<' (the <= 4 candidate matcher), dense ones of events with
    6-40 '<' (the MFMA matcher), and alphabet streams in random chunks (partial tags, look-alikes)."""
    rng = random.Random(seed)
    alpha = U.alphabet(tags)
    streams = []
    for _ in range(2):  # sparse
        evs = [H.event_bytes(rng, "".join(_tag_forms(rng, tags) + rng.choice(["x", " 思", "é", ""])
                                          for _ in range(rng.randint(1, 3)))) for _ in range(rng.randint(2, 8))]
        streams.append(evs + [b"data: [DONE]\n\n"])
    for _ in range(2):  # dense
        evs = [H.event_bytes(rng, "".join(_tag_forms(rng, tags) + rng.choice(["", "y", "я "])
                                          for _ in range(rng.randint(6, 40)))) for _ in range(rng.randint(1, 3))]
        streams.append(evs + [b"data: [DONE]\n\n"])
    for _ in range(rng.randint(0, 2)):
        raw = U.stream(rng, U.pieces(rng, tags, rng.randint(1, 30), alpha))
        streams.append(H.split_random(rng, raw, rng.choice([17, 64, 400])))
    return streams


def _differential(tags, hip, cpu, seed):
    streams = _batch(tags, seed)
    n = len(streams)
    want = H.run_engine(cpu, streams, [True] * n, [True] * n, H.EveryRound())
    got = H.run_engine(hip, streams, [True] * n, [True] * n, H.EveryRound())
    assert got == want, (tags, seed)
    ts = seed + 7
    want = H.run_engine(cpu, streams, [True] * n, [True] * n, random.Random(ts))
    got = H.run_engine(hip, streams, [True] * n, [True] * n, random.Random(ts))
    assert got == want, (tags, seed, "random ticks")


# ---------------------------------------------------------------- uncased: the literal kernels
@pytest.mark.parametrize("kfast", [None, "15", "0"])
@pytest.mark.parametrize("mode", ["launch", "lane_grid", "door"])
def test_uncased_set_on_the_literal_kernels(ext, mode, kfast, monkeypatch):
    """["思考", "a思考过程分"] is a literal tag set: a launch per tick, a lane's persistent grid
    and a door of a literal HipGrid (make_grid picks it) all match the CPU engine."""
    _kfast(monkeypatch, kfast)
    if mode == "launch":
        monkeypatch.setenv("QMX_PERSISTENT", "0")
    else:
        monkeypatch.delenv("QMX_PERSISTENT", raising=False)
    tags = U.UNCASED_SET
    assert not ext.tagset_has_classes(tags, False, True)
    grid = native.make_grid(tags, 0, 2, 4, unicode=True) if mode == "door" else None
    try:
        if grid is not None:
            assert grid.stats()["grid_classes"] == 0
        hip = _hip(tags, grid=grid, door=0) if grid is not None else _hip(tags)
        cpu = _cpu(tags)
        for seed in range(6):
            _differential(tags, hip, cpu, 100 + seed)
        _assert_all_on_gpu(_stats(hip))
    finally:
        if grid is not None:
            grid.stop()


# ---------------------------------------------------------------- pairs: the class kernels
@pytest.mark.parametrize("kfast", [None, "15", "0"])
@pytest.mark.parametrize("door", [False, True])
@pytest.mark.parametrize("ti", range(len(U.PAIR_SETS)))
def test_pair_set_on_the_class_kernels(ext, ti, door, kfast, monkeypatch):
    """Pair tag sets, tags in lower, upper and mixed case, look-alikes, sparse and dense tiles:
    a launch per tick (qmx_ctick_kernel) and a door of a class grid match the CPU engine,
    upper-case tags matched in place."""
    _kfast(monkeypatch, kfast)
    tags = U.PAIR_SETS[ti]
    assert ext.tagset_has_classes(tags, False, True)
    grid = native.make_grid(tags, 0, 2, 4, unicode=True) if door else None
    try:
        if grid is not None:
            assert grid.stats()["grid_classes"] == 1
        hip = _hip(tags, grid=grid, door=0) if grid is not None else _hip(tags)
        cpu = _cpu(tags)
        for seed in range(6):
            _differential(tags, hip, cpu, 1000 * ti + seed)
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
@pytest.mark.parametrize("text,tags", [("<RÉFLEXION>", ["réflexion"]), ("</abcdefghijklmnЯ>", ["abcdefghijklmnя"])])
def test_pair_tag_split_at_every_character(text, tags, depth, same_tile):
    """An upper-case tag split at every character, outside and inside a block, both parts in
    one tick and in two: the python oracle's output, decided on the GPU."""
    streams = _split_streams(text, "<" + tags[0].upper() + ">" if depth else "")
    if same_tile:
        streams = [[b"".join(s)] for s in streams]
    hip, cpu = _hip(tags), _cpu(tags)
    for i in range(0, len(streams), 6):
        batch = streams[i:i + 6]
        n = len(batch)
        want = H.run_engine(H.python_engine(tags), batch, [True] * n, [True] * n, H.EveryRound())
        assert want == H.run_engine(cpu, batch, [True] * n, [True] * n, H.EveryRound())
        got = H.run_engine(hip, batch, [True] * n, [True] * n, H.EveryRound())
        assert got == want, (text, depth, i)
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- finalize
@pytest.mark.parametrize("tags", [["é", "思考"], ["思考", "考"]])
def test_unfiltered_streams_finalize_on_the_gpu(tags):
    """Streams that are not filtered keep their tags for the finalize's strip: <É>x</é> (the
    backreference folds both sides), <思考>x</思考>, an open that never closes."""
    rng = random.Random(9)
    texts = ["a <É>x</é> b <é>y</É> c", "p<思考>x</思考>q <思考>", "<È>x</È> <é>unclosed", " <思考>1</思耂>2</思考>3 ",
             "<考>k</考>m<É>"]
    raw = [H.event_bytes(rng, t[:5]) + H.event_bytes(rng, t[5:]) + b"data: [DONE]\n\n" for t in texts]
    n = len(raw)
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    res = [H.run_engine(e, streams, [False] * n, [True] * n, random.Random(5))
           for e in (H.python_engine(tags), _cpu(tags), hip)]
    assert res[0] == res[1] == res[2]
    _assert_all_on_gpu(_stats(hip))


# ---------------------------------------------------------------- plumbing
def test_grid_pairing(ext):
    """A pair tag set needs a class grid, an uncased (literal) one a literal grid."""
    lit = ext.HipGrid(0, 2)
    cls = ext.HipGrid(0, 2, classes=True)
    try:
        with pytest.raises(ValueError, match="tick lanes"):
            _hip(["réflexion"], grid=lit, door=0)
        with pytest.raises(ValueError, match="class tag set only"):
            _hip(["思考"], grid=cls, door=0)
        _hip(["réflexion"], grid=cls, door=0)
        _hip(["思考"], grid=lit, door=1)
    finally:
        lit.stop()
        cls.stop()


def test_native_server_hip_unicode_tags_on_loop_ticks(ext, monkeypatch):
    """The native server on the HIP engine with ["think", "réflexion"], the key on, verify mode
    and the default tick mode: loop ticks on a class grid (/metrics: qmx_grid_classes 1), equal
    to the FastAPI app, every stream and final equal to the shadow CPU oracle."""
    import httpx
    import test_native_server as T
    import test_unicode_tags as TU
    from live_upstream import native_server

    scn = TU.unicode_server_scenario(("think", "réflexion"))
    monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(scn, "unicode_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    assert after["class_grid_launches"] > before["class_grid_launches"], (before, after)
    assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
    with native_server(scn[0], engine="hip") as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    assert len(lines) == 1 and lines[0].startswith("qmx_grid_classes 1"), lines
