"""GPU: class thinking tags on the persistent loop-tick grid (``HipGrid(..., classes=True)``).

A class grid launches ``qmx_ctick_persistent``: the literal grid's relay / claim / item loop
around the items compiled with the class paths.  Engines with a class tag set post into its
doors exactly as literal engines post into a literal grid's; everything after the kernel
(escalations, host finalize, host-opened streams) is the door path's shared code.  Every case
compares byte for byte with the C++ CPU engine or the python oracle, on a door, and stops its
grid when it is done.
"""
import random
import time

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.engine import FinalizeRequest
from quorum_amd.ops.native import NativeEngine

import class_tag_cases as C
import engine_harness as H

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def _door(tags, grid, door, **kw):
    return NativeEngine("hip", tags, device=0, classes=True, grid=grid, door=door, **dict(KW, **kw))


def _cpu(tags):
    return NativeEngine("cpu", tags, classes=True)


def _stats(eng):
    return dict(eng._e.kernel_stats())


def _stream(rng, pieces, per_event=3):
    """Upstream bytes: the pieces grouped into content events of 1..per_event pieces."""
    parts, i = [], 0
    while i < len(pieces):
        k = rng.randint(1, per_event)
        parts.append(H.event_bytes(rng, "".join(pieces[i:i + k])))
        i += k
    return b"".join(parts) + b"data: [DONE]\n\n"


def _assert_clean(ext, tags, raw):
    """The generator's own check: no candidate of a clean stream's content is suspect."""
    import json

    for r in raw:
        text = "".join(json.loads(ev[6:])["choices"][0]["delta"]["content"]
                       for ev in r.decode().split("\n\n") if ev.startswith("data: {"))
        assert ext.class_suspects(tags, text.encode()) == 0, (tags, text)
        assert ext.class_suspects(tags, text.encode(), strip=True) == 0, (tags, text)


def _clean_batch(ext, tags, seed, chunk):
    """4-6 clean streams of up to 30 pieces in chunks of up to `chunk` bytes, and a tick seed."""
    rng = random.Random(seed)
    n = rng.randint(4, 6)
    raw = [_stream(rng, C.clean_pieces(rng, tags, rng.randint(1, 30))) for _ in range(n)]
    _assert_clean(ext, tags, raw)
    return [H.split_random(rng, r, chunk) for r in raw], n, rng.randint(0, 10**9)


def _differential(ext, tags, eng, cpu, seed, chunk):
    streams, n, ts = _clean_batch(ext, tags, seed, chunk)
    want = H.run_engine(cpu, streams, [True] * n, [True] * n, random.Random(ts))
    got = H.run_engine(eng, streams, [True] * n, [True] * n, random.Random(ts))
    assert got == want, (tags, seed, chunk)


def _assert_all_on_gpu(st):
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0 and st["fin_items"] >= 2, st
    assert st["grid_ticks"] > 0, st


# ---------------------------------------------------------------- clean differential
@pytest.mark.parametrize("ti,kfast", [(1, None), (3, None), (5, None), (3, "0")])
def test_class_grid_doors_match_cpu(ext, ti, kfast, monkeypatch):
    """Three door engines on a three-door class grid, clean streams in chunks of 17 and 400
    bytes, 2 seeds per door: equal to the C++ CPU engine, nothing escalated, every finalize in
    the grid, the ticks counted as grid ticks.  kfast "0": the block paths."""
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    tags = C.CLEAN_SETS[ti]
    grid = ext.HipGrid(0, 3, 4, classes=True)
    try:
        engs = [_door(tags, grid, d) for d in range(3)]
        cpu = _cpu(tags)
        for d, eng in enumerate(engs):
            for chunk in (17, 400):
                for seed in range(2):
                    _differential(ext, tags, eng, cpu, 1000 * ti + 100 * d + 10 * chunk + seed, chunk)
        for eng in engs:
            _assert_all_on_gpu(_stats(eng))
        st = grid.stats()
        assert st["grid_classes"] == 1 and st["grid_doors"] == 3 and st["grid_launches"] >= 1, st
        assert st["grid_wg_per_cu"] == 1, st
    finally:
        grid.stop()


def test_class_grid_two_doors_per_engine(ext):
    """An engine with two doors of a class grid (buffer sets, kernel parameters — the class
    tables' pointer among them — and template tables per door) matches the CPU engine."""
    tags = C.CLEAN_SETS[3]
    grid = ext.HipGrid(0, 4, 4, classes=True)
    try:
        cpu = _cpu(tags)
        for door in (0, 2):
            eng = _door(tags, grid, door, ndoors=2)
            for chunk in (17, 400):
                _differential(ext, tags, eng, cpu, 7000 + door + chunk, chunk)
            _assert_all_on_gpu(_stats(eng))
    finally:
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
@pytest.mark.parametrize("text", ["<th.nk>", "</th.nk>", "<thXnk>", "</thXnk>"])
def test_class_grid_holdback_split_at_every_byte(ext, text, depth, same_tile):
    """A tag split at every byte, outside and inside a block, on a door, against the python
    oracle.  Separate ticks: decided in the grid.  same_tile: a tag whose first part the
    reference had released is decided by the host path — for "<thXnk>" outside a block the
    splits after "<thX", "<thXn", "<thXnk" (the earlier ones are prefixes of the source text,
    held: a real tag)."""
    tags = ["th.nk"]
    streams = _split_streams(text, "<th1nk>" if depth else "")
    if same_tile:
        streams = [[b"".join(s)] for s in streams]
    grid = ext.HipGrid(0, 2, 2, classes=True)
    try:
        eng = _door(tags, grid, 1)
        for i in range(0, len(streams), 6):
            batch = streams[i:i + 6]
            n = len(batch)
            want = H.run_engine(H.python_engine(tags), batch, [True] * n, [True] * n, H.EveryRound())
            got = H.run_engine(eng, batch, [True] * n, [True] * n, H.EveryRound())
            assert got == want, (text, depth, i)
        st = _stats(eng)
        assert st["grid_ticks"] > 0, st
        if not same_tile:
            assert st["escalations"] == 0, st
        elif text == "<thXnk>" and depth == 0:
            assert st["class_escalations"] == 3 and st["escalations"] == 3, st
    finally:
        grid.stop()


# ---------------------------------------------------------------- ambiguous windows
@pytest.mark.parametrize("tags,texts", [
    (["th.nk"], ["<th日nk>x</th日nk>y", "<th<nk>z", "<th>nk>z"]),
    (["a.", "a"], ["<a>>x</a>>y"]),
])
def test_class_grid_ambiguous_streams_go_to_the_host(ext, tags, texts):
    """A candidate whose class position holds '<', '>' or a non-ASCII byte, met by a door's
    sub-grid, is decided by the host path: the oracle's output, one escalation per such stream;
    the clean sibling on the same door stays in the grid."""
    rng = random.Random(1)
    # (the sibling of ["a.", "a"] uses the first tag only: "<a>" itself is suspect against "a.")
    sib = _stream(rng, C.clean_pieces(rng, tags[:1], 20))
    _assert_clean(ext, tags, [sib])
    raw = [H.event_bytes(rng, t[:3]) + H.event_bytes(rng, t[3:]) + H.event_bytes(rng, " tail") + b"data: [DONE]\n\n"
           for t in texts] + [sib]
    n = len(raw)
    streams = [H.split_random(rng, r, 64) for r in raw]
    grid = ext.HipGrid(0, 2, 2, classes=True)
    try:
        eng = _door(tags, grid, 0)
        want = H.run_engine(H.python_engine(tags), streams, [True] * n, [True] * n, random.Random(2))
        assert want == H.run_engine(_cpu(tags), streams, [True] * n, [True] * n, random.Random(2))
        got = H.run_engine(eng, streams, [True] * n, [True] * n, random.Random(2))
        assert got == want
        st = _stats(eng)
        assert st["escalations"] == len(texts) and st["class_escalations"] == len(texts), st
        assert st["grid_ticks"] > 0, st
    finally:
        grid.stop()


# ---------------------------------------------------------------- finalize
def test_class_grid_finalize_close_must_equal_the_captured_text(ext):
    """<thXnk>a</thYnk>b</thxnk>c: the first close by tag is not the open's captured text, so
    the grid's finalize item hands the request to the host (text "c"); the clean session beside
    it is finalized in the grid."""
    tags = ["th.nk"]
    grid = ext.HipGrid(0, 2, 2, classes=True)
    try:
        hip = _door(tags, grid, 0)
        rng = random.Random(4)
        texts = ["<thXnk>a</thYnk>b</thxnk>c", "<thXnk>a</thxnk>c d"]
        slots = [hip.open(i, False, True) for i in range(2)]
        for s, t in zip(slots, texts):
            hip.feed(s, H.event_bytes(rng, t) + b"data: [DONE]\n\n")
            hip.finish(s)
        for _ in range(20):
            if not hip.has_work():
                break
            hip.tick(H.CREATED)
        assert [hip.text(s) for s in slots] == texts
        fins = {}

        def finalize(slot):
            fid = hip.submit_finalize(FinalizeRequest([slot], True, "texts"))
            for _ in range(10):
                if not hip.has_work():
                    break
                fins.update(dict(hip.tick(H.CREATED)[1]))
            return fins[fid]

        before = _stats(hip)
        assert finalize(slots[1]) == ["c d"]
        mid = _stats(hip)
        assert mid["fin_host"] == before["fin_host"] and mid["fin_items"] == before["fin_items"] + 1, (before, mid)
        assert finalize(slots[0]) == ["c"]
        after = _stats(hip)
        assert after["fin_host"] == mid["fin_host"] + 1 and after["class_fin_host"] == mid["class_fin_host"] + 1, (mid, after)
        assert after["grid_ticks"] > 0, after  # (counted for ticks with stream tiles)
        for s in slots:
            hip.release(s)
    finally:
        grid.stop()


# ---------------------------------------------------------------- lifetime
def test_class_grid_idle_stop_and_relaunch(ext):
    """The host stops an idle class grid and the next post relaunches it: the relaunch is the
    class kernel again (the second batch's class tags are matched, equal to the CPU engine)."""
    tags = C.CLEAN_SETS[1]
    grid = ext.HipGrid(0, 2, 2, idle_ms=5, classes=True)
    try:
        eng = _door(tags, grid, 1)
        cpu = _cpu(tags)
        _differential(ext, tags, eng, cpu, 61, 64)
        launches = grid.stats()["grid_launches"]
        assert launches >= 1
        time.sleep(0.02)
        grid.housekeep()  # idle > 5 ms: stopped
        assert grid.stats()["grid_stops"] >= 1
        _differential(ext, tags, eng, cpu, 62, 64)
        st = grid.stats()
        assert st["grid_launches"] > launches and st["grid_classes"] == 1, st
        _assert_all_on_gpu(_stats(eng))
    finally:
        grid.stop()


# ---------------------------------------------------------------- plumbing
def test_class_grid_pairing_rules(ext):
    """A grid runs one kernel for all its doors: a class tag set needs a class grid, a literal
    tag set (with or without the classes flag on the engine) a literal one."""
    lit = ext.HipGrid(0, 2)
    cls = ext.HipGrid(0, 2, classes=True)
    try:
        with pytest.raises(ValueError, match="tick lanes"):
            NativeEngine("hip", ["think", "th.nk"], device=0, classes=True, grid=lit, door=0, **KW)
        with pytest.raises(ValueError):
            NativeEngine("hip", ["think"], device=0, classes=True, grid=cls, door=0, **KW)
        with pytest.raises(ValueError):
            NativeEngine("hip", ["think"], device=0, grid=cls, door=0, **KW)
        NativeEngine("hip", ["think", "th.nk"], device=0, classes=True, grid=cls, door=0, **KW)
        assert cls.stats()["grid_classes"] == 1 and lit.stats()["grid_classes"] == 0
    finally:
        lit.stop()
        cls.stop()


def test_make_grid_picks_the_kind(ext):
    """native.make_grid: the class grid only for a tag set that has class positions."""
    grids = [native.make_grid(["think", "t[0-9]"], 0, 2, classes=True), native.make_grid(["think"], 0, 2, classes=True),
             native.make_grid(["think"], 0, 2)]
    try:
        assert [g.stats()["grid_classes"] for g in grids] == [1, 0, 0]
    finally:
        for g in grids:
            g.stop()


# ---------------------------------------------------------------- server
@pytest.mark.parametrize("tick_mode,want", [(None, "qmx_grid_classes 1."), ("lanes", None)])
def test_native_server_metrics_show_the_grid_kernel(ext, tick_mode, want):
    """/metrics of a server with ["think", "th.nk"]: by default loop ticks on a class grid
    (qmx_grid_classes 1); tick_mode lanes still gives lanes (no grid, no such line)."""
    import httpx
    import test_class_tags as TC
    from live_upstream import native_server

    cfg = TC.class_server_scenario()[0]
    with native_server(cfg, engine="hip", tick_mode=tick_mode) as port:
        m = httpx.get(f"http://127.0.0.1:{port}/metrics").text
    lines = [l for l in m.splitlines() if l.startswith("qmx_grid_classes ")]
    if want is None:
        assert lines == [], lines
    else:
        assert len(lines) == 1 and lines[0].startswith(want), lines


@pytest.mark.parametrize("light_host", [None, "2"])
def test_native_server_hip_class_tags_on_loop_ticks(ext, monkeypatch, light_host):
    """The native server on the HIP engine with ["think", "th.nk"], verify mode and the default
    tick mode: loop ticks on a class grid (the server's counters: the class grid kernel was
    launched and the loops' ticks rode it), equal to the FastAPI app, every stream and final
    equal to the shadow CPU oracle.  light_host "2" (QMX_LIGHT_HOST): the idle loop's session
    runs on the host path beside the class grid — same output, same verification."""
    import test_class_tags as TC
    import test_native_server as T

    if light_host is None:
        monkeypatch.setenv("QMX_LIGHT_HOST", "0")
    else:
        monkeypatch.setenv("QMX_LIGHT_HOST", light_host)
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(TC.class_server_scenario(), "class_tags_hip_grid", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
    if light_host is None:
        assert after["class_grid_launches"] > before["class_grid_launches"], (before, after)
        assert after["class_grid_ticks"] > before["class_grid_ticks"], (before, after)
