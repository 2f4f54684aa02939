"""GPU: class thinking tags ('.', bracket classes, escaped punctuation) on the HIP engine.

A class tag set runs in the tick / finalize kernel that carries the class paths
(``qmx_ctick_kernel``): class tags are matched in place where every class position holds one
ASCII byte that is neither '<' nor '>', and a stream with an ambiguous (suspect) window, or a
finalize whose close is not its open's captured text, goes to the exact host path.  Every case
compares byte for byte with the C++ CPU engine or the python oracle.
"""
import random

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.engine import FinalizeRequest
from quorum_amd.ops.native import NativeEngine

import class_tag_cases as C
import engine_harness as H

pytestmark = pytest.mark.gpu

KW = dict(max_slots=64, content_cap=1 << 16)


def _hip(tags, **kw):
    return NativeEngine("hip", tags, device=0, classes=True, **dict(KW, **kw))


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


# ---------------------------------------------------------------- clean differential
@pytest.mark.parametrize("kfast", [None, "15", "0"])
@pytest.mark.parametrize("ti", range(len(C.CLEAN_SETS)))
def test_clean_streams_match_cpu(ti, kfast, monkeypatch):
    """Clean streams, chunk sizes 3 / 17 / 64 / 400, 8 seeds: HIP == C++ CPU engine (SSE,
    flags, content, finals), nothing escalated, every finalize on the GPU.  QMX_KFAST default,
    15 and 0 (the block paths)."""
    ext = native.require()
    if kfast is None:
        monkeypatch.delenv("QMX_KFAST", raising=False)
    else:
        monkeypatch.setenv("QMX_KFAST", kfast)
    tags = C.CLEAN_SETS[ti]
    hip, cpu = _hip(tags), _cpu(tags)
    for chunk in (3, 17, 64, 400):
        for seed in range(8):
            rng = random.Random(1000 * ti + 10 * chunk + seed)
            n = rng.randint(4, 6)
            raw = [_stream(rng, C.clean_pieces(rng, tags, rng.randint(1, 30))) for _ in range(n)]
            _assert_clean(ext, tags, raw)
            streams = [H.split_random(rng, r, chunk) for r in raw]
            ts = rng.randint(0, 10**9)
            want = H.run_engine(cpu, streams, [True] * n, [True] * n, random.Random(ts))
            got = H.run_engine(hip, streams, [True] * n, [True] * n, random.Random(ts))
            assert got == want, (tags, chunk, seed, raw)
    st = _stats(hip)
    assert st["escalations"] == 0 and st["class_escalations"] == 0, st
    assert st["fin_host"] == 0 and st["class_fin_host"] == 0 and st["fin_items"] >= 2, st


def test_clean_streams_unfiltered_finalize_on_gpu():
    """Streams that are not filtered as they pass keep their tags for the finalize's strip:
    blocks whose close repeats the open's text (in another case) are stripped by the
    class-aware K3 on the GPU, equal to the CPU engine and the oracle."""
    tags = C.CLEAN_SETS[3]
    hip = _hip(tags)
    rng = random.Random(77)
    n = 5
    raw = []
    for _ in range(n):
        pieces = []
        for _ in range(10):
            inst = C.instance(rng, rng.choice(tags))
            pieces += [C.plain_run(rng, 1, 8), f"<{inst}>", C.plain_run(rng, 0, 8), f"</{inst.swapcase()}>"]
        raw.append(_stream(rng, pieces))
    _assert_clean(native.require(), tags, raw)
    streams = [H.split_random(rng, r, 400) for r in raw]
    res = [H.run_engine(e, streams, [False] * n, [True] * n, random.Random(5))
           for e in (H.python_engine(tags), _cpu(tags), hip)]
    assert res[0] == res[1] == res[2]
    st = _stats(hip)
    assert st["fin_host"] == 0 and st["fin_items"] >= 2 and st["escalations"] == 0, st


# ---------------------------------------------------------------- dense tiles
def _dense_stream(rng, tags, n_lt):
    """One content event with exactly n_lt '<' (well-formed class tags and short runs)."""
    out = []
    for _ in range(n_lt):
        out.append(("<" if rng.random() < 0.55 else "</") + C.instance(rng, rng.choice(tags)) + ">" + C.plain_run(rng, 0, 3))
    return H.event_bytes(rng, "".join(out)) + b"data: [DONE]\n\n"


@pytest.mark.parametrize("ti", [1, 3, 5])
def test_dense_tiles(ti):
    """5..63 '<' in one tile, and more than 63 up to MAX_CAND: class tags, clean, whole streams
    in one tile each."""
    lim = native.require().kernel_limits()
    tags = C.CLEAN_SETS[ti]
    rng = random.Random(ti)
    counts = [5, 63, 64, min(lim["MAX_CAND"], 200), 17]
    raw = [_dense_stream(rng, tags, k) for k in counts]
    assert all(len(r) <= lim["TILE_MAX"] for r in raw)
    _assert_clean(native.require(), tags, raw)
    streams = [[r] for r in raw]
    n = len(raw)
    hip = _hip(tags)
    want = H.run_engine(_cpu(tags), streams, [True] * n, [True] * n, H.EveryRound())
    got = H.run_engine(hip, streams, [True] * n, [True] * n, H.EveryRound())
    assert got == want
    assert got == H.run_engine(H.python_engine(tags), streams, [True] * n, [True] * n, H.EveryRound())
    st = _stats(hip)
    assert st["escalations"] == 0 and st["fin_host"] == 0 and st["fin_items"] >= 2, st


# ---------------------------------------------------------------- window crossing
def test_class_positions_past_the_window():
    """Class positions inside and past the 16-byte matcher window: tags and near misses that
    differ only at such a position (a letter for the digit, a newline for the dot)."""
    tags = C.CLEAN_SETS[5]
    rng = random.Random(5)
    forms = ["<abcdefghijklmXop7rs>", "</ABCDEFGHIJKLM-OP0RS>", "<abcdefghijklm.opXrs>", "</abcdefghijklmZop/rs>",
             "<abcdefghijklm\nop1rs>", "<abcdefghijklmnopQ>", "</abcdefghijklmnop9>", "<abcdefghijklmnop\n>",
             "</abcdefghijklmnop\n>", "<abcdefghijklmnoq1>", "<think>", "</think>", "<abcdefghijklm.op7 ", "7rs> ", " t ", "\n"]
    raw = []
    for _ in range(6):
        raw.append(_stream(rng, [rng.choice(forms) for _ in range(30)]))
    _assert_clean(native.require(), tags, raw)
    n = len(raw)
    streams = [H.split_random(rng, r, rng.choice([17, 64, 400])) for r in raw]
    hip = _hip(tags)
    for filt in (True, False):
        res = [H.run_engine(e, streams, [filt] * n, [True] * n, random.Random(3))
               for e in (H.python_engine(tags), _cpu(tags), hip)]
        assert res[0] == res[1] == res[2], filt
    assert _stats(hip)["escalations"] == 0


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
def test_holdback_split_at_every_byte(text, depth, same_tile):
    """A tag split at every byte, outside and inside a block, against the python oracle: the
    source text "<th.nk>" is held outside a block at every split, "<thX" | "nk>" is released
    there (no tag) and recognised inside one.  same_tile: both parts in one tick — a tag whose
    first part the reference had released is then decided by the host path."""
    tags = ["th.nk"]
    streams = _split_streams(text, "<th1nk>" if depth else "")
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
    if not same_tile:
        assert st["escalations"] == 0, st
    elif text == "<thXnk>" and depth == 0:
        # splits after "<", "<t", "<th" are prefixes of the source text (held, a real tag);
        # after "<thX", "<thXn", "<thXnk" the first part was released
        assert st["class_escalations"] == 3 and st["escalations"] == 3, st


# ---------------------------------------------------------------- ambiguous windows
@pytest.mark.parametrize("tags,texts", [
    (["th.nk"], ["<th日nk>x</th日nk>y", "<th<nk>z", "<th>nk>z"]),
    (["a.", "a"], ["<a>>x</a>>y"]),
])
def test_ambiguous_streams_go_to_the_host(tags, texts):
    """A candidate whose class position holds '<', '>' or a non-ASCII byte is decided by the
    host path: the oracle's output, one escalation per such stream, the clean sibling on the
    same engine stays on the GPU."""
    rng = random.Random(1)
    # (the sibling of ["a.", "a"] uses the first tag only: "<a>" itself is suspect against "a.")
    sib = _stream(rng, C.clean_pieces(rng, tags[:1], 20))
    _assert_clean(native.require(), tags, [sib])
    raw = [H.event_bytes(rng, t[:3]) + H.event_bytes(rng, t[3:]) + H.event_bytes(rng, " tail") + b"data: [DONE]\n\n"
           for t in texts] + [sib]
    n = len(raw)
    streams = [H.split_random(rng, r, 64) for r in raw]
    hip = _hip(tags)
    want = H.run_engine(H.python_engine(tags), streams, [True] * n, [True] * n, random.Random(2))
    assert want == H.run_engine(_cpu(tags), streams, [True] * n, [True] * n, random.Random(2))
    got = H.run_engine(hip, streams, [True] * n, [True] * n, random.Random(2))
    assert got == want
    st = _stats(hip)
    assert st["escalations"] == len(texts) and st["class_escalations"] == len(texts), st


# ---------------------------------------------------------------- finalize
def test_finalize_close_must_equal_the_captured_text():
    """<thXnk>a</thYnk>b</thxnk>c: the first close by tag is not the open's captured text, so
    the request is finalized on the host (text "c"); the clean session beside it on the GPU."""
    tags = ["th.nk"]
    hip = _hip(tags)
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
    for s in slots:
        hip.release(s)


# ---------------------------------------------------------------- plumbing
def test_two_engines_keep_their_own_tables():
    """Two one-shot engines with different class tag sets in one process, both made before
    either runs: one slot and one content event each, finished and finalized with strip on —
    deltas, flags, content and the final event equal to a CPU engine of the same tags (an
    engine reading the other's device tables would strip the other's block)."""
    text = "<thXnk>a</thXnk>b<th1nk>c</th1nk>d"
    sets = [["th.nk"], ["th[0-9]nk"]]
    hips = [_hip(t) for t in sets]
    rng = random.Random(9)
    streams = [[H.event_bytes(rng, text) + b"data: [DONE]\n\n"]]
    for tags, hip, content in zip(sets, hips, ["bd", "<thXnk>a</thXnk>bd"]):
        want = H.run_engine(_cpu(tags), streams, [True], [True], H.EveryRound())
        got = H.run_engine(hip, streams, [True], [True], H.EveryRound())
        assert got == want, tags
        assert got[0][0][1:] == (1, content) and got[2] == [content], (tags, got)
        st = _stats(hip)
        assert st["escalations"] == 0 and st["fin_host"] == 0 and st["fin_items"] >= 1, st


def test_class_tags_need_tick_lanes():
    """The loop-tick grid runs the literal tag sets' kernel: an engine with a class tag set on a
    door of it is refused (the server picks tick lanes for such a config); a literal tag set
    with the flag on is an ordinary engine."""
    ext = native.require()
    grid = ext.HipGrid(0, 2)
    try:
        with pytest.raises(ValueError, match="tick lanes"):
            NativeEngine("hip", ["think", "th.nk"], device=0, classes=True, grid=grid, door=0, **KW)
        NativeEngine("hip", ["think"], device=0, classes=True, grid=grid, door=0, **KW)
    finally:
        grid.stop()


def test_native_server_hip_class_tags(monkeypatch):
    """The native server on the HIP engine with ["think", "th.nk"] and verify mode: equal to
    the FastAPI app, every stream and final equal to the shadow CPU oracle."""
    import test_class_tags as TC
    import test_native_server as T

    ext = native.require()
    before = ext.server_counters()
    monkeypatch.setattr(T, "ENGINE", "hip")
    monkeypatch.setattr(T, "VERIFY", True)
    T._compare(TC.class_server_scenario(), "class_tags_hip", None)
    after = ext.server_counters()
    assert after["verify_mismatches"] == before["verify_mismatches"]
    assert after["verify_checked"] > before["verify_checked"]
