"""Runs of any length in repeated thinking tags on the GPU (``runs=True``, ``runtime.native_run_tags``,
with ``classes``, ``variants``, ``extended`` and ``repeat``): the key, and the kernels' rule on the host.

The key changes nothing the host computes: the rows, the kind and the host engines' bytes are those of
``repeat`` alone.  It sets one bit of the device tables (``kVarRuns``), with which the kernels' candidate
walk takes a run of ASCII copies past an open-ended row with a cursor of its own.  That rule is
host-compilable (``qmx_text.h`` ``device_token_at``): ``class_candidates`` lists what it decides at every
'<', ``class_suspects`` counts what it leaves to the host, ``class_matches`` is the exact walk.
"""
import itertools
import random
import subprocess

import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import engine_harness as H
import repeat_tag_cases as X

KW = dict(X.KW, runs=True)
MIXED_KW = dict(X.MIXED_KW, runs=True)
HOST_KW = {k: v for k, v in KW.items() if k != "classes"}  # (class_suspects and its kin take no `classes`)
KEYS = {"native_regex_tags": True, "native_variant_tags": True, "native_extended_tags": True,
        "native_repeat_tags": True, "native_run_tags": True}


def _host_kw(kw):
    return {k: v for k, v in kw.items() if k != "classes"}


# ---------------------------------------------------------------- 1: the key
def test_runtime_config_key():
    from quorum_amd.utils.config import RuntimeConfig

    assert RuntimeConfig.from_config({}).native_run_tags is False
    assert RuntimeConfig.from_config({"runtime": {k: v for k, v in KEYS.items() if k != "native_run_tags"}}).native_run_tags is False
    assert RuntimeConfig.from_config({"runtime": KEYS}).native_run_tags is True
    with pytest.raises(ValueError, match="native_run_tags must be true or false"):
        RuntimeConfig.from_config({"runtime": dict(KEYS, native_run_tags="yes")})
    for missing in ("native_regex_tags", "native_variant_tags", "native_extended_tags", "native_repeat_tags"):
        rt = {k: v for k, v in KEYS.items() if k != missing}
        with pytest.raises(ValueError) as e:
            RuntimeConfig.from_config({"runtime": rt})
        if missing == "native_repeat_tags":
            assert str(e.value) == ("runtime.native_run_tags needs runtime.native_regex_tags, runtime.native_variant_tags, "
                                    "runtime.native_extended_tags and runtime.native_repeat_tags all true")


def test_native_config_and_make_engine_carry_the_key():
    from quorum_amd.ops.engine import make_engine
    from quorum_amd.runtime.native_server import native_config

    import test_repeat_tags as TR

    cfg = TR.repeat_server_scenario()[0]
    assert native_config(cfg, "127.0.0.1", 1, "cpu", 0, 1)["tag_runs"] is False
    d = native_config(dict(cfg, runtime=dict(KEYS)), "127.0.0.1", 1, "cpu", 0, 1)
    assert d["tag_runs"] is True and d["tag_repeat"] is True
    tags = ["Think", "step\\d+"]
    eng = make_engine("cpu", tags, **KW)
    assert isinstance(eng, NativeEngine) and eng.runs and eng.repeat
    assert make_engine("cpu", tags, **KW) is eng and make_engine("cpu", tags, **X.KW) is not eng
    assert not make_engine("cpu", tags, **X.KW).runs
    # without `repeat` the key is nothing: the tag needs the python engine, as before
    assert not isinstance(make_engine("cpu", tags, **dict(X.OFF_KW, runs=True)), NativeEngine)


def test_rows_kind_and_host_bytes_do_not_depend_on_the_key():
    for tag, rows, _alphabet in X.ACCEPTED:
        assert [r for r, _ in native.tagset_rows([tag], **KW)] == rows == [r for r, _ in native.tagset_rows([tag], **X.KW)]
    for k, (tags, kw, stems, run) in enumerate(X.DIFF_SETS):
        on = dict(kw, runs=True)
        assert native.tagset_ok(tags, **on)
        assert native.tagset_kind(tags, **on) == native.tagset_kind(tags, **kw)
        assert native.tagset_rows(tags, **on) == native.tagset_rows(tags, **kw)
        strip_on, strip_off = native.strip_fn(tags, **on), native.strip_fn(tags, **kw)
        rng = random.Random(k)
        raw = []
        for _ in range(4):
            texts = [X.diff_text(rng, rng.randint(0, 6), stems, run) for _ in range(rng.randint(1, 10))]
            assert all(strip_on(t, True) == strip_off(t, True) for t in texts)
            raw.append(b"".join(H.event_bytes(rng, t) for t in texts) + b"data: [DONE]\n\n")
        streams = [H.split_random(rng, r, rng.choice([3, 17, 64])) for r in raw]
        filt = [True, True, False, True]
        off = H.run_engine(NativeEngine("cpu", tags, **kw), streams, filt, [True] * 4, random.Random(k))
        assert H.run_engine(NativeEngine("cpu", tags, **on), streams, filt, [True] * 4, random.Random(k)) == off, tags
    # with the key off, and for a set without an open-ended row, the kernels' rule is what it was
    for tags, text in ((["think", "step\\d+"], b"<step12345>x</step123456>"), (["think\\s*"], b"<think     >")):
        for strip in (False, True):
            assert native.class_suspects(tags, text, strip=strip, **_host_kw(X.KW)) == text.count(b"<")
            assert native.class_suspects(tags, text, strip=strip, **HOST_KW) == 0
    off = dict(variants=True, extended=True)
    for text in (b"<step1>x</step2>", "<step٣>".encode(), b"<step<>"):
        assert (native.class_candidates(["step\\d"], text, runs=True, repeat=True, **off)
                == native.class_candidates(["step\\d"], text, **off))


# ---------------------------------------------------------------- 2: the rule against the exact walk
@pytest.mark.parametrize("tag,_rows,alphabet", X.ACCEPTED)
def test_the_rule_is_the_exact_walk_wherever_it_answers(tag, _rows, alphabet):
    """Every string s of up to 7 characters of the tag's six and '<', '>', '/', as "<s>x</s>": at every
    '<' the kernels' rule is suspect or answers the exact walk's token and byte length, with the
    streaming and with the strip tables.  (Enumerated inside the extension: 5.4 million strings.)"""
    assert len(set(alphabet)) == 6 and not set(alphabet) & set("<>/")
    alpha = (alphabet + "<>/").encode()
    for strip in (False, True):
        got = native.class_rule_sweep([tag], alpha, 7, strip=strip, **HOST_KW)
        assert got["texts"] == sum(9 ** n for n in range(8))
        assert got["mismatched"] == 0, (tag, strip, got["mismatches"])
        assert got["candidates"] > 2 * got["texts"] and got["suspects"] < got["candidates"]
        # (where the stem is short a name of 7 characters has a run longer than its rows: the cursor moved)
        if tag in ("hm+", "s\\d+", "a{2,}b", "x[ab]*y?", "n[^0-9x]+x", "a{0,}b"):
            assert got["beyond_rows"] > 0, (tag, got)
    # the same through the two list bindings, for the short strings
    for n in range(5):
        for s in map("".join, itertools.product(alphabet[:3] + alphabet[-1] + "<>/", repeat=n)):
            text = ("<%s>x</%s>" % (s, s)).encode()
            for strip in (False, True):
                rule = native.class_candidates([tag], text, strip=strip, **HOST_KW)
                exact = native.class_matches([tag], text, strip=strip, **HOST_KW)
                assert [p for p, _, _ in rule] == [p for p, _, _ in exact] == [i for i, c in enumerate(text) if c == 60]
                assert all(r[1] is None or r == e for r, e in zip(rule, exact)), (tag, text, rule, exact)


def test_long_runs_and_two_open_ended_positions():
    cand = lambda tags, text, **kw: native.class_candidates(tags, text.encode(), **dict(HOST_KW, **kw))  # noqa: E731
    # (["think", "step\d+"]: row 0 is think, rows 1-4 are step\d{4,}, step\d{3}, step\d{2}, step\d)
    tags = ["think", "step\\d+"]
    assert cand(tags, "<step12345>x</STEP123456789012>") == [(0, 2, 11), (12, -2, 19)]
    assert cand(tags, "<step1234>x</step12>") == [(0, 2, 10), (11, -4, 9)]
    assert cand(tags, "<step12345") == [(0, 0, 0)] and cand(tags, "<step12345x>") == [(0, 0, 0)]
    assert cand(tags, "<step12٣45>") == [(0, None, 0)] and cand(tags, "<step12345٣>") == [(0, None, 0)]
    assert cand(["v\\d+\\.\\d+"], "<v12345.678901>") == [(0, 1, 15)]
    assert cand(["v\\d+\\.\\d+"], "<v12345.>x<v12345x6>") == [(0, 0, 0), (10, 0, 0)]
    assert cand(["a\\d+[a-z]+"], "<A123456ABCDEFG>") == [(0, 1, 16)]
    assert cand(["think\\s*"], "<think      \n  >") == [(0, 1, 16)]
    assert cand(["think\\s*"], "<think  .  >") == [(0, 0, 0)]       # the streaming dot... a '.' is no space
    assert cand(["思\\d+"], "<思123456>x</思123456>", unicode=True, mixed=True) == [(0, 1, 11), (12, -1, 12)]


# ---------------------------------------------------------------- 3: no suspect candidate for ASCII runs
SUSPECT_SETS = [  # (tags, stems, what a run is made of, a stem whose run is of a class with a shorthand, its non-ASCII member)
    (["think", "step\\d+"], ["step", "think", "STEP", "Step", "ste"], "0123456789", "step", X.D3),
    (["think\\s*"], ["think", "THINK", "thin"], " \n\t", "think", "\u00a0"),
    (["hm+", "h\\d+"], ["h", "H", "hm", "HM"], "mM0123456789", "h", X.D3),
    (["v\\d+\\.\\d+"], ["v", "V", "v1.", "v12345."], "0123456789.", "v", X.D3),
]


def _ascii_text(rng, stems, run):
    out = []
    for _ in range(rng.randint(1, 16)):
        r = rng.random()
        name = rng.choice(stems) + "".join(rng.choice(run) for _ in range(rng.randint(0, 14)))
        if r < 0.45:
            out.append(rng.choice(["<", "</"]) + name + ">")
        elif r < 0.6:
            out.append(rng.choice(["<", "</"]) + name)
        elif r < 0.85:
            out.append(rng.choice(["<", ">", "/", "</", ">>", "<<"]))
        else:
            out.append("".join(rng.choice("".join(stems) + run) for _ in range(rng.randint(1, 6))))
    return "".join(out)


@pytest.mark.parametrize("k", range(len(SUSPECT_SETS)))
def test_no_suspect_candidate_for_ascii_runs(k):
    tags, stems, run, stem, wide = SUSPECT_SETS[k]
    suspects = lambda text, **kw: native.class_suspects(tags, text.encode(), **dict(HOST_KW, **kw))  # noqa: E731
    beyond = 0
    for seed in range(300):
        rng = random.Random(100 * k + seed)
        text = _ascii_text(rng, stems, run)
        assert text.isascii()
        assert suspects(text) == 0 == suspects(text, strip=True), text
        for strip in (False, True):  # (every candidate decided: as the exact walk, whatever the run's length)
            assert (native.class_candidates(tags, text.encode(), strip=strip, **HOST_KW)
                    == native.class_matches(tags, text.encode(), strip=strip, **HOST_KW)), text
        beyond += native.class_suspects(tags, text.encode(), **_host_kw(X.KW)) > 0
        # one non-ASCII member of the shorthand inside a run, within the rows or beyond them
        digits = "".join(rng.choice(run[-3:] if k == 2 else run.replace(".", "")) for _ in range(rng.randint(1, 9)))
        cut = rng.randint(0, len(digits))
        dirty = text + "<" + stem + digits[:cut] + wide + digits[cut:] + (".5>" if stem == "v" else ">")
        assert suspects(dirty) >= 1 and suspects(dirty, strip=True) >= 1, dirty
    assert beyond > 100  # (without the key, most of these texts leave the GPU)


def test_an_accepted_delimiter_in_a_run_is_suspect():
    tags = ["n[^0-9x]+x"]
    for strip in (False, True):
        assert native.class_suspects(tags, b"<n<x>", strip=strip, **HOST_KW) == 1
        assert native.class_suspects(tags, b"<nab<cdx>", strip=strip, **HOST_KW) == 1
        assert native.class_suspects(tags, b"<nabcde>fx>", strip=strip, **HOST_KW) == 1
        assert native.class_suspects(tags, b"<nabcdefx>x</NABCDEFX>", strip=strip, **HOST_KW) == 0
    assert native.class_candidates(tags, b"<nabcdefx>", **HOST_KW) == [(0, 1, 10)]


# ---------------------------------------------------------------- 4: the length bound
def test_a_match_is_at_most_61_bytes_on_the_host_mirror():
    tags = ["think", "step\\d+"]
    fits, over = "step" + "7" * 57, "step" + "7" * 58
    for strip in (False, True):
        for pre, sign in (("<", 1), ("</", -1)):
            text = (pre + fits + ">").encode()
            assert native.class_candidates(tags, text, strip=strip, **HOST_KW) == [(0, 2 * sign, len(text))]
            assert native.class_matches(tags, text, strip=strip, **HOST_KW) == [(0, 2 * sign, len(text))]
            text = (pre + over + ">").encode()
            assert native.class_candidates(tags, text, strip=strip, **HOST_KW) == [(0, 0, 0)]
            assert native.class_matches(tags, text, strip=strip, **HOST_KW) == [(0, 0, 0)]
    # a follower after the run counts too
    for name, tag in (("v" + "1" * 58 + ".5", True), ("v" + "1" * 58 + ".55", False), ("v1." + "5" * 59, False)):
        text = ("<%s>" % name).encode()
        want = [(0, 4, len(text))] if tag else [(0, 0, 0)]  # (row 3: v\\d\\d\\d\\d+\\.\\d)
        assert native.class_candidates(["v\\d+\\.\\d+"], text, **HOST_KW) == want == native.class_matches(["v\\d+\\.\\d+"], text, **HOST_KW)


# ---------------------------------------------------------------- 5: the stand-alone fuzz program
def test_fuzz_host_with_runs():
    """tools/csrc/fuzz_host.cpp as the stand-alone program it is (its own main, host code only, built
    with ASan and UBSan as tests/test_sanitizers.py builds it): the sets with unbounded repetition run a
    second time with ``runs``, where the kernels' rule must be the exact walk wherever it answers and
    the host engines' bytes must not change."""
    import os

    from quorum_amd.ops import build as B

    exe = {p.name: p for p in B.build_sanitized()}["qmx_fuzz_asan"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "600", "11"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and '"failures": 0' in r.stdout, (r.stdout, r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
