"""GPU tests: the HIP engine on the boundary cases (boundary_cases.py) vs the python oracle.

The reference is ``PyEngine`` over ``ops/reference.py`` — not the C++ CPU engine, which shares
qmx_text.h / qmx_lex.h with the kernels.  Every comparison is byte-exact (SSE bytes, flags,
texts, both finalize results).  The CPU engine's result is compared as well, so a failure says
at once whether HIP alone is wrong or HIP and CPU together.  Per case the counters of
``kernel_stats()`` show that the path under test ran: the designed number of escalations (0, or
1 for the ``+1`` cases), no finalize on the host, the tiles cut at MAX_EV events.

Kernel limits and the tests that sit on them (limit -> family / case -> test):

  kSpecTile, TILE_MAX, 16-byte vectors      A_feed_len, A_sep_at_tile_end_*   test_hip_matches_oracle
  s2_wave: in_len - start 4096, start & 7   A_first_frame                      test_hip_matches_oracle
  64 events per tile (one wave)             A_events_64                        test_hip_matches_oracle
  MAX_EV (WS_MORE, eof with MAX_EV events)  A_max_ev                           test_hip_matches_oracle (requeues)
  TPL_PRE_MAX, TPL_SUF_MAX                  B_tpl_pre_*, B_tpl_suf_*           test_template_admission
  kHoleTplBytes                             B_hole_len_*                       test_hole_template_admission
  kHoleMax                                  B_hole_count_*                     test_hole_count_admission
  kBackendTpl                               B_backend_index_*                  test_backend_table_entry
  S3a prepass: events of 256 bytes (wmask)  B_s3a_len_*, B_hole_offset         test_s3a_event_length
  TOK_CAP                                   B_tok_cap                          test_hip_matches_oracle (no host-side counter
                                                                               tells the lexer's fallback from its walk)
  candidates 0-65, MAX_CAND (+1 escalates)  C_cand_counts, C_cand_over         test_hip_matches_oracle
  Zn 2048, ndelta 64 (s4_wave, lane-0 tail) C_routes                           test_hip_matches_oracle
  npat 16 / 18 / 32 (MFMA column blocks)    C_tags_8 / _9 / _16                test_hip_matches_oracle
  16-byte window, kMaxTagLen                C_long_tags                        test_hip_matches_oracle
  kMaxTail (holdback), pattern words        C_holdback_cuts                    test_hip_matches_oracle
  16-bit tok_dep                            C_deep_nesting                     test_hip_matches_oracle
  content_cap, out_cap                      D_content_cap, D_out_cap_near_*    test_hip_matches_oracle
  16 KiB output window, clean / general     D_window_*, D_clean_vs_general     test_hip_matches_oracle
  escape classes, UTF-8 lengths             D_escape_edges                     test_hip_matches_oracle
  Wlen 2048, ndelta 64 (s6 sizing wave)     D_sizing_wave                      test_hip_matches_oracle
  FIN_WIN, 64 tokens per ballot step        E_win_*, E_windows_tokens          test_hip_matches_oracle
  FIN_BIG, BS segments per pass, seg_cap    E_segments                         test_hip_matches_oracle
  str.strip() code points                   E_strip_edges                      test_hip_matches_oracle
  K5 chunks, 16-byte stores, joiners        E_k5_*, E_joiner_*, E_texts_per_request   test_hip_matches_oracle

Families A, C and D run again through the one-shot kernel entry (QMX_PERSISTENT=0) and with
every one-wave fast path off (QMX_KFAST=0), so the block paths see the same edges.
"""
import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import boundary_cases as BC
import engine_harness as H

pytestmark = pytest.mark.gpu

LIMITS = native.require().kernel_limits()
FAMILIES = BC.families(LIMITS)
CASES = [c for fam in sorted(FAMILIES) for c in FAMILIES[fam]]
ACD = [c for fam in "ACD" for c in FAMILIES[fam]]

_cpu = {}


@pytest.fixture(scope="module")
def ext():
    e = native.require()
    assert e.device_count() > 0, "no GPU visible"
    return e


def cpu_result(case, strip):
    key = (case.name, strip)
    if key not in _cpu:
        _cpu[key] = H.run_case(NativeEngine("cpu", case.tags), case, strip)
    return _cpu[key]


def run_hip(case):
    """The case on a fresh HIP engine, every strip value: == the oracle, == the CPU engine,
    and the engine did the work itself.  Returns the last engine's counters."""
    st = None
    for strip in case.strips:
        eng = NativeEngine("hip", case.tags, device=0, **(case.kw or {}))
        got = H.run_case(eng, case, strip)
        st = eng._e.kernel_stats()
        print(case.name, strip, {k: st[k] for k in ("escalations", "requeues", "fin_host", "fin_items", "launches", "items")})
        H.assert_same(got, H.oracle_result(case, strip), case, "hip vs oracle")
        H.assert_same(got, cpu_result(case, strip), case, "hip vs cpu")
        assert st["escalations"] == case.escalations, st
        if case.escalations == 0:  # (a session with a stream on the host path is finalized there, by design)
            assert st["fin_host"] == 0, st
            assert st["fin_items"] >= 2 * len(case.groups or [0]), st
        if case.requeues is not None:
            assert st["requeues"] == case.requeues, st
    return st


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hip_matches_oracle(ext, case):
    run_hip(case)


@pytest.mark.parametrize("case", ACD, ids=[c.name for c in ACD])
def test_hip_one_shot_matches_oracle(ext, monkeypatch, case):
    monkeypatch.setenv("QMX_PERSISTENT", "0")
    run_hip(case)


@pytest.mark.parametrize("case", ACD, ids=[c.name for c in ACD])
def test_hip_fast_paths_off_matches_oracle(ext, monkeypatch, case):
    monkeypatch.setenv("QMX_KFAST", "0")
    run_hip(case)


def _s3(case, monkeypatch):
    monkeypatch.setenv("QMX_STAGE_TIMING", "1")  # per-item S3 counters
    st = run_hip(case)
    print(case.name, {k: st[k] for k in ("s3_events", "s3_template_hits", "s3_hole_hits", "s3_full_parses")})
    return st


def test_template_admission(ext, monkeypatch):
    """A per-stream template is published for a prefix of up to TPL_PRE_MAX bytes and a suffix
    of up to TPL_SUF_MAX: later events of that shape then hit it; one byte more and no event
    of the stream ever does."""
    for lim, cases in ((LIMITS["TPL_PRE_MAX"], BC.tpl_pre_cases(LIMITS)), (LIMITS["TPL_SUF_MAX"], BC.tpl_suf_cases(LIMITS))):
        for n, case in cases:
            st = _s3(case, monkeypatch)
            if n <= lim:
                # at least the two repeats of the warm event and the first content-only event
                assert st["s3_template_hits"] >= 3, (case.name, st)
            else:
                assert st["s3_template_hits"] == 0, (case.name, st)


def test_hole_template_admission(ext, monkeypatch):
    """An event of up to kHoleTplBytes bytes is published as a hole template, and the second
    stream's events of that shape hit it; one byte more and every event is parsed in full.
    (The content string starts past TPL_PRE_MAX: no per-stream template in either case.)"""
    for n, case in BC.hole_len_cases(LIMITS):
        st = _s3(case, monkeypatch)
        assert st["s3_template_hits"] == 0, (case.name, st)
        if n <= LIMITS["kHoleTplBytes"]:
            assert st["s3_hole_hits"] >= 4, (case.name, st)  # the second stream's content events
        else:
            # the 8 content events at least (role and finish events have other lengths; a
            # [DONE] event needs no parse)
            assert st["s3_full_parses"] >= 8, (case.name, st)


def test_hole_count_admission(ext, monkeypatch):
    """An event with up to kHoleMax holes is published as a hole template, and the later events
    of its shape — the second stream's four at least — hit it; with one hole more nothing is
    published and every content event is parsed in full.  (No per-stream template either way:
    the digits before the content string differ from event to event.)"""
    for nh, case in BC.hole_count_cases(LIMITS):
        st = _s3(case, monkeypatch)
        assert st["s3_template_hits"] == 0, (case.name, st)
        if nh <= LIMITS["kHoleMax"]:
            assert st["s3_hole_hits"] >= 4, (case.name, st)
        else:
            assert st["s3_hole_hits"] == 0 and st["s3_full_parses"] >= 8, (case.name, st)


def test_backend_table_entry(ext, monkeypatch):
    """Backend indices below kBackendTpl have a template table entry: the second stream's role
    and finish events at least (never a per-stream template's) hit the first one's hole
    templates.  Index kBackendTpl and above have none: no hole hit at all."""
    for idx, case in BC.backend_index_cases(LIMITS):
        st = _s3(case, monkeypatch)
        if idx < LIMITS["kBackendTpl"]:
            assert st["s3_hole_hits"] >= 2, (case.name, st)
        else:
            assert st["s3_hole_hits"] == 0, (case.name, st)


def test_s3a_event_length(ext, monkeypatch):
    """The S3a prepass resolves events of up to 256 bytes (32 lanes x 8 bytes, a hole
    template's word masks).  Of the 14 events of a case, seven content events have a template
    of their length by their tick (the first stream's 2nd-4th, the second stream's four): at
    most 7 are left to the S3 loop.  One byte more and all 8 content events are."""
    for n, case in BC.s3a_len_cases(LIMITS):
        st = _s3(case, monkeypatch)
        print(case.name, "s3a_unresolved", st["s3a_unresolved"])
        if n <= LIMITS["kHoleWmaskBytes"]:
            assert st["s3a_unresolved"] <= 7, (case.name, st)
        else:
            assert st["s3a_unresolved"] >= 8, (case.name, st)
