"""The boundary cases (boundary_cases.py) on the C++ CPU engine vs the python oracle.

This is the check that every generated case is a valid input the reference handles, and that
the host code the kernels share (qmx_text.h, qmx_lex.h) is right on each edge: SSE bytes,
flags, texts and both finalize results, byte for byte.  No case is skipped; the number of
cases and streams per family is pinned, so a generator that silently produces fewer fails.
The limits themselves are pinned too: a retune is a conscious edit here.
"""
import pytest

from quorum_amd.ops import native
from quorum_amd.ops.native import NativeEngine

import boundary_cases as BC
import engine_harness as H

LIMITS = native.require().kernel_limits()
FAMILIES = BC.families(LIMITS)
CASES = [(fam, c) for fam in sorted(FAMILIES) for c in FAMILIES[fam]]

# cases / streams per family (with today's limits)
EXPECTED = {"A": (6, 103), "B": (31, 81), "C": (9, 546), "D": (12, 1261), "E": (19, 1291)}

oracle = H.oracle_result


def test_kernel_limits_pinned():
    """Today's thresholds of the tick kernel and the finalize items.  Changing one moves every
    sweep of boundary_cases.py with it; this list is the one place to edit by hand."""
    assert LIMITS == {
        "BS": 512, "kSpecTile": 8192, "TILE_MAX": 16384, "MAX_EV": 512, "MAX_CAND": 1024, "TOK_CAP": 512,
        "TPL_PRE_MAX": 256, "TPL_SUF_MAX": 64, "kHoleTplBytes": 448, "kHoleMax": 16, "kHoleWmaskBytes": 256,
        "kBackendTpl": 16, "kWindow": 16, "kMaxTags": 16, "kMaxTagLen": 61, "kMaxTail": 64,
        "FIN_WIN": 8192, "FIN_BIG": 256,
    }


def test_case_counts():
    got = {fam: (len(cs), sum(len(c.streams) for c in cs)) for fam, cs in FAMILIES.items()}
    assert got == EXPECTED
    names = [c.name for _, c in CASES]
    assert len(set(names)) == len(names)


assert_same = H.assert_same


@pytest.mark.parametrize("fam,case", CASES, ids=[c.name for _, c in CASES])
def test_cpu_engine_matches_oracle(fam, case):
    for strip in case.strips:
        want = oracle(case, strip)
        got = H.run_case(NativeEngine("cpu", case.tags), case, strip)
        assert_same(got, want, case, "cpu vs oracle")


def test_deep_nesting_hides_every_letter():
    """What the oracle says about the deep-nesting streams (so the case tests what it means
    to): nothing is emitted, no text is kept, at any depth past 32768 or 65536."""
    case = next(c for _, c in CASES if c.name == "C_deep_nesting")
    res, fin, texts = oracle(case, True)
    assert all(r == (b"", 1, "") for r in res[:-1]), [r[0][-80:] for r in res]
    assert res[-1][2] == "visible" and texts == ["visible"]  # (the one plain stream of the case)
