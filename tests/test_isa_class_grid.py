"""Machine-code checks of the class tag sets' persistent grid kernel (no GPU needed).

``qmx_ctick_persistent`` is the loop-tick grid's relay / claim / item loop around the class
items (``run_item<true>``), one workgroup per CU.  Like the literal kernel it must keep
everything in registers and LDS; its name must not be counted among the literal tick kernels
by ``tests/test_isa.py`` (which pins exactly three of them).
"""
import subprocess

from test_isa import LLVM, code_object, kernel_resources  # noqa: F401  (code_object: the fixture)


def _class_grid_kernels(code_object):
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(code_object)], check=True,
                           capture_output=True, text=True).stdout
    return {k: v for k, v in kernel_resources(notes).items() if "qmx_ctick_persistent" in k}


def test_class_grid_kernel_has_no_scratch(code_object):
    """Exactly one class grid kernel (there is no two-workgroups-per-CU variant), named so that
    the literal kernels' count stays three; no VGPR spill, no scratch beyond one saved register
    of a call, at most 256 VGPRs (one 512-thread workgroup per CU) and one CU's LDS."""
    ks = _class_grid_kernels(code_object)
    assert len(ks) == 1, sorted(ks)
    (name, r), = ks.items()
    assert "qmx_tick_persistent" not in name and "qmx_tick_kernel" not in name, name
    assert r.get("vgpr_spill_count", 0) == 0, (name, r)
    assert r.get("private_segment_fixed_size", 0) <= 16, (name, r)
    assert r["vgpr_count"] <= 256, (name, r)
    assert r.get("group_segment_fixed_size", 0) <= 160 * 1024, (name, r)


def test_class_grid_kernel_sgpr_spill_ceiling(code_object):
    """SGPR spills (to VGPR lanes, not memory) may not creep up unnoticed: 389 in the build
    this test came with (256 VGPRs, no scratch, 79424 B LDS); the ceiling is that plus under
    10 %, the margin tests/test_isa.py gives the literal kernel (364 -> 400)."""
    (name, r), = _class_grid_kernels(code_object).items()
    assert r.get("sgpr_spill_count", 0) <= 425, (name, r)
