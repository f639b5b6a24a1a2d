"""Code generation with the mesh lights in (DLight type 2: csrc/device_lib.h mesh_light_sample / mesh_light_at_hit), read from the gfx950
code object the library carries exactly as tests/test_codegen_guard.py reads it.  A scene with a mesh light sets DeviceScene::general,
so the mesh branch of eye_emitter_hit is compiled into the ENV = true forms of the eye megakernel only: the plain timed forms keep
their names and the instruction counts they were profiled with, and the general forms -- whose emitter hit now selects the hit
triangle's normal and label -- stay inside the occupancy limits of tests/test_codegen_guard.py (128 VGPRs, 176 B of scratch, the
instruction count within 6 % of the profiled one).  Needs no GPU."""
import pytest

from tests.test_codegen_guard import PROFILED_INSTRUCTIONS, TIMED, code_object  # noqa: F401  (the fixture: the library's code object, disassembled)


def test_plain_timed_forms_are_untouched(code_object):  # noqa: F811
    meta, disasm = code_object
    for form, name in TIMED.items():
        assert name in meta, (form, [k for k in meta if "k_spcbpt" in k])
        if "plain" in form:
            # the mesh branch is `if (ENV && L.type == 2)`: nothing of it in the ENV = false forms (exactly the profiled counts + the
            # handful of instructions they have moved by since; the parent commit's code, symbol by symbol: tools/codegen_diff_symbols.py)
            assert abs(disasm[name]["instructions"] - PROFILED_INSTRUCTIONS[name]) <= 0.01 * PROFILED_INSTRUCTIONS[name], (form, disasm[name]["instructions"])
            assert meta[name]["private_segment_fixed_size"] <= 160 and meta[name]["vgpr_count"] <= 128


@pytest.mark.parametrize("form", [f for f in TIMED if "general" in f])
def test_general_forms_hold_the_mesh_branch_inside_the_guard(code_object, form):  # noqa: F811
    meta, disasm = code_object
    name = TIMED[form]
    m, d = meta[name], disasm[name]
    report = dict(m, **d)
    assert m["vgpr_count"] <= 128 and m["group_segment_fixed_size"] <= 40960 and m["private_segment_fixed_size"] <= 176, report
    assert abs(d["instructions"] - PROFILED_INSTRUCTIONS[name]) <= 0.06 * PROFILED_INSTRUCTIONS[name], report
    loops = d["traversal_loops"]
    assert loops and loops[0][1] == 0, report            # nothing spilled inside the traversal loop


def test_pt_with_the_mesh_branches_keeps_its_occupancy(code_object):  # noqa: F811
    """"pt" samples a mesh light at every vertex (one guide entry and one window of eight CMF values, not a chain of dependent probes)
    and dispatches on the light's type at an emitter hit: still no scratch, still under 112 VGPRs (88 / 100 before and after)."""
    meta, _ = code_object
    pt = {k: m for k, m in meta.items() if "k_ptIL" in k}
    assert len(pt) == 2, list(meta)
    for k, m in pt.items():
        assert m["vgpr_count"] <= 112 and m["private_segment_fixed_size"] == 0, (k, m)
