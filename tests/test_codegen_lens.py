"""Code generation of the thin-lens forms of the eye megakernel (k_spcbpt_lens<ENV>: spcbpt_set_lens with a radius > 0), read from the
gfx950 code object the library carries exactly as tests/test_codegen_guard.py reads it.  They run on a persistent grid sized like the
timed forms', so they must keep that occupancy: 128 VGPRs (4 waves per SIMD), at most 40 960 B of LDS (4 blocks per CU), nothing
spilled inside the traversal loop or the quad tail's.  Scratch: the lens form alone carries the camera position -- a lens point per
lane -- in registers across the traversal pass (csrc/eye_kernel_body.h), three floats, which the allocator rounds up to 16 B; the bar is
the SAME build's figure for the matching timed single-frame form plus those 16 B.  Measured: 144 B for both forms next to 128 B for
both timed ones.  The four timed k_spcbpt forms keep their names (the lens forms are kernels of their own).
Needs no GPU."""
import pytest

from tests.test_codegen_guard import TIMED, code_object  # noqa: F401  (the fixture: the library's code object, disassembled)

LENS = {"plain scene": ("_ZN3spc13k_spcbpt_lensILb0EEEvNS_7KParamsE", "single frame, plain scene"),
        "general scene": ("_ZN3spc13k_spcbpt_lensILb1EEEvNS_7KParamsE", "single frame, general scene")}


@pytest.mark.parametrize("form", list(LENS))
def test_lens_megakernel_resources(code_object, form):  # noqa: F811
    meta, disasm = code_object
    name, timed = LENS[form]
    assert name in meta, (form, [k for k in meta if "k_spcbpt" in k])
    m, d = meta[name], disasm[name]
    base = meta[TIMED[timed]]
    report = dict(m, **d)
    print(f"k_spcbpt_lens, {form}: {m['vgpr_count']} VGPRs, {m['private_segment_fixed_size']} B of scratch (timed form: {base['private_segment_fixed_size']} B), "
          f"{m['group_segment_fixed_size']} B of LDS, {d['instructions']} instructions (timed form: {disasm[TIMED[timed]]['instructions']})")
    assert m["vgpr_count"] <= 128, report
    assert m["group_segment_fixed_size"] <= 40960, report
    assert m["private_segment_fixed_size"] <= base["private_segment_fixed_size"] + 16, (report, base)
    loops = d["traversal_loops"]
    assert loops, report
    size, stores, loads = loops[0]
    assert stores == 0 and loads <= 6, report
    assert 1000 <= size <= 1500, report                  # the same pooled step as the timed forms'
    tail = d["quad_tail_loop"]
    assert tail and tail[0][1] == 0, report


def test_timed_megakernels_keep_their_names(code_object):  # noqa: F811
    meta, _ = code_object
    missing = [form for form, name in TIMED.items() if name not in meta]
    assert not missing, (missing, [k for k in meta if "k_spcbpt" in k])
