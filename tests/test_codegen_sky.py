"""Code generation of the eye megakernel forms whose escaped eye paths see the sky (k_spcbpt_sky<BATCH>: spcbpt_set_environment_mode,
SPCBPT_ENV_EYE_SEES_SKY), read from the gfx950 code object the library carries exactly as tests/test_codegen_guard.py reads it.
They run on the persistent grid sized for the timed forms, so they must keep that occupancy: 128 VGPRs (4 waves per SIMD), at most
40 960 B of LDS (4 blocks per CU), at most the 176 B of scratch of the general timed forms, and nothing spilled inside the traversal
loop.  The four timed k_spcbpt forms keep their names (the sky forms are kernels of their own).  Needs no GPU."""
import pytest

from tests.test_codegen_guard import TIMED, code_object  # noqa: F401  (the fixture: the library's code object, disassembled)

SKY = {"single frame": "_ZN3spc12k_spcbpt_skyILb0EEEvNS_7KParamsE", "batched": "_ZN3spc12k_spcbpt_skyILb1EEEvNS_7KParamsE"}


@pytest.mark.parametrize("form", list(SKY))
def test_sky_megakernel_resources(code_object, form):  # noqa: F811
    meta, disasm = code_object
    name = SKY[form]
    assert name in meta, (form, [k for k in meta if "k_spcbpt" in k])
    m, d = meta[name], disasm[name]
    report = dict(m, **d)
    assert m["vgpr_count"] <= 128, report
    assert m["group_segment_fixed_size"] <= 40960, report
    assert m["private_segment_fixed_size"] <= 176, report
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
