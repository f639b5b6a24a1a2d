"""tools/spcbpt_render --guides [N]: beside --denoise / --features a reflected-guide launch per frame, the denoiser switched to those
planes, and the planes written as <out>_guide_albedo.pfm / _guide_normal_depth.pfm / _guide_depth.pfm.  Without the flag every output
file keeps its bytes; with it the film and the first-hit files still do, and only the denoised image moves."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "spcbpt_render")


@pytest.fixture(scope="module")
def tool(gpu):
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return TOOL


def test_guides_flag(tool, pkg, tmp_path):
    root = str(tmp_path)
    path = pkg.scenes.write_scene(pkg.scenes.mirror_box(), root, "mirror_box")
    outs = {}
    for name, extra in (("plain", []), ("guides", ["--guides"]), ("guides0", ["--guides", "0"])):
        out = os.path.join(root, name)
        cmd = [tool, path, root, "--alg", "pt", "--dim=72x40", "--frames", "4", "--denoise", "--features", "--out", out] + extra
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        outs[name] = out
    read = lambda name, suffix: open(outs[name] + suffix, "rb").read()
    for suffix in (".pfm", ".ppm", "_albedo.pfm", "_normal.pfm", "_depth.pfm"):
        assert read("plain", suffix) == read("guides", suffix) == read("guides0", suffix), suffix
    assert not os.path.exists(outs["plain"] + "_guide_albedo.pfm")
    for suffix in ("_guide_albedo.pfm", "_guide_normal_depth.pfm", "_guide_depth.pfm"):
        assert len(read("guides", suffix)) > 72 * 40 * 12
    assert read("guides", "_guide_albedo.pfm") != read("guides", "_albedo.pfm")             # the mirrors show what they reflect
    assert read("guides", "_denoised.pfm") != read("plain", "_denoised.pfm")
    # no mirror followed: the first-hit planes, and the denoised image they give
    assert read("guides0", "_guide_albedo.pfm") == read("plain", "_albedo.pfm")
    assert read("guides0", "_guide_normal_depth.pfm") == read("plain", "_normal.pfm")
    assert read("guides0", "_denoised.pfm") == read("plain", "_denoised.pfm")
