"""tools/spcbpt_render --batch N: the uniform frames in groups of up to N through spcbpt_launch_light_batch,
spcbpt_build_sampler_batch and spcbpt_launch_eye_batch_film.  The files it writes and the error it prints must be those of the same
command without --batch, bit for bit; what has no batched form is refused with the reason."""
import os
import re
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


def _run(tool, path, root, out, extra):
    cmd = [tool, path, root, "--alg", "SPCBPT_eye", "--minimal", "--dim=72x40", "--frames", "6", "--out", out] + extra
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def test_batched_run_writes_the_per_frame_runs_bytes(tool, pkg, tmp_path):
    root = str(tmp_path)
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), root, "cornell")
    common = ["--target-error", "1e-9", "--robust", "5"]
    outs, reached = [], []
    for name, extra in (("plain", []), ("batched", ["--batch", "4"])):
        out = os.path.join(root, name)
        p = _run(tool, path, root, out, common + extra)
        assert p.returncode == 0, p.stdout[-3000:]
        m = re.search(r"(\d+) frames used, error reached (\S+) \(max (\S+) over (\d+) pixels\)", p.stdout)
        assert m, p.stdout[-3000:]
        assert int(m.group(1)) == 6 and int(m.group(4)) == 72 * 40
        reached.append(m.groups())
        outs.append(out)
    assert reached[0] == reached[1], reached
    assert float(reached[0][1]) > 0.0
    for suffix in (".pfm", ".ppm", "_robust.pfm", "_robust.ppm"):
        a, b = (open(o + suffix, "rb").read() for o in outs)
        assert len(a) > 72 * 40 * 3 and a == b, suffix


def test_batch_refuses_what_has_no_batched_form(tool, pkg, tmp_path):
    root = str(tmp_path)
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), root, "cornell")
    p = _run(tool, path, root, os.path.join(root, "no"), ["--batch", "4", "--features"])
    assert p.returncode != 0
    assert "--batch: not with --features: its per-frame launches have no batched form" in p.stdout, p.stdout[-2000:]
    assert not os.path.exists(os.path.join(root, "no.pfm"))
