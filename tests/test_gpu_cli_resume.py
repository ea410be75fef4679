"""pt_cli --checkpoint / --resume / --pass-spp: a render continued from a checkpoint file, or built up in
passes, writes the same PFM as the one-shot run, byte for byte; an option that contradicts the resumed file
is an error."""
import os
import subprocess

import pytest

from conftest import MODELS, ROOT, SCENE_SETS

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
SIZE = ["--width", "24", "--height", "16", "--bounces", "3", "--radius", "0.05", "--quiet"]


def _obj_args(name):
    args = []
    for obj, origin, scale, flip in SCENE_SETS[name]:
        args += ["--obj", "%s@%r,%r,%r@%r@%d" % ((os.path.join(MODELS, obj),) + tuple(float(v) for v in origin) +
                                                  (float(scale), flip))]
    return args


def _run(args):
    return subprocess.run([CLI] + _obj_args("cornell_blob") + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def one_shot(tmp_path_factory):
    d = tmp_path_factory.mktemp("oneshot")
    pfm = str(d / "b.pfm")
    r = _run(SIZE + ["--spp", "9", "--out", str(d / "b.ppm"), "--pfm", pfm])
    assert r.returncode == 0, r.stderr
    return open(pfm, "rb").read(), open(str(d / "b.ppm"), "rb").read()


def test_resume_equals_one_shot(tmp_path, one_shot):
    f, a, ppm = str(tmp_path / "f.ptacc"), str(tmp_path / "a.pfm"), str(tmp_path / "a.ppm")
    r = _run(SIZE + ["--spp", "4", "--checkpoint", f, "--out", str(tmp_path / "first.ppm")])
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(f) == 128 + 24 * 16 * 48
    # every fixed parameter comes from the file (no --width / --bounces / --radius here)
    r = _run(["--quiet", "--resume", f, "--spp", "5", "--pfm", a, "--out", ppm])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == one_shot[0]
    assert open(ppm, "rb").read() == one_shot[1]
    # an option that contradicts the file is an error, not an override; one that agrees is fine
    r = _run(["--quiet", "--resume", f, "--spp", "5", "--bounces", "4", "--out", ppm])
    assert r.returncode == 2 and "--bounces contradicts" in r.stderr
    r = _run(["--quiet", "--resume", f, "--spp", "0", "--bounces", "3", "--out", ppm])
    assert r.returncode == 0, r.stderr


def test_pass_spp_equals_one_shot(tmp_path, one_shot):
    a, f = str(tmp_path / "a.pfm"), str(tmp_path / "f.ptacc")
    args = [x for x in SIZE if x != "--quiet"]
    r = _run(args + ["--spp", "9", "--pass-spp", "2", "--pfm", a, "--out", str(tmp_path / "a.ppm"), "--checkpoint", f])
    assert r.returncode == 0, r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("sample ")] == ["sample %d" % k for k in (2, 4, 6, 8, 9)]
    assert open(a, "rb").read() == one_shot[0]
    assert os.path.getsize(f) == 128 + 24 * 16 * 48
