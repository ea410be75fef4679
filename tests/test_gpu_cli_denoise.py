"""pt_cli --denoise / --aov: the command-line tool's filtered PFM equals Renderer.denoise of Renderer.render, its
AOV files equal Renderer.features, and --denoise also applies to a resumed render."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, SCENE_SETS, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H = 24, 16
SIZE = ["--width", str(W), "--height", str(H), "--bounces", "3", "--quiet"]


def _run(args):
    objs = []
    for obj, origin, scale, flip in SCENE_SETS["cornell_blob"]:
        objs += ["--obj", "%s@%r,%r,%r@%r@%d" % ((os.path.join(MODELS, obj),) + tuple(float(v) for v in origin) +
                                                  (float(scale), flip))]
    return subprocess.run([CLI] + objs + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def api_side():
    cam = pt.make_camera(width=W, height=H, **scenes.CORNELL_CAMERA)
    with pt.Renderer(load_scene("cornell_blob"), 0) as r:
        feat = r.features(cam, W, H)
        img4 = r.render(cam, W, H, 4, bounces=3, seed=1234)[0]
        img9 = r.render(cam, W, H, 9, bounces=3, seed=1234)[0]
        return feat, r.denoise(img4, feat), r.denoise(img4, feat, iterations=2), r.denoise(img9, feat)


def test_denoise_and_aov_equal_the_api(tmp_path, api_side):
    feat, den4, den4_2, _ = api_side
    pfm, aov = str(tmp_path / "a.pfm"), str(tmp_path / "aov")
    r = _run(SIZE + ["--spp", "4", "--denoise", "--aov", aov, "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(pfm).tobytes() == den4.tobytes()
    for name in ("albedo", "normal", "position"):
        assert pt.read_pfm("%s_%s.pfm" % (aov, name)).tobytes() == np.ascontiguousarray(feat[name]).tobytes()
    depth = pt.read_pfm(aov + "_depth.pfm")
    assert depth.tobytes() == np.repeat(feat["depth"][..., None], 3, axis=2).tobytes()
    r = _run(SIZE + ["--spp", "4", "--denoise", "2", "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(pfm).tobytes() == den4_2.tobytes()
    r = _run(["--help"])
    assert "--denoise" in r.stderr and "--aov" in r.stderr


def test_resume_then_denoise(tmp_path, api_side):
    den9 = api_side[3]
    f, pfm = str(tmp_path / "f.ptacc"), str(tmp_path / "a.pfm")
    r = _run(SIZE + ["--spp", "4", "--checkpoint", f, "--out", str(tmp_path / "first.ppm")])
    assert r.returncode == 0, r.stderr
    r = _run(["--quiet", "--resume", f, "--spp", "5", "--pass-spp", "2", "--denoise", "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(pfm).tobytes() == den9.tobytes()
