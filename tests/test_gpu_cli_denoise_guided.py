"""pt_cli --denoise-guided / --variance-map: the command-line tool's filtered PFM equals Renderer.denoise_guided of the
accumulator's image with NoiseEstimate.variance(), the variance map round-trips through read_pfm, and --denoise-guided
without an estimator is a usage error."""
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
# a tolerance nothing meets: the run ends at the cap, after 3 passes of 4
LOOP = ["--spp", "12", "--pass-spp", "4", "--until-error", "1e-6"]


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
        with r.accumulator(cam, W, H, bounces=3, seed=1234) as acc, acc.noise() as est:
            for _ in range(3):
                acc.add(4)
                est.update(tol=1e-6)
            img, var = acc.image(), est.variance()
        return img, var, r.denoise_guided(img, feat, var), r.denoise_guided(img, feat, var, iterations=2, sigma_luma=0.5)


def test_guided_image_and_variance_map_equal_the_api(tmp_path, api_side):
    img, var, guided, guided_2 = api_side
    assert np.isfinite(var).all() and (var > 0).any() and guided.tobytes() != img.tobytes()
    pfm, vmap = str(tmp_path / "a.pfm"), str(tmp_path / "v.pfm")
    r = _run(SIZE + LOOP + ["--denoise-guided", "--variance-map", vmap, "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert "stopped at 12 samples" in r.stdout
    assert pt.read_pfm(pfm).tobytes() == guided.tobytes()
    assert pt.read_pfm(vmap).tobytes() == np.repeat(var[..., None], 3, axis=2).tobytes()
    r = _run(SIZE + LOOP + ["--denoise-guided", "2", "--sigma-luma", "0.5", "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(pfm).tobytes() == guided_2.tobytes()
    # --variance-map alone attaches an estimator and leaves the image unfiltered
    r = _run(SIZE + ["--spp", "12", "--pass-spp", "4", "--variance-map", vmap, "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(pfm).tobytes() == img.tobytes()
    assert pt.read_pfm(vmap).tobytes() == np.repeat(var[..., None], 3, axis=2).tobytes()


def test_usage_errors(tmp_path):
    for args in (["--spp", "4", "--denoise-guided"], ["--spp", "4", "--pass-spp", "2", "--denoise-guided", "3"]):
        r = _run(SIZE + args + ["--out", str(tmp_path / "a.ppm")])
        assert r.returncode == 2 and "--denoise-guided needs an estimator" in r.stderr and "usage:" in r.stderr
    r = _run(SIZE + LOOP + ["--denoise-guided", "--denoise", "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 2 and "--denoise-guided" in r.stderr
    r = _run(SIZE + LOOP + ["--denoise-guided", "--sigma-luma", "0", "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 2 and "--sigma-luma" in r.stderr
    r = _run(["--help"])
    assert "--denoise-guided" in r.stderr and "--sigma-luma" in r.stderr and "--variance-map" in r.stderr
