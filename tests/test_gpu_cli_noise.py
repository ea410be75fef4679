"""pt_cli --until-error / --error-map: the command-line tool stops at the sample count the Python loop
(Accumulator.add_until) stops at, writes the same image bytes, and its error map equals NoiseEstimate.error_map."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, SCENE_SETS, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, CAP = 24, 16, 30
SIZE = ["--width", str(W), "--height", str(H), "--bounces", "3"]


def _run(args):
    objs = []
    for obj, origin, scale, flip in SCENE_SETS["cornell_blob"]:
        objs += ["--obj", "%s@%r,%r,%r@%r@%d" % ((os.path.join(MODELS, obj),) + tuple(float(v) for v in origin) +
                                                  (float(scale), flip))]
    return subprocess.run([CLI] + objs + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def api_side():
    """The Python loop: passes of 4 until 90% of the pixels are within a relative standard error of 1.0."""
    cam = pt.make_camera(width=W, height=H, **scenes.CORNELL_CAMERA)
    with pt.Renderer(load_scene("cornell_blob"), 0) as r:
        with r.accumulator(cam, W, H, bounces=3, seed=1234) as acc:
            res = acc.add_until(4, CAP, tol=1.0, quantile=0.9)
            return res, acc.image(), acc._noise.error_map()


def test_until_error_and_error_map_equal_the_api(tmp_path, api_side):
    res, img, emap = api_side
    assert res["stopped_converged"] and res["samples"] < CAP
    pfm, err = str(tmp_path / "a.pfm"), str(tmp_path / "f.pfm")
    r = _run(SIZE + ["--spp", str(CAP), "--pass-spp", "4", "--until-error", "1.0", "--error-quantile", "0.9",
                     "--error-map", err, "--pfm", pfm, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [int(m.group(1)) for m in (re.match(r"sample (\d+)$", ln) for ln in lines) if m] == \
        list(range(4, res["samples"] + 1, 4))
    frac = [ln for ln in lines if ln.startswith("converged ")]
    assert len(frac) == res["passes"]
    s = res["summary"]
    assert frac[-1].startswith("converged %d of %d pixels" % (s["converged"], s["pixels"]))
    stop = [ln for ln in lines if ln.startswith("stopped at ")]
    assert stop == ["stopped at %d samples: converged" % res["samples"]]
    assert pt.read_pfm(pfm).tobytes() == img.tobytes()
    grey = pt.read_pfm(err)
    assert grey.tobytes() == np.repeat(emap[..., None], 3, axis=2).tobytes()


def test_cap_resume_and_refusals(tmp_path):
    f = str(tmp_path / "f.ptacc")
    r = _run(SIZE + ["--spp", "8", "--pass-spp", "4", "--until-error", "1e-6", "--checkpoint", f, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    assert "stopped at 8 samples: not converged" in r.stdout
    r = _run(["--resume", f, "--spp", "8", "--pass-spp", "4", "--until-error", "1.0", "--error-quantile", "0.9",
              "--out", str(tmp_path / "b.ppm")])
    assert r.returncode == 0, r.stderr
    assert "fresh window" in r.stdout and "(8 samples)" in r.stdout
    assert "stopped at 16 samples: converged" in r.stdout            # two batches of the new window
    for bad in (["--until-error", "0.1"], ["--pass-spp", "4", "--until-error", "0"],
                ["--pass-spp", "4", "--until-error", "0.1", "--error-quantile", "0"],
                ["--pass-spp", "4", "--until-error", "0.1", "--gpus", "2"], ["--pass-spp", "4", "--error-map", "x.pfm", "--gpus", "2"]):
        r = _run(SIZE + ["--spp", "8", "--out", str(tmp_path / "c.ppm")] + bad)
        assert r.returncode == 2, (bad, r.stderr)
    r = _run(["--help"])
    assert "--until-error" in r.stderr and "--error-map" in r.stderr
