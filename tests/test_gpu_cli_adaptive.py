"""pt_cli --adaptive / --count-map: the command-line tool's adaptive loop gives the Python API's
(Accumulator.add_adaptive) image and per-pixel sample counts byte for byte; --adaptive without --until-error is a
usage error (no GPU needed for that one)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, SCENE_SETS, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

from adaptive_ref import LOOP, SEED

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H = 24, 16
SIZE = ["--width", str(W), "--height", str(H), "--bounces", "3", "--seed", str(SEED)]


def _run(args):
    objs = []
    for obj, origin, scale, flip in SCENE_SETS["cornell_blob"]:
        objs += ["--obj", "%s@%r,%r,%r@%r@%d" % ((os.path.join(MODELS, obj),) + tuple(float(v) for v in origin) +
                                                  (float(scale), flip))]
    return subprocess.run([CLI] + objs + args, capture_output=True, text=True, timeout=300)


def test_adaptive_needs_until_error(tmp_path):
    for extra in ([], ["--pass-spp", "4"]):
        r = _run(SIZE + ["--spp", "8", "--adaptive", "--out", str(tmp_path / "a.ppm")] + extra)
        assert r.returncode == 2 and "--adaptive needs --until-error" in r.stderr and "usage:" in r.stderr
    r = _run(SIZE + ["--spp", "8", "--pass-spp", "4", "--until-error", "0.2", "--adaptive", "--checkpoint",
                     str(tmp_path / "f.ptacc"), "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 2 and "--checkpoint" in r.stderr


@pytest.mark.gpu
def test_adaptive_and_count_map_equal_the_api(tmp_path):
    cam = pt.make_camera(width=W, height=H, **scenes.CORNELL_CAMERA)
    with pt.Renderer(load_scene("cornell_blob"), 0) as r, r.accumulator(cam, W, H, bounces=3, seed=SEED) as acc:
        res = acc.add_adaptive(LOOP["pass_spp"], LOOP["cap"], tol=LOOP["tol"], quantile=LOOP["quantile"])
        img, counts = acc.image(), acc.counts()
    assert len(np.unique(counts)) == 7 and res["active"] > 0 and not res["stopped_converged"]
    pfm, cmap = str(tmp_path / "a.pfm"), str(tmp_path / "c.pfm")
    run = _run(SIZE + ["--spp", str(LOOP["cap"]), "--pass-spp", str(LOOP["pass_spp"]), "--until-error", str(LOOP["tol"]),
                       "--adaptive", "--error-quantile", "1", "--count-map", cmap, "--pfm", pfm,
                       "--out", str(tmp_path / "a.ppm")])
    assert run.returncode == 0, run.stderr
    assert "stopped at %d samples: not converged" % LOOP["cap"] in run.stdout
    froze = [ln for ln in run.stdout.splitlines() if ln.startswith("froze ")]
    assert len(froze) == res["passes"] - 1 and froze[-1].endswith("%d still sampled" % res["active"])
    assert pt.read_pfm(pfm).tobytes() == img.tobytes()
    assert pt.read_pfm(cmap).tobytes() == np.repeat(counts.astype(np.float32)[..., None], 3, axis=2).tobytes()
