"""pt_cli --camera-path FILE --temporal: the files of a 4-pose path on the Cornell fixture equal the Python sequence
(render, features, Temporal.push per pose) bit for bit -- the CLI does no trigonometry, the poses are the file's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, load_scene

import cudapathtracer_amd as pt
import temporal_ref

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, SPP, SEED = 48, 32, 2, 77
TARGET = (0.1, 0.9, -0.2)


def _cli(*args):
    base = [CLI, "--obj", os.path.join(MODELS, "cornell.obj"), "--quiet"]
    return subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _poses():
    return [temporal_ref.orbit_pose(i, 0.03)[0] for i in range(4)]


def _path_file(tmp_path):
    p = tmp_path / "path.txt"
    lines = ["# px py pz tx ty tz", ""]
    lines += ["%.9g %.9g %.9g %.9g %.9g %.9g" % (tuple(pos) + TARGET) for pos in _poses()]
    p.write_text("\n".join(lines) + "\n")
    return str(p)


@pytest.fixture(scope="module")
def sequence():
    """(out, var, features) of the last frame of the Python sequence, for the plain and the jittered run."""
    res = {}
    with pt.Renderer(load_scene("cornell"), 0) as r:
        for flags in (0, pt.PT_FLAG_JITTER):
            with r.temporal(W, H, max_history=3) as t:
                for k, pos in enumerate(_poses()):
                    cam = pt.make_camera(pos, 1.0, 3.0, 0.0, W, H)
                    view = pt.look_at(pos, TARGET, vfov=40.0, cam=cam)
                    img, _ = r.render(cam, W, H, SPP, seed=SEED + k, flags=flags, view=view)
                    feat = r.features(cam, W, H, view=view, flags=flags)
                    out, var = t.push(img, feat, cam, view, flags)
                assert t.frames == 4 and t.history_length().max() == 3
            res[flags] = (out, var, feat, r.denoise_guided(out, feat, var, iterations=3))
    return res


@pytest.mark.parametrize("jitter", [False, True])
def test_files_equal_the_python_sequence(sequence, tmp_path, jitter):
    out, var, feat, filtered = sequence[pt.PT_FLAG_JITTER if jitter else 0]
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    args = ["--width", W, "--height", H, "--spp", SPP, "--seed", SEED, "--vfov", 40, "--camera-path", _path_file(tmp_path),
            "--temporal", "--temporal-max", 3] + (["--jitter", "box"] if jitter else [])
    r = _cli(*args, "--pfm", t("a.pfm"), "--variance-map", t("v.pfm"), "--out", t("a.ppm"))
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(t("a.pfm")).tobytes() == out.tobytes()
    grey = pt.read_pfm(t("v.pfm"))
    assert np.isfinite(var).any() and np.isinf(var).any()
    for k in range(3):
        assert np.ascontiguousarray(grey[..., k]).tobytes() == var.tobytes()
    # filtered with the temporal variance; the variance map is still the unfiltered history's
    r = _cli(*args, "--denoise-guided", 3, "--pfm", t("g.pfm"), "--variance-map", t("w.pfm"), "--out", t("g.ppm"))
    assert r.returncode == 0, r.stderr
    assert pt.read_pfm(t("g.pfm")).tobytes() == filtered.tobytes() != out.tobytes()
    assert open(t("w.pfm"), "rb").read() == open(t("v.pfm"), "rb").read()


def test_usage_errors(tmp_path):
    path = _path_file(tmp_path)
    r = _cli("--temporal")
    assert r.returncode == 2 and "--temporal needs --camera-path" in r.stderr
    r = _cli("--camera-path", path)
    assert r.returncode == 2 and "--camera-path needs --temporal" in r.stderr
    r = _cli("--camera-path", path, "--temporal", "--pass-spp", 1)
    assert r.returncode == 2 and "independent frames" in r.stderr
    r = _cli("--camera-path", path, "--temporal", "--look-at", "0,1,0")
    assert r.returncode == 2 and "--look-at" in r.stderr
    r = _cli("--camera-path", path, "--temporal", "--temporal-max", 0)
    assert r.returncode == 2 and "--temporal-max" in r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("0 1 3 0 1\n")
    r = _cli("--camera-path", str(bad), "--temporal")
    assert r.returncode == 2 and "line 1" in r.stderr
    r = _cli("--camera-path", str(tmp_path / "none.txt"), "--temporal")
    assert r.returncode == 2 and "cannot read" in r.stderr
