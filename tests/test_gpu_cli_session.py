"""pt_cli --session / --resume-session: an adaptive convergence run that is stopped after 16 samples and resumed in
another process writes the image and the per-pixel counts of the uninterrupted run, byte for byte, and its estimator
continues the saved window; a contradicting option fails as with --resume; --adaptive --checkpoint is still a usage
error (no GPU needed for that one)."""
import os
import re
import subprocess

import pytest

from conftest import MODELS, ROOT, SCENE_SETS

import cudapathtracer_amd as pt

from adaptive_ref import LOOP, SEED

CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H = 24, 16
SIZE = ["--width", str(W), "--height", str(H), "--bounces", "3", "--seed", str(SEED)]
LOOP_ARGS = ["--until-error", str(LOOP["tol"]), "--adaptive", "--error-quantile", "1", "--pass-spp", str(LOOP["pass_spp"])]


def _run(args):
    objs = []
    for obj, origin, scale, flip in SCENE_SETS["cornell_blob"]:
        objs += ["--obj", "%s@%r,%r,%r@%r@%d" % ((os.path.join(MODELS, obj),) + tuple(float(v) for v in origin) +
                                                  (float(scale), flip))]
    return subprocess.run([CLI] + objs + args, capture_output=True, text=True, timeout=300)


def _samples(stdout):
    return [int(m.group(1)) for m in (re.match(r"sample (\d+)$", ln) for ln in stdout.splitlines()) if m]


def test_adaptive_checkpoint_is_still_a_usage_error(tmp_path):
    r = _run(SIZE + ["--spp", "8"] + LOOP_ARGS + ["--checkpoint", str(tmp_path / "f.ptacc"), "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 2 and "--checkpoint" in r.stderr and "usage:" in r.stderr
    assert "--session" in r.stderr and "--resume-session" in r.stderr          # (the usage text names the new options)
    r = _run(SIZE + ["--resume", "a", "--resume-session", "b", "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 2 and "choose one" in r.stderr


@pytest.mark.gpu
def test_a_resumed_session_equals_the_uninterrupted_run(tmp_path):
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    a = _run(SIZE + LOOP_ARGS + ["--spp", "32", "--pfm", t("a.pfm"), "--count-map", t("ca.pfm"), "--out", t("a.ppm")])
    assert a.returncode == 0, a.stderr
    assert _samples(a.stdout) == list(range(4, 33, 4))                         # it ran past 16: the split is inside the loop
    assert "stopped at 32 samples: not converged" in a.stdout
    b1 = _run(SIZE + LOOP_ARGS + ["--spp", "16", "--session", t("f.ptses"), "--out", t("b1.ppm")])
    assert b1.returncode == 0, b1.stderr
    assert _samples(b1.stdout) == [4, 8, 12, 16]
    i = pt.session_file_info(t("f.ptses"))
    assert i["samples"] == 16 and i["flags"] == 7 and i["noise_batches"] == 4 and 0 < i["frozen_pixels"] < W * H
    b2 = _run(["--resume-session", t("f.ptses"), "--spp", "16"] + LOOP_ARGS +
              ["--pfm", t("b.pfm"), "--count-map", t("cb.pfm"), "--out", t("b.ppm")])
    assert b2.returncode == 0, b2.stderr
    assert _samples(b2.stdout) == [20, 24, 28, 32]
    assert "16 samples done, adding 16" in b2.stdout
    assert "window saved in" in b2.stdout and "continues" in b2.stdout and "fresh window" not in b2.stdout
    assert "stopped at 32 samples: not converged" in b2.stdout
    froze = lambda out: [ln for ln in out.splitlines() if ln.startswith(("froze ", "converged "))]   # noqa: E731
    assert froze(b1.stdout) + froze(b2.stdout) == froze(a.stdout)              # every pass's summary and freeze, too
    for x, y in (("a.pfm", "b.pfm"), ("ca.pfm", "cb.pfm"), ("a.ppm", "b.ppm")):
        assert open(t(x), "rb").read() == open(t(y), "rb").read(), (x, y)


@pytest.mark.gpu
def test_resume_session_refuses_a_contradicting_option(tmp_path):
    f = str(tmp_path / "f.ptses")
    r = _run(SIZE + ["--spp", "4", "--session", f, "--out", str(tmp_path / "a.ppm")])
    assert r.returncode == 0, r.stderr
    for flag in ("--resume-session", "--resume"):
        r = _run([flag, f, "--spp", "4", "--width", str(W + 8), "--out", str(tmp_path / "b.ppm")])
        if flag == "--resume":                                                 # (format 1's reader does not take the file at all)
            assert r.returncode == 1 and "format version 2, this build reads 1" in r.stderr
        else:
            assert r.returncode == 2 and "--width contradicts the resumed file" in r.stderr
    r = _run(["--resume-session", f, "--spp", "4", "--width", str(W), "--out", str(tmp_path / "b.ppm")])
    assert r.returncode == 0 and "4 samples done, adding 4" in r.stdout        # the same value is no contradiction
