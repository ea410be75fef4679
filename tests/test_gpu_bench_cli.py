"""bench.py as a command on one GPU: a plain run times its steps and prints the result line without the
counting pass or the CPU baseline (those are --full's), and --dump-outputs DIR leaves the last timed step's
framebuffer in DIR/image.npy -- the image a direct render of the same scene, camera and seed returns, bit for bit.
A small Cornell frame (C2's scene at 48x40, 4 spp) keeps the run to the process start-up."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 48, 40, 4, 8


def _bench(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PT_BENCH_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "C2", "--width", str(W), "--height", str(H), "--spp", str(SPP),
           "--cache-dir", str(tmp_path / "scene")] + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(200)
def test_gpu_plain_bench_dumps_the_last_steps_framebuffer(tmp_path):
    out = tmp_path / "dump"
    d = _bench(tmp_path, "--dump-outputs", str(out))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["image_finite"] is True
    assert d["ms_per_step"] > 0
    # value is the timed steps' samples over their wall time
    assert d["value"] == pytest.approx(W * H * SPP / (d["ms_per_step"] * 1e-3) / 1e6, rel=2e-2)
    # a plain run: no counting pass, no CPU baseline
    assert d["roofline"] is None and d["cache_roofline"] is None and d["l1_roofline"] is None
    assert d["cpu_baseline"] is None
    assert sorted(os.listdir(str(out))) == ["image.npy"]
    img = np.load(str(out / "image.npy"))
    assert img.dtype == np.float32 and img.shape == (H, W, 3)
    # the same scene file, camera, seed and parameters through the blocking render call
    s = pt.Scene()
    models = str(tmp_path / "scene" / "models")
    s.load_obj(os.path.join(models, "cornell.obj"), mtl_basepath=models + "/")
    s.build_bvh()
    with pt.Renderer(s, 0) as r:
        ref, st = r.render(pt.make_camera(width=W, height=H, **scenes.CORNELL_CAMERA), W, H, SPP, bounces=BOUNCES)
    assert st["samples"] == W * H * SPP
    assert img.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes()


@pytest.mark.timeout(200)
def test_gpu_full_bench_adds_the_counting_pass_and_the_cpu_baseline(tmp_path):
    d = _bench(tmp_path, "--full", "--cpu-budget", "0.2", "--cpu-threads", "4")
    assert d["steps"] == 3 and d["image_finite"] is True and d["ms_per_step"] > 0
    roof = d["roofline"]
    assert roof["kernel"] == "render_unidir_wf" and roof["node_fetches"] >= 0 and roof["tri_tests"] > 0
    assert d["cache_roofline"]["algorithmic_bytes_per_launch"] > 0
    cpu = d["cpu_baseline"]
    assert cpu["unit"] == "Msamples/s" and cpu["value"] > 0 and cpu["cores"] == 4
