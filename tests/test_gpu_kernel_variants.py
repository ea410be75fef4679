"""Wavefront kernel instances that only a knob selects (pt::wavefront_variant, render_plan.h): PT_WF_MIN_WAVES and
PT_HEAD_MIN_WAVES pick other register budgets of the same kernels, so every one of them must give the default
instance's frame byte for byte, and the committed oracle render.  The knobs are read at pt_create: each case sets
them before it creates its renderer.  The PT_LANE_TIMING diagnostic rides on the same launch.
"""
import os

import numpy as np
import pytest

from conftest import GOLD, load_scene

import cudapathtracer_amd as pt

pytestmark = pytest.mark.gpu

CAM = dict(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0)
KNOBS = ("PT_WF_MIN_WAVES", "PT_HEAD_MIN_WAVES", "PT_WF_LDS_TREE", "PT_LANE_TIMING")
# scene, width, height, spp, bounces, integrator: the committed oracle renders
CORNELL = ("cornell", 24, 16, 3, 8, 0)
BLOB_HEAD = ("cornell_blob", 32, 32, 4, 3, 1)


def _golden(case):
    name, w, h, spp, bounces, integ = case
    return np.load(os.path.join(GOLD, "render_%s_%dx%d_s%d_b%d_i%d.npz" % (name, w, h, spp, bounces, integ)))["img"]


def _render(case, flags=0):
    name, w, h, spp, bounces, integ = case
    with pt.Renderer(load_scene(name), 0) as r:
        img, st = r.render(pt.make_camera(width=w, height=h, **CAM), w, h, spp, bounces=bounces, integrator=integ,
                           flags=flags)
    assert st["work_units"] > 0   # the wavefront path (the tile kernel has no units)
    assert st["samples"] == w * h * spp
    return img


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32).ravel(), np.asarray(b, np.float32).view(np.uint32).ravel())


@pytest.fixture(scope="module")
def default_frames():
    """Both cases on the default instances (no knob set), rendered once."""
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        return {case: _render(case) for case in (CORNELL, BLOB_HEAD)}


@pytest.mark.parametrize("env,flags", [
    ({"PT_WF_MIN_WAVES": "4"}, 0),                      # render_unidir_wf<false, 4, false>
    ({"PT_WF_MIN_WAVES": "6"}, 0),                      # render_unidir_wf<false, 6, false>
    ({"PT_WF_MIN_WAVES": "4"}, pt.PT_FLAG_COUNT),       # render_unidir_wf<true, 4, false>
    ({"PT_WF_LDS_TREE": "0"}, pt.PT_FLAG_COUNT),        # render_unidir_wf<true, 5, false>
], ids=["waves4", "waves6", "waves4-count", "no-lds-tree-count"])
def test_unidir_instances_give_the_default_frame(default_frames, monkeypatch, env, flags):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img = _render(CORNELL, flags)
    assert _same_bits(img, default_frames[CORNELL])
    assert _same_bits(img, _golden(CORNELL))


def test_head_four_waves_gives_the_default_frame(default_frames, monkeypatch):
    monkeypatch.setenv("PT_HEAD_MIN_WAVES", "4")        # render_head_wf<false, 4>
    img = _render(BLOB_HEAD)
    assert _same_bits(img, default_frames[BLOB_HEAD])
    assert _same_bits(img, _golden(BLOB_HEAD))


def test_lane_timing_appends_one_line_and_keeps_the_frame(default_frames, monkeypatch, tmp_path):
    path = tmp_path / "lane_timing.txt"
    monkeypatch.setenv("PT_LANE_TIMING", str(path))
    img = _render(CORNELL)
    lines = path.read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("lane_timing shards 1 lanes ")
    assert _same_bits(img, default_frames[CORNELL])
