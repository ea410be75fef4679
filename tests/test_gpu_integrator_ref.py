"""The GPU image against the REFERENCE's own integrators and running mean (tests/golden/integ_*.npz; see
integrator_ref.py and test_integrator_host.py): the fp32 image equals float32 of the `det` flavour's mean -- the
reference's text with cos/sin bound to or_sincos, folded by its own kernel.cu:551-552 -- in every bit, through the
oracle nowhere.  Only the committed fixtures are read.

A pixel is compared when none of its samples is flagged "reference undefined (d2)" (integrator 1's camera bounce
missed; the reference reads tris[-1] there).  Each test asserts how many pixels that left.

The pixel at Morton index 0, (0, 0), of a CAMERA render is left out, as tests/test_ref_gap.py leaves it out: DESIGN.md
decision d1 has that pixel draw a lens pair from its own stream before every sample (the race-free reading of
kernel.cu:547), and the fixtures hold no lens draws -- the argument order of those two draws is unspecified in the
reference and stays unpinned.  Renders along caller rays draw no lens pair anywhere: there every pixel counts."""
import numpy as np
import pytest

import cudapathtracer_amd as pt

import integrator_ref as ir

pytestmark = pytest.mark.gpu

SETS = ir.sets()
CAMERA_SETS = [s for s in SETS if s["kind"] == "camera"]
RAY_SETS = [s for s in SETS if s["kind"] == "rays"]


@pytest.fixture(scope="module")
def renderers():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pt.Renderer(ir.load_scene(name), 0)
        return cache[name]
    yield get
    for r in cache.values():
        r.close()


def _expected(s, camera):
    """(float32 mean of the det flavour (H, W, 3), mask (H, W) of the pixels to compare); asserts the mask's size."""
    f = ir.load(s["name"])
    w, h = s["w"], s["h"]
    use = f["flag"].sum(axis=1) == 0
    if camera:
        use[0] = False                                       # Morton index 0: see the module docstring
    n = int(use.sum())
    if s["scene"] == "closed":
        assert n >= 0.99 * w * h, n
    else:
        assert 3 * n >= w * h, n
    return f, f["mean_det"].astype(np.float32).reshape(h, w, 3), use.reshape(h, w)


def _check(tag, img, want, use):
    bad = ~ir.same_bits(np.ascontiguousarray(img, dtype=np.float32)[use], want[use]).all(axis=1)
    assert not bad.any(), "%s: %d of %d compared pixels differ from the reference's mean" % (tag, int(bad.sum()), int(use.sum()))


@pytest.mark.parametrize("s", CAMERA_SETS, ids=[s["name"] for s in CAMERA_SETS])
def test_camera_render_equals_reference_mean(s, renderers):
    _, want, use = _expected(s, camera=True)
    r = renderers(s["scene"])
    w, h, spp = s["w"], s["h"], s["spp"]
    cam = pt.make_camera(ir.CAMERA_POS[s["scene"]], ir.CAMERA["dist_from_film"], ir.CAMERA["focal_length"],
                         ir.CAMERA["radius"], w, h)
    args = (cam, w, h, spp, s["bounces"], s["integrator"], s["seed"])
    for tag, flags in (("wavefront", 0), ("reference traversal", pt.PT_FLAG_REFERENCE_TRAVERSAL),
                       ("reference BVH", pt.PT_FLAG_REFERENCE_BVH)):
        img, _ = r.render(*args, flags=flags)
        _check(tag, img, want, use)
    with r.accumulator(cam, w, h, s["bounces"], s["integrator"], s["seed"]) as acc:
        for k in (1, spp - 1):
            acc.add(k)
        assert acc.samples == spp
        _check("accumulator", acc.image(), want, use)
    parts = [r.render(*args, shard_index=i, shard_count=2)[0] for i in range(2)]
    _check("two shards", parts[0] + parts[1], want, use)


@pytest.mark.parametrize("s", RAY_SETS, ids=[s["name"] for s in RAY_SETS])
def test_caller_rays_equal_reference_mean(s, renderers):
    f, want, use = _expected(s, camera=False)
    r = renderers(s["scene"])
    w, h, spp = s["w"], s["h"], s["spp"]
    o, d = f["rays"][:, :3], f["rays"][:, 3:]
    img, _ = r.render_rays(o, d, w, h, spp, s["bounces"], s["integrator"], s["seed"])
    _check("render_rays", img, want, use)
    with r.accumulator_rays(o, d, w, h, s["bounces"], s["integrator"], s["seed"]) as acc:
        for k in (1, spp - 1):
            acc.add(k)
        assert acc.samples == spp
        _check("accumulator_rays", acc.image(), want, use)
