"""Resumable accumulation (pt_accum_*, Renderer.accumulator): a render built up in passes equals the one-shot
render -- and the oracle's f64 image -- in every bit, whatever the pass sizes, the unit split, the image
shape, the shard, and across a checkpoint file.

At these sizes every pixel goes through the chunked path by default (npix is far below the resident lanes);
PT_WF_CHUNKS=1 forces whole-pixel units.  Both are used."""
import os
import shutil

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, shard

pytestmark = pytest.mark.gpu

CAM = dict(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0)   # kernel.cu:642-648
W, H, SPP, BOUNCES = 24, 16, 9, 3
SPLITS = [[9], [1] * 9, [4, 5], [1, 8], [8, 1], [2, 3, 4]]
HEADER_BYTES = 128


def _cam(w, h, radius=0.0):
    return pt.make_camera(pos=CAM["pos"], dist_from_film=1.0, focal_length=3.0, radius=radius, width=w, height=h)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cb():
    s = load_scene("cornell_blob")
    r = pt.Renderer(s, 0)
    yield s, r
    r.close()


_ORACLE = {}
_PLAIN = {}


def _oracle(scene, w, h, spp, bounces, integ, radius, key):
    """The oracle's f64 image and counters, computed once per configuration."""
    k = (key, w, h, spp, bounces, integ, radius)
    if k not in _ORACLE:
        import oracle
        osc = oracle.OracleScene(scene.arrays())
        ocam = oracle.camera(CAM["pos"], CAM["dist_from_film"], CAM["focal_length"], radius, w, h)
        _ORACLE[k] = oracle.render(osc, ocam, w, h, spp, bounces, integ, 1234)
    return _ORACLE[k]


def _plain(r, n, integ, radius):
    """Renderer.render of the base case at n samples (cornell_blob context `r`), once per configuration."""
    k = (n, integ, radius)
    if k not in _PLAIN:
        _PLAIN[k] = r.render(_cam(W, H, radius), W, H, n, bounces=BOUNCES, integrator=integ)
    return _PLAIN[k]


def _run_split(r, scene, split, integ, radius, key="cb"):
    """Accumulate `split` on context r; after every pass the image equals the plain render at the samples so far,
    at the end the f64 mean equals the oracle's image and the summed stats the one-shot's."""
    total = sum(split)
    samples = rays_ref = 0
    with r.accumulator(_cam(W, H, radius), W, H, bounces=BOUNCES, integrator=integ) as acc:
        assert acc.samples == 0 and not acc.image().any() and not acc.mean64().any()
        for k in split:
            st = acc.add(k)
            samples += st["samples"]
            rays_ref += st["rays_reference"]
            assert st["samples"] == W * H * k
            assert acc.samples <= total
            img, _ = _plain(r, acc.samples, integ, radius) if key == "cb" else \
                r.render(_cam(W, H, radius), W, H, acc.samples, bounces=BOUNCES, integrator=integ)
            assert _same_bits(acc.image(), img), (split, acc.samples)
        assert acc.samples == total
        mean = acc.mean64()
        img32 = acc.image()
    ref, cnt = _oracle(scene, W, H, total, BOUNCES, integ, radius, "cornell_blob")
    assert _same_bits(mean, ref)
    assert _same_bits(img32, ref.astype(np.float32))
    assert samples == W * H * total
    assert rays_ref == cnt["traces"]
    if key == "cb":
        assert rays_ref == _plain(r, total, integ, radius)[1]["rays_reference"]


# ---------------------------------------------------------------- 1. passes equal one shot
@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_passes_equal_one_shot(cb, split, integ, radius):
    s, r = cb
    _run_split(r, s, split, integ, radius)


# ---------------------------------------------------------------- 2. unit shapes
UNIT_ENVS = [{"PT_WF_CHUNKS": "1"}, {"PT_WF_CHUNKS": "3"}, {"PT_WF_CHUNKS": "7"}, {"PT_WF_CHUNKS": "64"},
             {"PT_WF_CHUNKS": "4", "PT_WF_TAIL_NPIX": "37"}, {"PT_WF_CHUNKS": "4", "PT_WF_TAIL_NPIX": "100"},
             # (test_three_grade_split_units_bit_exact's first setting)
             {"PT_WF_MID_CHUNKS": "2", "PT_WF_FINE_PX": "0.0003", "PT_WF_FINE_CHUNKS": "4", "PT_WF_FIN_PX": "0.0001",
              "PT_WF_FIN_CHUNKS": "9"}]


@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("env", UNIT_ENVS, ids=lambda e: ",".join("%s=%s" % (k[6:], v) for k, v in e.items()))
def test_unit_shapes(monkeypatch, env, integ, radius):
    """A continuing chunk 0 (n != 1), more chunks than the pass has samples, chunk counts that do not divide the
    pass, lens draws in the replay, and Morton pixel 0, which draws lens values even at radius 0."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = load_scene("cornell_blob")
    with pt.Renderer(s, 0) as r:
        for split in ([1, 8], [4, 5], [2, 3, 4]):
            _run_split(r, s, split, integ, radius, key="env")


# ---------------------------------------------------------------- 3. shapes
def _against_oracle(scene, r, w, h, bounces, integ, split, key, pixel_order=0):
    total = sum(split)
    with r.accumulator(_cam(w, h), w, h, bounces=bounces, integrator=integ, pixel_order=pixel_order) as acc:
        for k in split:
            acc.add(k)
        img, mean = acc.image(), acc.mean64()
    one, _ = r.render(_cam(w, h), w, h, total, bounces=bounces, integrator=integ, pixel_order=pixel_order)
    assert _same_bits(img, one)
    ref, _ = _oracle(scene, w, h, total, bounces, integ, 0.0, key)
    if pixel_order == pt.PT_ORDER_MORTON:
        idx = np.array([[pt.morton_pxl_to_i(x, y) for x in range(w)] for y in range(h)])
        assert _same_bits(mean[idx], ref)
    else:
        assert _same_bits(mean, ref)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("w,h,bounces", [(13, 7, 3), (1, 1, 3), (40, 9, 3), (24, 16, 1), (24, 16, 16)])
def test_image_sizes_and_depths(cb, w, h, bounces, integ):
    s, r = cb
    _against_oracle(s, r, w, h, bounces, integ, [2, 3], "cornell_blob")


@pytest.mark.parametrize("integ", [0, 1])
def test_morton_pixel_order(cb, integ):
    s, r = cb
    _against_oracle(s, r, 16, 16, 3, integ, [2, 3], "cornell_blob", pixel_order=pt.PT_ORDER_MORTON)


@pytest.mark.parametrize("integ", [0, 1])
def test_emissive_sphere_scene(integ):
    s = load_scene("cornell")
    s.add_sphere((0.3, 0.5, 0.2), 0.25, (0.7, 0.7, 0.7), (4.0, 3.0, 2.0))
    with pt.Renderer(s, 0) as r:
        _against_oracle(s, r, 24, 16, 3, integ, [2, 3], "cornell_sphere")


# ---------------------------------------------------------------- 4. shards
@pytest.mark.parametrize("integ", [0, 1])
def test_shards_sum_to_one_shot(cb, integ):
    s, r = cb
    total = np.zeros((H, W, 3), dtype=np.float32)
    for i in range(3):
        with r.accumulator(_cam(W, H), W, H, bounces=BOUNCES, integrator=integ, shard_index=i, shard_count=3) as acc:
            acc.add(4)
            acc.add(5)
            img, mean = acc.image(), acc.mean64()
        mine = np.zeros(W * H, dtype=bool)
        mine[shard.shard_pixels(W, H, i, 3)] = True
        assert not img.reshape(-1, 3)[~mine].any() and not mean.reshape(-1, 3)[~mine].any()
        total += img
    assert _same_bits(total, _plain(r, 9, integ, 0.0)[0])


# ---------------------------------------------------------------- 5. both unidir instances
@pytest.mark.parametrize("integ", [0, 1])
def test_standin_scene_takes_the_memory_walk_instance(standin_scene, integ):
    """The stand-in's tree does not fit the LDS top (cornell's does): integrator 0's other instance."""
    from cudapathtracer_amd import scenes
    w, h = 64, 48
    cam = pt.make_camera(width=w, height=h, **scenes.SPONZA_STANDIN_CAMERA)
    with pt.Renderer(standin_scene, 0) as r:
        with r.accumulator(cam, w, h, bounces=BOUNCES, integrator=integ) as acc:
            acc.add(2)
            acc.add(4)
            img = acc.image()
        one, st = r.render(cam, w, h, 6, bounces=BOUNCES, integrator=integ)
    assert np.count_nonzero(one) > 0
    assert _same_bits(img, one)


# ---------------------------------------------------------------- 6. device output
def test_device_output_on_a_stream(cb):
    import torch
    s, r = cb
    stream = torch.cuda.Stream()
    buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with r.accumulator(_cam(W, H), W, H, bounces=BOUNCES) as acc:
        for k in (4, 5):
            acc.add(k, d_out_ptr=buf.data_ptr(), stream_ptr=stream.cuda_stream)
            assert _same_bits(buf.cpu().numpy(), acc.image())
    assert _same_bits(buf.cpu().numpy(), _plain(r, 9, 0, 0.0)[0])


# ---------------------------------------------------------------- 7. isolation
def test_plain_render_between_passes(cb):
    s, r = cb
    other = dict(bounces=5, integrator=1, seed=77)
    alone, _ = r.render(_cam(32, 32), 32, 32, 3, **other)
    with r.accumulator(_cam(W, H), W, H, bounces=BOUNCES) as acc:
        acc.add(4)
        between, _ = r.render(_cam(32, 32), 32, 32, 3, **other)
        acc.add(5)
        img = acc.image()
    assert _same_bits(between, alone)
    assert _same_bits(img, _plain(r, 9, 0, 0.0)[0])


# ---------------------------------------------------------------- 8. checkpoint
@pytest.mark.parametrize("integ", [0, 1])
def test_checkpoint_round_trip(tmp_path, integ):
    path = str(tmp_path / "state.ptacc")
    s = load_scene("cornell_blob")
    with pt.Renderer(s, 0) as r:
        one, _ = r.render(_cam(W, H, 0.05), W, H, 9, bounces=BOUNCES, integrator=integ)
        acc = r.accumulator(_cam(W, H, 0.05), W, H, bounces=BOUNCES, integrator=integ)
        acc.add(4)
        acc.save(path)
        acc.close()
    assert os.path.getsize(path) == HEADER_BYTES + W * H * 48
    info = pt.accum_file_info(path)
    assert info["samples"] == 4 and info["params"].width == W and info["params"].integrator == integ
    with pt.Renderer(load_scene("cornell_blob"), 0) as r2:
        with r2.load_accumulator(path) as acc:
            assert acc.samples == 4
            acc.add(5)
            assert _same_bits(acc.image(), one)
        # a truncated copy
        cut = str(tmp_path / "cut.ptacc")
        shutil.copy(path, cut)
        with open(cut, "r+b") as fh:
            fh.truncate(HEADER_BYTES + W * H * 48 - 17)
        with pytest.raises(pt.PtError) as e:
            r2.load_accumulator(cut)
        assert e.value.code == pt.PT_E_IO
    # another scene
    with pt.Renderer(load_scene("cornell"), 0) as r3:
        with pytest.raises(pt.PtError) as e:
            r3.load_accumulator(path)
        assert e.value.code == pt.PT_E_SCENE and "scene" in str(e.value)


# ---------------------------------------------------------------- 9. refusals
@pytest.mark.parametrize("flags", [pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH, pt.PT_FLAG_COUNT])
def test_unsupported_flags_are_refused(cb, flags):
    s, r = cb
    with pytest.raises(pt.PtError) as e:
        r.accumulator(_cam(W, H), W, H, flags=flags)
    assert e.value.code == pt.PT_E_INVALID and "pt_accum_create" in str(e.value)


def test_far_camera_is_refused(cb):
    s, r = cb
    far = pt.make_camera(pos=(0.0, 1.0, 1.0e4), dist_from_film=1.0, focal_length=3.0, radius=0.0, width=W, height=H)
    with pytest.raises(pt.PtError) as e:
        r.accumulator(far, W, H)
    assert e.value.code == pt.PT_E_INVALID


def test_head_on_the_tile_kernel_is_refused(monkeypatch):
    monkeypatch.setenv("PT_HEAD_WF", "0")
    with pt.Renderer(load_scene("cornell_blob"), 0) as r:
        with pytest.raises(pt.PtError) as e:
            r.accumulator(_cam(W, H), W, H, integrator=1)
        assert e.value.code == pt.PT_E_INVALID
        r.accumulator(_cam(W, H), W, H, integrator=0).close()   # integrator 0 still accumulates


def test_supported_flags_and_limits(cb):
    s, r = cb
    fl = pt.PT_FLAG_NO_DEAD_PATH_SKIP | pt.PT_FLAG_NO_PRIMARY_CACHE
    one, st1 = r.render(_cam(W, H), W, H, 9, bounces=BOUNCES, flags=fl)
    with r.accumulator(_cam(W, H), W, H, bounces=BOUNCES, flags=fl) as acc:
        traced = acc.add(4)["rays_traced"] + acc.add(5)["rays_traced"]
        assert acc.add(0)["samples"] == 0 and acc.samples == 9          # spp = 0: a no-op
        assert _same_bits(acc.image(), one)
        assert traced == st1["rays_traced"]                              # no memo, no skip: the same rays
        with pytest.raises(pt.PtError) as e:                             # a total the unit words cannot carry
            acc.add(2 ** 30)
        assert e.value.code == pt.PT_E_INVALID
        with pytest.raises(pt.PtError):
            acc.add(-1)
        assert acc.samples == 9
