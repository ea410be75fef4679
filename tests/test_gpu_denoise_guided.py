"""The variance-guided denoiser and the variance map on the GPU (pt_denoise_guided*, pt_noise_variance*): every case
is compared bit for bit with the numpy restatement (tests/denoise_guided_ref.py), on the default kernels, with every
step staged through LDS (PT_DENOISE_TILED_MAX=16) and on the direct gather (PT_DENOISE_DIRECT=1), which must also
equal each other."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, scenes, shard

import adaptive_ref
import denoise_guided_ref
import denoise_ref
import noise_ref

pytestmark = pytest.mark.gpu

BOUNCES, SEED = 3, 1234


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@contextlib.contextmanager
def direct_gather(on, tiled_max=None):
    """The library reads its knobs at every call: PT_DENOISE_DIRECT=1 runs every iteration on the direct gather,
    PT_DENOISE_TILED_MAX moves the largest LDS-staged step (default 4, at most 16)."""
    old = {k: os.environ.pop(k, None) for k in ("PT_DENOISE_DIRECT", "PT_DENOISE_TILED_MAX")}
    if on:
        os.environ["PT_DENOISE_DIRECT"] = "1"
    if tiled_max is not None:
        os.environ["PT_DENOISE_TILED_MAX"] = str(tiled_max)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def cb():
    s = load_scene("cornell_blob")
    with pt.Renderer(s, 0) as r:
        yield s, r


def _cam(w, h):
    return pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)


# ---------------------------------------------------------------- inputs
def _features(w, h, seed, unit_normals=False):
    """Random features: unit and (unless unit_normals) non-unit normals, nearly coplanar and scattered positions,
    albedos below the 1e-3 clamp, about 20% pass-through pixels, and pass-through pixels at every corner and along
    the borders."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w), dtype=pt.FEATURE)
    n = rng.normal(size=(h, w, 3))
    unit = n / np.linalg.norm(n, axis=2)[..., None]
    f["normal"] = unit if unit_normals else np.where(rng.random((h, w, 1)) < 0.5, unit, unit * rng.uniform(0.3, 1.5, (h, w, 1)))
    f["normal"][rng.random((h, w)) < 0.5] = f["normal"][h // 2, w // 2]          # many equal ones: weights near 1
    f["position"] = rng.uniform(-5, 5, (h, w, 3))
    f["position"][:, : (w + 1) // 2] *= 0.01
    f["depth"] = rng.uniform(0.1, 50, (h, w))
    f["albedo"] = rng.uniform(0, 1, (h, w, 3))
    f["albedo"][rng.random((h, w)) < 0.1] = 0.0
    f["prim"] = rng.integers(0, 1000, (h, w))
    kind = rng.random((h, w))
    f["prim"][kind < 0.1] = -1
    f["prim"][(kind >= 0.1) & (kind < 0.2)] |= pt.PT_FEATURE_EMISSIVE
    if w * h > 1:
        f["prim"][0, 0] = -1
        f["prim"][h - 1, w - 1] |= pt.PT_FEATURE_EMISSIVE
    if w > 4 and h > 2:
        f["prim"][0, w - 1] = f["prim"][h - 1, 0] = -1
        f["prim"][0, 1::3] = -1                                                   # along the top and the left border
        f["prim"][1::2, 0] |= pt.PT_FEATURE_EMISSIVE
    img = rng.uniform(0, 10, (h, w, 3)).astype(np.float32)
    return img, f


def _variance(w, h, seed, special=True):
    """Variances from far below to far above the image's squared luminance differences, and (special) every value
    the prepass treats on its own: 0, denormals, 1e30, +inf, NaN, negative, and one that overflows on demodulation."""
    rng = np.random.default_rng(seed + 1000)
    v = (10.0 ** rng.uniform(-6, 3, (h, w))).astype(np.float32)
    if special:
        pick = rng.random((h, w))
        for k, val in enumerate([0.0, 1e-42, 1e-39, 1e30, np.inf, np.nan, -1.0, -0.0, 3e38]):
            v[(pick >= 0.04 * k) & (pick < 0.04 * (k + 1))] = np.float32(val)
    return v


def _all_kernels(r, img, feat, var, **kw):
    """The filtered image, after checking that the default, the all-staged and the direct-gather runs agree."""
    with direct_gather(False):
        out = r.denoise_guided(img, feat, var, **kw)
    with direct_gather(True):
        direct = r.denoise_guided(img, feat, var, **kw)
    assert _bits(out) == _bits(direct), "tiled and direct-gather kernels differ"
    with direct_gather(False, tiled_max=16):
        staged = r.denoise_guided(img, feat, var, **kw)
    assert _bits(staged) == _bits(direct), "LDS staging at steps 8 / 16 differs from the direct gather"
    return out


def _check(r, img, feat, var, **kw):
    got = _all_kernels(r, img, feat, var, **kw)
    ref = denoise_guided_ref.denoise_guided_ref(img, feat, var, **kw)
    bad = int(np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32)))
    assert bad == 0, "%d of %d values differ from the numpy restatement" % (bad, got.size)
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    assert _bits(got[skip]) == _bits(img[skip])
    assert np.isfinite(got).all()
    return got


# ---------------------------------------------------------------- 1. the filter against the restatement
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (70, 45), (130, 9)])
def test_sizes(cb, w, h):
    """1x1 and 5x3: every tap but a few is outside; 70x45: one 64-wide tile and a remainder, lattice-row tiles of
    every step; 130x9: two tiles and a remainder, fewer rows than one block."""
    _, r = cb
    img, feat = _features(w, h, 11)
    var = _variance(w, h, 11)
    out = _check(r, img, feat, var)
    plain = r.denoise(img, feat)
    if w > 1:
        assert _bits(out) != _bits(plain) and _bits(out) != _bits(img)          # the variance did something


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_iterations(cb, iterations):
    _, r = cb
    img, feat = _features(70, 45, 12)
    out = _check(r, img, feat, _variance(70, 45, 12), iterations=iterations)
    if iterations == 0:
        assert _bits(out) == _bits(img)


def test_morton_order(cb):
    _, r = cb
    w = h = 32
    img, feat = _features(w, h, 13)
    var = _variance(w, h, 13)
    idx = np.array([[pt.morton_pxl_to_i(x, y) for x in range(w)] for y in range(h)])
    mimg, mfeat, mvar = np.zeros((w * h, 3), np.float32), np.zeros(w * h, pt.FEATURE), np.zeros(w * h, np.float32)
    mimg[idx], mfeat[idx], mvar[idx] = img, feat, var
    ref = denoise_guided_ref.denoise_guided_ref(img, feat, var)
    got = _all_kernels(r, mimg, mfeat, mvar, pixel_order=1)
    assert _bits(got[idx]) == _bits(ref)


@pytest.mark.parametrize("kw", [dict(demodulate=False), dict(sigma_color=2.0), dict(sigma_color=0.5, demodulate=False),
                                dict(sigma_luma=0.5), dict(sigma_luma=8.0, normal_power_log2=0)],
                         ids=["no_demodulate", "sigma_color", "both", "sigma_luma_low", "sigma_luma_high"])
def test_parameters(cb, kw):
    _, r = cb
    img, feat = _features(70, 45, 14)
    _check(r, img, feat, _variance(70, 45, 14), **kw)


@pytest.mark.parametrize("value", [0.0, 1e-42, 1e30, np.inf, np.nan, -1.0], ids=str)
def test_uniform_variance(cb, value):
    """One value everywhere.  0 and the denormal: only taps of exactly equal luminance keep their weight; the unknown
    values (1e30, inf, NaN, negative): the plain filter, byte for byte.  Unit normals, as a renderer's are: a pixel
    whose own tap weighs so little that its square underflows (a normal of length 0.3 raised to the 64th power) loses
    its variance, unknown or not, after one iteration."""
    _, r = cb
    img, feat = _features(70, 45, 15, unit_normals=True)
    out = _check(r, img, feat, np.full((45, 70), value, dtype=np.float32))
    if not (value >= 0 and value < 1e30):
        assert _bits(out) == _bits(r.denoise(img, feat))


def test_unknown_variance_is_pt_denoise(cb):
    """var = +inf against pt_denoise_device itself, on device pointers, on a render (not synthetic) and with
    sigma_color on."""
    import torch
    _, r = cb
    w, h = 70, 45
    img = r.render(_cam(w, h), w, h, 4, bounces=BOUNCES, seed=SEED)[0]
    feat = r.features(_cam(w, h), w, h)
    d_img = torch.from_numpy(img.copy()).cuda()
    d_feat = torch.from_numpy(np.frombuffer(feat.tobytes(), dtype=np.uint8).copy()).cuda()
    d_var = torch.full((h, w), float("inf"), dtype=torch.float32, device="cuda")
    for kw in (dict(), dict(sigma_color=0.5)):
        d_plain, d_guided = torch.zeros_like(d_img), torch.zeros_like(d_img)
        r.denoise_device(d_img.data_ptr(), d_feat.data_ptr(), d_plain.data_ptr(), w, h, **kw)
        r.denoise_guided_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), d_guided.data_ptr(), w, h, **kw)
        torch.cuda.synchronize()
        assert _bits(d_guided.cpu().numpy()) == _bits(d_plain.cpu().numpy())
        assert _bits(d_plain.cpu().numpy()) != _bits(img)


def test_in_place_on_device_pointers(cb):
    import torch
    _, r = cb
    w, h = 70, 45
    img, feat = _features(w, h, 16)
    var = _variance(w, h, 16)
    ref = denoise_guided_ref.denoise_guided_ref(img, feat, var)
    d_feat = torch.from_numpy(np.frombuffer(feat.tobytes(), dtype=np.uint8).copy()).cuda()
    d_var = torch.from_numpy(var).cuda()
    for direct in (False, True):
        d_img = torch.from_numpy(img.copy()).cuda()
        d_out = torch.zeros_like(d_img)
        with direct_gather(direct):
            r.denoise_guided_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), d_out.data_ptr(), w, h)
            r.denoise_guided_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), d_img.data_ptr(), w, h)   # out == in
        torch.cuda.synchronize()
        assert _bits(d_out.cpu().numpy()) == _bits(ref) and _bits(d_img.cpu().numpy()) == _bits(ref)
        assert _bits(d_var.cpu().numpy()) == _bits(var)


def test_plain_filter_after_the_guided_one(cb):
    """Both filters share the context's scratch: the plain one is unchanged by a guided call before it."""
    _, r = cb
    img, feat = _features(70, 45, 17)
    before = r.denoise(img, feat)
    r.denoise_guided(img, feat, _variance(70, 45, 17))
    assert _bits(r.denoise(img, feat)) == _bits(before) == _bits(denoise_ref.denoise_ref(img, feat))


def test_refusals(cb):
    _, r = cb
    img, feat = _features(24, 16, 18)
    var = _variance(24, 16, 18)
    for kw in (dict(sigma_luma=0.0), dict(sigma_luma=-2.0), dict(sigma_luma=float("nan")), dict(sigma_luma=float("inf")),
               dict(iterations=9), dict(sigma_depth=0.0)):
        with pytest.raises(pt.PtError) as e:
            r.denoise_guided(img, feat, var, **kw)
        assert e.value.code == pt.PT_E_INVALID, kw
    gp = pt.Renderer.denoise_guided_params()
    out = np.empty_like(img)
    L = _lib.lib()
    assert L.pt_denoise_guided(r._h, C.byref(gp), 24, 16, 0, img.ctypes.data, feat.ctypes.data, None,
                               out.ctypes.data) == pt.PT_E_INVALID
    assert b"null" in L.pt_last_error()
    assert L.pt_denoise_guided(r._h, C.byref(gp), 24, 16, 1, img.ctypes.data, feat.ctypes.data, var.ctypes.data,
                               out.ctypes.data) == pt.PT_E_INVALID
    assert b"Morton" in L.pt_last_error()
    with pytest.raises(ValueError):
        r.denoise_guided(img, feat, var[:-1])


def test_refused_while_a_render_is_in_flight(cb):
    import torch
    _, r = cb
    w, h = 24, 16
    img, feat = _features(w, h, 19)
    var = _variance(w, h, 19)
    d = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc, acc.noise() as est:
        r.render_device_async(_cam(w, h), d.data_ptr(), w, h, 2)
        try:
            with pytest.raises(pt.PtError) as e:
                r.denoise_guided(img, feat, var)
            assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
            with pytest.raises(pt.PtError) as e:
                est.variance()
            assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
        finally:
            r.wait()
    _check(r, img, feat, var)


# ---------------------------------------------------------------- 2. the variance map
def _mask(acc):
    p = acc.params
    m = np.zeros(p.width * p.height, dtype=bool)
    m[shard.shard_pixels(p.width, p.height, p.shard_index, p.shard_count, p.tile_w or 8, p.tile_h or 8)] = True
    return m.reshape(p.height, p.width)


@pytest.mark.parametrize("start", [0, 3], ids=["from_zero", "attached_at_3"])
@pytest.mark.parametrize("w,h", [(24, 16), (20, 13)])
def test_variance_map_scalar(cb, w, h, start):
    """Scalar sweep, checked after every pass: +inf before two batches, then m2 / ((b-1) n) with n the accumulator's
    count -- for an estimator attached at 3 samples the window weight W = n - 3 is not what divides."""
    _, r = cb
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        if start:
            acc.add(start)
        with acc.noise() as est:
            ref = noise_ref.NoiseRef(start, acc.mean64())
            assert np.isposinf(est.variance()).all()
            for i, k in enumerate((2, 3, 4)):
                acc.add(k)
                est.update()
                ref.update(acc.samples, acc.mean64())
                got = est.variance()
                want = denoise_guided_ref.variance_ref(ref, acc.samples)
                assert got.dtype == np.float32 and _bits(got) == _bits(want)
                assert np.isposinf(got).all() == (i == 0)
            window = (ref.m2 / (float(ref.batches - 1) * ref.W)).astype(np.float32)
            assert (_bits(got) == _bits(window)) == (start == 0)
            assert (got > 0).any() and np.isfinite(got).all()
            # no fold: samples added since the last update do not enter m2 (n_q is the accumulator's count)
            acc.add(1)
            assert _bits(est.variance()) == _bits(denoise_guided_ref.variance_ref(ref, acc.samples))


@pytest.mark.parametrize("w,h", [(24, 16), (20, 13)])
def test_variance_map_per_pixel(cb, w, h):
    """Per-pixel sweep: a random mask frozen between passes; frozen pixels divide by the count they were frozen at
    and keep their batch count, pixels frozen after one batch stay +inf."""
    _, r = cb
    rng = np.random.default_rng(5)
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc, acc.noise() as est:
        ref = adaptive_ref.AdaptiveRef(0, acc.mean64())
        counts = np.zeros((h, w), dtype=np.uint32)
        frozen = np.zeros((h, w), dtype=bool)
        for k in (2, 3, 4, 2):
            acc.add(k)
            counts[~frozen] = acc.samples
            est.update()
            ref.update(acc.samples, counts, acc.mean64())
            assert _bits(acc.counts()) == _bits(counts)
            got = est.variance()
            assert _bits(got) == _bits(denoise_guided_ref.variance_ref(ref, counts))
            m = rng.random((h, w)) < 0.3
            acc.freeze(m)
            frozen |= m
        assert np.isposinf(got[counts == 2]).all() and np.isfinite(got[counts > 2]).all()
        assert len(np.unique(counts)) == 4


def test_variance_map_shard(cb):
    import torch
    _, r = cb
    w, h = 24, 16
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED, shard_index=1, shard_count=2, tile=8) as acc, \
            acc.noise() as est:
        ref = noise_ref.NoiseRef(0, acc.mean64())
        for k in (2, 3):
            acc.add(k)
            est.update()
            ref.update(acc.samples, acc.mean64())
        mask = _mask(acc)
        assert 0 < mask.sum() < w * h
        want = denoise_guided_ref.variance_ref(ref, acc.samples)
        got = est.variance()
        assert _bits(got) == _bits(np.where(mask, want, np.float32(0.0)))
        buf = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        est.variance_device(buf.data_ptr())
        dev = buf.cpu().numpy()
        assert (dev[~mask] == -1.0).all() and _bits(dev[mask]) == _bits(want[mask])


def test_variance_map_morton(cb):
    _, r = cb
    w = h = 16
    idx = np.array([[pt.morton_pxl_to_i(x, y) for x in range(w)] for y in range(h)])
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED, pixel_order=pt.PT_ORDER_MORTON) as acc, \
            acc.noise() as est:
        ref = noise_ref.NoiseRef(0, acc.mean64())
        for k in (2, 3, 4):
            acc.add(k)
            est.update()
            ref.update(acc.samples, acc.mean64())
        got = est.variance()
        assert got.shape == (w * h,)
        want = denoise_guided_ref.variance_ref(ref, acc.samples)          # (in Morton order, like the mean it was fed)
        assert _bits(got) == _bits(want)
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc, acc.noise() as est:
        for k in (2, 3, 4):
            acc.add(k)
            est.update()
        assert _bits(est.variance()) == _bits(got[idx])


# ---------------------------------------------------------------- 3. end to end
def test_accumulator_to_filtered_image(cb):
    """cornell_blob 64x64, 8 passes of 4: noise.variance() and denoise_guided equal the restatement fed with the
    oracle's means, and the result is closer to the oracle's 2048-spp render than the noisy image (the host test's
    condition at 16 x 8 samples is `< 1`; here, at 32 samples, the restatement measured 0.61)."""
    import oracle
    s, r = cb
    w = h = 64
    kw = scenes.CORNELL_CAMERA
    osc = oracle.OracleScene(s.arrays())
    ocam = oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], kw["radius"], w, h)
    ref = noise_ref.NoiseRef(0, shape=(h, w))
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc, acc.noise() as est:
        for k in range(1, 9):
            acc.add(4)
            est.update()
            mean = oracle.render(osc, ocam, w, h, 4 * k, BOUNCES, 0, SEED)[0]
            ref.update(4 * k, mean)
        var = est.variance()
        img = acc.image()
    feat = r.features(_cam(w, h), w, h)
    assert _bits(img) == _bits(mean.astype(np.float32))
    assert _bits(var) == _bits(denoise_guided_ref.variance_ref(ref, 32))
    out = _all_kernels(r, img, feat, var)
    assert _bits(out) == _bits(denoise_guided_ref.denoise_guided_ref(mean.astype(np.float32), feat, var))
    clean = oracle.render(osc, ocam, w, h, 2048, BOUNCES, 0, 99)[0].astype(np.float32)
    e_noisy, e_out = denoise_ref.rmse(img, clean), denoise_ref.rmse(out, clean)
    print("rmse noisy %.4f guided %.4f ratio %.3f" % (e_noisy, e_out, e_out / e_noisy))
    assert e_out < e_noisy
