"""Temporal reprojection on the GPU (pt_temporal_*, pt_temporal.hip): every push is compared bit for bit with the numpy
restatement (tests/temporal_ref.py) -- the image, the variance, the history lengths, and through the next push the
planes the kernel stored.  Synthetic frames aim every pixel's reprojection at a chosen spot of the previous frame, so
each branch of the header's arithmetic is reached and the restatement's `stats` say so; real frames come from the
render and feature kernels along a look-at orbit."""
import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

import denoise_guided_ref
import temporal_ref
import view_ref
from temporal_ref import F, TemporalRef

pytestmark = pytest.mark.gpu

JIT = pt.PT_FLAG_JITTER
POS = (0.0, 1.0, 3.0)
# (pos, view) of the synthetic frames' cameras
NULL = (POS, None)
LOOK = temporal_ref.orbit_pose(3)
LOOK2 = temporal_ref.orbit_pose(9)
MIRROR = (POS, view_ref.MIRROR)
ORIGIN = ((0.0, 0.0, 0.0), None)      # with a power-of-two image the projections of chosen points are exact integers
NORMALS = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [0, -0.8, 0.6]], dtype=F)


@pytest.fixture(scope="module")
def renderers():
    out = {}
    for name in ("cornell", "cornell_blob"):
        out[name] = pt.Renderer(load_scene(name), 0)
    yield out
    for r in out.values():
        r.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _view(v):
    return None if v is None else pt.make_view(v[0], v[1], v[2], v[3])


def _cam(pose, w, h):
    return pt.make_camera(pose[0], 1.0, 3.0, 0.0, w, h), (pose[0], 1.0, 3.0, 0.0, w, h)


def _morton_index(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.array([view_ref.morton(int(x), int(y)) for x, y in zip(xs.reshape(-1), ys.reshape(-1))])


def _to_order(a, order):
    """A scanline (H, W, ...) array as the library takes it in `order`."""
    if order == pt.PT_ORDER_SCANLINE:
        return a
    h, w = a.shape[:2]
    out = np.empty((h * w,) + a.shape[2:], dtype=a.dtype)
    out[_morton_index(w, h)] = a.reshape((h * w,) + a.shape[2:])
    return out


def _from_order(a, order, w, h):
    if order == pt.PT_ORDER_SCANLINE:
        return a
    return a[_morton_index(w, h)].reshape((h, w) + a.shape[1:])


# ---------------------------------------------------------------- synthetic frames
def _world(pose, w, h, fx, fy, s):
    """The points at distance parameter s (camera-space depth s * dist; s < 0: behind) on the pinhole rays of `pose`
    through the film points (fx, fy), in float64, rounded to float32 once."""
    pos, view = pose
    R, U, B, film = view_ref.IDENTITY if view is None else view
    gx = (fx / w - 0.5) * film[0]
    gy = (fy / h - 0.5) * film[1]
    c = np.stack([-s * gx, -s * gy, -s * np.ones_like(gx)], axis=-1)       # dist_from_film = 1
    P = np.asarray(pos, dtype=np.float64) + c[..., :1] * np.asarray(R, dtype=np.float64) + \
        c[..., 1:2] * np.asarray(U, dtype=np.float64) + c[..., 2:] * np.asarray(B, dtype=np.float64)
    return P.astype(F)


def _frame(rng, w, h, prev_pose, prev_off, prev_feat, exact=False):
    """One frame of random colours and features.  With a previous frame, every pixel's position is aimed through the
    previous camera: at an exact pixel, within and just beyond the snap distance of one, anywhere in the image, in
    the band x0 = -1 / y0 = -1 and the last column / row, outside on each side, or behind the camera; its normal and
    depth make the tap under it pass both consistency tests, fail only the normal test or only the plane test."""
    img = rng.uniform(0, 10, (h, w, 3)).astype(F)
    f = np.zeros((h, w), dtype=pt.FEATURE)
    f["albedo"] = rng.uniform(0, 1, (h, w, 3))
    f["normal"] = NORMALS[rng.integers(0, len(NORMALS), (h, w))]
    f["prim"] = rng.integers(0, 1000, (h, w))
    f["prim"][rng.random((h, w)) < 0.1] |= pt.PT_FEATURE_EMISSIVE
    f["depth"] = rng.uniform(0.5, 5, (h, w))
    f["position"] = rng.uniform(-3, 3, (h, w, 3))
    if prev_feat is not None:
        kind = rng.integers(0, 12, (h, w))
        qx = rng.integers(0, w, (h, w)).astype(np.float64)
        qy = rng.integers(0, h, (h, w)).astype(np.float64)
        sign = rng.choice([-1.0, 1.0], (h, w))
        dx, dy = np.zeros((h, w)), np.zeros((h, w))
        dx[kind == 1], dy[kind == 1] = 0.012, -0.012                        # within the snap distance (1/64 = 0.0156)
        dx[kind == 2], dy[kind == 2] = 0.019, 0.019                         # just beyond it
        frac = (kind >= 3) & (kind <= 5)
        dx[frac], dy[frac] = rng.uniform(0.05, 0.95, frac.sum()), rng.uniform(0.05, 0.95, frac.sum())
        fx, fy = qx + sign * dx, qy + sign * dy
        edge = kind == 6                                                    # x0 = -1 or W - 1, y0 = -1 or H - 1
        fx[edge] = np.where(rng.random(edge.sum()) < 0.5, -rng.uniform(0.1, 0.9, edge.sum()), w - 1 + rng.uniform(0.1, 0.9, edge.sum()))
        edge = kind == 7
        fy[edge] = np.where(rng.random(edge.sum()) < 0.5, -rng.uniform(0.1, 0.9, edge.sum()), h - 1 + rng.uniform(0.1, 0.9, edge.sum()))
        out = kind == 8                                                     # outside on each side
        side = rng.integers(0, 4, (h, w))
        fx[out & (side == 0)] = -1.5
        fx[out & (side == 1)] = w + 0.5
        fy[out & (side == 2)] = -1.0 - 1e-3
        fy[out & (side == 3)] = h + 3.0
        s = rng.uniform(1.0, 5.0, (h, w))
        if exact:
            s = np.exp2(rng.integers(0, 3, (h, w)).astype(np.float64))     # powers of two keep the products exact
        s[kind == 9] *= -1.0                                                # behind the previous camera
        f["position"] = _world(prev_pose, w, h, fx + prev_off, fy + prev_off, s)
        # the tap under the aim: its normal (kept, or turned away), and a depth that opens or shuts the plane test
        x0 = np.clip(np.floor(fx + 1e-9).astype(int), 0, w - 1)
        y0 = np.clip(np.floor(fy + 1e-9).astype(int), 0, h - 1)
        f["normal"] = prev_feat["normal"][y0, x0]
        how = rng.integers(0, 4, (h, w))
        f["normal"][how == 1] *= F(-1)                                      # fails the normal test
        f["depth"] = np.where(how == 2, F(1e-6), F(1e6))                    # how == 2 fails the plane test
        f["depth"][how == 3] = rng.uniform(0.5, 5, np.count_nonzero(how == 3))
    miss = rng.random((h, w)) < 0.1
    f["prim"][miss] = -1
    return img, f


def _run(r, w, h, frames, order=pt.PT_ORDER_SCANLINE, seed=1, exact=False, want=(), **params):
    """Push random frames through the poses `frames` = [(pose, flags), ...] on the GPU and through the restatement;
    everything bit for bit after every push.  Returns the restatement's stats summed over the pushes."""
    rng = np.random.default_rng(seed)
    ref = TemporalRef(w, h, **params)
    total = {}
    with r.temporal(w, h, pixel_order=order, **params) as t:
        assert t.frames == 0 and not t.history_length().any()
        prev_pose, prev_off, prev_feat = None, 0.0, None
        for k, (pose, flags) in enumerate(frames):
            img, feat = _frame(rng, w, h, prev_pose, prev_off, prev_feat, exact)
            cam, rcam = _cam(pose, w, h)
            out, var = t.push(_to_order(img, order), _to_order(feat, order), cam, _view(pose[1]), flags)
            rout, rvar = ref.push(img, feat, rcam, pose[1], flags)
            out, var = _from_order(out, order, w, h), _from_order(var, order, w, h)
            n = _from_order(t.history_length(), order, w, h)
            for name, a, b in (("out", out, rout), ("var", var, rvar), ("history length", n, ref.history_length())):
                bad = int(np.count_nonzero(_bits(a) != _bits(b)))
                assert bad == 0, "push %d: %d of %d values of %s differ from the restatement" % (k, bad, a.size, name)
            assert t.frames == k + 1
            for key, v in ref.stats.items():
                total[key] = total.get(key, 0) + (v if not isinstance(v, bool) else int(v))
            prev_pose, prev_off, prev_feat = pose, (0.5 if flags & JIT else 0.0), feat
    for key in want:
        assert total.get(key, 0) > 0, (key, total)
    return total


EVERY_BRANCH = ("behind", "left", "right", "top", "bottom", "snapped", "just_beyond_snap", "fractional", "x0_minus1", "x0_last",
                "y0_minus1", "y0_last", "tap_outside", "tap_miss", "tap_normal_only", "tap_plane_only", "tap_pass", "history_used",
                "miss")


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (24, 16), (37, 19), (64, 64), (130, 70)])
def test_sizes(renderers, w, h):
    """None a multiple of the 64 x 4 block; 130x70 is three blocks wide with a remainder.  Every branch of the
    arithmetic is reached at every size that has the pixels for it."""
    frames = [(NULL, 0), (LOOK, 0), (LOOK2, 0), (LOOK2, 0), (MIRROR, 0)]
    _run(renderers["cornell"], w, h, frames, seed=w, want=EVERY_BRANCH if w * h >= 24 * 16 else ())


@pytest.mark.parametrize("size,order", [(16, pt.PT_ORDER_SCANLINE), (16, pt.PT_ORDER_MORTON), (32, pt.PT_ORDER_MORTON),
                                        (64, pt.PT_ORDER_SCANLINE)])
def test_exact_pixels_and_morton_order(renderers, size, order):
    """A camera at the origin and a power-of-two image: aims at pixels are exact integers before the snap."""
    _run(renderers["cornell"], size, size, [(ORIGIN, 0)] * 3, order=order, seed=size, exact=True, want=EVERY_BRANCH + ("exact",))


@pytest.mark.parametrize("flags", [(JIT, 0, 0), (0, JIT, 0), (JIT, JIT, JIT), (0, 0, JIT)])
@pytest.mark.parametrize("pose", ["null", "look", "mirror"])
def test_views_and_jitter(renderers, pose, flags):
    """NULL, look-at and mirrored views; PT_FLAG_JITTER on one, the other and both of two consecutive frames: the
    previous frame's flag alone decides off_prev."""
    p = dict(null=NULL, look=LOOK, mirror=MIRROR)[pose]
    _run(renderers["cornell"], 37, 19, [(p, f) for f in flags], seed=3, want=("snapped", "fractional", "tap_pass"))


@pytest.mark.parametrize("max_history,pushes", [(1, 3), (2, 4), (32, 35)])
def test_history_cap(renderers, max_history, pushes):
    """A still camera over fixed features: n' climbs by 1 a push up to max_history and stays there."""
    w, h = 24, 16
    r = renderers["cornell"]
    cam, rcam = _cam(LOOK, w, h)
    feat = r.features(cam, w, h, view=_view(LOOK[1]))
    hit = feat["prim"] >= 0
    assert hit.sum() > w * h // 2
    rng = np.random.default_rng(max_history)
    ref = TemporalRef(w, h, max_history=max_history)
    with r.temporal(w, h, max_history=max_history) as t:
        for k in range(pushes):
            img = rng.uniform(0, 4, (h, w, 3)).astype(F)
            out, var = t.push(img, feat, cam, _view(LOOK[1]))
            rout, rvar = ref.push(img, feat, rcam, LOOK[1])
            n = t.history_length()
            assert np.array_equal(_bits(out), _bits(rout)) and np.array_equal(_bits(var), _bits(rvar))
            assert np.array_equal(_bits(n), _bits(ref.history_length()))
            assert np.all(n[hit] == min(k + 1, max_history)) and np.all(n[~hit] == 1)
    assert ref.stats["n_at_cap"] >= hit.sum()


def test_device_buffers_aliasing_and_null_variance(renderers):
    """pt_temporal_push_device: out == in, and d_var = NULL; both equal the host variant's bits."""
    import torch
    r = renderers["cornell"]
    w, h = 70, 45
    rng = np.random.default_rng(8)
    frames, prev = [], (None, 0.0, None)
    for pose in (NULL, LOOK, LOOK2):
        img, feat = _frame(rng, w, h, *prev)
        frames.append((pose, img, feat))
        prev = (pose, 0.0, feat)
    with r.temporal(w, h) as host, r.temporal(w, h) as alias, r.temporal(w, h) as novar:
        for pose, img, feat in frames:
            cam, _ = _cam(pose, w, h)
            out, var = host.push(img, feat, cam, _view(pose[1]))
            d_feat = torch.from_numpy(np.frombuffer(feat.tobytes(), dtype=np.uint8).copy()).cuda()
            d_img = torch.from_numpy(img.copy()).cuda()
            d_var = torch.zeros(h * w, dtype=torch.float32, device="cuda")
            alias.push_device(d_img.data_ptr(), d_feat.data_ptr(), d_img.data_ptr(), cam, _view(pose[1]), d_var_ptr=d_var.data_ptr())
            torch.cuda.synchronize()
            assert d_img.cpu().numpy().tobytes() == out.tobytes() and d_var.cpu().numpy().tobytes() == var.tobytes()
            d_in = torch.from_numpy(img.copy()).cuda()
            d_out = torch.zeros_like(d_in)
            novar.push_device(d_in.data_ptr(), d_feat.data_ptr(), d_out.data_ptr(), cam, _view(pose[1]))
            torch.cuda.synchronize()
            assert d_out.cpu().numpy().tobytes() == out.tobytes() and d_in.cpu().numpy().tobytes() == img.tobytes()
        assert host.history_length().tobytes() == alias.history_length().tobytes() == novar.history_length().tobytes()
        with pytest.raises(pt.PtError) as e:                                  # a feature buffer off its 16-byte alignment
            novar.push_device(d_in.data_ptr(), d_feat.data_ptr() + 4, d_out.data_ptr(), cam, None)
        assert e.value.code == pt.PT_E_INVALID and "aligned" in str(e.value)


# ---------------------------------------------------------------- real frames
@pytest.mark.parametrize("scene,flags", [("cornell", 0), ("cornell_blob", 0), ("cornell_blob", JIT)])
def test_orbit_of_rendered_frames(renderers, scene, flags):
    """6 frames of 1 spp on the look-at orbit, rendered and featured on the GPU (both equal the oracle elsewhere),
    pushed on the GPU, against the restatement; then the variance-guided denoiser with the temporal variance against
    its restatement."""
    r = renderers[scene]
    S = 64
    ref = TemporalRef(S, S)
    with r.temporal(S, S) as t:
        for i in range(6):
            pose = temporal_ref.orbit_pose(i)
            cam, rcam = _cam(pose, S, S)
            img, _ = r.render(cam, S, S, 1, 3, 0, temporal_ref.ORBIT_SEED + i, flags, view=_view(pose[1]))
            feat = r.features(cam, S, S, view=_view(pose[1]), flags=flags)
            out, var = t.push(img, feat, cam, _view(pose[1]), flags)
            rout, rvar = ref.push(img, feat, rcam, pose[1], flags)
            assert np.array_equal(_bits(out), _bits(rout)) and np.array_equal(_bits(var), _bits(rvar)), i
            assert np.array_equal(_bits(t.history_length()), _bits(ref.history_length())), i
            if i:
                assert ref.stats["fractional"] > S * S // 2 and ref.stats["history_used"] > S * S // 2
    assert np.isfinite(var).sum() > S * S // 2 and ref.stats["n_max"] > 5.5
    got = r.denoise_guided(out, feat, var)
    want = denoise_guided_ref.denoise_guided_ref(out, feat, var)
    assert np.array_equal(_bits(got), _bits(want))
    assert got.tobytes() != out.tobytes()


def test_reset_two_histories_and_the_render_afterwards(renderers):
    r = renderers["cornell_blob"]
    w, h = 37, 19
    cam, rcam = _cam(LOOK, w, h)
    before, _ = r.render(cam, w, h, 2, view=_view(LOOK[1]))
    rng = np.random.default_rng(4)
    seq_a = [_frame(rng, w, h, None, 0.0, None)]
    seq_b = [_frame(rng, w, h, None, 0.0, None)]
    for _ in range(2):
        seq_a.append(_frame(rng, w, h, LOOK, 0.0, seq_a[-1][1]))
        seq_b.append(_frame(rng, w, h, LOOK, 0.0, seq_b[-1][1]))
    with r.temporal(w, h) as a, r.temporal(w, h, max_history=2, normal_min=0.5) as b:
        # a first push returns its input bit for bit, with an unknown variance
        out, var = a.push(*seq_a[0], cam, _view(LOOK[1]))
        assert out.tobytes() == seq_a[0][0].tobytes() and np.all(np.isinf(var)) and np.all(a.history_length() == 1)
        # interleaved with b, a gives what it gives alone
        ra, rb = TemporalRef(w, h), TemporalRef(w, h, max_history=2, normal_min=0.5)
        ra.push(*seq_a[0], rcam, LOOK[1])
        for k in range(3):
            ob, vb = b.push(*seq_b[k], cam, _view(LOOK[1]))
            wb, wvb = rb.push(*seq_b[k], rcam, LOOK[1])
            assert np.array_equal(_bits(ob), _bits(wb)) and np.array_equal(_bits(vb), _bits(wvb))
            if k:
                oa, va = a.push(*seq_a[k], cam, _view(LOOK[1]))
                wa, wva = ra.push(*seq_a[k], rcam, LOOK[1])
                assert np.array_equal(_bits(oa), _bits(wa)) and np.array_equal(_bits(va), _bits(wva))
        assert a.frames == 3 and np.isfinite(va).any()
        # reset starts over: the same frames give the same results again
        a.reset()
        assert a.frames == 0
        ra = TemporalRef(w, h)
        for k in range(3):
            oa, va = a.push(*seq_a[k], cam, _view(LOOK[1]))
            wa, wva = ra.push(*seq_a[k], rcam, LOOK[1])
            assert np.array_equal(_bits(oa), _bits(wa)) and np.array_equal(_bits(va), _bits(wva))
            if k == 0:
                assert oa.tobytes() == seq_a[0][0].tobytes() and np.all(np.isinf(va))
    after, _ = r.render(cam, w, h, 2, view=_view(LOOK[1]))
    assert after.tobytes() == before.tobytes()


def test_refusals(renderers):
    import torch
    r = renderers["cornell"]
    w, h = 24, 16
    with pytest.raises(pt.PtError) as e:
        r.temporal(w, h, pixel_order=pt.PT_ORDER_MORTON)
    assert e.value.code == pt.PT_E_INVALID and "Morton" in str(e.value)
    with pytest.raises(pt.PtError) as e:
        r.temporal(w, h, max_history=0)
    assert e.value.code == pt.PT_E_INVALID
    rng = np.random.default_rng(6)
    img, feat = _frame(rng, w, h, None, 0.0, None)
    cam, _ = _cam(NULL, w, h)
    with r.temporal(w, h) as t:
        with pytest.raises(pt.PtError) as e:
            t.push(img, feat, _cam(NULL, h, w)[0])                       # another camera size
        assert e.value.code == pt.PT_E_INVALID and "camera" in str(e.value)
        bad = pt.make_view((1, 0, 0), (0, 1, 0), (0, 0, 1.5))
        with pytest.raises(pt.PtError) as e:
            t.push(img, feat, cam, bad)
        assert e.value.code == pt.PT_E_INVALID and "orthonormal" in str(e.value)
        for field in ("dist_from_film", "focal_length"):
            c2 = _cam(NULL, w, h)[0]
            setattr(c2, field, 0.0)
            with pytest.raises(pt.PtError) as e:
                t.push(img, feat, c2)
            assert e.value.code == pt.PT_E_INVALID and field in str(e.value)
        d = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        r.render_device_async(cam, d.data_ptr(), w, h, 2)
        try:
            with pytest.raises(pt.PtError) as e:
                t.push(img, feat, cam)
            assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
            with pytest.raises(pt.PtError) as e:
                r.temporal(w, h)
            assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
        finally:
            r.wait()
        assert t.frames == 0                                              # no refused push counted
        out, var = t.push(img, feat, cam)
        assert out.tobytes() == img.tobytes() and t.frames == 1
