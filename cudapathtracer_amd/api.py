"""Host-side mirror of the reference's render flow (kernel.cu:565-790) over the C-ABI.

    scene = Scene()
    scene.load_obj("models/CornellBox-Original.obj", (0, 0, 0), 1)      # loadOBJ, modelLoader.h:125
    scene.load_obj("models/teapot.obj", (0.35, 0.6, 0.3), 0.75)         # kernel.cu:591-592
    scene.build_bvh()                                                   # buildBVH, BVH.h:443 + guard :627
    cam = make_camera(pos=(0, 1, 3), dist_from_film=1, focal_length=3, radius=0,
                      width=512, height=512)                            # kernel.cu:642-648
    with Renderer(scene) as r:                                          # uploads, kernel.cu:664-700
        img, stats = r.render(cam, 512, 512, spp=99, bounces=3)         # NUM_SAMPLES-1 samples, :709
    write_ppm("image.ppm", img)                                         # kernel.cu:763-778

Every call goes through libptamd.so; arrays returned to Python are copies of the C++ host
scene (numpy structured views for tests) or the float32 image the gfx950 kernel wrote.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

VEC3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
TRI = np.dtype([("v0", "<i4"), ("v1", "<i4"), ("v2", "<i4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                ("mat", "<i4")])
MAT = np.dtype([("albedo", "<f8", (3,)), ("emission", "<f8", (3,))])
NODE = np.dtype([("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("left", "<u4"), ("right", "<u4")])
SPHERE = np.dtype([("pos", "<f4", (3,)), ("rad", "<f4"), ("diffuse", "<f8", (3,)), ("emission", "<f8", (3,))])
FEATURE = np.dtype([("albedo", "<f4", (3,)), ("depth", "<f4"), ("normal", "<f4", (3,)), ("prim", "<i4"),
                    ("position", "<f4", (3,)), ("reserved", "<f4")])   # pt_feature, 48 B
assert FEATURE.itemsize == 48


def denoise_defaults():
    """pt_denoise_defaults as a dict."""
    dp = L.DenoiseParams()
    L.lib().pt_denoise_defaults(C.byref(dp))
    return {k: getattr(dp, k) for k, _ in dp._fields_}


def denoise_guided_defaults():
    """pt_denoise_guided_defaults as a dict: pt_denoise's fields and sigma_luma."""
    gp = L.DenoiseGuidedParams()
    L.lib().pt_denoise_guided_defaults(C.byref(gp))
    d = {k: getattr(gp.base, k) for k, _ in gp.base._fields_}
    d["sigma_luma"] = gp.sigma_luma
    return d


def noise_defaults():
    """pt_noise_defaults as a dict (tol, y_floor)."""
    np_ = L.NoiseParams()
    L.lib().pt_noise_defaults(C.byref(np_))
    return {k: getattr(np_, k) for k, _ in np_._fields_}


def _noise_params(tol, y_floor):
    d = noise_defaults()
    np_ = L.NoiseParams()
    np_.tol = float(d["tol"] if tol is None else tol)
    np_.y_floor = float(d["y_floor"] if y_floor is None else y_floor)
    return np_


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    buf = C.string_at(ptr, n * dtype.itemsize)
    return np.frombuffer(buf, dtype=dtype).copy()


class Scene:
    """The reference's scene globals (modelLoader.h:43-47) as an object owned by libptamd."""

    def __init__(self):
        self._h = L.lib().pt_scene_new()
        if not self._h:
            raise MemoryError("pt_scene_new failed")

    def close(self):
        if self._h:
            L.lib().pt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_obj(self, path, origin=(0.0, 0.0, 0.0), scale=1.0, flip_normals=False, mtl_basepath=None):
        """loadOBJ (modelLoader.h:125-210).  mtl_basepath=None is the reference's "models/"."""
        o = L.Vec3(*[float(v) for v in origin])
        L.check(L.lib().pt_scene_load_obj(self._h, str(path).encode(),
                                          None if mtl_basepath is None else str(mtl_basepath).encode(),
                                          o, float(scale), int(bool(flip_normals))))
        return self

    loadOBJ = load_obj

    @property
    def warning(self) -> str:
        return (L.lib().pt_scene_last_warning(self._h) or b"").decode(errors="replace")

    def build_bvh(self):
        """buildBVH (BVH.h:443-474) + the depth guard of kernel.cu:627-631."""
        L.check(L.lib().pt_scene_build_bvh(self._h))
        return self

    buildBVH = build_bvh

    def view(self) -> L.SceneView:
        v = L.SceneView()
        L.check(L.lib().pt_scene_view(self._h, C.byref(v)))
        return v

    def accel_digest(self):
        """(digest, BVH4 node count, BVH4 depth) of the render path's acceleration structure
        as pt_create would build it (host-only diagnostic)."""
        v = self.view()
        dg, n4, d4 = C.c_uint64(), C.c_uint32(), C.c_int32()
        L.check(L.lib().pt_accel_digest(C.byref(v), C.byref(dg), C.byref(n4), C.byref(d4)))
        return int(dg.value), int(n4.value), int(d4.value)

    def arrays(self):
        """Copies of verts/tris/mats/lights/bvh as numpy structured arrays (test surface)."""
        v = self.view()
        return dict(
            verts=_arr(v.verts, v.num_verts, VEC3),
            tris=_arr(v.tris, v.num_tris, TRI),
            mats=_arr(v.mats, v.num_mats, MAT),
            lights=_arr(v.lights, v.num_lights, np.dtype("<u4")),
            total_light_area=np.float32(v.total_light_area),
            bvh=_arr(v.bvh, v.bvh_size, NODE),
            bvh_depth=int(v.bvh_depth),
            spheres=_arr(v.spheres, v.num_spheres, SPHERE),
        )

    def add_sphere(self, pos, rad, diffuse, emission=(0.0, 0.0, 0.0)):
        """sphere.h primitive (this build's semantics); returns self."""
        sp = L.Sphere()
        sp.pos = L.Vec3(*[float(v) for v in pos])
        sp.rad = float(rad)
        for k in range(3):
            sp.diffuse[k] = float(diffuse[k])
            sp.emission[k] = float(emission[k])
        L.check(L.lib().pt_scene_add_sphere(self._h, C.byref(sp)))
        return self


def make_camera(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0, width=512, height=512):
    """camera.h:26-34 (defaults = kernel.cu:642-648)."""
    c = L.Camera()
    c.pos = L.Vec3(*[float(v) for v in pos])
    c.dist_from_film = float(dist_from_film)
    c.focal_length = float(focal_length)
    c.radius = float(radius)
    c.pxl_width = int(width)
    c.pxl_height = int(height)
    return c


def make_view(right, up, back, film=(1.0, 1.0)):
    """A pt_view: the world-space images of camera +x, +y, +z (the camera looks along -back) and the film's extent
    (1, 1 = the reference's unit square).  Not validated here: every call that takes it does (an orthonormal basis
    to 1e-3, finite, film > 0)."""
    v = L.View()
    for k in range(3):
        v.right[k], v.up[k], v.back[k] = float(right[k]), float(up[k]), float(back[k])
    v.film_w, v.film_h = float(film[0]), float(film[1])
    return v


def look_at(pos, target, up=(0.0, 1.0, 0.0), vfov=None, cam=None, width=None, height=None):
    """The view of a camera at `pos` looking at `target` (pt_view_look_at; film 1 x 1).  With vfov (degrees, the
    vertical field of view) the film is sized for it and for square pixels (pt_view_set_fov): that needs `cam` (its
    dist_from_film) and the image size, which default to the camera's pxl_width / pxl_height."""
    v = L.View()
    L.check(L.lib().pt_view_look_at(L.Vec3(*[float(c) for c in pos]), L.Vec3(*[float(c) for c in target]),
                                    L.Vec3(*[float(c) for c in up]), C.byref(v)))
    if vfov is not None:
        if cam is None:
            raise ValueError("look_at: vfov needs cam (its dist_from_film sizes the film)")
        w = cam.pxl_width if width is None else width
        h = cam.pxl_height if height is None else height
        L.check(L.lib().pt_view_set_fov(C.byref(v), C.byref(cam), float(vfov), int(w), int(h)))
    return v


def _view_ref(view):
    return None if view is None else C.byref(view)


def jitter_offset(flags, ua, ub):
    """(jx, jy): the film-point offset of a jittered sample's first two draws (pt_jitter_offset): (ua, ub) for
    PT_FLAG_JITTER, 0.5 + the tent's inverse CDF with PT_FLAG_JITTER_TENT as well, (0, 0) without the flag."""
    jx, jy = C.c_float(), C.c_float()
    L.check(L.lib().pt_jitter_offset(int(flags), float(ua), float(ub), C.byref(jx), C.byref(jy)))
    return jx.value, jy.value


def camera_ray(cam, idx, lens=False, u1=0.0, u2=0.0, view=None, jitter=None):
    """(origin, direction) of pixel `idx` (a Morton index): pt_camera_ray, or pt_camera_ray_view with a view, or
    pt_camera_ray_jitter through (px + jx, py + jy) with jitter=(jx, jy)."""
    o, d = L.Vec3(), L.Vec3()
    if jitter is not None:
        L.lib().pt_camera_ray_jitter(C.byref(cam), _view_ref(view), int(idx), float(jitter[0]), float(jitter[1]),
                                     int(bool(lens)), float(u1), float(u2), C.byref(o), C.byref(d))
    elif view is None:
        L.lib().pt_camera_ray(C.byref(cam), int(idx), int(bool(lens)), float(u1), float(u2), C.byref(o), C.byref(d))
    else:
        L.lib().pt_camera_ray_view(C.byref(cam), C.byref(view), int(idx), int(bool(lens)), float(u1), float(u2),
                                   C.byref(o), C.byref(d))
    return (o.x, o.y, o.z), (d.x, d.y, d.z)


def project(cam, P, view=None):
    """(front, sx, sy): the continuous pixel coordinates at which the pinhole ray of `cam` / `view` passes through the
    world point P (pt_project_view, the inverse of camera_ray with lens=False); front is False for a point that is
    not in front of the camera (sx, sy are then unspecified)."""
    sx, sy = C.c_float(), C.c_float()
    rc = L.lib().pt_project_view(C.byref(cam), _view_ref(view), L.Vec3(*[float(c) for c in P]), C.byref(sx), C.byref(sy))
    if rc < 0:
        L.check(rc)
    return bool(rc), sx.value, sy.value


def temporal_defaults():
    """pt_temporal_defaults as a dict (max_history, normal_min, plane_tol, flags)."""
    tp = L.TemporalParams()
    L.lib().pt_temporal_defaults(C.byref(tp))
    return {k: getattr(tp, k) for k, _ in tp._fields_}


def morton_pxl_to_i(x, y):
    return int(L.lib().pt_morton_pxl_to_i(int(x), int(y)))


def morton_i_to_pxl(i):
    x, y = C.c_uint32(), C.c_uint32()
    L.lib().pt_morton_i_to_pxl(int(i), C.byref(x), C.byref(y))
    return x.value, y.value


def write_ppm(path, img, pixel_order=0, width=None, height=None):
    """kernel.cu:763-778 on a (H, W, 3) float32 or float64 mean image, or on a Morton-ordered
    (W*H, 3) float32 buffer (pixel_order=PT_ORDER_MORTON, width/height given)."""
    img = np.ascontiguousarray(img)
    if pixel_order == L.PT_ORDER_MORTON:
        if width is None or height is None:
            raise ValueError("write_ppm: a Morton-ordered buffer needs width and height")
        width, height = int(width), int(height)
        if width <= 0 or height <= 0 or img.size != width * height * 3:
            raise ValueError("write_ppm: Morton buffer holds %d values, width*height*3 = %d"
                             % (img.size, max(width, 0) * max(height, 0) * 3))
        img = np.ascontiguousarray(img, dtype=np.float32)
        L.check(L.lib().pt_write_ppm_order(str(path).encode(), img.ctypes.data, width, height, 1))
        return
    if pixel_order != L.PT_ORDER_SCANLINE:
        raise ValueError("write_ppm: unknown pixel_order %r" % (pixel_order,))
    h, w = img.shape[:2]
    if img.dtype == np.float64:
        L.check(L.lib().pt_write_ppm_f64(str(path).encode(), img.ctypes.data, w, h))
    else:
        img = np.ascontiguousarray(img, dtype=np.float32)
        L.check(L.lib().pt_write_ppm(str(path).encode(), img.ctypes.data, w, h))


def tonemap_u8(c):
    return int(L.lib().pt_tonemap_u8(float(c)))


def write_ppm_codes(path, codes):
    """The reference PPM text from (H, W, 3) int32 tone-map codes (e.g. Renderer.tonemap)."""
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    h, w = codes.shape[:2]
    L.check(L.lib().pt_write_ppm_codes(str(path).encode(), codes.ctypes.data, w, h))


def write_pfm(path, img):
    """Lossless float dump (PFM, little-endian, rows bottom-up) of an (H, W, 3) mean image."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape[:2]
    L.check(L.lib().pt_write_pfm(str(path).encode(), img.ctypes.data, w, h))


def read_pfm(path):
    """Inverse of write_pfm: (H, W, 3) float32."""
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"PF"
        w, h = (int(v) for v in fh.readline().split())
        scale = float(fh.readline())
        data = np.frombuffer(fh.read(), dtype="<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3)[::-1].astype(np.float32)


class Renderer:
    """Device-resident scene on one GPU (pt_create) and the render call (pt_render)."""

    def __init__(self, scene: Scene, device: int = 0):
        err = C.c_int(0)
        self._scene_view = scene.view()
        self._h = L.lib().pt_create(C.byref(self._scene_view), int(device), C.byref(err))
        if not self._h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        self.device = device

    def close(self):
        if self._h:
            L.lib().pt_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def params(width, height, spp, bounces=3, integrator=0, seed=1234, flags=0, shard_index=0, shard_count=1,
               pixel_order=0, tile_w=0, tile_h=0):
        p = L.Params()
        p.width, p.height, p.spp, p.bounces = int(width), int(height), int(spp), int(bounces)
        p.integrator, p.flags, p.seed = int(integrator), int(flags), int(seed)
        p.shard_index, p.shard_count = int(shard_index), int(shard_count)
        p.pixel_order, p.tile_w, p.tile_h = int(pixel_order), int(tile_w), int(tile_h)
        return p

    def render(self, cam, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
               shard_index=0, shard_count=1, pixel_order=0, tile_w=0, tile_h=0, out=None, view=None):
        """Returns (image float32, stats dict).  The image is (H, W, 3) in scanline order, or the
        reference's Morton-indexed imgBuff (W*H, 3) with pixel_order=PT_ORDER_MORTON.  `out`: a
        C-contiguous float32 array of W*H*3 values to render into (reused across frames).  `view`: an oriented
        camera (make_view / look_at); None is the reference camera.  So for every call below that takes one."""
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        shape = (height * width, 3) if pixel_order == L.PT_ORDER_MORTON else (height, width, 3)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.size != width * height * 3 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of W*H*3 values")
        st = L.Stats()
        L.check(L.lib().pt_render_view(self._h, C.byref(p), C.byref(cam), _view_ref(view), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def render_device(self, cam, d_out_ptr, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
                      shard_index=0, shard_count=1, stream_ptr=None, pixel_order=0, tile_w=0, tile_h=0, view=None):
        """Render this shard into a caller-owned, zero-filled device buffer (e.g. a torch tensor)."""
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        st = L.Stats()
        L.check(L.lib().pt_render_device_view(self._h, C.byref(p), C.byref(cam), _view_ref(view), C.c_void_p(int(d_out_ptr)),
                                              None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(st)))
        return st.as_dict()

    def render_device_async(self, cam, d_out_ptr, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
                            shard_index=0, shard_count=1, stream_ptr=None, pixel_order=0, tile_w=0, tile_h=0, view=None):
        """Enqueue render_device's work on the stream and return at once (at most 2 in flight); collect
        the stats of the oldest with wait()."""
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        L.check(L.lib().pt_render_device_view_async(self._h, C.byref(p), C.byref(cam), _view_ref(view),
                                                    C.c_void_p(int(d_out_ptr)),
                                                    None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def wait(self):
        """Stats dict of the oldest render in flight (render_device_async), once it has finished."""
        st = L.Stats()
        L.check(L.lib().pt_render_wait(self._h, C.byref(st)))
        return st.as_dict()

    def accumulator(self, cam, width, height, bounces=3, integrator=0, seed=1234, flags=0, shard_index=0,
                    shard_count=1, pixel_order=0, tile=0, view=None):
        """A resumable render of this shard (pt_accum_create): everything but the sample count is fixed
        here; Accumulator.add(spp) then renders the next spp samples of every pixel.  `tile`: the shard
        tile size, one int or (tile_w, tile_h); 0 = 8."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, bounces, integrator, seed, flags, shard_index, shard_count, pixel_order,
                        tw, th)
        err = C.c_int(0)
        h = L.lib().pt_accum_create_view(self._h, C.byref(p), C.byref(cam), _view_ref(view), C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Accumulator(self, h, p)

    def load_accumulator(self, path):
        """The accumulator a checkpoint file holds (pt_accum_load), on this renderer: the file names every
        fixed parameter, the camera and the scene it was written for (PtError PT_E_SCENE if not this one)."""
        err = C.c_int(0)
        h = L.lib().pt_accum_load(self._h, str(path).encode(), C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_IO)
        return Accumulator(self, h, accum_file_info(path)["params"])

    def load_session(self, path, noise=True):
        """(Accumulator, NoiseEstimate or None): the progressive state a session file holds (pt_session_load), on
        this renderer.  The estimator continues the saved window; None when the file has none.  noise=False skips
        the file's estimator: Accumulator.noise() then opens a fresh window.  PtError PT_E_SCENE for another scene."""
        acc, est, has = C.c_void_p(None), C.c_void_p(None), C.c_int(0)
        L.check(L.lib().pt_session_load(self._h, str(path).encode(), C.byref(acc), C.byref(est) if noise else None,
                                        C.byref(has)))
        a = Accumulator(self, acc.value, session_file_info(path)["params"])
        if est.value:
            a._noise = NoiseEstimate(a, est.value)
        return a, a._noise

    def features(self, cam, width, height, pixel_order=0, shard_index=0, shard_count=1, tile=0, view=None, flags=0):
        """Primary-hit feature buffers (pt_render_features): a FEATURE structured array of shape (H, W) -- (W*H,)
        in Morton order -- with albedo, depth, normal, prim and position of each pixel's pinhole camera ray.
        Pixels outside the shard are all zero with prim = -1.  `tile`: one int or (tile_w, tile_h); 0 = 8.
        `flags`: the render's; with PT_FLAG_JITTER the ray goes through the centre of the pixel's footprint."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, 1, 0, 0, flags, shard_index, shard_count, pixel_order, tw, th)
        shape = (height * width,) if pixel_order == L.PT_ORDER_MORTON else (height, width)
        out = np.zeros(shape, dtype=FEATURE)
        L.check(L.lib().pt_render_features_view(self._h, C.byref(p), C.byref(cam), _view_ref(view), out.ctypes.data))
        return out

    def features_device(self, cam, d_feat_ptr, width, height, pixel_order=0, shard_index=0, shard_count=1, tile=0,
                        stream_ptr=None, view=None, flags=0):
        """This shard's features into a caller-owned device buffer of W*H 48-byte records (16-byte aligned);
        records of other pixels are left untouched.  `flags` as for features()."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, 1, 0, 0, flags, shard_index, shard_count, pixel_order, tw, th)
        L.check(L.lib().pt_render_features_view_device(self._h, C.byref(p), C.byref(cam), _view_ref(view),
                                                       C.c_void_p(int(d_feat_ptr)),
                                                       None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    @staticmethod
    def denoise_params(iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0, demodulate=True):
        dp = L.DenoiseParams()
        dp.iterations, dp.normal_power_log2 = int(iterations), int(normal_power_log2)
        dp.sigma_depth, dp.sigma_color = float(sigma_depth), float(sigma_color)
        dp.flags = 0 if demodulate else L.PT_DENOISE_NO_DEMODULATE
        return dp

    def denoise(self, img, features, iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0,
                demodulate=True, pixel_order=0):
        """The edge-avoiding a-trous filter (pt_denoise) over a mean image as render returns it, guided by
        `features` (features() of the same size and pixel order); returns the filtered image, same shape."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        feat = np.ascontiguousarray(features, dtype=FEATURE)
        if pixel_order == L.PT_ORDER_MORTON:
            n = img.size // 3
            w = h = int(round(n ** 0.5))
        else:
            h, w = img.shape[:2]
        if feat.size != w * h or img.size != w * h * 3:
            raise ValueError("denoise: image and features differ in size")
        dp = self.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_color, demodulate)
        out = np.empty_like(img)
        L.check(L.lib().pt_denoise(self._h, C.byref(dp), w, h, int(pixel_order), img.ctypes.data, feat.ctypes.data,
                                   out.ctypes.data))
        return out

    def denoise_device(self, d_in_ptr, d_feat_ptr, d_out_ptr, width, height, iterations=5, normal_power_log2=5,
                       sigma_depth=0.02, sigma_color=0.0, demodulate=True, pixel_order=0, stream_ptr=None):
        """pt_denoise_device on raw device pointers (d_out_ptr may equal d_in_ptr); blocking."""
        dp = self.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_color, demodulate)
        L.check(L.lib().pt_denoise_device(self._h, C.byref(dp), int(width), int(height), int(pixel_order),
                                          C.c_void_p(int(d_in_ptr)), C.c_void_p(int(d_feat_ptr)),
                                          C.c_void_p(int(d_out_ptr)),
                                          None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    @staticmethod
    def denoise_guided_params(iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0, demodulate=True,
                              sigma_luma=2.0):
        gp = L.DenoiseGuidedParams()
        gp.base = Renderer.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_color, demodulate)
        gp.sigma_luma = float(sigma_luma)
        return gp

    def denoise_guided(self, img, features, var, iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0,
                       demodulate=True, pixel_order=0, sigma_luma=2.0):
        """The variance-guided a-trous filter (pt_denoise_guided): denoise() with a weight on the luminance
        difference measured against `var`, the variance of each pixel's mean luminance (NoiseEstimate.variance(), or
        any array shaped like the image without its channel axis; inf or NaN = unknown).  Where the estimate says a
        pixel has converged the filter leaves it alone."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        feat = np.ascontiguousarray(features, dtype=FEATURE)
        var = np.ascontiguousarray(var, dtype=np.float32)
        if pixel_order == L.PT_ORDER_MORTON:
            n = img.size // 3
            w = h = int(round(n ** 0.5))
        else:
            h, w = img.shape[:2]
        if feat.size != w * h or img.size != w * h * 3 or var.size != w * h:
            raise ValueError("denoise_guided: image, features and variance differ in size")
        gp = self.denoise_guided_params(iterations, normal_power_log2, sigma_depth, sigma_color, demodulate, sigma_luma)
        out = np.empty_like(img)
        L.check(L.lib().pt_denoise_guided(self._h, C.byref(gp), w, h, int(pixel_order), img.ctypes.data, feat.ctypes.data,
                                          var.ctypes.data, out.ctypes.data))
        return out

    def denoise_guided_device(self, d_in_ptr, d_feat_ptr, d_var_ptr, d_out_ptr, width, height, iterations=5,
                              normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0, demodulate=True, pixel_order=0,
                              sigma_luma=2.0, stream_ptr=None):
        """pt_denoise_guided_device on raw device pointers (d_out_ptr may equal d_in_ptr); blocking."""
        gp = self.denoise_guided_params(iterations, normal_power_log2, sigma_depth, sigma_color, demodulate, sigma_luma)
        L.check(L.lib().pt_denoise_guided_device(self._h, C.byref(gp), int(width), int(height), int(pixel_order),
                                                 C.c_void_p(int(d_in_ptr)), C.c_void_p(int(d_feat_ptr)),
                                                 C.c_void_p(int(d_var_ptr)), C.c_void_p(int(d_out_ptr)),
                                                 None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def temporal(self, width, height, max_history=32, normal_min=0.9, plane_tol=0.02, pixel_order=0):
        """A temporal history for width x height images (pt_temporal_create): Temporal.push(img, features, cam, view)
        reprojects what it holds through the previous push's camera and accumulates the new frame into it, so the
        samples survive a camera move.  Close it before its renderer."""
        tp = L.TemporalParams()
        tp.max_history, tp.normal_min, tp.plane_tol, tp.flags = int(max_history), float(normal_min), float(plane_tol), 0
        err = C.c_int(0)
        h = L.lib().pt_temporal_create(self._h, C.byref(tp), int(width), int(height), int(pixel_order), C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Temporal(self, h, int(width), int(height), int(pixel_order))

    def tonemap(self, img):
        """Output step on the GPU: (H, W, 3) float32 mean image -> int32 codes equal to
        pt_tonemap_u8 (kernel.cu:763-778) per channel."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        h, w = img.shape[:2]
        codes = np.empty(img.shape, dtype=np.int32)
        L.check(L.lib().pt_tonemap(self._h, img.ctypes.data, w, h, codes.ctypes.data))
        return codes

    def tri_counts(self):
        """Per-triangle test counts (uint32[num_tris], original ids) of the last render with
        PT_FLAG_COUNT -- the reference's test[] buffer (kernel.cu:133, :694-697)."""
        n = int(self._scene_view.num_tris)
        out = np.zeros(n, dtype=np.uint32)
        L.check(L.lib().pt_tri_counts(self._h, out.ctypes.data, n))
        return out

    def trace_counts(self, origins, directions, reference_bvh=False):
        """trace() plus diagnostics: returns (tri, t, tri_counts uint32[num_tris], spill_entries)."""
        rays, n = self._rays(origins, directions)
        tri = np.empty(n, dtype=np.int32)
        t = np.empty(n, dtype=np.float32)
        counts = np.zeros(int(self._scene_view.num_tris), dtype=np.uint32)
        spills = C.c_uint64(0)
        L.check(L.lib().pt_trace_counts(self._h, n, rays.ctypes.data, tri.ctypes.data, t.ctypes.data,
                                        L.PT_FLAG_REFERENCE_BVH if reference_bvh else 0, counts.ctypes.data,
                                        C.byref(spills)))
        return tri, t, counts, int(spills.value)

    @staticmethod
    def _rays(origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions differ in shape")
        return np.ascontiguousarray(np.concatenate([o, d], axis=1)), len(o)

    def trace(self, origins, directions, reference_bvh=False):
        """The reference's trace() (kernel.cu:112-161) for a batch of rays: returns
        (tri int32[n] original triangle index or -1, t float32[n] closestT, 1e5 on a miss)."""
        rays, n = self._rays(origins, directions)
        tri = np.empty(n, dtype=np.int32)
        t = np.empty(n, dtype=np.float32)
        L.check(L.lib().pt_trace(self._h, n, rays.ctypes.data, tri.ctypes.data, t.ctypes.data,
                                 L.PT_FLAG_REFERENCE_BVH if reference_bvh else 0))
        return tri, t

    def trace_device(self, d_rays_ptr, n, d_tri_ptr, d_t_ptr, reference_bvh=False, stream_ptr=None):
        """pt_trace_device on raw device pointers: trace() for n rays {o.xyz, d.xyz} (float32[6n]) into int32[n]
        triangle ids and float32[n] distances, bit for bit what trace() returns; blocking."""
        L.check(L.lib().pt_trace_device(self._h, int(n), C.c_void_p(int(d_rays_ptr)), C.c_void_p(int(d_tri_ptr)),
                                        C.c_void_p(int(d_t_ptr)), L.PT_FLAG_REFERENCE_BVH if reference_bvh else 0,
                                        None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def occluded(self, origins, directions, tmax=None):
        """Is the segment of ray i up to tmax[i] blocked?  bool[n]: (tri >= 0) & (t < tmax) of trace(), in float32,
        answered without computing the closest hit.  tmax=None: any hit (1e5)."""
        rays, n = self._rays(origins, directions)
        occ = np.zeros(n, dtype=np.uint8)
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if len(tm) != n:
                raise ValueError("tmax needs one entry per ray")
        L.check(L.lib().pt_occluded(self._h, n, rays.ctypes.data, None if tm is None else tm.ctypes.data, occ.ctypes.data, 0))
        return occ.astype(bool)

    def occluded_device(self, d_rays_ptr, n, d_occ_ptr, d_tmax_ptr=None, stream_ptr=None):
        """pt_occluded_device on raw device pointers: uint8[n] answers (0 or 1) for n rays (float32[6n]) and their
        float32[n] bounds (None: 1e5 for every ray); blocking."""
        L.check(L.lib().pt_occluded_device(self._h, int(n), C.c_void_p(int(d_rays_ptr)),
                                           None if d_tmax_ptr is None else C.c_void_p(int(d_tmax_ptr)),
                                           C.c_void_p(int(d_occ_ptr)), 0,
                                           None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def render_rays(self, origins, directions, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
                    shard_index=0, shard_count=1, pixel_order=0, tile_w=0, tile_h=0, out=None):
        """Render along the caller's rays instead of a camera's (pt_render_rays): any projection, probes, baking.
        origins, directions: W*H float32 triples, the ray of pixel (x, y) at its index in `pixel_order` (y*W + x, or
        the Morton index); cudapathtracer_amd.rays builds common sets.  Returns (image, stats) as render().  Pixel
        (x, y) is the mean of spp samples of the integrator down its ray, seeded as render() seeds the pixel; no sample
        draws a lens pair, so the camera's own rays (rays.camera_rays) give render()'s image bit for bit except at
        pixel (0, 0).  A ray with a non-finite component or a zero direction is refused (PtError PT_E_INVALID naming
        the pixel).  A ray farther out than 64 scene extents, or a direction longer than a normalised one (d.d > 1 +
        2^-10), sends THE WHOLE RENDER to the tile kernel with the reference's own walk: exact, but much slower
        (stats["work_units"] == 0 shows that it happened).  flags: 0, PT_FLAG_NO_DEAD_PATH_SKIP,
        PT_FLAG_NO_PRIMARY_CACHE, PT_FLAG_REFERENCE_TRAVERSAL, PT_FLAG_REFERENCE_BVH."""
        rays, n = self._rays(origins, directions)
        if n != int(width) * int(height):
            raise ValueError("render_rays: %d rays for a %dx%d image" % (n, width, height))
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        shape = (height * width, 3) if pixel_order == L.PT_ORDER_MORTON else (height, width, 3)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.size != width * height * 3 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of W*H*3 values")
        st = L.Stats()
        L.check(L.lib().pt_render_rays(self._h, C.byref(p), rays.ctypes.data, out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def render_rays_device(self, d_rays_ptr, d_out_ptr, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
                           shard_index=0, shard_count=1, pixel_order=0, tile_w=0, tile_h=0, stream_ptr=None):
        """pt_render_rays_device on raw device pointers (e.g. torch tensors): W*H rays {o.xyz, d.xyz} (float32[6*W*H],
        8-byte aligned) into this shard's pixels of a caller-owned float32[W*H*3] buffer; blocking; returns the stats.
        Everything else as render_rays(), the whole-render fall-back for far or unnormalised rays included."""
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        st = L.Stats()
        L.check(L.lib().pt_render_rays_device(self._h, C.byref(p), C.c_void_p(int(d_rays_ptr)), C.c_void_p(int(d_out_ptr)),
                                              None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(st)))
        return st.as_dict()

    def accumulator_rays(self, origins, directions, width, height, bounces=3, integrator=0, seed=1234, flags=0,
                         shard_index=0, shard_count=1, pixel_order=0, tile=0):
        """A resumable render of this shard along the caller's rays (pt_accum_create_rays): accumulator() with the
        camera replaced by W*H rays indexed as for render_rays().  The accumulator copies the rays and keeps them for
        life.  add() in any split of passes equals render_rays() of the same total in every bit; noise estimates,
        add_until, add_adaptive and freeze work as on a camera accumulator, and freeze() at 0 samples masks pixels (a
        masked pixel still needs a valid ray).  Every ray must be regular: a far or unnormalised ray is refused here
        (PtError PT_E_INVALID; render_rays takes such a buffer).  flags: 0, PT_FLAG_NO_DEAD_PATH_SKIP,
        PT_FLAG_NO_PRIMARY_CACHE.  save() and save_session() are refused."""
        rays, n = self._rays(origins, directions)
        if n != int(width) * int(height):
            raise ValueError("accumulator_rays: %d rays for a %dx%d image" % (n, width, height))
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, bounces, integrator, seed, flags, shard_index, shard_count, pixel_order, tw, th)
        err = C.c_int(0)
        h = L.lib().pt_accum_create_rays(self._h, C.byref(p), rays.ctypes.data, C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Accumulator(self, h, p)

    def accumulator_rays_device(self, d_rays_ptr, width, height, bounces=3, integrator=0, seed=1234, flags=0,
                                shard_index=0, shard_count=1, pixel_order=0, tile=0, stream_ptr=None):
        """accumulator_rays() over W*H rays on the device (float32[6*W*H], 8-byte aligned; pt_accum_create_rays_device).
        The buffer is copied: it may be freed or overwritten once this returns."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, bounces, integrator, seed, flags, shard_index, shard_count, pixel_order, tw, th)
        err = C.c_int(0)
        h = L.lib().pt_accum_create_rays_device(self._h, C.byref(p), C.c_void_p(int(d_rays_ptr)),
                                                None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Accumulator(self, h, p)

    def accumulator_points(self, points, normals, width, height, bounces=3, integrator=0, seed=1234, flags=0,
                           shard_index=0, shard_count=1, pixel_order=0, tile=0):
        """A resumable irradiance render of this shard at the caller's points (pt_accum_create_points): a progressive
        bake.  accumulator_rays() with the rays replaced by W*H points {p, n} indexed as for render_irradiance(); the
        accumulator copies the points and keeps them for life.  add() in any split of passes equals
        render_irradiance() of the same total in every bit; noise estimates, add_until, add_adaptive and freeze work
        as on a camera accumulator, and freeze() at 0 samples masks texels (rays.chart_points names the uncovered
        ones; a masked texel still needs a valid point).  Every point must be regular: one beyond 64 scene extents is
        refused here (PtError PT_E_INVALID; render_irradiance takes such a buffer).  flags: 0,
        PT_FLAG_NO_DEAD_PATH_SKIP, PT_FLAG_NO_PRIMARY_CACHE (which changes nothing).  save() and save_session() are
        refused."""
        pts, n = self._rays(points, normals)
        if n != int(width) * int(height):
            raise ValueError("accumulator_points: %d points for a %dx%d image" % (n, width, height))
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, bounces, integrator, seed, flags, shard_index, shard_count, pixel_order, tw, th)
        err = C.c_int(0)
        h = L.lib().pt_accum_create_points(self._h, C.byref(p), pts.ctypes.data, C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Accumulator(self, h, p)

    def accumulator_points_device(self, d_points_ptr, width, height, bounces=3, integrator=0, seed=1234, flags=0,
                                  shard_index=0, shard_count=1, pixel_order=0, tile=0, stream_ptr=None):
        """accumulator_points() over W*H points on the device (float32[6*W*H], 8-byte aligned;
        pt_accum_create_points_device).  The buffer is copied: it may be freed or overwritten once this returns."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, bounces, integrator, seed, flags, shard_index, shard_count, pixel_order, tw, th)
        err = C.c_int(0)
        h = L.lib().pt_accum_create_points_device(self._h, C.byref(p), C.c_void_p(int(d_points_ptr)),
                                                  None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        return Accumulator(self, h, p)

    def features_rays(self, origins, directions, width, height, pixel_order=0, shard_index=0, shard_count=1, tile=0):
        """Feature buffers of the caller's rays (pt_render_features_rays): features() with each pixel's ray taken from
        the buffer as it stands.  depth is the hit distance along the given direction, in units of its length;
        position = o + d * depth.  Far and unnormalised rays are legal; an invalid ray refuses the call."""
        rays, n = self._rays(origins, directions)
        if n != int(width) * int(height):
            raise ValueError("features_rays: %d rays for a %dx%d image" % (n, width, height))
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, 1, 0, 0, 0, shard_index, shard_count, pixel_order, tw, th)
        shape = (height * width,) if pixel_order == L.PT_ORDER_MORTON else (height, width)
        out = np.zeros(shape, dtype=FEATURE)
        L.check(L.lib().pt_render_features_rays(self._h, C.byref(p), rays.ctypes.data, out.ctypes.data))
        return out

    def features_rays_device(self, d_rays_ptr, d_feat_ptr, width, height, pixel_order=0, shard_index=0, shard_count=1,
                             tile=0, stream_ptr=None):
        """This shard's ray features into a caller-owned device buffer of W*H 48-byte records (16-byte aligned), from
        W*H rays on the device (8-byte aligned); records of other pixels are left untouched."""
        tw, th = (tile, tile) if np.isscalar(tile) else tile
        p = self.params(width, height, 0, 1, 0, 0, 0, shard_index, shard_count, pixel_order, tw, th)
        L.check(L.lib().pt_render_features_rays_device(self._h, C.byref(p), C.c_void_p(int(d_rays_ptr)),
                                                       C.c_void_p(int(d_feat_ptr)),
                                                       None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def classify_rays_device(self, d_rays_ptr, n, stream_ptr=None):
        """The classes of n rays on the device (pt_rays_classify_device), as render_rays* sorts them: a dict of
        regular, irregular, invalid (counts) and first_invalid (lowest invalid index, 0xffffffff for none)."""
        rc = L.RayClasses()
        L.check(L.lib().pt_rays_classify_device(self._h, int(n), None if not d_rays_ptr else C.c_void_p(int(d_rays_ptr)),
                                                None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(rc)))
        return dict(regular=int(rc.regular), irregular=int(rc.irregular), invalid=int(rc.invalid),
                    first_invalid=int(rc.first_invalid))

    def render_irradiance(self, points, normals, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0,
                          shard_index=0, shard_count=1, pixel_order=0, tile_w=0, tile_h=0, out=None):
        """An irradiance render (pt_render_irradiance): every sample of pixel (x, y) leaves its point along a fresh
        cosine-weighted direction about its normal (the bounces' own cosineWeightedRay, its pair drawn first), so the
        pixel is the cosine-weighted mean of the incoming radiance, E / pi; a Lambertian texel's outgoing radiance is
        its albedo times that.  points, normals: W*H float32 triples indexed as render_rays' rays
        (cudapathtracer_amd.rays has grid_points, triangle_points, feature_points).  A point is used as given: lift it
        off its surface, or the integrator's self-hit rule (a first hit nearer than 0.002 zeroes the path) blackens
        it.  A non-finite component or a normal whose squared length is outside 1 +- 2^-10 is refused (PtError
        PT_E_INVALID naming the pixel); one point beyond 64 scene extents sends THE WHOLE RENDER to the slow exact tile
        kernel (stats["work_units"] == 0).  flags as render_rays; PT_FLAG_NO_PRIMARY_CACHE changes nothing.  Returns
        (image, stats)."""
        pts, n = self._rays(points, normals)
        if n != int(width) * int(height):
            raise ValueError("render_irradiance: %d points for a %dx%d image" % (n, width, height))
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        shape = (height * width, 3) if pixel_order == L.PT_ORDER_MORTON else (height, width, 3)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.size != width * height * 3 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of W*H*3 values")
        st = L.Stats()
        L.check(L.lib().pt_render_irradiance(self._h, C.byref(p), pts.ctypes.data, out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def render_irradiance_device(self, d_points_ptr, d_out_ptr, width, height, spp, bounces=3, integrator=0, seed=1234,
                                 flags=0, shard_index=0, shard_count=1, pixel_order=0, tile_w=0, tile_h=0, stream_ptr=None):
        """pt_render_irradiance_device on raw device pointers: W*H points {p.xyz, n.xyz} (float32[6*W*H], 8-byte
        aligned) into this shard's pixels of a caller-owned float32[W*H*3] buffer; blocking; returns the stats.
        Everything else as render_irradiance()."""
        p = self.params(width, height, spp, bounces, integrator, seed, flags, shard_index, shard_count,
                        pixel_order, tile_w, tile_h)
        st = L.Stats()
        L.check(L.lib().pt_render_irradiance_device(self._h, C.byref(p), C.c_void_p(int(d_points_ptr)),
                                                    C.c_void_p(int(d_out_ptr)),
                                                    None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(st)))
        return st.as_dict()

    def classify_points_device(self, d_points_ptr, n, stream_ptr=None):
        """The classes of n points on the device (pt_points_classify_device), as render_irradiance* sorts them: the
        dict of classify_rays_device."""
        rc = L.RayClasses()
        L.check(L.lib().pt_points_classify_device(self._h, int(n), None if not d_points_ptr else C.c_void_p(int(d_points_ptr)),
                                                  None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(rc)))
        return dict(regular=int(rc.regular), irregular=int(rc.irregular), invalid=int(rc.invalid),
                    first_invalid=int(rc.first_invalid))

    def lightmap_dilate(self, img, covered, radius, return_src=False):
        """The gutter fill that ends a bake (pt_lightmap_dilate): every uncovered texel of the (H, W, 3) float32 lightmap
        `img` takes the value of the nearest covered one within `radius` (0..16) texels in x and in y -- smallest
        i*i + j*j, ties to the smaller j, then the smaller i; no wrap-around -- bit for bit; covered texels, and
        uncovered ones with nothing in reach, keep theirs.  covered: (H, W), non-zero = covered (rays.chart_points'
        `covered`).  Returns the filled lightmap; with return_src also the (H, W) int32 index y*W + x each texel was
        taken from (its own for a covered one, -1 where nothing was in reach)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("lightmap_dilate: the lightmap must have shape (H, W, 3)")
        h, w = img.shape[:2]
        cov = np.ascontiguousarray(np.asarray(covered) != 0, dtype=np.uint8)
        if cov.size != w * h:
            raise ValueError("lightmap_dilate: lightmap and covered differ in size")
        out = np.empty_like(img)
        src = np.empty((h, w), dtype=np.int32) if return_src else None
        L.check(L.lib().pt_lightmap_dilate(self._h, w, h, int(radius), img.ctypes.data, cov.ctypes.data, out.ctypes.data,
                                           None if src is None else src.ctypes.data))
        return (out, src) if return_src else out

    def lightmap_dilate_device(self, d_in_ptr, d_covered_ptr, d_out_ptr, width, height, radius, d_src_ptr=None,
                               stream_ptr=None):
        """pt_lightmap_dilate_device on raw device pointers: W*H*3 float32 in and out (d_out_ptr may equal d_in_ptr), W*H
        covered bytes, optionally W*H int32 sources; blocking."""
        L.check(L.lib().pt_lightmap_dilate_device(self._h, int(width), int(height), int(radius),
                                                  None if not d_in_ptr else C.c_void_p(int(d_in_ptr)),
                                                  None if not d_covered_ptr else C.c_void_p(int(d_covered_ptr)),
                                                  None if not d_out_ptr else C.c_void_p(int(d_out_ptr)),
                                                  None if not d_src_ptr else C.c_void_p(int(d_src_ptr)),
                                                  None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    @staticmethod
    def lightmap_params(fill=(0.0, 0.0, 0.0), flags=0):
        lp = L.LightmapParams()
        lp.fill[0], lp.fill[1], lp.fill[2] = (float(v) for v in fill)
        lp.flags = int(flags)
        return lp

    def lightmap_shade(self, features, tri_uv, lightmap, fill=(0.0, 0.0, 0.0), flags=0):
        """A lightmapped view (pt_lightmap_shade): the colour of every record of a feature buffer (features(),
        features_rays(): any view, jitter or ray set) under the (H, W, 3) float32 `lightmap`, looked up bilinearly at the
        chart coordinates of the record's hit and multiplied by its albedo (PT_LIGHTMAP_NO_ALBEDO in flags: the value
        alone).  tri_uv: (num_tris, 6) float32, the chart coordinates of v0, v1, v2 of every original triangle, a NaN
        row for a triangle of no chart (rays.chart_uv_table).  Misses, emitters, spheres and triangles of no chart get
        `fill`.  Returns float32 of the features' shape + (3,)."""
        feat = np.ascontiguousarray(features, dtype=FEATURE)
        uv = np.ascontiguousarray(tri_uv, dtype=np.float32)
        lm = np.ascontiguousarray(lightmap, dtype=np.float32)
        if lm.ndim != 3 or lm.shape[2] != 3:
            raise ValueError("lightmap_shade: the lightmap must have shape (H, W, 3)")
        nt = int(self._scene_view.num_tris)
        if uv.size != nt * 6:
            raise ValueError("lightmap_shade: tri_uv must have shape (%d, 6)" % nt)
        lp = self.lightmap_params(fill, flags)
        out = np.zeros(feat.shape + (3,), dtype=np.float32)
        L.check(L.lib().pt_lightmap_shade(self._h, C.byref(lp), feat.size, feat.ctypes.data, uv.ctypes.data, lm.ctypes.data,
                                          lm.shape[1], lm.shape[0], out.ctypes.data))
        return out

    def lightmap_shade_device(self, d_feat_ptr, n, d_tri_uv_ptr, d_map_ptr, map_w, map_h, d_out_ptr, fill=(0.0, 0.0, 0.0),
                              flags=0, stream_ptr=None):
        """pt_lightmap_shade_device on raw device pointers: n 48-byte feature records (16-byte aligned), num_tris * 6
        float32 chart coordinates, map_w * map_h * 3 float32 lightmap, n * 3 float32 out; blocking."""
        lp = self.lightmap_params(fill, flags)
        L.check(L.lib().pt_lightmap_shade_device(self._h, C.byref(lp), int(n),
                                                 None if not d_feat_ptr else C.c_void_p(int(d_feat_ptr)),
                                                 None if not d_tri_uv_ptr else C.c_void_p(int(d_tri_uv_ptr)),
                                                 None if not d_map_ptr else C.c_void_p(int(d_map_ptr)), int(map_w), int(map_h),
                                                 None if not d_out_ptr else C.c_void_p(int(d_out_ptr)),
                                                 None if stream_ptr is None else C.c_void_p(int(stream_ptr))))


def accum_file_info(path):
    """Header of a checkpoint file (pt_accum_file_info, host-only): dict of params (spp = 0), camera,
    samples done and the scene digest."""
    p, cam, n, dg = L.Params(), L.Camera(), C.c_int64(0), C.c_uint64(0)
    L.check(L.lib().pt_accum_file_info(str(path).encode(), C.byref(p), C.byref(cam), C.byref(n), C.byref(dg)))
    return dict(params=p, camera=cam, samples=int(n.value), scene_digest=int(dg.value))


def session_file_info(path):
    """Header of a session file (pt_session_file_info, host-only): dict of params (spp = 0), camera, samples, the
    scene digest, flags (PT_SESSION_*), the estimator's noise_n0 / noise_W / noise_batches and frozen_pixels."""
    i = L.SessionInfo()
    L.check(L.lib().pt_session_file_info(str(path).encode(), C.byref(i)))
    return dict(params=i.params, camera=i.cam, samples=int(i.samples), scene_digest=int(i.scene_digest), flags=int(i.flags),
                noise_n0=int(i.noise_n0), noise_W=float(i.noise_W), noise_batches=int(i.noise_batches),
                frozen_pixels=int(i.frozen_pixels))


def session_file_view(path):
    """The view a session file holds (pt_session_file_view, host-only): a pt_view, or None for a file without one
    (format version 2)."""
    v, has = L.View(), C.c_int(0)
    L.check(L.lib().pt_session_file_view(str(path).encode(), C.byref(v), C.byref(has)))
    return v if has.value else None


class Accumulator:
    """Per-pixel XORWOW state and f64 running mean of one shard, kept on the renderer's device between
    passes (the reference's randState_device / imgBuffer_device, kernel.cu:527-553): a render built up
    with add() equals Renderer.render of the same total in every bit.  Close it before its renderer."""

    def __init__(self, renderer, handle, params):
        self._renderer = renderer   # (keeps the context alive as long as the accumulator)
        self._h = handle
        self.params = params
        self._noise = None          # the live NoiseEstimate, if any (closed before the accumulator)

    def close(self):
        if self._noise is not None:
            self._noise.close()
        if self._h:
            L.lib().pt_accum_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, spp, d_out_ptr=None, stream_ptr=None):
        """Render the next spp samples of every pixel; returns this pass's stats dict.  d_out_ptr: a device
        buffer of W*H*3 float32 that receives this shard's fp32 mean (other pixels untouched)."""
        st = L.Stats()
        L.check(L.lib().pt_accum_add(self._h, int(spp), None if d_out_ptr is None else C.c_void_p(int(d_out_ptr)),
                                     None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(st)))
        return st.as_dict()

    @property
    def samples(self):
        return int(L.lib().pt_accum_samples(self._h))

    @property
    def view(self):
        """The view the accumulator was created with (pt_accum_view), or None for the reference camera."""
        v, has = L.View(), C.c_int(0)
        L.check(L.lib().pt_accum_view(self._h, C.byref(v), C.byref(has)))
        return v if has.value else None

    @property
    def has_rays(self):
        """Whether the accumulator was built over a ray buffer (Renderer.accumulator_rays*; pt_accum_has_rays)."""
        return bool(L.lib().pt_accum_has_rays(self._h))

    @property
    def has_points(self):
        """Whether the accumulator was built over a point buffer (Renderer.accumulator_points*; pt_accum_has_points)."""
        return bool(L.lib().pt_accum_has_points(self._h))

    def _shape(self):
        p = self.params
        return (p.height * p.width, 3) if p.pixel_order == L.PT_ORDER_MORTON else (p.height, p.width, 3)

    def image(self):
        """The fp32 mean image as Renderer.render returns it (pixels outside the shard 0)."""
        out = np.zeros(self._shape(), dtype=np.float32)
        L.check(L.lib().pt_accum_read(self._h, out.ctypes.data, None))
        return out

    def mean64(self):
        """The f64 running mean itself (the reference's imgBuffer)."""
        out = np.zeros(self._shape(), dtype=np.float64)
        L.check(L.lib().pt_accum_read(self._h, None, out.ctypes.data))
        return out

    def save(self, path):
        L.check(L.lib().pt_accum_save(self._h, str(path).encode()))

    def save_session(self, path, noise=None):
        """Write the whole progressive state to a session file (pt_session_save): the accumulator, the frozen pixels'
        counts and, with noise = this accumulator's live NoiseEstimate, the estimator and its window."""
        L.check(L.lib().pt_session_save(self._h, None if noise is None else noise._h, str(path).encode()))

    def noise(self):
        """Attach a noise estimator (pt_noise_create): its window starts at the samples done so far.  One live
        estimator per accumulator; closing the accumulator closes it."""
        err = C.c_int(0)
        h = L.lib().pt_noise_create(self._h, C.byref(err))
        if not h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)
        self._noise = NoiseEstimate(self, h)
        return self._noise

    def add_until(self, pass_spp, max_samples, tol=None, quantile=0.95, min_batches=2, y_floor=None, d_out_ptr=None,
                  stream_ptr=None):
        """Add passes of pass_spp samples until `quantile` of the pixels have a relative standard error <= tol
        (after at least min_batches passes), or the total reaches max_samples (pt_accum_add_until).  Uses the
        live estimator, or attaches one.  Returns dict(passes, stopped_converged, samples, summary)."""
        est = self._noise if self._noise is not None else self.noise()
        cp = L.ConvergeParams()
        cp.pass_spp, cp.max_samples, cp.min_batches = int(pass_spp), int(max_samples), int(min_batches)
        cp.quantile = float(quantile)
        cp.noise = _noise_params(tol, y_floor)
        res = L.ConvergeResult()
        L.check(L.lib().pt_accum_add_until(self._h, est._h, C.byref(cp),
                                           None if d_out_ptr is None else C.c_void_p(int(d_out_ptr)),
                                           None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(res)))
        return dict(passes=int(res.passes), stopped_converged=bool(res.stopped_converged), samples=self.samples,
                    summary=res.last.as_dict())

    def freeze(self, mask):
        """Freeze the pixels where `mask` (shaped like the image without its channel axis) is non-zero: they are
        never sampled again, and add() renders the others only (pt_accum_freeze).  Permanent; zeros change nothing."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.size != self.params.width * self.params.height:
            raise ValueError("mask of %d entries for a %dx%d image" % (m.size, self.params.width, self.params.height))
        L.check(L.lib().pt_accum_freeze(self._h, m.ctypes.data))

    def counts(self):
        """Every pixel's sample count, uint32, shaped like the image without its channel axis (outside the shard 0)."""
        out = np.zeros(self._shape()[:-1], dtype=np.uint32)
        L.check(L.lib().pt_accum_counts(self._h, out.ctypes.data))
        return out

    def active_pixels(self):
        """The scanline ids y*W + x of the pixels still sampled, in work order (the device's active list)."""
        n = C.c_uint64(0)
        L.check(L.lib().pt_accum_active(self._h, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint32)
        if out.size:
            L.check(L.lib().pt_accum_active(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out

    def add_adaptive(self, pass_spp, max_samples, tol=None, quantile=0.95, min_batches=2, y_floor=None, d_out_ptr=None,
                     stream_ptr=None):
        """add_until that freezes every pixel once its relative standard error is <= tol and samples only the rest
        (pt_accum_add_adaptive).  Returns dict(passes, stopped_converged, samples, summary, active, samples_total)."""
        est = self._noise if self._noise is not None else self.noise()
        cp = L.ConvergeParams()
        cp.pass_spp, cp.max_samples, cp.min_batches = int(pass_spp), int(max_samples), int(min_batches)
        cp.quantile = float(quantile)
        cp.noise = _noise_params(tol, y_floor)
        res = L.AdaptiveResult()
        L.check(L.lib().pt_accum_add_adaptive(self._h, est._h, C.byref(cp),
                                              None if d_out_ptr is None else C.c_void_p(int(d_out_ptr)),
                                              None if stream_ptr is None else C.c_void_p(int(stream_ptr)), C.byref(res)))
        return dict(passes=int(res.passes), stopped_converged=bool(res.stopped_converged), samples=self.samples,
                    summary=res.last.as_dict(), active=int(res.active), samples_total=int(res.samples_total))


class NoiseEstimate:
    """Per-pixel noise estimate of an accumulator (pt_noise_*): batch means of the passes added since it was
    attached give the variance of each pixel's mean luminance; update() folds the newest pass and counts the
    converged pixels in the same sweep."""

    def __init__(self, accumulator, handle):
        self._acc = accumulator
        self._h = handle

    def close(self):
        if self._h:
            L.lib().pt_noise_destroy(self._h)
            self._h = None
            if self._acc._noise is self:
                self._acc._noise = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self):
        p = self._acc.params
        return (p.height * p.width,) if p.pixel_order == L.PT_ORDER_MORTON else (p.height, p.width)

    def update(self, tol=None, y_floor=None, stream_ptr=None):
        """Fold the samples added since the last update (if any) and return the summary dict: samples, batches,
        pixels, converged (relative standard error <= tol) and the 64-bin histogram of the squared error."""
        np_ = _noise_params(tol, y_floor)
        s = L.NoiseSummary()
        L.check(L.lib().pt_noise_update(self._h, C.byref(np_), None if stream_ptr is None else C.c_void_p(int(stream_ptr)),
                                        C.byref(s)))
        return s.as_dict()

    def freeze(self, tol=None, y_floor=None, stream_ptr=None):
        """Freeze every active pixel whose relative standard error is <= tol, on the device (pt_noise_freeze).
        Returns (newly_frozen, active)."""
        np_ = _noise_params(tol, y_floor)
        newly, active = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().pt_noise_freeze(self._h, C.byref(np_), None if stream_ptr is None else C.c_void_p(int(stream_ptr)),
                                        C.byref(newly), C.byref(active)))
        return int(newly.value), int(active.value)

    def read(self):
        """(mu, m2): the window's mean luminance and weighted sum of squared deviations, float64, shaped like the
        image without its channel axis (pixels outside the shard 0)."""
        mu, m2 = np.zeros(self._shape(), dtype=np.float64), np.zeros(self._shape(), dtype=np.float64)
        L.check(L.lib().pt_noise_read(self._h, mu.ctypes.data, m2.ctypes.data))
        return mu, m2

    def error_map(self, y_floor=None):
        """The squared relative standard error of every pixel's mean luminance, float32 (inf before two batches;
        pixels outside the shard 0)."""
        np_ = _noise_params(None, y_floor)
        out = np.zeros(self._shape(), dtype=np.float32)
        L.check(L.lib().pt_noise_map(self._h, C.byref(np_), out.ctypes.data))
        return out


    def variance(self):
        """The estimated variance of every pixel's mean luminance over all of its samples, float32 (pt_noise_variance:
        inf before two batches; pixels outside the shard 0): what Renderer.denoise_guided takes.  Reads the state of
        the last update()."""
        out = np.zeros(self._shape(), dtype=np.float32)
        L.check(L.lib().pt_noise_variance(self._h, out.ctypes.data))
        return out

    def variance_device(self, d_var_ptr, stream_ptr=None):
        """variance() into a device buffer of W*H float32; pixels outside the shard are left untouched."""
        L.check(L.lib().pt_noise_variance_device(self._h, C.c_void_p(int(d_var_ptr)),
                                                 None if stream_ptr is None else C.c_void_p(int(stream_ptr))))


class Temporal:
    """A temporal history of the image on the renderer's device (pt_temporal_*): every push reprojects it through the
    previous push's camera, folds the new frame in and returns the accumulated image with the variance of each pixel's
    mean luminance (inf = unknown), which Renderer.denoise_guided takes as it stands."""

    def __init__(self, renderer, handle, width, height, pixel_order):
        self._renderer = renderer   # (keeps the context alive as long as the history)
        self._h = handle
        self.width, self.height, self.pixel_order = width, height, pixel_order

    def close(self):
        if self._h:
            L.lib().pt_temporal_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self):
        return (self.height * self.width,) if self.pixel_order == L.PT_ORDER_MORTON else (self.height, self.width)

    def push(self, img, features, cam, view=None, flags=0):
        """(out, var) of the frame `img` with its `features` (features() through the same cam, view and flags), both
        in the history's pixel order: the accumulated image, shaped like img, and the variance of each pixel's mean
        luminance (float32, img's shape without the channel axis; inf where fewer than 2 samples are held).  Of
        `flags` only PT_FLAG_JITTER counts: the features were taken through the pixels' centres."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        feat = np.ascontiguousarray(features, dtype=FEATURE)
        n = self.width * self.height
        if feat.size != n or img.size != n * 3:
            raise ValueError("push: image or features are not %dx%d" % (self.width, self.height))
        out = np.empty_like(img)
        var = np.empty(self._shape(), dtype=np.float32)
        L.check(L.lib().pt_temporal_push(self._h, C.byref(cam), _view_ref(view), int(flags), img.ctypes.data, feat.ctypes.data,
                                         out.ctypes.data, var.ctypes.data))
        return out, var

    def push_device(self, d_in_ptr, d_feat_ptr, d_out_ptr, cam, view=None, flags=0, d_var_ptr=None, stream_ptr=None):
        """pt_temporal_push_device on raw device pointers (d_out_ptr may equal d_in_ptr, d_var_ptr may be None);
        blocking."""
        L.check(L.lib().pt_temporal_push_device(self._h, C.byref(cam), _view_ref(view), int(flags), C.c_void_p(int(d_in_ptr)),
                                                C.c_void_p(int(d_feat_ptr)), C.c_void_p(int(d_out_ptr)),
                                                None if d_var_ptr is None else C.c_void_p(int(d_var_ptr)),
                                                None if stream_ptr is None else C.c_void_p(int(stream_ptr))))

    def history_length(self):
        """The history length n' of every pixel as of the last push, float32 (all 0 before the first)."""
        out = np.zeros(self._shape(), dtype=np.float32)
        L.check(L.lib().pt_temporal_length(self._h, out.ctypes.data))
        return out

    @property
    def frames(self):
        """The pushes since the history was created or reset."""
        return int(L.lib().pt_temporal_frames(self._h))

    def reset(self):
        """Forget the history: the next push is a first push."""
        L.check(L.lib().pt_temporal_reset(self._h))


class Group:
    """One process, N GPUs (pt_group_*): renderer i renders image-tile shard i of N, and one RCCL
    reduce over xGMI sums the shards into the first renderer's device (bit-identical to one GPU).
    The renderers must live on distinct devices and outlive the group."""

    def __init__(self, renderers):
        self._renderers = list(renderers)
        arr = (C.c_void_p * len(self._renderers))(*[r._h for r in self._renderers])
        err = C.c_int(0)
        self._h = L.lib().pt_group_create(arr, len(self._renderers), C.byref(err))
        if not self._h:
            L.check(err.value if err.value != 0 else L.PT_E_HIP)

    def close(self):
        if self._h:
            L.lib().pt_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, cam, width, height, spp, bounces=3, integrator=0, seed=1234, flags=0, pixel_order=0,
               tile_w=0, tile_h=0, out=None, view=None):
        """Returns (image float32 (H, W, 3) -- (W*H, 3) in Morton order --, summed stats dict)."""
        p = Renderer.params(width, height, spp, bounces, integrator, seed, flags, 0, 1, pixel_order, tile_w, tile_h)
        shape = (height * width, 3) if pixel_order == L.PT_ORDER_MORTON else (height, width, 3)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.size != width * height * 3 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float32 array of W*H*3 values")
        st = L.Stats()
        L.check(L.lib().pt_render_group_view(self._h, C.byref(p), C.byref(cam), _view_ref(view), out.ctypes.data,
                                             C.byref(st)))
        return out, st.as_dict()
