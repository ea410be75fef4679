"""Glue for the tests of accumulators over caller-supplied points (include/pt/pt.h, pt_accum_create_points*): a point
accumulator after n samples holds irradiance_ref.render's f64 mean at n, so the references are that restatement at the
counts the tests use (1, 2, 4, 7 and the loop's), images composed from them for frozen pixels, and noise_ref /
adaptive_ref fed with those means -- as rays_accum_ref does for ray accumulators.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import cudapathtracer_amd as pt

import adaptive_ref
import denoise_ref
import irradiance_ref as iref
import oracle
from rays_accum_ref import checkerboard                                        # noqa: F401  (the tests' freeze masks)

F = np.float32
W, H, BOUNCES, SEED = 24, 16, 3, 1234
COUNTS = (1, 2, 4, 7)

# The adaptive case of tests/test_irradiance_accum_host.py (its condition, from the restatement) and of
# tests/test_gpu_irradiance_accum.py: the floor set (a), passes of 4, cap 32.  Chosen on the restatement, before any
# kernel ran: the floor under the light is the evenly lit case, so the tolerance is the one at which part of it has
# converged by the cap and part has not (see the host test's docstring for the counts it gives).
LOOP = dict(pass_spp=4, cap=32, tol=0.2, quantile=1.0, min_batches=2)
LOOP_SET = "a"


def camera_features_ref(scene_arrays, osc, w=W, h=H):
    """The suite camera's feature buffer from the restatement (denoise_ref.features_ref over the oracle's trace): what
    Renderer.features returns, without a device."""
    cam = pt.make_camera(iref.POS, 1.0, 3.0, 0.0, w, h)
    return denoise_ref.features_ref(scene_arrays, cam, w, h, lambda o, d: oracle.trace_batch(osc, o, d))


def host_sets(scene_arrays, osc):
    """Sets a and c of irradiance_ref without a device (c from the restated features)."""
    return {"a": iref.set_floor(W, H), "c": iref.set_features(camera_features_ref(scene_arrays, osc))}


def means(osc, name, p, n, integrator, w=W, h=H, key="cornell/"):
    """k -> the restatement's (h, w, 3) f64 mean after k samples at every point of set `name` (cached, read-only)."""
    return lambda k: iref.render_cached(key + name, osc, p, n, w, h, int(k), BOUNCES, integrator, SEED)[0]


def traces(osc, name, p, n, integrator, k, w=W, h=H, key="cornell/"):
    """The restatement's trace() count for k samples of every point (cumulative from sample 1)."""
    return iref.render_cached(key + name, osc, p, n, w, h, int(k), BOUNCES, integrator, SEED)[1]["traces"]


def frozen_at(render, mask, k_frozen, k_rest):
    """The image of an accumulator whose pixels under `mask` were frozen at k_frozen samples (0: masked, mean 0) while
    the others went on to k_rest: composed from the per-count means."""
    counts = np.where(mask, k_frozen, k_rest).astype(np.uint32)
    return adaptive_ref.compose(render, counts), counts


def floor_chart(arrays):
    """A chart laid on the Cornell floor for the masked-texel case: the floor's triangles (stored normal +y, every
    vertex at the lowest y of the scene) mapped into the chart by their own x, z over [-1, 1]^2 and shrunk about the
    centre, so a border of texels belongs to no triangle.  Returns (tris, uvs)."""
    t = arrays["tris"]
    v = arrays["verts"]
    y0 = float(np.min(v["y"]))
    on = [k for k in range(len(t)) if t[k]["ny"] > 0.9 and all(abs(float(v["y"][t[k][c]]) - y0) < 1e-6 for c in ("v0", "v1", "v2"))]
    assert on, "the scene has no floor triangles"
    uv = np.zeros((len(on), 3, 2), dtype=np.float64)
    for i, k in enumerate(on):
        for j, c in enumerate(("v0", "v1", "v2")):
            x, z = float(v["x"][t[k][c]]), float(v["z"][t[k][c]])
            uv[i, j] = (0.5 + 0.375 * x, 0.5 + 0.375 * z)
    return np.array(on, dtype=np.int64), uv
