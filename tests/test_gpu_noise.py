"""The noise estimator on the GPU (pt_noise_*, Accumulator.noise / add_until): the fold, the per-pixel error and the
whole convergence summary equal the numpy restatement (tests/noise_ref.py) in every bit, fed with the accumulator's
own f64 mean after every pass -- whatever the pass sizes, the image shape, the pixel order, the shard and the point
at which the estimator was attached; and attaching one changes nothing about the render."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, shard

import noise_ref

pytestmark = pytest.mark.gpu

CAM = dict(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0)   # test_gpu_accumulate.py's
BOUNCES = 3
TOLS = (0.05, 0.25, 1.0)
SPLITS = [[2, 3, 4], [1] * 5, [4, 1, 4]]


def _cam(w, h):
    return pt.make_camera(width=w, height=h, **CAM)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def cb():
    with pt.Renderer(load_scene("cornell_blob"), 0) as r:
        yield r


def _mask(acc):
    """The pixels of the accumulator's shard, shaped like NoiseEstimate's arrays (scanline order only)."""
    p = acc.params
    m = np.zeros(p.width * p.height, dtype=bool)
    m[shard.shard_pixels(p.width, p.height, p.shard_index, p.shard_count, p.tile_w or 8, p.tile_h or 8)] = True
    return m.reshape(p.height, p.width)


def _check_state(est, ref, mask):
    mu, m2 = est.read()
    assert _bits(mu) == _bits(np.where(mask, ref.mu, 0.0)) and _bits(m2) == _bits(np.where(mask, ref.m2, 0.0))


def _check_summary(est, ref, mask, acc, tols=TOLS, y_floor=None):
    """update() (which folds at most once: the later calls only re-summarise) and error_map() against the restatement."""
    out = {}
    for tol in tols:
        s = est.update(tol=tol, y_floor=y_floor)
        want = ref.summary(tol, noise_ref.Y_FLOOR if y_floor is None else y_floor, mask)
        assert s["samples"] == acc.samples
        assert {k: s[k] for k in want} == want, (tol, s, want)
        assert sum(s["hist"]) == s["pixels"] == int(mask.sum())
        out[tol] = s
    emap = est.error_map(y_floor=y_floor)
    want = np.where(mask, ref.error_map(noise_ref.Y_FLOOR if y_floor is None else y_floor), np.float32(0.0))
    assert emap.dtype == np.float32 and _bits(emap) == _bits(want)
    return out


def _run_split(r, w, h, integ, split, bounces=BOUNCES, start=0, **kw):
    """Accumulate `start` samples, attach an estimator, then `split`; everything checked after every pass.
    Returns the summaries after the last pass, by tol."""
    with r.accumulator(_cam(w, h), w, h, bounces=bounces, integrator=integ, **kw) as acc:
        if start:
            acc.add(start)
        mask = _mask(acc) if not kw.get("pixel_order") else np.ones(w * h, dtype=bool)
        with acc.noise() as est:
            ref = noise_ref.NoiseRef(start, acc.mean64())
            _check_state(est, ref, mask)
            for k in split:
                acc.add(k)
                assert ref.update(acc.samples, acc.mean64())
                last = _check_summary(est, ref, mask, acc)
                _check_state(est, ref, mask)
                assert last[TOLS[0]]["batches"] == ref.batches
    return last


# ---------------------------------------------------------------- 1. fold and state
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("w,h", [(24, 16), (20, 13)])     # 20x13: partial 8x8 blocks, slots outside the image
def test_fold_state_and_summary(cb, w, h, split, integ):
    last = _run_split(cb, w, h, integ, split)
    # not trivially all-or-nothing, and the exact-zero pixels (black: bin 0) are there
    assert 0 < last[0.25]["converged"] < last[0.25]["pixels"] == w * h
    assert last[0.25]["hist"][0] > 0 and last[0.25]["hist"][63] == 0


# ---------------------------------------------------------------- 2. before two batches
def test_before_two_batches(cb):
    w, h = 24, 16
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc, acc.noise() as est:
        s = est.update()
        assert (s["samples"], s["batches"], s["converged"], s["hist"][63]) == (0, 0, 0, w * h)   # nothing to fold yet
        acc.add(3)
        s = est.update(tol=1.0)
        assert (s["samples"], s["batches"], s["pixels"], s["converged"]) == (3, 1, w * h, 0)
        assert s["hist"][63] == w * h and sum(s["hist"]) == w * h
        assert np.isposinf(est.error_map()).all()
        state = [_bits(a) for a in est.read()]
        s2 = est.update(tol=0.5)                      # no new samples: re-summarised, not folded
        assert s2["batches"] == 1 and s2["samples"] == 3 and s2["hist"] == s["hist"]
        assert [_bits(a) for a in est.read()] == state


# ---------------------------------------------------------------- 3. bin clamps
def test_bin_clamps(cb):
    w, h = 24, 16
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc, acc.noise() as est:
        ref = noise_ref.NoiseRef(0, acc.mean64())
        for k in (2, 3, 4):
            acc.add(k)
            ref.update(acc.samples, acc.mean64())
            est.update()
        mask = np.ones((h, w), dtype=bool)
        nonzero = int(np.count_nonzero(ref.error_map(1e12)))
        assert 0 < nonzero < w * h
        s = _check_summary(est, ref, mask, acc, tols=(0.05,), y_floor=1e12)[0.05]
        assert s["hist"][1] == nonzero and s["hist"][0] == w * h - nonzero      # every non-zero pixel: the low clamp
        # y_floor = 1e30: (float)rel2 underflows to 0 everywhere, yet `converged` follows the f64 value
        s = _check_summary(est, ref, mask, acc, tols=(1e-30,), y_floor=1e30)[1e-30]
        assert s["hist"][0] == w * h
        assert w * h - nonzero < s["converged"] < w * h


# ---------------------------------------------------------------- 4. window start
@pytest.mark.parametrize("integ", [0, 1])
def test_window_starts_where_the_estimator_is_attached(cb, integ):
    last = _run_split(cb, 24, 16, integ, [2, 4], start=3)
    assert last[0.25]["samples"] == 9 and last[0.25]["batches"] == 2


# ---------------------------------------------------------------- 5. layouts
def test_morton_pixel_order(cb):
    last = _run_split(cb, 16, 16, 0, [2, 3, 4], pixel_order=pt.PT_ORDER_MORTON)
    assert 0 < last[0.25]["converged"] < 256


def test_shards_add_up(cb):
    import torch
    w, h = 24, 16
    whole = _run_split(cb, w, h, 0, [2, 3, 4])
    parts = [_run_split(cb, w, h, 0, [2, 3, 4], shard_index=i, shard_count=2, tile=8) for i in range(2)]
    n = C.c_uint32(0)
    assert _lib.lib().pt_shard_pixels(w, h, 1, 2, 8, 8, None, 0, C.byref(n)) == 0
    for tol in TOLS:
        assert parts[1][tol]["pixels"] == n.value and 0 < n.value < w * h
        for key in ("pixels", "converged"):
            assert parts[0][tol][key] + parts[1][tol][key] == whole[tol][key]
        assert [a + b for a, b in zip(parts[0][tol]["hist"], parts[1][tol]["hist"])] == whole[tol]["hist"]
    # the device variant leaves the pixels of other shards untouched
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES, shard_index=1, shard_count=2, tile=8) as acc, acc.noise() as est:
        for k in (2, 3):
            acc.add(k)
            est.update()
        buf = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        d = _lib.NoiseParams(0.05, 0.01)
        _lib.check(_lib.lib().pt_noise_map_device(est._h, C.byref(d), C.c_void_p(buf.data_ptr()), None))
        got, mask = buf.cpu().numpy(), _mask(acc)
        assert (got[~mask] == -1.0).all() and _bits(got[mask]) == _bits(est.error_map()[mask])


# ---------------------------------------------------------------- 6. grid-stride path
def test_more_slots_than_one_sweep_of_the_grid(cb):
    """The update's grid is capped at 4 blocks of 256 lanes per CU: 262144 slots a sweep on 256 CUs.  520x516 pads to
    520x520 = 270400 slots, so the first blocks' lanes take a second slot.  Bounces 2: with 1 only the light's own
    pixels are not black, and a skipped slot would go unseen."""
    last = _run_split(cb, 520, 516, 0, [1, 1, 2], bounces=2)
    assert last[0.25]["pixels"] == 520 * 516 and 0 < last[0.25]["converged"] < 520 * 516
    assert last[0.25]["hist"][0] < 520 * 516 * 3 // 4


# ---------------------------------------------------------------- 7. add_until
def _stops(s, min_batches, quantile):
    return s["batches"] >= min_batches and s["converged"] >= int(np.ceil(np.float64(np.float32(quantile)) * s["pixels"]))


@pytest.mark.parametrize("tol,quantile,early", [(1e-6, 0.95, False), (1.0, 0.9, True)])
def test_add_until_is_the_manual_loop(cb, tol, quantile, early):
    w, h, pass_spp, cap = 24, 16, 4, 30      # (the cap is no multiple of the pass: the last pass is shorter)
    # the manual loop, with the restatement alongside
    steps = []
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc, acc.noise() as est:
        ref = noise_ref.NoiseRef(0, acc.mean64())
        while acc.samples < cap:
            acc.add(min(pass_spp, cap - acc.samples))
            s = est.update(tol=tol)
            ref.update(acc.samples, acc.mean64())
            want = ref.summary(tol)
            assert {k: s[k] for k in want} == want
            steps.append(s)
            if _stops(want, 2, quantile):
                break
        manual_img, manual_state, stopped = acc.image(), est.read(), _stops(steps[-1], 2, quantile)
    assert stopped == early and (steps[-1]["samples"] < cap) == early          # (on the restatement: really before the cap)
    # one call
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc:
        res = acc.add_until(pass_spp, cap, tol=tol, quantile=quantile)
        assert res["passes"] == len(steps) and res["stopped_converged"] == early
        assert res["samples"] == acc.samples == steps[-1]["samples"] and res["summary"] == steps[-1]
        assert _bits(acc.image()) == _bits(manual_img)
        assert [_bits(a) for a in acc._noise.read()] == [_bits(a) for a in manual_state]
        plain, _ = cb.render(_cam(w, h), w, h, acc.samples, bounces=BOUNCES)
        assert _bits(acc.image()) == _bits(plain)
    # step for step: a cap that grows by one pass per call
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc:
        for i, want in enumerate(steps):
            res = acc.add_until(pass_spp, want["samples"], tol=tol, quantile=quantile)
            assert res["passes"] == 1 and res["summary"] == want
            assert res["stopped_converged"] == (early and i == len(steps) - 1)
    # and an accumulator without an estimator renders the same image
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc:
        for s in steps:
            acc.add(s["samples"] - acc.samples)
        assert _bits(acc.image()) == _bits(manual_img)


# ---------------------------------------------------------------- 8. refusals
def test_refusals(cb):
    w, h = 24, 16
    with cb.accumulator(_cam(w, h), w, h, bounces=BOUNCES) as acc:
        est = acc.noise()
        with pytest.raises(pt.PtError) as e:
            acc.noise()
        assert e.value.code == pt.PT_E_INVALID and "estimator" in str(e.value)
        assert acc._noise is est
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pt.PtError) as e:
                est.update(tol=bad)
            assert e.value.code == pt.PT_E_INVALID
            with pytest.raises(pt.PtError):
                est.error_map(y_floor=bad)
        for kw in (dict(quantile=0.0), dict(quantile=1.5), dict(min_batches=1)):
            with pytest.raises(pt.PtError) as e:
                acc.add_until(4, 8, tol=0.05, **kw)
            assert e.value.code == pt.PT_E_INVALID
        with pytest.raises(pt.PtError):
            acc.add_until(0, 8, tol=0.05)
        assert acc.samples == 0
        est.close()
        acc.noise().close()                 # after closing the first, another may attach
