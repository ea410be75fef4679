"""Session files on the GPU (pt_session_save / pt_session_load): the file holds the live state, section by section, as
tests/session_ref.py reads it from the format's table; with nothing frozen and no estimator its records are format
1's; and an adaptive or until-error render that is saved, closed and loaded on another context continues exactly as the
one that never stopped.  All comparisons are of bytes."""
import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import shard

import adaptive_ref
import session_ref
from adaptive_ref import BOUNCES, LOOP, SEED
from session_ref import ACTIVE, COUNTS, NOISE, NOISE_PER_PIXEL

pytestmark = pytest.mark.gpu

CAM = dict(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0)
SHAPES = [(24, 16), (20, 13)]            # 384 slots: two 256-thread blocks; 20x13: partial 8x8 blocks, slots outside the image
KW = dict(tol=LOOP["tol"], quantile=LOOP["quantile"], min_batches=LOOP["min_batches"])
PASS, HALF, CAP = LOOP["pass_spp"], 16, LOOP["cap"]


def _cam(w, h):
    return pt.make_camera(width=w, height=h, **CAM)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx + yy) % 2 == 0


@pytest.fixture(scope="module")
def cb():
    s = load_scene("cornell_blob")
    with pt.Renderer(s, 0) as r, pt.Renderer(s, 0) as r2:
        yield s, r, r2


def _state(acc, est):
    """Everything a later call can show of an accumulator and its estimator, as bytes."""
    out = dict(mean=_bits(acc.mean64()), image=_bits(acc.image()), counts=_bits(acc.counts()),
               active=_bits(acc.active_pixels()), samples=acc.samples)
    if est is not None:
        mu, m2 = est.read()
        out.update(mu=_bits(mu), m2=_bits(m2), emap=_bits(est.error_map()), var=_bits(est.variance()))
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


def _frozen(acc, w, h):
    """The frozen pixels, (h, w) in scanline order: what the device's active list does not name."""
    m = np.ones(w * h, dtype=bool)
    m[acc.active_pixels()] = False
    return m.reshape(h, w)


# ---------------------------------------------------------------- 1. the file against the live state
def _check_file(f, acc, est, ref, w, h):
    d = session_ref.read(f)
    hd = d["header"]
    counts = acc.counts()
    frozen = _frozen(acc, w, h)
    assert int(hd["flags"]) == COUNTS | NOISE | NOISE_PER_PIXEL
    assert int(hd["samples"]) == acc.samples and int(hd["noise_n0"]) == ref.n0 == acc.samples
    assert int(hd["noise_batches"]) == ref.batches and float(hd["noise_W"]) == float(acc.samples)
    assert int(hd["frozen_pixels"]) == int(frozen.sum()) > 0
    p = hd["params"]
    assert (int(p["width"]), int(p["height"]), int(p["spp"]), int(p["bounces"]), int(p["seed"])) == (w, h, 0, BOUNCES, SEED)
    assert _bits(d["A"]["mean"]) == _bits(acc.mean64())
    assert d["A"]["rng"].any(axis=-1).all()                                   # (every pixel was sampled: a live XORWOW state)
    assert _bits(d["B"]) == _bits(np.where(frozen, counts, ACTIVE).astype(np.uint32))
    mu, m2 = est.read()
    assert _bits(d["C"]["mu"]) == _bits(mu) == _bits(ref.mu) and _bits(d["C"]["m2"]) == _bits(m2) == _bits(ref.m2)
    assert _bits(d["C"]["prev"]) == _bits(ref.prev)
    assert _bits(d["D"]["W_q"]) == _bits(ref.Wq) and _bits(d["D"]["b_q"]) == _bits(ref.bq)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("w,h", SHAPES)
def test_file_against_the_live_state(cb, tmp_path, w, h, integ):
    s, r, _ = cb
    f = str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, integrator=integ, seed=SEED) as acc, acc.noise() as est:
        ref = adaptive_ref.AdaptiveRef(0, acc.mean64())
        acc.add(2)
        acc.freeze(_checker(w, h))
        acc.add(3)
        est.update()
        assert ref.update(acc.samples, acc.counts(), acc.mean64())
        assert est.freeze(tol=0.25) == (0, int((~_checker(w, h)).sum()))      # (one batch: every error is +inf)
        acc.add(4)
        est.update()
        assert ref.update(acc.samples, acc.counts(), acc.mean64())
        acc.save_session(f, est)
        _check_file(f, acc, est, ref, w, h)
        assert sorted(np.unique(acc.counts())) == [2, 9] and sorted(np.unique(ref.bq)) == [1, 2]
        # ... and once the estimator itself has frozen pixels: three counts, and pixels whose window stopped early
        want = ref.converged(0.25) & (acc.counts() == 9)
        newly, active = est.freeze(tol=0.25)
        assert 0 < newly == int(want.sum()) and active == int((acc.counts() == 9).sum()) - newly > 0
        acc.add(1)
        est.update()
        assert ref.update(acc.samples, acc.counts(), acc.mean64())
        acc.save_session(f, est)
        _check_file(f, acc, est, ref, w, h)
        assert sorted(np.unique(acc.counts())) == [2, 9, 10]


# ---------------------------------------------------------------- 2. the bridge to format 1
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("n", [0, 3])
def test_section_a_is_format_1(cb, tmp_path, w, h, n):
    s, r, _ = cb
    f1, f2 = str(tmp_path / "a.ptacc"), str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.add(n)
        acc.save(f1)
        acc.save_session(f2)
    one, two = open(f1, "rb").read(), open(f2, "rb").read()
    assert len(one) == 128 + w * h * 48 and len(two) == 192 + w * h * 48
    assert two[192:] == one[128:] and two[16:128] == one[16:128] and two[128:192] == bytes(64)
    i = pt.session_file_info(f2)
    assert i["flags"] == 0 and i["samples"] == n and i["frozen_pixels"] == 0 and i["noise_batches"] == 0
    assert i["scene_digest"] == pt.accum_file_info(f1)["scene_digest"]
    with r.load_session(f2)[0] as again, r.load_accumulator(f1) as old:       # and both continue alike
        again.add(2)
        old.add(2)
        assert again.samples == n + 2 and _bits(again.mean64()) == _bits(old.mean64())


# ---------------------------------------------------------------- 3. resume equals never stopping: the adaptive loop
def _adaptive_whole(r, w, h, integ, **geom):
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, integrator=integ, seed=SEED, **geom) as acc:
        res = acc.add_adaptive(PASS, CAP, **KW)
        return res, _state(acc, acc._noise)


def _adaptive_split(r, r2, f, w, h, integ, **geom):
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, integrator=integ, seed=SEED, **geom) as acc:
        first = acc.add_adaptive(PASS, HALF, **KW)
        acc.save_session(f, acc._noise)
    acc, est = r2.load_session(f)                                              # (the first accumulator and estimator are gone)
    with acc:
        assert est is not None and acc.samples == first["samples"]
        res = acc.add_adaptive(PASS, CAP, **KW)
        return first, res, _state(acc, est)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("w,h", SHAPES)
def test_resumed_adaptive_run_equals_the_uninterrupted_one(cb, tmp_path, w, h, integ):
    s, r, r2 = cb
    whole, want = _adaptive_whole(r, w, h, integ)
    assert whole["stopped_converged"] is False and whole["passes"] == 8        # (so the split at 16 is inside the loop)
    first, res, got = _adaptive_split(r, r2, str(tmp_path / "s.ptses"), w, h, integ)
    assert first["passes"] == 4 and first["samples"] == HALF and 0 < first["active"] < w * h
    _same(got, want)
    assert res["passes"] == 4 and res["stopped_converged"] is False and res["samples"] == CAP
    for k in ("summary", "active", "samples_total"):
        assert res[k] == whole[k], k
    assert res["summary"]["batches"] == 8


# ---------------------------------------------------------------- 4. ... and the until-error loop
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("w,h", SHAPES)
def test_resumed_until_run_equals_the_uninterrupted_one(cb, tmp_path, w, h, integ):
    s, r, r2 = cb
    f = str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, integrator=integ, seed=SEED) as acc:
        whole = acc.add_until(PASS, CAP, **KW)
        want = _state(acc, acc._noise)
    # (the pixels the adaptive loop still samples at the cap have not converged in any pass, and this loop samples
    # them just so: with quantile 1 it cannot stop before the cap)
    assert whole["stopped_converged"] is False and whole["passes"] == 8
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, integrator=integ, seed=SEED) as acc:
        first = acc.add_until(PASS, HALF, **KW)
        acc.save_session(f, acc._noise)
    i = pt.session_file_info(f)
    assert i["flags"] == NOISE and (i["noise_n0"], i["noise_W"], i["noise_batches"]) == (HALF, float(HALF), 4)
    assert session_ref.read(f)["D"] is None and first["passes"] == 4
    acc, est = r2.load_session(f)
    with acc:
        res = acc.add_until(PASS, CAP, **KW)
        _same(_state(acc, est), want)
    assert res["passes"] == 4 and res["stopped_converged"] is False and res["summary"] == whole["summary"]


@pytest.mark.parametrize("frozen", [False, True])
def test_saved_between_add_and_update(cb, tmp_path, frozen):
    s, r, r2 = cb
    w, h = 20, 13
    f = str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc, acc.noise() as est:
        acc.add(4)
        est.update()
        if frozen:
            acc.freeze(_checker(w, h))                                         # (the estimator has not seen it yet: no section D)
        acc.add(3)
        acc.save_session(f, est)
        i = pt.session_file_info(f)
        assert i["flags"] == (COUNTS | NOISE if frozen else NOISE) and (i["samples"], i["noise_n0"], i["noise_batches"]) == (7, 4, 1)
        want_sum = est.update(tol=0.25)
        want = _state(acc, est)
    acc, est = r2.load_session(f)
    with acc:
        assert est.update(tol=0.25) == want_sum and want_sum["batches"] == 2
        _same(_state(acc, est), want)


# ---------------------------------------------------------------- 5. geometry
def test_two_shards_resumed_are_the_unsharded_resumed_run(cb, tmp_path):
    s, r, r2 = cb
    w, h, tile = 37, 19, (16, 8)
    mean = np.zeros((h, w, 3), dtype=np.float64)
    counts = np.zeros((h, w), dtype=np.uint32)
    mu = np.zeros((h, w), dtype=np.float64)
    for i in range(2):
        f = str(tmp_path / ("s%d.ptses" % i))
        with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED, shard_index=i, shard_count=2, tile=tile) as acc:
            acc.add_adaptive(PASS, HALF, **KW)
            acc.save_session(f, acc._noise)
        mine = np.zeros(w * h, dtype=bool)
        mine[shard.shard_pixels(w, h, i, 2, tile[0], tile[1])] = True
        mine = mine.reshape(h, w)
        d = session_ref.read(f)
        assert 0 < mine.sum() < w * h and int(d["header"]["params"]["shard_index"]) == i
        assert int(d["header"]["flags"]) == COUNTS | NOISE | NOISE_PER_PIXEL  # (each shard has frozen pixels by 16 samples)
        for sec in "ABCD":                                                     # pixels outside the shard: all zero
            assert not np.frombuffer(_bits(d[sec][~mine]), dtype=np.uint8).any(), sec
        assert (d["B"][mine] != 0).any() and int(d["header"]["frozen_pixels"]) == int((d["B"][mine] != ACTIVE).sum())
        acc, est = r2.load_session(f)
        with acc:
            acc.add_adaptive(PASS, CAP, **KW)
            assert not acc.counts()[~mine].any()
            mean += acc.mean64()
            counts += acc.counts()
            mu += est.read()[0]
    first, res, got = _adaptive_split(r, r2, str(tmp_path / "s.ptses"), w, h, 0)
    assert got["mean"] == _bits(mean) and got["counts"] == _bits(counts) and got["mu"] == _bits(mu)
    whole, want = _adaptive_whole(r, w, h, 0)
    _same(got, want)


def test_morton_pixel_order(cb, tmp_path):
    s, r, r2 = cb
    w = h = 16
    whole, want = _adaptive_whole(r, w, h, 0, pixel_order=pt.PT_ORDER_MORTON)
    first, res, got = _adaptive_split(r, r2, str(tmp_path / "s.ptses"), w, h, 0, pixel_order=pt.PT_ORDER_MORTON)
    _same(got, want)
    assert res["summary"] == whole["summary"] and first["passes"] + res["passes"] == whole["passes"]
    # the file is in scanline order whatever the accumulator's: section B against the Morton-indexed counts
    f = str(tmp_path / "m.ptses")
    idx = np.array([[pt.morton_pxl_to_i(x, y) for x in range(w)] for y in range(h)])
    acc, est = r2.load_session(str(tmp_path / "s.ptses"))
    with acc:
        acc.save_session(f, est)
        c = acc.counts()[idx]
        assert _bits(session_ref.read(f)["B"]) == _bits(np.where(_frozen(acc, w, h), c, ACTIVE).astype(np.uint32))
        assert _bits(session_ref.read(f)["A"]["mean"]) == _bits(acc.mean64()[idx])
    assert open(f, "rb").read() == open(str(tmp_path / "s.ptses"), "rb").read()   # (a load and a save: the same file)


def test_empty_shard(cb, tmp_path):
    s, r, r2 = cb
    w, h = 24, 16
    f = str(tmp_path / "s.ptses")
    before, _ = r2.render(_cam(w, h), w, h, 2, bounces=BOUNCES, seed=SEED)
    geom = dict(shard_index=5, shard_count=6, tile=(16, 8))                    # 4 tiles: shards 4 and 5 own none
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED, **geom) as acc, acc.noise() as est:
        acc.add(3)
        est.update()
        acc.save_session(f, est)
    blob = open(f, "rb").read()
    assert len(blob) == 192 + w * h * 88 and blob[192:] == bytes(w * h * 88)   # the header plus zeros: sections A and C
    i = pt.session_file_info(f)
    assert i["flags"] == NOISE and (i["samples"], i["noise_n0"], i["noise_batches"], i["frozen_pixels"]) == (3, 3, 1, 0)
    assert (i["params"].shard_index, i["params"].shard_count) == (5, 6)
    acc, est = r2.load_session(f)
    with acc:
        assert acc.samples == 3 and not acc.mean64().any() and not acc.counts().any() and acc.active_pixels().size == 0
        res = acc.add_adaptive(PASS, CAP, **KW)                                # pt.h's empty-shard table
        assert res["passes"] == 0 and res["stopped_converged"] is True and res["active"] == 0 and res["samples_total"] == 0
        assert acc.samples == 3 and res["summary"]["pixels"] == 0 and res["summary"]["batches"] == 1
        acc.save_session(str(tmp_path / "t.ptses"), est)
        assert open(str(tmp_path / "t.ptses"), "rb").read() == blob
    after, _ = r2.render(_cam(w, h), w, h, 2, bounces=BOUNCES, seed=SEED)
    assert _bits(after) == _bits(before)


# ---------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("w,h", SHAPES)
def test_saved_at_zero_samples_with_pixels_frozen_at_zero(cb, tmp_path, w, h):
    s, r, r2 = cb
    f = str(tmp_path / "s.ptses")
    mask = _checker(w, h)
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.freeze(mask)
        acc.save_session(f)
        d = session_ref.read(f)
        assert int(d["header"]["flags"]) == COUNTS and int(d["header"]["samples"]) == 0
        assert int(d["header"]["frozen_pixels"]) == int(mask.sum())
        assert not np.frombuffer(_bits(d["A"]), dtype=np.uint8).any()
        assert _bits(d["B"]) == _bits(np.where(mask, 0, ACTIVE).astype(np.uint32))
        acc.add(2)
        acc.add(3)
        want = _state(acc, None)
    acc, est = r2.load_session(f)
    with acc:
        assert est is None and acc.samples == 0
        st = acc.add(2)                                                        # (the active pixels' first samples)
        assert st["samples"] == int((~mask).sum()) * 2
        acc.add(3)
        _same(_state(acc, None), want)
        assert sorted(np.unique(acc.counts())) == [0, 5] and not acc.mean64()[mask].any()


def test_every_pixel_frozen(cb, tmp_path):
    s, r, r2 = cb
    w, h = 20, 13
    f = str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.add(2)
        acc.freeze(np.ones((h, w), dtype=bool))
        acc.save_session(f)
        want = _state(acc, None)
    assert pt.session_file_info(f)["frozen_pixels"] == w * h
    acc, _ = r2.load_session(f)
    with acc:
        st = acc.add(3)
        assert st["samples"] == 0 and st["rays_traced"] == 0 and acc.samples == 2 and acc.active_pixels().size == 0
        _same(_state(acc, None), want)


def test_the_estimator_can_be_left_in_the_file(cb, tmp_path):
    s, r, r2 = cb
    w, h = 24, 16
    f = str(tmp_path / "s.ptses")
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.add_adaptive(PASS, HALF, **KW)
        acc.save_session(f, acc._noise)
        want = _state(acc, None)
        with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as other, other.noise() as stranger:
            with pytest.raises(pt.PtError) as e:                               # not this accumulator's live estimator
                acc.save_session(f + ".no", stranger)
            assert e.value.code == pt.PT_E_INVALID and "pt_session_save" in str(e.value)
    acc, est = r2.load_session(f, noise=False)
    with acc:
        assert est is None and acc._noise is None
        _same(_state(acc, None), want)
        fresh = acc.noise()                                                    # a fresh window at the resumed state, as today
        summ = fresh.update()
        assert summ["batches"] == 0 and summ["samples"] == HALF and np.isposinf(fresh.error_map()).all()
        acc.add(PASS)
        assert fresh.update()["batches"] == 1


def test_refused_while_renders_are_in_flight(cb, tmp_path):
    import torch
    s, r, r2 = cb
    w, h = 24, 16
    f = str(tmp_path / "s.ptses")
    d = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.add(2)
        acc.save_session(f)
        r.render_device_async(_cam(w, h), d.data_ptr(), w, h, 2)
        try:
            with pytest.raises(pt.PtError) as e:
                acc.save_session(f + ".no")
            assert e.value.code == pt.PT_E_INVALID and "pt_session_save" in str(e.value) and "in flight" in str(e.value)
            with pytest.raises(pt.PtError) as e:
                r.load_session(f)
            assert e.value.code == pt.PT_E_INVALID and "pt_session_load" in str(e.value) and "in flight" in str(e.value)
        finally:
            r.wait()
        acc.save_session(f + ".yes")                                           # and afterwards it is taken again
        assert open(f + ".yes", "rb").read() == open(f, "rb").read()


# ---------------------------------------------------------------- 7. refusals on real files
def test_refused_loads_leave_the_context_as_it_was(cb, tmp_path):
    s, r, r2 = cb
    w, h = 24, 16
    f, g = str(tmp_path / "s.ptses"), str(tmp_path / "bad.ptses")
    reference, _ = r2.render(_cam(w, h), w, h, 2, bounces=BOUNCES, seed=SEED)
    with r.accumulator(_cam(w, h), w, h, bounces=BOUNCES, seed=SEED) as acc:
        acc.add_adaptive(PASS, HALF, **KW)
        acc.save_session(f, acc._noise)
    good = open(f, "rb").read()
    d = session_ref.read(f)
    samples, frozen = int(d["header"]["samples"]), int(d["header"]["frozen_pixels"])
    assert samples == HALF and 0 < frozen < w * h

    def refused(renderer, path, code, *words):
        with pytest.raises(pt.PtError) as e:
            renderer.load_session(path)
        assert e.value.code == code and "pt_session_load" in str(e.value), str(e.value)
        for word in words:
            assert word in str(e.value)
        img, _ = renderer.render(_cam(w, h), w, h, 2, bounces=BOUNCES, seed=SEED)
        return img

    with pt.Renderer(load_scene("cornell"), 0) as other:                      # another scene
        want, _ = other.render(_cam(w, h), w, h, 2, bounces=BOUNCES, seed=SEED)
        assert _bits(refused(other, f, pt.PT_E_SCENE, "another scene")) == _bits(want)
    off_b = 192 + w * h * 48
    for pix in (0, w * h - 1, int(np.flatnonzero(d["B"].reshape(-1) != ACTIVE)[0])):   # an active and a frozen pixel's word
        bad = bytearray(good)
        bad[off_b + 4 * pix: off_b + 4 * pix + 4] = np.uint32(samples + 1).tobytes()
        open(g, "wb").write(bytes(bad))
        assert _bits(refused(r2, g, pt.PT_E_INVALID, "section-B")) == _bits(reference)
    for delta in (1, -1):                                                      # the header's frozen count off by one
        bad = bytearray(good)
        bad[160:168] = np.uint64(frozen + delta).tobytes()
        open(g, "wb").write(bytes(bad))
        assert _bits(refused(r2, g, pt.PT_E_INVALID, "frozen")) == _bits(reference)
    open(g, "wb").write(good[:-1])
    assert _bits(refused(r2, g, pt.PT_E_IO, "truncated")) == _bits(reference)
    bad = bytearray(good)                                                      # parameters no accumulator takes: PT_FLAG_COUNT
    bad[36:40] = np.uint32(pt.PT_FLAG_COUNT).tobytes()
    open(g, "wb").write(bytes(bad))
    assert _bits(refused(r2, g, pt.PT_E_INVALID, "flags 0x8")) == _bits(reference)
    bad = bytearray(good)                                                      # per-pixel planes without frozen-at counts
    bad[128:132] = np.uint32(NOISE | NOISE_PER_PIXEL).tobytes()
    open(g, "wb").write(bytes(bad))
    assert _bits(refused(r2, g, pt.PT_E_INVALID, "0x1")) == _bits(reference)
    acc, est = r2.load_session(f)                                              # and the good file still loads
    with acc:
        assert est is not None and acc.samples == HALF
