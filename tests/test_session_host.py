"""Session files without a GPU (pt_session_save / pt_session_load / pt_session_file_info): the null-argument refusals,
and the header checks of pt_session_file_info on files that tests/session_ref.py writes from the format's table; the
reader of format version 1 refuses a version-2 file."""
import ctypes as C

import numpy as np
import pytest

import conftest  # noqa: F401  (builds the library once)

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib

import session_ref
from session_ref import COUNTS, NOISE, NOISE_PER_PIXEL

W, H = 5, 3


def _err():
    return (_lib.lib().pt_last_error() or b"").decode()


def _info(path):
    with pytest.raises(pt.PtError) as e:
        pt.session_file_info(path)
    return e.value.code, str(e.value)


def test_null_arguments_name_the_function():
    L = _lib.lib()
    assert L.pt_session_save(None, None, None) == _lib.PT_E_INVALID
    assert "pt_session_save" in _err() and "null" in _err()
    assert L.pt_session_save(None, None, b"/nowhere/f") == _lib.PT_E_INVALID and "pt_session_save" in _err()
    acc, est, has = C.c_void_p(0x55), C.c_void_p(0x55), C.c_int(7)
    assert L.pt_session_load(None, b"/nowhere/f", C.byref(acc), C.byref(est), C.byref(has)) == _lib.PT_E_INVALID
    assert "pt_session_load" in _err() and "null" in _err()
    assert acc.value is None and est.value is None and has.value == 0          # both outputs null on failure
    assert L.pt_session_load(None, None, None, None, None) == _lib.PT_E_INVALID and "pt_session_load" in _err()
    info = _lib.SessionInfo()
    assert L.pt_session_file_info(None, C.byref(info)) == _lib.PT_E_INVALID
    assert "pt_session_file_info" in _err() and "null" in _err()
    assert L.pt_session_file_info(b"/nowhere/f", None) == _lib.PT_E_INVALID and "pt_session_file_info" in _err()
    assert L.pt_session_file_info(b"/nowhere/f", C.byref(info)) == _lib.PT_E_IO and "pt_session_file_info" in _err()


def test_a_good_header_round_trips_every_field(tmp_path):
    f = str(tmp_path / "s.ptses")
    h = session_ref.header(W, H, samples=40, flags=COUNTS | NOISE | NOISE_PER_PIXEL, noise_n0=36, noise_W=36.0,
                           noise_batches=9, frozen_pixels=7, bounces=5, integrator=1, seed=(1 << 40) + 99, shard_index=1,
                           shard_count=3, pixel_order=0, tile_w=16, tile_h=8, scene_digest=0xFEDCBA9876543210)
    h["camera"]["radius"] = 0.05
    session_ref.write(f, h)
    i = pt.session_file_info(f)
    p, c = i["params"], i["camera"]
    assert (p.width, p.height, p.spp, p.bounces, p.integrator, p.flags, p.seed) == (W, H, 0, 5, 1, 0, (1 << 40) + 99)
    assert (p.shard_index, p.shard_count, p.pixel_order, p.tile_w, p.tile_h) == (1, 3, 0, 16, 8)
    assert (c.pos.x, c.pos.y, c.pos.z, c.dist_from_film, c.focal_length) == (0.0, 1.0, 3.0, 1.0, 3.0)
    assert c.radius == np.float32(0.05) and (c.pxl_width, c.pxl_height) == (W, H)
    assert i["samples"] == 40 and i["scene_digest"] == 0xFEDCBA9876543210
    assert i["flags"] == 7 and (i["noise_n0"], i["noise_W"], i["noise_batches"]) == (36, 36.0, 9) and i["frozen_pixels"] == 7
    for flags in (0, COUNTS, NOISE, COUNTS | NOISE):                          # every legal set of sections has its size
        session_ref.write(f, session_ref.header(W, H, samples=4, flags=flags))
        assert pt.session_file_info(f)["flags"] == flags


def test_the_reference_reader_reads_what_its_writer_wrote(tmp_path):
    f = str(tmp_path / "s.ptses")
    rng = np.random.default_rng(7)
    a = np.zeros((H, W), dtype=session_ref.REC_A)
    a["rng"], a["mean"] = rng.integers(0, 1 << 32, (H, W, 6), dtype=np.uint64), rng.random((H, W, 3))
    b = np.where(rng.random((H, W)) < 0.5, session_ref.ACTIVE, 3).astype(np.uint32)
    c = np.zeros((H, W), dtype=session_ref.REC_C)
    c["prev"], c["mu"], c["m2"] = rng.random((H, W, 3)), rng.random((H, W)), rng.random((H, W))
    d = np.zeros((H, W), dtype=session_ref.REC_D)
    d["W_q"], d["b_q"] = 8, 2
    frozen = int((b != session_ref.ACTIVE).sum())
    h = session_ref.header(W, H, samples=8, flags=7, noise_n0=8, noise_W=8.0, noise_batches=2, frozen_pixels=frozen)
    session_ref.write(f, h, A=a, B=b, C=c, D=d)
    got = session_ref.read(f)
    for name, want in (("A", a), ("B", b), ("C", c), ("D", d)):
        assert got[name].tobytes() == want.tobytes(), name
    assert len(open(f, "rb").read()) == 192 + W * H * 100 and pt.session_file_info(f)["frozen_pixels"] == frozen
    session_ref.write(f, session_ref.header(W, H, samples=8, flags=COUNTS, frozen_pixels=frozen), B=b)
    got = session_ref.read(f)
    assert got["C"] is None and got["D"] is None and got["B"].tobytes() == b.tobytes() and not got["A"]["rng"].any()


def test_header_refusals(tmp_path):
    f = str(tmp_path / "s.ptses")
    ok = dict(samples=8, flags=NOISE, noise_n0=8, noise_W=8.0, noise_batches=2)

    def refused(code, *words, tail=b"", cut=0, **kw):
        session_ref.write(f, session_ref.header(W, H, **dict(ok, **kw)), tail=tail, cut=cut)
        got, msg = _info(f)
        assert got == code and "pt_session_file_info" in msg, (kw, msg)
        for w in words:
            assert w in msg, (w, msg)

    session_ref.write(f, session_ref.header(W, H, **ok))
    assert pt.session_file_info(f)["samples"] == 8
    refused(pt.PT_E_INVALID, "magic", magic=b"PTACCUX\0")
    refused(pt.PT_E_INVALID, "header", header_bytes=128)
    refused(pt.PT_E_INVALID, "header", header_bytes=200)
    refused(pt.PT_E_INVALID, "version 3", version=3)
    refused(pt.PT_E_INVALID, "flag", flags=NOISE | 0x8)
    refused(pt.PT_E_INVALID, "flag", flags=0x80000000)
    refused(pt.PT_E_INVALID, "0x4", flags=NOISE_PER_PIXEL)
    refused(pt.PT_E_INVALID, "0x4", flags=COUNTS | NOISE_PER_PIXEL)
    refused(pt.PT_E_INVALID, "0x1", flags=NOISE | NOISE_PER_PIXEL)              # planes the per-pixel kernels cannot run on
    refused(pt.PT_E_INVALID, "noise W", noise_W=9.0)
    refused(pt.PT_E_INVALID, "noise W", noise_W=-1.0)
    refused(pt.PT_E_INVALID, "noise W", noise_W=float("nan"))
    refused(pt.PT_E_INVALID, "noise W", noise_W=float(1 << 40))
    refused(pt.PT_E_INVALID, "batches", noise_batches=-1)
    refused(pt.PT_E_INVALID, "n0", noise_n0=9)
    refused(pt.PT_E_INVALID, "n0", noise_n0=-1)
    refused(pt.PT_E_IO, "truncated", cut=1)
    refused(pt.PT_E_INVALID, "bytes", tail=b"\0")
    refused(pt.PT_E_INVALID, "frozen", flags=COUNTS, frozen_pixels=W * H + 1)


def test_a_genuine_version_1_header_names_both_versions(tmp_path):
    """A checkpoint as pt_accum_save lays it out (128-byte header, 48-byte records): not a session file."""
    f = str(tmp_path / "a.ptacc")
    h = session_ref.header(W, H, samples=4, version=1, header_bytes=128)
    with open(f, "wb") as fh:
        fh.write(h.tobytes()[:128] + bytes(W * H * 48))
    assert pt.accum_file_info(f)["samples"] == 4                               # (it is one, to its own reader)
    code, msg = _info(f)
    assert code == pt.PT_E_INVALID and "version 1" in msg and " 2" in msg


def test_an_image_without_pixels(tmp_path):
    f = str(tmp_path / "s.ptses")
    for w, h in ((0, 7), (7, 0)):
        session_ref.write(f, session_ref.header(w, h))
        code, msg = _info(f)
        assert code == pt.PT_E_INVALID and "%dx%d" % (w, h) in msg


def test_the_reader_of_format_1_refuses_a_session_file(tmp_path):
    f = str(tmp_path / "s.ptses")
    session_ref.write(f, session_ref.header(W, H, samples=4))
    assert pt.session_file_info(f)["samples"] == 4
    with pytest.raises(pt.PtError) as e:
        pt.accum_file_info(f)
    assert e.value.code == pt.PT_E_INVALID and "format version 2, this build reads 1" in str(e.value)
