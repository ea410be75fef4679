"""The pt_accum_* entry points without a device: argument checks, and the checkpoint header as pt.h documents
it -- packed here by hand, field by field, so the format is pinned by this file and not by the library."""
import ctypes as C
import struct

import pytest

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib

MAGIC = b"PTACCUM\0"
HEADER_BYTES = 128
RECORD_BYTES = 48
W, H = 5, 3


def _header(magic=MAGIC, version=1, header_bytes=HEADER_BYTES, width=W, height=H, samples=7, digest=0x1122334455667788):
    params = struct.pack("<6iQ5i4x", width, height, 0, 3, 1, 0x2, 4321, 1, 3, 0, 16, 8)   # 56 B, spp = 0
    cam = struct.pack("<6f2i", 0.0, 1.0, 3.0, 1.0, 3.0, 0.05, width, height)              # 32 B
    h = struct.pack("<8sII", magic, version, header_bytes) + params + cam + struct.pack("<qQII", samples, digest, 36, 2)
    assert len(h) == HEADER_BYTES
    return h


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p).encode()


def _info(path):
    L = _lib.lib()
    p, cam, n, dg = _lib.Params(), _lib.Camera(), C.c_int64(-1), C.c_uint64(0)
    rc = L.pt_accum_file_info(path, C.byref(p), C.byref(cam), C.byref(n), C.byref(dg))
    return rc, p, cam, n.value, dg.value, (L.pt_last_error() or b"").decode()


def test_null_and_invalid_arguments():
    L = _lib.lib()
    err = C.c_int(0)
    p, cam = _lib.Params(), _lib.Camera()

    def msg():
        return (L.pt_last_error() or b"").decode()

    assert not L.pt_accum_create(None, C.byref(p), C.byref(cam), C.byref(err))
    assert err.value == _lib.PT_E_INVALID and "pt_accum_create" in msg()
    assert not L.pt_accum_create(None, None, None, None)          # (a null err pointer too)
    assert L.pt_accum_add(None, 4, None, None, None) == _lib.PT_E_INVALID and "pt_accum_add" in msg()
    assert L.pt_accum_read(None, None, None) == _lib.PT_E_INVALID and "pt_accum_read" in msg()
    assert L.pt_accum_save(None, b"/nonexistent/x") == _lib.PT_E_INVALID and "pt_accum_save" in msg()
    err.value = 0
    assert not L.pt_accum_load(None, b"/nonexistent/x", C.byref(err))
    assert err.value == _lib.PT_E_INVALID and "pt_accum_load" in msg()
    assert L.pt_accum_file_info(None, None, None, None, None) == _lib.PT_E_INVALID and "pt_accum_file_info" in msg()
    assert L.pt_accum_samples(None) == 0
    L.pt_accum_destroy(None)


def test_file_info_reads_a_hand_packed_header(tmp_path):
    path = _write(tmp_path, "ok.ptacc", _header() + bytes(W * H * RECORD_BYTES))
    rc, p, cam, n, dg, _ = _info(path)
    assert rc == _lib.PT_OK
    assert (p.width, p.height, p.spp, p.bounces, p.integrator, p.flags, p.seed) == (W, H, 0, 3, 1, 0x2, 4321)
    assert (p.shard_index, p.shard_count, p.pixel_order, p.tile_w, p.tile_h) == (1, 3, 0, 16, 8)
    assert (cam.pos.x, cam.pos.y, cam.pos.z) == (0.0, 1.0, 3.0)
    assert (cam.dist_from_film, cam.focal_length, cam.pxl_width, cam.pxl_height) == (1.0, 3.0, W, H)
    assert abs(cam.radius - 0.05) < 1e-7
    assert n == 7 and dg == 0x1122334455667788
    # any out pointer may be null; the Python wrapper agrees
    assert _lib.lib().pt_accum_file_info(path, None, None, None, None) == _lib.PT_OK
    info = pt.accum_file_info(path.decode())
    assert info["samples"] == 7 and info["scene_digest"] == dg and info["params"].seed == 4321


@pytest.mark.parametrize("name,data,code", [
    ("magic", _header(magic=b"PTACCUX\0") + bytes(W * H * RECORD_BYTES), _lib.PT_E_INVALID),
    ("version", _header(version=2) + bytes(W * H * RECORD_BYTES), _lib.PT_E_INVALID),
    ("hsize", _header(header_bytes=120) + bytes(W * H * RECORD_BYTES), _lib.PT_E_INVALID),
    ("short_header", _header()[:HEADER_BYTES - 1], _lib.PT_E_IO),
    ("empty", b"", _lib.PT_E_IO),
    ("truncated", _header() + bytes(W * H * RECORD_BYTES - 1), _lib.PT_E_IO),
    ("too_long", _header() + bytes(W * H * RECORD_BYTES + 48), _lib.PT_E_INVALID),
])
def test_file_info_rejects(tmp_path, name, data, code):
    rc, _, _, n, _, msg = _info(_write(tmp_path, name + ".ptacc", data))
    assert rc == code and "pt_accum_file_info" in msg
    assert n == -1                                                # nothing written on failure


def test_file_info_missing_file(tmp_path):
    rc, _, _, _, _, msg = _info(str(tmp_path / "absent.ptacc").encode())
    assert rc == _lib.PT_E_IO and "cannot open" in msg
    with pytest.raises(pt.PtError) as e:
        pt.accum_file_info(str(tmp_path / "absent.ptacc"))
    assert e.value.code == pt.PT_E_IO
