"""numpy reader and writer of the session file format (include/pt/pt.h, "session files"), written from the format's
table and not from the C++:

      0  "PTACCUM\\0"   8 uint32 version = 2   12 uint32 header bytes = 192
     16  pt_params 56 B (spp 0)   72 pt_camera 32 B   104 int64 samples   112 uint64 digest   120 uint32 num_tris, num_spheres
    128  uint32 flags (0x1 COUNTS, 0x2 NOISE, 0x4 NOISE_PER_PIXEL)   132 uint32 0
    136  int64 noise n0   144 f64 noise W   152 int32 noise batches   156 uint32 0   160 uint64 frozen pixels   168..191 zero
    192  sections of W*H entries in scanline order: A 48 B always, B 4 B (COUNTS), C 40 B (NOISE), D 8 B (NOISE_PER_PIXEL)

    read(path) -> dict(header fields..., A=, B=, C=, D=)    (absent sections: None)
    write(path, header dict, A=None, B=None, C=None, D=None, tail=b"")   (A None: zeros; sections follow the flags)
"""
import numpy as np

MAGIC = b"PTACCUM\0"
COUNTS, NOISE, NOISE_PER_PIXEL = 0x1, 0x2, 0x4
ACTIVE = 0xFFFFFFFF

PARAMS = np.dtype([("width", "<i4"), ("height", "<i4"), ("spp", "<i4"), ("bounces", "<i4"), ("integrator", "<i4"),
                   ("flags", "<u4"), ("seed", "<u8"), ("shard_index", "<i4"), ("shard_count", "<i4"),
                   ("pixel_order", "<i4"), ("tile_w", "<i4"), ("tile_h", "<i4"), ("pad", "<u4")])
CAMERA = np.dtype([("pos", "<f4", (3,)), ("dist_from_film", "<f4"), ("focal_length", "<f4"), ("radius", "<f4"),
                   ("pxl_width", "<i4"), ("pxl_height", "<i4")])
HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("header_bytes", "<u4"), ("params", PARAMS), ("camera", CAMERA),
                   ("samples", "<i8"), ("scene_digest", "<u8"), ("num_tris", "<u4"), ("num_spheres", "<u4"),
                   ("flags", "<u4"), ("zero0", "<u4"), ("noise_n0", "<i8"), ("noise_W", "<f8"), ("noise_batches", "<i4"),
                   ("zero1", "<u4"), ("frozen_pixels", "<u8"), ("zero2", "V24")])
REC_A = np.dtype([("rng", "<u4", (6,)), ("mean", "<f8", (3,))])
REC_B = np.dtype("<u4")
REC_C = np.dtype([("prev", "<f8", (3,)), ("mu", "<f8"), ("m2", "<f8")])
REC_D = np.dtype([("W_q", "<u4"), ("b_q", "<u4")])
assert PARAMS.itemsize == 56 and CAMERA.itemsize == 32 and HEADER.itemsize == 192
assert (REC_A.itemsize, REC_B.itemsize, REC_C.itemsize, REC_D.itemsize) == (48, 4, 40, 8)
assert HEADER.fields["flags"][1] == 128 and HEADER.fields["noise_n0"][1] == 136 and HEADER.fields["frozen_pixels"][1] == 160

SECTIONS = (("A", REC_A, 0), ("B", REC_B, COUNTS), ("C", REC_C, NOISE), ("D", REC_D, NOISE_PER_PIXEL))


def header(width, height, samples=0, flags=0, noise_n0=0, noise_W=0.0, noise_batches=0, frozen_pixels=0, version=2,
           header_bytes=192, magic=MAGIC, bounces=3, integrator=0, seed=1234, shard_index=0, shard_count=1,
           pixel_order=0, tile_w=0, tile_h=0, scene_digest=0x1234567890ABCDEF, num_tris=12, num_spheres=0):
    """A header record with every field given or defaulted (the camera: the Cornell one)."""
    h = np.zeros((), dtype=HEADER)
    h["magic"], h["version"], h["header_bytes"] = magic, version, header_bytes
    p = h["params"]
    p["width"], p["height"], p["bounces"], p["integrator"], p["seed"] = width, height, bounces, integrator, seed
    p["shard_index"], p["shard_count"], p["pixel_order"], p["tile_w"], p["tile_h"] = shard_index, shard_count, pixel_order, tile_w, tile_h
    c = h["camera"]
    c["pos"], c["dist_from_film"], c["focal_length"], c["radius"] = (0.0, 1.0, 3.0), 1.0, 3.0, 0.0
    c["pxl_width"], c["pxl_height"] = width, height
    h["samples"], h["scene_digest"], h["num_tris"], h["num_spheres"] = samples, scene_digest, num_tris, num_spheres
    h["flags"], h["noise_n0"], h["noise_W"], h["noise_batches"], h["frozen_pixels"] = flags, noise_n0, noise_W, noise_batches, frozen_pixels
    return h


def write(path, h, A=None, B=None, C=None, D=None, tail=b"", cut=0):
    """The file of header `h` and the sections its flags name (None: all zero); `tail` is appended, `cut` bytes are
    cut off the end."""
    n = max(int(h["params"]["width"]), 0) * max(int(h["params"]["height"]), 0)
    given = dict(A=A, B=B, C=C, D=D)
    blob = h.tobytes()
    for name, dt, flag in SECTIONS:
        if flag and not int(h["flags"]) & flag:
            continue
        sec = given[name]
        sec = np.zeros(n, dtype=dt) if sec is None else np.ascontiguousarray(sec, dtype=dt).reshape(-1)
        assert sec.size == n
        blob += sec.tobytes()
    blob += tail
    if cut:
        blob = blob[:-cut]
    with open(path, "wb") as f:
        f.write(blob)


def read(path):
    """dict(header=the HEADER record, A=, B=, C=, D=): each section as an (H, W) array of its record type, None when
    the flags do not name it.  Asserts the file's size."""
    blob = open(path, "rb").read()
    h = np.frombuffer(blob[:192], dtype=HEADER)[0]
    assert h["magic"] == MAGIC.rstrip(b"\0") or bytes(blob[:8]) == MAGIC
    assert h["version"] == 2 and h["header_bytes"] == 192
    w, hh = int(h["params"]["width"]), int(h["params"]["height"])
    out, off = dict(header=h), 192
    for name, dt, flag in SECTIONS:
        if flag and not int(h["flags"]) & flag:
            out[name] = None
            continue
        out[name] = np.frombuffer(blob, dtype=dt, count=w * hh, offset=off).reshape(hh, w)
        off += w * hh * dt.itemsize
    assert off == len(blob), (off, len(blob))
    assert bytes(blob[132:136]) == b"\0" * 4 and bytes(blob[156:160]) == b"\0" * 4 and bytes(blob[168:192]) == b"\0" * 24
    return out
