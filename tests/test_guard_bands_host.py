"""The arena helper of the guard-band tests (tests/guard_bands.py) on CPU tensors: its layout arithmetic, and that a
write outside the payload is reported where it happened.  This is the demonstration that an overrun would be seen; no
kernel is ever broken on purpose to show it."""
import numpy as np
import pytest
import torch

import guard_bands as gb
from guard_bands import Arena

SIZES = [0, 1, 12, 48, 37 * 19 * 12, 65 * 33 * 48]


@pytest.mark.parametrize("placement", gb.PLACEMENTS)
@pytest.mark.parametrize("align", gb.ALIGNMENTS)
def test_layout(align, placement):
    for n in SIZES:
        g = gb.guard_bytes(n)
        assert g % 256 == 0 and g >= 64 * 1024 and g >= 4 * n and g - 256 < max(64 * 1024, 4 * n)
        a = Arena(n, align, gb.OUT_FILL, "cpu", placement)
        assert a.ptr == a.raw.data_ptr() + a.start and a.ptr % align == 0
        if placement == "wide":
            assert a.ptr % 256 == 0
        else:
            assert a.ptr % 256 == align                       # the documented alignment and no more
            assert align == 1 or a.ptr % (2 * align) != 0
        # everything in front of the payload is front guard, everything behind it back guard; both are large enough
        assert a.front_bytes == a.start >= g and a.back_bytes == a.total - a.end >= g
        assert a.end - a.start == n and a.front_bytes + n + a.back_bytes == a.raw.numel()
        assert a.front_bytes < g + 256 + align + 1
        raw = a.raw.numpy()
        assert (raw == gb.OUT_FILL).all() and a.guards_intact() and a.damage() is None


@pytest.mark.parametrize("placement", gb.PLACEMENTS)
@pytest.mark.parametrize("align", gb.ALIGNMENTS)
def test_the_payload_abuts_the_back_guard(align, placement):
    n = 37 * 19 * 4
    a = Arena(n, align, 0xFF, "cpu", placement)
    a.fill_payload(0x11)
    raw = a.raw.numpy()
    assert (raw[:a.start] == 0xFF).all() and (raw[a.start:a.start + n] == 0x11).all() and (raw[a.start + n:] == 0xFF).all()
    assert raw[a.start + n - 1] == 0x11 and raw[a.start + n] == 0xFF        # no padding between payload and guard
    assert a.guards_intact()
    if align == 1:                                                          # (a byte buffer: `covered`)
        v = a.view(torch.uint8, (19, 37 * 4))
        v[18, 37 * 4 - 1] = 0x22
        assert v.data_ptr() == a.ptr and a.guards_intact() and raw[a.start + n - 1] == 0x22
        return
    v = a.view(torch.float32, (19, 37))
    assert v.data_ptr() == a.ptr and v.numel() * 4 == n
    v[18, 36] = 1.0                                                         # the last element ends where the guard begins
    assert a.guards_intact() and raw[a.start + n - 4:a.start + n].tobytes() == np.float32(1.0).tobytes()


@pytest.mark.parametrize("placement", gb.PLACEMENTS)
@pytest.mark.parametrize("align", gb.ALIGNMENTS)
@pytest.mark.parametrize("fill", [gb.OUT_FILL, 0x00, 0xFF])
def test_a_one_byte_write_outside_is_reported_where_it_is(align, placement, fill):
    n = 65 * 33
    other = 0x5A
    spots = {"just before": lambda a: a.start - 1, "just after": lambda a: a.end, "the front guard's far end": lambda a: 0,
             "the back guard's far end": lambda a: a.total - 1}
    for name, spot in spots.items():
        a = Arena(n, align, fill, "cpu", placement)
        at = spot(a)
        a.raw[at] = other
        assert not a.guards_intact(), name
        assert a.damage() == (at - a.start, at - a.start), name
        assert str(at - a.start) in a.describe(), name
    a = Arena(n, align, fill, "cpu", placement)
    a.raw[a.start - 1] = other
    a.raw[a.end] = other
    assert a.damage() == (-1, n)
    assert "front guard" in a.describe() and "0 past the end" in a.describe()
    # writes inside the payload are no damage, whatever they are
    a = Arena(n, align, fill, "cpu", placement)
    a.raw[a.start] = other
    a.raw[a.end - 1] = other
    assert a.guards_intact() and a.describe() == "guards intact"
    # a byte that is rewritten with the fill itself cannot be seen: the reason inputs are run under two poisons
    a.raw[a.end] = fill
    assert a.guards_intact()


@pytest.mark.parametrize("placement", gb.PLACEMENTS)
def test_load_round_trips(placement):
    rng = np.random.default_rng(3)
    rec = np.dtype([("a", "<f4", (3,)), ("d", "<f4"), ("n", "<f4", (3,)), ("prim", "<i4"), ("p", "<f4", (3,)), ("r", "<f4")])
    for align, data in ((4, rng.random((19, 37, 3)).astype(np.float32)), (8, rng.random((65 * 33, 6)).astype(np.float32)),
                        (1, (rng.random((33, 65)) < 0.5).astype(np.uint8)), (4, rng.integers(-5, 5, 257).astype(np.int32)),
                        (16, np.frombuffer(rng.bytes(48 * 7), dtype=rec))):
        a = Arena(data.nbytes, align, 0x00, "cpu", placement).load(data)
        assert a.payload_bytes() == data.tobytes() and a.guards_intact()
        assert a.read(data.dtype, data.shape).tobytes() == data.tobytes()
        with pytest.raises(ValueError):
            a.load(np.zeros(data.nbytes + 1, np.uint8))
    with pytest.raises(ValueError):
        Arena(16, 3, 0, "cpu")
    with pytest.raises(ValueError):
        Arena(16, 4, 0, "cpu", "loose")
