"""Guard bands for device buffers: an Arena is one uint8 allocation laid out as [front guard | payload | back guard],
both guards filled with one byte, so that a store outside the payload is seen afterwards and a load from outside it
reads a chosen poison instead of whatever the allocator left there.  The tests hand `ptr` to a *_device entry point in
place of an exact-sized tensor (test_gpu_guard_bands.py); the helper itself runs on CPU tensors too
(test_guard_bands_host.py).

    a = Arena(w * h * 12, 4, OUT_FILL, "cuda", "tight")      # an output: float32[w*h*3]
    b = Arena(rays.nbytes, 8, 0xFF, "cuda").load(rays)       # an input, poisoned with NaN / prim -1 / covered
    call(b.ptr, a.ptr)
    assert a.guards_intact(), a.describe()
    got = a.read(np.float32, (h, w, 3))

Both guards are at least max(64 KiB, 4 * nbytes) bytes, rounded up to 256: more than a kernel overruns by if it stores
its whole rounded-up grid at the image's row stride, so such a store lands in the arena and nowhere else.  The
payload's last byte is followed directly by the back guard.  Placements of the payload's first byte, both legal for
the alignment include/pt/pt.h documents for the buffer: "wide" on the 256-byte boundary behind the front guard,
"tight" `align` bytes later -- the pointer then has the documented alignment and no more.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
import torch

MIN_GUARD = 64 * 1024
BOUNDARY = 256
PLACEMENTS = ("wide", "tight")
OUT_FILL = 0xA5                 # outputs: the sentinel byte of test_gpu_shard_geometry.py
POISONS = (0x00, 0xFF)          # inputs: 0.0 / prim 0 / uncovered, and NaN / prim -1 / covered
ALIGNMENTS = (16, 8, 4, 1)      # feature records; ray and point buffers; float and int32 images and tables; covered


def guard_bytes(nbytes):
    """The least size of either guard of a payload of nbytes."""
    g = max(MIN_GUARD, 4 * int(nbytes))
    return (g + BOUNDARY - 1) // BOUNDARY * BOUNDARY


class Arena:
    def __init__(self, nbytes, align, fill, device, placement="wide"):
        if align not in ALIGNMENTS or placement not in PLACEMENTS or not 0 <= int(fill) <= 255 or nbytes < 0:
            raise ValueError("Arena(%r, %r, %r, %r, %r)" % (nbytes, align, fill, device, placement))
        self.nbytes, self.align, self.fill, self.placement = int(nbytes), int(align), int(fill), placement
        g = guard_bytes(nbytes)
        # the allocation's own address is not promised to sit on the boundary: up to BOUNDARY - 1 bytes of slack in front
        self.raw = torch.full((g + BOUNDARY + self.align + self.nbytes + g,), self.fill, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        self.start = g + (-(base + g)) % BOUNDARY + (self.align if placement == "tight" else 0)
        self.end = self.start + self.nbytes
        self.total = int(self.raw.numel())
        self.ptr = base + self.start

    # ---- the layout, for the helper's own test
    @property
    def front_bytes(self):
        return self.start

    @property
    def back_bytes(self):
        return self.total - self.end

    # ---- the payload
    def _payload(self):
        return self.raw[self.start:self.end]

    def view(self, dtype, shape):
        """The payload as a torch tensor of `dtype` (a torch dtype) and `shape`: a view, not a copy."""
        return self._payload().view(dtype).view(shape)

    def load(self, array):
        """Copy the bytes of a numpy array (exactly nbytes of them) into the payload; returns self."""
        b = np.frombuffer(np.ascontiguousarray(array).tobytes(), dtype=np.uint8)
        if b.size != self.nbytes:
            raise ValueError("load: %d bytes into a payload of %d" % (b.size, self.nbytes))
        if self.nbytes:
            self._payload().copy_(torch.from_numpy(b.copy()))
        return self

    def fill_payload(self, byte):
        self._payload().fill_(int(byte))
        return self

    def payload_bytes(self):
        """The payload's bytes on the host."""
        return self._payload().cpu().numpy().tobytes()

    def read(self, dtype, shape=(-1,)):
        """The payload on the host as a numpy array of `dtype` (structured ones too) and `shape`."""
        return np.frombuffer(self.payload_bytes(), dtype=dtype).reshape(shape)

    # ---- the guards
    def damage(self):
        """None while every guard byte holds the fill; else (first, last): the offsets of the first and the last changed
        byte relative to the payload's first byte (negative in the front guard, >= nbytes in the back guard)."""
        bad = self.raw != self.fill
        bad[self.start:self.end] = False
        if not bool(bad.any()):
            return None
        idx = torch.nonzero(bad).reshape(-1)
        return int(idx[0]) - self.start, int(idx[-1]) - self.start

    def guards_intact(self):
        return self.damage() is None

    def describe(self):
        d = self.damage()
        if d is None:
            return "guards intact"
        where = lambda o: "%d (front guard)" % o if o < 0 else "%d (back guard, %d past the end)" % (o, o - self.nbytes)
        return "guard bytes changed: first at offset %s, last at offset %s of a %d-byte payload (%s, align %d)" % (
            where(d[0]), where(d[1]), self.nbytes, self.placement, self.align)
