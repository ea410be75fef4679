"""The shard geometries of tests/test_gpu_shard_geometry.py and of the `grid` probe cases in
tests/test_render_plan_host.py: tiles larger than 8x8 on images they do not divide, uneven shards, and shards that
own no tile at all (shard_index >= the tile count).  The pixel counts are shard.shard_pixels' on the CPU, written
down so that a change of the mapping is noticed.

    id: (width, height, tile_w, tile_h, shard_count, pixel_order, pixels per shard)
"""
GEOMETRIES = {
    "A": (24, 16, 16, 8, 3, 0, (192, 64, 128)),          # 2 blocks per tile, partial right-hand tiles, uneven shards
    "B": (24, 16, 16, 8, 6, 0, (128, 64, 128, 64, 0, 0)),  # two empty shards beside four that own pixels
    "C": (20, 13, 16, 24, 3, 0, (208, 52, 0)),           # tile taller than the image, 6 blocks per tile, one empty shard
    "D": (37, 19, 32, 8, 4, 0, (352, 55, 256, 40)),      # 4 blocks in a row, ragged in both directions
    "E": (20, 13, 256, 256, 2, 0, (260, 0)),             # one tile of 65536 slots holding 260 pixels
    "F": (32, 32, 16, 8, 3, 1, (384, 384, 256)),         # non-square tiles with PT_ORDER_MORTON
    "G": (1, 1, 8, 8, 2, 0, (1, 0)),                     # the smallest image
}


class Geometry:
    def __init__(self, gid):
        self.id = gid
        self.w, self.h, self.tw, self.th, self.shards, self.order, self.pixels = GEOMETRIES[gid]

    def __repr__(self):
        return "%s:%dx%d/%dx%d/%d" % (self.id, self.w, self.h, self.tw, self.th, self.shards)

    def nonempty(self):
        return [k for k in range(self.shards) if self.pixels[k]]

    def empty(self):
        return [k for k in range(self.shards) if not self.pixels[k]]
