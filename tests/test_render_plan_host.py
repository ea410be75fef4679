"""The render's host decisions, checked without a GPU: the work-unit plan (pt::plan_units), the tile grid
(pt::tile_grid, pt::validate_render, pt_shard_pixels) and the scene packer (pt::pack_scene).

tests/host_probe.cpp calls them in libptamd.so directly and prints JSON; `make host_probe` (not part of `all`)
builds it.  The GPU suite checks the same code in place: bit equality of every render with the oracle, and the
exact work_units / split_pixels of pt_stats under the PT_WF_* and PT_LBUF_BUDGET_MB settings.
"""
import json
import os
import random
import subprocess

import pytest

from conftest import MODELS, ROOT
from shard_geometries import GEOMETRIES, Geometry

CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
PROBE = os.path.join(CSRC, "build", "host_probe")
CUS = 256
LDS_FIXED = 21088   # integrator 0's block: 4 x 5120 B of rings + 160 B of counters + 208 + 240 B of probe and light records
PLAN_KEYS = ("nwhole", "ntail", "nmid", "chunks_mid", "chunks", "nfin", "chunks_fin", "nunits", "blocks")


@pytest.fixture(scope="module")
def probe():
    # every run: a probe left from an earlier build would call the library with stale struct layouts (the
    # target depends on the shared headers, never on the library, so this costs nothing when nothing changed)
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_probe"])

    def run(args, lines=None):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
        # (the probe's rpath names the library's directory at build time; a moved tree finds it here)
        env["LD_LIBRARY_PATH"] = os.pathsep.join(filter(None, [os.path.join(ROOT, "cudapathtracer_amd"), env.get("LD_LIBRARY_PATH")]))
        out = subprocess.run([PROBE] + list(args), input="\n".join(lines or []) + "\n", env=env, text=True,
                             stdout=subprocess.PIPE, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


def plan_line(npix, spp, budget="inf", env=None, head=0, count=0):
    return " ".join([str(npix), str(spp), str(CUS), str(head), str(count), str(LDS_FIXED), str(budget)] +
                    ["%s=%s" % kv for kv in (env or {}).items()])


# (npix, spp, budget callable's answer in bytes, knobs) -> nwhole, ntail, nmid, chunks_mid, chunks, nfin, chunks_fin,
# nunits, blocks: a by-hand restatement of render_enqueue's arithmetic before it moved, with 256 CUs, integrator 0 and
# default knobs.  Rows 1-5, 7 and 10-12 were also read from pt_stats (work_units, split_pixels) of renders of the
# Cornell fixture on an MI355X before the move.
PLAN_TABLE = [
    (4096, 16, "inf", {}, (0, 4096, 0, 1, 8, 4096, 16, 65536, 256)),
    (3072, 6, "inf", {}, (0, 3072, 0, 1, 6, 0, 1, 18432, 72)),
    (3072, 6, 2097, {}, (3058, 14, 0, 1, 6, 0, 1, 3142, 13)),
    (3072, 6, 0, {}, (3072, 0, 0, 1, 1, 0, 1, 3072, 12)),
    (2073600, 8, "inf", {}, (1582080, 491520, 0, 1, 6, 65536, 8, 4662272, 1280)),
    (2073600, 256, "inf", {}, (1582080, 491520, 0, 1, 6, 65536, 64, 8332288, 1280)),
    (518400, 8, "inf", {}, (163840, 354560, 190720, 3, 8, 0, 1, 2046720, 1280)),
    (518400, 256, "inf", {}, (163840, 354560, 190720, 3, 8, 65536, 64, 5716736, 1280)),
    (259200, 256, "inf", {}, (0, 259200, 95360, 3, 8, 65536, 64, 5266816, 1280)),
    (4096, 1, "inf", {}, (4096, 0, 0, 1, 1, 0, 1, 4096, 16)),
    (4096, 16, "inf", {"PT_WF_CHUNKS": 4, "PT_WF_TAIL_NPIX": 37}, (4059, 37, 0, 1, 4, 37, 16, 4651, 19)),
    (4096, 16, "inf", {"PT_WF_CHUNKS": 3}, (0, 4096, 0, 1, 3, 4096, 16, 65536, 256)),
    # the 32-bit guard: splitting 65528^2 pixel slots would number more than 2^32-1 units, so all stay whole
    (65528 * 65528, 256, "inf", {}, (65528 * 65528, 0, 0, 1, 1, 0, 1, 65528 * 65528, 1280)),
]


def test_plan_units_table(probe):
    got = probe(["plan"], [plan_line(n, s, b, e) for n, s, b, e, _ in PLAN_TABLE])
    assert len(got) == len(PLAN_TABLE)
    for (npix, spp, budget, env, want), g in zip(PLAN_TABLE, got):
        assert g["rc"] == 0 and g["npix"] == npix
        assert tuple(g[k] for k in PLAN_KEYS) == want, (npix, spp, budget, env)


def test_plan_units_budget_in_mb_is_the_callables_budget(probe):
    """PT_LBUF_BUDGET_MB=0.002 is the 2097 bytes of the table's third row (split_pixels == 14 in
    tests/test_gpu_parity.py), and the callable is then not asked."""
    g, = probe(["plan"], [plan_line(3072, 6, "inf", {"PT_LBUF_BUDGET_MB": "0.002"})])
    assert tuple(g[k] for k in PLAN_KEYS) == PLAN_TABLE[2][4] and g["budget_calls"] == 0


def nothing_to_split(npix, spp, env, wpc):
    """The settings under which no pixel can be split whatever the budget: one sample per pixel, an explicit
    tail of no pixels or of one chunk, and, on a frame large enough to take the whole-pixels-then-tail rule
    (npix >= 2.5 lanes), one tail chunk or no tail pixels per lane.  (Small shards choose their chunk count
    from npix and are not predicted here.)"""
    chunks_all = int(env.get("PT_WF_CHUNKS", 0))
    tail_chunks = int(env.get("PT_WF_TAIL_CHUNKS", 6))
    if spp == 1:
        return True
    if "PT_WF_TAIL_NPIX" in env:
        return int(env["PT_WF_TAIL_NPIX"]) == 0 or (chunks_all if chunks_all > 0 else tail_chunks) <= 1
    if chunks_all > 0:
        return chunks_all == 1
    lanes = CUS * max(1, wpc // 4) * 256
    if 2 * npix >= 5 * lanes:
        return tail_chunks <= 1 or float(env.get("PT_WF_TAIL_PX", 1.5)) == 0
    return False


def test_plan_units_invariants(probe):
    rng = random.Random(20261019)
    cases = []
    for _ in range(400):
        npix = rng.choice([64, 640, 4096, 65536, 259200, 518400, 2073600, rng.randrange(1, 1 << 22) * 64,
                           rng.randrange((1 << 26) - 4096, 1 << 26) * 64 - 64 * rng.randrange(2)])
        spp = rng.choice([1, 2, 3, 5, 8, 16, 63, 64, 65, 256, 4096])
        env = {}
        for key, values in (("PT_WF_CHUNKS", [0, 1, 2, 7, 300]), ("PT_WF_TAIL_CHUNKS", [0, 1, 2, 6, 9]),
                            ("PT_WF_TAIL_PX", [0, 0.3, 1.5, 40]), ("PT_WF_TAIL_NPIX", [0, 1, 37, 100000, 1 << 33]),
                            ("PT_WF_MID_CHUNKS", [-1, 0, 1, 2, 5]), ("PT_WF_FINE_PX", [0, 0.5, 3]),
                            ("PT_WF_FINE_CHUNKS", [0, 2, 12]), ("PT_WF_WHOLE_PX", [0, 0.5, 2]), ("PT_WF_WHOLE_MIN", [0, 1.25, 9]),
                            ("PT_WF_FIN_PX", [0, 0.2, 5]), ("PT_WF_FIN_CHUNKS", [0, 4, 64, 1000]), ("PT_WF_MIN_WAVES", [4, 5, 6]),
                            ("PT_WF_WAVES_PER_CU", [4, 20, 32])):
            if rng.random() < 0.25:
                env[key] = rng.choice(values)
        budget = rng.choice(["inf", "inf", 0, 1, 2097, 1 << 20, 1 << 30, 1 << 36])
        if rng.random() < 0.25:
            env["PT_LBUF_BUDGET_MB"] = rng.choice(["0", "0.002", "1", "64", "1e6"])
        cases.append((npix, spp, budget, env, rng.randrange(2), rng.randrange(2)))
    got = probe(["plan"], [plan_line(n, s, b, e, h, c) for n, s, b, e, h, c in cases])
    assert len(got) == len(cases)
    split_seen = called = nothing = 0
    for (npix, spp, budget, env, head, count), g in zip(cases, got):
        what = (npix, spp, budget, env, head, count, g)
        assert g["rc"] == 0 and g["npix"] == npix
        assert g["nunits"] == (g["nwhole"] + g["nmid"] * g["chunks_mid"] + (g["ntail"] - g["nmid"] - g["nfin"]) * g["chunks"] +
                               g["nfin"] * g["chunks_fin"]), what
        assert g["nwhole"] + g["ntail"] == npix, what
        assert g["nmid"] + g["nfin"] <= g["ntail"], what
        biggest = max(g["chunks"], g["chunks_mid"], g["chunks_fin"])
        assert all(1 <= g[k] <= spp for k in ("chunks", "chunks_mid", "chunks_fin")), what
        assert npix + g["ntail"] * (biggest - 1) <= 2**32 - 1, what
        assert 1 <= g["blocks"] <= CUS * max(1, g["wpc"] // 4) and g["blocks"] * 256 < g["nunits"] + 256, what
        assert 1 <= g["top_nodes"] <= 97, what
        # the budget is asked at most once, and never when the environment gives it or when nothing was to be split
        assert g["budget_calls"] <= 1, what
        if "PT_LBUF_BUDGET_MB" in env or nothing_to_split(npix, spp, env, g["wpc"]):
            assert g["budget_calls"] == 0, what
            nothing += "PT_LBUF_BUDGET_MB" not in env
        if g["budget_calls"] == 0 and "PT_LBUF_BUDGET_MB" not in env:
            assert g["ntail"] == 0, what    # (asked whenever pixels are split)
        split_seen += g["ntail"] > 0
        called += g["budget_calls"]
    assert split_seen > 100 and called > 100 and nothing > 40   # (the cases do reach these paths)


def test_tile_grid_shards_partition_the_image(probe):
    cases = [(w, h, t, t, s, 4) for w in (63, 64, 65) for h in (47, 48, 49) for t in (0, 8, 16, 256) for s in range(4)]
    got = probe(["grid"], [" ".join(map(str, c)) for c in cases])
    assert len(got) == len(cases)
    for i in range(0, len(cases), 4):
        w, h, t = cases[i][:3]
        shards = got[i:i + 4]
        tw = t or 8
        for g in shards:
            assert g["validate_rc"] == 0 and g["shard_pixels_rc"] == 0 and g["fits"]
            assert (g["tile_w"], g["tile_h"]) == (tw, tw)
            assert g["tiles_x"] == -(-w // tw) and g["ntiles"] == -(-w // tw) * -(-h // tw)
            assert g["tile_bx"] == tw // 8 and g["tile_blocks"] == (tw // 8) ** 2
            assert g["npix"] == g["ntiles_shard"] * tw * tw
            assert g["grid_slots"] == g["ntiles"] * tw * tw
        assert sum(g["ntiles_shard"] for g in shards) == shards[0]["ntiles"]
        assert sum(g["in_image"] for g in shards) == w * h


def test_tile_grid_of_the_gpu_shard_geometries(probe):
    """tests/shard_geometries.py: non-square tiles larger than 8x8 on images they do not divide, and shards with
    shard_index >= ntiles, which are legal and own nothing.  pt::tile_grid and pt_shard_pixels against shard.py."""
    from cudapathtracer_amd import shard
    cases = [(Geometry(g), k) for g in sorted(GEOMETRIES) for k in range(Geometry(g).shards)]
    got = probe(["grid"], ["%d %d %d %d %d %d" % (g.w, g.h, g.tw, g.th, k, g.shards) for g, k in cases])
    assert len(got) == len(cases)
    empty = 0
    for (g, k), r in zip(cases, got):
        pix = shard.shard_pixels(g.w, g.h, k, g.shards, g.tw, g.th)
        tiles = shard.shard_tiles(g.w, g.h, k, g.shards, g.tw, g.th)
        tx, ty = shard.tiles_shape(g.w, g.h, g.tw, g.th)
        assert len(pix) == g.pixels[k], (g, k)
        assert r["validate_rc"] == 0 and r["shard_pixels_rc"] == 0 and r["fits"], (g, k)
        assert (r["tile_w"], r["tile_h"], r["tiles_x"], r["ntiles"]) == (g.tw, g.th, tx, tx * ty), (g, k)
        assert (r["tile_bx"], r["tile_blocks"]) == (g.tw // 8, (g.tw // 8) * (g.th // 8)), (g, k)
        assert r["in_image"] == len(pix) and r["ntiles_shard"] == len(tiles), (g, k)
        assert r["npix"] == len(tiles) * g.tw * g.th and r["grid_slots"] == tx * ty * g.tw * g.th, (g, k)
        if k >= tx * ty:
            assert r["ntiles_shard"] == 0 and r["npix"] == 0 and r["in_image"] == 0, (g, k)
            empty += 1
    assert empty == 5                                      # B: 2, C, E and G: 1 each
    for g in map(Geometry, sorted(GEOMETRIES)):            # the shards partition the image
        every = sorted(p for k in range(g.shards) for p in shard.shard_pixels(g.w, g.h, k, g.shards, g.tw, g.th))
        assert every == list(range(g.w * g.h)), g


def test_plan_units_of_an_empty_shard(probe):
    """npix == 0: the empty plan whatever the knobs say, and the budget is not asked (no division by npix)."""
    envs = [{}, {"PT_WF_CHUNKS": 4}, {"PT_WF_CHUNKS": 4, "PT_WF_TAIL_NPIX": 37}, {"PT_WF_TAIL_CHUNKS": 1},
            {"PT_WF_FIN_CHUNKS": 64, "PT_WF_FIN_PX": 5}]
    cases = [(spp, e, head) for spp in (1, 9) for e in envs for head in (0, 1)]
    got = probe(["plan"], [plan_line(0, spp, "inf", e, head=head) for spp, e, head in cases])
    assert len(got) == len(cases)
    for case, g in zip(cases, got):
        assert g["rc"] == 0 and g["npix"] == 0 and g["budget_calls"] == 0, case
        assert tuple(g[k] for k in PLAN_KEYS) == (0, 0, 0, 1, 1, 0, 1, 0, 0), case
        assert g["wpc"] == 20 and 1 <= g["top_nodes"] <= 97, case


def test_tile_grid_rejects_more_than_2_32_slots(probe):
    """65535 pads to 65536 in tiles of 8 or of 256: 2^32 slots, one more than a 32-bit unit index numbers."""
    got = probe(["grid"], ["65535 65535 0 0 0 1", "65535 65535 256 256 0 1", "65535 65535 8 8 1 2", "65528 65535 0 0 0 4096"])
    for g in got[:3]:
        assert g["grid_slots"] == 2**32 and not g["fits"]
        assert g["validate_rc"] == -1 and g["shard_pixels_rc"] == -1   # PT_E_INVALID
    # one tile column less fits (a 1/4096 shard of it, so that pt_shard_pixels walks 2^20 slots, not 2^32)
    g = got[3]
    assert g["fits"] and g["validate_rc"] == 0 and g["shard_pixels_rc"] == 0
    assert g["grid_slots"] == 65528 * 65536 and g["npix"] * 4096 == g["grid_slots"]


@pytest.mark.parametrize("name", ["cornell", "cornell_blob", "quad", "spheres"])
def test_pack_scene(probe, name):
    p, = probe(["pack", name, MODELS])
    assert p["rc"] == 0
    nt, n4 = p["nt"], p["n4"]
    assert p["digest_first"] == p["digest_second"]            # packing twice gives equal bytes
    assert p["last_light_prim"] == 0                          # lights[num_lights]: "nothing picked"
    assert p["sizes"]["lights"] == p["num_lights"] + 1
    if name == "spheres":
        assert nt == 0 and n4 == 0 and p["node4_mask"] == 1 and p["top_nodes"] == 0
        assert all(p["sizes"][k] == 0 for k in ("nodes", "rnodes", "tris_leaf", "tris_orig", "nodes4", "acc_tris"))
        assert p["sizes"]["spheres"] == 2 and p["sizes"]["mats"] == 2
        return
    assert nt >= 2 and p["sizes"]["nodes"] == p["sizes"]["rnodes"] == p["nn"] == nt - 1
    assert sorted(p["tris_leaf_id"]) == list(range(nt))
    assert sorted(p["acc_id"]) == list(range(nt))
    assert p["hrec_id"] == p["acc_id"] and p["hrec_parent"] == p["acc_parent"]
    assert all(x < p["nn"] for x in p["acc_parent"])
    # the BVH4: inner children in range, the leaf children's slots (first slot of the node, mask within kLeafBits)
    # cover every triangle slot once
    LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
    assert len(p["child"]) == 4 * n4 and p["sizes"]["nodes4"] == n4
    assert n4 <= p["node4_mask"] + 1 <= max(2, 2 * n4 - 1)
    slots, parent = [], {}
    for node in range(n4):
        for c in p["child"][4 * node:4 * node + 4]:
            if c == EMPTY:
                continue
            if c & LEAF:
                base, mask = (c & ~LEAF) >> p["leaf_bits"], c & ((1 << p["leaf_bits"]) - 1)
                assert mask != 0
                slots += [base + b for b in range(p["leaf_bits"]) if mask >> b & 1]
            else:
                assert c < n4 and c != 0 and c not in parent   # (a tree: node 0 is the root, one parent each)
                parent[c] = node
    assert sorted(slots) == list(range(nt))
    assert sorted(parent) == list(range(1, n4))
    # the LDS-staged top is a connected subtree from the root
    top = p["top_nodes"]
    assert top == min(n4, p["top_nodes_max"])
    assert all(parent[c] < top for c in range(1, top))


# pt::wavefront_variant: (head, count, accum, lds_tree, PT_WF_MIN_WAVES, PT_HEAD_MIN_WAVES) -> the instance's
# (head, count, min_waves, lds_walk, accum), ANY standing for every value of that input.  The table is the launch
# ladder of render_enqueue before the choice moved, row by row, quirks included: integrator 1 counts at 5 waves
# whatever PT_HEAD_MIN_WAVES says and has no LDS walk; integrator 0 counts at 5 waves for PT_WF_MIN_WAVES=6, and its
# 4- and 6-wave instances ignore the LDS tree.
ANY = None
VARIANT_TABLE = [
    ((1, 0, 1, ANY, ANY, ANY), (1, 0, 5, 0, 1)),   # render_head_accum_wf
    ((1, 1, 0, ANY, ANY, ANY), (1, 1, 5, 0, 0)),   # render_head_wf<true, 5>
    ((1, 0, 0, ANY, ANY, 4), (1, 0, 4, 0, 0)),     # render_head_wf<false, 4>
    ((1, 0, 0, ANY, ANY, 5), (1, 0, 5, 0, 0)),     # render_head_wf<false, 5>
    ((0, 0, 1, 1, ANY, ANY), (0, 0, 5, 1, 1)),     # render_unidir_accum_wf<true>
    ((0, 0, 1, 0, ANY, ANY), (0, 0, 5, 0, 1)),     # render_unidir_accum_wf<false>
    ((0, 1, 0, ANY, 4, ANY), (0, 1, 4, 0, 0)),     # render_unidir_wf<true, 4, false>
    ((0, 1, 0, 1, 5, ANY), (0, 1, 5, 1, 0)),       # render_unidir_wf<true, 5, true>
    ((0, 1, 0, 0, 5, ANY), (0, 1, 5, 0, 0)),       # render_unidir_wf<true, 5, false>
    ((0, 1, 0, 1, 6, ANY), (0, 1, 5, 1, 0)),       # (6 counts at 5)
    ((0, 1, 0, 0, 6, ANY), (0, 1, 5, 0, 0)),
    ((0, 0, 0, ANY, 6, ANY), (0, 0, 6, 0, 0)),     # render_unidir_wf<false, 6, false>
    ((0, 0, 0, 1, 5, ANY), (0, 0, 5, 1, 0)),       # render_unidir_wf<false, 5, true>
    ((0, 0, 0, 0, 5, ANY), (0, 0, 5, 0, 0)),       # render_unidir_wf<false, 5, false>
    ((0, 0, 0, ANY, 4, ANY), (0, 0, 4, 0, 0)),     # render_unidir_wf<false, 4, false>
]


def test_wavefront_variant_table(probe):
    got = probe(["variants"])
    # every legal input once: accum with count is left out
    assert sorted(tuple(g["in"]) for g in got) == sorted(
        (h, c, a, t, wf, hw) for h in (0, 1) for c, a in ((0, 0), (0, 1), (1, 0)) for t in (0, 1) for wf in (4, 5, 6)
        for hw in (4, 5))
    for g in got:
        rows = [want for key, want in VARIANT_TABLE if all(k is ANY or k == v for k, v in zip(key, g["in"]))]
        assert len(rows) == 1, g["in"]
        assert (g["head"], g["count"], g["min_waves"], g["lds_walk"], g["accum"]) == rows[0], g["in"]
