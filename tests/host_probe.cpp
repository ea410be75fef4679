// host_probe -- the render's host decisions called directly, without a GPU: pt::plan_units, pt::tile_grid,
// pt::validate_render and pt::pack_scene of libptamd.so.  Driven by tests/test_render_plan_host.py; prints one
// JSON object per line.
//
//   host_probe plan            stdin lines: npix spp num_cus head count lds_fixed budget [PT_X=value ...]
//                              (budget: bytes the budget callable answers, or "inf")
//   host_probe grid            stdin lines: w h tile_w tile_h shard_index shard_count
//   host_probe variants        pt::wavefront_variant over head, count, accum, lds_tree, PT_WF_MIN_WAVES 4..6,
//                              PT_HEAD_MIN_WAVES 4..5
//   host_probe pack NAME DIR  NAME: cornell | cornell_blob | quad | spheres; DIR: the models directory
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hip/pt_scene_pack.h"
#include "host/host_internal.h"
#include "host/render_plan.h"

using namespace ptd;

static int run_plan()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        pt::PlanInput in{};
        int head = 0, count = 0;
        std::string budget, kv;
        if (!(is >> in.npix >> in.spp >> in.num_cus >> head >> count >> in.lds_fixed >> budget)) continue;
        in.head = head != 0;
        in.count = count != 0;
        in.top_nodes = kTopNodesMax;
        in.top_node_bytes = kTopNodeBytes;
        std::vector<std::string> keys;
        while (is >> kv) {
            const size_t eq = kv.find('=');
            keys.push_back(kv.substr(0, eq));
            setenv(keys.back().c_str(), kv.substr(eq + 1).c_str(), 1);
        }
        const pt::RenderKnobs k = pt::read_render_knobs(kQueues, kTopNodesMax);
        int calls = 0;
        auto fn = [&](uint64_t* bytes) -> int {
            ++calls;
            *bytes = budget == "inf" ? ~0ull : strtoull(budget.c_str(), nullptr, 10);
            return PT_OK;
        };
        pt::UnitPlan u{};
        const int rc = pt::plan_units(in, k, fn, &u);
        for (const std::string& key : keys) unsetenv(key.c_str());
        printf("{\"rc\": %d, \"npix\": %u, \"nwhole\": %u, \"ntail\": %u, \"nmid\": %u, \"chunks_mid\": %u, \"chunks\": %u, "
               "\"nfin\": %u, \"chunks_fin\": %u, \"nunits\": %u, \"blocks\": %u, \"wpc\": %u, \"top_nodes\": %u, "
               "\"budget_calls\": %d}\n",
               rc, u.npix, u.nwhole, u.ntail, u.nmid, u.chunks_mid, u.chunks, u.nfin, u.chunks_fin, u.nunits, u.blocks, u.wpc,
               u.top_nodes, calls);
    }
    return 0;
}

static int run_grid()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        pt_params p;
        memset(&p, 0, sizeof(p));
        if (!(is >> p.width >> p.height >> p.tile_w >> p.tile_h >> p.shard_index >> p.shard_count)) continue;
        p.spp = 1;
        p.bounces = 1;
        pt_camera cam;
        memset(&cam, 0, sizeof(cam));
        cam.pxl_width = p.width;
        cam.pxl_height = p.height;
        const int vrc = pt::validate_render(&p, &cam);
        const pt::TileGrid g = pt::tile_grid(p);
        uint32_t n = 0;
        const int src = pt_shard_pixels(p.width, p.height, p.shard_index, p.shard_count, p.tile_w, p.tile_h, nullptr, 0, &n);
        printf("{\"validate_rc\": %d, \"shard_pixels_rc\": %d, \"in_image\": %u, \"tile_w\": %u, \"tile_h\": %u, \"tiles_x\": %u, "
               "\"ntiles\": %u, \"ntiles_shard\": %u, \"tile_bx\": %u, \"tile_blocks\": %u, \"npix\": %u, \"grid_slots\": %llu, "
               "\"fits\": %s}\n",
               vrc, src, n, g.tile_w, g.tile_h, g.tiles_x, g.ntiles, g.ntiles_shard, g.tile_bx, g.tile_blocks, g.npix,
               (unsigned long long)g.grid_slots, g.fits() ? "true" : "false");
    }
    return 0;
}

// pt::wavefront_variant for every legal combination of its inputs, one line each
static int run_variants()
{
    for (int head = 0; head < 2; ++head)
        for (int count = 0; count < 2; ++count)
            for (int accum = 0; accum < 2 - count; ++accum)   // (an accumulating pass never counts)
                for (int lds_tree = 0; lds_tree < 2; ++lds_tree)
                    for (int wf = 4; wf <= 6; ++wf)
                        for (int hw = 4; hw <= 5; ++hw) {
                            const pt::WavefrontVariant v = pt::wavefront_variant(head, count, accum, lds_tree, wf, hw);
                            printf("{\"in\": [%d, %d, %d, %d, %d, %d], \"head\": %d, \"count\": %d, \"min_waves\": %d, "
                                   "\"lds_walk\": %d, \"accum\": %d}\n",
                                   head, count, accum, lds_tree, wf, hw, v.head, v.count, v.min_waves, v.lds_walk, v.accum);
                        }
    return 0;
}

template <typename T>
static uint64_t hash_vec(const std::vector<T>& v, uint64_t h)
{
    const uint64_t n = v.size();
    h = pt::fnv1a(&n, sizeof(n), h);
    return pt::fnv1a(v.data(), v.size() * sizeof(T), h);
}

// every byte pack_scene produced: the vectors and the scalars, field by field
static uint64_t digest(const pt::PackedScene& P)
{
    uint64_t h = pt::kFnvBasis;
    h = hash_vec(P.nodes, h); h = hash_vec(P.rnodes, h); h = hash_vec(P.rparent, h); h = hash_vec(P.tris_leaf, h);
    h = hash_vec(P.tris_orig, h); h = hash_vec(P.shade, h); h = hash_vec(P.shade_m, h); h = hash_vec(P.mats, h);
    h = hash_vec(P.lights, h); h = hash_vec(P.spheres, h); h = hash_vec(P.nodes4, h); h = hash_vec(P.acc_tris, h);
    h = hash_vec(P.hrec, h); h = hash_vec(P.emis, h); h = hash_vec(P.jump, h); h = hash_vec(P.tone, h);
    const uint32_t words[] = {P.num_tris, (uint32_t)P.depth, P.scene_fast, P.node_mask, P.num_lights, P.num_spheres,
                              P.sphere_mat_base, P.top_nodes, P.n4, (uint32_t)P.acc4_depth, P.node4_mask, P.num_emis, P.tone_ok,
                              P.scene_spheres, P.knobs.wf_threshold, P.knobs.wf_root_first};
    h = pt::fnv1a(words, sizeof(words), h);
    h = pt::fnv1a(P.root, sizeof(P.root), h);
    h = pt::fnv1a(P.acc_root, sizeof(P.acc_root), h);
    h = pt::fnv1a(&P.scene_extent, 4, h);
    h = pt::fnv1a(&P.total_light_area, 4, h);
    return pt::fnv1a(&P.scene_digest, 8, h);
}

static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

template <typename F>
static void print_list(const char* name, size_t n, F at)
{
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < n; ++i) printf("%s%u", i ? ", " : "", (unsigned)at(i));
    printf("]");
}

static int run_pack(const std::string& name, const std::string& dir)
{
    pt_host_scene* hs = pt_scene_new();
    const pt_vec3 zero = {0.0f, 0.0f, 0.0f};
    int rc = PT_OK;
    auto load = [&](const char* obj, pt_vec3 origin, float scale) {
        if (rc == PT_OK) rc = pt_scene_load_obj(hs, (dir + "/" + obj).c_str(), (dir + "/").c_str(), origin, scale, 0);
    };
    if (name == "cornell" || name == "cornell_blob") load("cornell.obj", zero, 1.0f);
    if (name == "cornell_blob") load("blob.obj", pt_vec3{0.35f, 0.6f, 0.3f}, 0.75f);
    if (name == "quad") load("quad.obj", zero, 1.0f);
    if (name == "spheres") {
        pt_sphere s;
        memset(&s, 0, sizeof(s));
        s.pos = pt_vec3{0.0f, 2.0f, 0.0f}; s.rad = 0.5f;
        s.emission[0] = s.emission[1] = s.emission[2] = 4.0;
        rc = pt_scene_add_sphere(hs, &s);
        memset(&s, 0, sizeof(s));
        s.pos = pt_vec3{0.0f, 0.0f, 0.0f}; s.rad = 1.0f;
        s.diffuse[0] = s.diffuse[1] = s.diffuse[2] = 0.7;
        if (rc == PT_OK) rc = pt_scene_add_sphere(hs, &s);
    } else if (rc == PT_OK) {
        rc = pt_scene_build_bvh(hs);
    }
    pt_scene sc;
    if (rc == PT_OK) rc = pt_scene_view(hs, &sc);
    if (rc != PT_OK) {
        printf("{\"rc\": %d, \"error\": \"scene: %s\"}\n", rc, pt_last_error());
        return 1;
    }
    const pt::RenderKnobs k = pt::read_render_knobs(kQueues, kTopNodesMax);
    pt::PhaseTimer timer{false};
    pt::PackedScene P, Q;
    rc = pt::pack_scene(sc, k, &timer, &P);
    if (rc == PT_OK) rc = pt::pack_scene(sc, k, &timer, &Q);
    if (rc != PT_OK) {
        printf("{\"rc\": %d, \"error\": \"pack_scene: %s\"}\n", rc, pt_last_error());
        return 1;
    }
    printf("{\"rc\": 0, \"nt\": %u, \"nn\": %u, \"num_lights\": %u, \"n4\": %u, \"top_nodes\": %u, \"node4_mask\": %u, "
           "\"leaf_bits\": %u, \"top_nodes_max\": %u, \"digest_first\": \"%016llx\", \"digest_second\": \"%016llx\", "
           "\"sizes\": {\"nodes\": %zu, \"rnodes\": %zu, \"tris_leaf\": %zu, \"tris_orig\": %zu, \"nodes4\": %zu, \"acc_tris\": %zu, "
           "\"hrec\": %zu, \"lights\": %zu, \"spheres\": %zu, \"mats\": %zu}, \"last_light_prim\": %d",
           sc.num_tris, sc.bvh_size, sc.num_lights, P.n4, P.top_nodes, P.node4_mask, kLeafBits, kTopNodesMax,
           (unsigned long long)digest(P), (unsigned long long)digest(Q), P.nodes.size(), P.rnodes.size(), P.tris_leaf.size(),
           P.tris_orig.size(), P.nodes4.size(), P.acc_tris.size(), P.hrec.size(), P.lights.size(), P.spheres.size(), P.mats.size(),
           P.lights[sc.num_lights].tri);
    print_list("tris_leaf_id", P.tris_leaf.size(), [&](size_t i) { return bits_of(P.tris_leaf[i].c.y); });
    print_list("acc_id", P.acc_tris.size(), [&](size_t i) { return bits_of(P.acc_tris[i].c.y); });
    print_list("acc_parent", P.acc_tris.size(), [&](size_t i) { return bits_of(P.acc_tris[i].c.w); });
    print_list("hrec_id", P.acc_tris.size(), [&](size_t i) { return bits_of(P.hrec[3 * i + 1].w); });
    print_list("hrec_parent", P.acc_tris.size(), [&](size_t i) { return bits_of(P.hrec[3 * i + 1].z); });
    print_list("child", P.nodes4.size() * 4, [&](size_t i) {
        const uint4 c = P.nodes4[i / 4].child;
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
        return w[i % 4];
    });
    printf("}\n");
    pt_scene_free(hs);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan") return run_plan();
    if (mode == "grid") return run_grid();
    if (mode == "variants") return run_variants();
    if (mode == "pack" && argc > 3) return run_pack(argv[2], argv[3]);
    fprintf(stderr, "usage: host_probe plan | grid | variants | pack NAME MODELS_DIR\n");
    return 2;
}
