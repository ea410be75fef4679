// pt_scene_pack.cpp -- pt::pack_scene: a validated pt_scene turned into the kernels' records.  Host arithmetic
// only, but part of the bit contract (the edge subtractions of tri_rec, light_rec's area): built with the
// library's compiler and -ffp-contract=off.
#include "pt_scene_pack.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>

using namespace ptd;

namespace pt {

void PhaseTimer::lap(const char* what)
{
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "pt_create: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
    t0 = now;
}

// GF(2) jump tables J_k = A^(2^(67+k)), k = 0..31, rocRAND's bit-image layout.
static void build_jump_tables(std::vector<uint32_t>& out)
{
    auto apply = [](const uint32_t* img, uint32_t v[5]) {
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (int b = 0; b < 160; ++b)
            if ((v[b >> 5] >> (b & 31)) & 1u)
                for (int w = 0; w < 5; ++w) r[w] ^= img[b * 5 + w];
        memcpy(v, r, sizeof(r));
    };
    std::vector<uint32_t> m(800), tmp(800);
    for (int b = 0; b < 160; ++b) {   // one XORWOW step on the 160-bit xorshift state
        uint32_t v[5] = {0, 0, 0, 0, 0};
        v[b >> 5] = 1u << (b & 31);
        const uint32_t t = v[0] ^ (v[0] >> 2);
        uint32_t nv[5] = {v[1], v[2], v[3], v[4], (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))};
        memcpy(&m[b * 5], nv, sizeof(nv));
    }
    auto square = [&]() {
        for (int b = 0; b < 160; ++b) {
            uint32_t v[5];
            memcpy(v, &m[b * 5], sizeof(v));
            apply(m.data(), v);
            memcpy(&tmp[b * 5], v, sizeof(v));
        }
        m.swap(tmp);
    };
    for (int i = 0; i < 67; ++i) square();
    out.resize(32 * 800);
    for (int k = 0; k < 32; ++k) {
        memcpy(&out[k * 800], m.data(), 800 * sizeof(uint32_t));
        square();
    }
}

// Byte-sliced form of the jump tables for rng_init: entry (k, j, x) = J_k * (x << 8j).
static void build_jump_bytes(const std::vector<uint32_t>& img, std::vector<uint32_t>& out)
{
    out.assign((size_t)32 * 20 * 256 * kJumpEntryWords, 0u);
    for (int k = 0; k < 32; ++k)
        for (int j = 0; j < 20; ++j)
            for (int x = 0; x < 256; ++x) {
                uint32_t* e = &out[(((size_t)k * 20 + j) * 256 + x) * kJumpEntryWords];
                for (int i = 0; i < 8; ++i)
                    if ((x >> i) & 1)
                        for (int w = 0; w < 5; ++w) e[w] ^= img[(size_t)k * 800 + (8 * j + i) * 5 + w];
            }
}

// The scene's indices: every triangle, light and sphere refers to something that exists.
static int check_indices(const pt_scene& sc)
{
    const uint32_t nt = sc.num_tris;
    for (uint32_t i = 0; i < nt; ++i) {
        const pt_triangle& t = sc.tris[i];
        if ((uint32_t)t.v0 >= sc.num_verts || (uint32_t)t.v1 >= sc.num_verts || (uint32_t)t.v2 >= sc.num_verts ||
            (uint32_t)t.mat >= sc.num_mats)
            return fail(PT_E_SCENE, "pt_create: triangle %u has an out-of-range vertex or material index", i);
    }
    for (uint32_t j = 0; j < sc.num_lights; ++j) {
        const uint32_t e = sc.lights[j];
        if ((e & PT_LIGHT_SPHERE) ? (e ^ PT_LIGHT_SPHERE) >= sc.num_spheres : e >= nt)
            return fail(PT_E_SCENE, "pt_create: light %u has an out-of-range primitive (0x%x)", j, e);
    }
    for (uint32_t k = 0; k < sc.num_spheres; ++k)
        if (!(sc.spheres[k].rad > 0.0f) || !std::isfinite(sc.spheres[k].rad))
            return fail(PT_E_SCENE, "pt_create: sphere %u has radius %g", k, (double)sc.spheres[k].rad);
    return PT_OK;
}

// The reference BVH is a tree over the triangles: every reference in range, every triangle reached once.
// leaf_order = the triangles in left-first DFS order (the order trace() meets leaves), leaf_rank its inverse.
// The same walk checks what the device walks rely on (pt.h, pt_scene): finite boxes, every child box within its
// parent's, every triangle's vertices within its parent node's box, and the tree's true depth (a leaf counts 1, a
// node 1 + its deeper child) below PT_MAX_BVH_DEPTH and not above sc.bvh_depth.  check_indices comes first.
static int check_bvh(const pt_scene& sc, std::vector<uint32_t>* leaf_rank, std::vector<uint32_t>* leaf_order)
{
    const uint32_t nt = sc.num_tris, nn = sc.bvh_size;
    leaf_rank->assign(nt, 0xffffffffu);
    leaf_order->clear();
    leaf_order->reserve(nt);
    if (nt == 0) return PT_OK;
    struct Entry { uint32_t ref, parent; int32_t level; };   // level: 1 for the root; parent of the root: itself
    std::vector<Entry> st;
    st.push_back({0u, 0u, 1});
    size_t visits = 0;
    int32_t depth = 0;
    while (!st.empty()) {
        const Entry e = st.back();
        st.pop_back();
        if (++visits > 4ull * nt + 8) return fail(PT_E_SCENE, "pt_create: BVH is not a tree");
        if (e.level > depth) depth = e.level;
        if (e.ref & PT_BVH_LEAF_FLAG) {
            const uint32_t k = e.ref ^ PT_BVH_LEAF_FLAG;
            if (k >= nt || (*leaf_rank)[k] != 0xffffffffu) return fail(PT_E_SCENE, "pt_create: bad BVH leaf %u", k);
            (*leaf_rank)[k] = (uint32_t)leaf_order->size();
            leaf_order->push_back(k);
            const pt_bvh_node& p = sc.bvh[e.parent];
            const pt_triangle& t = sc.tris[k];
            for (int32_t vi : {t.v0, t.v1, t.v2}) {
                const pt_vec3& v = sc.verts[vi];
                if (!(v.x >= p.lo.x && v.x <= p.hi.x && v.y >= p.lo.y && v.y <= p.hi.y && v.z >= p.lo.z && v.z <= p.hi.z))
                    return fail(PT_E_SCENE, "pt_create: triangle %u has vertex %d (%.9g %.9g %.9g) outside the box of its BVH node %u",
                                k, vi, (double)v.x, (double)v.y, (double)v.z, e.parent);
            }
        } else {
            if (e.ref >= nn) return fail(PT_E_SCENE, "pt_create: BVH child %u out of range", e.ref);
            const pt_bvh_node& x = sc.bvh[e.ref];
            const float b[6] = {x.lo.x, x.lo.y, x.lo.z, x.hi.x, x.hi.y, x.hi.z};
            for (int q = 0; q < 6; ++q)
                if (!std::isfinite(b[q])) return fail(PT_E_SCENE, "pt_create: BVH node %u has a box coordinate that is not finite", e.ref);
            if (e.level > 1) {
                const pt_bvh_node& p = sc.bvh[e.parent];
                if (!(x.lo.x >= p.lo.x && x.lo.y >= p.lo.y && x.lo.z >= p.lo.z && x.hi.x <= p.hi.x && x.hi.y <= p.hi.y && x.hi.z <= p.hi.z))
                    return fail(PT_E_SCENE, "pt_create: the box of BVH node %u is not within the box of its parent, node %u", e.ref, e.parent);
            }
            st.push_back({x.right, e.ref, e.level + 1});
            st.push_back({x.left, e.ref, e.level + 1});
        }
    }
    if (leaf_order->size() != nt) return fail(PT_E_SCENE, "pt_create: BVH reaches %zu of %u triangles", leaf_order->size(), nt);
    if (depth >= PT_MAX_BVH_DEPTH)
        return fail(PT_E_BVH_DEPTH, "pt_create: the BVH is %d levels deep (bvh_depth says %d), the limit is %d", depth, sc.bvh_depth,
                    PT_MAX_BVH_DEPTH - 1);
    if (sc.bvh_depth < depth)
        return fail(PT_E_SCENE, "pt_create: bvh_depth is %d but the BVH is %d levels deep (the stacks are sized by it)", sc.bvh_depth, depth);
    return PT_OK;
}

int check_scene(const pt_scene& sc, SceneCheck* out)
{
    if (int rc = check_indices(sc)) return rc;
    return check_bvh(sc, &out->leaf_rank, &out->leaf_order);
}

// what the scene is, for pt_accum_save / pt_accum_load: every array the caller passed
static uint64_t scene_digest(const pt_scene& sc)
{
    uint64_t h = kFnvBasis;
    h = fnv1a(sc.verts, (size_t)sc.num_verts * sizeof(pt_vec3), h);
    h = fnv1a(sc.tris, (size_t)sc.num_tris * sizeof(pt_triangle), h);
    h = fnv1a(sc.mats, (size_t)sc.num_mats * sizeof(pt_material), h);
    h = fnv1a(sc.lights, (size_t)sc.num_lights * sizeof(uint32_t), h);
    h = fnv1a(&sc.total_light_area, sizeof(float), h);
    h = fnv1a(sc.bvh, (size_t)sc.bvh_size * sizeof(pt_bvh_node), h);
    h = fnv1a(sc.spheres, (size_t)sc.num_spheres * sizeof(pt_sphere), h);
    return h;
}

// a record permuted for tri_hit_pk: {v0.xy, e1.xy}, {e2.xy, v0.z, e1.z}
static DTri tri_pk(const DTri& r)
{
    DTri q;
    q.a = make_float4(r.a.x, r.a.y, r.a.w, r.b.x);
    q.b = make_float4(r.b.z, r.b.w, r.a.z, r.b.y);
    q.c = r.c;
    return q;
}

static uint32_t index_mask(uint32_t n)   // the low bits that hold an index < n
{
    uint32_t bits = 1;
    while ((1u << bits) < n) ++bits;
    return (bits >= 31) ? 0x7fffffffu : ((1u << bits) - 1u);
}

// The render-path BVH4 (accel_build.cpp: binned SAH binary BVH collapsed to 4 wide) as device records: node
// order, triangle slots, leaf masks.  tri_rec(k) = the intersection record of triangle k.
template <typename TriRec>
static int pack_bvh4(const pt_scene& sc, const RenderKnobs& knobs, PhaseTimer* timer, const TriRec& tri_rec, PackedScene* P)
{
    const uint32_t nt = sc.num_tris;
    AccelBvh acc;
    constexpr int kW = 4;
    Accel4 acc4;
    timer->lap("reference-BVH records");
    int rc4 = build_accel(sc, &acc);
    timer->lap("SAH BVH build");
    if (timer->on && rc4 == PT_OK) fprintf(stderr, "pt_create: render BVH SAH cost %.6g\n", accel_sah_cost(acc));
    if (rc4 == PT_OK) rc4 = collapse_accel4(acc, &acc4);
    timer->lap("BVH4 collapse");
    // the structural check (every node and slot reached once, <= 8 leaf triangles per node, nested
    // boxes) is O(nodes): the walk's exactness argument and its 8-bit leaf masks rely on it
    if (rc4 == PT_OK) rc4 = validate_accel4(acc, acc4);
    timer->lap("BVH4 validate");
    if (rc4 != PT_OK) return rc4;
    // Node order: the kTopNodesMax nodes most likely to be visited first (best-first by box
    // surface area from the root: a connected top subtree, staged in LDS by the wavefront
    // kernel), then the others in their DFS order.
    const uint32_t n4 = (uint32_t)acc4.nodes.size();
    std::vector<uint32_t> new_of(n4, ~0u), old_of;
    old_of.reserve(n4);
    {
        std::vector<std::pair<float, uint32_t>> heap{{INFINITY, 0u}};
        while (!heap.empty() && old_of.size() < kTopNodesMax) {
            std::pop_heap(heap.begin(), heap.end());
            const uint32_t o = heap.back().second;
            heap.pop_back();
            new_of[o] = (uint32_t)old_of.size();
            old_of.push_back(o);
            const auto& x = acc4.nodes[o];
            for (int k = 0; k < kW; ++k) {
                if (x.child[k] == kAccel4Empty || (x.child[k] & PT_BVH_LEAF_FLAG)) continue;
                const float b[6] = {x.lo[0][k], x.lo[1][k], x.lo[2][k], x.hi[0][k], x.hi[1][k], x.hi[2][k]};
                const float ex = b[3] - b[0], ey = b[4] - b[1], ez = b[5] - b[2];
                heap.push_back({ex * ey + ey * ez + ez * ex, x.child[k]});
                std::push_heap(heap.begin(), heap.end());
            }
        }
        for (uint32_t o = 0; o < n4; ++o)
            if (new_of[o] == ~0u) { new_of[o] = (uint32_t)old_of.size(); old_of.push_back(o); }
    }
    P->top_nodes = std::min(std::max(knobs.wf_top, 1u), n4);   // (>= 1: the wavefront walk reads the LDS top unconditionally)
    P->n4 = n4;
    // A tree the LDS top holds whole (small scenes: C2's Cornell box) is walked with no node fetch
    // from memory, so a walk step is cheap: waves stay in the walk phase until 62 lanes wait to
    // shade, and a new ray's first two visits (not four) run in the shading pass (C2: 6879 -> 7081
    // Msamples/s, same box, profiles/r03_c2_knobs; the stand-in's defaults are unchanged).
    if (n4 <= P->top_nodes) {
        if (!knobs.wf_threshold_set) P->knobs.wf_threshold = 62;
        if (!knobs.wf_root_first_set) P->knobs.wf_root_first = 2;
    }
    std::vector<DNode4>& an = P->nodes4;
    an.resize(n4);
    // Triangle slots: the triangles of each node's leaf children (in node order) get consecutive
    // slots, and each node lists its leaf children first -- the walk queues a node's entered
    // leaves as one entry (first slot, 8-bit mask of slots).  A leaf child's word is
    // kLeaf | the node's first leaf slot << kLeafBits | its slot bits relative to it.
    // slot_leaf[s] = the binary BVH's leaf slot (one triangle) of render slot s.
    std::vector<uint32_t> slot_leaf;
    slot_leaf.reserve(nt);
    for (size_t i = 0; i < n4; ++i) {
        auto x0 = acc4.nodes[old_of[i]], x = x0;
        auto is_leaf = [](uint32_t r) { return r != kAccel4Empty && (r & PT_BVH_LEAF_FLAG); };
        int order[kW], m = 0;
        for (int k = 0; k < kW; ++k) if (is_leaf(x0.child[k])) order[m++] = k;
        for (int k = 0; k < kW; ++k) if (!is_leaf(x0.child[k])) order[m++] = k;
        const uint32_t base = (uint32_t)slot_leaf.size();
        for (int k = 0; k < kW; ++k) {
            const int q = order[k];
            for (int ax = 0; ax < 3; ++ax) { x.lo[ax][k] = x0.lo[ax][q]; x.hi[ax][k] = x0.hi[ax][q]; }
            x.child[k] = x0.child[q];
            if (is_leaf(x.child[k])) {
                const uint32_t first = (uint32_t)slot_leaf.size() - base, cnt = accel_leaf_count(x.child[k]);
                for (uint32_t j = 0; j < cnt; ++j) slot_leaf.push_back(accel_leaf_slot(x.child[k]) + j);
                static_assert(kAccel4LeafTris <= kLeafBits, "leaf slot mask width");
                if (first + cnt > kLeafBits || base >= (1u << (31 - kLeafBits)))
                    return fail(PT_E_SCENE, "pt_create: %u triangles exceed the render path's leaf slot range", nt);
                x.child[k] = PT_BVH_LEAF_FLAG | (base << kLeafBits) | (((1u << cnt) - 1u) << first);
            }
        }
        for (int k = 0; k < kW; ++k)
            if (x.child[k] != kAccel4Empty && !(x.child[k] & PT_BVH_LEAF_FLAG)) x.child[k] = new_of[x.child[k]];
        an[i].lox = make_float4(x.lo[0][0], x.lo[0][1], x.lo[0][2], x.lo[0][3]);
        an[i].loy = make_float4(x.lo[1][0], x.lo[1][1], x.lo[1][2], x.lo[1][3]);
        an[i].loz = make_float4(x.lo[2][0], x.lo[2][1], x.lo[2][2], x.lo[2][3]);
        an[i].hix = make_float4(x.hi[0][0], x.hi[0][1], x.hi[0][2], x.hi[0][3]);
        an[i].hiy = make_float4(x.hi[1][0], x.hi[1][1], x.hi[1][2], x.hi[1][3]);
        an[i].hiz = make_float4(x.hi[2][0], x.hi[2][1], x.hi[2][2], x.hi[2][3]);
        an[i].child = make_uint4(x.child[0], x.child[1], x.child[2], x.child[3]);
        an[i].pad = make_uint4(0u, 0u, 0u, 0u);
    }
    if (slot_leaf.size() != nt) return fail(PT_E_SCENE, "pt_create: BVH4 reaches %zu of %u triangles", slot_leaf.size(), nt);
    P->acc_tris.resize(nt);
    for (uint32_t i = 0; i < nt; ++i) P->acc_tris[i] = tri_pk(tri_rec(acc.leaf_order[slot_leaf[i]]));
    memcpy(P->acc_root, acc.root_box, sizeof(P->acc_root));
    P->acc4_depth = acc4.depth;
    P->node4_mask = index_mask(n4);
    return PT_OK;
}

int pack_scene(const pt_scene& scene, const RenderKnobs& knobs, PhaseTimer* timer, PackedScene* P, const SceneCheck* checked)
{
    const pt_scene* sc = &scene;
    *P = PackedScene();
    const uint32_t nt = sc->num_tris, nn = sc->bvh_size;
    SceneCheck own;
    if (!checked) {
        if (int rc = check_scene(scene, &own)) return rc;
        checked = &own;
        timer->lap("scene validation");
    }
    const std::vector<uint32_t>&leaf_rank = checked->leaf_rank, &leaf_order = checked->leaf_order;

    P->num_tris = nt;
    P->scene_digest = scene_digest(scene);
    P->scene_spheres = sc->num_spheres;
    P->depth = sc->bvh_depth;
    P->knobs = knobs;

    std::vector<uint32_t> ref_parent(nt, 0u);
    for (uint32_t i = 0; i < nn; ++i) {
        if (sc->bvh[i].left & PT_BVH_LEAF_FLAG) ref_parent[sc->bvh[i].left ^ PT_BVH_LEAF_FLAG] = i;
        if (sc->bvh[i].right & PT_BVH_LEAF_FLAG) ref_parent[sc->bvh[i].right ^ PT_BVH_LEAF_FLAG] = i;
    }
    auto tri_rec = [&](uint32_t k) {
        const pt_triangle& t = sc->tris[k];
        const pt_vec3 a = sc->verts[t.v0], b = sc->verts[t.v1], cc = sc->verts[t.v2];
        DTri r;
        const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;   // modelLoader.h:58
        const float e2x = cc.x - a.x, e2y = cc.y - a.y, e2z = cc.z - a.z; // modelLoader.h:59
        r.a = make_float4(a.x, a.y, a.z, e1x);
        r.b = make_float4(e1y, e1z, e2x, e2y);
        const uint32_t words[3] = {k, leaf_rank[k], ref_parent[k]};
        float f[3];
        memcpy(f, words, sizeof(f));
        r.c = make_float4(e2z, f[0], f[1], f[2]);
        return r;
    };
    std::vector<DTri>&tl = P->tris_leaf, &to = P->tris_orig;
    tl.resize(nt);
    to.resize(nt);
    for (uint32_t i = 0; i < nt; ++i) { to[i] = tri_rec(i); tl[i] = tri_rec(leaf_order[i]); }
    std::vector<RNode>& rn = P->rnodes;
    std::vector<DNode>& dn = P->nodes;
    rn.resize(nn);
    dn.resize(nn);
    auto box_of = [&](uint32_t ref, float* b) {   // box of a child; leaves carry no box
        if (ref & PT_BVH_LEAF_FLAG) { for (int q = 0; q < 6; ++q) b[q] = 0.0f; return; }
        const pt_bvh_node& x = sc->bvh[ref];
        b[0] = x.lo.x; b[1] = x.lo.y; b[2] = x.lo.z; b[3] = x.hi.x; b[4] = x.hi.y; b[5] = x.hi.z;
    };
    auto remap = [&](uint32_t ref) {
        return (ref & PT_BVH_LEAF_FLAG) ? (PT_BVH_LEAF_FLAG | leaf_rank[ref ^ PT_BVH_LEAF_FLAG]) : ref;
    };
    float lo_all[3] = {1e30f, 1e30f, 1e30f}, hi_all[3] = {-1e30f, -1e30f, -1e30f};
    for (uint32_t i = 0; i < nn; ++i) {
        const pt_bvh_node& x = sc->bvh[i];
        memcpy(rn[i].lo, &x.lo, 12);
        memcpy(rn[i].hi, &x.hi, 12);
        rn[i].left = x.left;
        rn[i].right = x.right;
        float b0[6], b1[6];
        box_of(x.left, b0);
        box_of(x.right, b1);
        dn[i].a = make_float4(b0[0], b0[1], b0[2], b0[3]);
        dn[i].b = make_float4(b0[4], b0[5], b1[0], b1[1]);
        dn[i].c = make_float4(b1[2], b1[3], b1[4], b1[5]);
        dn[i].d = make_uint4(remap(x.left), remap(x.right), 0u, 0u);
    }
    for (int q = 0; q < 6; ++q) P->root[q] = 0.0f;
    if (nt > 0) {
        const pt_bvh_node& r = sc->bvh[0];
        P->root[0] = r.lo.x; P->root[1] = r.lo.y; P->root[2] = r.lo.z;
        P->root[3] = r.hi.x; P->root[4] = r.hi.y; P->root[5] = r.hi.z;
    }
    // The scene extent is that of the geometry: the vertices the triangles use (build_accel's `ext`, which sizes the
    // BVH4 boxes' margin) and the spheres.  Not the root box: a caller's may be looser, and origin_max, near_camera()
    // and cull_abs scale with the extent (64 extents is as far as that margin covers the BVH4 walk's box test).
    for (uint32_t i = 0; i < nt; ++i)
        for (int32_t vi : {sc->tris[i].v0, sc->tris[i].v1, sc->tris[i].v2}) {
            const float cc[3] = {sc->verts[vi].x, sc->verts[vi].y, sc->verts[vi].z};
            for (int q = 0; q < 3; ++q) {
                lo_all[q] = std::fmin(lo_all[q], cc[q]);
                hi_all[q] = std::fmax(hi_all[q], cc[q]);
            }
        }
    for (uint32_t k = 0; k < sc->num_spheres; ++k) {   // the scene extent covers the spheres too
        const pt_sphere& sp = sc->spheres[k];
        const float cc[3] = {sp.pos.x, sp.pos.y, sp.pos.z};
        for (int q = 0; q < 3; ++q) {
            lo_all[q] = std::fmin(lo_all[q], cc[q] - sp.rad);
            hi_all[q] = std::fmax(hi_all[q], cc[q] + sp.rad);
        }
    }
    {
        float ext = 0.0f;
        for (int q = 0; q < 3; ++q) {
            const float e = std::fabs(hi_all[q]) > std::fabs(lo_all[q]) ? std::fabs(hi_all[q]) : std::fabs(lo_all[q]);
            ext = ext > e ? ext : e;
        }
        P->scene_extent = (ext > 0.0f && std::isfinite(ext)) ? ext : 1.0f;
    }
    {
        // Markstein-quotient precondition on the scene (pt_device.h div_mk): every vertex and box
        // coordinate is 0 or has magnitude in [2^-50, 2^20].  (A caller's boxes need not be min/max of vertices.)
        bool ok = true;
        auto in_range = [&](float c) {
            const float m = std::fabs(c);
            if (!(m == 0.0f || (m >= 0x1p-50f && m <= 0x1p20f))) ok = false;
        };
        for (uint32_t v = 0; v < sc->num_verts && ok; ++v)
            for (float c : {sc->verts[v].x, sc->verts[v].y, sc->verts[v].z}) in_range(c);
        for (uint32_t i = 0; i < nn && ok; ++i)
            for (float c : {sc->bvh[i].lo.x, sc->bvh[i].lo.y, sc->bvh[i].lo.z, sc->bvh[i].hi.x, sc->bvh[i].hi.y, sc->bvh[i].hi.z}) in_range(c);
        P->scene_fast = ok;
        P->node_mask = index_mask(nn);
    }
    if (nt == 0) {   // spheres only: no triangle structures (kernels skip the walk)
        for (int q = 0; q < 3; ++q) { P->acc_root[q] = INFINITY; P->acc_root[3 + q] = -INFINITY; }
        P->acc4_depth = 0;
        P->node4_mask = 1u;
    } else if (int rc = pack_bvh4(scene, knobs, timer, tri_rec, P)) {
        return rc;
    }
    const std::vector<DTri>& at = P->acc_tris;
    P->rparent.assign(nn, 0u);
    for (uint32_t i = 0; i < nn; ++i) {
        if (!(sc->bvh[i].left & PT_BVH_LEAF_FLAG)) P->rparent[sc->bvh[i].left] = i;
        if (!(sc->bvh[i].right & PT_BVH_LEAF_FLAG)) P->rparent[sc->bvh[i].right] = i;
    }
    // per render-path slot: the winner check's box (the reference parent's node of its triangle), parent and
    // triangle id, and the shading normal and material (Args::hrec)
    std::vector<float4>& hr = P->hrec;
    hr.assign((size_t)3 * std::max<size_t>(at.size(), 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t sl = 0; sl < at.size(); ++sl) {
        uint32_t parent, tid;
        memcpy(&parent, &at[sl].c.w, 4);
        memcpy(&tid, &at[sl].c.y, 4);
        const RNode& b = rn[parent];
        float fpar, ftid, fmat;
        memcpy(&fpar, &parent, 4);
        memcpy(&ftid, &tid, 4);
        memcpy(&fmat, &sc->tris[tid].mat, 4);
        hr[3 * sl] = make_float4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
        hr[3 * sl + 1] = make_float4(b.hi[1], b.hi[2], fpar, ftid);
        hr[3 * sl + 2] = make_float4(sc->tris[tid].norm.x, sc->tris[tid].norm.y, sc->tris[tid].norm.z, fmat);
    }
    // last-bounce light probe (shade_lane begin_trace): every triangle whose material has
    // emission.r != 0 (the integrator's emission test, kernel.cu:453 -- not the caller's light list)
    std::vector<DTri>& em = P->emis;
    for (uint32_t i = 0; i < nt; ++i)
        if (sc->mats[sc->tris[i].mat].emission[0] != 0) em.push_back(tri_pk(tri_rec(i)));
    if (em.size() > kMaxProbeEmitters || sc->num_spheres > 0 || knobs.no_light_probe) em.clear();
    P->num_emis = (uint32_t)em.size();
    std::vector<DShade>& sh = P->shade;
    sh.resize(nt);
    for (uint32_t i = 0; i < nt; ++i) {
        sh[i].nx = sc->tris[i].norm.x; sh[i].ny = sc->tris[i].norm.y; sh[i].nz = sc->tris[i].norm.z;
        sh[i].mat = sc->tris[i].mat;
    }
    // the merged per-triangle shading record (Args::shade_m) when every material colour is a float
    std::vector<float4>& shm = P->shade_m;
    {
        bool exact = nt > 0 && !knobs.no_shade_m;
        for (uint32_t i = 0; i < sc->num_mats && exact; ++i)
            for (int q = 0; q < 3; ++q)
                exact = exact && (double)(float)sc->mats[i].albedo[q] == sc->mats[i].albedo[q] &&
                        (double)(float)sc->mats[i].emission[q] == sc->mats[i].emission[q];
        if (exact) {
            shm.resize((size_t)3 * nt);
            for (uint32_t i = 0; i < nt; ++i) {
                const pt_material& m = sc->mats[sc->tris[i].mat];
                shm[3 * (size_t)i] = make_float4(sc->tris[i].norm.x, sc->tris[i].norm.y, sc->tris[i].norm.z, (float)m.emission[0]);
                shm[3 * (size_t)i + 1] = make_float4((float)m.albedo[0], (float)m.albedo[1], (float)m.albedo[2], (float)m.emission[1]);
                float mbits;
                memcpy(&mbits, &sc->tris[i].mat, 4);
                shm[3 * (size_t)i + 2] = make_float4((float)m.emission[2], mbits, 0.0f, 0.0f);
            }
        }
    }
    // scene materials, then one per sphere (sphere.h diffuse / emm)
    std::vector<DMat>& mt = P->mats;
    mt.resize(sc->num_mats + sc->num_spheres);
    for (uint32_t i = 0; i < sc->num_mats; ++i) {
        for (int q = 0; q < 3; ++q) { mt[i].albedo[q] = sc->mats[i].albedo[q]; mt[i].emission[q] = sc->mats[i].emission[q]; }
    }
    for (uint32_t k = 0; k < sc->num_spheres; ++k) {
        DMat& m = mt[sc->num_mats + k];
        for (int q = 0; q < 3; ++q) { m.albedo[q] = sc->spheres[k].diffuse[q]; m.emission[q] = sc->spheres[k].emission[q]; }
    }
    P->spheres.resize(sc->num_spheres);
    for (uint32_t k = 0; k < sc->num_spheres; ++k)
        P->spheres[k] = make_float4(sc->spheres[k].pos.x, sc->spheres[k].pos.y, sc->spheres[k].pos.z, sc->spheres[k].rad);
    P->num_spheres = sc->num_spheres;
    P->sphere_mat_base = sc->num_mats;
    std::vector<DLight>& lt = P->lights;
    lt.resize(sc->num_lights + 1);
    auto light_rec = [&](uint32_t tri) {
        const pt_triangle& t = sc->tris[tri];
        const pt_vec3 a = sc->verts[t.v0], b = sc->verts[t.v1], cc = sc->verts[t.v2];
        DLight L;
        const float a1x = b.x - a.x, a1y = b.y - a.y, a1z = b.z - a.z;
        const float a2x = cc.x - a.x, a2y = cc.y - a.y, a2z = cc.z - a.z;
        // length(cross(a1, a2)) / 2, kernel.cu:477-478
        const float cx = a1y * a2z - a1z * a2y, cy = a1z * a2x - a1x * a2z, cz = a1x * a2y - a1y * a2x;
        L.area = sqrtf(cx * cx + cy * cy + cz * cz) / 2;
        L.tri = (int32_t)tri;
        L.v0[0] = a.x; L.v0[1] = a.y; L.v0[2] = a.z;
        L.a1[0] = a1x; L.a1[1] = a1y; L.a1[2] = a1z;
        L.a2[0] = a2x; L.a2[1] = a2y; L.a2[2] = a2z;
        L.pad = 0.0f;
        return L;
    };
    // sphere light (d8 policy): area 4*3.14159*r^2, center in v0, radius in a1[0], pad = 1
    auto sphere_light = [&](uint32_t k) {
        DLight L;
        memset(&L, 0, sizeof(L));
        const pt_sphere& q = sc->spheres[k];
        L.area = sphere_area(q.rad);
        L.tri = (int32_t)(nt + k);
        L.v0[0] = q.pos.x; L.v0[1] = q.pos.y; L.v0[2] = q.pos.z;
        L.a1[0] = q.rad;
        L.pad = 1.0f;
        return L;
    };
    for (uint32_t j = 0; j < sc->num_lights; ++j) {
        const uint32_t e = sc->lights[j];
        lt[j] = (e & PT_LIGHT_SPHERE) ? sphere_light(e ^ PT_LIGHT_SPHERE) : light_rec(e);
    }
    lt[sc->num_lights] = (nt > 0) ? light_rec(0) : sphere_light(0);   // "nothing picked": primitive 0
    P->num_lights = sc->num_lights;
    P->total_light_area = sc->total_light_area;
    std::vector<uint32_t> jump_img;
    build_jump_tables(jump_img);
    build_jump_bytes(jump_img, P->jump);
    P->tone.resize(256);
    P->tone_ok = tonemap_thresholds(P->tone.data());

    // the BVH4 walk addresses nodes and triangle records by 32-bit byte offsets (pt_device.h
    // walk4_step): larger structures take the exact reference-BVH walk for every ray
    if ((uint64_t)P->nodes4.size() * sizeof(DNode4) >= (1ull << 32) || (uint64_t)at.size() * sizeof(DTri) >= (1ull << 32))
        P->scene_fast = false;
    timer->lap("records + jump/tone tables");
    return PT_OK;
}

}  // namespace pt
