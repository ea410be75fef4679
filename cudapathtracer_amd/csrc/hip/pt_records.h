// pt_records.h -- the records the kernels read from HBM and the layout constants the host packs them by.
// Plain structs over HIP's vector types: pt_device.h (the kernels) and pt_scene_pack.cpp (the host code that
// fills them) include it; nothing here needs a device compiler.
#pragma once

#include <hip/hip_vector_types.h>
#include <stdint.h>

namespace ptd {

// ------------------------------------------------------------------ HBM layout
// Both children of one reference BVH node in one 64-B record (4 x 16-B loads).  Child ref:
// inner -> node index (same index as the reference's BFS array), leaf -> kLeaf | slot, where
// slot is the triangle's position in left-first DFS leaf order (its tie-break rank).
struct alignas(16) DNode {
    float4 a;   // c0.lo.xyz, c0.hi.x
    float4 b;   // c0.hi.yz, c1.lo.xy
    float4 c;   // c1.lo.z, c1.hi.xyz
    uint4 d;    // c0 ref, c1 ref, -, -
};
static_assert(sizeof(DNode) == 64, "node record is 64 B");

// The reference's own node (BVH.h:111-115), used by the reference-order walk.
struct alignas(16) RNode {
    float lo[3], hi[3];
    uint32_t left, right;
};
static_assert(sizeof(RNode) == 32, "reference node is 32 B");

// Intersection record: v0, e1 = v1-v0, e2 = v2-v0 (the exact subtractions triIntersect does,
// modelLoader.h:58-59, so precomputing them is bit-exact), original triangle id.
struct alignas(16) DTri {
    float4 a;   // v0.xyz, e1.x
    float4 b;   // e1.yz, e2.xy
    float4 c;   // e2.z, id, rank, parent (bits): rank = position in the reference's left-first DFS
                //   leaf order (tie-break), parent = the reference BVH node whose child it is
};
static_assert(sizeof(DTri) == 48, "triangle record is 48 B");

// Shading record by original triangle id: normal + material (modelLoader.h:14-19).
struct alignas(16) DShade {
    float nx, ny, nz;
    int32_t mat;
};

struct DMat {   // materialDesc (modelLoader.h:21-25)
    double albedo[3];
    double emission[3];
};

// Emissive triangle for the area-CDF pick (kernel.cu:468-495): area precomputed with the
// reference's float expression length(cross(a1,a2))/2; slot num_lights holds triangle 0,
// the reference's fallback when nothing is picked.
struct alignas(16) DLight {
    float area;
    int32_t tri;
    float v0[3], a1[3], a2[3];
    float pad;
};
static_assert(sizeof(DLight) == 48, "light record is 48 B");

struct Cam {    // camera.h:26-34
    float pos[3];
    float dist, focal, radius;
    int32_t w, h;
};

// Node of the render-path BVH4 (collapsed SAH BVH): 4 child boxes SoA + 4 child refs, 128 B.
struct alignas(16) DNode4 {
    float4 lox, loy, loz, hix, hiy, hiz;
    uint4 child;     // inner index, kLeaf | slot, or 0xffffffff (empty); leaf children first, with
                     // consecutive triangle slots (child k of a node's leaves at slot base + k)
    uint4 pad;
};
static_assert(sizeof(DNode4) == 128, "BVH4 node is 128 B");

// ------------------------------------------------------------------ layout constants
// Byte-sliced jump tables (rng_init, pt_device.h): 5 words per entry, padded to 8.
constexpr int kJumpEntryWords = 8;
constexpr int kLeafRing = 4;               // LDS leaf-queue entries per lane (one per node with entered leaves)
constexpr int kRing = 16;                 // LDS stack entries per lane; deeper entries spill to HBM
// leaf queue entry: (the node's first leaf slot << kLeafBits) | mask of the entered leaves' slots
// (a node's leaf children hold at most kLeafBits triangles; slots < 2^(31 - kLeafBits))
constexpr uint32_t kLeafBits = 8;
constexpr int kWaveLdsWords = (kRing + kLeafRing) * 64;
// BVH4 nodes 0..top-1 (the best-first top of the tree, pack_scene) are staged in the block's LDS
// by the wavefront kernel, 112 B each (the node without its pad; stride 28 dwords, so 16
// consecutive nodes occupy disjoint banks): lanes visiting them read LDS instead of issuing
// vector-memory loads -- the kernel's limiting pipe (TA/TD, DESIGN.md "Measurement").
constexpr uint32_t kTopNodeBytes = 112;
// what fits next to the rings with 5 blocks of 256 threads per CU: LDS is granted in 1280-B granules,
// 32000 B per block = 4 x 5120 B of rings + 160 B of counters + 208 B of light-probe emitters
// (pt_render.hip) + 240 B of NEE light records + 97 x 112 B
constexpr uint32_t kTopNodesMax = 97;
constexpr uint32_t kQueues = 8;              // unit counters (Args::unit_queues > 1)
constexpr uint32_t kMaxProbeEmitters = 4;    // last-bounce light probe: at most this many emissive triangles

}  // namespace ptd
