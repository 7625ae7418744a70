// arx_scene.cpp -- the host-only scene image behind arx_set_scene (arx_internal.hpp SceneImage): input
// checks, the content hashes, the process-wide cache of built scenes, the build itself and the byte
// image a group's rank 0 broadcasts.  Nothing here touches a device.
#include <atomic>
#include <cmath>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {
std::atomic<uint64_t> g_scene_builds{0};

// 64-bit content hash (word-wise multiply / xor-shift mix; not cryptographic): identifies a built
// tree in stored profiles (arx_stats::tree_hash).
uint64_t hash_words(const void* p, size_t bytes, uint64_t h) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        uint64_t w;
        std::memcpy(&w, b + i, 8);
        h ^= w * 0x9E3779B97F4A7C15ull;
        h = (h << 27 | h >> 37) * 0xC2B2AE3D27D4EB4Full;
    }
    for (; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return h;
}

uint64_t scene_hash(const BvhBuild& b) {
    uint64_t h = hash_words(b.nodes.data(), b.nodes.size() * sizeof(BvhNode), 0x243F6A8885A308D3ull);
    return hash_words(b.tris.data(), b.tris.size() * sizeof(TriRec), h);
}

// serialized scene: header, nodes, triangle records
struct SceneHeader {
    uint64_t magic;
    uint64_t n_nodes, n_tris;
    int64_t n_input;
    uint64_t hash;
    ChildRef root;
    int32_t depth;
    int32_t pad;
};
constexpr uint64_t kSceneMagic = 0x3145435341585241ull;  // "ARXSCE1"

// The part of a scene image derived from its BVH2: the coded copy.
void finish_scene_image(SceneImage& img) {
    img.coded.resize(img.bvh.nodes.size());
    code_nodes(img.bvh.nodes.data(), img.bvh.nodes.size(), img.coded.data());
}

// Process-wide cache of built scenes, keyed by a 128-bit hash of the input arrays: renderers and
// groups given the same geometry (a second group for frames in flight, a C++ shim beside a Python
// renderer) share one build.  Weak references: a scene no renderer holds any more is rebuilt.
std::mutex g_scene_cache_mu;
std::map<std::pair<uint64_t, uint64_t>, std::weak_ptr<const SceneImage>> g_scene_cache;

// The builder settings a tree depends on (build_params(): leaf size from arx_debug_set_leaf_max,
// the tools' edits), hashed field by field so the scene cache never hands out a tree built with
// other settings.  `threads` only changes the build's speed, not its result.
uint64_t build_params_hash() {
    const BuildParams& b = build_params();
    const int32_t iv[] = {b.bins, b.leaf_max, b.spatial ? 1 : 0, b.spatial_bins, b.spatial_max_depth, b.max_depth,
                          b.rotation_passes};
    const float fv[] = {b.trav_cost, b.isect_cost, b.spatial_alpha, b.spatial_budget};
    return hash_words(fv, sizeof(fv), hash_words(iv, sizeof(iv), 0xB7E151628AED2A6Bull));
}
}  // namespace

arx_status arx::check_scene_input(const float* tri_v, const float* tri_abs, int64_t n) {
    if (n < 0 || (n > 0 && (!tri_v || !tri_abs))) return fail(ARX_ERR_INVALID_ARGUMENT, "bad scene arrays");
    if (n > (int64_t)0x3fffffff) return fail(ARX_ERR_INVALID_ARGUMENT, "too many triangles");
    for (int64_t i = 0; i < 9 * n; ++i)
        if (!std::isfinite(tri_v[i])) return fail(ARX_ERR_INVALID_ARGUMENT, "non-finite vertex at %lld", (long long)i / 9);
    // absorption in [0, 1], or the receiver marks -1 / -2 (getMaterialAbsorption): the int64
    // fixed-point histogram's headroom (arx_frac_bits) assumes a ray's energy never grows
    for (int64_t i = 0; i < n; ++i) {
        const float ab = tri_abs[i];
        if (!(ab >= 0.0f && ab <= 1.0f) && ab != -1.0f && ab != -2.0f)
            return fail(ARX_ERR_INVALID_ARGUMENT, "absorption %g of triangle %lld: must be in [0, 1] (or -1 / -2 receiver)",
                        (double)ab, (long long)i);
    }
    return ARX_OK;
}

// The trace kernel addresses nodes and triangle records through buffer resources with 32-bit byte
// offsets and num_records 0x7fffffff (arx_trace_device.hpp buffer_rsrc; a load past it returns zeros, which
// the leaf step uses for idle lanes): every record must end below 2^31 bytes, or a triangle would read
// back as zeros (det 0, a silently dropped hit).  44.7 M triangle records / 33.5 M coded nodes.
arx_status arx::check_buffer_offsets(size_t n_nodes, size_t n_tris) {
    constexpr uint64_t kMax = 0x7fffffffull;
    if ((uint64_t)n_tris * sizeof(TriRec) > kMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "scene too large: %llu triangle records x %zu B exceed the trace kernel's "
                    "31-bit buffer offsets", (unsigned long long)n_tris, sizeof(TriRec));
    if ((uint64_t)n_nodes * sizeof(BvhNode) > kMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "scene too large: %llu BVH nodes x %zu B exceed the trace kernel's "
                    "31-bit buffer offsets", (unsigned long long)n_nodes, sizeof(BvhNode));
    return ARX_OK;
}

// The opt-in CW4 collapse and its buffer's triangle image, made once, on first request.
const SceneImage::Wide& SceneImage::wide() const {
    std::call_once(wide_once_, [this] {
        collapse_w4(bvh, 1, 0, bvh.root, kW4SceneRoot, kW4SceneUnit, wide_.w4);
        wide_.wimage.assign((size_t)wide_.w4.unit_end * 4, 0u);
        for (const auto& lt : wide_.w4.leaf_tris)
            std::memcpy(wide_.wimage.data() + (size_t)lt.first * 4, &bvh.tris[(size_t)lt.second], sizeof(TriRec));
    });
    return wide_;
}

SceneRef arx::build_scene_image(const float* tri_v, const float* tri_abs, int64_t n) {
    const size_t bytes = (size_t)(n > 0 ? n : 0);
    const uint64_t prm = build_params_hash();
    const std::pair<uint64_t, uint64_t> key{
        hash_words(tri_abs, bytes * sizeof(float), hash_words(tri_v, 9 * bytes * sizeof(float), 0x9E3779B97F4A7C15ull)) ^ prm,
        hash_words(tri_v, 9 * bytes * sizeof(float), hash_words(tri_abs, bytes * sizeof(float), 0x6A09E667F3BCC909ull) ^
                                                         (uint64_t)n)};
    {
        std::lock_guard<std::mutex> lock(g_scene_cache_mu);
        auto it = g_scene_cache.find(key);
        if (it != g_scene_cache.end()) {
            if (SceneRef hit = it->second.lock()) return hit;
            g_scene_cache.erase(it);
        }
    }
    auto img = std::make_shared<SceneImage>();
    build_bvh(tri_v, tri_abs, 0.5f, n, 0, img->bvh);
    bfs_prefix_order(img->bvh, 1023);  // the top levels of the scene tree breadth-first (node locality)
    relocate_bvh(img->bvh, 1, 0);
    finish_scene_image(*img);
    img->n_input = n;
    img->hash = scene_hash(img->bvh);
    g_scene_builds.fetch_add(1);
    std::lock_guard<std::mutex> lock(g_scene_cache_mu);
    for (auto it = g_scene_cache.begin(); it != g_scene_cache.end();)  // drop scenes nobody holds any more
        it = it->second.expired() ? g_scene_cache.erase(it) : std::next(it);
    g_scene_cache[key] = img;
    return img;
}

std::vector<uint8_t> arx::serialize_scene(const SceneImage& s) {
    SceneHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = kSceneMagic;
    h.n_nodes = s.bvh.nodes.size();
    h.n_tris = s.bvh.tris.size();
    h.n_input = s.n_input;
    h.hash = s.hash;
    h.root = s.bvh.root;
    h.depth = s.bvh.depth;
    const size_t nb = h.n_nodes * sizeof(BvhNode), tb = h.n_tris * sizeof(TriRec);
    std::vector<uint8_t> out(sizeof(h) + nb + tb);
    std::memcpy(out.data(), &h, sizeof(h));
    if (nb) std::memcpy(out.data() + sizeof(h), s.bvh.nodes.data(), nb);
    if (tb) std::memcpy(out.data() + sizeof(h) + nb, s.bvh.tris.data(), tb);
    return out;
}

SceneRef arx::deserialize_scene(const uint8_t* p, size_t n, const char** why) {
    SceneHeader h;
    if (!p || n < sizeof(h)) {
        *why = "short scene image";
        return nullptr;
    }
    std::memcpy(&h, p, sizeof(h));
    if (h.magic != kSceneMagic || h.n_nodes > (1ull << 31) || h.n_tris > (1ull << 31) ||
        n != sizeof(h) + h.n_nodes * sizeof(BvhNode) + h.n_tris * sizeof(TriRec)) {
        *why = "malformed scene image";
        return nullptr;
    }
    auto img = std::make_shared<SceneImage>();
    img->bvh.nodes.resize(h.n_nodes);
    img->bvh.tris.resize(h.n_tris);
    if (h.n_nodes) std::memcpy(img->bvh.nodes.data(), p + sizeof(h), h.n_nodes * sizeof(BvhNode));
    if (h.n_tris)
        std::memcpy(img->bvh.tris.data(), p + sizeof(h) + h.n_nodes * sizeof(BvhNode), h.n_tris * sizeof(TriRec));
    img->bvh.root = h.root;
    img->bvh.depth = h.depth;
    img->n_input = h.n_input;
    img->hash = scene_hash(img->bvh);
    if (img->hash != h.hash) {
        *why = "scene image hash mismatch";
        return nullptr;
    }
    if (!validate_bvh_range(img->bvh.nodes.data(), 1, img->bvh.nodes.size(), 1 + img->bvh.nodes.size(),
                            img->bvh.tris.size(), why))
        return nullptr;
    finish_scene_image(*img);
    return img;
}

extern "C" {

uint64_t arx_scene_build_count(void) { return g_scene_builds.load(); }

arx_status arx_debug_scene_roundtrip(const float* tri_v, const float* tri_abs, int64_t n, uint64_t* hash,
                                     uint64_t* bytes) {
    arx_status st = check_scene_input(tri_v, tri_abs, n);
    if (st != ARX_OK) return st;
    SceneRef a = build_scene_image(tri_v, tri_abs, n);
    const std::vector<uint8_t> img = serialize_scene(*a);
    const char* why = "";
    SceneRef b = deserialize_scene(img.data(), img.size(), &why);
    if (!b) return fail(ARX_ERR_INTERNAL, "scene image: %s", why);
    const bool same = a->hash == b->hash && a->n_input == b->n_input && a->bvh.depth == b->bvh.depth &&
                      a->bvh.nodes.size() == b->bvh.nodes.size() && a->bvh.tris.size() == b->bvh.tris.size() &&
                      std::memcmp(a->bvh.nodes.data(), b->bvh.nodes.data(), a->bvh.nodes.size() * sizeof(BvhNode)) == 0 &&
                      std::memcmp(a->bvh.tris.data(), b->bvh.tris.data(), a->bvh.tris.size() * sizeof(TriRec)) == 0 &&
                      std::memcmp(a->coded.data(), b->coded.data(), a->coded.size() * sizeof(BvhNode)) == 0 &&
                      a->wide().wimage == b->wide().wimage && a->wide().w4.nodes.size() == b->wide().w4.nodes.size() &&
                      std::memcmp(a->wide().w4.nodes.data(), b->wide().w4.nodes.data(),
                                  a->wide().w4.nodes.size() * sizeof(W4NodeF)) == 0 &&
                      std::memcmp(&a->bvh.root, &b->bvh.root, sizeof(ChildRef)) == 0;
    if (!same) return fail(ARX_ERR_INTERNAL, "scene image round trip changed the tree");
    if (hash) *hash = a->hash;
    if (bytes) *bytes = img.size();
    return ARX_OK;
}

arx_status arx_debug_check_tree_limits(uint64_t n_nodes, uint64_t n_tris) {
    return check_buffer_offsets((size_t)n_nodes, (size_t)n_tris);
}

arx_status arx_debug_set_leaf_max(int32_t leaf_max) {
    if (leaf_max < 1 || leaf_max > 15) return fail(ARX_ERR_INVALID_ARGUMENT, "leaf_max %d outside [1, 15]", leaf_max);
    build_params().leaf_max = leaf_max;
    return ARX_OK;
}

}  // extern "C"
