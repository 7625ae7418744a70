// arx_capi_device_scene.cpp -- the device scene behind the C ABI (include/arx.h): the receiver model, its
// placement, and ensure_device_scene -- the tree on the device brought up to date before a launch (buffers,
// quantization grid, uploads, re-quantization, the receiver's refit) -- with the arx_debug_* entry points
// that read or steer it.
//
// Host-side counterpart of R/prebuild/obj_raytracer/AudioRenderer.cpp (buildAccel, buildSBT, reload),
// re-designed for HIP: persistent device buffers, and no full rebuild when the listener moves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

// OptixModel.cpp:178-193 (glm::rotate(mat4(1), -radians(yaw), +Y) * v, then + camera),
// restated with glm's exact operation order (matrix_transform.inl rotate, type_mat4x4.inl
// operator*): x' = (c*x + R10*y) + (s*z + 0), y' = (0*x + R11*y) + (0*z + 0),
// z' = (-s*x + 0*y) + (c*z + 0) with c = cos(-a), s = sin(-a), R11 = c + (1 - c).
void place_vertices(const float* local, int64_t n_vertices, float x, float y, float z, float yaw_deg, float* out) {
    const float ang = yaw_deg * static_cast<float>(0.01745329251994329576923690768489);  // glm::radians
    const float a = -ang;
    const float c = std::cos(a);
    const float s = std::sin(a);
    const float t1 = 1.0f - c;   // temp = (1 - c) * axis, axis = (0, 1, 0)
    const float r00 = c + 0.0f * 0.0f;
    const float r10 = t1 * 0.0f - s * 0.0f;
    const float r20 = 0.0f * 0.0f + s * 1.0f;
    const float r01 = 0.0f * 1.0f + s * 0.0f;
    const float r11 = c + t1 * 1.0f;
    const float r21 = 0.0f * 1.0f - s * 0.0f;
    const float r02 = 0.0f * 0.0f - s * 1.0f;
    const float r12 = t1 * 0.0f + s * 0.0f;
    const float r22 = c + 0.0f * 0.0f;
    for (int64_t i = 0; i < n_vertices; ++i) {
        const float vx = local[3 * i + 0], vy = local[3 * i + 1], vz = local[3 * i + 2];
        const float ox = (r00 * vx + r10 * vy) + (r20 * vz + 0.0f * 1.0f);
        const float oy = (r01 * vx + r11 * vy) + (r21 * vz + 0.0f * 1.0f);
        const float oz = (r02 * vx + r12 * vy) + (r22 * vz + 0.0f * 1.0f);
        out[3 * i + 0] = x + ox;
        out[3 * i + 1] = y + oy;
        out[3 * i + 2] = z + oz;
    }
}

}  // namespace

// Rotation of place_vertices (row-major r00 r10 r20 / r01 r11 r21 / r02 r12 r22), exactly its floats.
void arx::receiver_rotation(float yaw_deg, float m[9]) {
    const float ang = yaw_deg * static_cast<float>(0.01745329251994329576923690768489);
    const float a = -ang, c = std::cos(a), s = std::sin(a), t1 = 1.0f - c;
    m[0] = c + 0.0f * 0.0f; m[1] = t1 * 0.0f - s * 0.0f; m[2] = 0.0f * 0.0f + s * 1.0f;
    m[3] = 0.0f * 1.0f + s * 0.0f; m[4] = c + t1 * 1.0f; m[5] = 0.0f * 1.0f - s * 0.0f;
    m[6] = 0.0f * 0.0f - s * 1.0f; m[7] = t1 * 0.0f + s * 0.0f; m[8] = c + 0.0f * 0.0f;
}

namespace {

// The receiver sub-tree, built once in the receiver's local frame whenever the receiver model or
// the scene changes (its triangle ids and offsets follow the scene); listener moves refit it on
// the device (arx_receiver.hip).  Larger receivers than the refit kernel's LDS holds are rebuilt on
// the host per move instead (recv_refit = false).
arx_status prepare_receiver_model(arx_renderer* r) {
    std::vector<float> tv, ab;
    float radius = 0.0f;
    for (int side = 0; side < 2; ++side) {
        const std::vector<float>& loc = r->recv_local[side];
        tv.insert(tv.end(), loc.begin(), loc.end());
        ab.insert(ab.end(), loc.size() / 9, side == 0 ? -1.0f : -2.0f);
        for (size_t i = 0; i + 2 < loc.size(); i += 3)
            radius = std::max(radius, std::sqrt(loc[i] * loc[i] + loc[i + 1] * loc[i + 1] + loc[i + 2] * loc[i + 2]));
    }
    const int64_t n = (int64_t)ab.size();
    r->recv_refit = n <= kRefitMaxTris;
    r->recv_radius = radius * 1.0001f + 1e-6f;  // |R v| = |v|: the rotated halves stay in this ball
    if (!r->recv_refit) return ARX_OK;
    const BvhBuild& sc = r->scene_img->bvh;
    build_bvh(tv.data(), ab.data(), 0.0f, n, (int32_t)r->scene_img->n_input, r->recv);
    relocate_bvh(r->recv, 1 + (int32_t)sc.nodes.size(), (int32_t)sc.tris.size());
    const char* why = "";
    const size_t total_nodes = 1 + sc.nodes.size() + r->recv.nodes.size();
    const size_t total_tris = sc.tris.size() + r->recv.tris.size();
    if (!validate_bvh_range(r->recv.nodes.data(), 1 + sc.nodes.size(), r->recv.nodes.size(), total_nodes,
                            total_tris, &why))
        return fail(ARX_ERR_INTERNAL, "BVH validation failed (receiver): %s", why);
    // refit schedule: inner nodes by depth, deepest level first
    const int32_t base = 1 + (int32_t)sc.nodes.size();
    std::vector<int32_t> depth(r->recv.nodes.size(), 0);
    int32_t max_d = 0;
    for (size_t i = 0; i < r->recv.nodes.size(); ++i)  // parents precede children (pre-order)
        for (int c = 0; c < 2; ++c)
            if (r->recv.nodes[i].d[2 + c] == 0) {
                const int32_t ch = r->recv.nodes[i].d[c] - base;
                depth[(size_t)ch] = depth[i] + 1;
                max_d = std::max(max_d, depth[(size_t)ch]);
            }
    std::vector<int32_t> order, start;
    for (int32_t d = max_d; d >= 0 && !r->recv.nodes.empty(); --d) {
        start.push_back((int32_t)order.size());
        for (size_t i = 0; i < r->recv.nodes.size(); ++i)
            if (depth[i] == d) order.push_back((int32_t)i);
    }
    start.push_back((int32_t)order.size());
    r->recv_levels = r->recv.nodes.empty() ? 0 : (int32_t)start.size() - 1;
    if (receiver_refit_lds((int32_t)r->recv.tris.size(), (int32_t)r->recv.nodes.size(), r->recv_levels) > 160 * 1024) {
        r->recv_refit = false;  // beyond one workgroup's LDS: rebuilt on the host per move instead
        return ARX_OK;
    }
    // made anew for every model, at its size
    arx_status st;
    r->d_recv_local.release();
    r->d_recv_nodes.release();
    r->d_recv_levels.release();
    if ((st = r->d_recv_local.reserve(std::max<size_t>(1, r->recv.tris.size()))) != ARX_OK ||
        (st = r->d_recv_nodes.reserve(std::max<size_t>(1, r->recv.nodes.size()))) != ARX_OK ||
        (st = r->d_recv_levels.reserve(order.size() + start.size())) != ARX_OK)
        return st;
    if (!r->recv.tris.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_local.p, r->recv.tris.data(), r->recv.tris.size() * sizeof(TriRec),
                               hipMemcpyHostToDevice, r->stream));
    if (!r->recv.nodes.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_nodes.p, r->recv.nodes.data(), r->recv.nodes.size() * sizeof(BvhNode),
                               hipMemcpyHostToDevice, r->stream));
    std::vector<int32_t> lv(order);
    lv.insert(lv.end(), start.begin(), start.end());
    ARX_HIP(hipMemcpyAsync(r->d_recv_levels.p, lv.data(), lv.size() * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));  // pageable sources
    r->recv_level_count = (int32_t)order.size();
    if (!r->use_w4) return ARX_OK;
    // opt-in CW4 path only: the receiver's CW4 layout (root at unit kW4RecvRoot, blocks after the
    // scene's) for the refit
    collapse_w4(r->recv, base, (int32_t)sc.tris.size(), r->recv.root, kW4RecvRoot, r->scene_img->wide().w4.unit_end,
                r->recv4);
    std::vector<int32_t> w4n(11 * r->recv4.nodes.size()), w4t(2 * r->recv4.leaf_tris.size());
    for (size_t i = 0; i < r->recv4.nodes.size(); ++i) {
        std::copy(r->recv4.src.begin() + 8 * i, r->recv4.src.begin() + 8 * i + 8, w4n.begin() + 11 * i);
        w4n[11 * i + 8] = (int32_t)r->recv4.nodes[i].meta;
        w4n[11 * i + 9] = (int32_t)r->recv4.nodes[i].base;
        w4n[11 * i + 10] = (int32_t)r->recv4.nodes[i].self;
    }
    for (size_t i = 0; i < r->recv4.leaf_tris.size(); ++i) {
        w4t[2 * i] = (int32_t)r->recv4.leaf_tris[i].first;
        w4t[2 * i + 1] = r->recv4.leaf_tris[i].second;
    }
    r->d_recv_w4.release();
    r->d_recv_w4_tris.release();
    if ((st = r->d_recv_w4.reserve(std::max<size_t>(1, w4n.size()))) != ARX_OK ||
        (st = r->d_recv_w4_tris.reserve(std::max<size_t>(1, w4t.size()))) != ARX_OK)
        return st;
    if (!w4n.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_w4.p, w4n.data(), w4n.size() * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    if (!w4t.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_w4_tris.p, w4t.data(), w4t.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                               r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));  // pageable sources
    return ARX_OK;
}

// Box padding of the refit kernel for a receiver at `centre`: at least the builder's
// 1e-5 * max|coordinate| for any vertex of the placed receiver (|v| <= |centre| + radius).
float builder_pad(const arx_renderer* r, const float centre[3]) {
    float mx = 0.0f;
    for (int k = 0; k < 3; ++k) mx = std::max(mx, std::fabs(centre[k]));
    return std::max(1e-5f * (mx + r->recv_radius) * 1.001f, 1e-6f);
}

// The grid over the emitter, the scene and, where given, the box [blo, bhi]; keep_old: and the grid in
// use, with half the extent as margin (a grid that grows) instead of a tenth (a new one).
QGrid span_grid(const arx_renderer* r, const float* blo, const float* bhi, bool keep_old) {
    const BvhBuild& sc = r->scene_img->bvh;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = hi[k] = r->emitter[k];
        if (sc.root.count >= 0) {
            lo[k] = std::min(lo[k], sc.root.lo[k]);
            hi[k] = std::max(hi[k], sc.root.hi[k]);
        }
        if (blo) {
            lo[k] = std::min(lo[k], blo[k]);
            hi[k] = std::max(hi[k], bhi[k]);
        }
        if (keep_old) {
            lo[k] = std::min(lo[k], r->qgrid.origin[k]);
            hi[k] = std::max(hi[k], r->qgrid.origin[k] + 65000.0f * r->qgrid.scale[k]);
        }
    }
    return make_qgrid(lo, hi, keep_old ? 0.5 : 0.1);
}

const SceneImage::Wide& wide_of(const arx_renderer* r) {
    static const SceneImage::Wide kNoWide;
    return r->use_w4 ? r->scene_img->wide() : kNoWide;
}

// What one ensure_device_scene found so far, handed from step to step.
struct SceneUpdate {
    bool model_changed, pose_changed;
    size_t n_nodes, n_tris;
    bool full;    // the scene is uploaded again (new scene, or its arrays were re-made)
    bool regrid;  // the quantization grid was made or grown
    float rlo[3], rhi[3];  // the placed receiver's bound
    bool recv_empty;
};

// Host path (receivers beyond the refit kernel's capacity): receiver halves placed in world space, left
// then right (placeReceiver OptixModel.cpp:153-157), sub-tree rebuilt.
void place_host_receiver(arx_renderer* r) {
    const SceneImage& img = *r->scene_img;
    const BvhBuild& sc = img.bvh;
    std::vector<float> tv;
    std::vector<float> ab;
    for (int side = 0; side < 2; ++side) {
        const std::vector<float>& loc = r->recv_local[side];
        const int64_t nt = (int64_t)loc.size() / 9;
        size_t base = tv.size();
        tv.resize(base + loc.size());
        place_vertices(loc.data(), 3 * nt, r->center[0], r->center[1], r->center[2], r->yaw, tv.data() + base);
        ab.insert(ab.end(), (size_t)nt, side == 0 ? -1.0f : -2.0f);
    }
    build_bvh(tv.data(), ab.data(), 0.0f, (int64_t)ab.size(), (int32_t)img.n_input, r->recv);
    relocate_bvh(r->recv, 1 + (int32_t)sc.nodes.size(), (int32_t)sc.tris.size());
    if (r->use_w4)
        collapse_w4(r->recv, 1 + (int32_t)sc.nodes.size(), (int32_t)sc.tris.size(), r->recv.root, kW4RecvRoot,
                    img.wide().w4.unit_end, r->recv4);
}

// Room for the tree: the node and triangle arrays, and the opt-in CW4 copy's (use_w4 only: the buffer
// holds the scene's units, then the receiver's; the f32 records are the top node, the scene's nodes and
// (host-built receivers) the receiver's).  An array that is re-made holds nothing: u.full.
arx_status reserve_tree(arx_renderer* r, SceneUpdate& u) {
    arx_status st;
    if (u.n_nodes > r->nodes_cap()) {
        if ((st = r->d_cnodes.reserve(u.n_nodes, 1024)) != ARX_OK || (st = r->d_qnodes.reserve(u.n_nodes, 1024)) != ARX_OK)
            return st;
        u.full = true;
    }
    if (u.n_tris > r->d_tris.cap || !r->d_tris.p) {
        if ((st = r->d_tris.reserve(u.n_tris, 4096)) != ARX_OK) return st;
        u.full = true;
    }
    const SceneImage::Wide& wide = wide_of(r);
    const size_t w_units = r->use_w4 ? std::max<size_t>(r->recv4.unit_end, wide.w4.unit_end) : 0;
    const size_t host_recv_w4 = (r->recv_refit || !r->use_w4) ? 0 : r->recv4.nodes.size();
    const size_t n_w4f = r->use_w4 ? 1 + wide.w4.nodes.size() + host_recv_w4 : 0;
    if (w_units > r->d_wbuf.cap) {
        if ((st = r->d_wbuf.reserve(w_units, 4096)) != ARX_OK) return st;
        u.full = true;
    }
    if (n_w4f > r->d_w4f.cap) {
        if ((st = r->d_w4f.reserve(n_w4f, 1024)) != ARX_OK) return st;
        u.full = true;
    }
    r->n_w4f = n_w4f;
    return ARX_OK;
}

// The quantization grid: made when the scene changes, grown when the receiver leaves it (a
// listener walking out of the room): the new grid spans the old one, the scene, the receiver
// and the emitter with half the extent as margin, so such a walk re-grids once or twice, not
// per frame.  Either way the quantized copy is re-made on the device from the coded nodes
// (launch_requant16): no host quantization, no upload, no synchronisation inside a frame.  An
// emitter off the grid (checked per launch, arx_trace_rays) makes that launch take the f32 nodes.
void update_grid(arx_renderer* r, SceneUpdate& u) {
    receiver_bound(r, r->center, u.rlo, u.rhi, &u.recv_empty);
    const bool grow = !u.full && r->qgrid_set && u.pose_changed && !u.recv_empty && !qgrid_contains(r->qgrid, u.rlo, u.rhi);
    u.regrid = u.full || !r->qgrid_set || grow;
    if (u.regrid) {
        r->qgrid = span_grid(r, u.recv_empty ? nullptr : u.rlo, u.rhi, grow);
        r->qgrid_set = true;
    }
}

// CW4 (opt-in): the scene's buffer image and node records once per scene; the top node's
// record (child 0 the scene root, child 1 the host-built receiver's root or, on the refit
// path, a placeholder the refit kernel replaces); a host-built receiver's records and triangles.
// wtop and rimage are the caller's: pageable sources that live until its synchronisation.
arx_status upload_w4(arx_renderer* r, bool full, W4NodeF& wtop, std::vector<uint32_t>& rimage) {
    const BvhBuild& sc = r->scene_img->bvh;
    const SceneImage::Wide& wide = wide_of(r);
    const bool host_recv = !r->recv_refit;
    std::memset(&wtop, 0, sizeof(wtop));
    wtop.base = kW4SceneRoot;
    wtop.self = 0;
    if (sc.root.count >= 0) {
        wtop.meta |= 1u;
        for (int k = 0; k < 3; ++k) {
            wtop.lo[0][k] = sc.root.lo[k];
            wtop.hi[0][k] = sc.root.hi[k];
        }
    }
    if (host_recv && r->recv.root.count >= 0) {
        wtop.meta |= 1u << 2;
        for (int k = 0; k < 3; ++k) {
            wtop.lo[1][k] = r->recv.root.lo[k];
            wtop.hi[1][k] = r->recv.root.hi[k];
        }
    }
    ARX_HIP(hipMemcpyAsync(r->d_w4f.p, &wtop, sizeof(W4NodeF), hipMemcpyHostToDevice, r->stream));
    if (full && !wide.wimage.empty())
        ARX_HIP(hipMemcpyAsync(r->d_wbuf.p, wide.wimage.data(), wide.wimage.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, r->stream));
    if (full && !wide.w4.nodes.empty())
        ARX_HIP(hipMemcpyAsync(r->d_w4f.p + 1, wide.w4.nodes.data(), wide.w4.nodes.size() * sizeof(W4NodeF),
                               hipMemcpyHostToDevice, r->stream));
    if (!host_recv) return ARX_OK;
    if (!r->recv4.nodes.empty())
        ARX_HIP(hipMemcpyAsync(r->d_w4f.p + 1 + wide.w4.nodes.size(), r->recv4.nodes.data(),
                               r->recv4.nodes.size() * sizeof(W4NodeF), hipMemcpyHostToDevice, r->stream));
    const size_t u0 = wide.w4.unit_end;
    rimage.assign((r->recv4.unit_end - u0) * 4, 0u);
    for (const auto& lt : r->recv4.leaf_tris)
        std::memcpy(rimage.data() + (size_t)(lt.first - u0) * 4, &r->recv.tris[(size_t)lt.second], sizeof(TriRec));
    if (!rimage.empty())
        ARX_HIP(hipMemcpyAsync(r->d_wbuf.p + u0, rimage.data(), rimage.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               r->stream));
    return ARX_OK;
}

// Host uploads, only when the scene or the receiver model changed, or on the host-receiver
// path: the top node (its receiver child comes from the refit kernel on the refit path),
// the scene's coded nodes and triangles, the receiver part on the host path.
arx_status upload_tree(arx_renderer* r, const SceneUpdate& u) {
    const SceneImage& img = *r->scene_img;
    const BvhBuild& sc = img.bvh;
    const bool host_recv = !r->recv_refit;
    BvhNode top = make_node(sc.root, host_recv ? r->recv.root : empty_child());
    const char* why = "";
    if ((host_recv && !validate_bvh_range(r->recv.nodes.data(), 1 + sc.nodes.size(), r->recv.nodes.size(), u.n_nodes,
                                          u.n_tris, &why)) ||
        !validate_bvh_range(&top, 0, 1, u.n_nodes, u.n_tris, &why))
        return fail(ARX_ERR_INTERNAL, "BVH validation failed: %s", why);
    BvhNode ctop;  // pageable sources below live until the synchronisation at the end of this function
    code_nodes(&top, 1, &ctop);
    std::vector<BvhNode> crecv(host_recv ? r->recv.nodes.size() : 0);
    if (host_recv) code_nodes(r->recv.nodes.data(), r->recv.nodes.size(), crecv.data());
    ARX_HIP(hipMemcpyAsync(r->d_cnodes.p, &ctop, sizeof(BvhNode), hipMemcpyHostToDevice, r->stream));
    if (u.full && !img.coded.empty())
        ARX_HIP(hipMemcpyAsync(r->d_cnodes.p + 1, img.coded.data(), img.coded.size() * sizeof(BvhNode),
                               hipMemcpyHostToDevice, r->stream));
    if (u.full && !sc.tris.empty())
        ARX_HIP(hipMemcpyAsync(r->d_tris.p, sc.tris.data(), sc.tris.size() * sizeof(TriRec), hipMemcpyHostToDevice,
                               r->stream));
    if (host_recv && !crecv.empty())
        ARX_HIP(hipMemcpyAsync(r->d_cnodes.p + 1 + sc.nodes.size(), crecv.data(), crecv.size() * sizeof(BvhNode),
                               hipMemcpyHostToDevice, r->stream));
    if (host_recv && !r->recv.tris.empty())
        ARX_HIP(hipMemcpyAsync(r->d_tris.p + sc.tris.size(), r->recv.tris.data(), r->recv.tris.size() * sizeof(TriRec),
                               hipMemcpyHostToDevice, r->stream));
    W4NodeF wtop;
    std::vector<uint32_t> rimage;
    if (r->use_w4)
        if (const arx_status st = upload_w4(r, u.full, wtop, rimage); st != ARX_OK) return st;
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

// The listener move itself: one kernel, no host copies, no synchronisation.
arx_status refit_receiver(arx_renderer* r) {
    const BvhBuild& sc = r->scene_img->bvh;
    RefitArgs a = refit_args(r);
    receiver_rotation(r->yaw, a.m);
    for (int k = 0; k < 3; ++k) a.t[k] = r->center[k];
    // >= the builder's pad; receiver_bound covers it (a debug pad does not: the off-grid test)
    a.pad = refit_pad(r, r->center);
    if (!r->q_valid) a.qnodes = nullptr;
    if (r->q_valid && r->use_w4) {  // the opt-in CW4 copy follows the quantized one (same grid)
        a.wbuf = r->d_wbuf.p;
        a.w4_nodes = r->d_recv_w4.p;
        a.n_w4 = (int32_t)r->recv4.nodes.size();
        a.w4_tris = r->d_recv_w4_tris.p;
        a.n_w4_tris = (int32_t)r->recv4.leaf_tris.size();
        a.scene_nonempty = sc.root.count >= 0 ? 1 : 0;
        for (int k = 0; k < 3; ++k) {
            a.scene_lo[k] = sc.root.lo[k];
            a.scene_hi[k] = sc.root.hi[k];
        }
    }
    if (a.n_tris > 0) ARX_HIP(launch_receiver_refit(a, r->stream));
    return ARX_OK;
}

}  // namespace

float arx::refit_pad(const arx_renderer* r, const float centre[3]) {
    return r->debug_refit_pad > 0.0f ? r->debug_refit_pad : builder_pad(r, centre);
}

void arx::receiver_bound(const arx_renderer* r, const float centre[3], float lo[3], float hi[3], bool* empty) {
    *empty = (r->recv_local[0].size() + r->recv_local[1].size()) == 0;
    const float pad = r->recv_refit ? builder_pad(r, centre) : 0.0f;
    for (int k = 0; k < 3; ++k) {
        if (r->recv_refit) {
            lo[k] = centre[k] - r->recv_radius - 2.0f * pad;
            hi[k] = centre[k] + r->recv_radius + 2.0f * pad;
        } else {
            lo[k] = r->recv.root.lo[k];
            hi[k] = r->recv.root.hi[k];
        }
    }
}

bool arx::emitter_in_receiver_box(const arx_renderer* r, const float centre[3], float grow) {
    float lo[3], hi[3];
    bool empty = false;
    receiver_bound(r, centre, lo, hi, &empty);
    bool inside = !empty;
    for (int k = 0; k < 3; ++k) inside = inside && r->emitter[k] >= lo[k] - grow && r->emitter[k] <= hi[k] + grow;
    return inside;
}

RefitArgs arx::refit_args(const arx_renderer* r) {
    const BvhBuild& sc = r->scene_img->bvh;
    RefitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.local_tris = r->d_recv_local.p;
    a.n_tris = (int32_t)r->recv.tris.size();
    a.tri_base = (int32_t)sc.tris.size();
    a.local_nodes = r->d_recv_nodes.p;
    a.n_nodes = (int32_t)r->recv.nodes.size();
    a.node_base = 1 + (int32_t)sc.nodes.size();
    a.level_nodes = r->d_recv_levels.p;
    a.level_start = r->d_recv_levels.p + r->recv_level_count;
    a.n_levels = r->recv_levels;
    a.root_ref = r->recv.root.ref;
    a.root_count = r->recv.root.count;
    a.grid = r->qgrid;
    a.tris = r->d_tris.p;
    a.cnodes = r->d_cnodes.p;
    a.qnodes = r->d_qnodes.p;
    a.flag = r->d_tree_flag.p;
    a.flag_value = r->tree_gen;
    return a;
}

arx_status arx::ensure_device_scene(arx_renderer* r) {
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    const bool writes = r->scene_dirty || r->recv_model_dirty || r->recv_pose_dirty || !r->qgrid_set;
    arx_status st;
    if (writes) {
        // the uploads, re-quantization and receiver refit below write the tree the other frame in
        // flight may still be tracing
        if ((st = fif_wait_traced(r)) != ARX_OK) return st;
        ++r->tree_gen;  // this write's off-grid flag value (arx_renderer::d_tree_flag)
    }
    const SceneImage& img = *r->scene_img;
    const BvhBuild& sc = img.bvh;
    SceneUpdate u{};
    u.model_changed = r->recv_model_dirty || r->scene_dirty;
    if (u.model_changed && (st = prepare_receiver_model(r)) != ARX_OK) return st;
    u.pose_changed = u.model_changed || r->recv_pose_dirty;
    const bool host_recv = !r->recv_refit;
    if (host_recv && u.pose_changed) place_host_receiver(r);
    u.n_nodes = 1 + sc.nodes.size() + r->recv.nodes.size();
    u.n_tris = sc.tris.size() + r->recv.tris.size();
    if ((st = check_buffer_offsets(u.n_nodes, u.n_tris)) != ARX_OK) return st;
    u.full = r->scene_dirty;
    if ((st = reserve_tree(r, u)) != ARX_OK) return st;
    update_grid(r, u);
    const bool top_changed = u.full || u.model_changed || (host_recv && u.pose_changed);
    if (top_changed && (st = upload_tree(r, u)) != ARX_OK) return st;
    if (u.regrid || top_changed) {
        // the quantized copy of the top node and the scene (and the host-built receiver) from the
        // coded nodes on the device; on the refit path the refit below writes the receiver's
        // quantized nodes itself (its coded ones may not exist yet)
        const size_t nq = host_recv ? u.n_nodes : 1 + sc.nodes.size();
        ARX_HIP(launch_requant16(r->d_cnodes.p, nq, r->qgrid, r->d_qnodes.p, r->d_tree_flag.p, r->tree_gen, r->stream));
        if (r->use_w4)
            ARX_HIP(launch_requant_w4(r->d_w4f.p, r->n_w4f, r->qgrid, r->d_wbuf.p, r->d_tree_flag.p, r->tree_gen, r->stream));
        ++r->requants;
    }
    r->q_valid = u.recv_empty || qgrid_contains(r->qgrid, u.rlo, u.rhi);
    if (r->recv_refit && (u.pose_changed || u.full || u.regrid) && (st = refit_receiver(r)) != ARX_OK) return st;
    r->scene_dirty = false;
    r->recv_model_dirty = false;
    r->recv_pose_dirty = false;
    if (writes && (st = fif_done_scene(r)) != ARX_OK) return st;  // the other frame set's next trace waits for these writes
    r->stats.n_scene_tris = img.n_input;
    r->stats.n_receiver_tris = (int64_t)r->recv.tris.size();
    r->stats.n_nodes = (int64_t)u.n_nodes;
    r->stats.bvh_depth = 1 + std::max(sc.depth, r->recv.depth);
    r->stats.tree_hash = img.hash;
    r->depth4 = r->use_w4 ? 1 + std::max(wide_of(r).w4.depth, r->recv4.depth) : 0;
    return ARX_OK;
}

arx_status arx::grow_grid_for(arx_renderer* r, const float ulo[3], const float uhi[3]) {
    const BvhBuild& sc = r->scene_img->bvh;
    ++r->tree_gen;
    r->qgrid = span_grid(r, ulo, uhi, true);
    ARX_HIP(launch_requant16(r->d_cnodes.p, 1 + sc.nodes.size(), r->qgrid, r->d_qnodes.p, r->d_tree_flag.p, r->tree_gen, r->stream));
    ++r->requants;
    r->recv_pose_dirty = true;
    return ARX_OK;
}

bool arx::widen_tree_arrays(arx_renderer* r, size_t need_nodes, size_t need_tris) {
    if (need_nodes <= r->nodes_cap() && need_tris <= r->d_tris.cap) return true;
    if (sync_renderer(r) != ARX_OK) return false;
    if (need_nodes > r->nodes_cap()) {
        BvhNode* cn = nullptr;
        QNode2* qn = nullptr;
        const size_t cap = need_nodes + 1024;
        if (hipMalloc(&cn, cap * sizeof(BvhNode)) != hipSuccess || hipMalloc(&qn, cap * sizeof(QNode2)) != hipSuccess ||
            hipMemcpy(cn, r->d_cnodes.p, r->d_cnodes.bytes(), hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(qn, r->d_qnodes.p, r->d_qnodes.bytes(), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(cn);
            hipFree(qn);
            return false;
        }
        r->d_cnodes.adopt(cn, cap);
        r->d_qnodes.adopt(qn, cap);
    }
    if (need_tris > r->d_tris.cap) {
        TriRec* tr = nullptr;
        const size_t cap = need_tris + 4096;
        if (hipMalloc(&tr, cap * sizeof(TriRec)) != hipSuccess ||
            hipMemcpy(tr, r->d_tris.p, r->d_tris.bytes(), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(tr);
            return false;
        }
        r->d_tris.adopt(tr, cap);
    }
    return true;
}

arx_status arx::set_scene_image(arx_renderer* r, SceneRef img) {
    const char* why = "";
    const BvhBuild& b = img->bvh;
    const arx_status fit = check_buffer_offsets(1 + b.nodes.size(), b.tris.size());
    if (fit != ARX_OK) return fit;
    if (!validate_bvh_range(b.nodes.data(), 1, b.nodes.size(), 1 + b.nodes.size(), b.tris.size(), &why))
        return fail(ARX_ERR_INTERNAL, "BVH validation failed (scene): %s", why);
    r->scene_img = std::move(img);
    ++r->scene_gen;
    r->scene_dirty = true;
    r->recv_model_dirty = true;  // receiver ids and offsets follow the scene
    r->bands.n_bands = 0;        // a band table belongs to the scene it was checked against
    return ARX_OK;
}

extern "C" {

arx_status arx_set_scene(arx_renderer* r, const float* tri_v, const float* tri_abs, int64_t n) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const arx_status st = check_scene_input(tri_v, tri_abs, n);
    if (st != ARX_OK) return st;
    SceneRef img = build_scene_image(tri_v, tri_abs, n);
    if (!img) return fail(ARX_ERR_OUT_OF_MEMORY, "scene build failed");
    return set_scene_image(r, std::move(img));
}

arx_status arx_set_receiver_model(arx_renderer* r, int side, const float* tri_v, int64_t n) {
    if (!r || side < 0 || side > 1 || n < 0 || (n > 0 && !tri_v))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad receiver model arguments");
    r->recv_local[side].assign(tri_v, tri_v + 9 * n);
    r->recv_model_dirty = true;
    return ARX_OK;
}

arx_status arx_place_receiver_vertices(const float* local_xyz, int64_t n_vertices, float x, float y, float z,
                                       float yaw_deg, float* out_xyz) {
    if (n_vertices < 0 || (n_vertices > 0 && (!local_xyz || !out_xyz)))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    place_vertices(local_xyz, n_vertices, x, y, z, yaw_deg, out_xyz);
    return ARX_OK;
}

arx_status arx_debug_node_images(arx_renderer* r, void* cnodes, void* qnodes, size_t n_nodes, float* grid,
                                 uint64_t* requants) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_nodes > (size_t)r->stats.n_nodes) return fail(ARX_ERR_INVALID_ARGUMENT, "only %lld nodes", (long long)r->stats.n_nodes);
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (cnodes && n_nodes) ARX_HIP(hipMemcpy(cnodes, r->d_cnodes.p, n_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (qnodes && n_nodes) ARX_HIP(hipMemcpy(qnodes, r->d_qnodes.p, n_nodes * sizeof(QNode2), hipMemcpyDeviceToHost));
    if (grid)
        for (int k = 0; k < 3; ++k) {
            grid[k] = r->qgrid.origin[k];
            grid[3 + k] = r->qgrid.scale[k];
        }
    if (requants) *requants = r->requants;
    return ARX_OK;
}

arx_status arx_debug_set_refit_pad(arx_renderer* r, float pad) {
    if (!r || !(pad >= 0.0f) || !std::isfinite(pad)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    r->debug_refit_pad = pad;
    r->recv_pose_dirty = true;  // the next trace refits with it
    return ARX_OK;
}

}  // extern "C"

