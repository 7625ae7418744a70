// arx_capi_trace.cpp -- one frame behind the C ABI (include/arx.h): the receiver model and the
// device scene, the trace launch, the IR's finalize and its room-acoustic analysis, and the arx_debug_*
// entry points of the trace.
//
// Host-side counterpart of R/prebuild/obj_raytracer/AudioRenderer.cpp (buildAccel, buildSBT, reload,
// render), re-designed for HIP: persistent device buffers, and no full rebuild when the listener moves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

#ifndef ARX_TRACE_PROF
#define ARX_TRACE_PROF 0  // measurement builds only (build.py --exp TAG -D ARX_TRACE_PROF=1)
#endif

float arx::initial_energy(const arx_config& c) {
    // devicePrograms.cu:208 -- (x*y*z) is an int product in the reference
    const int32_t n = c.rays_x * c.rays_y * c.rays_z;
    return (float)((double)c.base_power / ((double)n * 4.18879020478));
}

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

// Rotation of place_vertices (row-major r00 r10 r20 / r01 r11 r21 / r02 r12 r22), exactly its floats.
void receiver_rotation(float yaw_deg, float m[9]) {
    const float ang = yaw_deg * static_cast<float>(0.01745329251994329576923690768489);
    const float a = -ang, c = std::cos(a), s = std::sin(a), t1 = 1.0f - c;
    m[0] = c + 0.0f * 0.0f; m[1] = t1 * 0.0f - s * 0.0f; m[2] = 0.0f * 0.0f + s * 1.0f;
    m[3] = 0.0f * 1.0f + s * 0.0f; m[4] = c + t1 * 1.0f; m[5] = 0.0f * 1.0f - s * 0.0f;
    m[6] = 0.0f * 0.0f - s * 1.0f; m[7] = t1 * 0.0f + s * 0.0f; m[8] = c + 0.0f * 0.0f;
}

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
    hipFree(r->d_recv_local);
    hipFree(r->d_recv_nodes);
    hipFree(r->d_recv_levels);
    r->d_recv_local = nullptr;
    r->d_recv_nodes = nullptr;
    r->d_recv_levels = nullptr;
    ARX_HIP(hipMalloc(&r->d_recv_local, std::max<size_t>(1, r->recv.tris.size()) * sizeof(TriRec)));
    ARX_HIP(hipMalloc(&r->d_recv_nodes, std::max<size_t>(1, r->recv.nodes.size()) * sizeof(BvhNode)));
    ARX_HIP(hipMalloc(&r->d_recv_levels, (order.size() + start.size()) * sizeof(int32_t)));
    if (!r->recv.tris.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_local, r->recv.tris.data(), r->recv.tris.size() * sizeof(TriRec),
                               hipMemcpyHostToDevice, r->stream));
    if (!r->recv.nodes.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_nodes, r->recv.nodes.data(), r->recv.nodes.size() * sizeof(BvhNode),
                               hipMemcpyHostToDevice, r->stream));
    std::vector<int32_t> lv(order);
    lv.insert(lv.end(), start.begin(), start.end());
    ARX_HIP(hipMemcpyAsync(r->d_recv_levels, lv.data(), lv.size() * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
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
    hipFree(r->d_recv_w4);
    hipFree(r->d_recv_w4_tris);
    r->d_recv_w4 = nullptr;
    r->d_recv_w4_tris = nullptr;
    ARX_HIP(hipMalloc(&r->d_recv_w4, std::max<size_t>(1, w4n.size()) * sizeof(int32_t)));
    ARX_HIP(hipMalloc(&r->d_recv_w4_tris, std::max<size_t>(1, w4t.size()) * sizeof(int32_t)));
    if (!w4n.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_w4, w4n.data(), w4n.size() * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    if (!w4t.empty())
        ARX_HIP(hipMemcpyAsync(r->d_recv_w4_tris, w4t.data(), w4t.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                               r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));  // pageable sources
    return ARX_OK;
}

// Box padding of the refit kernel (RefitArgs::pad): at least the builder's 1e-5 * max|coordinate|
// for any vertex of the placed receiver (|v| <= |center| + radius).
float refit_pad(const arx_renderer* r) {
    float mx = 0.0f;
    for (int k = 0; k < 3; ++k) mx = std::max(mx, std::fabs(r->center[k]));
    return std::max(1e-5f * (mx + r->recv_radius) * 1.001f, 1e-6f);
}

// World-space bound of the placed receiver (for the quantization grid): the refit path's ball
// widened by the refit kernel's box padding (the padded boxes it quantizes must stay on the grid),
// or the host-built sub-tree's root box.
void receiver_bound(const arx_renderer* r, float lo[3], float hi[3], bool* empty) {
    *empty = (r->recv_local[0].size() + r->recv_local[1].size()) == 0;
    const float pad = r->recv_refit ? refit_pad(r) : 0.0f;
    for (int k = 0; k < 3; ++k) {
        if (r->recv_refit) {
            lo[k] = r->center[k] - r->recv_radius - 2.0f * pad;
            hi[k] = r->center[k] + r->recv_radius + 2.0f * pad;
        } else {
            lo[k] = r->recv.root.lo[k];
            hi[k] = r->recv.root.hi[k];
        }
    }
}

arx_status ensure_device_scene(arx_renderer* r) {
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    const bool writes = r->scene_dirty || r->recv_model_dirty || r->recv_pose_dirty || !r->qgrid_set;
    if (writes) {
        // the uploads, re-quantization and receiver refit below write the tree the other frame in
        // flight may still be tracing
        const arx_status st = fif_wait_traced(r);
        if (st != ARX_OK) return st;
        ++r->tree_gen;  // this write's off-grid flag value (arx_renderer::d_tree_flag)
    }
    const SceneImage& img = *r->scene_img;
    const BvhBuild& sc = img.bvh;
    const bool model_changed = r->recv_model_dirty || r->scene_dirty;
    if (model_changed) {
        arx_status st = prepare_receiver_model(r);
        if (st != ARX_OK) return st;
    }
    const bool pose_changed = model_changed || r->recv_pose_dirty;
    if (!r->recv_refit && pose_changed) {
        // host path (receivers beyond the refit kernel's capacity): receiver halves placed in world
        // space, left then right (placeReceiver OptixModel.cpp:153-157), sub-tree rebuilt
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
    const size_t n_nodes = 1 + sc.nodes.size() + r->recv.nodes.size();
    const size_t n_tris = sc.tris.size() + r->recv.tris.size();
    arx_status fit = check_buffer_offsets(n_nodes, n_tris);
    if (fit != ARX_OK) return fit;
    bool full = r->scene_dirty;
    if (n_nodes > r->nodes_cap) {
        if (r->d_cnodes) ARX_HIP(hipFree(r->d_cnodes));
        if (r->d_qnodes) ARX_HIP(hipFree(r->d_qnodes));
        r->d_cnodes = nullptr;
        r->d_qnodes = nullptr;
        size_t cap = n_nodes + 1024;
        ARX_HIP(hipMalloc(&r->d_cnodes, cap * sizeof(BvhNode)));
        ARX_HIP(hipMalloc(&r->d_qnodes, cap * sizeof(QNode2)));
        r->nodes_cap = cap;
        full = true;
    }
    if (n_tris > r->tris_cap || r->d_tris == nullptr) {
        if (r->d_tris) ARX_HIP(hipFree(r->d_tris));
        r->d_tris = nullptr;
        size_t cap = std::max<size_t>(n_tris + 4096, 1);
        ARX_HIP(hipMalloc(&r->d_tris, cap * sizeof(TriRec)));
        r->tris_cap = cap;
        full = true;
    }
    // CW4 (opt-in, use_w4 only): the buffer holds the scene's units, then the receiver's; the f32
    // records are the top node, the scene's nodes and (host-built receivers) the receiver's
    static const SceneImage::Wide kNoWide;
    const SceneImage::Wide& wide = r->use_w4 ? img.wide() : kNoWide;
    const size_t w_units = r->use_w4 ? std::max<size_t>(r->recv4.unit_end, wide.w4.unit_end) : 0;
    const size_t host_recv_w4 = (r->recv_refit || !r->use_w4) ? 0 : r->recv4.nodes.size();
    const size_t n_w4f = r->use_w4 ? 1 + wide.w4.nodes.size() + host_recv_w4 : 0;
    if (w_units > r->wbuf_cap) {
        if (r->d_wbuf) ARX_HIP(hipFree(r->d_wbuf));
        r->d_wbuf = nullptr;
        const size_t cap = w_units + 4096;
        ARX_HIP(hipMalloc(&r->d_wbuf, cap * 16));
        r->wbuf_cap = cap;
        full = true;
    }
    if (n_w4f > r->w4f_cap) {
        if (r->d_w4f) ARX_HIP(hipFree(r->d_w4f));
        r->d_w4f = nullptr;
        const size_t cap = n_w4f + 1024;
        ARX_HIP(hipMalloc(&r->d_w4f, cap * sizeof(W4NodeF)));
        r->w4f_cap = cap;
        full = true;
    }
    r->n_w4f = n_w4f;
    // The quantization grid: made when the scene changes, grown when the receiver leaves it (a
    // listener walking out of the room): the new grid spans the old one, the scene, the receiver
    // and the emitter with half the extent as margin, so such a walk re-grids once or twice, not
    // per frame.  Either way the quantized copy is re-made on the device from the coded nodes
    // (launch_requant16): no host quantization, no upload, no synchronisation inside a frame.  An
    // emitter off the grid (checked per launch, arx_trace_rays) makes that launch take the f32 nodes.
    float rlo[3], rhi[3];
    bool recv_empty = false;
    receiver_bound(r, rlo, rhi, &recv_empty);
    const bool grow = !full && r->qgrid_set && pose_changed && !recv_empty && !qgrid_contains(r->qgrid, rlo, rhi);
    const bool regrid = full || !r->qgrid_set || grow;
    if (regrid) {
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) {
            lo[k] = hi[k] = r->emitter[k];
            if (sc.root.count >= 0) {
                lo[k] = std::min(lo[k], sc.root.lo[k]);
                hi[k] = std::max(hi[k], sc.root.hi[k]);
            }
            if (!recv_empty) {
                lo[k] = std::min(lo[k], rlo[k]);
                hi[k] = std::max(hi[k], rhi[k]);
            }
            if (grow) {
                lo[k] = std::min(lo[k], r->qgrid.origin[k]);
                hi[k] = std::max(hi[k], r->qgrid.origin[k] + 65000.0f * r->qgrid.scale[k]);
            }
        }
        r->qgrid = make_qgrid(lo, hi, grow ? 0.5 : 0.1);
        r->qgrid_set = true;
    }
    const bool host_recv = !r->recv_refit;
    const bool top_changed = full || model_changed || (host_recv && pose_changed);
    if (full || top_changed) {
        // host uploads, only when the scene or the receiver model changed, or on the host-receiver
        // path: the top node (its receiver child comes from the refit kernel on the refit path),
        // the scene's coded nodes and triangles, the receiver part on the host path
        BvhNode top = make_node(sc.root, host_recv ? r->recv.root : empty_child());
        const char* why = "";
        if ((host_recv && !validate_bvh_range(r->recv.nodes.data(), 1 + sc.nodes.size(), r->recv.nodes.size(), n_nodes,
                                              n_tris, &why)) ||
            !validate_bvh_range(&top, 0, 1, n_nodes, n_tris, &why))
            return fail(ARX_ERR_INTERNAL, "BVH validation failed: %s", why);
        BvhNode ctop;  // pageable sources below live until the synchronisation at the end of this block
        code_nodes(&top, 1, &ctop);
        std::vector<BvhNode> crecv(host_recv ? r->recv.nodes.size() : 0);
        if (host_recv) code_nodes(r->recv.nodes.data(), r->recv.nodes.size(), crecv.data());
        ARX_HIP(hipMemcpyAsync(r->d_cnodes, &ctop, sizeof(BvhNode), hipMemcpyHostToDevice, r->stream));
        if (full && !img.coded.empty())
            ARX_HIP(hipMemcpyAsync(r->d_cnodes + 1, img.coded.data(), img.coded.size() * sizeof(BvhNode),
                                   hipMemcpyHostToDevice, r->stream));
        if (full && !sc.tris.empty())
            ARX_HIP(hipMemcpyAsync(r->d_tris, sc.tris.data(), sc.tris.size() * sizeof(TriRec), hipMemcpyHostToDevice,
                                   r->stream));
        if (host_recv && !crecv.empty())
            ARX_HIP(hipMemcpyAsync(r->d_cnodes + 1 + sc.nodes.size(), crecv.data(), crecv.size() * sizeof(BvhNode),
                                   hipMemcpyHostToDevice, r->stream));
        if (host_recv && !r->recv.tris.empty())
            ARX_HIP(hipMemcpyAsync(r->d_tris + sc.tris.size(), r->recv.tris.data(), r->recv.tris.size() * sizeof(TriRec),
                                   hipMemcpyHostToDevice, r->stream));
        // CW4 (opt-in): the scene's buffer image and node records once per scene; the top node's
        // record (child 0 the scene root, child 1 the host-built receiver's root or, on the refit
        // path, a placeholder the refit kernel replaces); a host-built receiver's records and triangles
        std::vector<uint32_t> rimage;
        if (r->use_w4) {
            W4NodeF wtop;
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
            ARX_HIP(hipMemcpyAsync(r->d_w4f, &wtop, sizeof(W4NodeF), hipMemcpyHostToDevice, r->stream));
            if (full && !wide.wimage.empty())
                ARX_HIP(hipMemcpyAsync(r->d_wbuf, wide.wimage.data(), wide.wimage.size() * sizeof(uint32_t),
                                       hipMemcpyHostToDevice, r->stream));
            if (full && !wide.w4.nodes.empty())
                ARX_HIP(hipMemcpyAsync(r->d_w4f + 1, wide.w4.nodes.data(), wide.w4.nodes.size() * sizeof(W4NodeF),
                                       hipMemcpyHostToDevice, r->stream));
            if (host_recv) {
                if (!r->recv4.nodes.empty())
                    ARX_HIP(hipMemcpyAsync(r->d_w4f + 1 + wide.w4.nodes.size(), r->recv4.nodes.data(),
                                           r->recv4.nodes.size() * sizeof(W4NodeF), hipMemcpyHostToDevice, r->stream));
                const size_t u0 = wide.w4.unit_end;
                rimage.assign((r->recv4.unit_end - u0) * 4, 0u);
                for (const auto& lt : r->recv4.leaf_tris)
                    std::memcpy(rimage.data() + (size_t)(lt.first - u0) * 4, &r->recv.tris[(size_t)lt.second], sizeof(TriRec));
                if (!rimage.empty())
                    ARX_HIP(hipMemcpyAsync(r->d_wbuf + u0, rimage.data(), rimage.size() * sizeof(uint32_t),
                                           hipMemcpyHostToDevice, r->stream));
            }
        }
        ARX_HIP(hipStreamSynchronize(r->stream));
    }
    if (regrid || top_changed) {
        // the quantized copy of the top node and the scene (and the host-built receiver) from the
        // coded nodes on the device; on the refit path the refit below writes the receiver's
        // quantized nodes itself (its coded ones may not exist yet)
        const size_t nq = host_recv ? n_nodes : 1 + sc.nodes.size();
        ARX_HIP(launch_requant16(r->d_cnodes, nq, r->qgrid, r->d_qnodes, r->d_tree_flag, r->tree_gen, r->stream));
        if (r->use_w4)
            ARX_HIP(launch_requant_w4(r->d_w4f, r->n_w4f, r->qgrid, r->d_wbuf, r->d_tree_flag, r->tree_gen, r->stream));
        ++r->requants;
    }
    r->q_valid = recv_empty || qgrid_contains(r->qgrid, rlo, rhi);
    if (r->recv_refit && (pose_changed || full || regrid)) {
        // the listener move itself: one kernel, no host copies, no synchronisation
        RefitArgs a;
        std::memset(&a, 0, sizeof(a));
        a.local_tris = r->d_recv_local;
        a.n_tris = (int32_t)r->recv.tris.size();
        a.tri_base = (int32_t)sc.tris.size();
        a.local_nodes = r->d_recv_nodes;
        a.n_nodes = (int32_t)r->recv.nodes.size();
        a.node_base = 1 + (int32_t)sc.nodes.size();
        a.level_nodes = r->d_recv_levels;
        a.level_start = r->d_recv_levels + r->recv_level_count;
        a.n_levels = r->recv_levels;
        a.root_ref = r->recv.root.ref;
        a.root_count = r->recv.root.count;
        receiver_rotation(r->yaw, a.m);
        for (int k = 0; k < 3; ++k) a.t[k] = r->center[k];
        // >= the builder's pad; receiver_bound covers it (a debug pad does not: the off-grid test)
        a.pad = r->debug_refit_pad > 0.0f ? r->debug_refit_pad : refit_pad(r);
        a.grid = r->qgrid;
        a.tris = r->d_tris;
        a.cnodes = r->d_cnodes;
        a.qnodes = r->q_valid ? r->d_qnodes : nullptr;
        a.flag = r->d_tree_flag;
        a.flag_value = r->tree_gen;
        if (r->q_valid && r->use_w4) {  // the opt-in CW4 copy follows the quantized one (same grid)
            a.wbuf = r->d_wbuf;
            a.w4_nodes = r->d_recv_w4;
            a.n_w4 = (int32_t)r->recv4.nodes.size();
            a.w4_tris = r->d_recv_w4_tris;
            a.n_w4_tris = (int32_t)r->recv4.leaf_tris.size();
            a.scene_nonempty = sc.root.count >= 0 ? 1 : 0;
            for (int k = 0; k < 3; ++k) {
                a.scene_lo[k] = sc.root.lo[k];
                a.scene_hi[k] = sc.root.hi[k];
            }
        }
        if (a.n_tris > 0) ARX_HIP(launch_receiver_refit(a, r->stream));
    }
    r->scene_dirty = false;
    r->recv_model_dirty = false;
    r->recv_pose_dirty = false;
    if (writes) {  // the other frame set's next trace waits for these writes
        const arx_status st = fif_done_scene(r);
        if (st != ARX_OK) return st;
    }
    r->stats.n_scene_tris = img.n_input;
    r->stats.n_receiver_tris = (int64_t)r->recv.tris.size();
    r->stats.n_nodes = (int64_t)n_nodes;
    r->stats.bvh_depth = 1 + std::max(sc.depth, r->recv.depth);
    r->stats.tree_hash = img.hash;
    r->depth4 = r->use_w4 ? 1 + std::max(wide.w4.depth, r->recv4.depth) : 0;
    return ARX_OK;
}

static_assert(kPathFrames == arx_renderer::kMaxFrames, "one last-replay event per frame set");

// The path cache's buffers for a recording of n rays and `need` bytes of records: made at the first
// recording and kept across keys; a buffer that must grow is freed once every frame set's stream is
// idle (a replay of the key before may still read it).  *fits false: the device has no room for them (the
// cache is optional: the caller traces the launch instead); what was freed stays freed.
arx_status path_cache_reserve(arx_renderer* r, uint64_t n, uint64_t need, bool* fits) {
    PathCache& pc = r->path_cache;
    *fits = true;
    auto room = [&](void** p, size_t bytes) {  // true: allocated; false: out of memory (error cleared)
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            *p = nullptr;
            *fits = false;
        }
        return e;
    };
    if (!pc.ev_recorded) ARX_HIP(hipEventCreateWithFlags(&pc.ev_recorded, hipEventDisableTiming));
    for (hipEvent_t& e : pc.ev_replayed)
        if (!e) ARX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!pc.d_scratch) ARX_HIP(hipMalloc(&pc.d_scratch, (kCursor + 1) * sizeof(unsigned long long)));
    if (!pc.h_scratch) ARX_HIP(hipHostMalloc(&pc.h_scratch, kCounters * sizeof(unsigned long long), hipHostMallocDefault));
    if (n <= pc.dirs_cap && need <= pc.cap_bytes) return ARX_OK;
    const arx_status st = sync_renderer(r);
    if (st != ARX_OK) return st;
    if (n > pc.dirs_cap) {
        hipFree(pc.d_dirs);
        pc.d_dirs = nullptr;
        pc.dirs_cap = 0;
        if (const hipError_t e = room(&pc.d_dirs, n * 16); e == hipErrorOutOfMemory) return ARX_OK;
        else ARX_HIP(e);
        pc.dirs_cap = n;
    }
    if (need > pc.cap_bytes) {
        hipFree(pc.d_hits);
        pc.d_hits = nullptr;
        pc.cap_bytes = 0;
        if (const hipError_t e = room(&pc.d_hits, need); e == hipErrorOutOfMemory) return ARX_OK;
        else ARX_HIP(e);
        pc.cap_bytes = need;
    }
    return ARX_OK;
}

// The path filter's planes for a recording of n rays (outside the cap, optional).  False: no room on the
// device (the error cleared; that size is not tried again), and the launch records and replays
// unfiltered.  Called behind path_cache_reserve: a buffer that must grow is freed with every stream idle.
bool path_filter_reserve(arx_renderer* r, uint64_t n, uint32_t max_bounces) {
    PathCache& pc = r->path_cache;
    const uint64_t need = path_filter_plane_bytes(n, max_bounces);
    if (need <= pc.filter_cap) return true;
    if (pc.filter_no_room > 0 && need >= pc.filter_no_room) return false;
    if (sync_renderer(r) != ARX_OK) return false;
    hipFree(pc.d_filter);
    pc.d_filter = nullptr;
    pc.filter_cap = 0;
    if (hipMalloc(&pc.d_filter, need) != hipSuccess) {
        (void)hipGetLastError();
        pc.d_filter = nullptr;
        pc.filter_no_room = need;
        return false;
    }
    pc.filter_cap = need;
    return true;
}

// The current frame set's candidate list for n rays; false as above (the frame replays unfiltered).
bool path_filter_list_reserve(arx_renderer* r, uint64_t n) {
    PathCache& pc = r->path_cache;
    arx_renderer::FrameSet& f = r->cur();
    if (n <= f.filter_list_cap) return true;
    const uint64_t need = path_filter_list_bytes(n);
    if (pc.filter_list_no_room > 0 && need >= pc.filter_list_no_room) return false;
    if (f.d_filter_list) {  // an earlier replay on this set's stream may still write it
        if (hipStreamSynchronize(f.stream) != hipSuccess) return false;
        hipFree(f.d_filter_list);
    }
    f.d_filter_list = nullptr;
    f.filter_list_cap = 0;
    if (hipMalloc(&f.d_filter_list, need) != hipSuccess) {
        (void)hipGetLastError();
        f.d_filter_list = nullptr;
        pc.filter_list_no_room = need;
        return false;
    }
    f.filter_list_cap = n;
    return true;
}

// The filter's margin (filter_kernel): kFilterMargin plus the slab test's own slack, 2^-18 of the
// largest coordinate magnitude the grid spans (scene, emitter and receiver lie on it).
float path_filter_grow(const QGrid& g) {
    float m = 0.0f;
    for (int k = 0; k < 3; ++k)
        m = std::max(m, std::max(std::fabs(g.origin[k]), std::fabs(g.origin[k] + 65536.0f * g.scale[k])));
    return kFilterMargin + std::ldexp(m, -18);
}

}  // namespace

void arx::free_path_cache(PathCache& p) {
    hipFree(p.d_dirs);
    hipFree(p.d_hits);
    hipFree(p.d_filter);
    hipFree(p.d_scratch);
    if (p.h_scratch) hipHostFree(p.h_scratch);
    if (p.ev_recorded) hipEventDestroy(p.ev_recorded);
    for (hipEvent_t e : p.ev_replayed)
        if (e) hipEventDestroy(e);
    const int32_t mode = p.mode, filter_on = p.filter_on;
    const uint64_t max_bytes = p.max_bytes;
    p = PathCache{};
    p.mode = mode;
    p.filter_on = filter_on;
    p.max_bytes = max_bytes;
    p.state = mode == 1 ? kPathTraced : kPathOff;
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

arx_status arx::trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end, bool timed, bool clear,
                           ReplayProbe* probe) {
    if (probe) probe->ready = probe->recorded = false;
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (ray_end < ray_begin) return fail(ARX_ERR_INVALID_ARGUMENT, "ray_end < ray_begin");
    // global ray ids index the launch of N = x*y*z rays: energies are normalised by N and the
    // int64 fixed point's headroom (arx_frac_bits) assumes at most N rays per histogram
    if (ray_end > n_rays(r->cfg))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ray_end %llu exceeds the launch's %llu rays", (unsigned long long)ray_end,
                    (unsigned long long)n_rays(r->cfg));
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = ensure_device_scene(r);
    if (st != ARX_OK) return st;
    arx_renderer::FrameSet& f = r->cur();
    const arx_config& c = r->cfg;
    TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cnodes = r->d_cnodes;
    // quantized nodes only while the emitter (the one ray origin off the geometry) is on the
    // grid: the slab arithmetic's error bound assumes origins within the grid's extent
    const float* em = r->emitter;
    a.qnodes = (r->q_valid && !r->force_f32_nodes && qgrid_contains(r->qgrid, em, em)) ? r->d_qnodes : nullptr;
    // the CW4 tree on the same condition when asked for (arx_debug_set_trace_path bit 3; measured
    // 1.9x slower than the BVH2 on C3: DESIGN.md section 6.3)
    a.wbuf = (a.qnodes && r->use_w4 && !r->force_global_stack) ? r->d_wbuf : nullptr;
    a.qgrid = r->qgrid;
    a.tris = r->d_tris;
    a.hist = r->hist();
    a.counters = f.d_counters;
    a.cursor = f.d_counters + kCursor;
    a.seed = c.seed;
    a.ray_begin = ray_begin;
    a.ray_end = ray_end;
    for (int k = 0; k < 3; ++k) {
        a.emitter[k] = r->emitter[k];
        a.center[k] = r->center[k];
    }
    a.e0 = initial_energy(c);
    a.inv_unit = (a.e0 != 0.0f) ? std::ldexp(1.0, arx_frac_bits(n_rays(c))) / (double)a.e0 : 0.0;
    a.energy_thres = c.energy_thres;
    a.hrtf = c.hrtf_absorption_rate;
    int32_t secs = r->ir_len / c.sample_rate;  // devicePrograms.cu:227-228
    secs = std::max(1, std::min(secs, 999));
    a.dist_limit = (float)(secs * kSpeedOfSound + 1);
    a.max_bounces = c.max_bounces;
    a.sample_rate = c.sample_rate;
    a.ir_len = r->ir_len;
    a.delay = (int32_t)((double)c.sample_rate * 0.00044);  // devicePrograms.cu:125
    a.is_mono = c.is_mono;
    a.bvh_depth = r->stats.bvh_depth;
    if (clear) {
        a.clear_bins = 2 * (uint64_t)r->ir_len;
        a.clear_counters = kCounters;
    }
    if (ray_end == ray_begin) {  // nothing to trace: the clear alone
        if (probe) return ARX_OK;
        if (clear) ARX_HIP(launch_clear(r->hist(), 2 * (uint64_t)r->ir_len, f.d_counters, (int)kCounters, r->stream));
        return ARX_OK;
    }
    const uint64_t n_launch = ray_end - ray_begin;
    if (n_launch > f.dirs_cap) {  // direction pre-pass buffer; what the old one held is forgotten
        if (f.d_dirs) ARX_HIP(hipFree(f.d_dirs));
        f.d_dirs = nullptr;
        f.dirs_cap = 0;
        f.dirs_valid = f.dirs_sorted = false;
        ARX_HIP(hipMalloc(&f.d_dirs, n_launch * 16));
        f.dirs_cap = n_launch;
    }
    const bool gstack = r->force_global_stack || a.bvh_depth + 1 > kLdsStack;
    // CW4: up to three pushes per level; the rows beyond the LDS rows overflow into a global column
    const size_t w4_rows = (size_t)std::max(1, 3 * r->depth4 + 3 - kLdsStack);
    if (gstack || a.wbuf) {  // trees deeper than the LDS stack: one global column of bvh_depth + 1 entries per lane
        const size_t lanes = trace_max_lanes(r->cus);
        const size_t need = (a.wbuf ? w4_rows : (size_t)(a.bvh_depth + 1)) * lanes;
        if (need > r->gstack_cap) {
            if (r->d_gstack) ARX_HIP(hipFree(r->d_gstack));
            r->d_gstack = nullptr;
            r->gstack_cap = 0;
            ARX_HIP(hipMalloc(&r->d_gstack, need * sizeof(int32_t)));
            r->gstack_cap = need;
        }
        a.gstack = r->d_gstack;
        a.gstack_lanes = lanes;
        // one global stack per renderer: with frames in flight, after the other frames' traces
        if (const arx_status w = fif_wait_traced(r); w != ARX_OK) return w;
    }
#if ARX_TRACE_PROF  // measurement builds only: per-wave records (arx_debug_trace_profile)
    {
        const size_t words = (size_t)r->cus * 64 * kProfWords;  // >= waves of any trace grid
        if (!r->d_prof) {
            ARX_HIP(hipMalloc(&r->d_prof, words * sizeof(unsigned long long)));
            r->prof_words = words;
        }
        ARX_HIP(hipMemsetAsync(r->d_prof, 0, words * sizeof(unsigned long long), r->stream));
        a.prof = r->d_prof;
    }
#endif
    // frames in flight: after the other frame set's last writes to the tree (its refit, re-gridding
    // or upload), which this launch reads
    if (const arx_status w = fif_wait_scene(r); w != ARX_OK) return w;
    const int fmt = a.wbuf ? kFmtW4 : (a.qnodes ? kFmtQ16 : kFmtF32);
    // the instance launch_trace takes (ray pool or small launch): the profile guard reads these
    const int small = trace_uses_small_block(a, r->cus, r->force_global_stack) ? 1 : 0;
    // The direction buffer across launches (arx_debug_set_ray_order, include/arx.h).  Kept while seed
    // and ray range stay (every launch kind); for launches that take the pool on the 16-bit LDS-stack
    // instance, the pool's slots ordered longest first: the first launch of a key runs the measuring
    // instance on directions in ray order and the sort follows it on the same stream into the set's
    // second buffer; the launches after it run the product instance on that buffer as long as the key
    // holds.  Per frame set: its own stream and buffers, nothing new crosses streams.
    // (a caller's other stream, arx_set_stream, is not ordered after the launch that wrote them: re-made)
    const bool kept = r->ray_order != 2 && f.dirs_valid && f.dirs_stream == r->stream && f.dirs_seed == c.seed &&
                      f.dirs_begin == ray_begin && f.dirs_count == n_launch;
    const bool ordered = r->ray_order == 1 && trace_can_measure(a, r->cus, r->force_global_stack);
    OrderKey key;
    std::memset(&key, 0, sizeof(key));
    if (ordered) {
        key.scene_gen = r->scene_gen;
        key.tree_hash = r->stats.tree_hash;
        key.seed = c.seed;
        key.ray_begin = ray_begin;
        key.ray_end = ray_end;
        for (int k = 0; k < 3; ++k) key.emitter[k] = r->emitter[k];
        key.e0 = a.e0;
        key.energy_thres = a.energy_thres;
        key.hrtf = a.hrtf;
        key.dist_limit = a.dist_limit;
        key.max_bounces = a.max_bounces;
        key.dyn_share = trace_pool_share();
        key.is_mono = a.is_mono;
        key.instance = fmt;
    }
    const bool use_sorted = ordered && kept && f.dirs_sorted && std::memcmp(&key, &f.order_key, sizeof(key)) == 0;
    const bool measure = ordered && !use_sorted;
    const bool fill_dirs = !use_sorted && !(kept && !f.dirs_sorted);
    if (measure && f.order_cap != f.dirs_cap) {  // the two buffers swap: always the same size
        hipFree(f.d_dirs_alt);
        hipFree(f.d_cost);
        f.d_dirs_alt = nullptr;
        f.d_cost = nullptr;
        f.order_cap = 0;
        ARX_HIP(hipMalloc(&f.d_dirs_alt, f.dirs_cap * 16));
        ARX_HIP(hipMalloc(&f.d_cost, f.dirs_cap * sizeof(unsigned short)));
        if (!f.d_order_bins) ARX_HIP(hipMalloc(&f.d_order_bins, order_bins_bytes()));
        f.order_cap = f.dirs_cap;
    }
    a.dirs = f.d_dirs;
    a.cost = measure ? f.d_cost : nullptr;
    const int inst = measure ? kInstMeasure : (small ? kInstSmall : kInstPool);
    r->stats.trace_format = fmt;
    r->stats.trace_vgprs = r->occ[fmt][inst][0];
    r->stats.trace_waves_per_simd = r->occ[fmt][inst][1];
    r->stats.trace_waves_target = r->occ[fmt][inst][2];
    if (timed && !probe && (st = r->trace_ring.begin(r->stream)) != ARX_OK) return st;
    // Frames in flight: a ray-pool launch is sized for half the CUs' wave slots, so the next frame's
    // launch runs beside it for its whole length instead of only in its tail.  A launch of 1M rays
    // gives each lane about three rays; the last of them leave the lanes idle one by one, and a wave
    // holds its slot until its last lane is done (C3 on the full grid: 5.87e9 queries/s at 1M rays
    // against 7.23e9 at 10M).  Two half grids side by side: C3 2.60 -> 2.44 ms per frame (DESIGN.md
    // section 6.3, profiles/r06/grid_ab_*.txt); more than half each makes a launch's last blocks wait
    // for the other's (55 %: 2.9 ms).  One frame in flight keeps the full grid, and so do the traces
    // on the renderer's one global stack (deep trees, CW4): they wait for every other frame's trace
    // above, so they never run beside one.
#ifndef ARX_SHARED_GRID_PCT
#define ARX_SHARED_GRID_PCT 50  // design experiments only (build.py --exp): other shares
#endif
    const bool shared_grid = r->fif >= 2 && !small && !gstack && !a.wbuf;
    const int grid_cus = shared_grid ? std::max(1, r->cus * ARX_SHARED_GRID_PCT / 100) : r->cus;
    r->stats.trace_grid_cus = grid_cus;
    // The path cache (arx_debug_set_path_cache, include/arx.h).  A launch whose key equals the previous
    // launch's, on a direction buffer in its final state (one this launch would neither fill nor
    // measure), records the scene-only hits and replays them; the launches of that key after it only
    // replay.  Everything else is traced as above and costs what it did.
    PathCache& pc = r->path_cache;
    // a probe decides what this launch would do and leaves what the last launch did as it was
    const OrderKey probe_last_key = pc.last_key;
    const bool probe_last_valid = pc.last_valid, probe_last_filtered = pc.last_filtered;
    const int32_t probe_state = pc.state;
    pc.last_filtered = false;
    const bool cacheable = pc.mode == 1 && r->stream == f.stream && trace_can_cache(a, r->force_global_stack);
    bool replay = false, record = false;
    if (pc.mode != 1) {
        pc.state = kPathOff;
        pc.recorded = pc.last_valid = false;
    } else if (!cacheable) {
        pc.state = kPathNotCacheable;
        pc.recorded = pc.last_valid = false;
    } else {
        OrderKey pk = key;
        if (!ordered) {
            pk.scene_gen = r->scene_gen;
            pk.tree_hash = r->stats.tree_hash;
            pk.seed = c.seed;
            pk.ray_begin = ray_begin;
            pk.ray_end = ray_end;
            for (int k = 0; k < 3; ++k) pk.emitter[k] = r->emitter[k];
            pk.e0 = a.e0;
            pk.energy_thres = a.energy_thres;
            pk.hrtf = a.hrtf;
            pk.dist_limit = a.dist_limit;
            pk.max_bounces = a.max_bounces;
            pk.is_mono = a.is_mono;
        }
        pk.dyn_share = 0;  // the cache carries its own directions: neither shapes a ray's path
        pk.instance = 0;
        const bool repeated = pc.last_valid && std::memcmp(&pk, &pc.last_key, sizeof(pk)) == 0;
        if (pc.recorded && std::memcmp(&pk, &pc.key, sizeof(pk)) != 0) pc.recorded = false;
        pc.last_key = pk;
        pc.last_valid = true;
        pc.state = kPathTraced;
        const bool final_dirs = !fill_dirs && !measure;
        const uint64_t need = arx_debug_path_cache_bytes(n_launch, a.max_bounces);
        if (need > pc.max_bytes || (pc.no_room > 0 && need >= pc.no_room)) {  // over the cap, or known not to fit
            pc.state = kPathOverCap;
            pc.recorded = false;
        } else if (final_dirs && pc.recorded) {
            replay = true;
        } else if (final_dirs && repeated) {
            record = replay = true;
        }
        if (record && !probe) {
            bool fits = true;
            if ((st = path_cache_reserve(r, n_launch, need, &fits)) != ARX_OK) return st;
            if (fits) {
                pc.key = pk;
            } else {  // no room on the device for an optional cache: this launch is traced like an over-cap one
                record = replay = false;
                pc.state = kPathOverCap;
                pc.no_room = need;  // not tried again per frame (arx_debug_set_path_cache forgets it)
            }
        }
    }
    if (probe) {
        probe->recorded = replay && !record && pc.rec_stream == r->stream;
        probe->ready = probe->recorded && pc.filter_on && pc.has_state && pc.d_filter;
        probe->state = pc.state;
        probe->args = a;
        probe->args.dirs = pc.d_dirs;
        probe->args.rec = pc.d_hits;
        probe->planes = pc.d_filter;
        pc.last_key = probe_last_key;
        pc.last_valid = probe_last_valid;
        pc.last_filtered = probe_last_filtered;
        pc.state = probe_state;
        return ARX_OK;
    }
    if (replay) {
        TraceArgs pa = a;
        pa.dirs = pc.d_dirs;
        pa.rec = pc.d_hits;
        if (record) {
            // the cache may still be read by the other sets' replays of the key before
            for (int k = 0; k < r->fif; ++k)
                if (pc.replayed[k] && k != r->slot) ARX_HIP(hipStreamWaitEvent(r->stream, pc.ev_replayed[k], 0));
            for (bool& b : pc.replayed) b = false;
            ARX_HIP(hipMemcpyAsync(pc.d_dirs, f.d_dirs, n_launch * 16, hipMemcpyDeviceToDevice, r->stream));
            TraceArgs ra = pa;
            ra.hist = nullptr;
            ra.counters = pc.d_scratch;
            ra.cursor = pc.d_scratch + kCursor;
            ra.clear_bins = 0;
            ra.clear_counters = kCounters;
            // with the filter on, what every query starts from as well (outside the cap; without room
            // for it, records alone as before)
            pc.has_state = pc.filter_on && a.max_bounces >= 1 && a.max_bounces <= kFilterMaxBounces &&
                           path_filter_reserve(r, n_launch, a.max_bounces);
            ra.gstack = pc.has_state ? static_cast<int32_t*>(pc.d_filter) : nullptr;
            ARX_HIP(launch_path_record(ra, grid_cus, r->stream));
            pc.recorded = true;
            pc.bytes = kPathRecordBytes * (uint64_t)a.max_bounces * n_launch;
            pc.rec_stream = r->stream;
            ARX_HIP(hipEventRecord(pc.ev_recorded, r->stream));
        } else if (pc.rec_stream != r->stream) {
            ARX_HIP(hipStreamWaitEvent(r->stream, pc.ev_recorded, 0));
        }
        // Filtered unless the emitter lies inside the receiver's grown box: every ray would be a
        // candidate at bounce 0, and the frame takes the unfiltered kernel, which costs what it did.
        bool filtered = pc.filter_on && pc.has_state;
        if (filtered) {
            float lo[3], hi[3];
            bool empty = false;
            receiver_bound(r, lo, hi, &empty);
            const float grow = 2.0f * path_filter_grow(a.qgrid);
            bool inside = !empty;
            for (int k = 0; k < 3; ++k) inside = inside && r->emitter[k] >= lo[k] - grow && r->emitter[k] <= hi[k] + grow;
            filtered = !inside && path_filter_list_reserve(r, n_launch);
        }
        if (filtered) {
            FilterArgs fa;
            fa.planes = pc.d_filter;
            fa.list = static_cast<FilterCand*>(f.d_filter_list);
            fa.heads = fa.list + f.filter_list_cap;
            fa.grow = path_filter_grow(a.qgrid);
            ARX_HIP(launch_path_replay_filtered(pa, fa, r->stream));
            pc.last_filtered = true;
            pc.filter_slot = r->slot;
            pc.filter_rays = n_launch;
        } else {
            ARX_HIP(launch_path_replay(pa, r->stream));
        }
        if (r->fif > 1) {
            ARX_HIP(hipEventRecord(pc.ev_replayed[r->slot], r->stream));
            pc.replayed[r->slot] = true;
        }
        pc.state = record ? kPathRecorded : kPathReplayed;
        if (timed && (st = r->trace_ring.end(r->stream)) != ARX_OK) return st;
        return fif_done_traced(r);
    }
    f.dirs_valid = false;  // until the launches below are issued
    ARX_HIP(launch_trace(a, grid_cus, r->stream, r->force_global_stack, fill_dirs));
    f.dirs_stream = r->stream;
    f.dirs_seed = c.seed;
    f.dirs_begin = ray_begin;
    f.dirs_count = n_launch;
    f.dirs_sorted = use_sorted;
    if (measure) {  // inside the launch's timing window: a cost this frame pays
        ARX_HIP(launch_order_pool(f.d_dirs, f.d_dirs_alt, f.d_cost, f.d_order_bins, n_launch, r->stream));
        std::swap(f.d_dirs, f.d_dirs_alt);
        f.order_key = key;
        f.dirs_sorted = true;
    }
    f.dirs_valid = true;
    if (timed && (st = r->trace_ring.end(r->stream)) != ARX_OK) return st;
    return fif_done_traced(r);
}

// ---- a batch of listeners (arx_render_listeners) ----------------------------------------------------
namespace {

constexpr uint64_t kListenerCounterWords = 16;  // a listener's block: kCounters counters, its candidate tally, padding

// arx_debug_listener_bytes' per-listener terms (include/arx.h)
uint64_t listener_bytes_each(uint64_t n, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris) {
    return (uint64_t)recv_nodes * (sizeof(BvhNode) + sizeof(QNode2)) + (uint64_t)recv_tris * sizeof(TriRec) +
           (sizeof(BvhNode) + sizeof(QNode2)) + sizeof(ListenerEntry) + 16ull * (uint64_t)ir_len +
           kListenerCounterWords * 8 + 3 * sizeof(arx_acoustics) + 8ull * (uint64_t)ir_len + path_filter_list_bytes(n) +
           4 * listener_work_words(n);
}

// One chunk's scratch (ListenerBatch::d_scratch): byte offsets, every region 16-B aligned.
struct ListenerScratch {
    uint64_t lists, list_stride, work, work_stride, table, hist, counters, res, ir, edc, acou, total;
};
ListenerScratch listener_scratch(uint64_t n, int32_t ir_len, int32_t chunk) {
    ListenerScratch s;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15) & ~15ull;
        return o;
    };
    const uint64_t J = (uint64_t)chunk;
    s.list_stride = path_filter_list_bytes(n);
    s.lists = take(J * s.list_stride);
    s.work_stride = 4 * listener_work_words(n);
    s.work = take(J * s.work_stride);
    s.table = take(J * sizeof(ListenerEntry));
    s.hist = take(J * 16 * (uint64_t)ir_len);
    s.counters = take(J * kListenerCounterWords * 8);
    s.res = take(J * 3 * sizeof(arx_acoustics));
    s.ir = take(J * 8 * (uint64_t)ir_len);  // the chunk's left IRs, then its right IRs
    s.edc = take(24 * (uint64_t)ir_len);
    s.acou = take(acoustics_scratch_bytes());
    s.total = at;
    return s;
}

// The pinned block of a call of n listeners: table entries by batched order; counter blocks and results by
// batched order in [0, n) and by pose index in [n, 2n) for the poses that went the one-listener route; the
// tree's off-grid flag as the chunks left it.
struct ListenerPinned {
    ListenerEntry* entries;
    unsigned long long* counters;
    arx_acoustics* res;
    unsigned int* flag;
};
size_t listener_pinned_bytes(size_t n) {
    return n * sizeof(ListenerEntry) + 2 * n * kListenerCounterWords * 8 + 2 * n * 3 * sizeof(arx_acoustics) + 16;
}
ListenerPinned listener_pinned(void* base, size_t n) {
    ListenerPinned p;
    char* c = static_cast<char*>(base);
    p.entries = reinterpret_cast<ListenerEntry*>(c);
    c += n * sizeof(ListenerEntry);
    p.counters = reinterpret_cast<unsigned long long*>(c);
    c += 2 * n * kListenerCounterWords * 8;
    p.res = reinterpret_cast<arx_acoustics*>(c);
    c += 2 * n * 3 * sizeof(arx_acoustics);
    p.flag = reinterpret_cast<unsigned int*>(c);
    return p;
}

// The node and triangle arrays widened to hold a chunk's slots: new buffers, what the old ones held copied
// on the device.  False: no room (the error cleared; the arrays as they were).
bool widen_tree_arrays(arx_renderer* r, size_t need_nodes, size_t need_tris) {
    if (need_nodes <= r->nodes_cap && need_tris <= r->tris_cap) return true;
    if (sync_renderer(r) != ARX_OK) return false;
    if (need_nodes > r->nodes_cap) {
        BvhNode* cn = nullptr;
        QNode2* qn = nullptr;
        const size_t cap = need_nodes + 1024;
        if (hipMalloc(&cn, cap * sizeof(BvhNode)) != hipSuccess || hipMalloc(&qn, cap * sizeof(QNode2)) != hipSuccess ||
            hipMemcpy(cn, r->d_cnodes, r->nodes_cap * sizeof(BvhNode), hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(qn, r->d_qnodes, r->nodes_cap * sizeof(QNode2), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(cn);
            hipFree(qn);
            return false;
        }
        hipFree(r->d_cnodes);
        hipFree(r->d_qnodes);
        r->d_cnodes = cn;
        r->d_qnodes = qn;
        r->nodes_cap = cap;
    }
    if (need_tris > r->tris_cap) {
        TriRec* tr = nullptr;
        const size_t cap = need_tris + 4096;
        if (hipMalloc(&tr, cap * sizeof(TriRec)) != hipSuccess ||
            hipMemcpy(tr, r->d_tris, r->tris_cap * sizeof(TriRec), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(tr);
            return false;
        }
        hipFree(r->d_tris);
        r->d_tris = tr;
        r->tris_cap = cap;
    }
    return true;
}

// The chunk scratch for `chunk` listeners of n rays; false: no room (that size is not tried again).
bool listener_scratch_reserve(arx_renderer* r, uint64_t n, int32_t chunk) {
    ListenerBatch& lb = r->listeners;
    if (lb.d_scratch && lb.rays == n && lb.ir_len == r->ir_len && lb.chunk >= chunk) return true;
    const uint64_t need = listener_scratch(n, r->ir_len, chunk).total;
    if (lb.no_room > 0 && need >= lb.no_room) return false;
    if (sync_renderer(r) != ARX_OK) return false;
    hipFree(lb.d_scratch);
    lb.d_scratch = nullptr;
    lb.scratch_bytes = 0;
    lb.chunk = 0;
    if (hipMalloc(&lb.d_scratch, need) != hipSuccess) {
        (void)hipGetLastError();
        lb.d_scratch = nullptr;
        lb.no_room = need;
        return false;
    }
    lb.scratch_bytes = need;
    lb.chunk = chunk;
    lb.rays = n;
    lb.ir_len = r->ir_len;
    return true;
}

// The grid grown once for a batch, as ensure_device_scene's `grow` branch grows it for a walking listener:
// the new grid spans the old one, the scene, the emitter and [ulo, uhi] with half the extent as margin, the
// top node and the scene are re-quantized on the device, and the renderer's own receiver is refit for it
// by the next ensure_device_scene.
arx_status grow_grid_for(arx_renderer* r, const float ulo[3], const float uhi[3]) {
    const BvhBuild& sc = r->scene_img->bvh;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(r->emitter[k], ulo[k]);
        hi[k] = std::max(r->emitter[k], uhi[k]);
        if (sc.root.count >= 0) {
            lo[k] = std::min(lo[k], sc.root.lo[k]);
            hi[k] = std::max(hi[k], sc.root.hi[k]);
        }
        lo[k] = std::min(lo[k], r->qgrid.origin[k]);
        hi[k] = std::max(hi[k], r->qgrid.origin[k] + 65000.0f * r->qgrid.scale[k]);
    }
    ++r->tree_gen;
    r->qgrid = make_qgrid(lo, hi, 0.5);
    ARX_HIP(launch_requant16(r->d_cnodes, 1 + sc.nodes.size(), r->qgrid, r->d_qnodes, r->d_tree_flag, r->tree_gen, r->stream));
    ++r->requants;
    r->recv_pose_dirty = true;
    return ARX_OK;
}

struct ListenerOut {
    float* ir_left;
    float* ir_right;
    arx_acoustics* acoustics;
    arx_listener_result* results;
};

arx_status render_listeners(arx_renderer* r, const arx_listener_pose* poses, size_t n, const ListenerOut& out,
                            const ListenerPinned& pin) {
    ListenerBatch& lb = r->listeners;
    const uint64_t N = n_rays(r->cfg);
    const size_t ir_len = (size_t)r->ir_len;
    const bool analyse = out.acoustics != nullptr;
    std::vector<int32_t> route(n, ARX_LISTENER_SINGLE);
    std::vector<size_t> where(n, 0);  // the listener's block in pin.counters / pin.res
    arx_status st;
    // The one-listener route: the loop's own step, then its outputs queued on the stream.
    auto single = [&](size_t j) -> arx_status {
        const arx_listener_pose& p = poses[j];
        arx_status s1 = arx_set_listener(r, p.x, p.y, p.z, p.yaw_deg);
        if (s1 == ARX_OK) s1 = arx_render(r, nullptr);
        if (s1 == ARX_OK && analyse && !r->cur().acou.queued) s1 = arx_analyze_ir(r);
        if (s1 != ARX_OK) return s1;
        const arx_renderer::FrameSet& f = r->cur();
        where[j] = n + j;
        if (out.ir_left) {
            ARX_HIP(hipMemcpyAsync(out.ir_left + j * ir_len, f.d_ir, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
            ARX_HIP(hipMemcpyAsync(out.ir_right + j * ir_len, f.d_ir + ir_len, ir_len * sizeof(float), hipMemcpyDefault,
                                   r->stream));
        }
        unsigned long long* hc = pin.counters + where[j] * kListenerCounterWords;
        hc[kCounters] = 0;
        ARX_HIP(hipMemcpyAsync(hc, f.d_counters, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
        if (analyse)
            ARX_HIP(hipMemcpyAsync(pin.res + 3 * where[j], f.acou.d_res, 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost,
                                   r->stream));
        route[j] = ARX_LISTENER_SINGLE;
        return ARX_OK;
    };
    // 1. the warm-up: the next pose through arx_render proper until the key is recorded with its filter state
    size_t first = 0;
    ReplayProbe probe;
    for (; first < n; ++first) {
        if ((st = trace_rays(r, 0, N, false, false, &probe)) != ARX_OK) return st;
        const bool can = probe.ready && r->recv_refit && !r->recv.tris.empty() && !r->use_w4 && N > 0 &&
                         r->cfg.max_bounces <= kFilterMaxBounces;
        if (can) break;
        if ((st = single(first)) != ARX_OK) return st;
    }
    // 2. the batched poses: grid, slots and scratch before the first launch; any "no" sends the rest through the loop
    std::vector<size_t> batched;
    bool batch = first < n;
    if (batch) {
        // the union of the remaining poses' receiver bounds on the grid (grown once if need be)
        const float keep[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
        float ulo[3] = {1e30f, 1e30f, 1e30f}, uhi[3] = {-1e30f, -1e30f, -1e30f};
        for (size_t j = first; j < n; ++j) {
            r->center[0] = poses[j].x; r->center[1] = poses[j].y; r->center[2] = poses[j].z;
            float lo[3], hi[3];
            bool empty = false;
            receiver_bound(r, lo, hi, &empty);
            for (int k = 0; k < 3; ++k) {
                ulo[k] = std::min(ulo[k], lo[k]);
                uhi[k] = std::max(uhi[k], hi[k]);
            }
        }
        for (int k = 0; k < 3; ++k) r->center[k] = keep[k];
        if (!qgrid_contains(r->qgrid, ulo, uhi) && (st = grow_grid_for(r, ulo, uhi)) != ARX_OK) return st;
    }
    const int64_t recv_nodes = (int64_t)r->recv.nodes.size(), recv_tris = (int64_t)r->recv.tris.size();
    const int64_t own_nodes = r->scene_img ? 1 + (int64_t)r->scene_img->bvh.nodes.size() + recv_nodes : 0;
    const int64_t own_tris = r->scene_img ? (int64_t)r->scene_img->bvh.tris.size() + recv_tris : 0;
    int32_t chunk = 0;
    if (batch) {
        const uint64_t each = listener_bytes_each(N, r->ir_len, recv_nodes, recv_tris);
        chunk = lb.forced_chunk > 0 ? lb.forced_chunk : (int32_t)std::min<uint64_t>(kListenerChunkMax, kListenerBudget / each);
        chunk = (int32_t)std::min<size_t>((size_t)chunk, n - first);
        batch = chunk >= 1;
    }
    if (batch) {
        // the extended tree must pass the kernels' offset limits and the structural check, slot by slot
        const ListenerLayout last = listener_layout(own_nodes, own_tris, recv_nodes, recv_tris, chunk, chunk - 1, trace_node_cache());
        batch = check_buffer_offsets((size_t)last.total_nodes, (size_t)last.total_tris) == ARX_OK;
        std::vector<BvhNode> moved(r->recv.nodes);
        for (int32_t s = 0; batch && s < chunk; s += std::max(1, chunk - 1)) {  // the first and the last slot
            const ListenerLayout l = listener_layout(own_nodes, own_tris, recv_nodes, recv_tris, chunk, s, trace_node_cache());
            const int32_t ns = (int32_t)(l.node_begin - (own_nodes - recv_nodes)), ts = (int32_t)(l.tri_begin - (own_tris - recv_tris));
            for (size_t i = 0; i < moved.size(); ++i)
                for (int c = 0; c < 2; ++c) {
                    const int32_t cnt = r->recv.nodes[i].d[2 + c];
                    moved[i].d[c] = r->recv.nodes[i].d[c] + (cnt == 0 ? ns : cnt > 0 ? ts : 0);
                }
            const char* why = "";
            batch = validate_bvh_range(moved.data(), (size_t)l.node_begin, moved.size(), (size_t)last.total_nodes,
                                       (size_t)last.total_tris, &why);
        }
        batch = batch && widen_tree_arrays(r, (size_t)last.total_nodes, (size_t)last.total_tris) &&
                listener_scratch_reserve(r, N, chunk);
        chunk = std::min(chunk, std::max(lb.chunk, 0));
    }
    if (batch) {
        // the arrays may have moved and the grid grown: the replay's arguments as they stand now
        if ((st = trace_rays(r, 0, N, false, false, &probe)) != ARX_OK) return st;
        batch = probe.ready && chunk >= 1;
    }
    const ListenerScratch sc = listener_scratch(lb.rays, lb.ir_len, std::max(lb.chunk, 1));
    char* const d_base = static_cast<char*>(lb.d_scratch);
    const float fgrow = batch ? path_filter_grow(probe.args.qgrid) : 0.0f;
    if (batch) {
        // which poses are batched: not those whose box holds the emitter (every ray a candidate), nor one off the grid
        const float keep[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
        for (size_t j = first; j < n; ++j) {
            r->center[0] = poses[j].x; r->center[1] = poses[j].y; r->center[2] = poses[j].z;
            float lo[3], hi[3];
            bool empty = false;
            receiver_bound(r, lo, hi, &empty);
            bool inside = !empty;
            for (int k = 0; k < 3; ++k)
                inside = inside && r->emitter[k] >= lo[k] - 2.0f * fgrow && r->emitter[k] <= hi[k] + 2.0f * fgrow;
            if (inside || !qgrid_contains(r->qgrid, lo, hi)) continue;
            const size_t b = batched.size();
            const int32_t slot = (int32_t)(b % (size_t)chunk);
            const ListenerLayout l = listener_layout(own_nodes, own_tris, recv_nodes, recv_tris, chunk, slot, trace_node_cache());
            ListenerEntry& e = pin.entries[b];
            std::memset(&e, 0, sizeof(e));
            for (int k = 0; k < 3; ++k) e.center[k] = r->center[k];
            e.top = (int32_t)l.top;
            receiver_rotation(poses[j].yaw_deg, e.m);
            e.pad = r->debug_refit_pad > 0.0f ? r->debug_refit_pad : refit_pad(r);
            e.node_shift = (int32_t)(l.node_begin - (own_nodes - recv_nodes));
            e.tri_shift = (int32_t)(l.tri_begin - (own_tris - recv_tris));
            e.hist = reinterpret_cast<unsigned long long*>(d_base + sc.hist) + (size_t)slot * 2 * ir_len;
            e.counters = reinterpret_cast<unsigned long long*>(d_base + sc.counters) + (size_t)slot * kListenerCounterWords;
            e.cand = e.counters + kCounters;
            e.list = reinterpret_cast<FilterCand*>(d_base + sc.lists + (uint64_t)slot * sc.list_stride);
            e.heads = e.list + N;
            e.work = reinterpret_cast<unsigned int*>(d_base + sc.work + (uint64_t)slot * sc.work_stride);
            where[j] = b;
            route[j] = ARX_LISTENER_BATCHED;
            batched.push_back(j);
        }
        for (int k = 0; k < 3; ++k) r->center[k] = keep[k];
        r->yaw = keep[3];
    }
    // 3. the poses that take the one-listener route in place; the call's last pose waits, so that its frame is the last
    for (size_t j = first; j + 1 < n; ++j)
        if (route[j] == ARX_LISTENER_SINGLE && (st = single(j)) != ARX_OK) return st;
    // 4. the chunks, all on the one stream
    const float e0 = initial_energy(r->cfg);
    const double unit = std::ldexp((double)e0, -arx_frac_bits(N));
    for (size_t c0 = 0; c0 < batched.size(); c0 += (size_t)chunk) {
        const int32_t J = (int32_t)std::min<size_t>((size_t)chunk, batched.size() - c0);
        ListenerEntry* d_table = reinterpret_cast<ListenerEntry*>(d_base + sc.table);
        unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(d_base + sc.hist);
        unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_base + sc.counters);
        arx_acoustics* d_res = reinterpret_cast<arx_acoustics*>(d_base + sc.res);
        float* d_irl = reinterpret_cast<float*>(d_base + sc.ir);
        float* d_irr = d_irl + (size_t)lb.chunk * ir_len;
        ARX_HIP(hipMemcpyAsync(d_table, pin.entries + c0, (size_t)J * sizeof(ListenerEntry), hipMemcpyHostToDevice, r->stream));
        ARX_HIP(launch_clear(d_hist, (uint64_t)J * 2 * ir_len, d_cnt, (int)(J * kListenerCounterWords), r->stream));
        RefitArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.local_tris = r->d_recv_local;
        ra.n_tris = (int32_t)recv_tris;
        ra.tri_base = (int32_t)(own_tris - recv_tris);
        ra.local_nodes = r->d_recv_nodes;
        ra.n_nodes = (int32_t)recv_nodes;
        ra.node_base = (int32_t)(own_nodes - recv_nodes);
        ra.level_nodes = r->d_recv_levels;
        ra.level_start = r->d_recv_levels + r->recv_level_count;
        ra.n_levels = r->recv_levels;
        ra.root_ref = r->recv.root.ref;
        ra.root_count = r->recv.root.count;
        ra.grid = r->qgrid;
        ra.tris = r->d_tris;
        ra.cnodes = r->d_cnodes;
        ra.qnodes = r->d_qnodes;
        ra.flag = r->d_tree_flag;
        ra.flag_value = r->tree_gen;
        ARX_HIP(launch_receiver_refit_multi(ra, d_table, J, r->stream));
        FilterArgs fa;
        fa.planes = probe.planes;
        fa.list = nullptr;  // per listener, from the table
        fa.heads = nullptr;
        fa.grow = fgrow;
        ARX_HIP(launch_listeners_replay(probe.args, fa, d_table, J, r->stream));
        for (int32_t i = 0; i < J; ++i) {
            const size_t j = batched[c0 + (size_t)i];
            const long long* h = reinterpret_cast<const long long*>(d_hist + (size_t)i * 2 * ir_len);
            float* il = d_irl + (size_t)i * ir_len;
            float* irr = d_irr + (size_t)i * ir_len;
            ARX_HIP(launch_finalize_ir(h, il, irr, r->ir_len, unit, r->cfg.is_mono, r->stream));
            ++r->ir_generation;
            if (analyse) {
                AcousticsArgs args{};
                args.hist = h;
                args.n = r->ir_len;
                args.sample_rate = r->cfg.sample_rate;
                args.unit = unit;
                args.edc = reinterpret_cast<long long*>(d_base + sc.edc);
                args.out = d_res + 3 * i;
                args.scratch = d_base + sc.acou;
                args.shape = r->scan_shape == 0 ? kScanDefault : r->scan_shape;
                ARX_HIP(launch_acoustics(args, r->stream));
            }
            if (out.ir_left) {
                ARX_HIP(hipMemcpyAsync(out.ir_left + j * ir_len, il, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
                ARX_HIP(hipMemcpyAsync(out.ir_right + j * ir_len, irr, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
            }
        }
        ARX_HIP(hipMemcpyAsync(pin.counters + c0 * kListenerCounterWords, d_cnt, (size_t)J * kListenerCounterWords * 8,
                               hipMemcpyDeviceToHost, r->stream));
        if (analyse)
            ARX_HIP(hipMemcpyAsync(pin.res + 3 * c0, d_res, (size_t)J * 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
        ARX_HIP(hipMemcpyAsync(pin.flag, r->d_tree_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
        pin.flag[1] = r->tree_gen;
        // the call's last pose is the renderer's last frame: histogram, counters, IR, candidate list, analysis
        if (batched.back() == n - 1 && c0 + (size_t)J == batched.size()) {
            const int32_t i = J - 1;
            if ((st = begin_frame(r)) != ARX_OK) return st;
            arx_renderer::FrameSet& f = r->cur();
            ARX_HIP(hipMemcpyAsync(f.d_hist, d_hist + (size_t)i * 2 * ir_len, 2 * ir_len * sizeof(unsigned long long),
                                   hipMemcpyDeviceToDevice, r->stream));
            ARX_HIP(hipMemcpyAsync(f.d_counters, d_cnt + (size_t)i * kListenerCounterWords, kCounters * sizeof(unsigned long long),
                                   hipMemcpyDeviceToDevice, r->stream));
            ARX_HIP(hipMemcpyAsync(f.d_ir, d_irl + (size_t)i * ir_len, ir_len * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
            ARX_HIP(hipMemcpyAsync(f.d_ir + ir_len, d_irr + (size_t)i * ir_len, ir_len * sizeof(float), hipMemcpyDeviceToDevice,
                                   r->stream));
            PathCache& pc = r->path_cache;
            pc.state = kPathReplayed;
            pc.last_key = pc.key;
            pc.last_valid = true;
            pc.last_filtered = false;
            if (path_filter_list_reserve(r, N)) {
                ARX_HIP(hipMemcpyAsync(f.d_filter_list, d_base + sc.lists + (uint64_t)i * sc.list_stride, N * sizeof(FilterCand),
                                       hipMemcpyDeviceToDevice, r->stream));
                ARX_HIP(hipMemcpyAsync(static_cast<FilterCand*>(f.d_filter_list) + f.filter_list_cap,
                                       d_base + sc.lists + (uint64_t)i * sc.list_stride + N * sizeof(FilterCand),
                                       16 * path_filter_heads(N), hipMemcpyDeviceToDevice, r->stream));
                pc.last_filtered = true;
                pc.filter_slot = r->slot;
                pc.filter_rays = N;
            }
            r->conv_ir_dirty = true;
            r->conv_live_ir_dirty = true;
            const arx_listener_pose& p = poses[n - 1];
            r->center[0] = p.x; r->center[1] = p.y; r->center[2] = p.z;
            r->yaw = p.yaw_deg;
            if ((analyse || r->auto_analyze) && (st = arx_analyze_ir(r)) != ARX_OK) return st;
        }
    }
    if (n >= 1 && first < n && route[n - 1] == ARX_LISTENER_SINGLE && (st = single(n - 1)) != ARX_OK) return st;
    // 5. the one synchronisation, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (!batched.empty() && pin.flag[1] != 0 && pin.flag[0] == pin.flag[1])
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    for (size_t j = 0; j < n; ++j) {
        const unsigned long long* hc = pin.counters + where[j] * kListenerCounterWords;
        if (out.results) {
            arx_listener_result& o = out.results[j];
            std::memset(&o, 0, sizeof(o));
            o.queries = hc[0];
            o.receiver_hits = hc[1];
            o.misses = hc[2];
            o.candidate_rays = route[j] == ARX_LISTENER_BATCHED ? hc[kCounters] : 0;
            o.route = route[j];
        }
        if (analyse) std::memcpy(out.acoustics + 3 * j, pin.res + 3 * where[j], 3 * sizeof(arx_acoustics));
    }
    return ARX_OK;
}

}  // namespace

void arx::free_listener_batch(ListenerBatch& b) {
    hipFree(b.d_scratch);
    if (b.h_pinned) hipHostFree(b.h_pinned);
    if (b.ev0) hipEventDestroy(b.ev0);
    if (b.ev1) hipEventDestroy(b.ev1);
    const int32_t forced = b.forced_chunk;
    b = ListenerBatch{};
    b.forced_chunk = forced;
}

extern "C" {

arx_status arx_render_listeners(arx_renderer* r, const arx_listener_pose* poses, size_t n, float* ir_left, float* ir_right,
                                arx_acoustics* acoustics, arx_listener_result* results, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n == 0) return ARX_OK;
    if (!poses) return fail(ARX_ERR_INVALID_ARGUMENT, "poses is NULL");
    if ((ir_left == nullptr) != (ir_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ir_left and ir_right: both or neither");
    for (size_t j = 0; j < n; ++j)
        if (!std::isfinite(poses[j].x) || !std::isfinite(poses[j].y) || !std::isfinite(poses[j].z) ||
            !std::isfinite(poses[j].yaw_deg))
            return fail(ARX_ERR_INVALID_ARGUMENT, "pose %zu is not finite", j);
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs one frame in flight");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own stream");
    if (r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own histogram");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ListenerBatch& lb = r->listeners;
    if (n > lb.h_listeners) {  // nothing of an earlier call is in flight: every call ends synchronised
        if (lb.h_pinned) hipHostFree(lb.h_pinned);
        lb.h_pinned = nullptr;
        lb.h_listeners = 0;
        ARX_HIP(hipHostMalloc(&lb.h_pinned, listener_pinned_bytes(n), hipHostMallocDefault));
        lb.h_listeners = n;
    }
    const ListenerPinned pin = listener_pinned(lb.h_pinned, n);
    pin.flag[0] = pin.flag[1] = 0u;
    const bool timed = r->timing || ms != nullptr;
    if (timed) {
        if (!lb.ev0) ARX_HIP(hipEventCreate(&lb.ev0));
        if (!lb.ev1) ARX_HIP(hipEventCreate(&lb.ev1));
        ARX_HIP(hipEventRecord(lb.ev0, r->stream));
    }
    const float saved[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
    const ListenerOut out{ir_left, ir_right, acoustics, results};
    arx_status st = render_listeners(r, poses, n, out, pin);
    arx_set_listener(r, saved[0], saved[1], saved[2], saved[3]);  // the listener set before the call, refit by the next frame
    if (st != ARX_OK) return st;
    if (timed) {
        ARX_HIP(hipEventRecord(lb.ev1, r->stream));
        ARX_HIP(hipEventSynchronize(lb.ev1));
        float t = 0.0f;
        ARX_HIP(hipEventElapsedTime(&t, lb.ev0, lb.ev1));
        if (ms) *ms = (double)t;
    }
    return ARX_OK;
}

arx_status arx_debug_set_listener_chunk(arx_renderer* r, int32_t listeners) {
    if (!r || listeners < 0 || listeners > kListenerChunkMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "listener chunk: 0 (automatic) or 1..%d", kListenerChunkMax);
    r->listeners.forced_chunk = listeners;
    return ARX_OK;
}

uint64_t arx_debug_listener_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t listeners) {
    if (ir_len < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 0) return 0;
    return (uint64_t)listeners * listener_bytes_each(n_rays, ir_len, recv_nodes, recv_tris);
}

arx_status arx_debug_listener_layout(int64_t n_scene_nodes, int64_t n_scene_tris, int64_t recv_nodes, int64_t recv_tris,
                                     int32_t listeners, int32_t slot, int64_t out5[5]) {
    if (!out5 || n_scene_nodes < 0 || n_scene_tris < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 1 ||
        listeners > kListenerChunkMax || slot < 0 || slot >= listeners)
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad listener layout arguments");
    const ListenerLayout l = listener_layout(1 + n_scene_nodes + recv_nodes, n_scene_tris + recv_tris, recv_nodes, recv_tris,
                                             listeners, slot, trace_node_cache());
    const arx_status fit = check_buffer_offsets((size_t)l.total_nodes, (size_t)l.total_tris);
    if (fit != ARX_OK) return fit;
    out5[0] = l.node_begin;
    out5[1] = l.node_begin + recv_nodes;
    out5[2] = l.tri_begin;
    out5[3] = l.tri_begin + recv_tris;
    out5[4] = l.top;
    return ARX_OK;
}

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

arx_status arx_clear_histogram(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const arx_status st = arx::begin_frame(r);
    if (st != ARX_OK) return st;
    ARX_HIP(launch_clear(r->hist(), 2 * (uint64_t)r->ir_len, r->cur().d_counters, (int)kCounters, r->stream));
    return ARX_OK;
}

arx_status arx_trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end) {
    return r ? arx::trace_rays(r, ray_begin, ray_end, r->timing) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

arx_status arx_finalize_ir(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const float e0 = initial_energy(r->cfg);
    const double unit = std::ldexp((double)e0, -arx_frac_bits(n_rays(r->cfg)));
    ARX_HIP(launch_finalize_ir((const long long*)r->hist(), r->cur().d_ir, r->cur().d_ir + r->ir_len, r->ir_len, unit,
                               r->cfg.is_mono, r->stream));
    r->conv_ir_dirty = true;
    r->conv_live_ir_dirty = true;
    ++r->ir_generation;
    return ARX_OK;
}

arx_status arx_render(arx_renderer* r, double* render_ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
#ifdef ARX_EXP_SEPARATE_CLEAR  // design experiments only: the clear as a launch of its own (round-5 A/B)
    arx_status st = arx_clear_histogram(r);
    if (st != ARX_OK) return st;
    st = arx::trace_rays(r, 0, n_rays(r->cfg), r->timing || render_ms != nullptr, false);
#else
    arx_status st = arx::begin_frame(r);  // the clear rides on the direction pre-pass
    if (st != ARX_OK) return st;
    st = arx::trace_rays(r, 0, n_rays(r->cfg), r->timing || render_ms != nullptr, true);
#endif
    if (st != ARX_OK) return st;
    st = arx_finalize_ir(r);
    if (st != ARX_OK) return st;
    if (r->auto_analyze && (st = arx_analyze_ir(r)) != ARX_OK) return st;
    if (render_ms) return r->trace_ring.last_ms(true, render_ms);
    return ARX_OK;
}

arx_status arx_analyze_ir(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_renderer::Acoustics& a = r->cur().acou;
    if (!a.d_edc) {  // this frame set's first analysis
        hipError_t e;
        if ((e = hipMalloc(&a.d_edc, 3 * (size_t)r->ir_len * sizeof(long long))) != hipSuccess ||
            (e = hipMalloc(&a.d_res, 3 * sizeof(arx_acoustics))) != hipSuccess ||
            (e = hipMalloc(&a.d_scratch, acoustics_scratch_bytes())) != hipSuccess) {
            free_acoustics(a);
            return fail(e == hipErrorOutOfMemory ? ARX_ERR_OUT_OF_MEMORY : ARX_ERR_HIP, "arx_analyze_ir: %s",
                        hipGetErrorString(e));
        }
    }
    if (r->timing)
        if (const arx_status st = r->analysis_ring.begin(r->stream); st != ARX_OK) return st;
    AcousticsArgs args{};
    args.hist = (const long long*)r->hist();
    args.n = r->ir_len;
    args.sample_rate = r->cfg.sample_rate;
    args.unit = std::ldexp((double)initial_energy(r->cfg), -arx_frac_bits(n_rays(r->cfg)));
    args.edc = a.d_edc;
    args.out = a.d_res;
    args.scratch = a.d_scratch;
    args.shape = r->scan_shape == 0 ? kScanDefault : r->scan_shape;
    ARX_HIP(launch_acoustics(args, r->stream));
    if (r->timing)
        if (const arx_status st = r->analysis_ring.end(r->stream); st != ARX_OK) return st;
    a.queued = true;
    return ARX_OK;
}

arx_status arx_set_auto_analyze(arx_renderer* r, int32_t on) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->auto_analyze = on != 0;
    return ARX_OK;
}

arx_status arx_debug_set_scan_shape(arx_renderer* r, int32_t shape) {
    if (!r || shape < 0 || shape > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "scan shape: 0, 1 or 2");
    r->scan_shape = shape;
    return ARX_OK;
}

arx_status arx_get_acoustics(arx_renderer* r, int32_t channel, arx_acoustics* out) {
    if (!r || !out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel < 0 || channel > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "channel %d: 0 left, 1 right, 2 sum", channel);
    if (!r->cur().acou.queued) return fail(ARX_ERR_NOT_READY, "no analysis was queued for the last frame (arx_analyze_ir)");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipMemcpyAsync(out, r->cur().acou.d_res + channel, sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

arx_status arx_edc_device(arx_renderer* r, int64_t** d_edc, size_t* n) {
    if (!r || !d_edc) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *d_edc = (int64_t*)r->cur().acou.d_edc;
    if (n) *n = 3 * (size_t)r->ir_len;
    return ARX_OK;
}

arx_status arx_copy_edc(arx_renderer* r, int32_t channel, int64_t* h_edc, size_t ir_len) {
    if (!r || !h_edc) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel < 0 || channel > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "channel %d: 0 left, 1 right, 2 sum", channel);
    if (ir_len != (size_t)r->ir_len) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu != %d", ir_len, r->ir_len);
    if (!r->cur().acou.queued) return fail(ARX_ERR_NOT_READY, "no analysis was queued for the last frame (arx_analyze_ir)");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipMemcpyAsync(h_edc, r->cur().acou.d_edc + (size_t)channel * ir_len, ir_len * sizeof(int64_t),
                           hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

arx_status arx_debug_trace_counters(arx_renderer* r, uint64_t* out, size_t n) {
    if (!r || !out || n > (size_t)kCounters) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const arx_renderer::FrameSet& f = r->cur();
    ARX_HIP(hipMemcpyAsync(f.h_counters, f.d_counters, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    for (size_t i = 0; i < n; ++i) out[i] = f.h_counters[i];
    return ARX_OK;
}

arx_status arx_debug_node_images(arx_renderer* r, void* cnodes, void* qnodes, size_t n_nodes, float* grid,
                                 uint64_t* requants) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_nodes > (size_t)r->stats.n_nodes) return fail(ARX_ERR_INVALID_ARGUMENT, "only %lld nodes", (long long)r->stats.n_nodes);
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (cnodes && n_nodes) ARX_HIP(hipMemcpy(cnodes, r->d_cnodes, n_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (qnodes && n_nodes) ARX_HIP(hipMemcpy(qnodes, r->d_qnodes, n_nodes * sizeof(QNode2), hipMemcpyDeviceToHost));
    if (grid)
        for (int k = 0; k < 3; ++k) {
            grid[k] = r->qgrid.origin[k];
            grid[3 + k] = r->qgrid.scale[k];
        }
    if (requants) *requants = r->requants;
    return ARX_OK;
}

arx_status arx_debug_trace_profile(arx_renderer* r, uint64_t* out, size_t n_words, size_t* n_out) {
    if (!r || (n_words > 0 && !out)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!r->d_prof) return fail(ARX_ERR_NOT_READY, "not a profiling build (ARX_TRACE_PROF) or no trace yet");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    const size_t k = std::min(n_words, r->prof_words);
    ARX_HIP(hipMemcpy(out, r->d_prof, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n_out) *n_out = k;
    return ARX_OK;
}

arx_status arx_debug_set_refit_pad(arx_renderer* r, float pad) {
    if (!r || !(pad >= 0.0f) || !std::isfinite(pad)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    r->debug_refit_pad = pad;
    r->recv_pose_dirty = true;  // the next trace refits with it
    return ARX_OK;
}

arx_status arx_debug_set_trace_path(arx_renderer* r, int path) {
    if (!r || path < 0 || path > 15 || (path & 4)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    r->force_f32_nodes = (path & 1) != 0;
    r->force_global_stack = (path & 2) != 0;
    const bool w4 = (path & 8) != 0;
    if (w4 && !r->use_w4) {  // the opt-in CW4 copy is made and uploaded at the next trace
        r->scene_dirty = true;
        r->recv_model_dirty = true;
    }
    r->use_w4 = w4;
    return ARX_OK;
}

arx_status arx_debug_set_ray_order(arx_renderer* r, int32_t mode) {
    if (!r || mode < 0 || mode > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "ray order: 0, 1 or 2");
    r->ray_order = mode;
    return ARX_OK;
}

arx_status arx_debug_set_path_cache(arx_renderer* r, int32_t mode, uint64_t max_bytes) {
    if (!r || mode < 0 || mode > 1) return fail(ARX_ERR_INVALID_ARGUMENT, "path cache: mode 0 or 1");
    PathCache& pc = r->path_cache;
    pc.mode = mode;
    pc.max_bytes = max_bytes;
    pc.recorded = pc.last_valid = false;  // the next launch is traced
    pc.no_room = 0;
    pc.state = mode == 1 ? kPathTraced : kPathOff;
    return ARX_OK;
}

arx_status arx_debug_path_cache_state(arx_renderer* r, int32_t* state, uint64_t* bytes, uint64_t* queries_recorded) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const PathCache& pc = r->path_cache;
    if (state) *state = pc.state;
    if (bytes) *bytes = pc.recorded ? pc.bytes : 0;
    if (queries_recorded) {
        *queries_recorded = 0;
        if (pc.recorded) {  // the recording's own query counter (its scratch block)
            ARX_HIP(hipSetDevice(r->cfg.device));
            ARX_HIP(hipMemcpyAsync(pc.h_scratch, pc.d_scratch, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   pc.rec_stream));
            ARX_HIP(hipStreamSynchronize(pc.rec_stream));
            *queries_recorded = pc.h_scratch[0];
        }
    }
    return ARX_OK;
}

arx_status arx_debug_set_path_filter(arx_renderer* r, int32_t on) {
    if (!r || on < 0 || on > 1) return fail(ARX_ERR_INVALID_ARGUMENT, "path filter: 0 or 1");
    PathCache& pc = r->path_cache;
    // switched on over records that came without state: they are forgotten, so the key's next launch
    // records again, once, with it
    if (on && !pc.filter_on && pc.recorded && !pc.has_state) pc.recorded = false;
    if (on && !pc.filter_on) pc.filter_no_room = pc.filter_list_no_room = 0;
    pc.filter_on = on;
    return ARX_OK;
}

arx_status arx_debug_path_filter_state(arx_renderer* r, int32_t* filtered, uint64_t* bytes, uint64_t* candidate_rays,
                                       uint64_t* candidate_queries) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const PathCache& pc = r->path_cache;
    if (filtered) *filtered = pc.last_filtered ? 1 : 0;
    if (bytes) {
        *bytes = pc.filter_cap;
        for (const arx_renderer::FrameSet& f : r->sets)
            if (f.d_filter_list) *bytes += path_filter_list_bytes(f.filter_list_cap);
    }
    if (candidate_rays) *candidate_rays = 0;
    if (candidate_queries) *candidate_queries = 0;
    const arx_renderer::FrameSet& f = r->sets[pc.filter_slot];
    if ((candidate_rays || candidate_queries) && pc.last_filtered && f.d_filter_list) {
        // the heads the launch's filter blocks left behind the list: {candidate rays, candidate queries, ...}
        std::vector<uint32_t> h(4 * path_filter_heads(pc.filter_rays));
        ARX_HIP(hipSetDevice(r->cfg.device));
        ARX_HIP(hipStreamSynchronize(f.stream));
        ARX_HIP(hipMemcpy(h.data(), static_cast<const FilterCand*>(f.d_filter_list) + f.filter_list_cap,
                          h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t rays = 0, queries = 0;
        for (size_t k = 0; k < h.size(); k += 4) {
            rays += h[k];
            queries += h[k + 1];
        }
        if (candidate_rays) *candidate_rays = rays;
        if (candidate_queries) *candidate_queries = queries;
    }
    return ARX_OK;
}

uint64_t arx_debug_path_filter_bytes(uint64_t n_rays, uint32_t max_bounces, uint32_t n_lists) {
    return path_filter_plane_bytes(n_rays, max_bounces) + (uint64_t)n_lists * path_filter_list_bytes(n_rays);
}

uint64_t arx_debug_path_cache_bytes(uint64_t n_rays, uint32_t max_bounces) {
    return kPathRecordBytes * n_rays * (uint64_t)max_bounces;
}

arx_status arx_debug_ray_order_buffer(arx_renderer* r, float* h_out_xyzw, uint64_t count, uint64_t* first_ray,
                                      uint64_t* n_static, int32_t* sorted) {
    if (!r || (count > 0 && !h_out_xyzw)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    const arx_renderer::FrameSet& f = r->cur();
    if (!f.dirs_valid) return fail(ARX_ERR_NOT_READY, "no trace on this frame set yet");
    if (count > f.dirs_count) return fail(ARX_ERR_INVALID_ARGUMENT, "the buffer holds %llu rays", (unsigned long long)f.dirs_count);
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (count > 0) ARX_HIP(hipMemcpy(h_out_xyzw, f.d_dirs, count * 16, hipMemcpyDeviceToHost));
    if (first_ray) *first_ray = f.dirs_begin;
    if (n_static) *n_static = f.dirs_sorted ? pool_static_rays(f.dirs_count, trace_pool_share()) : f.dirs_count;
    if (sorted) *sorted = f.dirs_sorted ? 1 : 0;
    return ARX_OK;
}

arx_status arx_debug_ray_order_host(uint64_t n, uint32_t dyn_share, uint32_t steps, uint64_t* n_static, uint32_t* cost16,
                                    uint32_t* build_share) {
    if (n_static) *n_static = pool_static_rays(n, dyn_share);
    if (cost16) *cost16 = ray_cost16(steps);
    if (build_share) *build_share = trace_pool_share();
    return ARX_OK;
}

arx_status arx_debug_ray_directions(uint64_t seed, uint64_t first, uint64_t count, float* h_out, int device) {
    if (count > 0 && !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL output");
    if (count == 0) return ARX_OK;
    ARX_HIP(hipSetDevice(device));
    float* d = nullptr;
    ARX_HIP(hipMalloc(&d, 3 * count * sizeof(float)));
    hipError_t e = launch_ray_directions(seed, first, count, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_out, d, 3 * count * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail(ARX_ERR_HIP, "ray directions: %s", hipGetErrorString(e));
    return ARX_OK;
}

}  // extern "C"
